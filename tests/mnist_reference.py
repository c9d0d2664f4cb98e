"""The ConvSBS classifier restated in plain torch on the CPU, on `oracle.ref_cpu.convsbs_forward`: the reference of the
GPU tests of `dctn_amd.mnist_model` in whatever dtype it is run in (float64: the reference; float32: the yardstick of the
project's 4x rule).  Differentiable: autograd goes through the oracle's einsums."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import ref_cpu as R


def layout(model):
    """[[(positions, number of cores), ...] per layer]: what `forward` needs beside the flat list of cores."""
    return [[([(p.h, p.w) for p in s.spec.positions], len(s.cores)) for s in layer.strings] for layer in model.conv_sbses]


def forward(cores, lay, quantum):
    """cores: flat list in state_dict order; quantum: (1, B, H, W, 2).  Returns (logits, [every string's output])."""
    channels, k, outputs = list(quantum.unbind(0)), 0, []
    for strings in lay:
        outs = []
        for positions, n in strings:
            outs.append(R.convsbs_forward(cores[k : k + n], positions, channels))
            k += n
        outputs.extend(outs)
        channels = outs
    (result,) = channels
    return result.mean(dim=(1, 2)), outputs


def loss_and_grads(cores, lay, quantum, labels):
    leaves = [c.detach().clone().requires_grad_(True) for c in cores]
    logits, _ = forward(leaves, lay, quantum)
    loss = F.cross_entropy(logits, labels)
    loss.backward()
    return logits.detach(), loss.detach(), [c.grad for c in leaves]


def ulp32(x):
    """One float32 ulp at the magnitude of x."""
    return float(np.spacing(np.float32(abs(float(x)))))


def four_times_rule(label, got, ref32, ref64, normwise=False, check=True):
    """The project's float32 rule (tests/test_gpu_full_recipe.py:148-161): the error of `got` against the float64 values is at
    most 4 x the error of the reference's own float32 values, with a floor of one float32 ulp of the largest reference
    magnitude.  Max-abs error, or the 2-norm of the difference (`normwise`).  Prints the figures, then asserts - or, with
    ``check=False``, returns whether the rule holds, for a caller that prints every figure before it asserts."""
    got, ref32, ref64 = (torch.as_tensor(np.asarray(t) if not isinstance(t, torch.Tensor) else t).detach().cpu().double()
                         for t in (got, ref32, ref64))
    err = (lambda a: float((a - ref64).norm())) if normwise else (lambda a: float((a - ref64).abs().max()))
    e_got, e_ref, floor = err(got), err(ref32), ulp32(ref64.abs().max())
    print(f"\n{label}: error {e_got:.4e}, the reference's float32 error {e_ref:.4e}, bound {max(4 * e_ref, floor):.4e} "
          f"(ulp {floor:.2e})")
    if check:
        assert e_got <= max(4 * e_ref, floor), label
    return e_got <= max(4 * e_ref, floor)


# ------------------------------------------------------------------ the training recipe, restated
def calibrate(cores, lay, quantum):
    """`scale_layers_using_batch` (the reference's mnist.py:265-284) on a flat list of cores, in their dtype: every string is
    divided by the unbiased std of its output, spread over its cores, layer by layer.  Returns the new cores."""
    cores = [c.detach().clone() for c in cores]
    channels, k = list(quantum.unbind(0)), 0
    with torch.no_grad():
        for strings in lay:
            spans = []
            for positions, n in strings:
                std = R.convsbs_forward(cores[k : k + n], positions, channels).std().item()
                assert std > 0.0 and np.isfinite(std), "the restated calibration expects strings it can scale"
                for c in cores[k : k + n]:
                    c *= (std ** -1) ** (1 / n)
                spans.append((positions, k, n))
                k += n
            channels = [R.convsbs_forward(cores[a : a + n], positions, channels) for positions, a, n in spans]
    return cores


def train(cores, lay, batches, rates, steps_per_epoch, alpha, momentum, weight_decay, eps=1e-8):
    """``torch.optim.RMSprop`` over the restated model with the per-epoch rate: ``batches`` is a list of (quantum, labels)
    in the cores' dtype.  Returns (losses, final cores)."""
    leaves = [c.detach().clone().requires_grad_(True) for c in cores]
    opt = torch.optim.RMSprop(leaves, lr=rates[0], alpha=alpha, eps=eps, weight_decay=weight_decay, momentum=momentum)
    losses = []
    for k, (quantum, labels) in enumerate(batches):
        for group in opt.param_groups:
            group["lr"] = rates[min(k // steps_per_epoch, len(rates) - 1)]
        opt.zero_grad()
        logits, _ = forward(leaves, lay, quantum)
        loss = F.cross_entropy(logits, labels)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    return losses, [c.detach() for c in leaves]
