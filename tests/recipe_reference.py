"""The whole training recipe in plain torch on the CPU: a helper for tests/test_host_recipe_reference.py and
tests/test_gpu_full_recipe.py, not a test.

One iteration is: pick the batch, apply the feature map, mask every core, forward, cross-entropy, regulariser, backward,
torch.optim.Adam.  Everything runs in the dtype the caller names (float64 for the reference, float32 for the yardstick a
float32 GPU run is judged by).  Nothing here touches a kernel or `dctn_amd.training`; the only things taken from the
package are the Python restatements of the two counter-based generators (`batches.expected_indices`,
`dropout.expected_keep`) and the feature map's two lambdas, and from the oracle the forward and the tensor-network inner
product.

`CASES` holds the two model cases of the GPU tests with every seed and hyper-parameter, so that the host test can check the
input condition on exactly the runs the GPU tests compare against.  The model seeds were picked by that condition
(tests/test_host_recipe_reference.py) out of the first few dozen: about one seed in three meets it for both starts.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import torch
import torch.nn.functional as F
from torch import Tensor

from dctn_amd import batches, dropout
from dctn_amd.window_stats import φ_cos_sin_squared_1 as PHI
from oracle import ref_cpu as R

N_SAMPLES, GLOBAL_BATCH, ITERATIONS = 37, 8, 7   # 4 batches an epoch: 7 iterations cross the boundary and the remainder
P_KEEP = 0.75                                    # exact in bfloat16, float32 and float64


@dataclass(frozen=True)
class Case:
    name: str
    spec: Tuple[Tuple[int, int], ...]
    image_size: int
    reg: str                 # "epswise": coeff * (|W|^2 + sum |core|^2); "composition": coeff * (|W|^2 + <epses, epses>)
    reg_coeff: float
    lr: float = 1e-3
    weight_decay: float = 1e-3
    scale: float = 0.8
    model_seed: int = 11
    data_seed: int = 0
    dropout_seed: int = 0x0123456789ABCDEF
    batch_seed: int = 0x1234567890ABCDEF


CASES: Dict[str, Case] = {
    # one core, the fused layer + head kernels; the regulariser lives in the optimizer (FlatAdam(l2=reg_coeff))
    "cfg2": Case("cfg2", ((3, 4),), 28, "epswise", 1e-2),
    # two cores = two dropout segments, separate EPS and head kernels; the regulariser goes through autograd
    "two_layer": Case("two_layer", ((2, 3), (2, 4)), 10, "composition", 1e-2, model_seed=26),
}


def make_data(case: Case) -> Tuple[Tensor, Tensor]:
    """(N_SAMPLES, size, size) uint8 intensities with both ends of the range present, and labels."""
    g = torch.Generator().manual_seed(case.data_seed)
    size = case.image_size
    images = torch.randint(0, 256, (N_SAMPLES, size, size), dtype=torch.uint8, generator=g)
    images[0, 0, :2] = torch.tensor([0, 255], dtype=torch.uint8)
    return images, torch.randint(0, 10, (N_SAMPLES,), generator=g)


def initial_model(case: Case, dtype: torch.dtype, device=torch.device("cpu"), seed: Optional[int] = None):
    """The model of a case.  Its initialisation draws from the CPU generator only, so the same seed gives the same values
    whatever the device."""
    from dctn_amd.eps_plus_linear import EPSesPlusLinear, UnitTheoreticalOutputStd

    torch.manual_seed(case.model_seed if seed is None else seed)
    return EPSesPlusLinear(case.spec, UnitTheoreticalOutputStd(), P_KEEP, device, dtype, image_size=case.image_size)


def initial_parameters(case: Case, dtype: torch.dtype) -> List[Tensor]:
    """[core 0, ..., linear.weight, linear.bias] in `dtype` as detached CPU tensors: the float32 values of `initial_model`,
    rounded when `dtype` is narrower (a bfloat16 `randn` returns exact zeros now and then, and a dropped zero weight has
    an exactly zero gradient: harmless, but not what the input condition of the tests is stated for)."""
    m = initial_model(case, torch.float32)
    return [p.detach().clone().to(dtype) for p in list(m.epses) + [m.linear.weight, m.linear.bias]]


def make_batch(images: Tensor, labels: Tensor, idx: Sequence[int], dtype: torch.dtype,
               scale: float) -> Tuple[Tensor, Tensor]:
    """`scale * phi(images / 255)` of the given samples as (1, len(idx), H, W, 2), and their labels.  The arithmetic runs in
    `dtype`; a dtype narrower than float32 gets the float32 values rounded (what a loader that casts its float32 data set
    to the model dtype gives)."""
    work = dtype if dtype in (torch.float32, torch.float64) else torch.float32
    idx = torch.as_tensor(list(idx), dtype=torch.int64)
    u = images[idx].to(work) / 255
    x = torch.stack(tuple(f(u) for f in PHI), dim=3).unsqueeze(0) * scale
    return x.to(dtype), labels[idx]


def keep_mask(seed: int, draw: int, segment: int, shape: Sequence[int], p: float, dtype: torch.dtype) -> Tensor:
    """1 / 0 in `dtype`: the keep flags of core number `segment` under draw `draw`."""
    numel = 1
    for s in shape:
        numel *= int(s)
    return torch.tensor(dropout.expected_keep(seed, draw, segment, numel, p), dtype=dtype).view(tuple(shape))


def regulariser(reg: str, cores: Sequence[Tensor], weight: Tensor) -> Tensor:
    if reg == "epswise":
        return (weight ** 2).sum() + sum((c ** 2).sum() for c in cores)
    if reg == "composition":
        return (weight ** 2).sum() + R.epses_inner_product(cores, cores)
    raise ValueError(reg)


def run_recipe(params0: Sequence[Tensor], *, dtype: torch.dtype, n: int, p: float, dropout_seed: int, lr: float,
               weight_decay: float, reg: str, reg_coeff: float, images: Optional[Tensor] = None,
               labels: Optional[Tensor] = None, batch_seed: int = 0, batch_size: int = GLOBAL_BATCH, scale: float = 1.0,
               rank: int = 0, world: int = 1, hand_batches: Optional[Sequence[Tuple[Tensor, Tensor]]] = None,
               master_dtype: Optional[torch.dtype] = None) -> List[Dict]:
    """`n` iterations from `params0` = [cores..., linear.weight, linear.bias].  Iteration k (from 0) trains on batch k of
    (`batch_seed`, `rank` of `world`) - or on `hand_batches[k]` = (x, y) - under draw k of `dropout_seed`.

    `master_dtype` (float32 with `dtype` = bfloat16): the mixed-precision recipe - Adam and the regulariser work on
    `master_dtype` copies, the forward and backward on their rounding to `dtype`.

    Returns one dictionary per iteration: `loss` and `reg_term` (Python floats; the term is unscaled), `indices` (None for
    a hand-given batch), `params` (copies, after the step, in `dtype`), `masters` (copies in `master_dtype`, or None) and
    `adam_grads` (what Adam saw: the gradient of loss + reg_coeff * reg_term plus weight_decay * parameter)."""
    hold = dtype if master_dtype is None else master_dtype
    leaves = [t.detach().clone().to(hold).requires_grad_(True) for t in params0]
    opt = torch.optim.Adam(leaves, lr=lr, weight_decay=weight_decay)
    history = []
    for k in range(n):
        if hand_batches is not None:
            (x, y), idx = hand_batches[k], None
            x = x.to(dtype)
        else:
            idx = batches.expected_indices(batch_seed, k, images.shape[0], batch_size, rank, world)
            x, y = make_batch(images, labels, idx, dtype, scale)
        work = leaves if master_dtype is None else [t.to(dtype) for t in leaves]
        cores, weight, bias = work[:-2], work[-2], work[-1]
        if p < 1.0:   # the model's gate: no mask at p == 1
            cores = [keep_mask(dropout_seed, k, s, c.shape, p, dtype) * c / p for s, c in enumerate(cores)]
        logits = R.eps_plus_linear_forward(cores, weight, bias, x)
        loss = F.cross_entropy(logits if logits.dtype in (torch.float32, torch.float64) else logits.float(), y)
        reg_term = regulariser(reg, leaves[:-2], leaves[-2])
        opt.zero_grad(set_to_none=True)
        (loss + reg_term * reg_coeff).backward()
        adam_grads = [(t.grad + weight_decay * t.detach()).clone() for t in leaves]
        opt.step()
        history.append(dict(loss=float(loss.detach()), reg_term=float(reg_term.detach()), indices=idx,
                            params=[t.detach().to(dtype).clone() for t in leaves],
                            masters=None if master_dtype is None else [t.detach().clone() for t in leaves],
                            adam_grads=adam_grads))
    return history


def run_case(case: Case, dtype: torch.dtype, n: int = ITERATIONS, *, params_dtype: Optional[torch.dtype] = None,
             master_dtype: Optional[torch.dtype] = None) -> List[Dict]:
    """`run_recipe` on a case's own data, seeds and hyper-parameters.  `params_dtype`: the dtype the initial values are
    drawn in (they are then widened exactly to `dtype`); default `dtype`, except float32 for a float64 run, so that the
    float64 reference and the float32 runs start from the same numbers."""
    if params_dtype is None:
        params_dtype = torch.float32 if dtype == torch.float64 else dtype
    images, labels = make_data(case)
    return run_recipe(initial_parameters(case, params_dtype), dtype=dtype, n=n, p=P_KEEP, dropout_seed=case.dropout_seed,
                      lr=case.lr, weight_decay=case.weight_decay, reg=case.reg, reg_coeff=case.reg_coeff, images=images,
                      labels=labels, batch_seed=case.batch_seed, scale=case.scale, master_dtype=master_dtype)


def flat(tensors: Sequence[Tensor]) -> Tensor:
    return torch.cat([t.detach().double().reshape(-1).cpu() for t in tensors])


def rel_err(w: Sequence[Tensor], w_ref: Sequence[Tensor], w0: Sequence[Tensor]) -> float:
    """e = |w - w_ref| / |w_ref - w0| over all parameters (as tests/test_gpu_flat_adam.py's `_rel_err`)."""
    return float((flat(w) - flat(w_ref)).norm() / (flat(w_ref) - flat(w0)).norm())
