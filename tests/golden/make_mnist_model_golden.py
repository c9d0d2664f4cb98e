#!/usr/bin/env python3
"""Generate the golden vectors of the ConvSBS classifier by running the REFERENCE's own model (authoring container only).

Usage (needs /root/reference, which never travels to the GPU box):
    python tests/golden/make_mnist_model_golden.py

What runs: ``DCTNMnistModel`` of the reference's mnist.py on the CPU - its constructor, ``scale_layers_using_batch`` and
``forward`` - with torch's cross-entropy and autograd.  mnist.py is a runner: it imports packages that are not installed
here (ignite, libcrap, click_log, torchvision, tensorboard), none of which the model touches.  They are replaced by empty
stand-ins of OUR OWN whose every attribute is a do-nothing object and whose decorators hand the function back unchanged;
the two packages the model's arithmetic goes through, opt_einsum and more_itertools, get `make_golden.py`'s sequencers.

Output: tests/golden/mnist_model_*.npz.  Arrays only: images, labels, cores, logits, losses, gradients and the settings
of the case.  Cores and gradients are numbered in ``state_dict`` order (``names``).
    init_k            the initial cores (float32 values, stored as float64)
    cal64_k / cal32_k the cores after scale_layers_using_batch(images), run in float64 / in the reference's float32
    logits64, loss64, grad64_k   forward, cross-entropy and its gradient from cal64 in float64
    logits32, loss32, grad32_k   the same from cal64 rounded to float32, in float32: the reference's own float32 error
"""
import importlib.abc
import importlib.machinery
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402

REF = MG.REF
STAND_INS = ("ignite", "libcrap", "click_log", "torchvision", "torch.utils.tensorboard", "tensorboard")


class _Anything:
    """Every attribute is another one; called with one function it is a pass-through decorator, otherwise it returns
    another one (which then is)."""

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return _Anything()

    def __call__(self, *args, **kwargs):
        if len(args) == 1 and not kwargs and isinstance(args[0], types.FunctionType):
            return args[0]
        return _Anything()


class _StandInModule(types.ModuleType):
    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return _Anything()


class _StandInFinder(importlib.abc.MetaPathFinder, importlib.abc.Loader):
    def find_spec(self, fullname, path=None, target=None):
        if any(fullname == root or fullname.startswith(root + ".") for root in STAND_INS):
            return importlib.machinery.ModuleSpec(fullname, self, is_package=True)
        return None

    def create_module(self, spec):
        mod = _StandInModule(spec.name)
        mod.__path__ = []
        return mod

    def exec_module(self, module):
        pass


def _reference_mnist():
    assert os.path.isdir(REF), "reference not mounted: this script only runs in the authoring container"
    sys.dont_write_bytecode = True
    MG._install_sequencers()
    sys.meta_path.insert(0, _StandInFinder())
    sys.path.insert(0, REF)
    import mnist

    return mnist


def _run(model, images, labels):
    model.zero_grad()
    logits = model(images)
    loss = torch.nn.functional.cross_entropy(logits, labels)
    loss.backward()
    return logits.detach(), loss.detach(), [p.grad.detach().clone() for p in model.parameters()]


def case(mnist, name, *, layers, bond, trace_edge, batch, size, cos_sin_squared, multiplier, init_std, seed):
    from dctn.conv_sbs import DumbNormalInitialization

    torch.manual_seed(seed)
    build = lambda: mnist.DCTNMnistModel(layers, bond, trace_edge, DumbNormalInitialization(init_std), cos_sin_squared, multiplier)
    m64 = build().double()
    names = list(m64.state_dict())
    init = [v.clone() for v in m64.state_dict().values()]
    images = torch.rand(batch, 1, size, size).double()   # float32 values: both runs see the same images
    labels = torch.randint(0, 10, (batch,))
    m32 = build().float()
    m32.load_state_dict({k: v.float() for k, v in zip(names, init)})
    torch.set_default_dtype(torch.float64)   # the reference's own assertion compares with torch.tensor(1.0)
    m64.scale_layers_using_batch(images)
    torch.set_default_dtype(torch.float32)
    m32.scale_layers_using_batch(images.float())
    cal64 = [v.clone() for v in m64.state_dict().values()]
    cal32 = [v.clone() for v in m32.state_dict().values()]
    logits64, loss64, grad64 = _run(m64, images, labels)
    m32.load_state_dict({k: v.float() for k, v in zip(names, cal64)})
    logits32, loss32, grad32 = _run(m32, images.float(), labels)
    assert [n for n, _ in m64.named_parameters()] == names
    arrays = dict(names=np.array(names), images=images, labels=labels, layers=layers, bond=bond, trace_edge=trace_edge,
                  cos_sin_squared=cos_sin_squared, multiplier=multiplier, logits64=logits64, loss64=loss64,
                  logits32=logits32, loss32=loss32)
    for k in range(len(names)):
        arrays[f"init_{k}"], arrays[f"cal64_{k}"], arrays[f"cal32_{k}"] = init[k], cal64[k], cal32[k]
        arrays[f"grad64_{k}"], arrays[f"grad32_{k}"] = grad64[k], grad32[k]
    MG.npz(name, **arrays)
    print(name, "loss", float(loss64), float(loss32), "max |logit|", float(logits64.abs().max()))


def main():
    # the seeds are ones at which the reference's float32 calibration passes its own assertion (std == 1 within
    # torch.allclose's defaults after every layer) and no layer underflows: with 9-core strings of bond 2 the outputs are
    # heavy-tailed, and at most seeds a float32 layer's std is 0 or misses that assertion on so small a batch
    mnist = _reference_mnist()
    case(mnist, "mnist_model_l3_b2_open", layers=3, bond=2, trace_edge=False, batch=3, size=10, cos_sin_squared=False,
         multiplier=1.0, init_std=0.6, seed=16)
    case(mnist, "mnist_model_l2_b3_ring", layers=2, bond=3, trace_edge=True, batch=2, size=11, cos_sin_squared=True,
         multiplier=1.3, init_std=0.6, seed=7)


if __name__ == "__main__":
    main()
