"""Component dropout of the EPS cores as one launch each way (dctn_amd/csrc/core_dropout.hip).

The reference builds ``mask * core / p`` with ``mask = p.expand_as(core).bernoulli()`` for every core
(dctn/eps_plus_linear.py:139-143).  Here the mask is a pure function of (seed, draw, core number, element index) - a
counter-based generator, Philox4x32-10 - so nothing core-sized is stored, every rank of a data-parallel run that holds
the same 16-byte state block draws the same mask, and a resumed run reproduces its masks from ``{"seed", "draws_done"}``.
The draw count lives on the device and the forward launch itself advances it: a captured graph draws d, d + 1, ... on its
replays.  include/dctn_amd.h holds the normative definition; `expected_keep` restates it in plain Python.
"""
from __future__ import annotations

import math
from typing import List, Sequence, Tuple

import torch
from torch import Tensor

from . import _lib as L

MAX_CORES = 8   # segments of one launch (include/dctn_amd.h)
_M0, _M1, _W0, _W1, _MASK32 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85, 0xFFFFFFFF


def philox4x32_10(counter: Sequence[int], key: Sequence[int]) -> Tuple[int, int, int, int]:
    """The four output words of Philox4x32-10 for a 4-word counter and a 2-word key."""
    c0, c1, c2, c3 = (int(c) & _MASK32 for c in counter)
    k0, k1 = (int(k) & _MASK32 for k in key)
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & _MASK32, (p0 >> 32) ^ c3 ^ k1, p0 & _MASK32
        k0, k1 = (k0 + _W0) & _MASK32, (k1 + _W1) & _MASK32
    return c0, c1, c2, c3


def keep_threshold(p: float) -> int:
    """T of the mask definition: a component is kept iff its word is below it.  ``p``: the keep probability AS THE TENSOR
    DTYPE STORES IT (``float(model.p)``; the bfloat16 0.9 is 0.8984375)."""
    return min(math.floor(float(p) * 4294967296.0), _MASK32)


def expected_keep(seed: int, draw: int, segment: int, numel: int, p: float) -> List[bool]:
    """Keep flags of the ``numel`` elements of core number ``segment`` of a call, under draw ``draw`` of ``seed``."""
    key = (seed & _MASK32, (seed >> 32) & _MASK32)
    threshold = keep_threshold(p)
    keep: List[bool] = []
    for block in range((numel + 3) // 4):
        keep.extend(word < threshold for word in philox4x32_10((block, 0, draw, segment), key))
    return keep[:numel]


def new_state(seed: int, device: torch.device, draws_done: int = 0) -> Tensor:
    """The 16-byte device block {uint32 seed_lo, seed_hi, draws_done, ticket} as four int32 (same bits)."""
    if not 0 <= int(seed) < 1 << 64:
        raise ValueError(f"the dropout seed is a 64-bit unsigned integer, got {seed}")
    if not 0 <= int(draws_done) < 1 << 32:
        raise ValueError(f"draws_done is a 32-bit unsigned integer, got {draws_done}")
    assert L.lib().dctn_core_dropout_state_bytes() == 16
    words = [int(seed) & _MASK32, int(seed) >> 32, int(draws_done), 0]
    return torch.tensor([w - (1 << 32) if w >= 1 << 31 else w for w in words], dtype=torch.int32).to(device)


def read_state(block: Tensor) -> dict:
    """``{"seed", "draws_done"}`` of a state block or of a draw record (reads the device: it synchronises)."""
    w = [int(v) & _MASK32 for v in block.detach().cpu().tolist()]
    return {"seed": w[0] | (w[1] << 32), "draws_done": w[2]}


def _check(tensors: Sequence[Tensor], p: Tensor) -> torch.device:
    dev = L.require_device(*tensors, p)
    if not 1 <= len(tensors) <= MAX_CORES:
        raise NotImplementedError(f"fused component dropout takes 1 .. {MAX_CORES} cores in one launch, got {len(tensors)}")
    if any(t.dtype != p.dtype for t in tensors):
        raise TypeError(f"fused component dropout: the cores must have the dtype of p ({p.dtype})")
    return dev


class _CoreDropoutFunction(torch.autograd.Function):
    """(p, state, *cores) -> (*masked cores, record).  Saves the 16-byte draw record (and a reference to ``p``); the
    backward regenerates the mask from it.  The op is the only consumer of each masked core's gradient, so the backward
    applies the mask IN PLACE on the tensor it receives and returns a fresh alias of it: the gradients that the fused
    head backward laid back to back stay where they are, and `_FlatOptimizer._grads()` keeps reading them in place
    (a returned tensor that autograd's input buffer still refers to would be copied by AccumulateGrad)."""

    @staticmethod
    def forward(ctx, p: Tensor, state: Tensor, *cores: Tensor):
        dev = _check(cores, p)
        src = [c.contiguous() for c in cores]
        out = [torch.empty_like(c) for c in src]
        record = torch.empty(4, dtype=torch.int32, device=dev)
        L.check(L.lib().dctn_core_dropout_fwd(L.ptr_array(src), L.ptr_array(out), L.i64_array([c.numel() for c in src]),
                                              len(src), p.data_ptr(), state.data_ptr(), record.data_ptr(),
                                              L.dtype_code(p), L.stream_ptr(dev)), "component dropout forward")
        ctx.save_for_backward(record, p)
        ctx.mark_non_differentiable(record)
        ctx.set_materialize_grads(False)   # no zero-fill launch for the record's (absent) gradient
        return (*out, record)

    @staticmethod
    def backward(ctx, *grads):
        record, p = ctx.saved_tensors
        need = ctx.needs_input_grad[2:]
        # a core that needs no gradient (or got none) is skipped by the kernel and keeps its number
        live = [g is not None and need[i] for i, g in enumerate(grads[:-1])]
        if not any(live):
            return (None, None, *([None] * len(need)))
        gs = [(g if g.is_contiguous() else g.contiguous()) if on else None for g, on in zip(grads[:-1], live)]
        ptrs = L.ptr_array(gs)
        L.check(L.lib().dctn_core_dropout_bwd(ptrs, ptrs, L.i64_array([1 if g is None else g.numel() for g in gs]),
                                              len(gs), p.data_ptr(), record.data_ptr(), L.dtype_code(p),
                                              L.stream_ptr(p.device)), "component dropout backward")
        result = [None if g is None else g.view(g.shape) for g in gs]
        return (None, None, *result)


def core_dropout(cores: Sequence[Tensor], p: Tensor, state: Tensor) -> Tuple[Tuple[Tensor, ...], Tensor]:
    """``keep ? core / p : 0`` for every core, in one launch; advances ``state``.  Returns (masked cores, draw record)."""
    *out, record = _CoreDropoutFunction.apply(p, state, *cores)
    return tuple(out), record


def keep_masks(record: Tensor, p: Tensor, shapes: Sequence[Sequence[int]], dtype: torch.dtype) -> Tuple[Tensor, ...]:
    """The keep masks (1 / 0 in ``dtype``) of the draw a forward recorded, for cores of the given shapes in call order."""
    masks = [torch.empty(tuple(s), dtype=dtype, device=record.device) for s in shapes]
    pv = p.to(device=record.device, dtype=dtype)
    dev = _check(masks, pv)
    L.check(L.lib().dctn_core_dropout_mask(L.ptr_array(masks), L.i64_array([m.numel() for m in masks]), len(masks),
                                           pv.data_ptr(), record.data_ptr(), L.dtype_code(pv), L.stream_ptr(dev)),
            "component dropout mask")
    return tuple(masks)
