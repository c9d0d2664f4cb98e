"""Scoring a model on a data loader (mirror of the reference's dctn/evaluation.py:7-22), with the two
sums reduced over the data-parallel ranks when a process group is up: every rank scores its own
shard and all ranks return the same global numbers."""
from __future__ import annotations

from typing import Iterable, Tuple

import torch
import torch.nn.functional as F

from . import ddp


def score(model, dl: Iterable, device) -> Tuple[float, float]:
    """Mean cross-entropy and accuracy over all batches of ``dl`` (items ``(x, y, indices)`` with ``x``
    in the (channels, batch, height, width, features) layout).  ``model(x)`` returns unnormalised
    log-probabilities (batch, classes)."""
    num_samples = torch.zeros((), dtype=torch.float64, device=device)
    num_correct = torch.zeros((), dtype=torch.float64, device=device)
    sum_loss = torch.zeros((), dtype=torch.float64, device=device)
    with torch.no_grad():
        for x, y, _ in iter(dl):
            y = y.to(device)
            out = model(x.to(device)).float()
            num_samples += len(y)
            sum_loss += F.cross_entropy(out, y, reduction="sum").double()
            num_correct += (out.argmax(dim=1) == y).sum().double()
    sum_loss, num_correct, num_samples = ddp.all_reduce_scalar_sums(sum_loss, num_correct, num_samples)
    return float(sum_loss / num_samples), float(num_correct / num_samples)


def score_fused(model, dl: Iterable, device) -> Tuple[float, float]:
    """``score`` with everything after ``model(x)`` as ONE kernel launch per batch (`dctn_ce_score_accumulate`: the
    batch's sum of cross-entropies, number of correct rows and number of rows added to three float64 values on the
    device) and no device-to-host read until the loop ends.  Same contract and return value; the logits are read in
    the dtype the model returns them in (float32 or bfloat16; the row arithmetic is float32 either way).  GPU only:
    there is no CPU implementation of the kernel."""
    from . import _lib as L

    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError(f"dctn_amd: score_fused runs on an MI355X device only, got '{device}' (use `score` there)")
    acc = torch.zeros(3, dtype=torch.float64, device=device)
    with torch.no_grad():
        for x, y, _ in iter(dl):
            y = y.to(device).contiguous().long()
            out = model(x.to(device)).contiguous()
            dev = L.require_device(out, y, acc)
            assert out.ndim == 2 and y.shape == (out.shape[0],)
            with torch.cuda.device(dev):
                L.check(L.lib().dctn_ce_score_accumulate(out.data_ptr(), y.data_ptr(), acc.data_ptr(), out.shape[0],
                                                         out.shape[1], L.dtype_code(out), L.stream_ptr(dev)),
                        "fused scoring")
    sum_loss, num_correct, num_samples = ddp.all_reduce_scalar_sums(acc[0], acc[1], acc[2])
    return float(sum_loss / num_samples), float(num_correct / num_samples)
