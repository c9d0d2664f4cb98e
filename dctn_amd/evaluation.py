"""Scoring a model on a data loader (mirror of the reference's dctn/evaluation.py:7-22), with the two
sums reduced over the data-parallel ranks when a process group is up: every rank scores its own
shard and all ranks return the same global numbers."""
from __future__ import annotations

from typing import Any, Callable, Dict, Iterable, Tuple

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


class GraphedScore:
    """A whole scoring pass over ``src`` (a ``batches.DeviceBatches`` built with ``shuffle=False``) replayed from ONE
    captured HIP graph of ONE batch: ``src.draw_padded_into`` -> ``model(x)`` -> `dctn_ce_score_accumulate` into three
    float64 sums on the device, under ``torch.no_grad()`` with the model in eval mode.  A pass is ``src.padded_steps``
    replays: the source's device counter does the walking, every batch has the full shape, and the rows past the last
    sample are padding the score kernel skips (label -100).  The graph's size and capture time do not depend on the data
    set.  Same numbers as `score_fused` fed the same padded batches, bit for bit.
    ``GraphedScore.with_batches_per_launch(model, src, k)`` (k must divide ``src.padded_steps``: ValueError) captures k
    batches back to back, so a pass is ``padded_steps / k`` launches; the batches are added to the three sums in the same
    order, so the sums are those of the per-batch form, bit for bit.

    The constructor runs ``warmup`` eager batches (kernel attributes, the allocator), puts the source's counter back to 0
    with ``load_state_dict`` and captures; it restores ``model.training``, as every pass does.  ``src`` belongs to this
    scorer alone (its counter is what the graph walks on).  The graph reads the LIVE parameters through their storage: it
    holds no copy, so a pass scores the weights as they are when its replays run, and training replays enqueued behind
    ``launch()`` do not change its result (stream order).  It touches neither the training source's counter, nor the
    dropout state block (eval mode draws no mask), nor the optimizer.

    One pass at a time: ``launch()`` assumes the counter at 0 (mod ``padded_steps``) - where the constructor and every
    complete pass leave it - and zeroes the sums, so a second ``launch()`` before ``read()`` wipes what the first pass has
    added so far and the next ``read()`` returns neither pass's score; any other draw from ``src`` shifts the walk
    without notice.  Call ``read()`` after every ``launch()``.

    ``launch()`` zeroes the sums and enqueues the replays; it never synchronises.  ``read()`` reduces the three sums over
    the data-parallel ranks (`ddp.all_reduce_scalar_sums`, as `score_fused`) and returns ``(mean_ce, accuracy)``; the
    integer ``rows`` and ``correct`` of the pass are attributes afterwards.  ``scorer()`` is ``launch()`` then ``read()``.
    """

    def __init__(self, model, src, warmup: int = 1):
        self._build(model, src, warmup, 1)

    @classmethod
    def with_batches_per_launch(cls, model, src, batches_per_launch: int, warmup: int = 1) -> "GraphedScore":
        """A scorer whose graph holds ``batches_per_launch`` batches (the constructor's form holds one)."""
        self = cls.__new__(cls)
        self._build(model, src, warmup, batches_per_launch)
        return self

    def _build(self, model, src, warmup: int, batches_per_launch: int) -> None:
        from . import _lib as L

        if src.shuffle:
            raise ValueError("GraphedScore walks a sequential source: build it with shuffle=False")
        k = int(batches_per_launch)
        if k != batches_per_launch or k < 1 or src.padded_steps % k != 0:
            raise ValueError(f"batches_per_launch must divide the source's padded_steps ({src.padded_steps}), got "
                             f"{batches_per_launch!r}: a pass is a whole number of launches")
        self.batches_per_launch = k
        assert warmup >= 1, "capture needs at least one eager batch first (kernel attributes, lazy initialisation)"
        self.model, self.src, self._L = model, src, L
        self.rows = self.correct = None
        dev = src.device
        self.x, self.y, self.indices = src.empty_batch()
        self.acc = torch.zeros(3, dtype=torch.float64, device=dev)
        was_training = model.training
        model.eval()
        try:
            start = dict(src.state_dict(), batches_done=0)
            side = torch.cuda.Stream(dev)
            side.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(side), torch.no_grad():
                for _ in range(warmup):
                    self._one_batch()
            torch.cuda.current_stream(dev).wait_stream(side)
            torch.cuda.synchronize(dev)
            src.load_state_dict(start)   # outside the capture: a pass starts at 0 (mod padded_steps)
            self.graph = torch.cuda.CUDAGraph()
            with torch.no_grad(), torch.cuda.graph(self.graph, capture_error_mode="thread_local"):
                for _ in range(k):   # back to back on the one capture stream: a single chain
                    self._one_batch()
        finally:
            model.train(was_training)

    def _one_batch(self) -> None:
        L = self._L
        self.src.draw_padded_into(self.x, self.y, self.indices)
        out = self.model(self.x).contiguous()
        dev = L.require_device(out, self.y, self.acc)
        assert out.ndim == 2 and self.y.shape == (out.shape[0],)
        with torch.cuda.device(dev):
            L.check(L.lib().dctn_ce_score_accumulate(out.data_ptr(), self.y.data_ptr(), self.acc.data_ptr(), out.shape[0],
                                                     out.shape[1], L.dtype_code(out), L.stream_ptr(dev)), "fused scoring")

    def launch(self) -> None:
        """Enqueues one pass on the current stream; does not wait for it."""
        self.acc.zero_()
        for _ in range(self.src.padded_steps // self.batches_per_launch):
            self.graph.replay()

    def read(self) -> Tuple[float, float]:
        """``(mean_ce, accuracy)`` of the pass last launched (reads the device: it synchronises)."""
        sum_loss, num_correct, num_samples = ddp.all_reduce_scalar_sums(self.acc[0], self.acc[1], self.acc[2])
        self.rows, self.correct = int(round(float(num_samples))), int(round(float(num_correct)))
        return float(sum_loss / num_samples), float(num_correct / num_samples)

    def __call__(self) -> Tuple[float, float]:
        self.launch()
        return self.read()


def make_evaluation_hook(train_scorer, val_scorer, ema=None) -> Callable[[Dict[str, Any], Dict[str, Any]], None]:
    """``f(st_x, st_it)`` that fills ``train_mean_ce``, ``train_acc``, ``val_mean_ce`` and ``val_acc`` - what
    `training._checkpoint_tag`, the checkpointers and the early stopper read - from two scorers with ``launch()`` /
    ``read()`` (`GraphedScore`); for ``at_iter_start=[every_n_iters_intervals(...)(hook), ...]`` of `training.train`.  Both
    passes are enqueued before either is read.  ``ema`` (a `training.WeightEMA`): once both were read, the validation
    scorer runs a second pass under ``ema.applied()`` - its graph reads the live parameter storage, which then holds the
    averaged weights - and fills ``ema_val_mean_ce`` and ``ema_val_acc``."""

    def hook(st_x, st_it) -> None:
        train_scorer.launch()
        val_scorer.launch()
        st_it["train_mean_ce"], st_it["train_acc"] = train_scorer.read()
        st_it["val_mean_ce"], st_it["val_acc"] = val_scorer.read()
        if ema is not None:
            with ema.applied():
                val_scorer.launch()
                st_it["ema_val_mean_ce"], st_it["ema_val_acc"] = val_scorer.read()

    return hook
