"""One training iteration, data-parallel.

The reference's loop (dctn/training.py:62-84) is: forward, ``loss_fn(output, y)``, a regulariser
term scaled by ``reg_coeff``, ``optimizer.zero_grad()``, backward of the sum, ``optimizer.step()``,
with callback hooks around it.  Here the same sequence is one function; between backward and the
optimizer step the parameter gradients are averaged over the ranks (``ddp.FlatGradAllReducer``: in
place on the fused backward's flat gradient buffer when the model provides one).

``train`` and the callbacks below it mirror the reference's loop and hook objects
(dctn/training.py:23-248: same names, arguments, ``st_x`` / ``st_it`` dictionaries and checkpoint file
names) for SURVEY 8(f) row f4, made safe for one process per GPU: gradients are averaged over the ranks
before the ``after_back`` hooks, a stop requested on any rank stops all of them in the same iteration,
and only rank 0 touches checkpoint files.
"""
from __future__ import annotations

import contextlib
import ctypes
import math
import os
from collections import deque
from logging import getLogger
from typing import Any, Callable, Dict, Iterable, Iterator, Optional, Sequence, Tuple

import torch
import torch.distributed as dist
from torch import Tensor

from . import ddp

StX = Dict[Any, Any]   # state that lives across iterations
StIt = Dict[Any, Any]  # state of one iteration


def train_step(
    model: torch.nn.Module,
    x: Tensor,
    y: Tensor,
    loss_fn: Callable[[Tensor, Tensor], Tensor],
    optimizer: torch.optim.Optimizer,
    reg_fn: Optional[Callable[[torch.nn.Module], Tensor]] = None,
    reg_coeff: float = 0.0,
    reducer: Optional[ddp.FlatGradAllReducer] = None,
    monitor=None,
    indices: Optional[Tensor] = None,
) -> Dict[str, Tensor]:
    """``x``: this rank's shard (channels, batch, height, width, features); ``y``: its labels.
    Returns the detached ``output``, ``loss`` and ``reg_term`` of this rank.  ``monitor`` (a `batch_monitor.BatchMonitor`):
    the iteration ends with its record of ``x``, the output, ``y`` and ``indices`` (the batch's sample numbers, or None) -
    this rank's shard in a data-parallel run."""
    _refuse_image_batch(monitor, x)
    model.train()
    output = model(x)
    loss = loss_fn(output if getattr(loss_fn, "accepts_low_precision", False) else output.float(), y)
    optimizer.zero_grad(set_to_none=True)
    if reg_fn is not None:
        reg_term = reg_fn(model)
        (loss + reg_term.float() * reg_coeff).backward()
    else:   # no fill / multiply / add launches for a term that is not there
        reg_term = output.new_zeros((), dtype=torch.float32)
        loss.backward()
    if reducer is not None:
        reducer()
    optimizer.step()
    if monitor is not None:
        monitor.record(x, output.detach(), y, indices)
    return {"output": output.detach(), "loss": loss.detach(), "reg_term": reg_term.detach()}


def _refuse_image_batch(monitor, x: Tensor) -> None:
    """A batch monitor reads the quantum form of the batch; the image form of `DCTNMnistModel.forward` is refused before
    anything runs."""
    if monitor is not None and x.ndim == 4:
        raise ValueError(f"the batch monitor reads the QUANTUM form of the batch, (C, B, H, W, Q) as a DeviceBatches draws "
                         f"it; the step was given a {tuple(x.shape)} image batch")


class GraphedTrainStep:
    """The same iteration replayed from captured HIP graphs (the step of the small models is launch
    bound: ~40 kernels of a few microseconds each once loss, regulariser and optimizer are counted).

    Single process: one graph holds forward, loss, regulariser, backward and the optimizer step.
    Data parallel over RCCL (``graph_allreduce=None``, the default): the collective is captured into the one graph
    as well (one launch per iteration from the host) when a child-process probe (`ddp.probe_allreduce_capture`,
    every rank at the same point) shows that such a capture works on this machine - a capture that fails cannot be
    recovered from inside a process (later collectives fail), so it is tried where a failure is free; when the
    probe fails, or with another backend, or with ``graph_allreduce=False``: forward + backward are one graph,
    the gradient all-reduce runs eagerly on the same stream, the optimizer step is a second graph.
    ``graph_allreduce=True`` skips the probe and insists.
    Inputs are copied into static buffers, so
    every call must use the batch shape of the example; the optimizer must be capturable
    (``FlatSGD`` / ``FlatAdam`` below, ``torch.optim.SGD``, or ``torch.optim.Adam(..., capturable=True)``).

    The dictionary a call returns holds the graph's STATIC output buffers (no copy kernels in the iteration): the
    next call overwrites them.  A caller that keeps ``loss`` / ``output`` across iterations must ``.clone()`` them
    (``train_step`` returns fresh tensors).

    ``batch_source`` (a ``batches.DeviceBatches``): the graph then holds the ENTIRE iteration - its first node draws the
    batch into the static buffers (``batch_source.draw_into``), every replay trains on the next batch of the source, and
    the step is called with no arguments.  ``example_x`` / ``example_y`` may be None (the buffers take the source's
    shapes), and the returned dictionary gains ``"indices"``, the sample numbers of the batch (a static buffer like the
    others).  The warm-up iterations consume real draws and are real training steps, as they already are on the example
    batch: after construction the source stands at batch ``warmup``.

    A gradient guard needs no argument here: the step captures whatever ``optimizer.step()`` launches, so with
    ``FlatAdam(..., guard=GradGuard(dev, max_norm))`` the check and the guarded step kernel are two nodes of the one
    graph, or of the optimizer's graph ``g_opt`` in the split form, where the check then sees the all-reduced
    gradients.  The host still reads nothing between replays.  Once the guard has halted, replays go on running
    forward and backward but the optimizer writes nothing; with a ``batch_source`` the source and the dropout
    counter go on advancing meanwhile.  The guard counts its checks from the first warm-up iteration, as the source
    counts its draws, so (both fresh at construction) ``batch_source.expected_indices(guard.read()["bad_step"])`` names
    the batch that set the latch.  ``guard.max_norm`` may be assigned and ``guard.reset()`` called between replays.

    ``trace`` (a `StepTrace`): every iteration - the warm-up ones too, as they advance every other counter - ends with
    ``trace.record(...)`` behind ``optimizer.step()`` (in the split data-parallel form at the end of the optimizer's
    graph ``g_opt``): one 64-byte record per iteration in a ring on the device, holding the loss, the rows of the batch and
    how many were classified correctly, the guard's norm / coefficient / latch, Adam's step count and rate and the
    source's counter.  ``trace.read()`` fetches the records whenever the host likes.  In a data-parallel run every rank
    records its own shard's loss and counts.

    ``iters_per_launch=K`` > 1: the one graph holds K whole iterations back to back (draw, forward, loss, backward, the
    in-graph all-reduce if there is one, optimizer step, trace record) as a single chain of nodes, and one call runs K
    iterations for one graph launch from the host.  It needs a ``batch_source`` (ValueError) and, with a reducer, the
    all-reduce inside the graph (ValueError naming ``graph_allreduce``: the split form cannot work).  The call returns
    the LAST iteration's static buffers and ``"iters"`` = K (a step of one iteration per launch returns the keys it always
    returned; ``step.iters_per_launch`` holds K either way); what the inner iterations saw is in the trace.  The graph's
    memory pool does not grow K-fold: the allocator gives the blocks an iteration has freed to the next one.  The
    host's settings - ``optimizer.lr = ...``, ``guard.max_norm = ...``, ``guard.reset()`` - are device writes in stream
    order BETWEEN launches: they take effect at a launch boundary, for all K iterations of the next launch.  Once the
    guard halts inside a launch, the rest of that launch runs forward and backward and applies nothing, as replays do.
    With the defaults (K = 1, no trace) the captured graph is exactly what it was without these arguments.

    ``monitor`` (a `batch_monitor.BatchMonitor`): every iteration - the warm-up ones too - ends with ``monitor.record(...)``
    beside the trace record: ONE more launch that, every ``period``-th time, writes the input statistics of the static
    batch buffer, the logits' min / max / mean / std, the histogram of their softmax and every sample's probability of
    its true class, prediction, label and (with a ``batch_source``) sample number into a ring of rows on the device.  With
    ``iters_per_launch=K`` every recorded inner iteration keeps its row.  The monitor reads the (C, B, H, W, Q) batch a
    `DeviceBatches` draws: a 4-d image batch is refused (ValueError).  In a data-parallel run each rank records its own
    shard.  Without ``monitor`` the graph holds no node for it.
    """

    def __init__(self, model: torch.nn.Module, example_x: Optional[Tensor], example_y: Optional[Tensor],
                 loss_fn: Callable[[Tensor, Tensor], Tensor], optimizer: torch.optim.Optimizer,
                 reg_fn: Optional[Callable[[torch.nn.Module], Tensor]] = None, reg_coeff: float = 0.0,
                 reducer: Optional[ddp.FlatGradAllReducer] = None, warmup: int = 3,
                 graph_allreduce: Optional[bool] = None, *, iters_per_launch: int = 1, trace=None, monitor=None,
                 batch_source=None):
        self.model, self.optimizer, self.reducer = model, optimizer, reducer
        self.batch_source = batch_source
        self._ema = getattr(optimizer, "ema", None)   # a WeightEMA: no replay while it is applied
        K = int(iters_per_launch)
        if K != iters_per_launch or K < 1:
            raise ValueError(f"iters_per_launch must be an integer >= 1, got {iters_per_launch!r}")
        self.iters_per_launch, self.trace = K, trace
        if K > 1:
            if batch_source is None:
                raise ValueError("iters_per_launch > 1 needs a batch_source: the inner iterations of a launch draw their "
                                 "own batches, the host cannot hand them in")
            if reducer is not None and (reducer.world > 1 or not reducer.skip_single_rank) and graph_allreduce is False:
                raise ValueError("iters_per_launch > 1 needs the gradient all-reduce inside the graph: graph_allreduce=False "
                                 "(forward + backward graph, eager all-reduce, optimizer graph) cannot run K iterations in "
                                 "one launch")
        if batch_source is None:
            self.x, self.y = example_x.clone(), example_y.clone()
        else:
            self.x, self.y, self.indices = batch_source.empty_batch()
        self.monitor = monitor
        _refuse_image_batch(monitor, self.x)
        dev = self.x.device
        reduces = reducer is not None and (reducer.world > 1 or not reducer.skip_single_rank)
        if reduces and graph_allreduce is None:
            graph_allreduce = False
            if dist.is_initialized() and dist.get_backend() == "nccl":
                some = next(p for p in model.parameters() if p.requires_grad)
                ok = ddp.probe_allreduce_capture(numel=sum(p.numel() for p in model.parameters() if p.requires_grad),
                                                 dtype=some.dtype, local_rank=dev.index)
                graph_allreduce = ddp.all_ranks_agree(ok, dev)
        graph_allreduce = bool(graph_allreduce) and reduces
        if K > 1 and reduces and not graph_allreduce:
            raise ValueError("iters_per_launch > 1 needs the gradient all-reduce inside the graph, and the capture probe "
                             "said no on this machine (graph_allreduce): use iters_per_launch=1, or a reducer whose "
                             "all-reduce is a plain kernel launch (algorithm='direct') with graph_allreduce=True")
        split = reduces

        def fwd_bwd():
            if batch_source is not None:
                batch_source.draw_into(self.x, self.y, self.indices)
            model.train()
            out = model(self.x)
            loss = loss_fn(out if getattr(loss_fn, "accepts_low_precision", False) else out.float(), self.y)
            optimizer.zero_grad(set_to_none=True)
            if reg_fn is not None:
                reg = reg_fn(model)
                total = loss + reg.float() * reg_coeff
            else:   # no fill / multiply / add nodes in the graph for a term that is not there
                reg, total = no_reg, loss
            # a ready-made "1" (created during the eager warm-up, never inside the capture): autograd's own root
            # gradient would be a fill node
            total.backward(unit_seed(dev, total.dtype))
            return out, loss, reg

        def record(out, loss, reg):   # the iteration's last launches; nothing at all without a trace or a monitor
            if trace is not None:
                trace.record(out, self.y, loss, reg=None if reg is no_reg else reg,
                             guard=getattr(optimizer, "guard", None), optimizer=optimizer, batch_source=batch_source)
            if monitor is not None:
                monitor.record(self.x, out.detach(), self.y, self.indices if batch_source is not None else None)

        def iterations():   # K whole iterations back to back on the one capture stream: a single chain, no forks
            last = None
            for _ in range(K):
                del last   # the iteration before is over: its buffers go back to the graph's pool before the next one asks
                last = fwd_bwd()
                if reduces:
                    reducer()
                optimizer.step()
                record(*last)
            return last

        no_reg = torch.zeros((), dtype=torch.float32, device=dev)
        assert warmup >= 1, "capture needs at least one eager iteration first (lazy optimizer state, kernel attributes)"
        side = torch.cuda.Stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            for _ in range(warmup):
                last = fwd_bwd()
                if split:
                    reducer()
                optimizer.step()
                record(*last)
                del last   # nothing of a warm-up iteration (its autograd graph) is alive when the capture begins
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
        self.g_opt = None
        self.allreduce_in_graph = False
        if reduces and graph_allreduce:
            try:   # the whole iteration, collective included, as one graph
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, capture_error_mode="thread_local"):
                    self.out, self.loss, self.reg = iterations()
                self.g_main, self.allreduce_in_graph, split = g, True, False
                return
            except Exception as e:
                # no fallback: after a failed capture later collectives of this process fail ("invalid argument")
                raise RuntimeError("capturing the all-reduce into the iteration's graph failed; rerun with "
                                   "graph_allreduce=False") from e
        self.g_main = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.g_main, capture_error_mode="thread_local"):
            if split:   # (K == 1: checked above)
                self.out, self.loss, self.reg = fwd_bwd()
            else:
                self.out, self.loss, self.reg = iterations()
        if split:
            self.g_opt = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.g_opt, capture_error_mode="thread_local"):
                optimizer.step()
                record(self.out, self.loss, self.reg)

    def __call__(self, x: Optional[Tensor] = None, y: Optional[Tensor] = None) -> Dict[str, Tensor]:
        if self._ema is not None:
            self._ema._refuse_applied("a GraphedTrainStep launch")
        if self.batch_source is not None:
            if x is not None or y is not None:
                raise TypeError("a GraphedTrainStep with a batch_source draws its own batches: call it without arguments")
        else:
            if x is None or y is None:
                raise TypeError("GraphedTrainStep.__call__ needs the batch (x, y)")
            if x is not self.x:   # a data pipeline may fill the static buffers `step.x` / `step.y` itself and pass them
                self.x.copy_(x, non_blocking=True)
            if y is not self.y:
                self.y.copy_(y, non_blocking=True)
        self.g_main.replay()
        if self.g_opt is not None:
            self.reducer()
            self.g_opt.replay()
        result = {"output": self.out, "loss": self.loss, "reg_term": self.reg}
        if self.batch_source is not None:
            result["indices"] = self.indices
        if self.iters_per_launch > 1:   # (one iteration per launch returns the keys it always returned)
            result["iters"] = self.iters_per_launch
        return result


# ------------------------------------------------------------------------------- fused iteration tail
from . import _lib as L  # noqa: E402


# Constant "1" tensors used as the gradient seed of a scalar loss (GraphedTrainStep), one per (device, dtype), kept alive
# for the life of the process so that their addresses are never reused: a backward that receives one of them knows
# its incoming gradient is exactly 1 without reading it.
_UNIT_SEED_TENSORS: Dict = {}
_UNIT_SEEDS = set()


def unit_seed(device: torch.device, dtype: torch.dtype) -> Tensor:
    key = (str(device), dtype)
    seed = _UNIT_SEED_TENSORS.get(key)
    if seed is None:
        seed = _UNIT_SEED_TENSORS[key] = torch.ones((), dtype=dtype, device=device)
        _UNIT_SEEDS.add(seed.data_ptr())
    return seed


class _FusedCrossEntropy(torch.autograd.Function):
    """``F.cross_entropy(logits, labels)`` (mean reduction) as HIP kernels instead of cast + log-softmax + nll and
    their three backward launches.  When the logits need a gradient the forward kernel also leaves
    ``(softmax - onehot) / B`` (`dctn_ce_loss_fwd_grad`); the backward returns it as is when the incoming gradient is
    a registered constant 1 (the seed GraphedTrainStep passes), otherwise `dctn_ce_loss_bwd` scales by the incoming
    scalar."""

    @staticmethod
    def forward(ctx, logits: Tensor, labels: Tensor) -> Tensor:
        dev = L.require_device(logits, labels)
        lg, lb = logits.contiguous(), labels.contiguous().long()
        assert lg.ndim == 2 and lb.shape == (lg.shape[0],)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        if ctx.needs_input_grad[0]:
            unit = torch.empty_like(lg)
            L.check(L.lib().dctn_ce_loss_fwd_grad(lg.data_ptr(), lb.data_ptr(), loss.data_ptr(), unit.data_ptr(),
                                                  lg.shape[0], lg.shape[1], L.dtype_code(lg), L.stream_ptr(dev)),
                    "cross-entropy forward")
            ctx.save_for_backward(lg, lb, unit)
        else:
            L.check(L.lib().dctn_ce_loss_fwd(lg.data_ptr(), lb.data_ptr(), loss.data_ptr(), lg.shape[0], lg.shape[1],
                                             L.dtype_code(lg), L.stream_ptr(dev)), "cross-entropy forward")
        return loss

    @staticmethod
    def backward(ctx, d_loss: Tensor):
        lg, lb, unit = ctx.saved_tensors
        if d_loss.data_ptr() in _UNIT_SEEDS:
            # inside a capture the saved tensor itself is handed on (one node less; the graph owns it).  Eagerly it is
            # cloned: AccumulateGrad may steal a returned gradient and accumulate into it in place, which would
            # corrupt the saved tensor for a second backward(retain_graph=True)
            return (unit if torch.cuda.is_current_stream_capturing() else unit.clone()), None
        dev = lg.device
        g = d_loss.to(torch.float32).contiguous()
        d_logits = torch.empty_like(lg)
        L.check(L.lib().dctn_ce_loss_bwd(lg.data_ptr(), lb.data_ptr(), g.data_ptr(), d_logits.data_ptr(), lg.shape[0],
                                         lg.shape[1], L.dtype_code(lg), L.stream_ptr(dev)), "cross-entropy backward")
        return d_logits, None


def fused_cross_entropy(logits: Tensor, labels: Tensor) -> Tensor:
    """Mean cross-entropy of (batch, classes) logits (float32 or bfloat16) as a float32 scalar, with
    `F.cross_entropy`'s defaults: rows labelled -100 (its ignore_index) add nothing, get a zero gradient and do not count
    in the mean.  Any other label outside [0, classes) makes the loss and that row's gradient NaN (torch raises there;
    the reference's loaders never produce one: dctn/dataset_loading.py:282-286)."""
    return L.on_device(_FusedCrossEntropy.apply, logits, labels)


fused_cross_entropy.accepts_low_precision = True   # train_step / GraphedTrainStep skip their float32 cast


def _write_cell(cell: Tensor, value) -> None:
    """The small write into one cell of a device block (a one-element view of it): asynchronous, on the current stream of
    the cell's device, so that replays of an already captured graph read the new value.  The caller refuses captures."""
    if cell.is_cuda:
        with torch.cuda.device(cell.device):
            cell.fill_(value)
    else:
        cell.fill_(value)


def _refuse_capture(device: torch.device, message: str) -> None:
    """RuntimeError(``message``) while the current stream of a CUDA ``device`` is being captured: a write or a read of a
    device block from the host would become a node of that graph, or fail it.  A block on the CPU is never captured, and
    the runtime is not asked."""
    if device.type == "cuda" and torch.cuda.is_current_stream_capturing():
        raise RuntimeError(message)


class _WordTable:
    """What `LRSchedule`, `ParamGroups` and `WeightEMA` share: a block ``_block`` of ``WORDS`` int32 words on ``device``
    that is uploaded whole from ``host_block(...)``, changed between launches only, and restored from its own bytes (no
    host scalars travel beside it).  Each class turns restored bytes into words itself: the three complaints about a
    wrong size differ in more than the class's name."""

    _READS = "table"   # what the refusal says the captured step reads from the device

    def _upload(self, *counts) -> None:
        with torch.no_grad():
            self._block.copy_(torch.from_numpy(self.host_block(*counts)))

    def _no_capture(self, what: str) -> None:
        _refuse_capture(self.device, f"{type(self).__name__}.{what} during a graph capture: the captured step reads the "
                                     f"{self._READS} from the device, change it between replays")

    def run_host(self) -> None:
        return None


class GradGuard:
    """The device-side gradient guard: a non-finite halt and global norm clipping that a captured iteration carries
    with it (`dctn_grad_guard_check`, include/dctn_amd.h).  Pass one to ``FlatAdam(..., guard=g)`` or
    ``FlatSGD(..., guard=g)``: ``step()`` then launches the check in front of the guarded step kernel.

    The check forms the squared norm of the flat gradient buffer in float64 and leaves a decision in a 32-byte DEVICE
    block {max_norm, last_norm, halted, bad_step, seen, clipped, ticket, coef} that the step kernel obeys:

    - a non-finite value anywhere in the gradients (or in the optional loss scalar) sets the latch ``halted`` and
      records ``bad_step`` = the number of checks that ran before this one; the step is NOT applied, and neither is any
      later one until ``reset()`` - parameters, moments, master copy and step count stay as the last good step left
      them.  This is the reference's stop-on-NaN-loss hook without a host read per iteration;
    - otherwise the gradients are multiplied by ``coef = min(1, max_norm / (norm + 1e-6))``,
      ``torch.nn.utils.clip_grad_norm_``'s coefficient, as one rounded float32 product per element.  The clip applies to
      the gradient as it stands in the buffer (after the all-reduce; a regulariser that went through ``reg_fn`` and
      autograd is in the buffer and is clipped with it); ``weight_decay * w`` and the kernel's fused ``2 * l2 * w`` come
      after it - ``clip_grad_norm_`` followed by ``Adam(weight_decay=...)``.  ``max_norm=None`` (+inf) never clips, and
      a step whose ``coef`` is 1 is, bit for bit, the unguarded step.

    ``max_norm`` may be assigned at any time outside a capture (a tiny asynchronous device write, as ``FlatAdam.lr``):
    replays of an already captured graph follow it.  ``read()`` returns the block as a dictionary and synchronises;
    nothing else here does.  ``state_dict()`` / ``load_state_dict()`` carry the block.
    """

    FIELDS = ("max_norm", "last_norm", "halted", "bad_step", "seen", "clipped", "ticket", "coef")
    _FLOATS = (0, 1, 7)

    def __init__(self, device, max_norm: Optional[float] = None):
        self.device = torch.device(device)
        lib = L.lib()
        assert lib.dctn_grad_guard_state_bytes() == 32
        self._block = torch.zeros(8, dtype=torch.int32, device=self.device)
        # one float64 slot per workgroup of the check; the grid never exceeds what the largest n asks for
        self._partials = torch.empty(lib.dctn_grad_guard_num_partials(1 << 62), dtype=torch.float64, device=self.device)
        self._cells = self._block.view(torch.float32)
        self._max_norm = float("nan")
        self._write(dict(max_norm=float("inf") if max_norm is None else float(max_norm), last_norm=0.0, halted=0,
                         bad_step=-1, seen=0, clipped=0, ticket=0, coef=0.0))

    def _write(self, values: Dict[str, Any]) -> None:
        host = torch.zeros(8, dtype=torch.int32)
        for i, name in enumerate(self.FIELDS):
            if i in self._FLOATS:
                host.view(torch.float32)[i] = float(values[name])
            else:
                host[i] = int(values[name])
        self._max_norm = float(values["max_norm"])
        with torch.no_grad():
            self._block.copy_(host)

    @property
    def max_norm(self) -> float:
        return self._max_norm

    @max_norm.setter
    def max_norm(self, value: Optional[float]) -> None:
        _refuse_capture(self.device, "GradGuard.max_norm cannot be assigned during a graph capture: the captured check "
                                     "reads the threshold from the device, assign it between replays")
        self._max_norm = float("inf") if value is None else float(value)
        _write_cell(self._cells[0:1], self._max_norm)

    def check(self, grads: Tensor, loss: Optional[Tensor] = None) -> None:
        """Launches the check over the flat gradient buffer ``grads`` (and the float32 device scalar ``loss``)."""
        if loss is not None and (loss.dtype != torch.float32 or loss.numel() != 1 or loss.device != grads.device):
            raise TypeError("GradGuard: the loss must be a float32 scalar on the gradients' device")
        L.check(L.lib().dctn_grad_guard_check(grads.data_ptr(), grads.numel(), L.dtype_code(grads),
                                              None if loss is None else loss.data_ptr(), self._partials.data_ptr(),
                                              self._block.data_ptr(), L.stream_ptr(grads.device)), "gradient guard")

    def read(self) -> Dict[str, Any]:
        """The block as a dictionary (synchronises)."""
        host = self._block.cpu()
        floats = host.view(torch.float32)
        return {name: (float(floats[i]) if i in self._FLOATS else int(host[i])) for i, name in enumerate(self.FIELDS)}

    @property
    def halted(self) -> bool:
        """Whether the latch is set (read from the device: synchronises)."""
        return bool(self._block[2].item())

    def reset(self, counters: bool = False) -> None:
        """Clears the latch and ``bad_step`` (asynchronous; not during a capture): the next step is applied again.
        ``counters=True`` also zeroes ``seen`` and ``clipped``, so that ``bad_step`` counts from here."""
        _refuse_capture(self.device, "GradGuard.reset() during a graph capture would become a node of that graph")
        with torch.no_grad():
            self._block[2:3].zero_()
            self._block[3:4].fill_(-1)
            if counters:
                self._block[4:6].zero_()

    def state_dict(self) -> Dict[str, Any]:
        return self.read()

    def load_state_dict(self, state: Dict[str, Any]) -> None:
        self._write({**state, "ticket": 0})

    # A part of a run (`checkpoint.RunState`): the device tensors that travel, the host scalars
    # beside them, and how the host mirrors follow tensors that were put back.
    def run_regions(self):
        return [("block", self._block)]

    def run_host(self) -> Dict[str, Any]:
        return dict(max_norm=self._max_norm)

    def run_restored(self, host: Dict[str, Any], blocks) -> None:
        self._max_norm = float(host["max_norm"])

    @staticmethod
    def decide(total_sq: float, max_norm: float, halted_before: bool = False, loss: Optional[float] = None):
        """The kernel's decision on the host, in the kernel's number formats: ``(apply, coef, norm)`` for a float64 sum
        of squares ``total_sq``, a float32 threshold and an optional loss value."""
        import math

        total = torch.tensor(float(total_sq), dtype=torch.float64)
        norm = total.sqrt().to(torch.float32)
        finite = math.isfinite(float(total_sq)) and (loss is None or math.isfinite(float(loss)))
        if halted_before or not finite:
            return False, 0.0, float(norm)
        threshold = torch.tensor(float(max_norm), dtype=torch.float32).double()
        coef = (threshold / (norm.double() + 1e-6)).to(torch.float32)
        return True, min(1.0, float(coef)), float(norm)


class StepTrace:
    """The device-side step trace (`dctn_step_trace_record`, include/dctn_amd.h): a 16-byte head {records_done, ...} and a
    ring of ``capacity`` 64-byte records on the device.  ``record(...)`` enqueues ONE launch that writes the next slot and
    advances the head - it reads nothing on the host, so it can be captured, and replays fill consecutive slots
    (``GraphedTrainStep(..., trace=...)`` ends every iteration with it).  ``read()`` copies head and ring in stream order
    and returns the records not yet returned as a numpy structured array (`StepTrace.RECORD`) ordered by ``seq``;
    ``lost`` is then the number of records that were overwritten before they were read (the ring holds the last
    ``capacity``).  ``capacity`` may be any number >= 1.  ``state_dict()`` / ``load_state_dict()`` carry the head, so a
    resumed run continues its ``seq`` (`checkpoint.RunState(..., trace=...)` carries head and ring in place).

    Fields of a record: ``seq``; ``present`` (bits `PRESENT`: which of reg / guard / adam / source were given; an absent
    block's fields are 0); ``loss`` and ``reg`` (the float32 scalars' bits); ``rows`` (labels other than -100) and
    ``correct`` (label = lowest index of the row's maximum; `dctn_ce_score_accumulate`'s rules); ``grad_norm``, ``coef``,
    ``halted``, ``bad_step`` (the guard's block after this iteration's check); ``opt_steps_done``, ``lr`` (`FlatAdam`'s
    block after the step); ``batches_done`` (the source's counter after the iteration's draw)."""

    RECORD = None   # the numpy dtype of a record, set below the class (64 bytes)
    PRESENT = {"reg": L.TRACE_HAS_REG, "guard": L.TRACE_HAS_GUARD, "adam": L.TRACE_HAS_ADAM, "source": L.TRACE_HAS_SOURCE}

    def __init__(self, device, capacity: int = 4096):
        if int(capacity) != capacity or capacity < 1:
            raise ValueError(f"StepTrace: capacity must be an integer >= 1, got {capacity!r}")
        self.device, self.capacity = torch.device(device), int(capacity)
        lib = L.lib()
        assert lib.dctn_step_trace_head_bytes() == 16 and lib.dctn_step_trace_record_bytes() == 64
        self._head = torch.zeros(4, dtype=torch.int32, device=self.device)
        self._ring = torch.zeros(16 * self.capacity, dtype=torch.int32, device=self.device)
        self._last_read = 0   # records returned so far = the seq the next read() starts at
        self.lost = 0

    def record(self, logits: Tensor, labels: Tensor, loss: Tensor, reg: Optional[Tensor] = None,
               guard: Optional["GradGuard"] = None, optimizer=None, batch_source=None) -> None:
        """Enqueues the launch on the current stream.  ``logits`` (B, C) float32 / bfloat16, ``labels`` int64, ``loss`` and
        ``reg`` float32 device scalars (a ``reg`` of another dtype is cast first: one more launch).  The Adam block is
        taken from a `FlatAdam` or a `FlatRMSprop`, or from a `FlatSGD` that owns one (with a schedule, a group table or
        a weight average: the same layout); a `FlatSGD` without one (or any other optimizer) has no device block and
        passes none."""
        dev = L.require_device(logits, labels, loss)
        if logits.ndim != 2 or labels.shape != (logits.shape[0],) or labels.dtype != torch.int64:
            raise TypeError("StepTrace.record: logits (batch, classes) and int64 labels (batch,)")
        if loss.dtype != torch.float32 or loss.numel() != 1:
            raise TypeError("StepTrace.record: the loss must be a float32 scalar on the logits' device")
        if not (logits.is_contiguous() and labels.is_contiguous()):
            raise TypeError("StepTrace.record: logits and labels must be contiguous (a copy here would be a launch per step)")
        if reg is not None:
            if reg.numel() != 1:
                raise TypeError("StepTrace.record: reg must be a scalar")
            reg = reg.detach().to(device=dev, dtype=torch.float32)
        # (a FlatSGD has the block only with a schedule: the same 16 bytes; a FlatRMSprop always has it)
        adam = getattr(optimizer, "_state", None) if isinstance(optimizer, _FlatOptimizer) else None
        L.check(L.lib().dctn_step_trace_record(
            logits.data_ptr(), labels.data_ptr(), loss.data_ptr(), None if reg is None else reg.data_ptr(),
            None if guard is None else guard._block.data_ptr(), None if adam is None else adam.data_ptr(),
            None if batch_source is None else batch_source._state.data_ptr(), self._head.data_ptr(),
            self._ring.data_ptr(), self.capacity, logits.shape[0], logits.shape[1], L.dtype_code(logits),
            L.stream_ptr(dev)), "step trace")

    @staticmethod
    def decode(head_bytes, ring_bytes, capacity: int, last_read: int):
        """The slot arithmetic on the host: ``(records, lost, records_done)`` for the bytes of a head and a ring.  The ring
        holds the records ``seq`` in [max(0, done - capacity), done), record ``seq`` in slot ``seq % capacity``; returned
        are those with ``seq >= last_read``, in order; ``lost`` = how many records between ``last_read`` and the window's
        start are gone.  A ``last_read`` past ``done`` (the head was put back to an earlier state) returns nothing."""
        import numpy as np

        capacity, last_read = int(capacity), int(last_read)
        if capacity < 1 or last_read < 0:
            raise ValueError(f"StepTrace.decode: capacity >= 1 and last_read >= 0, got {capacity}, {last_read}")
        head = np.frombuffer(bytes(head_bytes), dtype="<u4")
        ring = np.frombuffer(bytes(ring_bytes), dtype=StepTrace.RECORD)
        if head.size != 4 or ring.size != capacity:
            raise ValueError(f"StepTrace.decode: a head of 16 bytes and a ring of {capacity} records of 64 bytes, got "
                             f"{len(bytes(head_bytes))} and {len(bytes(ring_bytes))} bytes")
        done = int(head[0])
        start = max(0, done - capacity)
        lost = max(0, start - last_read)
        seqs = np.arange(max(start, last_read), done, dtype=np.int64)
        records = ring[seqs % capacity].copy()
        if records.size and not np.array_equal(records["seq"].astype(np.int64), seqs):
            raise RuntimeError("StepTrace.decode: the ring's records do not carry the sequence numbers the head implies "
                               "(head and ring were not read at one point of the stream)")
        return records, lost, done

    def read(self):
        """The records not yet returned, ordered by ``seq`` (copies head and ring in stream order: it synchronises)."""
        _refuse_capture(self.device, "StepTrace.read() copies to the host: not during a graph capture")
        both = torch.cat((self._head, self._ring)).cpu().numpy()   # one copy kernel, one transfer: one point of the stream
        records, self.lost, done = self.decode(both[:4].tobytes(), both[4:].tobytes(), self.capacity, self._last_read)
        self._last_read = done
        return records

    def state_dict(self) -> Dict[str, Any]:
        words = [int(v) & 0xFFFFFFFF for v in self._head.cpu().tolist()]
        return {"records_done": words[0], "capacity": self.capacity}

    def load_state_dict(self, state: Dict[str, Any]) -> None:
        """Puts the head back (in place: a captured graph keeps its pointer); the records before it count as read."""
        done = int(state["records_done"]) & 0xFFFFFFFF
        host = torch.tensor([done - (1 << 32) if done >= 1 << 31 else done, 0, 0, 0], dtype=torch.int32)
        with torch.no_grad():
            self._head.copy_(host)
        self._last_read, self.lost = done, 0

    # a part of a run, as `GradGuard`
    def run_regions(self):
        return [("head", self._head), ("ring", self._ring)]

    def run_host(self) -> None:
        return None

    def run_restored(self, host, blocks) -> None:
        """Head and ring came back with their regions: the records before the head count as read."""
        self._last_read, self.lost = int(blocks["head"][:4].view("<u4")[0]), 0


def _trace_record_dtype():
    import numpy as np

    return np.dtype([("seq", "<u4"), ("present", "<u4"), ("loss", "<f4"), ("reg", "<f4"), ("rows", "<i4"),
                     ("correct", "<i4"), ("grad_norm", "<f4"), ("coef", "<f4"), ("halted", "<u4"), ("bad_step", "<i4"),
                     ("opt_steps_done", "<i4"), ("lr", "<f4"), ("batches_done", "<u4"), ("pad", "<u4", (3,))])


StepTrace.RECORD = _trace_record_dtype()
assert StepTrace.RECORD.itemsize == 64


class LRSchedule(_WordTable):
    """A learning-rate schedule that lives on the device (`dctn_adam_l2_step_scheduled` / `dctn_sgd_l2_step_scheduled`,
    include/dctn_amd.h): a table of at most 64 knots ``(step, lr)`` in a 784-byte DEVICE block that the optimizer launch
    itself evaluates at the device step count.  Pass one to ``FlatAdam(..., schedule=s)`` or ``FlatSGD(..., schedule=s)``:
    every replay of a captured step, and each of the K iterations of ``GraphedTrainStep(iters_per_launch=K)``, then
    steps with its own rate - no host write, no further graph node.

    The step index ``s`` is the 0-based index of the step being taken (the first step uses the value at 0, as
    ``torch.optim.lr_scheduler.LambdaLR``).  The value is ``lr[0]`` in front of the first knot, ``lr[n-1]`` from the last
    knot on, ``lr[i]`` on a segment with ``hold[i]`` set, and otherwise linear between the two knots around ``s``: one
    float64 division, multiplication and addition, rounded to float32, then one float32 product with ``scale``.
    ``value(step)`` is that arithmetic in numpy, bit for bit what the kernel uses (and what `dctn_lr_schedule_value`
    returns on the host).  A step the gradient guard skipped does not count: the schedule holds its place with the
    optimizer's step count.

    ``hold``: one flag per knot (None: every segment linear).  ``set(knots, hold)`` rewrites the table in place and
    ``scale`` may be assigned, both between launches only (RuntimeError during a capture, as ``FlatAdam.lr``): replays of
    an already captured graph follow them.  ``device`` may be "cpu" for host-side use of the table; an optimizer takes a
    schedule on its own device only.  ``state_dict()`` / ``load_state_dict()`` carry the table and the scale.
    """

    MAX_KNOTS = 64
    WORDS = 196   # 784 bytes: n_knots, scale, reserved[2], k[64], lr[64], hold[64]

    def __init__(self, device, knots, hold=None):
        self.device = torch.device(device)
        self._k, self._lr, self._hold = self._validated(knots, hold)
        self._scale = 1.0
        self._block = torch.zeros(self.WORDS, dtype=torch.int32, device=self.device)
        self._scale_cell = self._block.view(torch.float32)[1:2]
        self._upload()

    # ---------------------------------------------------------------------------------------- host arithmetic
    @classmethod
    def _validated(cls, knots, hold):
        import math

        import numpy as np

        knots = [tuple(pair) for pair in knots]
        if not 1 <= len(knots) <= cls.MAX_KNOTS:
            raise ValueError(f"LRSchedule: 1 to {cls.MAX_KNOTS} knots, got {len(knots)}")
        ks, lrs = [], []
        for step, lr in knots:
            if int(step) != step or not 0 <= int(step) < 1 << 31:
                raise ValueError(f"LRSchedule: a knot's step is an integer in [0, 2^31), got {step!r}")
            if ks and int(step) <= ks[-1]:
                raise ValueError(f"LRSchedule: the knots' steps must increase strictly, got {ks[-1]} then {step}")
            with np.errstate(over="ignore"):
                rate = float(np.float32(lr))   # the table holds float32 values
            if not (math.isfinite(rate) and rate >= 0.0):
                raise ValueError(f"LRSchedule: a rate must be finite (in float32) and >= 0, got {lr!r}")
            ks.append(int(step))
            lrs.append(rate)
        if hold is None:
            holds = [0] * len(ks)
        else:
            holds = [1 if h else 0 for h in hold]
            if len(holds) != len(ks):
                raise ValueError(f"LRSchedule: one hold flag per knot: {len(holds)} flags, {len(ks)} knots")
        return ks, lrs, holds

    @staticmethod
    def _validated_scale(scale) -> float:
        import math

        import numpy as np

        with np.errstate(over="ignore"):
            value = float(np.float32(scale))
        if not (math.isfinite(value) and value >= 0.0):
            raise ValueError(f"LRSchedule: the scale must be finite (in float32) and >= 0, got {scale!r}")
        return value

    @staticmethod
    def evaluate(k, lr, hold, scale, step) -> float:
        """The value at ``step`` of the table (``k``, ``lr``, ``hold``) times ``scale``, in the kernel's number formats."""
        import bisect

        import numpy as np

        s, n = int(step), len(k)
        reached = bisect.bisect_right(k, s)   # knots with k <= s
        i = max(reached, 1) - 1
        value = np.float32(lr[i])
        if 0 < reached < n and not hold[i]:
            a, b = np.float64(np.float32(lr[i])), np.float64(np.float32(lr[i + 1]))
            frac = np.float64(s - k[i]) / np.float64(k[i + 1] - k[i])
            rise = (b - a) * frac
            value = np.float32(a + rise)
        return float(np.float32(value * np.float32(scale)))

    def value(self, step: int) -> float:
        """The rate of the step with 0-based index ``step``, scale applied: the kernel's bits."""
        return self.evaluate(self._k, self._lr, self._hold, self._scale, step)

    def host_block(self):
        """The 784 bytes of the block as a numpy int32 array of 196 words (what `dctn_lr_schedule_value` takes)."""
        import numpy as np

        words = np.zeros(self.WORDS, dtype=np.int32)
        n = len(self._k)
        words[0] = n
        words.view(np.float32)[1] = self._scale
        words[4: 4 + n] = self._k
        words.view(np.float32)[68: 68 + n] = self._lr
        words[132: 132 + n] = self._hold
        return words

    @classmethod
    def decode(cls, words):
        """``(knots, hold, scale)`` of a block given as 196 int32 words (or its 784 bytes)."""
        import numpy as np

        words = np.frombuffer(bytes(words), dtype="<i4") if not isinstance(words, np.ndarray) else words.view("<i4").reshape(-1)
        if words.size != cls.WORDS:
            raise ValueError(f"LRSchedule.decode: a block has {cls.WORDS * 4} bytes, got {words.size * 4}")
        n = int(words[0])
        if not 1 <= n <= cls.MAX_KNOTS:
            raise ValueError(f"LRSchedule.decode: n_knots = {n}")
        floats = words.view(np.float32)
        knots = [(int(words[4 + i]), float(floats[68 + i])) for i in range(n)]
        return knots, [int(words[132 + i] != 0) for i in range(n)], float(floats[1])

    # ---------------------------------------------------------------------------------------- the device block
    def set(self, knots, hold=None) -> None:
        """Rewrites the table in place (the scale stays): the next launch, a replay included, follows it."""
        self._no_capture("set()")
        self._k, self._lr, self._hold = self._validated(knots, hold)
        self._upload()

    @property
    def scale(self) -> float:
        return self._scale

    @scale.setter
    def scale(self, value: float) -> None:
        self._no_capture("scale cannot be assigned")
        self._scale = self._validated_scale(value)
        _write_cell(self._scale_cell, self._scale)

    @property
    def knots(self):
        return list(zip(self._k, self._lr))

    @property
    def hold(self):
        return list(self._hold)

    def state_dict(self) -> Dict[str, Any]:
        return {"knots": [[k, lr] for k, lr in zip(self._k, self._lr)], "hold": list(self._hold), "scale": self._scale}

    def load_state_dict(self, state: Dict[str, Any]) -> None:
        self._no_capture("load_state_dict()")
        scale = self._validated_scale(state["scale"])
        self._k, self._lr, self._hold = self._validated(state["knots"], state["hold"])
        self._scale = scale
        self._upload()

    # a part of a run, as `GradGuard`; the optimizer that holds the schedule lists the block among its own regions
    def run_regions(self):
        return [("schedule", self._block)]

    def run_restored(self, host, blocks) -> None:
        """Sets the host copy from the block's bytes (`checkpoint.RunState.load` put the block itself back)."""
        knots, hold, scale = self.decode(blocks["schedule"])
        self._k, self._lr, self._hold = self._validated(knots, hold)
        self._scale = self._validated_scale(scale)

    # ---------------------------------------------------------------------------------------- builders
    @classmethod
    def constant(cls, device, lr: float) -> "LRSchedule":
        return cls(device, [(0, lr)])

    @classmethod
    def warmup(cls, device, peak: float, warmup_steps: int, start: float = 0.0) -> "LRSchedule":
        """Linear from ``start`` at step 0 to ``peak`` at step ``warmup_steps``, then constant."""
        if int(warmup_steps) < 1:
            return cls.constant(device, peak)
        return cls(device, [(0, start), (int(warmup_steps), peak)])

    @classmethod
    def warmup_cosine(cls, device, peak: float, warmup_steps: int, total_steps: int, final: float = 0.0) -> "LRSchedule":
        """Linear from 0 to ``peak`` over ``warmup_steps``, then half a cosine from ``peak`` down to ``final`` at
        ``total_steps`` (constant after it), the cosine sampled on the knots the warm-up leaves free - 63 of them, 64
        without a warm-up, fewer when the decay has fewer steps - with linear pieces between them."""
        import math

        warm, total = max(int(warmup_steps), 0), int(total_steps)
        if total <= warm:
            raise ValueError(f"LRSchedule.warmup_cosine: total_steps ({total_steps}) must exceed warmup_steps ({warmup_steps})")
        free = cls.MAX_KNOTS - (1 if warm > 0 else 0)
        m = min(free, total - warm + 1)   # sample points, both ends included; >= 2
        steps = [warm + (j * (total - warm)) // (m - 1) for j in range(m)]   # strictly increasing: m - 1 <= total - warm
        knots = [(0, 0.0)] if warm > 0 else []
        for s in steps:
            knots.append((s, final + (peak - final) * 0.5 * (1.0 + math.cos(math.pi * (s - warm) / (total - warm)))))
        knots[-1] = (total, final)   # cos(pi) in floating point is -1 exactly, but say it
        return cls(device, knots)

    @classmethod
    def milestones(cls, device, lr: float, milestones: Sequence[int], gamma: float) -> "LRSchedule":
        """``torch.optim.lr_scheduler.MultiStepLR``: ``lr * gamma^j`` from the j-th milestone on, held in between."""
        marks = [int(m) for m in milestones]
        if any(m < 1 for m in marks):
            raise ValueError(f"LRSchedule.milestones: milestones are steps >= 1, got {list(milestones)}")
        knots = [(0, lr)] + [(m, lr * gamma ** (j + 1)) for j, m in enumerate(marks)]
        return cls(device, knots, hold=[1] * len(knots))

    @classmethod
    def per_epoch(cls, device, rates: Sequence[float], steps_per_epoch: int) -> "LRSchedule":
        """One rate per epoch, held for the epoch's ``steps_per_epoch`` steps: step ``s`` gets
        ``rates[s // steps_per_epoch]``, and the last rate holds from the last epoch on.  What a scheduler stepped once
        per epoch gives (the reference's classifier warms up so, mnist.py:490-494); at most 64 epochs fit the table."""
        rates = [r for r in rates]
        if int(steps_per_epoch) != steps_per_epoch or int(steps_per_epoch) < 1:
            raise ValueError(f"LRSchedule.per_epoch: steps_per_epoch is an integer >= 1, got {steps_per_epoch!r}")
        if not 1 <= len(rates) <= cls.MAX_KNOTS:
            raise ValueError(f"LRSchedule.per_epoch: 1 to {cls.MAX_KNOTS} rates (one knot per epoch), got {len(rates)}")
        return cls(device, [(e * int(steps_per_epoch), r) for e, r in enumerate(rates)], hold=[1] * len(rates))


class ParamGroup:
    """One entry of a `ParamGroups` table: the parameters it names (matched by identity) get ``lr_scale``,
    ``weight_decay`` (None: the optimizer's own value) and ``frozen``."""

    def __init__(self, params, lr_scale: float = 1.0, weight_decay: Optional[float] = None, frozen: bool = False):
        self.params = [params] if isinstance(params, Tensor) else list(params)
        self.lr_scale, self.weight_decay, self.frozen = lr_scale, weight_decay, bool(frozen)


class ParamGroups(_WordTable):
    """A parameter-group table that lives on the device (`dctn_adam_l2_step_grouped` / `dctn_sgd_l2_step_grouped`,
    include/dctn_amd.h): one SEGMENT per parameter of the optimizer's flat buffer, each with its own rate multiplier,
    weight decay, frozen flag and step count, in a 1552-byte DEVICE block that the ONE optimizer launch obeys.  Pass it
    to ``FlatAdam(..., groups=g)`` or ``FlatSGD(..., groups=g)``.

    ``params``: the optimizer's parameters in flat order (regularised + others), at most 64 (NotImplementedError).
    ``entries``: `ParamGroup` objects; a parameter no entry names takes the defaults (scale 1, the optimizer's weight
    decay, not frozen); naming a parameter that is not in ``params``, or one twice, raises ValueError.

    A segment's rate is the float32 product ``rate * lr_scale``; Adam's bias corrections and SGD's first step follow the
    SEGMENT's own count of steps, as ``torch.optim`` keeps one ``state["step"]`` / ``momentum_buffer`` per parameter.  A
    frozen segment is not touched at all - parameters, master copy, moments and its count stay, its gradient is not read
    (it may be None) - but it still counts in ``reg_value()``: the reference's regulariser sums every core whatever
    ``requires_grad`` says.  ``from_requires_grad`` freezes what has ``requires_grad = False``: the reference's
    ``--freeze-eps``.

    ``set`` / ``freeze`` are small writes on the current stream BETWEEN launches (RuntimeError during a capture, as
    ``LRSchedule.set``): replays of an already captured graph follow them.  ``steps`` reads the counts from the device
    (it synchronises).  ``segment_of(i)`` is the host mirror of the kernel's lookup.  The guard's norm and the
    all-reduce still cover the whole flat buffer, frozen segments included.
    """

    MAX_SEGMENTS = 64
    WORDS = 388   # 1552 bytes: n_segments, reserved[3], int64 end[64], lr_scale[64], weight_decay[64], flags[64], steps[64]
    _END, _SCALE, _WD, _FLAGS, _STEPS = 4, 132, 196, 260, 324   # word offsets

    def __init__(self, params, entries=()):
        import numpy as np

        self.params = [p for p in params]
        if not self.params:
            raise ValueError("ParamGroups: no parameters")
        if len(self.params) > self.MAX_SEGMENTS:
            raise NotImplementedError(f"ParamGroups: at most {self.MAX_SEGMENTS} parameters (one segment per lane of a "
                                      f"wave), got {len(self.params)}")
        if any(p.numel() < 1 for p in self.params):
            raise ValueError("ParamGroups: a parameter without elements has no segment")
        self.device = self.params[0].device
        self._index = {id(p): i for i, p in enumerate(self.params)}
        if len(self._index) != len(self.params):
            raise ValueError("ParamGroups: a parameter appears twice in `params`")
        k = len(self.params)
        self._ends = np.cumsum([p.numel() for p in self.params]).astype(np.int64)
        self._scale = [1.0] * k
        self._wd: list = [None] * k            # None: the optimizer's own value, known once an optimizer binds the table
        self._frozen = [False] * k
        self._default_wd, self._wd_allowed = 0.0, True
        named = set()
        for entry in entries:
            if not isinstance(entry, ParamGroup):
                raise TypeError(f"ParamGroups: an entry is a ParamGroup, got {type(entry).__name__}")
            scale, wd = self._validated("lr_scale", entry.lr_scale), entry.weight_decay
            wd = None if wd is None else self._validated("weight_decay", wd)
            for p in entry.params:
                i = self._index.get(id(p))
                if i is None:
                    raise ValueError("ParamGroups: an entry names a parameter that is not one of the optimizer's")
                if i in named:
                    raise ValueError(f"ParamGroups: parameter {i} is named by two entries")
                named.add(i)
                self._scale[i], self._wd[i], self._frozen[i] = scale, wd, entry.frozen
        self._block = torch.zeros(self.WORDS, dtype=torch.int32, device=self.device)
        self._upload(np.zeros(k, dtype=np.int32))

    @classmethod
    def from_requires_grad(cls, params, entries=()) -> "ParamGroups":
        """The table of ``entries`` with every parameter whose ``requires_grad`` is False frozen as well."""
        groups = cls(params, entries)
        for i, p in enumerate(groups.params):
            if not p.requires_grad:
                groups._frozen[i] = True
        groups._upload(groups._host_steps())
        return groups

    # ---------------------------------------------------------------------------------------- host side
    @staticmethod
    def _validated(what: str, value) -> float:
        import math

        import numpy as np

        with np.errstate(over="ignore"):
            v = float(np.float32(value))
        if not (math.isfinite(v) and v >= 0.0):
            raise ValueError(f"ParamGroups: {what} must be finite (in float32) and >= 0, got {value!r}")
        return v

    def __len__(self) -> int:
        return len(self.params)

    def index_of(self, param) -> int:
        """The segment of a parameter (or the index itself when an int is given)."""
        if isinstance(param, int):
            if not 0 <= param < len(self.params):
                raise ValueError(f"ParamGroups: no segment {param}")
            return param
        i = self._index.get(id(param))
        if i is None:
            raise ValueError("ParamGroups: not one of the table's parameters")
        return i

    def segment_of(self, i: int) -> int:
        """The segment that holds flat element ``i``: what the kernel's cursor finds."""
        import numpy as np

        if not 0 <= int(i) < int(self._ends[-1]):
            raise IndexError(f"ParamGroups.segment_of: element {i} of {int(self._ends[-1])}")
        return int(np.searchsorted(self._ends, int(i), side="right"))

    @property
    def ends(self):
        return [int(e) for e in self._ends]

    @property
    def lr_scales(self):
        return list(self._scale)

    @property
    def weight_decays(self):
        """Every segment's weight decay as the kernel gets it (None entries resolved to the optimizer's value)."""
        return [self._default_wd if w is None else w for w in self._wd]

    @property
    def frozen(self):
        return list(self._frozen)

    def host_block(self, steps=None):
        """The 1552 bytes of the block as a numpy int32 array of 388 words (what `dctn_param_groups_check` takes), with
        ``steps`` as the counts (zeros when None)."""
        import numpy as np

        k = len(self.params)
        words = np.zeros(self.WORDS, dtype=np.int32)
        words[0] = k
        words[self._END: self._END + 128].view(np.int64)[:k] = self._ends
        floats = words.view(np.float32)
        floats[self._SCALE: self._SCALE + k] = self._scale
        floats[self._WD: self._WD + k] = self.weight_decays
        words[self._FLAGS: self._FLAGS + k] = [1 if f else 0 for f in self._frozen]
        if steps is not None:
            words[self._STEPS: self._STEPS + k] = steps
        return words

    # ---------------------------------------------------------------------------------------- the device block
    def _host_steps(self):
        return self._block[self._STEPS: self._STEPS + len(self.params)].cpu().numpy()

    def _bind(self, default_weight_decay: Optional[float], owner: str) -> None:
        """An optimizer takes the table: None weight decays become its value; an optimizer without weight decay
        (``default_weight_decay`` None) refuses explicit ones."""
        if default_weight_decay is None:
            if any(w is not None for w in self._wd):
                raise ValueError(f"{owner} has no weight decay: a ParamGroup for it must leave weight_decay=None")
            self._default_wd, self._wd_allowed = 0.0, False
        else:
            self._default_wd, self._wd_allowed = self._validated("weight_decay", default_weight_decay), True
        self._upload(self._host_steps())

    def set(self, param, lr_scale: Optional[float] = None, weight_decay: Optional[float] = None,
            frozen: Optional[bool] = None) -> None:
        """Changes one segment (``param``: the parameter, or its index) in place; arguments left None stay as they are.
        The next launch, a replay included, follows it."""
        self._no_capture("set()")
        i = self.index_of(param)
        if weight_decay is not None and not self._wd_allowed:
            raise ValueError("ParamGroups.set: the optimizer that holds this table has no weight decay")
        floats = self._block.view(torch.float32)
        if lr_scale is not None:
            self._scale[i] = self._validated("lr_scale", lr_scale)
            _write_cell(floats[self._SCALE + i: self._SCALE + i + 1], self._scale[i])
        if weight_decay is not None:
            self._wd[i] = self._validated("weight_decay", weight_decay)
            _write_cell(floats[self._WD + i: self._WD + i + 1], self._wd[i])
        if frozen is not None:
            self._frozen[i] = bool(frozen)
            _write_cell(self._block[self._FLAGS + i: self._FLAGS + i + 1], 1 if frozen else 0)

    def freeze(self, param, flag: bool = True) -> None:
        """Freezes (or with ``flag=False`` releases) one segment from the next launch on.  A released segment goes on from
        its own count of steps: its bias corrections are those of a parameter that has taken that many steps."""
        self.set(param, frozen=bool(flag))

    @property
    def steps(self):
        """The segments' step counts, read from the device (it synchronises)."""
        return [int(s) for s in self._host_steps()]

    def state_dict(self) -> Dict[str, Any]:
        return {"ends": self.ends, "lr_scale": list(self._scale), "weight_decay": list(self._wd),
                "frozen": [bool(f) for f in self._frozen], "steps": self.steps}

    def load_state_dict(self, state: Dict[str, Any]) -> None:
        self._no_capture("load_state_dict()")
        k = len(self.params)
        if [int(e) for e in state["ends"]] != self.ends:
            raise ValueError(f"ParamGroups.load_state_dict: the state's segments end at {list(state['ends'])}, this "
                             f"table's at {self.ends}")
        if not (len(state["lr_scale"]) == len(state["weight_decay"]) == len(state["frozen"]) == len(state["steps"]) == k):
            raise ValueError(f"ParamGroups.load_state_dict: {k} segments, the state's lists disagree")
        wds = [None if w is None else self._validated("weight_decay", w) for w in state["weight_decay"]]
        if not self._wd_allowed and any(w is not None for w in wds):
            raise ValueError("ParamGroups.load_state_dict: the optimizer that holds this table has no weight decay")
        steps = [int(s) for s in state["steps"]]
        if any(s < 0 for s in steps):
            raise ValueError("ParamGroups.load_state_dict: a negative step count")
        self._scale = [self._validated("lr_scale", s) for s in state["lr_scale"]]
        self._wd, self._frozen = wds, [bool(f) for f in state["frozen"]]
        import numpy as np

        self._upload(np.array(steps, dtype=np.int32))

    # a part of a run, as `GradGuard`; the optimizer that holds the table lists the block among its own regions
    def run_regions(self):
        return [("groups", self._block)]

    def run_restored(self, host, blocks) -> None:
        """Sets the host copy from the block's bytes (`checkpoint.RunState.load` put the block itself back)."""
        import numpy as np

        words = np.ascontiguousarray(blocks["groups"]).view("<i4").reshape(-1)
        k = len(self.params)
        if words.size != self.WORDS or int(words[0]) != k:
            raise ValueError(f"ParamGroups: the block describes {int(words[0]) if words.size else '?'} segments, this "
                             f"table has {k}")
        ends = words[self._END: self._END + 128].view(np.int64)[:k]
        if not np.array_equal(ends, self._ends):
            raise ValueError(f"ParamGroups: the block's segments end at {ends.tolist()}, this table's at {self.ends}")
        floats = words.view(np.float32)
        self._scale = [float(x) for x in floats[self._SCALE: self._SCALE + k]]
        saved = [float(x) for x in floats[self._WD: self._WD + k]]
        # (a None stays a None where the block holds the bound optimizer's value; an optimizer without weight decay)
        self._wd = [None if not self._wd_allowed or (old is None and x == self._default_wd) else x
                    for old, x in zip(self._wd, saved)]
        self._frozen = [bool(x & 1) for x in words[self._FLAGS: self._FLAGS + k]]


def param_groups_for(model, freeze_eps=(), head_lr_scale: float = 1.0) -> ParamGroups:
    """The table of an ``EPSesPlusLinear`` for the runner's flags, over the parameters in the order
    ``list(model.epses) + [model.linear.weight, model.linear.bias]`` (what `FlatAdam` is given as regularised + others):
    the cores listed in ``freeze_eps`` (the reference's ``--freeze-eps INDEX``) and every parameter whose
    ``requires_grad`` is False are frozen, and the head (``linear.weight`` and ``linear.bias``) steps with
    ``head_lr_scale`` times the rate."""
    epses = list(model.epses)
    frozen = sorted({int(i) for i in freeze_eps})
    if any(not 0 <= i < len(epses) for i in frozen):
        raise ValueError(f"param_groups_for: freeze_eps {list(freeze_eps)} with {len(epses)} EPSes")
    entries = [ParamGroup([epses[i] for i in frozen], frozen=True)] if frozen else []
    entries.append(ParamGroup([model.linear.weight, model.linear.bias], lr_scale=head_lr_scale))
    return ParamGroups.from_requires_grad(epses + [model.linear.weight, model.linear.bias], entries)


class WeightEMA(_WordTable):
    """An exponential moving average of the weights that the optimizer's step kernel keeps (include/dctn_amd.h, "A
    weight average").  Pass one to ``FlatAdam(..., ema=e)`` or ``FlatSGD(..., ema=e)``: the optimizer binds it -
    ``e.values`` (float32, one per element of the flat buffer) starts as the master copy where there is one, else as the
    exact widening of the parameters - and every ``step()`` then updates the average in the launch that updates the
    parameters, from the value the optimizer keeps for each element (the float32 master value, else the parameter as
    stored): ``ema = ema + omd * (w - ema)`` in three rounded float32 operations.  A captured step, and each of the K
    iterations of one launch, carries it; a step the guard skipped leaves it alone; a frozen segment's average stays.

    ``omd = float32(1 - d_u)`` with ``d_u = decay``, or with ``warmup`` ``min(decay, (1 + u) / (10 + u))`` where ``u`` is
    the number of updates so far, which the launch reads from and advances in a 32-byte DEVICE block {decay, flags,
    updates, last_omd}.  ``e.updates`` and ``e.last_omd`` read the block (they synchronise); ``e.decay = x`` is a one-cell
    asynchronous write between replays (not during a capture); ``e.reset()`` starts the average again from the current
    weights with ``updates = 0`` - call it after ``refresh_master()``.  `weight` and `mirror` are the host mirrors of
    the two pieces of arithmetic, bit for bit.

    Every captured graph reads the LIVE parameter storage, so scoring the averaged model means putting it there:
    ``e.apply()`` stashes the parameters and writes ``values`` rounded to their dtype in their place (one launch; the
    master copy is not touched), ``e.restore()`` puts the stash back, ``with e.applied(): ...`` does both.  While applied,
    ``optimizer.step()``, a `GraphedTrainStep` call, ``RunState.snapshot()`` and a second ``apply()`` raise RuntimeError.

    One decay for all parameters.  ``state_dict()`` / ``load_state_dict()`` carry the block and the values; the
    optimizer's own state_dict holds them under ``"ema"``, and `checkpoint.RunState` carries both as regions."""

    WORDS = 8
    _WARMUP = 1
    _READS = "block"

    def __init__(self, device, decay: float = 0.999, warmup: bool = True):
        self.device = torch.device(device)
        self._decay = self._validated(decay)
        self.warmup = bool(warmup)
        assert L.lib().dctn_weight_ema_bytes() == 4 * self.WORDS
        self._block = torch.zeros(self.WORDS, dtype=torch.int32, device=self.device)
        self._decay_cell = self._block.view(torch.float32)[0:1]
        self.values: Optional[Tensor] = None
        self._stash: Optional[Tensor] = None
        self._owner = None
        self._applied = False
        self._upload(0, 0.0)

    # ---------------------------------------------------------------------------------------- host arithmetic
    @staticmethod
    def _validated(decay) -> float:
        import numpy as np

        d = float(np.float32(decay))
        if not (math.isfinite(d) and 0.0 <= d < 1.0):
            raise ValueError(f"WeightEMA: decay must be in [0, 1) as a float32, got {decay!r}")
        return d

    @staticmethod
    def weight(decay, warmup, u) -> float:
        """``omd`` of the launch after ``u`` updates: the kernel's float64 arithmetic, rounded once to float32."""
        import numpy as np

        d = float(np.float32(decay))
        if warmup:
            d = min(d, (1.0 + float(u)) / (10.0 + float(u)))
        return float(np.float32(1.0 - d))

    @staticmethod
    def mirror(ema, w, omd):
        """The element update on numpy float32 arrays: a subtraction, a product and a sum, each rounded on its own."""
        import numpy as np

        ema, w = np.asarray(ema, dtype=np.float32), np.asarray(w, dtype=np.float32)
        return ema + np.float32(omd) * (w - ema)

    def host_block(self, updates: int = 0, last_omd: float = 0.0):
        """The 32-byte block as int32 words (include/dctn_amd.h)."""
        import numpy as np

        words = np.zeros(self.WORDS, dtype=np.int32)
        floats = words.view(np.float32)
        floats[0] = self._decay
        words[1] = self._WARMUP if self.warmup else 0
        words[2] = int(updates)
        floats[3] = float(last_omd)
        return words

    # ---------------------------------------------------------------------------------------- the device block
    @property
    def decay(self) -> float:
        return self._decay

    @decay.setter
    def decay(self, value: float) -> None:
        self._no_capture("decay cannot be assigned")
        self._decay = self._validated(value)
        _write_cell(self._decay_cell, self._decay)

    @property
    def updates(self) -> int:
        """Updates done so far (read from the device: synchronises; steps the guard skipped do not count)."""
        return int(self._block[2].item())

    @property
    def last_omd(self) -> float:
        """The weight the last update used, 0 before the first (read from the device: synchronises)."""
        return float(self._block.view(torch.float32)[3].item())

    @property
    def is_applied(self) -> bool:
        return self._applied

    # ---------------------------------------------------------------------------------------- binding
    def _bind(self, owner) -> None:
        """The optimizer's constructor: allocates the values and the stash beside ``owner.flat`` and starts the average."""
        if self._owner is not None:
            raise ValueError("this WeightEMA already belongs to an optimizer: one average per optimizer")
        if self.device != owner.flat.device:
            raise ValueError(f"the average's block is on {self.device}, the parameters on {owner.flat.device}")
        self.values = torch.empty(owner.n, dtype=torch.float32, device=self.device)
        self._stash = torch.empty(owner.n, dtype=owner.flat.dtype, device=self.device)
        self._owner = owner
        self._desc = L.WeightEma(ema=self.values.data_ptr(), block=self._block.data_ptr())
        self._desc_ref = ctypes.byref(self._desc)
        self.reset()

    def _bound(self, what: str):
        if self._owner is None:
            raise RuntimeError(f"WeightEMA.{what}: not bound to an optimizer (pass it as FlatAdam(..., ema=e))")
        return self._owner

    def reset(self) -> None:
        """Starts the average again: the values from the master copy where there is one, else from the parameters by exact
        widening, and ``updates = 0``.  Not during a capture, and not while applied."""
        owner = self._bound("reset()")
        self._no_capture("reset()")
        if self._applied:
            raise RuntimeError("WeightEMA.reset() while the average is applied: restore() first")
        with torch.no_grad():
            self.values.copy_(owner.flat if owner.master is None else owner.master)
        self._upload(0, 0.0)

    # ---------------------------------------------------------------------------------------- scoring under the average
    def apply(self) -> None:
        """Puts the averaged weights, rounded to the parameters' dtype, in the live parameter storage (one launch)."""
        owner = self._bound("apply()")
        if self._applied:
            raise RuntimeError("WeightEMA.apply(): the average is already applied; restore() first")
        flat = owner.flat
        L.check(L.lib().dctn_weight_ema_apply(flat.data_ptr(), self._stash.data_ptr(), self.values.data_ptr(), owner.n,
                                              L.dtype_code(flat), L.stream_ptr(flat.device)), "weight average apply")
        self._applied = True

    def restore(self) -> None:
        """Puts the parameters back as `apply` found them."""
        if not self._applied:
            raise RuntimeError("WeightEMA.restore(): the average is not applied")
        flat = self._owner.flat
        L.check(L.lib().dctn_weight_ema_restore(flat.data_ptr(), self._stash.data_ptr(), self._owner.n,
                                                L.dtype_code(flat), L.stream_ptr(flat.device)), "weight average restore")
        self._applied = False

    @contextlib.contextmanager
    def applied(self):
        self.apply()
        try:
            yield self
        finally:
            self.restore()

    def _refuse_applied(self, what: str) -> None:
        if self._applied:
            raise RuntimeError(f"{what} while the weight average is applied: the parameter storage holds the averaged "
                               "weights, call restore() first")

    # ---------------------------------------------------------------------------------------- state
    def state_dict(self) -> Dict[str, Any]:
        self._bound("state_dict()")
        return {"decay": self._decay, "warmup": self.warmup, "updates": self.updates, "last_omd": self.last_omd,
                "values": self.values.clone()}

    def load_state_dict(self, state: Dict[str, Any]) -> None:
        owner = self._bound("load_state_dict()")
        self._no_capture("load_state_dict()")
        self._refuse_applied("WeightEMA.load_state_dict()")
        if state["values"].numel() != owner.n:
            raise ValueError(f"the state holds {state['values'].numel()} averaged values, the parameters {owner.n}")
        self._decay, self.warmup = self._validated(state["decay"]), bool(state["warmup"])
        with torch.no_grad():
            self.values.copy_(state["values"].reshape(-1))
        self._upload(int(state["updates"]), float(state["last_omd"]))

    # a part of a run, as `GradGuard`; the optimizer that holds the average lists both among its own regions
    def run_regions(self):
        return [("ema", self.values), ("ema_block", self._block)]

    def run_restored(self, host, blocks) -> None:
        """Sets the host copy from the block's bytes (`checkpoint.RunState.load` put the block itself back)."""
        import numpy as np

        words = np.ascontiguousarray(blocks["ema_block"]).view("<i4").reshape(-1)
        if words.size != self.WORDS:
            raise ValueError(f"WeightEMA: a block has {4 * self.WORDS} bytes, got {4 * words.size}")
        self._decay = self._validated(words.view(np.float32)[0])
        self.warmup = bool(int(words[1]) & self._WARMUP)


class _TakesParamStats(type):
    """The constructor call of the flat optimizers.  ``param_stats=`` is the one option all three take in the same place
    and the same way, so it is taken HERE, keyword-only by construction, and bound once the subclass's ``__init__`` has
    allocated every buffer (the master copy among them); the ``__init__`` lists themselves stay what callers who pass
    positionally rely on."""

    def __call__(cls, *args, param_stats=None, **kw):
        optimizer = super().__call__(*args, **kw)
        optimizer._bind_param_stats(param_stats)
        return optimizer


class _FlatOptimizer(metaclass=_TakesParamStats):
    """What FlatSGD, FlatAdam and FlatRMSprop share: the parameters moved into ONE flat buffer (their ``.data`` become views of it,
    in the order regularised + others), the gradients read in place when they already sit back to back in that
    order (the fused EPS + head backward allocates them so) and gathered otherwise, and the regulariser's value left
    by the step kernel as one partial sum of squares per workgroup.

    ``master_weights=True`` with bfloat16 parameters adds ``master``: a float32 copy of the flat buffer (initialised
    by exact widening) that the step kernel updates; the bfloat16 parameters then only receive its rounding.  With
    float32 parameters the option changes nothing and ``master`` is None.

    A subclass declares what it keeps, and `state_dict`, `load_state_dict`, `run_host` and `run_restored` are written
    from that once:

    ``_STATE``    the attributes that travel in ``state_dict()`` between ``lr`` and the master copy, in its key order:
                  scalar hyper-parameters and per-element buffers.  One that is None (FlatSGD's ``weight_decay`` left off,
                  FlatRMSprop's ``buf`` without momentum) does not travel.
    ``_MOMENTS``  those of them that are per-element float32 buffers, which ``run_regions()`` lists as well.  The rest
                  are the hyper-parameters: floats, or a tuple of floats (a list in ``run_host()``, whose file is JSON).
    ``_COUNT``    the key of the step count in ``state_dict()``.
    ``_BLOCK_ALWAYS``  whether the step kernel reads rate and count from the 16-byte step block whatever the options;
                  False: only with a schedule, a group table or a weight average, and otherwise the launch takes them from
                  the host (``_state`` is then None).
    ``_READS_RATE``  who, in the words of the refusal to assign ``lr`` during a capture, reads the rate from the device."""

    _STATE: Tuple[str, ...] = ()
    _MOMENTS: Tuple[str, ...] = ()
    _COUNT = "t"
    _BLOCK_ALWAYS = True
    _READS_RATE = "the captured step"

    def __init__(self, regularised, others, num_partials: Callable[[int], int], master_weights: bool = False,
                 guard: Optional["GradGuard"] = None, guard_loss=None, schedule: Optional["LRSchedule"] = None,
                 groups: Optional["ParamGroups"] = None, ema: Optional["WeightEMA"] = None):
        # ema: a WeightEMA that the step kernel updates; bound here, once the master copy exists
        # groups: a ParamGroups table over exactly these parameters that the step kernel obeys
        # guard: a GradGuard whose check runs in front of every step; guard_loss: the float32 device scalar the check
        # looks at beside the gradients, or a callable that returns it (the loss tensor of a training loop is a new one
        # every iteration)
        # schedule: an LRSchedule whose block the step kernel evaluates at the device step count
        self.guard, self.guard_loss = guard, guard_loss
        if schedule is not None and not isinstance(schedule, LRSchedule):
            raise TypeError(f"schedule must be an LRSchedule, got {type(schedule).__name__}")
        self.schedule = schedule
        if ema is not None and not isinstance(ema, WeightEMA):
            raise TypeError(f"ema must be a WeightEMA, got {type(ema).__name__}")
        self.reg_params = [p for p in regularised]
        self.params = self.reg_params + [p for p in others]
        assert self.params and len({p.dtype for p in self.params}) == 1 and len({p.device for p in self.params}) == 1
        ref = self.params[0]
        self.n = sum(p.numel() for p in self.params)
        self.n_reg = sum(p.numel() for p in self.reg_params)
        self.flat = torch.empty(self.n, dtype=ref.dtype, device=ref.device)
        off = 0
        with torch.no_grad():
            for p in self.params:
                view = self.flat[off : off + p.numel()].view_as(p)
                view.copy_(p)
                p.data = view
                off += p.numel()
        # one partial sum of squares per workgroup of the kernel; added up only when the value is asked for
        self.sq_sum = torch.zeros(num_partials(self.n), dtype=torch.float32, device=ref.device)
        self.flat_grad = torch.zeros(self.n, dtype=ref.dtype, device=ref.device)
        self.master: Optional[Tensor] = None
        if master_weights and ref.dtype == torch.bfloat16:
            self.master = self.flat.to(torch.float32)
        if schedule is not None and schedule.device != self.flat.device:
            raise ValueError(f"the schedule's block is on {schedule.device}, the parameters on {self.flat.device}")
        if groups is not None:
            if not isinstance(groups, ParamGroups):
                raise TypeError(f"groups must be a ParamGroups, got {type(groups).__name__}")
            if len(groups.params) != len(self.params) or any(a is not b for a, b in zip(groups.params, self.params)):
                raise ValueError("the ParamGroups table must be built over the optimizer's parameters in flat order "
                                 "(regularised + others)")
            if groups.device != self.flat.device:
                raise ValueError(f"the group table's block is on {groups.device}, the parameters on {self.flat.device}")
            assert L.lib().dctn_param_groups_bytes() == 4 * ParamGroups.WORDS and groups.ends[-1] == self.n
        self.groups = groups
        self.ema = ema
        if ema is not None:
            ema._bind(self)
        self.param_stats = None   # set by the constructor call (`_TakesParamStats`)

    def _bind_param_stats(self, param_stats) -> None:
        """``param_stats``: a `param_stats.ParamStats` whose record every ``step()`` ends with, or None.  It gets the
        segments' sizes here: one per parameter, in flat order."""
        if param_stats is not None:
            from .param_stats import ParamStats

            if not isinstance(param_stats, ParamStats):
                raise TypeError(f"param_stats must be a ParamStats, got {type(param_stats).__name__}")
            if len(self.params) > ParamGroups.MAX_SEGMENTS:
                raise NotImplementedError(f"param_stats: at most {ParamGroups.MAX_SEGMENTS} parameters (one segment each), "
                                          f"got {len(self.params)}")
            if len(param_stats.names) != len(self.params):
                raise ValueError(f"the monitor holds {len(param_stats.names)} names, the optimizer {len(self.params)} "
                                 "parameters: one name per parameter, in flat order (regularised + others)")
            if param_stats.device != self.flat.device:
                raise ValueError(f"the monitor's block is on {param_stats.device}, the parameters on {self.flat.device}")
            param_stats.bind([p.numel() for p in self.params])
        self.param_stats = param_stats

    def _finish_init(self, lr: float, what: str) -> None:
        """A subclass's constructor ends here, its hyper-parameters set and its buffers allocated."""
        self._own_step_block(lr)
        if self.groups is not None:
            self.groups._bind(self.weight_decay, type(self).__name__)
        self._describe(what)

    def _own_step_block(self, lr: float) -> None:
        """Allocates the step block {int32 steps_done, float32 lr, uint32 ticket, uint32 reserved} (include/dctn_amd.h)
        where the step kernel reads one, and sets the rate: in the block's cell, or, for a launch that takes it from the
        host, in ``_lr`` alone."""
        self._state: Optional[Tensor] = None
        if self._BLOCK_ALWAYS or self.schedule is not None or self.groups is not None or self.ema is not None:
            assert L.lib().dctn_adam_state_bytes() == 16
            self._state = torch.zeros(4, dtype=torch.int32, device=self.flat.device)
            self._lr_cell = self._state.view(torch.float32)[1:2]
        if self.schedule is None:
            self.lr = lr
        else:   # the block's rate cell is the kernel's to write: the rate of the step just taken
            self._lr = float(lr)
            assert L.lib().dctn_lr_schedule_bytes() == 4 * LRSchedule.WORDS

    @property
    def lr(self) -> float:
        """Without a schedule the host copy of the rate (what the next launch gets, or what the block's cell holds); with
        one, ``schedule.value(t)`` (reads the device)."""
        return self._lr if self.schedule is None else self._scheduled_lr()

    @lr.setter
    def lr(self, value: float) -> None:
        if self.schedule is not None:
            self._refuse_lr()
        if self._state is not None:   # the step reads the rate from the block: a tiny asynchronous write
            _refuse_capture(self.flat.device, f"{type(self).__name__}.lr cannot be assigned during a graph capture: "
                                              f"{self._READS_RATE} reads the rate from the device, assign it between replays")
            _write_cell(self._lr_cell, float(value))
        self._lr = float(value)

    @property
    def t(self) -> int:
        """Number of steps taken: read from the step block where there is one (it synchronises; steps the guard skipped
        do not count), otherwise the host's count of launches."""
        return self._steps if self._state is None else int(self._state[0].item())

    def _scheduled_lr(self) -> float:
        """``schedule.value(t)``, scale applied: the rate of the next step (reads the step count from the device)."""
        return self.schedule.value(self.t)

    def _refuse_lr(self):
        raise RuntimeError(f"{type(self).__name__}.lr cannot be assigned with a schedule: the step kernel evaluates the "
                           "schedule's table on the device; change the table with schedule.set(...) or multiply every "
                           "rate with schedule.scale = ...")

    def refresh_master(self) -> None:
        """Rebuilds the float32 master copy from the current bfloat16 parameters (nothing to do without one).  Call it
        after anything wrote the parameters behind the optimizer's back - ``model.load_state_dict``,
        ``ddp.broadcast_parameters`` - or the next step starts from the values the master held before.  A `WeightEMA`
        goes on averaging from the old weights: ``ema.reset()`` starts it again from the new ones."""
        if self.master is not None:
            with torch.no_grad():
                self.master.copy_(self.flat)

    def _load_master(self, state: Dict[str, Any]) -> None:
        if self.master is None:
            return
        saved = state.get("master")
        if saved is None:   # a state written without the option: the parameters are all there is
            self.refresh_master()
            return
        if saved.numel() != self.n:
            raise ValueError(f"optimizer state holds {saved.numel()} master values, the parameters {self.n}")
        with torch.no_grad():
            self.master.copy_(saved.reshape(-1))

    def _load_ema(self, state: Dict[str, Any]) -> None:
        """After the parameters' and the master's values are in place: the saved average, or a fresh one from them."""
        if self.ema is None:
            return
        saved = state.get("ema")
        if saved is None:   # a state written without the option
            self.ema.reset()
        else:
            self.ema.load_state_dict(saved)

    def _hyper(self):
        """The names of the hyper-parameters this optimizer has, in ``_STATE``'s order."""
        return [k for k in self._STATE if k not in self._MOMENTS and getattr(self, k) is not None]

    def _set_hyper(self, values: Dict[str, Any]) -> None:
        for k in self._hyper():
            v = values[k]
            setattr(self, k, tuple(float(x) for x in v) if isinstance(v, (tuple, list)) else float(v))

    def state_dict(self) -> Dict[str, Any]:
        """Everything a resumed run needs besides the parameters themselves (those are the model's state_dict)."""
        state = {self._COUNT: self.t, "lr": self.lr}
        for k in self._STATE:
            v = getattr(self, k)
            if v is not None:
                state[k] = v.clone() if k in self._MOMENTS else v
        if self.master is not None:
            state["master"] = self.master.clone()
        if self.ema is not None:
            state["ema"] = self.ema.state_dict()
        return state

    def _check_state(self, state: Dict[str, Any]) -> None:
        """Refuses a state that does not fit this optimizer, before anything of it is taken."""
        if any(state[k].numel() != self.n for k in self._MOMENTS):
            raise ValueError(f"optimizer state holds {state[self._MOMENTS[0]].numel()} values, the parameters {self.n}")

    def load_state_dict(self, state: Dict[str, Any]) -> None:
        self._check_state(state)
        self._set_hyper(state)
        with torch.no_grad():
            for k in self._MOMENTS:
                getattr(self, k).copy_(state[k].reshape(-1))
        if self.schedule is None:
            self.lr = state["lr"]
        if self._state is not None:   # the block as the kernel would have left it: the count, and the rate of the last step
            self._put_step_block(int(state[self._COUNT]))
        self._load_master(state)
        self._load_ema(state)

    def zero_grad(self, set_to_none: bool = True) -> None:
        for p in self.params:
            if set_to_none:
                p.grad = None
            elif p.grad is not None:
                p.grad.zero_()

    def _grads(self) -> Tensor:
        grads = [p.grad for p in self.params]
        base, off, st = None, 0, None
        ok = all(g is not None and g.is_contiguous() for g in grads)
        if ok:
            g0 = grads[0]
            base, st = g0.data_ptr(), g0.untyped_storage()
            for g in grads:
                if g.untyped_storage().data_ptr() != st.data_ptr() or g.data_ptr() != base + off * g.element_size():
                    ok = False
                    break
                off += g.numel()
        if ok:
            return grads[0].new_empty(0).set_(st, grads[0].storage_offset(), (self.n,), (1,))
        torch.cat([(g if g is not None else torch.zeros_like(p)).reshape(-1) for g, p in zip(grads, self.params)],
                  out=self.flat_grad)
        return self.flat_grad

    def _describe(self, what: str) -> None:
        """Builds the step's descriptor (dctn_flat_step_t, include/dctn_amd.h) once, when the subclass has allocated its
        buffers: every pointer in it - ``flat``, ``master``, ``sq_sum``, the step block, the guard, schedule and group
        blocks - is stable for the optimizer's life.  An option that is off is NULL.  ``what`` names the call, with the
        active options, in the message of a failed check."""
        assert L.lib().dctn_flat_step_bytes() == ctypes.sizeof(L.FlatStep)
        blocks = {"master weights": self.master, "guard": None if self.guard is None else self.guard._block,
                  "schedule": None if self.schedule is None else self.schedule._block,
                  "groups": None if self.groups is None else self.groups._block,
                  "weight average": None if self.ema is None else self.ema._block}
        ptr = {name: None if t is None else t.data_ptr() for name, t in blocks.items()}
        self._desc = L.FlatStep(params=self.flat.data_ptr(), master=ptr["master weights"], grads=None,
                                sq_sum=self.sq_sum.data_ptr(),
                                state=None if self._state is None else self._state.data_ptr(), guard=ptr["guard"],
                                schedule=ptr["schedule"], groups=ptr["groups"], n=self.n, n_reg=self.n_reg, l2=self.l2,
                                dtype=L.dtype_code(self.flat))
        self._desc_ref = ctypes.byref(self._desc)
        self._ema_ref = None if self.ema is None else self.ema._desc_ref   # dctn_weight_ema_t, built when it was bound
        on = [name for name, p in ptr.items() if p is not None]
        self._what = what + (f" ({', '.join(on)})" if on else "")

    def _begin_step(self) -> Tensor:
        """What changes from one step to the next goes into the descriptor - where the gradients lie, and ``n_reg`` and
        ``l2``, plain attributes a caller may have assigned - and the guard's check is launched in front of the step.
        Returns the gradients' buffer for `_end_step`."""
        if self.ema is not None:
            self.ema._refuse_applied(f"{type(self).__name__}.step()")
        g = self._grads()
        d = self._desc
        d.grads, d.n_reg, d.l2 = g.data_ptr(), self.n_reg, self.l2
        if self.guard is not None:
            self.guard.check(g, self.guard_loss() if callable(self.guard_loss) else self.guard_loss)
        return g

    def _end_step(self, g: Tensor) -> None:
        """Behind the step launch: the monitor's record, when there is one, of the weights the step just wrote (the master
        copy where there is one) and of the gradients it read - as they stand in the buffer, before the guard's
        coefficient.  A step the guard skipped is recorded too: its weights are simply unchanged."""
        if self.param_stats is not None:
            self.param_stats.record(self.flat, self.master, g)

    def _put_step_block(self, steps: int) -> None:
        """Writes the 16-byte step block: ``steps`` taken, the rate of the last of them."""
        host = torch.zeros(4, dtype=torch.int32)
        host[0] = int(steps)
        if self.schedule is None:   # the rate the host set
            host.view(torch.float32)[1] = self._lr
        else:
            host.view(torch.float32)[1] = self.schedule.value(steps - 1) if steps > 0 else 0.0
        with torch.no_grad():
            self._state.copy_(host)

    def reg_value(self) -> Tensor:
        """l2 * sum of squared Frobenius norms of the regularised parameters, as of the last step."""
        return self.sq_sum.sum() * self.l2

    # A part of a run, as `GradGuard`.  `_MOMENTS` names the subclass's per-element buffers; `run_host()` is the
    # dictionary of its hyper-parameters (`_lr`: the host copy - with a schedule the rate is in the blocks, and reading
    # `lr` would synchronise), and `run_restored()` sets them again.
    def run_regions(self):
        """In file order.  The schedule's block stands in front of the step block, so that a file and a run that disagree
        about the schedule differ at that entry first; the group table's block, the segments' step counts in it, follows
        it.  ``state``: FlatAdam; a FlatSGD with a schedule, a group table or an average.  A `WeightEMA`'s values and block
        stand behind the master copy."""
        regions = [("flat", self.flat)] + [(name, getattr(self, name)) for name in self._MOMENTS]
        if self.master is not None:
            regions.append(("master", self.master))
        for part in (self.ema, self.schedule, self.groups):
            if part is not None:
                regions += part.run_regions()
        if self._state is not None:
            regions.append(("state", self._state))
        regions.append(("sq_sum", self.sq_sum))
        if self.param_stats is not None:   # behind everything a run without a monitor writes
            regions += self.param_stats.run_regions()
        return regions

    def run_host(self) -> Dict[str, Any]:
        host = dict(kind=type(self).__name__, lr=self._lr)
        for k in self._hyper():
            v = getattr(self, k)
            host[k] = list(v) if isinstance(v, tuple) else v
        if self.param_stats is not None:
            host["param_stats"] = self.param_stats.run_host()
        return host

    def run_check(self, host: Dict[str, Any]) -> None:
        if host["kind"] != type(self).__name__:
            raise ValueError(f"snapshot: entry 'optimizer' is {host['kind']} in the file, {type(self).__name__} in the run")

    def run_restored(self, host: Dict[str, Any], blocks) -> None:
        """The blocks came back - the rate itself with the 16-byte block: the host scalars follow the file's, and the host
        copies of the average's, the schedule's and the group table's follow their blocks."""
        self._lr = float(host["lr"])
        self._set_hyper(host)
        for part in (self.ema, self.schedule, self.groups):
            if part is not None:
                part.run_restored(None, {name: blocks[name] for name, _ in part.run_regions()})
        if self.param_stats is not None:
            self.param_stats.run_restored(host.get("param_stats"), {name: blocks[name] for name, _ in
                                                                    self.param_stats.run_regions()})


class FlatSGD(_FlatOptimizer):
    """SGD with momentum plus the reference's L2 regulariser, as ONE kernel per step over one flat
    parameter buffer.  ``step()`` makes one library call whatever the options, `dctn_sgd_flat_step` with a descriptor of
    the step built at construction; alone it launches the kernel of `dctn_sgd_l2_step`, and each option below names the
    older entry point that launches the same kernel as that option does here.

    ``regularised``: the parameters whose squared Frobenius norms the regulariser sums (for
    EPSesPlusLinear.epswise_l2_regularizer: every core and ``linear.weight``,
    dctn/eps_plus_linear.py:149-153); ``others``: the rest (``linear.bias``).  Adding
    ``l2 * sum ||w||^2`` to the loss and letting autograd differentiate it is the same update as adding
    ``2 * l2 * w`` to the gradient, which is what the kernel does; ``reg_value()`` returns the term's
    value (before the update) for logging.  The parameters are moved into one buffer (their ``.data``
    become views of it, in the order regularised + others); when the gradients already sit back to back
    in that order (the fused EPS + head backward allocates them so) the step reads them in place,
    otherwise they are gathered first.  Semantics of torch.optim.SGD(momentum, dampening = 0).

    ``master_weights=True``: bfloat16 parameters get a float32 master copy that the kernel updates
    (the kernel of `dctn_sgd_l2_step_master`); an update below half an ulp of the bfloat16 value is then kept instead of rounded
    away.  ``state_dict()`` / ``load_state_dict()`` carry the momentum buffer, the step count, the hyper-parameters
    and the master copy.

    ``guard`` (a `GradGuard`) / ``guard_loss``: ``step()`` launches the guard's check and then the guarded kernel
    (that of `dctn_sgd_l2_step_guarded`): gradients clipped to ``guard.max_norm`` in front of the ``2 * l2 * w`` term, and no
    write at all once the guard has halted.  Without a guard ``step()`` makes the calls it always made.

    ``schedule`` (an `LRSchedule`): ``step()`` launches the kernel of `dctn_sgd_l2_step_scheduled` (behind the guard's check
    when there is a guard).  The optimizer then owns a 16-byte DEVICE block {steps_done, lr, ticket, reserved} - `FlatAdam`'s - that
    the launch advances: the rate is the schedule's value at ``steps_done`` and the first step is ``steps_done == 0``,
    both read on the device, so a captured step changes its rate from replay to replay (without a schedule a captured
    step replays the ``lr`` and ``first_step`` it was captured with).  ``opt.lr`` returns ``schedule.value(opt.t)``;
    assigning it raises RuntimeError (``schedule.set`` / ``schedule.scale`` change the rate); the ``lr`` argument is
    not used.  The schedule object is fixed for the life of a captured graph; its table and scale may change between
    replays.  ``opt.t`` and ``state_dict()["steps"]`` are read from the block.  Without a schedule ``step()`` makes
    the calls it always made.

    ``groups`` (a `ParamGroups` over exactly these parameters): ``step()`` launches the kernel of
    `dctn_sgd_l2_step_grouped` (behind the guard's check when there is a guard): every parameter steps with ``rate * lr_scale`` of its segment, takes its
    first step when ITS count is 0, and is left alone while frozen.  The optimizer then owns the 16-byte step block
    whether or not there is a schedule: without one ``opt.lr = x`` writes the block's rate cell (not during a capture),
    and a captured step follows it.  ``opt.t`` stays the global count.  Without the ``weight_decay`` option a `ParamGroup`
    for this optimizer leaves ``weight_decay=None`` (ValueError otherwise).  The table's state is not part of ``state_dict()``; save
    ``groups.state_dict()`` beside it (`checkpoint.RunState` carries its block).  Without ``groups`` ``step()`` makes
    the calls it always made.

    ``ema`` (a `WeightEMA`): ``step()`` calls `dctn_sgd_flat_step_ema`, and the one launch also moves the average of every
    element it stores to, from the value the optimizer keeps for it.  The optimizer then owns the 16-byte step block, as
    with a group table: the rate and the first step are read on the device, and ``opt.lr = x`` writes the block's rate
    cell.  ``state_dict()`` holds the average under ``"ema"``.  Without ``ema`` ``step()`` makes the calls it always made.

    ``weight_decay`` (a float >= 0, ``0.0`` included): torch.optim.SGD's coupled weight decay,
    ``g += weight_decay * w`` in front of the ``2 * l2 * w`` term and the momentum (behind the guard's clip).  ``step()``
    then calls `dctn_sgd_flat_step_decay` whatever the other options; a `ParamGroups` table is bound with this value as
    its default, and a `ParamGroup` may name its own.  ``state_dict()`` and ``run_host()`` carry it under
    ``"weight_decay"``.  ``None`` (the default): the optimizer has no weight decay, refuses a table that names one, and
    ``step()`` makes the calls it always made.

    ``param_stats`` (a `param_stats.ParamStats`): `FlatAdam`'s option - every ``step()`` ends with the monitor's record of
    the weights it wrote and the gradients it read.  Without it ``step()`` makes the calls it always made.
    """

    def __init__(self, regularised, others=(), lr: float = 1e-3, momentum: float = 0.0, l2: float = 0.0,
                 master_weights: bool = False, guard: Optional["GradGuard"] = None, guard_loss=None, *,
                 schedule: Optional["LRSchedule"] = None, groups: Optional["ParamGroups"] = None,
                 ema: Optional["WeightEMA"] = None, weight_decay: Optional[float] = None):
        super().__init__(regularised, others, L.lib().dctn_sgd_l2_num_partials, master_weights, guard, guard_loss,
                         schedule, groups, ema)
        self.momentum, self.l2 = float(momentum), float(l2)
        if weight_decay is not None and not float(weight_decay) >= 0.0:
            raise ValueError(f"invalid SGD weight_decay: {weight_decay}")
        self.weight_decay: Optional[float] = None if weight_decay is None else float(weight_decay)
        self.buf = torch.zeros(self.n, dtype=torch.float32, device=self.flat.device)
        self._steps = 0   # the host's count of launches: `t`, and the step's `first_step`, where there is no step block
        self._finish_init(lr, "fused SGD step")

    _STATE = ("momentum", "l2", "buf", "weight_decay")
    _MOMENTS = ("buf",)
    _COUNT = "steps"
    _BLOCK_ALWAYS = False
    _READS_RATE = "the captured step of an optimizer with a group table or a weight average"

    @torch.no_grad()
    def step(self) -> None:
        g = self._begin_step()
        # Without a schedule or a group table the launch takes the rate and `first` from the host.  `first` is the host's
        # count of launches, and under a guard the host does not know whether the guard let a launch through.  A skipped
        # step 0 leaves the momentum buffer at its zeros, and the next launch, with first = 0, forms momentum * 0 + g = g:
        # the update a first step makes.  (With either option the kernel reads both from the step block instead.)
        if self.weight_decay is not None:
            L.check(L.lib().dctn_sgd_flat_step_decay(self._desc_ref, self._ema_ref, self.buf.data_ptr(), self._lr,
                                                     self.momentum, self.weight_decay, 1 if self._steps == 0 else 0,
                                                     L.stream_ptr(self.flat.device)), self._what)
        elif self._ema_ref is None:
            L.check(L.lib().dctn_sgd_flat_step(self._desc_ref, self.buf.data_ptr(), self._lr, self.momentum,
                                               1 if self._steps == 0 else 0, L.stream_ptr(self.flat.device)), self._what)
        else:
            L.check(L.lib().dctn_sgd_flat_step_ema(self._desc_ref, self._ema_ref, self.buf.data_ptr(), self._lr,
                                                   self.momentum, 1 if self._steps == 0 else 0,
                                                   L.stream_ptr(self.flat.device)), self._what)
        self._steps += 1
        self._end_step(g)

    def _with_own_decay(self, values: Dict[str, Any]) -> Dict[str, Any]:
        """(a state written without the ``weight_decay`` option keeps this optimizer's value)"""
        return values if self.weight_decay is None else {"weight_decay": self.weight_decay, **values}

    def load_state_dict(self, state: Dict[str, Any]) -> None:
        super().load_state_dict(self._with_own_decay(state))
        self._steps = int(state["steps"])

    def run_host(self) -> Dict[str, Any]:
        host = super().run_host()
        decay = host.pop("weight_decay", None)   # the count stands in front of it
        host["steps"] = self._steps
        return host if decay is None else dict(host, weight_decay=decay)

    def run_restored(self, host: Dict[str, Any], blocks) -> None:
        self._steps = int(host["steps"])
        super().run_restored(self._with_own_decay(host), blocks)


class FlatAdam(_FlatOptimizer):
    """torch.optim.Adam (coupled ``weight_decay``, no amsgrad - what the reference's recipe builds,
    new_runner.py:496-498) plus the reference's L2 regulariser, as ONE kernel per step over one flat parameter
    buffer.  ``step()`` makes one library call whatever the options, `dctn_adam_flat_step` with a descriptor of the step
    built at construction; alone it launches the kernel of `dctn_adam_l2_step`, and each option below names the older
    entry point that launches the same kernel as that option does here.  Construction, gradient handling and ``reg_value()`` are FlatSGD's; the moments
    ``m`` / ``v`` are float32 whatever the parameter dtype.

    The step count ``t`` and the learning rate live in a small DEVICE block that the kernel reads and whose ``t`` the
    same launch advances: a `GraphedTrainStep` that captured ``step()`` gets t, t+1, ... on its replays, and
    assigning ``opt.lr`` (a tiny asynchronous write on the current stream; not allowed during a capture) changes the
    rate of every later step, replays of an already captured graph included.  Reading ``opt.lr`` returns the host
    copy; ``opt.t`` reads the device (it synchronises).  ``state_dict()`` / ``load_state_dict()`` carry t, lr, m, v,
    the hyper-parameters and the master copy when there is one: a run resumed from them continues bit-identically.

    ``master_weights=True``: bfloat16 parameters get a float32 master copy ``master`` that the same launch updates
    (the kernel of `dctn_adam_l2_step_master`); the parameters receive its rounding and are never read by the step.  Without it a
    bfloat16 weight whose Adam step (about ``lr``) is below half an ulp of its value does not move at all.  The
    master follows, bit for bit, what FlatAdam does on float32 parameters given the same gradients.  Call
    ``refresh_master()`` after writing the parameters from outside.

    ``guard`` (a `GradGuard`) / ``guard_loss`` (a float32 device scalar, or a callable returning one): ``step()``
    launches the guard's check over the gradients and then the guarded kernel (that of `dctn_adam_l2_step_guarded`;
    two launches instead of one).  The gradients are clipped to ``guard.max_norm`` as they stand in the buffer - after the
    all-reduce, in front of ``weight_decay * w`` and the fused ``2 * l2 * w``: ``clip_grad_norm_`` followed by
    ``Adam(weight_decay=...)``; a regulariser passed through ``reg_fn`` is in the buffer and is clipped with it.  Once
    the guard has halted, a step writes nothing: parameters, ``m``, ``v``, ``master`` and ``t`` stay as they are.  The
    guard's state is not part of this optimizer's ``state_dict()``; save ``guard.state_dict()`` beside it.  Without a
    guard ``step()`` makes the calls it always made.

    ``schedule`` (an `LRSchedule`): ``step()`` launches the kernel of `dctn_adam_l2_step_scheduled` (behind the guard's
    check when there is a guard): the kernel evaluates the schedule's table at the device step count instead of reading the
    block's rate, and leaves the rate it used in the block, so `StepTrace` records the rate of every iteration.  Every
    replay of a captured step, and each of the K iterations of one launch, gets its own rate with no host write.
    ``opt.lr`` returns ``schedule.value(opt.t)`` (it reads the device); assigning it raises RuntimeError
    (``schedule.set`` / ``schedule.scale`` change the rate); the ``lr`` argument is not used.  A step the guard skipped
    does not advance ``t``, so the schedule holds its place.  The schedule object is fixed for the life of a captured
    graph; its table and scale may change between replays.  The schedule's state is not part of ``state_dict()``; save
    ``schedule.state_dict()`` beside it (`checkpoint.RunState` carries its block).  Without a schedule ``step()``
    makes the calls it always made.

    ``groups`` (a `ParamGroups` over exactly these parameters): ``step()`` launches the kernel of
    `dctn_adam_l2_step_grouped` (behind the guard's check when there is a guard, with the schedule when there is one): ``torch.optim.Adam`` with
    ``param_groups`` and parameters without a gradient, in the one launch.  Every parameter steps with
    ``rate * lr_scale`` and the weight decay of its segment, its bias corrections follow ITS count of steps, and a frozen
    parameter is left alone - value, master copy, moments and count; a gradient of None is fine - while its squares
    still count in ``reg_value()``.  ``opt.t`` stays the global count; ``groups.steps`` reads the segments'.  A clipped
    step clips every unfrozen segment by the one coefficient: the guard's norm, like the all-reduce, covers the whole
    flat buffer, frozen segments included.  The table's state is not part of ``state_dict()``; save
    ``groups.state_dict()`` beside it (`checkpoint.RunState` carries its block).  Without ``groups`` ``step()`` makes
    the calls it always made.

    ``ema`` (a `WeightEMA`): ``step()`` calls `dctn_adam_flat_step_ema`, and the one launch also moves the average of
    every element it stores to, from the value the optimizer keeps for it - the master value where there is one.  A step
    the guard skipped and a frozen segment leave their averages alone; every other buffer holds the bits it would hold
    without the average.  ``state_dict()`` holds the average under ``"ema"``; a state without one resets it from the
    parameters.  Without ``ema`` ``step()`` makes the calls it always made.

    ``param_stats`` (keyword only, taken by the constructor call of all three flat optimizers and bound behind
    ``__init__``; a `param_stats.ParamStats` with one name per parameter, in flat order): every ``step()`` ends with one
    more launch, `dctn_param_stats`, behind the step: sum, sum of squares, largest magnitude and non-finite count of every
    parameter as the step left it - the master copy where there is one - and of its gradient as it stands in the buffer
    the step read, before the guard's coefficient.  A step the guard skipped is recorded too.  A captured ``step()``
    carries the record, so each of the K iterations of one launch leaves its row.  No other buffer changes a bit.
    Without ``param_stats`` ``step()`` makes the calls it always made.
    """

    def __init__(self, regularised, others=(), lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 0.0, l2: float = 0.0, master_weights: bool = False,
                 guard: Optional["GradGuard"] = None, guard_loss=None, *, schedule: Optional["LRSchedule"] = None,
                 groups: Optional["ParamGroups"] = None, ema: Optional["WeightEMA"] = None):
        super().__init__(regularised, others, L.lib().dctn_adam_l2_num_partials, master_weights, guard, guard_loss,
                         schedule, groups, ema)
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0 and lr >= 0.0 and eps >= 0.0 and weight_decay >= 0.0):
            raise ValueError(f"invalid Adam hyper-parameters: lr={lr} betas={betas} eps={eps} weight_decay={weight_decay}")
        self.betas, self.eps = (float(betas[0]), float(betas[1])), float(eps)
        self.weight_decay, self.l2 = float(weight_decay), float(l2)
        dev = self.flat.device
        self.m = torch.zeros(self.n, dtype=torch.float32, device=dev)
        self.v = torch.zeros(self.n, dtype=torch.float32, device=dev)
        self._finish_init(lr, "fused Adam step")

    _STATE = ("m", "v", "betas", "eps", "weight_decay", "l2")
    _MOMENTS = ("m", "v")

    @torch.no_grad()
    def step(self) -> None:
        g = self._begin_step()
        # (with a group table every segment's weight decay is in the table, and the launch ignores this one)
        if self._ema_ref is None:
            L.check(L.lib().dctn_adam_flat_step(self._desc_ref, self.m.data_ptr(), self.v.data_ptr(), self.betas[0],
                                                self.betas[1], self.eps, self.weight_decay, L.stream_ptr(self.flat.device)),
                    self._what)
        else:
            L.check(L.lib().dctn_adam_flat_step_ema(self._desc_ref, self._ema_ref, self.m.data_ptr(), self.v.data_ptr(),
                                                    self.betas[0], self.betas[1], self.eps, self.weight_decay,
                                                    L.stream_ptr(self.flat.device)), self._what)
        self._end_step(g)


class FlatRMSprop(_FlatOptimizer):
    """torch.optim.RMSprop (coupled ``weight_decay``, optional ``momentum``, not centered - what the reference's
    classifier script builds, mnist.py:466-476) plus the reference's L2 regulariser, as ONE kernel per step over one
    flat parameter buffer: ``step()`` makes one library call, `dctn_rmsprop_flat_step`, whatever the options.
    Construction, gradient handling and ``reg_value()`` are FlatSGD's; ``square_avg`` is float32 whatever the parameter
    dtype, and so is the momentum buffer ``buf``, which exists only with ``momentum > 0`` (fixed at construction: without
    it the launch moves nothing for a buffer).  Both start from zeros, as torch's, so there is no first-step case.

    The step count and the learning rate live in `FlatAdam`'s 16-byte DEVICE block, with its behaviour: the launch
    advances the count, a captured ``step()`` follows ``opt.lr = x`` assigned between replays, ``opt.t`` reads the device.
    ``master_weights``, ``guard`` / ``guard_loss``, ``schedule``, ``groups``, ``ema`` and ``param_stats`` are `FlatAdam`'s options with its
    semantics (a segment of a group table has no bias correction to keep: it steps with ``rate * lr_scale`` and its own
    weight decay, and its count only advances).  ``state_dict()`` / ``load_state_dict()`` carry t, lr, the buffers, the
    hyper-parameters, the master copy and the average: a run resumed from them continues bit-identically.
    ``centered=True`` is not offered.
    """

    def __init__(self, regularised, others=(), lr: float = 1e-2, alpha: float = 0.99, eps: float = 1e-8,
                 weight_decay: float = 0.0, momentum: float = 0.0, l2: float = 0.0, master_weights: bool = False,
                 guard: Optional["GradGuard"] = None, guard_loss=None, *, schedule: Optional["LRSchedule"] = None,
                 groups: Optional["ParamGroups"] = None, ema: Optional["WeightEMA"] = None):
        super().__init__(regularised, others, L.lib().dctn_rmsprop_num_partials, master_weights, guard, guard_loss,
                         schedule, groups, ema)
        if not (0.0 <= alpha < 1.0 and lr >= 0.0 and eps >= 0.0 and weight_decay >= 0.0 and momentum >= 0.0):
            raise ValueError(f"invalid RMSprop hyper-parameters: lr={lr} alpha={alpha} eps={eps} "
                             f"weight_decay={weight_decay} momentum={momentum}")
        self.alpha, self.eps, self.momentum = float(alpha), float(eps), float(momentum)
        self.weight_decay, self.l2 = float(weight_decay), float(l2)
        dev = self.flat.device
        self.square_avg = torch.zeros(self.n, dtype=torch.float32, device=dev)
        self.buf: Optional[Tensor] = torch.zeros(self.n, dtype=torch.float32, device=dev) if self.momentum > 0.0 else None
        self._MOMENTS = ("square_avg",) if self.buf is None else ("square_avg", "buf")
        self._finish_init(lr, "fused RMSprop step")

    _STATE = ("square_avg", "alpha", "eps", "weight_decay", "momentum", "l2", "buf")   # (`_MOMENTS`: per instance)

    @torch.no_grad()
    def step(self) -> None:
        g = self._begin_step()
        # (with a group table every segment's weight decay is in the table, and the launch ignores this one)
        L.check(L.lib().dctn_rmsprop_flat_step(self._desc_ref, self._ema_ref, self.square_avg.data_ptr(),
                                               None if self.buf is None else self.buf.data_ptr(), self.alpha, self.eps,
                                               self.weight_decay, self.momentum, L.stream_ptr(self.flat.device)),
                self._what)
        self._end_step(g)

    def _same_momentum(self, saved, complaint: str) -> None:
        if (float(saved) > 0.0) != (self.buf is not None):
            raise ValueError(complaint.format(saved, self.momentum))

    def _check_state(self, state: Dict[str, Any]) -> None:
        if state["square_avg"].numel() == self.n:   # (a wrong size is refused first, below)
            self._same_momentum(state["momentum"], "optimizer state was written with momentum {}, this optimizer was built "
                                "with {}: the momentum buffer exists from construction or not at all")
        super()._check_state(state)

    def run_restored(self, host: Dict[str, Any], blocks) -> None:
        self._same_momentum(host["momentum"], "snapshot: the optimizer was saved with momentum {}, the run's was built "
                            "with {}")
        super().run_restored(host, blocks)


# ------------------------------------------------------------------------------------------------
# The reference's training loop and its hooks (dctn/training.py:14-248), one process per GPU
# ------------------------------------------------------------------------------------------------
def _world() -> int:
    return dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1


def batches_forever(dl: Iterable) -> Iterator[Any]:
    """Cycles through ``dl`` again and again (a new pass — a new shuffle — each time it runs out)."""
    while True:
        for batch in dl:
            yield batch


def train(dl, model, optimizer, dev, loss_fn, reg_fn, reg_coeff: float, at_iter_start, after_back,
          after_param_upd, first_iter: int = 0) -> Tuple[StX, StIt]:
    """The loop of dctn/training.py:23-84.  ``dl`` yields ``(x, y, indices)`` (this rank's shard under
    ``torch.distributed``); ``loss_fn(output, y)`` and ``reg_fn(st_x, st_it)`` return 0-dim tensors; the three
    hook lists hold callables ``f(st_x, st_it)`` run at the start of an iteration, after ``backward()`` (the
    gradients they see are already averaged over the ranks) and after ``optimizer.step()``.  A hook stops
    the loop by setting ``st_it["stop"]``; with several ranks the flag is OR-ed over them so that all
    leave in the same iteration.  Returns the two state dictionaries of the last iteration.

    ``first_iter``: ``num_iters_done`` counts from it, so the schedules of the hooks and the checkpoint names of a run
    resumed from a snapshot (`checkpoint.RunState.load`, whose extras hold the last finished iteration) continue where
    the saved run stood.  The default, 0, is a run from the start."""
    st_x: StX = dict(model=model.to(dev), optimizer=optimizer, loss_fn=loss_fn, reg_fn=reg_fn, reg_coeff=reg_coeff,
                     at_iter_start=list(at_iter_start), after_back=list(after_back),
                     after_param_upd=list(after_param_upd), dev=dev)
    world = _world()
    reducer = None
    if world > 1:
        # the reference is one process with one seed; here every rank drew its own random parameters, and averaged
        # gradients on different models would diverge silently: everybody starts from rank 0's model
        ddp.broadcast_parameters(list(st_x["model"].parameters()) + list(st_x["model"].buffers()))
        if hasattr(st_x["model"], "_refresh_p"):
            st_x["model"]._refresh_p()
        # the optimizer was built before this broadcast: a float32 master copy of the parameters (FlatAdam / FlatSGD
        # with master_weights) still holds this rank's own initialisation
        if getattr(optimizer, "refresh_master", None) is not None:
            optimizer.refresh_master()
        reducer = ddp.FlatGradAllReducer(st_x["model"].parameters(), average=True)
    st_it: StIt = {}

    def run_hooks(key: str) -> None:
        for hook in tuple(st_x[key]):   # a hook may remove itself
            hook(st_x, st_it)

    for count, (x, y, indices) in enumerate(batches_forever(dl), int(first_iter)):
        st_it = dict(num_iters_done=count, x=x.to(dev), y=y.to(dev), indices=indices.to(dev), stop=False)
        run_hooks("at_iter_start")
        st_x["model"].train()
        st_it["output"] = st_x["model"](st_it["x"])
        st_it["loss"] = st_x["loss_fn"](st_it["output"], st_it["y"])
        st_it["reg_term"] = st_x["reg_fn"](st_x, st_it)
        st_x["optimizer"].zero_grad()
        (st_it["loss"] + st_it["reg_term"] * st_x["reg_coeff"]).backward()
        if reducer is not None:
            reducer()
        run_hooks("after_back")
        st_x["optimizer"].step()
        run_hooks("after_param_upd")
        if world > 1:
            flag = torch.tensor([1.0 if st_it["stop"] else 0.0], device=dev)
            dist.all_reduce(flag, op=dist.ReduceOp.MAX)
            st_it["stop"] = bool(flag.item() > 0)
        if st_it["stop"]:
            break
    return st_x, st_it


def train_graphed(step: "GraphedTrainStep", n_iters: int, after_launch=(), first_iter: int = 0) -> Tuple[StX, StIt]:
    """The replay-loop counterpart of `train` for a `GraphedTrainStep` built with a ``batch_source``: calls ``step()``
    until ``n_iters`` iterations are done (a launch runs ``step.iters_per_launch`` = K of them, so the last launch may
    overshoot ``n_iters`` by up to K - 1), and after each launch runs the hooks ``f(st_x, st_it)`` of ``after_launch``.
    ``st_it`` holds what the launch returned (``output``, ``loss``, ``reg_term``, ``indices``: the static buffers of its
    LAST iteration), ``stop`` and ``num_iters_done`` = the number of the last finished iteration, counted from
    ``first_iter`` as `train` counts (a run resumed from a snapshot passes ``extras["num_iters_done"] + 1``); ``st_x`` holds
    ``model``, ``optimizer``, ``step`` and ``dev``.  A hook stops the loop by setting ``st_it["stop"]``; with several
    ranks the flag is OR-ed over them, as in `train`.  Returns the two dictionaries of the last launch.

    `checkpoint.RunCheckpointer`, `make_stopper_on_device_halt`, `evaluation.make_evaluation_hook` and
    `make_trace_logger` work unchanged as such hooks.  Hooks run at launch boundaries only and ``num_iters_done``
    advances by K between two calls, so the period of a hook gated with `every_n_iters_intervals` should be a multiple
    of K - any other period never (or irregularly) coincides with a launch boundary."""
    if step.batch_source is None:
        raise ValueError("train_graphed drives a GraphedTrainStep that draws its own batches: build it with a batch_source")
    K = int(step.iters_per_launch)
    dev = step.x.device
    st_x: StX = dict(model=step.model, optimizer=step.optimizer, step=step, dev=dev, after_launch=list(after_launch))
    st_it: StIt = {}
    world = _world()
    done = 0
    while done < int(n_iters):
        out = step()
        done += K
        st_it = dict(out, num_iters_done=int(first_iter) + done - 1, stop=False)
        for hook in tuple(st_x["after_launch"]):   # a hook may remove itself
            hook(st_x, st_it)
        if world > 1:
            flag = torch.tensor([1.0 if st_it["stop"] else 0.0], device=dev)
            dist.all_reduce(flag, op=dist.ReduceOp.MAX)
            st_it["stop"] = bool(flag.item() > 0)
        if st_it["stop"]:
            break
    return st_x, st_it


class _TraceLogger:
    """Hook for `train_graphed`: every ``every`` calls (launches) it reads the trace - the one synchronisation it makes -
    and hands ``sink`` the new records (a `StepTrace.RECORD` array, possibly empty) and the number lost since the last
    read."""

    def __init__(self, trace: "StepTrace", every: int, sink: Callable[..., None]):
        assert every >= 1
        self.trace, self.every, self.sink = trace, int(every), sink
        self._calls = 0

    def __call__(self, st_x: StX, st_it: StIt) -> None:
        self._calls += 1
        if self._calls % self.every == 0:
            self.flush()

    def flush(self) -> None:
        """Reads now (call it when the loop ends, for the launches after the last multiple of ``every``)."""
        records = self.trace.read()
        self.sink(records, self.trace.lost)


def make_trace_logger(trace: "StepTrace", every: int, sink: Callable[..., None]) -> Callable[[StX, StIt], None]:
    """``sink(records, lost)`` is called every ``every`` launches with the records written since the last call.  Choose
    ``trace.capacity >= every * iters_per_launch`` and nothing is lost."""
    return _TraceLogger(trace, every, sink)


def make_histogram_logger(hists, every: int, sink: Callable[..., None]) -> Callable[[StX, StIt], None]:
    """Hook for ``train_graphed(after_launch=[...])``: every ``every`` launches it reads ``hists`` (a
    `tensor_hist.OutputHistograms`: the one synchronisation), calls ``sink(name, summary, num_iters_done)`` per name and
    resets the blocks.  ``summary`` holds the arguments of ``SummaryWriter.add_histogram_raw``: ``min``, ``max``, ``num``,
    ``bucket_limits`` and ``bucket_counts`` are exact, ``sum`` and ``sum_squares`` approximations from the buckets' centres
    (`tensor_hist.histogram_summary`)."""
    from .tensor_hist import HistogramLogger

    return HistogramLogger(hists, every, sink)


def make_tt_stats_logger(tt, every: int, sink: Callable[..., None], first_iter: int = 0) -> Callable[[StX, StIt], None]:
    """Hook for ``train_graphed(after_launch=[...])``: every ``every`` launches it reads ``tt`` (a `tt_stats.TTStats`: the
    one synchronisation) and, for every row not yet read, calls ``sink("mean_of_tt_tensor/" + name, mean, first_iter + call)``
    and ``sink("std_of_tt_tensor/" + name, std, first_iter + call)`` per string - the reference's two tags
    (conv_sbs_statistics_logging.py) in ``add_scalar``'s argument order.  ``flush()`` reads and reports at once.  Give the
    ring ``capacity >= every * iters_per_launch / period`` rows and nothing is lost."""
    from .tt_stats import TTStatsLogger

    return TTStatsLogger(tt, every, sink, first_iter)


def make_param_stats_logger(ps, every: int, sink: Callable[..., None], first_iter: int = 0, weight_tag: str = "weights_norm",
                            grad_tag: str = "grads_norm") -> Callable[[StX, StIt], None]:
    """Hook for ``train_graphed(after_launch=[...])``: every ``every`` launches it reads ``ps`` (a `param_stats.ParamStats`
    held by the optimizer: the one synchronisation) and, for every row not yet read and every parameter, calls
    ``sink(f"{weight_tag}/{name.replace('.', '/')}", norm of the parameter, first_iter + call)`` and
    ``sink(f"{grad_tag}/{name.replace('.', '/')}", norm of its gradient, first_iter + call)``, in ``add_scalar``'s argument
    order.  ``flush()`` reads and reports at once.  The default tags are meant to be what ignite's ``WeightsScalarHandler``
    and ``GradsScalarHandler`` write for ``reduction=torch.norm`` (the reference's add_weights_and_grads_logging,
    mnist.py:535); neither ignite nor the reference's ``libcrap`` was at hand to confirm the spelling, which is why both are
    arguments.  Give the ring ``capacity >= every * iters_per_launch / period`` rows and nothing is lost."""
    from .param_stats import ParamStatsLogger

    return ParamStatsLogger(ps, every, sink, first_iter, weight_tag, grad_tag)


def make_batch_monitor_logger(mon, every: int, scalar_sink: Callable[..., None], histogram_sink=None, sample_sink=None,
                              first_iter: int = 0) -> Callable[[StX, StIt], None]:
    """Hook for ``train_graphed(after_launch=[...])``: every ``every`` launches it reads ``mon`` (the step's
    `batch_monitor.BatchMonitor`: the one synchronisation) and reports every row not yet read with
    ``iteration = first_iter + call``: ``scalar_sink(tag, value, iteration)`` for ``train_input/dumb_mean``,
    ``train_input/dumb_std``, ``train_input_intermediate_output_std_of_coordinates_of_windows/`` and
    ``train_outputs_of_the_whole_model_intermediate_output_dumb_{min,max,mean,std}/`` (the reference's tags,
    mnist.py:298-311 and :555-591; ``add_scalar``'s argument order), ``histogram_sink(tag, summary, iteration)`` for
    ``train_outputs_of_the_whole_model_intermediate_output_logits_as_probabilities/`` with the arguments of
    ``add_histogram_raw`` (`batch_monitor.histogram_summary`), and ``sample_sink(iteration, index, label, pred, p_true)``
    with the four per-sample arrays (new_runner.py:512-531).  ``flush()`` reads and reports at once.  Give the ring
    ``capacity >= every * iters_per_launch / period`` rows and nothing is lost."""
    from .batch_monitor import BatchMonitorLogger

    return BatchMonitorLogger(mon, every, scalar_sink, histogram_sink, sample_sink, first_iter)


def every_n_iters_intervals(*intervals):
    """Decorator factory: ``intervals`` are ``(length, period)`` pairs laid end to end from iteration 0; the
    hook runs when ``num_iters_done`` is a multiple of the period of the interval it falls in.  The last
    length may be ``None`` (forever); otherwise "every iteration" continues after the last interval."""
    spans = list(intervals)
    if spans[-1][0] is not None:
        spans.append((None, 1))
    starts, begin = [], 0
    for length, _ in spans:
        starts.append(begin)
        begin = begin + length if length is not None else begin
    periods = [period for _, period in spans]

    def decorate(func: Callable[[StX, StIt], None]) -> Callable[[StX, StIt], None]:
        def gated(st_x: StX, st_it: StIt) -> None:
            n = st_it["num_iters_done"]
            period = periods[0]
            for start, candidate in zip(starts, periods):
                if n >= start:
                    period = candidate
            if n % period == 0:
                func(st_x, st_it)

        return gated

    return decorate


def _checkpoint_tag(st_it: StIt) -> str:
    """The metric part of the reference's checkpoint names (training.py:135-140,161-166)."""
    return (f"nitd={st_it['num_iters_done']:07}_tracc={st_it['train_acc']:.4f}_vacc={st_it['val_acc']:.4f}_"
            f"trmce={st_it['train_mean_ce']:.4f}_vmce={st_it['val_mean_ce']:.4f}")


class Checkpointer:
    """Writes ``model.state_dict()`` files into ``dir`` — on rank 0 only; the other ranks hold the same
    parameters and skip the file system."""

    def __init__(self, dir: str):
        self.dir = dir

    def save(self, st_x: StX, filename: str) -> None:
        if ddp.is_rank0():
            torch.save(st_x["model"].state_dict(), os.path.join(self.dir, filename))

    def remove_file(self, filename: str) -> None:
        if ddp.is_rank0():
            os.remove(os.path.join(self.dir, filename))


class LastModelsCheckpointer(Checkpointer):
    """One checkpoint per call, the newest ``n`` are kept."""

    def __init__(self, dir: str, n: int):
        super().__init__(dir)
        assert n >= 1
        self.n = n
        self.filenames: deque = deque()

    def __call__(self, st_x: StX, st_it: StIt) -> None:
        name = f"model_{_checkpoint_tag(st_it)}.pth"
        self.save(st_x, name)
        self.filenames.appendleft(name)
        while len(self.filenames) > self.n:
            self.remove_file(self.filenames.pop())


class BestModelCheckpointer(Checkpointer):
    """Keeps the single checkpoint with the best ``st_it[key]`` seen so far."""

    def __init__(self, dir: str, key: str, low_is_good: bool):
        super().__init__(dir)
        self.key, self.low_is_good = key, low_is_good
        self.best_value = float("inf") if low_is_good else float("-inf")
        self.filename: Optional[str] = None

    def __call__(self, st_x: StX, st_it: StIt) -> None:
        value = st_it[self.key]
        better = value < self.best_value if self.low_is_good else value > self.best_value
        if not better:
            return
        name = f"model_best_{self.key}_{_checkpoint_tag(st_it)}.pth"
        self.save(st_x, name)
        self.best_value = value
        if self.filename is not None:
            self.remove_file(self.filename)
        self.filename = name


class ValuesNotImprovingEarlyStopper:
    """Requests a stop once more than ``patience`` consecutive calls brought no improvement of any of the
    watched ``st_it`` values; ``keys`` holds ``(key, low_is_good)`` pairs."""

    def __init__(self, patience: int, keys: Sequence[Tuple[str, bool]]):
        self.patience, self.keys = patience, tuple(keys)
        self.best_values = [float("inf") if low else float("-inf") for _, low in self.keys]
        self.num_bad_calls = 0

    def __call__(self, st_x: StX, st_it: StIt) -> None:
        improved = False
        for slot, (key, low_is_good) in enumerate(self.keys):
            value, best = st_it[key], self.best_values[slot]
            if (value < best) if low_is_good else (value > best):
                self.best_values[slot] = value
                improved = True
        self.num_bad_calls = 0 if improved else self.num_bad_calls + 1
        if self.num_bad_calls > self.patience:
            st_it["stop"] = True
            getLogger(__name__).info(f"Early stopping at st_it['num_iters_done']={st_it['num_iters_done']}")


class _StopAfter:
    """Hook that raises the stop flag from iteration ``n`` on."""

    def __init__(self, n: int):
        self.n = n

    def __call__(self, st_x: StX, st_it: StIt) -> None:
        st_it["stop"] = st_it["stop"] or st_it["num_iters_done"] >= self.n


def make_stopper_after_n_iters(n: int) -> Callable[[StX, StIt], None]:
    return _StopAfter(n)


class _StopOnNonFiniteLoss:
    """Hook for the ``after_back`` list: on a NaN / infinite loss it raises the stop flag and leaves what is needed
    to reproduce the failure - the model's state_dict (named after the iteration, loss and regulariser term) and the
    batch (``x``, ``y``, ``indices``, ``output``) - in ``dir/nan_loss_stop`` (``nan_loss_stop_rank<r>`` when several
    ranks run: every rank that saw a non-finite loss writes its own).  Same file names as dctn/training.py:213-237."""

    DUMPED = ("x", "y", "indices", "output")

    def __init__(self, dir: str, set_breakpoint: bool):
        self.dir, self.set_breakpoint = dir, set_breakpoint

    def _target(self) -> str:
        leaf = "nan_loss_stop" if _world() == 1 else f"nan_loss_stop_rank{dist.get_rank()}"
        return os.path.join(self.dir, leaf)

    def __call__(self, st_x: StX, st_it: StIt) -> None:
        if bool(torch.isfinite(st_it["loss"])):
            return
        log = getLogger(__name__)
        log.warning("Stopping because of NaN or Inf loss")
        st_it["stop"] = True
        target = self._target()
        if os.path.exists(target):
            log.error(f"subdir={target!r} already exists")
        else:
            os.mkdir(target)
            tag = f"nitd={st_it['num_iters_done']}_loss={st_it['loss']:.3f}_reg_term={st_it['reg_term']:.3f}"
            torch.save(st_x["model"].state_dict(), os.path.join(target, f"model_{tag}.pth"))
            for key in self.DUMPED:
                torch.save(st_it[key], os.path.join(target, key + ".pth"))
        if self.set_breakpoint:
            breakpoint()


def make_stopper_on_nan_loss(dir: str, set_breakpoint: bool) -> Callable[[StX, StIt], None]:
    return _StopOnNonFiniteLoss(dir, set_breakpoint)


class _StopOnDeviceHalt:
    """Hook for the ``after_back`` list of a run whose optimizer carries a `GradGuard`: every ``every`` calls it reads
    the guard's block (the only synchronisation it makes) and, when the latch is set, raises the stop flag and writes
    the artefact `_StopOnNonFiniteLoss` writes - ``dir/nan_loss_stop`` (``nan_loss_stop_rank<r>`` with several ranks)
    holding the model's state_dict and whatever of ``x``, ``y``, ``indices``, ``output`` the iteration's dictionary
    has - with ``bad_step`` and ``last_norm`` in the model file's name and the whole block in ``guard.pth``.  The
    parameters it saves are those of the last good step: the guard kept the optimizer from applying any later one.
    The batch in ``st_it`` is the current one, up to ``every`` iterations after the one that set the latch;
    ``bad_step`` names that one."""

    DUMPED = _StopOnNonFiniteLoss.DUMPED

    def __init__(self, dir: str, guard: "GradGuard", every: int):
        assert every >= 1
        self.dir, self.guard, self.every = dir, guard, int(every)
        self._calls = 0

    def _target(self) -> str:
        leaf = "nan_loss_stop" if _world() == 1 else f"nan_loss_stop_rank{dist.get_rank()}"
        return os.path.join(self.dir, leaf)

    def __call__(self, st_x: StX, st_it: StIt) -> None:
        self._calls += 1
        if self._calls % self.every != 0:
            return
        state = self.guard.read()
        if not state["halted"]:
            return
        log = getLogger(__name__)
        log.warning(f"Stopping: the gradient guard halted at its check number {state['bad_step']} "
                    f"(last gradient norm {state['last_norm']})")
        st_it["stop"] = True
        target = self._target()
        if os.path.exists(target):
            log.error(f"subdir={target!r} already exists")
            return
        os.mkdir(target)
        tag = f"nitd={st_it['num_iters_done']}"
        if "loss" in st_it and "reg_term" in st_it:
            loss, reg_term = (float(torch.as_tensor(st_it[k]).detach()) for k in ("loss", "reg_term"))
            tag += f"_loss={loss:.3f}_reg_term={reg_term:.3f}"
        tag += f"_bad_step={state['bad_step']}_last_norm={state['last_norm']:.3e}"
        torch.save(st_x["model"].state_dict(), os.path.join(target, f"model_{tag}.pth"))
        torch.save(state, os.path.join(target, "guard.pth"))
        for key in self.DUMPED:
            if key in st_it:
                torch.save(st_it[key], os.path.join(target, key + ".pth"))


def make_stopper_on_device_halt(dir: str, guard: "GradGuard", every: int = 1) -> Callable[[StX, StIt], None]:
    return _StopOnDeviceHalt(dir, guard, every)


class _LRPlateauHook:
    """``torch.optim.lr_scheduler.ReduceLROnPlateau`` on an `LRSchedule`'s scale: called after every evaluation (an
    `evaluation.make_evaluation_hook`-style hook behind the one that fills ``st_it[key]``), it multiplies
    ``schedule.scale`` by ``factor`` once ``st_it[key]`` has not improved for ``patience`` calls in a row, never below
    ``min_scale``, and starts counting again.  Host logic: the scale is one device write at a launch boundary."""

    def __init__(self, schedule: "LRSchedule", key: str, low_is_good: bool, factor: float, patience: int,
                 min_scale: float = 0.0):
        if not 0.0 < factor < 1.0 or patience < 1 or min_scale < 0.0:
            raise ValueError(f"plateau hook: 0 < factor < 1, patience >= 1, min_scale >= 0; got {factor}, {patience}, {min_scale}")
        self.schedule, self.key, self.low_is_good = schedule, key, bool(low_is_good)
        self.factor, self.patience, self.min_scale = float(factor), int(patience), float(min_scale)
        self.best_value = float("inf") if low_is_good else float("-inf")
        self.num_bad_calls = 0

    def __call__(self, st_x: StX, st_it: StIt) -> None:
        value = float(st_it[self.key])
        if (value < self.best_value) if self.low_is_good else (value > self.best_value):
            self.best_value, self.num_bad_calls = value, 0
            return
        self.num_bad_calls += 1
        if self.num_bad_calls >= self.patience:
            self.num_bad_calls = 0
            new = LRSchedule._validated_scale(max(self.schedule.scale * self.factor, self.min_scale))   # as the block holds it
            if new != self.schedule.scale:
                self.schedule.scale = new
                getLogger(__name__).info(f"{self.key} on a plateau at st_it['num_iters_done']={st_it.get('num_iters_done')}: "
                                         f"learning-rate scale -> {self.schedule.scale}")


def make_lr_plateau_hook(schedule: "LRSchedule", key: str, low_is_good: bool, factor: float, patience: int,
                         min_scale: float = 0.0) -> Callable[[StX, StIt], None]:
    return _LRPlateauHook(schedule, key, low_is_good, factor, patience, min_scale)


def log_parameters_stats(st_x: StX, st_it: StIt) -> None:
    """Mean / std / shape of every parameter, one log line each."""
    log = getLogger(f"{__name__}.log_parameters_stats")
    log.info(f"After {st_it['num_iters_done']:07} iters:")
    with torch.no_grad():
        for name, param in st_x["model"].named_parameters():
            log.info(f"{name}: mu={param.float().mean():.7e}, sigma={param.float().std(unbiased=False):.7e}, "
                     f"shape={tuple(param.shape)}")
