"""Whole-run snapshots: everything a training run keeps on the device, gathered by one launch, saved without stalling
the stream, and put back in place under the graphs that were captured over it (dctn_amd/csrc/run_state.hip;
include/dctn_amd.h holds the normative arena layout and digest, DESIGN.md section 7a the ordering).

The reference's runner only has ``--load-model-state``.  Here the optimizer (`FlatAdam` / `FlatSGD`: flat parameters,
moments or momentum, master copy, step block, regulariser partials), the gradient guard, the fused dropout and the batch
source all keep their state in fixed device buffers so that captured graphs can replay it; `RunState` names those
buffers, `RunState.snapshot()` gathers them at one point of the stream into one arena and copies the arena to pinned host
memory on a side stream, `Snapshot.save()` writes one file, and `RunState.load()` scatters a file back IN PLACE: a
`GraphedTrainStep` captured over the buffers goes on replaying them, and the run continues bit for bit.

File (no pickle): ``DCTNRUN1`` | uint64 manifest length | UTF-8 JSON manifest | zero padding to a multiple of 4096 | the
arena.  The manifest holds the format version, per region its name, dtype, shape, byte count, arena offset and digest
(s1, s2), where the model's state_dict entries lie inside the regions, the host scalars (hyper-parameters, the source's
plan, ``guard.max_norm``) and the caller's extras.

Limits: masks of the torch-op dropout (torch's generator) are not restored - use `use_fused_dropout`; ``torch.optim``
optimizers are refused (their state is not in fixed buffers); a region must start at a multiple of 4 bytes.
"""
from __future__ import annotations

import json
import os
import struct
from collections import deque
from typing import Any, Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch
from torch import Tensor

from . import _lib as L
from .ddp import is_rank0

MAGIC = b"DCTNRUN1"
FORMAT_VERSION = 1
PAGE = 4096          # the arena starts at a multiple of it in the file
MAX_REGIONS = 16     # regions of one launch (dctn_state_max_regions)
_MASK64 = (1 << 64) - 1

_DTYPES = {"float32": torch.float32, "float64": torch.float64, "bfloat16": torch.bfloat16, "float16": torch.float16,
           "int32": torch.int32, "int64": torch.int64, "int16": torch.int16, "int8": torch.int8, "uint8": torch.uint8,
           "bool": torch.bool}
_ITEMSIZE = {name: torch.empty((), dtype=dt).element_size() for name, dt in _DTYPES.items()}


# ------------------------------------------------------------------------------------------------ host arithmetic
def digest(buffer) -> Tuple[int, int]:
    """``(s1, s2)`` of a buffer of bytes (bytes, bytearray, memoryview or a numpy array, taken as its bytes): the bytes
    zero-padded to a multiple of 16, read as little-endian uint32 words w_0 .. w_(m-1); s1 = sum w_i and
    s2 = sum (i + 1) w_i, both mod 2^64.  What `dctn_state_gather` / `dctn_state_scatter` leave per region."""
    raw = np.ascontiguousarray(buffer).view(np.uint8).reshape(-1) if isinstance(buffer, np.ndarray) else np.frombuffer(
        buffer, dtype=np.uint8)
    padded = np.zeros(-(-raw.size // 16) * 16, dtype=np.uint8)
    padded[: raw.size] = raw
    words = padded.view("<u4").astype(np.uint64)
    weights = np.arange(1, words.size + 1, dtype=np.uint64)
    return int(words.sum(dtype=np.uint64)) & _MASK64, int((words * weights).sum(dtype=np.uint64)) & _MASK64


def arena_layout(byte_counts: Sequence[int]) -> Tuple[List[int], int]:
    """``(offsets, total)``: region r starts at the sum of the earlier lengths, each rounded up to 16."""
    offsets, total = [], 0
    for n in byte_counts:
        if int(n) < 1:
            raise ValueError(f"a region holds at least one byte, got {n}")
        offsets.append(total)
        total += -(-int(n) // 16) * 16
    return offsets, total


def _dtype_name(dtype: torch.dtype) -> str:
    name = str(dtype).replace("torch.", "")
    if name not in _DTYPES:
        raise TypeError(f"a snapshot cannot hold {dtype} tensors")
    return name


# ------------------------------------------------------------------------------------------------ the file
def write_file(path: str, manifest: Dict[str, Any], arena: np.ndarray) -> None:
    """Writes magic, manifest and arena to a temporary name beside ``path``, then `os.replace`: a reader sees the old
    file or the whole new one."""
    arena = np.ascontiguousarray(arena).view(np.uint8).reshape(-1)
    text = json.dumps(manifest).encode("utf-8")
    head = MAGIC + struct.pack("<Q", len(text)) + text
    head += b"\0" * (-len(head) % PAGE)
    tmp = f"{path}.tmp{os.getpid()}"
    try:
        with open(tmp, "wb") as f:
            f.write(head)
            f.write(memoryview(arena))
            f.flush()
            os.fsync(f.fileno())
        os.replace(tmp, path)
    except BaseException:
        if os.path.exists(tmp):
            os.remove(tmp)
        raise


def read_file(path: str) -> Tuple[Dict[str, Any], np.ndarray]:
    """``(manifest, arena)`` of a snapshot file, the arena as a uint8 array.  Checks the magic, the lengths and that
    the regions tile the arena as `arena_layout` says; the digests are `verify_digests`'s."""
    with open(path, "rb") as f:
        head = f.read(16)
        if len(head) < 16:
            raise ValueError(f"{path}: truncated: {len(head)} bytes, the header alone has 16")
        if head[:8] != MAGIC:
            raise ValueError(f"{path}: wrong magic {head[:8]!r}, a run snapshot starts with {MAGIC!r}")
        (length,) = struct.unpack("<Q", head[8:])
        text = f.read(length) if length < 1 << 32 else b""
        if len(text) != length:
            raise ValueError(f"{path}: truncated: the manifest has {length} bytes, the file holds {len(text)} of them")
        try:
            manifest = json.loads(text.decode("utf-8"))
        except ValueError as e:
            raise ValueError(f"{path}: the manifest is not JSON: {e}") from None
        if manifest.get("format") != FORMAT_VERSION:
            raise ValueError(f"{path}: format version {manifest.get('format')!r}, this build reads {FORMAT_VERSION}")
        regions = manifest["regions"]
        offsets, total = arena_layout([r["bytes"] for r in regions])
        for r, off in zip(regions, offsets):
            if r["offset"] != off:
                raise ValueError(f"{path}: region {r['name']!r} at offset {r['offset']}, the layout puts it at {off}")
            if r["bytes"] != _ITEMSIZE.get(r["dtype"], 0) * int(np.prod(r["shape"], dtype=np.int64)):
                raise ValueError(f"{path}: region {r['name']!r}: {r['bytes']} bytes do not hold {r['shape']} {r['dtype']}")
        f.seek(-(-(16 + length) // PAGE) * PAGE)
        arena = np.fromfile(f, dtype=np.uint8)
    if arena.size != total:
        raise ValueError(f"{path}: truncated: the arena has {total} bytes, the file holds {arena.size} of them"
                         if arena.size < total else f"{path}: {arena.size - total} bytes follow the arena")
    return manifest, arena


def verify_digests(manifest: Dict[str, Any], arena: np.ndarray, what: str = "snapshot") -> None:
    """Raises ValueError naming the first region whose bytes do not give the manifest's digest."""
    for r in manifest["regions"]:
        got = digest(arena[r["offset"]: r["offset"] + r["bytes"]])
        if got != (r["s1"], r["s2"]):
            raise ValueError(f"{what}: region {r['name']!r} is damaged: its bytes give the digest {got}, the manifest "
                             f"says {(r['s1'], r['s2'])}")


def check_regions(manifest: Dict[str, Any], expected: Sequence[Tuple[str, str, Sequence[int]]],
                  what: str = "snapshot") -> None:
    """Holds the manifest's regions to ``expected``, a list of ``(name, dtype name, shape)``: the same entries in the same
    order.  Raises ValueError naming the first entry that differs."""
    saved = manifest["regions"]
    for i, (name, dtype, shape) in enumerate(expected):
        if i >= len(saved):
            raise ValueError(f"{what}: entry {name!r} is missing (the file holds {len(saved)} regions, the run {len(expected)})")
        r = saved[i]
        if r["name"] != name:
            raise ValueError(f"{what}: entry {i} is {r['name']!r} in the file, {name!r} in the run")
        if r["dtype"] != dtype:
            raise ValueError(f"{what}: entry {name!r} is {r['dtype']} in the file, {dtype} in the run")
        if list(r["shape"]) != list(shape):
            raise ValueError(f"{what}: entry {name!r} has shape {list(r['shape'])} in the file, {list(shape)} in the run")
    if len(saved) > len(expected):
        raise ValueError(f"{what}: entry {saved[len(expected)]['name']!r} of the file is not part of the run")


def build_manifest(entries: Sequence[Tuple[str, str, Sequence[int]]], digests: Sequence[Tuple[int, int]],
                   model: Optional[List[Dict[str, Any]]] = None, host: Optional[Dict[str, Any]] = None,
                   extras: Optional[Dict[str, Any]] = None) -> Dict[str, Any]:
    byte_counts = [_ITEMSIZE[dtype] * int(np.prod(shape, dtype=np.int64)) for _, dtype, shape in entries]
    offsets, total = arena_layout(byte_counts)
    regions = [dict(name=name, dtype=dtype, shape=[int(s) for s in shape], bytes=n, offset=off, s1=int(d[0]), s2=int(d[1]))
               for (name, dtype, shape), n, off, d in zip(entries, byte_counts, offsets, digests)]
    return dict(format=FORMAT_VERSION, arena_bytes=total, regions=regions, model=model or [], host=host or {},
                extras=extras or {})


def save_arrays(path: str, arrays: Dict[str, np.ndarray], host: Optional[Dict[str, Any]] = None,
                extras: Optional[Dict[str, Any]] = None) -> None:
    """A snapshot file from named numpy arrays (tools and tests; no device)."""
    entries = [(name, a.dtype.name, a.shape) for name, a in arrays.items()]
    manifest = build_manifest(entries, [digest(a) for a in arrays.values()], host=host, extras=extras)
    arena = np.zeros(manifest["arena_bytes"], dtype=np.uint8)
    for r, a in zip(manifest["regions"], arrays.values()):
        arena[r["offset"]: r["offset"] + r["bytes"]] = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    write_file(path, manifest, arena)


def load_arrays(path: str, expected: Optional[Sequence[Tuple[str, str, Sequence[int]]]] = None):
    """``(manifest, {name: array})`` of a file whose regions have numpy dtypes; checks ``expected`` (see `check_regions`)
    and every digest."""
    manifest, arena = read_file(path)
    if expected is not None:
        check_regions(manifest, expected, path)
    verify_digests(manifest, arena, path)
    return manifest, {r["name"]: arena[r["offset"]: r["offset"] + r["bytes"]].view(np.dtype(r["dtype"])).reshape(r["shape"])
                      for r in manifest["regions"]}


def read_model_state(path: str, ema: bool = False) -> Dict[str, Tensor]:
    """The model's state_dict (``epses.i``, ``linear.weight``, ``linear.bias``, ``p``) of a snapshot file as CPU tensors,
    for ``model.load_state_dict`` / ``--load-model-state``-style use without building the run.  Every digest is checked.
    ``ema=True``: every entry that lies in the optimizer's flat buffer comes from the run's weight average
    (`training.WeightEMA`) instead, its float32 values cast to the entry's dtype (round to nearest even, as
    ``WeightEMA.apply()``); ValueError for a file without one."""
    manifest, arena = read_file(path)
    verify_digests(manifest, arena, path)
    regions = {r["name"]: r for r in manifest["regions"]}
    averaged = regions.get("optimizer.ema")
    if ema and averaged is None:
        raise ValueError(f"{path}: the run was saved without a weight average (no region 'optimizer.ema')")
    state = {}
    for e in manifest["model"]:
        r = regions[e["region"]]
        item = _ITEMSIZE[e["dtype"]]
        n = item * int(np.prod(e["shape"], dtype=np.int64))
        if e["offset"] + n > r["bytes"]:
            raise ValueError(f"{path}: model entry {e['key']!r} reaches past region {r['name']!r}")
        if ema and e["region"] == "optimizer.flat":   # the same elements of the float32 average
            start = averaged["offset"] + e["offset"] // item * 4
            if (e["offset"] // item) * 4 + n // item * 4 > averaged["bytes"]:
                raise ValueError(f"{path}: model entry {e['key']!r} reaches past the weight average")
            raw = torch.from_numpy(arena[start: start + n // item * 4].copy()).view(torch.float32)
            state[e["key"]] = raw.to(_DTYPES[e["dtype"]]).reshape(e["shape"])
            continue
        start = r["offset"] + e["offset"]
        raw = torch.from_numpy(arena[start: start + n].copy())
        state[e["key"]] = raw.view(_DTYPES[e["dtype"]]).reshape(e["shape"])
    return state


# ------------------------------------------------------------------------------------------------ the run
class Snapshot:
    """One `RunState.snapshot()`: the arena and the device's digests on their way to pinned host memory."""

    def __init__(self, manifest: Dict[str, Any], arena: Tensor, digests: Tensor, done: "torch.cuda.Event"):
        self.manifest, self._arena, self._digests, self._done = manifest, arena, digests, done
        self._checked = False

    @property
    def extras(self) -> Dict[str, Any]:
        return self.manifest["extras"]

    def ready(self) -> bool:
        """Whether the copy to the host has finished (does not block)."""
        return self._done.query()

    def wait(self) -> "Snapshot":
        self._done.synchronize()
        return self

    def _finish(self) -> np.ndarray:
        """Waits for the copy, then holds the host bytes to the device's digests."""
        self.wait()
        arena = self._arena.numpy()
        if not self._checked:
            device = self._digests.numpy().view(np.uint64).reshape(-1, 2)
            for r, (s1, s2) in zip(self.manifest["regions"], device):
                got = digest(arena[r["offset"]: r["offset"] + r["bytes"]])
                if got != (int(s1), int(s2)):
                    raise RuntimeError(f"snapshot: region {r['name']!r} arrived damaged: the host bytes give the digest "
                                       f"{got}, the device computed {(int(s1), int(s2))}")
                r["s1"], r["s2"] = int(s1), int(s2)
            self._checked = True
        return arena

    def save(self, path: str) -> str:
        """Waits for the copy, recomputes every region's digest from the host bytes (raises if one differs from the
        device's) and writes the file through a temporary name and `os.replace`."""
        write_file(path, self.manifest, self._finish())
        return path


def run_parts(model, optimizer, batch_source, guard, trace=None) -> List[Tuple[str, Any]]:
    """``[(slot, part), ...]`` in file order: the components of a run that say themselves what they keep on the device.
    A part has ``run_regions()`` -> ``[(local name, tensor), ...]`` in file order, ``run_host()`` -> its JSON-able host
    scalars or None, ``run_restored(host, blocks)`` which sets its host mirrors once its regions were put back
    (``blocks``: local name -> the file's bytes of that region, a uint8 view into the arena), and, where there is
    something to refuse, ``run_check(host)`` which raises ValueError before anything is written.  The model is a part
    only for what its state_dict does not hold; any other ``nn.Module`` is none."""
    if optimizer is not None and not hasattr(optimizer, "run_regions"):
        raise TypeError(f"RunState takes a FlatAdam or a FlatSGD, got {type(optimizer).__name__}: a snapshot gathers FIXED "
                        "device buffers that captured graphs replay, and a torch.optim optimizer keeps its state in "
                        "per-parameter tensors it creates lazily and may replace")
    slots = (("optimizer", optimizer), ("model", model if hasattr(model, "run_regions") else None), ("guard", guard),
             ("batch_source", batch_source), ("trace", trace))
    return [(slot, part) for slot, part in slots if part is not None]


def run_regions(model, optimizer, batch_source, guard, trace=None):
    """``(regions, model entries)``: the named device tensors of a run, in file order - the optimizer's, every entry of
    the model's state_dict that does not lie inside ``optimizer.flat``, then the other parts' - and where each
    state_dict entry lies in them.  Needs no device."""
    regions: List[Tuple[str, Tensor]] = []
    behind: List[Tuple[str, Tensor]] = []
    for slot, part in run_parts(model, optimizer, batch_source, guard, trace):
        (regions if slot == "optimizer" else behind).extend((f"{slot}.{name}", t) for name, t in part.run_regions())
    flat = dict(regions).get("optimizer.flat")
    entries = []
    for key, t in model.state_dict(keep_vars=True).items():
        t = t.detach()
        inside = (flat is not None and t.numel() and t.is_contiguous() and t.dtype == flat.dtype
                  and flat.data_ptr() <= t.data_ptr()
                  and t.data_ptr() + t.numel() * t.element_size() <= flat.data_ptr() + flat.numel() * flat.element_size())
        if inside:
            entries.append(dict(key=key, region="optimizer.flat", offset=t.data_ptr() - flat.data_ptr(),
                                dtype=_dtype_name(t.dtype), shape=list(t.shape)))
        else:
            regions.append((f"model.{key}", t))
            entries.append(dict(key=key, region=f"model.{key}", offset=0, dtype=_dtype_name(t.dtype), shape=list(t.shape)))
    return regions + behind, entries


class RunState:
    """The device state of a training run as named regions.  Each part of the run (`run_parts`) lists its own, and
    `RunState` puts the slot's name in front: a `FlatAdam` / `FlatSGD` as ``optimizer.`` its flat parameter buffer, the
    moments (or the momentum buffer), the master copy, the values and the block of its `WeightEMA`, the blocks of its
    `LRSchedule` and its `ParamGroups` table, the
    16-byte step block and ``sq_sum``, each only when the optimizer has it (a file and a run that disagree about an option
    are refused at that entry; runs without an option keep their region lists and their files); every entry of the
    model's state_dict that does not live in the flat buffer (the buffer ``p``; without an optimizer every parameter) as
    a region of its own; the model's fused dropout state; the guard's block (``guard`` defaults to the optimizer's); the
    batch source's block; with ``trace`` (a `training.StepTrace`) its head and ring, so that a resumed run continues its
    ``seq``.  The host scalars travel in the manifest, one entry per part that has some: the hyper-parameters and ``lr``,
    `FlatSGD`'s step count, the source's ``n`` / ``batch_size`` / ``seed``, ``guard.max_norm``.

    ``snapshot(extras)`` never blocks the host: it enqueues the gather on the current stream (one launch per 16 regions)
    and the copy of arena and digests to pinned memory on a side stream behind an event; the next ``snapshot()`` makes the
    training stream wait ON THE DEVICE for that copy before it overwrites the one arena.  ``load(path)`` checks names,
    dtypes, shapes and digests on the host before it writes anything, then uploads and scatters in place and sets the
    host mirrors; it returns the extras.  Every region must start at a multiple of 4 bytes (NotImplementedError)."""

    def __init__(self, model: torch.nn.Module, optimizer=None, *, batch_source=None, guard=None, trace=None):
        if guard is None:
            guard = getattr(optimizer, "guard", None)
        self.model, self.optimizer, self.batch_source, self.guard = model, optimizer, batch_source, guard
        self.trace = trace
        self._parts = run_parts(model, optimizer, batch_source, guard, trace)
        regions, self._model_entries = run_regions(model, optimizer, batch_source, guard, trace)
        if not regions:
            raise ValueError("RunState: nothing to save")
        self.device = L.require_device(*(t for _, t in regions))
        for name, t in regions:
            if not t.is_contiguous() or t.numel() < 1:
                raise ValueError(f"RunState: region {name!r} must be a contiguous, non-empty tensor")
        self.names = [name for name, _ in regions]
        self.tensors = [t for _, t in regions]
        self.entries = [(name, _dtype_name(t.dtype), tuple(t.shape)) for name, t in regions]
        self.byte_counts = [t.numel() * t.element_size() for t in self.tensors]
        self.offsets, self.arena_bytes = arena_layout(self.byte_counts)
        lib = L.lib()
        assert lib.dctn_state_max_regions() == MAX_REGIONS
        assert lib.dctn_state_arena_bytes(L.i64_array(self.byte_counts[:MAX_REGIONS]),
                                          min(len(regions), MAX_REGIONS)) == arena_layout(self.byte_counts[:MAX_REGIONS])[1]
        with torch.cuda.device(self.device):
            self._arena = torch.empty(self.arena_bytes, dtype=torch.uint8, device=self.device)
            self._digests = torch.empty(2 * len(regions), dtype=torch.int64, device=self.device)
            self._side = torch.cuda.Stream(self.device)
        self._arena.record_stream(self._side)
        self._digests.record_stream(self._side)
        self._copy_done: Optional[torch.cuda.Event] = None

    # ------------------------------------------------------------------------------------------ launches
    def _launch(self, scatter: bool) -> None:
        lib, stream = L.lib(), L.stream_ptr(self.device)
        for first in range(0, len(self.tensors), MAX_REGIONS):
            group = slice(first, first + MAX_REGIONS)
            tensors, counts = self.tensors[group], self.byte_counts[group]
            arena = self._arena.data_ptr() + self.offsets[first]
            digests = self._digests.data_ptr() + 16 * first
            if scatter:
                rc = lib.dctn_state_scatter(arena, L.ptr_array(tensors), L.i64_array(counts), len(tensors), digests, stream)
            else:
                rc = lib.dctn_state_gather(L.ptr_array(tensors), L.i64_array(counts), len(tensors), arena,
                                           arena_layout(counts)[1], digests, stream)
            what = ", ".join(self.names[group])
            L.check(rc, f"run state {'scatter' if scatter else 'gather'} ({what}; every region starts at a multiple of 4 bytes)")

    def _check_alignment(self) -> None:
        for name, t in zip(self.names, self.tensors):
            if t.data_ptr() % 4:
                raise NotImplementedError(f"RunState: region {name!r} starts at an address that is no multiple of 4 "
                                          "(a bfloat16 view at an odd element): nothing was launched")

    def _refuse_applied(self, what: str) -> None:
        """While a `training.WeightEMA` is applied the flat buffer holds the averaged weights, not the live ones."""
        ema = getattr(self.optimizer, "ema", None)
        if ema is not None:
            ema._refuse_applied(what)

    def _host_scalars(self) -> Dict[str, Any]:
        scalars = ((slot, part.run_host()) for slot, part in self._parts)
        return {slot: host for slot, host in scalars if host is not None}

    # ------------------------------------------------------------------------------------------ snapshot
    def snapshot(self, extras: Optional[Dict[str, Any]] = None) -> Snapshot:
        """The run as it stands at this point of the current stream.  ``extras``: JSON-able host state that `load`
        hands back (``num_iters_done``, an early stopper's counters, the best value seen)."""
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("RunState.snapshot() records events and copies to the host: not during a graph capture")
        self._refuse_applied("RunState.snapshot()")
        extras = json.loads(json.dumps({} if extras is None else extras))   # JSON-able, and a copy
        self._check_alignment()
        manifest = build_manifest(self.entries, [(0, 0)] * len(self.entries), self._model_entries, self._host_scalars(),
                                  extras)
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device)
            if self._copy_done is not None:   # the one arena is free once the last copy has read it: a device-side wait
                stream.wait_event(self._copy_done)
            self._launch(scatter=False)
            gathered = torch.cuda.Event()
            gathered.record(stream)
            host_arena = torch.empty(self.arena_bytes, dtype=torch.uint8, pin_memory=True)
            host_digests = torch.empty(2 * len(self.tensors), dtype=torch.int64, pin_memory=True)
            with torch.cuda.stream(self._side):
                self._side.wait_event(gathered)
                host_arena.copy_(self._arena, non_blocking=True)
                host_digests.copy_(self._digests, non_blocking=True)
                done = torch.cuda.Event()
                done.record(self._side)
        self._copy_done = done
        return Snapshot(manifest, host_arena, host_digests, done)

    # ------------------------------------------------------------------------------------------ load
    def _check_host(self, host: Dict[str, Any]) -> None:
        """Every part's host scalars are in the file, no other part's are, and no part refuses its own."""
        live = self._host_scalars()
        for slot in {**live, **host}:
            if (host.get(slot) is None) != (slot not in live):
                raise ValueError(f"snapshot: entry {slot!r} is {'missing from' if slot in live else 'only in'} the file")
        for slot, part in self._parts:
            if hasattr(part, "run_check"):
                part.run_check(host[slot])

    def load(self, path: str) -> Dict[str, Any]:
        """Puts a saved run back IN PLACE and returns its extras.  Nothing on the device is written before every name,
        dtype, shape and digest has been checked on the host (ValueError naming the entry); after the scatter the
        device's digests of what it read are held to the manifest's."""
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("RunState.load() writes the run's buffers from the host: not during a graph capture")
        self._refuse_applied("RunState.load()")
        manifest, arena = read_file(path)
        check_regions(manifest, self.entries, path)
        self._check_host(manifest["host"])
        verify_digests(manifest, arena, path)
        self._check_alignment()
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device)
            if self._copy_done is not None:
                stream.wait_event(self._copy_done)
            self._arena.copy_(torch.from_numpy(arena))
            self._launch(scatter=True)
            device = self._digests.cpu().numpy().view(np.uint64).reshape(-1, 2)   # the one synchronisation
        for r, (s1, s2) in zip(manifest["regions"], device):
            if (int(s1), int(s2)) != (r["s1"], r["s2"]):
                raise RuntimeError(f"{path}: region {r['name']!r} was damaged on its way to the device: the scatter read "
                                   f"the digest {(int(s1), int(s2))}, the manifest says {(r['s1'], r['s2'])}")
        # the regions came back: every part's host mirrors follow, from its host scalars and the file's bytes of its regions
        saved = {r["name"]: arena[r["offset"]: r["offset"] + r["bytes"]] for r in manifest["regions"]}
        for slot, part in self._parts:
            part.run_restored(manifest["host"].get(slot), {name: saved[f"{slot}.{name}"] for name, _ in part.run_regions()})
        return manifest["extras"]


class RunCheckpointer:
    """Hook for `training.train` (the ``after_param_upd`` list) and for a hand-written replay loop: every call takes a
    `RunState.snapshot` tagged with ``st_it["num_iters_done"]`` - on rank 0 only; the other ranks hold the same state -
    and writes the PREVIOUS call's snapshot to ``dir/run_nitd=<7 digits>.dctn`` (its copy has had a whole interval to
    finish; if it has not, this waits for it).  The newest ``n`` files are kept.  ``flush()`` writes the pending one:
    call it when the loop ends.  ``extras(st_x, st_it)``, optional, returns more JSON-able host state to save.

    The snapshot is the state AFTER iteration ``num_iters_done``: resume with ``run.load(path)`` and
    ``train(..., first_iter=extras["num_iters_done"] + 1)``."""

    def __init__(self, dir: str, run: RunState, n: int,
                 extras: Optional[Callable[[Dict[Any, Any], Dict[Any, Any]], Dict[str, Any]]] = None):
        assert n >= 1
        self.dir, self.run, self.n, self.extras = dir, run, int(n), extras
        self.filenames: deque = deque()
        self._pending: Optional[Tuple[Snapshot, str]] = None

    def __call__(self, st_x: Dict[Any, Any], st_it: Dict[Any, Any]) -> None:
        if not is_rank0():
            return
        more = {} if self.extras is None else dict(self.extras(st_x, st_it))
        done = int(st_it["num_iters_done"])
        snap = self.run.snapshot({**more, "num_iters_done": done})
        previous, self._pending = self._pending, (snap, f"run_nitd={done:07}.dctn")
        if previous is not None:
            self._write(*previous)

    def _write(self, snap: Snapshot, name: str) -> None:
        snap.save(os.path.join(self.dir, name))
        self.filenames.appendleft(name)
        while len(self.filenames) > self.n:
            os.remove(os.path.join(self.dir, self.filenames.pop()))

    def flush(self) -> Optional[str]:
        """Writes the pending snapshot (waits for its copy); returns the newest file's path, if any."""
        if self._pending is not None:
            previous, self._pending = self._pending, None
            self._write(*previous)
        return os.path.join(self.dir, self.filenames[0]) if self.filenames else None
