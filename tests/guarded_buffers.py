"""A guarded, poisoned arena for the buffers the dctn_amd host modules hand to the kernel library (DESIGN.md "Buffer
contract tests").  include/dctn_amd.h promises that outputs are overwritten, that a workspace of exactly the queried size
is enough and needs nothing of its previous content, and that a call touches nothing outside its buffers; torch's
allocator (512-byte rounding inside large segments, frequently zero memory) and `_lib.workspace` (256-byte rounding, a
grow-only cache) hide a breach of any of them.  Used explicitly:

    with guarded(fill=0xFF) as arena:
        x = arena.place(x)                  # inputs: same values, inside a guarded allocation
        y = eps(core, x); y.backward(dy)
    arena.check()                           # synchronises, then asserts every guard byte is intact

While active, `torch.empty` / `torch.empty_like` / `torch.zeros` as the host modules in `MODULES` call them, and
`_lib.workspace`, come from the arena: every buffer is a view into its own uint8 allocation [guard | payload | guard],
the payload 512-byte aligned (what torch gives callers), the trailing guard at the very next byte after the payload, both
guards `GUARD` bytes of 0xFF (NaN as float32, float64 and bf16).  Payloads of empty / empty_like / workspace hold the
`fill` byte, those of zeros stay zero.  `workspace(n)` is exactly n bytes.  torch itself is not patched: each module's
`torch` name is bound to a proxy for the length of the block.  (`Tensor.new_zeros` is a method of the tensor, not of the
module's `torch`: the one scalar `training.py` makes with it stays torch's.)

Stale mode (`stale=True`, or a `StalePool` shared by several arenas): workspaces are carved from one buffer that is never
refilled, so each call inherits the flags, tickets and partial records of the one before - what the grow-only cache and
the caching allocator do in training.  Each view starts at the pool's aligned origin and ends at a temporary 0xFF guard
laid over the pool's own bytes, which are put back when the next workspace is asked for."""
from __future__ import annotations

import importlib
import os
import sys

import torch

GUARD = 64 << 10
ALIGN = 512
MODULES = ("eps", "eps_plus_linear", "conv_sbs", "logmatmulexp", "tn_inner", "window_stats", "training", "evaluation")
PATTERNS = {0xFF: "NaN; integers at their maximum", 0x7B: "large finite values", 0x00: "zero"}
LOG_ENV = "DCTN_GUARDED_LOG"   # a file that receives one line per allocation as it is made (to locate a GPU fault)

_HERE = os.path.abspath(__file__)
_active = None


def current():
    """The active arena, or None."""
    return _active


class GuardDamaged(AssertionError):
    pass


def _site():
    f = sys._getframe(1)
    while f is not None and os.path.abspath(f.f_code.co_filename) == _HERE:
        f = f.f_back
    if f is None:
        return "?:0"
    name = f.f_globals.get("__name__", os.path.basename(f.f_code.co_filename))
    return f"{name}:{f.f_lineno}"


def _shape(size):
    if len(size) == 1 and hasattr(size[0], "__iter__"):
        size = tuple(size[0])
    return tuple(int(s) for s in size)


def _numel(shape):
    n = 1
    for s in shape:
        n *= s
    return n


class _Record:
    __slots__ = ("site", "what", "nbytes", "lead", "trail", "keep")

    def __init__(self, site, what, nbytes, lead, trail, keep):
        self.site, self.what, self.nbytes, self.lead, self.trail, self.keep = site, what, nbytes, lead, trail, keep


def _guarded_bytes(nbytes, device):
    """(base, offset): a uint8 allocation of 0xFF bytes and the 512-aligned payload offset inside it."""
    base = torch.empty(2 * GUARD + nbytes + ALIGN, dtype=torch.uint8, device=device)
    base.fill_(0xFF)
    off = GUARD + (-(base.data_ptr() + GUARD)) % ALIGN
    return base, off


class StalePool:
    """The never-refilled workspace buffer of stale mode, one per device; shareable between arenas."""

    def __init__(self, fill=0xFF, capacity=1 << 20):
        self.fill, self.capacity = fill, capacity
        self.bufs = {}      # device -> (base, origin offset, capacity)
        self.live = {}      # device -> (record, guard view, saved bytes)

    def _buffer(self, device, nbytes):
        have = self.bufs.get(device)
        if have is not None and have[2] >= nbytes:
            return have
        cap = self.capacity
        while cap < nbytes:
            cap *= 2
        base, off = _guarded_bytes(cap + GUARD, device)
        base[off:off + cap + GUARD].fill_(self.fill)
        if have is not None:   # growing keeps what the smaller buffer held
            base[off:off + have[2]].copy_(have[0][have[1]:have[1] + have[2]])
        self.bufs[device] = (base, off, cap)
        return self.bufs[device]

    def retire(self, device):
        """Snapshots the temporary guard of the last workspace (for `check`) and gives the pool its bytes back."""
        live = self.live.pop(device, None)
        if live is not None:
            rec, guard, saved = live
            rec.trail = guard.clone()
            guard.copy_(saved)

    def carve(self, nbytes, device, site):
        self.retire(device)
        base, off, _ = self._buffer(device, nbytes)
        guard = base[off + nbytes:off + nbytes + GUARD]
        saved = guard.clone()
        guard.fill_(0xFF)
        rec = _Record(site, f"stale workspace of {nbytes} bytes", nbytes, base[off - GUARD:off], guard, base)
        self.live[device] = (rec, guard, saved)
        return base, off, rec


class _TorchProxy:
    """`torch` as a host module sees it inside the block: three allocation functions from the arena, the rest torch's."""

    def __init__(self, arena):
        self._arena = arena

    def __getattr__(self, name):
        return getattr(torch, name)

    def empty(self, *size, dtype=None, device=None, **kw):
        if kw:
            return torch.empty(*size, dtype=dtype, device=device, **kw)
        return self._arena.empty(_shape(size), dtype, device)

    def zeros(self, *size, dtype=None, device=None, **kw):
        if kw:
            return torch.zeros(*size, dtype=dtype, device=device, **kw)
        return self._arena.zeros(_shape(size), dtype, device)

    def empty_like(self, t, dtype=None, device=None, **kw):
        if kw:
            return torch.empty_like(t, dtype=dtype, device=device, **kw)
        return self._arena.empty_like(t, dtype, device)


class guarded:
    def __init__(self, fill=0xFF, stale=False, log=None):
        assert 0 <= int(fill) <= 0xFF
        self.fill = int(fill)
        self.pool = stale if isinstance(stale, StalePool) else (StalePool(self.fill) if stale else None)
        self.records = []
        self.count = {"empty": 0, "zeros": 0, "workspace": 0, "place": 0}
        self._log = log if log is not None else os.environ.get(LOG_ENV)
        self._undo = []

    # ---------------------------------------------------------------------------------------- activation
    def __enter__(self):
        global _active
        if _active is not None:
            raise RuntimeError("guarded(): an arena is already active")
        if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("guarded(): the arena does not run under stream capture")
        from dctn_amd import _lib

        proxy = _TorchProxy(self)
        try:
            for name in MODULES:
                mod = importlib.import_module("dctn_amd." + name)
                self._undo.append((mod, "torch", mod.torch))
                mod.torch = proxy
            self._undo.append((_lib, "workspace", _lib.workspace))
            _lib.workspace = self.workspace
        except BaseException:
            self._restore()
            raise
        _active = self
        return self

    def _restore(self):
        while self._undo:
            obj, name, value = self._undo.pop()
            setattr(obj, name, value)

    def __exit__(self, *exc):
        global _active
        self._restore()
        _active = None
        if self.pool is not None:
            for device in list(self.pool.live):   # stream-ordered after the last call that used it
                self.pool.retire(device)
        return False

    # ---------------------------------------------------------------------------------------- allocation
    def _note(self, rec):
        self.records.append(rec)
        if self._log:
            with open(self._log, "a") as f:
                f.write(f"{rec.site} {rec.what}\n")

    def _alloc(self, nbytes, device, fill, what, site):
        device = torch.device("cpu" if device is None else device)
        base, off = _guarded_bytes(nbytes, device)
        if nbytes and fill != 0xFF:
            base[off:off + nbytes].fill_(fill)
        self._note(_Record(site, what, nbytes, base[:off], base[off + nbytes:], base))
        return base, off

    def _typed(self, shape, dtype, device, fill, kind, strides=None):
        dtype = torch.get_default_dtype() if dtype is None else dtype
        item = torch.empty((), dtype=dtype).element_size()
        n = _numel(shape)
        base, off = self._alloc(n * item, device, fill, f"{kind} {tuple(shape)} {dtype}", _site())
        flat = base[off:off + n * item].view(dtype)
        return flat.view(shape) if strides is None else flat.as_strided(shape, strides)

    def empty(self, shape, dtype=None, device=None):
        self.count["empty"] += 1
        return self._typed(tuple(shape), dtype, device, self.fill, "empty")

    def zeros(self, shape, dtype=None, device=None):
        self.count["zeros"] += 1
        return self._typed(tuple(shape), dtype, device, 0x00, "zeros")

    def empty_like(self, t, dtype=None, device=None):
        self.count["empty"] += 1
        dtype = t.dtype if dtype is None else dtype
        strides = torch.empty_like(t, device="meta").stride()   # torch keeps the strides of a dense tensor
        return self._typed(tuple(t.shape), dtype, t.device if device is None else device, self.fill, "empty_like", strides)

    def workspace(self, nbytes, dev):
        """`_lib.workspace` under the arena: exactly `nbytes` (a zero-length view for 0: see `ZeroLength`)."""
        self.count["workspace"] += 1
        nbytes = int(nbytes)
        site = _site()
        if self.pool is not None:
            base, off, rec = self.pool.carve(nbytes, torch.device(dev), site)
            self._note(rec)
        else:
            base, off = self._alloc(nbytes, dev, self.fill, f"workspace of {nbytes} bytes", site)
        view = base[off:off + nbytes]
        return view if nbytes else ZeroLength(view, base.data_ptr() + off)

    def place(self, t):
        """The same values (and strides, for a dense tensor) inside a guarded allocation, on the tensor's device."""
        self.count["place"] += 1
        src = t.detach()
        dense = torch.empty_like(src, device="meta")
        if dense.stride() == src.stride():
            out = self._typed(tuple(src.shape), src.dtype, src.device, 0xFF, "place", src.stride())
        else:
            out = self._typed(tuple(src.shape), src.dtype, src.device, 0xFF, "place")
        out.copy_(src)
        return out.requires_grad_(t.requires_grad)

    # ---------------------------------------------------------------------------------------- verification
    def check(self):
        """Synchronises, then raises GuardDamaged for the first allocation whose leading or trailing guard changed."""
        if _active is self:
            raise RuntimeError("guarded.check() belongs after the block")
        if torch.cuda.is_available():
            torch.cuda.synchronize()
        if not self.records:
            return
        flags = [torch.stack(((r.lead != 0xFF).any(), (r.trail != 0xFF).any())).cpu() for r in self.records]
        hits = torch.stack(flags).tolist()
        for rec, (lead_hit, trail_hit) in zip(self.records, hits):
            if lead_hit:
                bad = torch.nonzero(rec.lead != 0xFF).flatten()
                start = int(bad[-1]) - rec.lead.numel()   # relative to the payload start: negative
                raise GuardDamaged(
                    f"leading guard damaged: {rec.what} allocated at {rec.site}; {bad.numel()} byte(s) changed, the nearest "
                    f"{-start} byte(s) before the payload start (offset {start - rec.nbytes} from the payload end), "
                    f"value 0x{int(rec.lead[bad[-1]]):02x}")
            if trail_hit:
                bad = torch.nonzero(rec.trail != 0xFF).flatten()
                raise GuardDamaged(
                    f"trailing guard damaged: {rec.what} allocated at {rec.site}; {bad.numel()} byte(s) changed, the first at "
                    f"offset +{int(bad[0])} from the payload end, value 0x{int(rec.trail[bad[0]]):02x}")

    def release(self):
        self.records.clear()


class ZeroLength:
    """What `workspace(0)` returns: torch answers `data_ptr() == 0` for every tensor without elements, and the library
    must be given a non-null pointer into the arena; callers use `data_ptr()` and `numel()` only."""

    def __init__(self, view, ptr):
        self.view, self._ptr = view, ptr
        self.dtype, self.device, self.shape = view.dtype, view.device, view.shape

    def data_ptr(self):
        return self._ptr

    def numel(self):
        return 0

    def __len__(self):
        return 0


def decode(fill, dtype):
    """The value every element of a buffer of `fill` bytes has in `dtype`."""
    item = torch.empty((), dtype=dtype).element_size()
    return torch.full((item,), fill, dtype=torch.uint8).view(dtype)[0]
