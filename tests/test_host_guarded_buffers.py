"""Host checks of the guarded arena (tests/guarded_buffers.py) on CPU tensors: alignment and exact sizes, patching
confined to the dctn_amd host modules and undone on exit, damage reports, the zero-length workspace, the fill patterns."""
import importlib

import pytest
import torch

from dctn_amd import _lib as L
from tests import guarded_buffers as G
from tests.guarded_buffers import GUARD, GuardDamaged, StalePool, guarded

CPU = torch.device("cpu")


def _modules():
    return [importlib.import_module("dctn_amd." + n) for n in G.MODULES]


def test_payloads_are_aligned_exact_and_filled():
    import dctn_amd.eps as E

    with guarded(fill=0x7B) as arena:
        a = E.torch.empty((3, 5), dtype=torch.float32, device=CPU)
        b = E.torch.empty(7, dtype=torch.uint8)
        z = E.torch.zeros(2, dtype=torch.float64, device=CPU)
        like = E.torch.empty_like(torch.ones(4, 6, dtype=torch.bfloat16).t())
        ws = L.workspace(1001, CPU)
        placed = arena.place(torch.arange(24.0).reshape(2, 3, 4).permute(0, 2, 1))
    assert a.shape == (3, 5) and a.dtype == torch.float32 and b.shape == (7,) and b.dtype == torch.uint8
    assert ws.dtype == torch.uint8 and ws.numel() == 1001            # not max(n, 256), not rounded
    assert like.shape == (6, 4) and like.stride() == (1, 6)          # torch.empty_like keeps a dense tensor's strides
    assert torch.equal(placed, torch.arange(24.0).reshape(2, 3, 4).permute(0, 2, 1)) and placed.stride() == (12, 1, 4)
    for t in (a, b, z, like, ws, placed):
        assert t.data_ptr() % 512 == 0
    assert float(a[0, 0]) == float(G.decode(0x7B, torch.float32)) and int(b[3]) == 0x7B and int(ws[1000]) == 0x7B
    assert torch.equal(z, torch.zeros(2, dtype=torch.float64))       # accumulators by contract stay zero
    # the guards: GUARD bytes or more on each side, the trailing one at the very next byte after the payload
    for rec, nbytes in zip(arena.records, (60, 7, 16, 48, 1001, 96)):
        assert rec.nbytes == nbytes and rec.lead.numel() >= GUARD and rec.trail.numel() >= GUARD
        assert rec.trail.data_ptr() == rec.lead.data_ptr() + rec.lead.numel() + nbytes
        assert bool((rec.lead == 0xFF).all()) and bool((rec.trail == 0xFF).all())
    assert arena.count == {"empty": 3, "zeros": 1, "workspace": 1, "place": 1}
    arena.check()


def test_patching_is_confined_and_undone_on_exit_and_on_exception():
    import dctn_amd.ddp as ddp
    import dctn_amd.utils as utils

    real_ws = L.workspace
    with guarded():
        assert all(isinstance(m.torch, G._TorchProxy) for m in _modules())
        assert L.workspace is not real_ws
        assert L.torch is torch and ddp.torch is torch and getattr(utils, "torch", torch) is torch   # not host modules
        assert torch.empty.__module__ != G.__name__                                               # torch itself untouched
        import dctn_amd.eps as E
        assert E.torch.float32 is torch.float32 and E.torch.cuda is torch.cuda                     # everything else forwarded
        with pytest.raises(RuntimeError, match="already active"):
            guarded().__enter__()
    assert all(m.torch is torch for m in _modules()) and L.workspace is real_ws and G.current() is None
    with pytest.raises(ZeroDivisionError):
        with guarded():
            1 / 0
    assert all(m.torch is torch for m in _modules()) and L.workspace is real_ws and G.current() is None


def _line_of(marker):
    with open(__file__) as f:
        return next(i for i, line in enumerate(f, 1) if marker in line and "_line_of" not in line)


def test_damage_to_the_trailing_guard_is_reported_with_site_and_offset():
    import dctn_amd.eps as E

    with guarded() as arena:
        ok = E.torch.empty(5, dtype=torch.float32)
        out = E.torch.empty((3, 5), dtype=torch.float32)   # SITE-TRAIL
    arena.check()
    base = arena.records[1].keep
    start = out.data_ptr() - base.data_ptr()
    base[start + 60 + 2] = 0x01             # the third byte past the end of `out`
    with pytest.raises(GuardDamaged) as e:
        arena.check()
    msg = str(e.value)
    assert "trailing guard" in msg and f"{__name__}:{_line_of('SITE-TRAIL')}" in msg
    assert "(3, 5)" in msg and "torch.float32" in msg and "offset +2 from the payload end" in msg and "0x01" in msg
    del ok


def test_damage_to_the_leading_guard_is_reported():
    with guarded() as arena:
        ws = L.workspace(300, CPU)   # SITE-LEAD
    base = arena.records[0].keep
    start = ws.data_ptr() - base.data_ptr()
    base[start - 4] = 0x00
    with pytest.raises(GuardDamaged) as e:
        arena.check()
    msg = str(e.value)
    assert "leading guard" in msg and f"{__name__}:{_line_of('SITE-LEAD')}" in msg and "workspace of 300 bytes" in msg
    assert "4 byte(s) before the payload start" in msg and "offset -304 from the payload end" in msg


def test_zero_length_workspace_has_a_pointer_into_the_arena():
    with guarded() as arena:
        ws = L.workspace(0, CPU)
    assert ws.numel() == 0 and ws.data_ptr() != 0 and ws.data_ptr() % 512 == 0
    rec = arena.records[0]
    assert ws.data_ptr() == rec.trail.data_ptr() == rec.lead.data_ptr() + rec.lead.numel()
    arena.check()


@pytest.mark.parametrize("fill,f32,f64,bf16", [(0xFF, None, None, None), (0x7B, 1.3e36, 6.5e286, 1.3e36), (0x00, 0.0, 0.0, 0.0)])
def test_fill_patterns_decode_as_stated(fill, f32, f64, bf16):
    for dtype, want in ((torch.float32, f32), (torch.float64, f64), (torch.bfloat16, bf16)):
        got = float(G.decode(fill, dtype))
        if want is None:
            assert got != got                               # NaN in all three formats
        else:
            assert got == want or abs(got - want) <= 0.01 * want
    assert int(torch.full((4,), fill, dtype=torch.uint8).view(torch.int32)[0]) == {0xFF: -1, 0x7B: 0x7B7B7B7B, 0x00: 0}[fill]
    assert int(torch.full((4,), 0xFF, dtype=torch.uint8).view(torch.int32)[0]) & 0xFFFFFFFF == 0xFFFFFFFF   # counters at max


def test_stale_workspaces_inherit_their_content_and_keep_an_exact_end():
    pool = StalePool(fill=0x7B, capacity=4096)
    with guarded(fill=0xFF, stale=pool) as a1:
        w1 = L.workspace(1000, CPU)
        assert w1.numel() == 1000 and w1.data_ptr() % 512 == 0 and int(w1[0]) == 0x7B
        w1[:] = 0x11                                        # what a kernel leaves behind
        w2 = L.workspace(600, CPU)                          # the next call: same origin, shorter, inherits
        assert w2.data_ptr() == w1.data_ptr() and int(w2[599]) == 0x11
        assert int(w1[600]) == 0xFF                         # the temporary guard begins at the very next byte
        w2[:] = 0x22
    a1.check()
    with guarded(fill=0xFF, stale=pool) as a2:              # the pool outlives the arena
        w3 = L.workspace(5000, CPU)                         # grows: keeps what the smaller buffer held
        assert [int(w3[i]) for i in (0, 599, 600, 999, 1000, 4999)] == [0x22, 0x22, 0x11, 0x11, 0x7B, 0x7B]
        w3[4990:] = 0x33
        w4 = L.workspace(4995, CPU)
        w4.data_ptr()
        a2.records[-1].trail[1] = 0x05                      # one byte past the end of the 4995-byte view
    with pytest.raises(GuardDamaged, match=r"stale workspace of 4995 bytes.*offset \+1 from the payload end"):
        a2.check()
    with guarded(stale=pool) as a3:
        w5 = L.workspace(5000, CPU)
        assert [int(w5[i]) for i in (4989, 4990, 4994, 4995, 4996, 4999)] == [0x7B, 0x33, 0x33, 0x33, 0x33, 0x33]  # bytes put back
    a3.check()


def test_the_arena_refuses_to_activate_while_a_stream_captures(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    real_ws = L.workspace
    with pytest.raises(RuntimeError, match="capture"):
        with guarded():
            pass
    assert all(m.torch is torch for m in _modules()) and L.workspace is real_ws and G.current() is None

