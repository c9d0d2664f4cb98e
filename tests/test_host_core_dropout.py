"""Host-side checks of the fused component dropout (no GPU needed): the entry points are declared, exported and bound,
they validate their arguments before any launch, the Python restatement of the mask definition meets Philox4x32-10's
known answers, and the opt-in on the model leaves the checkpoint format alone."""
import math
import os
import re
import subprocess

import pytest
import torch

from dctn_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dctn_core_dropout_state_bytes", "dctn_core_dropout_fwd", "dctn_core_dropout_bwd", "dctn_core_dropout_mask")


def test_new_entry_points_are_in_header_library_and_bindings():
    header = open(os.path.join(ROOT, "include", "dctn_amd.h")).read()
    declared = set(re.findall(r"\b(dctn_[a-z0-9_]+)\s*\(", header))
    exported = set()
    for line in subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True,
                               check=True).stdout.splitlines():
        parts = line.split()
        if len(parts) == 3 and parts[1] == "T":
            exported.add(parts[2])
    for name in NEW:
        assert name in declared, f"{name} is not declared in include/dctn_amd.h"
        assert name in exported, f"{name} is not exported by {_lib.LIB_PATH}"
        assert name in _lib.SIGNATURES, f"{name} is missing from _lib.SIGNATURES"


def test_version_and_state_block_size():
    assert _lib.lib().dctn_version() >= 502
    assert _lib.lib().dctn_core_dropout_state_bytes() == 16
    header = open(os.path.join(ROOT, "include", "dctn_amd.h")).read()
    assert "dctn_core_dropout_state_bytes() = 16" in header


def test_entry_points_validate_their_arguments_without_a_device():
    L = _lib
    fwd, bwd, mask = L.lib().dctn_core_dropout_fwd, L.lib().dctn_core_dropout_bwd, L.lib().dctn_core_dropout_mask

    def ptrs(n, value=64):
        return (L.c_void * n)(*[value] * n)

    one = L.i64_array([4])
    assert fwd(ptrs(1), ptrs(1), one, 1, None, 64, 64, L.F32, None) == L.ERR_NULL          # p
    assert fwd(ptrs(1), ptrs(1), one, 1, 64, None, 64, L.F32, None) == L.ERR_NULL          # state
    assert fwd(ptrs(1), ptrs(1), one, 1, 64, 64, None, L.F32, None) == L.ERR_NULL          # record
    assert fwd(ptrs(1, None), ptrs(1), one, 1, 64, 64, 64, L.F32, None) == L.ERR_NULL      # a core
    assert mask(ptrs(1, None), one, 1, 64, 64, L.F32, None) == L.ERR_NULL
    assert bwd(ptrs(1, None), ptrs(1), one, 1, 64, 64, L.F32, None) == L.ERR_NULL          # d_out without d_core's twin
    assert fwd(ptrs(1), ptrs(1), one, 0, 64, 64, 64, L.F32, None) == L.ERR_BAD_SHAPE
    assert fwd(ptrs(9), ptrs(9), L.i64_array([4] * 9), 9, 64, 64, 64, L.F32, None) == L.ERR_UNSUPPORTED
    assert mask(ptrs(9), L.i64_array([4] * 9), 9, 64, 64, L.F32, None) == L.ERR_UNSUPPORTED
    assert fwd(ptrs(1), ptrs(1), one, 1, 64, 64, 64, 7, None) == L.ERR_BAD_DTYPE
    for bad in (0, -1, 1 << 34, 1 << 40):   # e >> 2 is one 32-bit counter word: cores stay below 2^34 elements
        n = L.i64_array([bad])
        assert fwd(ptrs(1), ptrs(1), n, 1, 64, 64, 64, L.BF16, None) == L.ERR_BAD_SHAPE, bad
        assert bwd(ptrs(1), ptrs(1), n, 1, 64, 64, L.F64, None) == L.ERR_BAD_SHAPE, bad
        assert mask(ptrs(1), n, 1, 64, 64, L.F32, None) == L.ERR_BAD_SHAPE, bad


KNOWN_ANSWERS = (   # Philox4x32-10 (Random123's known-answer vectors)
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
)


@pytest.mark.parametrize("counter,key,want", KNOWN_ANSWERS)
def test_philox_known_answers(counter, key, want):
    from dctn_amd.dropout import philox4x32_10

    assert " ".join(f"{w:08x}" for w in philox4x32_10(counter, key)) == want


def test_expected_keep_uses_the_documented_counter_layout():
    from dctn_amd.dropout import expected_keep, keep_threshold, philox4x32_10

    seed, draw, seg = (0x299F31D0 << 32) | 0xA4093822, 0x13198A2E, 0x03707344
    keep = expected_keep(seed, draw, seg, 11, 0.5)   # the last block is partial: 3 elements
    assert len(keep) == 11
    for e in range(11):
        # counter = (e >> 2, 0, draw, segment), key = (seed & 0xFFFFFFFF, seed >> 32), word e & 3
        w = philox4x32_10((e >> 2, 0, draw, seg), (0xA4093822, 0x299F31D0))[e & 3]
        assert keep[e] == (w < (1 << 31))
    assert keep_threshold(1.0) == (1 << 32) - 1 and keep_threshold(0.8984375) == 0xE6000000
    assert keep_threshold(float(torch.tensor(0.9, dtype=torch.bfloat16))) == 0xE6000000


@pytest.mark.parametrize("p,kept", [(0.5, 9906), (0.9, 17937), (0.25, 4936)])
def test_keep_rate(p, kept):
    from dctn_amd.dropout import expected_keep

    n = 20_000
    got = sum(expected_keep(0x0123456789ABCDEF, 3, 0, n, p))
    print(f"p={p}: kept {got} of {n}, {(got - n * p) / math.sqrt(n * p * (1 - p)):+.2f} sigma")
    assert abs(got - n * p) <= 5 * math.sqrt(n * p * (1 - p))
    assert got == kept


def _cpu_model(p=0.5):
    from dctn_amd.eps_plus_linear import EPSesPlusLinear, UnitTheoreticalOutputStd

    torch.manual_seed(0)
    return EPSesPlusLinear(((3, 4), (2, 3)), UnitTheoreticalOutputStd(), p, torch.device("cpu"), torch.float32, image_size=10)


def test_use_fused_dropout_raises_for_a_cpu_model():
    m = _cpu_model()
    with pytest.raises(RuntimeError, match="MI355X"):
        m.use_fused_dropout(7)
    with pytest.raises(RuntimeError, match="use_fused_dropout"):
        m.dropout_state_dict()


def test_use_fused_dropout_leaves_the_state_dict_keys_alone():
    from dctn_amd import dropout

    m = _cpu_model()
    keys = set(m.state_dict())
    assert keys == {"p", "epses.0", "epses.1", "linear.weight", "linear.bias"}
    assert [name for name, _ in m.named_buffers()] == ["p"]
    with pytest.raises(RuntimeError):
        m.use_fused_dropout(7)
    assert set(m.state_dict()) == keys
    # what use_fused_dropout installs on a GPU model, placed on the CPU here: a buffer (so `.to()` and the broadcast of
    # the buffers carry it) that stays out of the state_dict
    m._dropout_state = dropout.new_state(0xFEDCBA9876543210, torch.device("cpu"), draws_done=5)
    assert set(m.state_dict()) == keys
    assert sorted(name for name, _ in m.named_buffers()) == ["_dropout_state", "p"]
    assert m.dropout_state_dict() == {"seed": 0xFEDCBA9876543210, "draws_done": 5}
    m.load_dropout_state_dict({"seed": 3, "draws_done": 4_000_000_000})
    assert m.dropout_state_dict() == {"seed": 3, "draws_done": 4_000_000_000}
    assert m._dropout_state.dtype == torch.int32 and m._dropout_state.tolist()[3] == 0
    m2 = _cpu_model()
    m2.load_state_dict(m.state_dict())   # checkpoints interchange with a model that never opted in
