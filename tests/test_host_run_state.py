"""Host checks (no GPU) of the whole-run snapshots: the digest and the arena layout in plain Python, the file format and
its error messages, the entry points' validation codes (decided on the host before any launch) and the header."""
import ctypes
import json
import os
import re
import struct

import numpy as np
import pytest

from dctn_amd import _lib
from dctn_amd import checkpoint as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("dctn_state_max_regions", "dctn_state_arena_bytes", "dctn_state_gather", "dctn_state_scatter")


def _loop_digest(raw: bytes):
    """The definition as a plain loop over padded words."""
    padded = raw + b"\0" * (-len(raw) % 16)
    s1 = s2 = 0
    for i in range(len(padded) // 4):
        w = int.from_bytes(padded[4 * i: 4 * i + 4], "little")
        s1 = (s1 + w) % (1 << 64)
        s2 = (s2 + (i + 1) * w) % (1 << 64)
    return s1, s2


# ------------------------------------------------------------------ digest and layout
def test_digest_of_a_hand_computed_case():
    # bytes 01 00 00 00 | 02 00 00 00 | ff ff ff ff | 05 (+ 3 zero bytes): words 1, 2, 0xFFFFFFFF, 5
    raw = bytes([1, 0, 0, 0, 2, 0, 0, 0, 0xFF, 0xFF, 0xFF, 0xFF, 5])
    assert C.digest(raw) == (1 + 2 + 0xFFFFFFFF + 5, 1 * 1 + 2 * 2 + 3 * 0xFFFFFFFF + 4 * 5)
    assert C.digest(raw) == (4294967303, 12884901910)
    assert C.digest(b"") == (0, 0) and C.digest(b"\0" * 40) == (0, 0)
    assert C.digest(np.array([1, 2], dtype="<u4")) == (3, 5)


def test_digest_wraps_at_two_to_the_64():
    n = 1 << 17   # 2^17 words of 0xFFFFFFFF: s2 = (2^32 - 1) * n (n + 1) / 2 passes 2^64
    raw = b"\xff" * (4 * n)
    want = ((0xFFFFFFFF * n) % (1 << 64), (0xFFFFFFFF * (n * (n + 1) // 2)) % (1 << 64))
    assert 0xFFFFFFFF * (n * (n + 1) // 2) >= 1 << 64
    assert C.digest(raw) == want


@pytest.mark.parametrize("n", range(34))
def test_digest_of_short_buffers_equals_the_plain_loop(n):
    raw = np.random.default_rng(100 + n).integers(0, 256, n, dtype=np.uint8).tobytes()
    assert C.digest(raw) == _loop_digest(raw)
    assert C.digest(np.frombuffer(raw, dtype=np.uint8)) == _loop_digest(raw)


def test_arena_offsets_round_every_length_up_to_16():
    assert C.arena_layout([1, 15, 16, 17]) == ([0, 16, 32, 48], 80)
    assert C.arena_layout([17, 1]) == ([0, 32], 48)
    with pytest.raises(ValueError):
        C.arena_layout([4, 0])
    lib = _lib.lib()
    for lengths in ([1, 15, 16, 17], [17], [4095, 4096, 4097, (1 << 20) + 5]):
        assert lib.dctn_state_arena_bytes(_lib.i64_array(lengths), len(lengths)) == C.arena_layout(lengths)[1]


# ------------------------------------------------------------------ the file
def _arrays():
    rng = np.random.default_rng(7)
    return {"a.flat": rng.standard_normal(37).astype(np.float32), "b.block": np.arange(4, dtype=np.int32),
            "c.bytes": rng.integers(0, 256, (3, 11), dtype=np.uint8), "d.wide": rng.standard_normal(5)}


def _expected(arrays):
    return [(name, a.dtype.name, a.shape) for name, a in arrays.items()]


def test_file_round_trip_from_numpy_buffers(tmp_path):
    arrays, path = _arrays(), str(tmp_path / "run.dctn")
    C.save_arrays(path, arrays, host={"optimizer": {"lr": 1e-3, "max_norm": float("inf")}}, extras={"num_iters_done": 41})
    raw = open(path, "rb").read()
    assert raw[:8] == b"DCTNRUN1"
    (length,) = struct.unpack("<Q", raw[8:16])
    manifest = json.loads(raw[16: 16 + length].decode("utf-8"))
    start = -(-(16 + length) // 4096) * 4096
    assert set(raw[16 + length: start]) <= {0} and len(raw) == start + manifest["arena_bytes"]
    assert manifest["format"] == 1 and manifest["extras"] == {"num_iters_done": 41}
    assert manifest["host"]["optimizer"] == {"lr": 1e-3, "max_norm": float("inf")}
    assert [r["offset"] for r in manifest["regions"]] == C.arena_layout([a.nbytes for a in arrays.values()])[0]
    for r, (name, a) in zip(manifest["regions"], arrays.items()):
        assert (r["name"], r["dtype"], tuple(r["shape"]), r["bytes"]) == (name, a.dtype.name, a.shape, a.nbytes)
        assert (r["s1"], r["s2"]) == _loop_digest(a.tobytes())
        body = raw[start + r["offset"]: start + r["offset"] + -(-r["bytes"] // 16) * 16]
        assert body[: r["bytes"]] == a.tobytes() and set(body[r["bytes"]:]) <= {0}
    got_manifest, got = C.load_arrays(path, _expected(arrays))
    assert got_manifest == manifest and list(got) == list(arrays)
    for name, a in arrays.items():
        assert got[name].dtype == a.dtype and np.array_equal(got[name], a)
    assert not [f for f in os.listdir(tmp_path) if f != "run.dctn"]   # the temporary name is gone


def test_a_damaged_file_is_refused_and_the_message_names_what_is_wrong(tmp_path):
    arrays, path = _arrays(), str(tmp_path / "run.dctn")
    C.save_arrays(path, arrays)
    raw = open(path, "rb").read()
    manifest, _ = C.read_file(path)
    start = len(raw) - manifest["arena_bytes"]

    def write(data):
        bad = str(tmp_path / "bad.dctn")
        open(bad, "wb").write(data)
        return bad

    with pytest.raises(ValueError, match="truncated.*arena"):
        C.load_arrays(write(raw[:-5]))
    with pytest.raises(ValueError, match="truncated.*manifest"):
        C.load_arrays(write(raw[:40]))
    with pytest.raises(ValueError, match="truncated"):
        C.load_arrays(write(raw[:7]))
    with pytest.raises(ValueError, match="wrong magic"):
        C.load_arrays(write(b"DCTNRUN2" + raw[8:]))
    # one flipped byte in the arena, inside region c.bytes
    at = start + manifest["regions"][2]["offset"] + 5
    flipped = raw[:at] + bytes([raw[at] ^ 0x10]) + raw[at + 1:]
    with pytest.raises(ValueError, match="'c.bytes' is damaged"):
        C.load_arrays(write(flipped), _expected(arrays))
    # a flipped padding byte is not part of any region
    pad = start + manifest["regions"][0]["offset"] + manifest["regions"][0]["bytes"]
    C.load_arrays(write(raw[:pad] + b"\x01" + raw[pad + 1:]), _expected(arrays))
    # an entry renamed / reshaped / retyped against the live run
    want = _expected(arrays)
    with pytest.raises(ValueError, match="'b.block' in the file, 'b.renamed' in the run"):
        C.load_arrays(path, [want[0], ("b.renamed",) + want[1][1:]] + want[2:])
    with pytest.raises(ValueError, match=r"'c.bytes' has shape \[3, 11\] in the file, \[11, 3\] in the run"):
        C.load_arrays(path, want[:2] + [("c.bytes", "uint8", (11, 3))] + want[3:])
    with pytest.raises(ValueError, match="'a.flat' is float32 in the file, float64 in the run"):
        C.load_arrays(path, [("a.flat", "float64", (37,))] + want[1:])
    with pytest.raises(ValueError, match="'e.more' is missing"):
        C.load_arrays(path, want + [("e.more", "int32", (1,))])
    with pytest.raises(ValueError, match="'d.wide' of the file is not part of the run"):
        C.load_arrays(path, want[:3])


def test_read_model_state_finds_the_entries_inside_the_regions(tmp_path):
    import torch

    flat = np.arange(10, dtype=np.float32)
    entries = [("optimizer.flat", "float32", (10,)), ("model.p", "float32", ())]
    p = np.array(0.9, dtype=np.float32)
    model = [dict(key="epses.0", region="optimizer.flat", offset=0, dtype="float32", shape=[2, 3]),
             dict(key="linear.bias", region="optimizer.flat", offset=24, dtype="float32", shape=[4]),
             dict(key="p", region="model.p", offset=0, dtype="float32", shape=[])]
    manifest = C.build_manifest(entries, [C.digest(flat), C.digest(p.tobytes())], model=model)
    arena = np.zeros(manifest["arena_bytes"], dtype=np.uint8)
    arena[:40] = flat.view(np.uint8)
    arena[48:52] = np.frombuffer(p.tobytes(), dtype=np.uint8)
    path = str(tmp_path / "m.dctn")
    C.write_file(path, manifest, arena)
    state = C.read_model_state(path)
    assert list(state) == ["epses.0", "linear.bias", "p"]
    assert torch.equal(state["epses.0"], torch.arange(6, dtype=torch.float32).reshape(2, 3))
    assert torch.equal(state["linear.bias"], torch.arange(6, 10, dtype=torch.float32))
    assert state["p"].shape == () and float(state["p"]) == float(p)


# ------------------------------------------------------------------ the C-ABI
def test_entry_points_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "dctn_amd.h")).read()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header), f"{name} is not declared in include/dctn_amd.h"
        assert name in _lib.SIGNATURES, f"{name} is missing from _lib.SIGNATURES"
    assert "run_state.hip" in open(os.path.join(ROOT, "dctn_amd", "csrc", "Makefile")).read()
    assert _lib.lib().dctn_version() >= 508
    assert _lib.lib().dctn_state_max_regions() == 16 == C.MAX_REGIONS


def test_argument_validation_happens_on_the_host():
    """Every code is decided before any launch, so fake non-null pointers do (tests/test_host_logic.py does the same)."""
    lib = _lib.lib()
    ptrs = lambda *v: (ctypes.c_void_p * len(v))(*v)   # noqa: E731
    i64 = _lib.i64_array
    one, n = ptrs(64), i64([20])
    # NULL: the table, the lengths, an entry, the arena, the digests
    assert lib.dctn_state_gather(None, n, 1, 4096, 32, 8192, None) == _lib.ERR_NULL
    assert lib.dctn_state_gather(one, None, 1, 4096, 32, 8192, None) == _lib.ERR_NULL
    assert lib.dctn_state_gather(ptrs(64, None), i64([20, 4]), 2, 4096, 48, 8192, None) == _lib.ERR_NULL
    assert lib.dctn_state_gather(one, n, 1, None, 32, 8192, None) == _lib.ERR_NULL
    assert lib.dctn_state_gather(one, n, 1, 4096, 32, None, None) == _lib.ERR_NULL
    assert lib.dctn_state_scatter(None, one, n, 1, 8192, None) == _lib.ERR_NULL
    assert lib.dctn_state_scatter(4096, None, n, 1, 8192, None) == _lib.ERR_NULL
    assert lib.dctn_state_scatter(4096, ptrs(None), n, 1, 8192, None) == _lib.ERR_NULL
    # BAD_SHAPE: no regions, an empty region, an arena size that is not exactly the padded sum
    assert lib.dctn_state_gather(one, n, 0, 4096, 32, 8192, None) == _lib.ERR_BAD_SHAPE
    assert lib.dctn_state_gather(one, i64([0]), 1, 4096, 0, 8192, None) == _lib.ERR_BAD_SHAPE
    assert lib.dctn_state_scatter(4096, one, i64([-4]), 1, 8192, None) == _lib.ERR_BAD_SHAPE
    for wrong in (20, 31, 33, 48):
        assert lib.dctn_state_gather(one, n, 1, 4096, wrong, 8192, None) == _lib.ERR_BAD_SHAPE
    # UNSUPPORTED: more than 16 regions, an address that is no multiple of 4
    many = ptrs(*([64] * 17))
    assert lib.dctn_state_gather(many, i64([4] * 17), 17, 4096, 16 * 17, 8192, None) == _lib.ERR_UNSUPPORTED
    assert lib.dctn_state_scatter(4096, many, i64([4] * 17), 17, 8192, None) == _lib.ERR_UNSUPPORTED
    for odd in (65, 66, 67):
        assert lib.dctn_state_gather(ptrs(odd), n, 1, 4096, 32, 8192, None) == _lib.ERR_UNSUPPORTED
        assert lib.dctn_state_scatter(4096, ptrs(64, odd), i64([20, 4]), 2, 8192, None) == _lib.ERR_UNSUPPORTED
    # the size query: the padded sum, 0 for a table it cannot describe
    assert lib.dctn_state_arena_bytes(i64([1, 15, 16, 17]), 4) == 80
    assert lib.dctn_state_arena_bytes(None, 1) == 0 and lib.dctn_state_arena_bytes(i64([4]), 0) == 0
    assert lib.dctn_state_arena_bytes(i64([4, 0]), 2) == 0 and lib.dctn_state_arena_bytes(i64([4] * 17), 17) == 0


def test_a_torch_optimizer_is_refused_with_the_reason():
    import torch

    model = torch.nn.Linear(3, 2)
    with pytest.raises(TypeError, match="fixed|FIXED"):
        C.RunState(model, torch.optim.Adam(model.parameters()))


def test_train_counts_from_first_iter():
    import inspect

    from dctn_amd import training

    assert inspect.signature(training.train).parameters["first_iter"].default == 0
    import dctn.checkpoint

    assert dctn.checkpoint is C
