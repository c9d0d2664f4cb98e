"""Host-side checks of the device batch source (no GPU needed): the Python restatement of the epoch order meets the known
answers and is a bijection, the entry points are declared, exported and bound, they validate their arguments before any
launch, and the batch arithmetic of `DeviceBatches` (steps per epoch, shards, errors) is what the header states."""
import os
import re
import subprocess

import pytest
import torch

from dctn_amd import _lib
from dctn_amd import batches as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dctn_batch_state_bytes", "dctn_batch_draw", "dctn_batch_gather")
SEED = 0x1234567890ABCDEF


def test_round_keys_known_answer():
    assert " ".join(f"{k:08x}" for k in B.round_keys(SEED, 3)) == "cfdc7eb1 620a8e7f f889c7d3 b9627ffb 66808ef0 fbab6a68"
    assert B.TAG == 0x53485546


@pytest.mark.parametrize("n,first", [(10, [7, 3, 0, 1, 8, 9, 4, 5]), (1000, [176, 606, 381, 213, 539, 788, 444, 234]),
                                     (50000, [34113, 6073, 8814, 11441, 18111, 13, 905, 39356])])
def test_order_known_answers(n, first):
    assert [B.order_at(SEED, 3, n, i) for i in range(8)] == first
    assert B.order(SEED, 3, n)[:8] == first


def test_whole_orders_at_the_ends_of_the_seed_and_epoch_ranges():
    assert B.order(0, 0, 12) == [1, 5, 3, 9, 6, 11, 4, 2, 10, 8, 7, 0]
    assert B.order((1 << 64) - 1, (1 << 32) - 1, 12) == [4, 0, 3, 1, 7, 11, 2, 9, 6, 10, 8, 5]


@pytest.mark.parametrize("n", [1, 2, 3, 5, 37, 257, 1000, 1025, 4097])
def test_order_is_a_bijection(n):
    for epoch in (0, 1):
        assert sorted(B.order(SEED, epoch, n)) == list(range(n))


def test_order_differs_between_epochs():
    assert B.order(SEED, 0, 1000) != B.order(SEED, 1, 1000)


def test_one_pass_is_a_bijection_on_the_power_of_two_range():
    K = B.round_keys(SEED, 0)
    for b in (2, 3, 6, 11):   # even and odd widths: the halves swap widths every round
        assert sorted(B.perm_once(v, b, K) for v in range(1 << b)) == list(range(1 << b))


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


def test_version_state_block_size_and_constants():
    assert _lib.lib().dctn_version() >= 503
    assert _lib.lib().dctn_batch_state_bytes() == 16
    header = open(os.path.join(ROOT, "include", "dctn_amd.h")).read()
    assert "dctn_batch_state_bytes() = 16" in header
    enums = dict(re.findall(r"DCTN_(BATCH_[A-Z0-9_]+)\s*=\s*(\d+)", header))
    assert {k: int(v) for k, v in enums.items()} == {"BATCH_SRC_U8_TABLE": _lib.BATCH_SRC_U8_TABLE,
                                                     "BATCH_SRC_ROWS": _lib.BATCH_SRC_ROWS,
                                                     "BATCH_SRC_COLOUR": _lib.BATCH_SRC_COLOUR,
                                                     "BATCH_IDENTITY_ORDER": _lib.BATCH_IDENTITY_ORDER}


def test_entry_points_validate_their_arguments_without_a_device():
    L = _lib
    draw, gather = L.lib().dctn_batch_draw, L.lib().dctn_batch_gather
    U8, ROWS = L.BATCH_SRC_U8_TABLE, L.BATCH_SRC_ROWS
    P = 64   # any non-null address: nothing is launched

    def d(src=P, table=P, labels=P, x=P, y=P, idx=P, state=P, n=37, G=8, Bl=8, off=0, row=25, width=2, kind=U8, flags=0,
          dtype=L.F32):
        return draw(src, table, labels, x, y, idx, state, n, G, Bl, off, row, width, kind, flags, dtype, None)

    def g(src=P, table=P, labels=P, sample=P, x=P, y=P, idx=P, n=37, count=8, row=25, width=2, kind=U8, dtype=L.F32):
        return gather(src, table, labels, sample, x, y, idx, n, count, row, width, kind, dtype, None)

    for name in ("src", "table", "labels", "x", "y", "idx", "state"):
        assert d(**{name: None}) == L.ERR_NULL, name
    for name in ("src", "table", "labels", "sample", "x", "y", "idx"):
        assert g(**{name: None}) == L.ERR_NULL, name
    assert d(n=0) == L.ERR_BAD_SHAPE and g(n=0) == L.ERR_BAD_SHAPE
    assert d(n=1 << 31, G=8) == L.ERR_BAD_SHAPE and g(n=1 << 31) == L.ERR_BAD_SHAPE
    assert d(n=7, G=8) == L.ERR_BAD_SHAPE                     # G > n
    assert d(G=0, Bl=0) == L.ERR_BAD_SHAPE
    assert d(Bl=0) == L.ERR_BAD_SHAPE and g(count=0) == L.ERR_BAD_SHAPE
    assert d(Bl=4, off=5) == L.ERR_BAD_SHAPE                  # the shard ends beyond the global batch
    assert d(Bl=4, off=-1) == L.ERR_BAD_SHAPE
    assert d(row=0) == L.ERR_BAD_SHAPE and g(width=0) == L.ERR_BAD_SHAPE
    assert d(kind=2) == L.ERR_BAD_SHAPE and g(kind=-1) == L.ERR_BAD_SHAPE
    assert d(flags=2) == L.ERR_BAD_SHAPE
    assert d(width=5) == L.ERR_UNSUPPORTED and g(width=5) == L.ERR_UNSUPPORTED            # Q = 5
    assert d(width=5, kind=ROWS, table=None) == L.ERR_UNSUPPORTED                         # C = 5
    assert d(dtype=7) == L.ERR_BAD_DTYPE and g(dtype=3) == L.ERR_BAD_DTYPE


def test_kernel_names_come_from_a_table():
    """tests/test_host_buffer_contract.py asks for a GUARDED entry for every LITERAL name in a dctn_set_last_kernel call;
    the batch kernels report theirs through a table, and tests/test_gpu_batches.py holds them to the contract.  The
    table and its one call are batch_call.hip's, for all three kernel files."""
    assert "dctn_set_last_kernel" not in open(os.path.join(ROOT, "dctn_amd", "csrc", "batch_source.hip")).read()
    src = open(os.path.join(ROOT, "dctn_amd", "csrc", "batch_call.hip")).read()
    calls = re.findall(r"dctn_set_last_kernel\((.*?)\);", src, re.S)
    assert calls == ["BATCH_KERNEL_NAMES[draw ? 0 : 1][c->augment ? 1 : 0][c->src_kind][c->dtype]"]
    assert len(re.findall(r'"([a-z0-9_]+)"', src)) == 24   # (the table holds nothing but today's 12 + 6 + 6 names)
    names = set(re.findall(r'"(batch_[a-z0-9_]+)"', src))
    assert names == {f"batch_{op}_{kind}_{dt}" for op in ("draw", "gather") for kind in ("u8", "rows")
                     for dt in ("f32", "f64", "bf16")}


# ------------------------------------------------------------------ the arithmetic of a source
def test_steps_per_epoch_and_shards():
    assert B.steps_per_epoch(37, 8) == 4 and B.steps_per_epoch(37, 8, drop_last=False) == 5
    assert B.steps_per_epoch(1000, 1000) == 1 and B.steps_per_epoch(40, 8, drop_last=False) == 5
    with pytest.raises(ValueError):
        B.steps_per_epoch(7, 8)                # S >= 1
    with pytest.raises(ValueError):
        B.steps_per_epoch(7, 0)
    assert B.local_batch(8, 1, 2) == 4
    with pytest.raises(ValueError):
        B.local_batch(9, 0, 2)                 # the global batch must divide over the ranks
    with pytest.raises(ValueError):
        B.local_batch(8, 2, 2)


def test_expected_indices_follow_the_counter_through_the_epochs():
    n, G, S = 37, 8, 4
    for k in (0, 3, 4, 9):
        epoch, first = k // S, (k % S) * G
        want = B.order(SEED, epoch, n)[first : first + G]
        assert B.expected_indices(SEED, k, n, G) == want
        halves = [B.expected_indices(SEED, k, n, G, rank=r, world=2) for r in range(2)]
        assert halves[0] + halves[1] == want and len(halves[0]) == 4
        assert B.expected_indices(SEED, k, n, G, shuffle=False) == list(range(first, first + G))
    seen = sum((B.expected_indices(SEED, k, n, G) for k in range(S)), [])
    assert len(set(seen)) == 32                                     # one epoch: 32 distinct samples, 5 dropped
    assert B.expected_indices(SEED, 4, n, G) == B.order(SEED, 1, n)[:8]


def test_feature_table_is_the_reference_formulation_per_intensity():
    from dctn_amd.window_stats import φ_cos_sin_squared_1 as phi

    g = torch.Generator().manual_seed(0)
    images = torch.randint(0, 256, (6, 5, 7), dtype=torch.uint8, generator=g)
    scale = 1.46
    for dtype in (torch.float32, torch.bfloat16, torch.float64):
        table = B.feature_table(phi, scale, dtype)
        assert table.shape == (256, 2) and table.dtype == dtype
        # dctn/dataset_loading.py:60-63 and the runner's `x *= scale`, on the whole tensor
        full = (torch.stack(tuple(f(images.float() / 255.0) for f in phi), dim=3) * scale).to(dtype)
        assert torch.equal(table[images.long()], full)


def test_constructor_arithmetic_errors_come_before_the_device():
    images = torch.zeros(37, 5, 5, dtype=torch.uint8)
    labels = torch.zeros(37, dtype=torch.int64)
    kw = dict(dtype=torch.float32, seed=1)
    with pytest.raises(ValueError):
        B.DeviceBatches(images, labels, 38, **kw)                            # S = 0
    with pytest.raises(ValueError):
        B.DeviceBatches(images, labels, 9, rank=0, world=2, **kw)            # 9 does not divide over 2 ranks
    with pytest.raises(ValueError):
        B.DeviceBatches(images, labels[:5], 8, **kw)
    with pytest.raises(ValueError):
        B.DeviceBatches(images, labels, 8, shuffle=True, drop_last=False, **kw)
    with pytest.raises(ValueError):
        B.DeviceBatches(images, labels, 8, dtype=torch.float32, seed=1 << 64)
    with pytest.raises(TypeError):
        B.DeviceBatches(images.float(), labels, 8, **kw)                     # float intensities: from_features
    with pytest.raises(TypeError):
        B.DeviceBatches(images, labels, 8, dtype=torch.float16, seed=1)
    with pytest.raises(NotImplementedError):
        B.DeviceBatches.from_features(torch.zeros(5, 37, 3), labels, 8, seed=1)


@pytest.mark.skipif(torch.cuda.is_available(), reason="with a GPU the source is built (tests/test_gpu_batches.py)")
def test_a_source_without_a_gpu_raises():
    images = torch.zeros(37, 5, 5, dtype=torch.uint8)
    labels = torch.zeros(37, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        B.DeviceBatches(images, labels, 8, dtype=torch.float32, seed=1)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        B.DeviceBatches.from_features(torch.zeros(1, 37, 5, 5, 2), labels, 8, seed=1)


def test_graphed_train_step_keeps_its_signature():
    import inspect

    from dctn_amd.training import GraphedTrainStep

    params = inspect.signature(GraphedTrainStep.__init__).parameters
    assert list(params)[-1] == "batch_source" and params["batch_source"].default is None
