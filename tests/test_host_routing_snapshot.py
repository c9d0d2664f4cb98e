"""Host-only: every dispatch query answers what the commit before the routing refactor answered.

tests/golden/routing_parent.npz was recorded from that commit's library by tests/golden/make_routing_parent.py (which
also defines the cases); here the library under test answers the same queries.  A family, a saved-buffer size or a
workspace size that moves is a behaviour change: the buffer-contract tests hand the kernels exactly these sizes."""
import numpy as np
import pytest

from dctn_amd import _lib
from tests.golden import make_routing_parent as M

RECORD = np.load(M.RECORD)
COLUMNS = "family, saved, fwd ws, stats ws, bwd ws (dx, dcore) = (1,1), (1,0), (0,1), head bwd ws"


@pytest.fixture(scope="module")
def lib():
    handle = _lib.lib()
    limits, recorded = M.device_limits(handle), RECORD["device_limits"].tolist()
    if limits != recorded:
        pytest.skip(f"the plans depend on the device: recorded for {recorded} (CUs, LDS bytes), this one is {limits}")
    return handle


def test_record_comes_from_a_named_commit_and_reaches_every_family():
    assert len(str(RECORD["parent_commit"])) == 40
    assert int(RECORD["eps_families"].sum()) == len(list(M.eps_grid())) * len(M.DTYPES) * len(M.POLICIES)
    assert (RECORD["eps_families"].sum(0)[1:] > 0).all()   # families 0 .. 5 somewhere in the whole grid
    committed = set(RECORD["eps_rows"][:, 3].tolist()) | set(RECORD["eps_extra"][:, 0].tolist())
    assert committed == {-1, 0, 1, 2, 3, 4, 5}


def test_committed_eps_rows_one_by_one(lib):
    grid = list(M.eps_grid())
    assert len(RECORD["eps_rows"]) > 6000
    for dtype, policy, i, *row in RECORD["eps_rows"].tolist():
        assert M.eps_row(lib, grid[i], dtype, policy) == row, (grid[i], dtype, policy, COLUMNS)
    for (shape, dtype, policy), row in zip(M.EPS_EXTRA, RECORD["eps_extra"].tolist(), strict=True):
        assert M.eps_row(lib, shape, dtype, policy) == row, (shape, dtype, policy, COLUMNS)


def test_whole_eps_grid_by_bucket_digest(lib):
    buckets = M.eps_buckets(lib)
    assert list(buckets) == [tuple(b) for b in RECORD["eps_buckets"].tolist()]
    for n, (key, (digest, hist, _)) in enumerate(buckets.items()):
        assert hist == RECORD["eps_families"][n].tolist(), f"rows per family of (dtype, policy) = {key}"
        assert digest == str(RECORD["eps_sha256"][n]), f"a row of (dtype, policy) = {key} outside the committed ones moved"


def test_convsbs_queries(lib):
    rows = M.sbs_rows(lib)
    assert list(rows) == RECORD["sbs_names"].tolist()
    for name, row in rows.items():
        assert row == RECORD[f"sbs_{name}"].tolist(), name
