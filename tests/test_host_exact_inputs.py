"""Host checks of the exact-input regime (tests/exact_inputs.py): the budgets hold, the one-hot closed form is the
oracle, the expected values see every window, and every kernel name the library can report has an exact GPU test."""
import ast
import glob
import os
import re

import pytest
import torch

from oracle import ref_cpu as R
from tests import exact_inputs as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SNAKE9 = ((0, 0), (0, 1), (0, 2), (1, 2), (1, 1), (1, 0), (2, 0), (2, 1), (2, 2))


@pytest.mark.parametrize("C,K,Q,O,B,H,W,halves", [(1, 3, 2, 4, 5, 10, 10, False), (2, 2, 2, 4, 3, 9, 7, False),
                                                   (1, 2, 3, 5, 4, 7, 8, True), (1, 4, 2, 4, 2, 9, 8, True),
                                                   (1, 2, 8, 5, 3, 9, 10, True)])
def test_eps_budgets_hold_for_small_cases(C, K, Q, O, B, H, W, halves):
    x = X.pixels(C, B, H, W, Q, seed=B + H, halves=halves)
    core = X.eps_core(Q, K * K * C, O, seed=B + H + 1)
    dy = X.small_ints((B, H - K + 1, W - K + 1, O), seed=B + H + 2, vmax=3, nonzero=True)
    mags = X.eps_mags(core, x, dy)
    report = X.check_budget(mags, torch.float32, None if halves else X.eps_bf16_intermediates(core, x, dy, "halves"))
    assert 0 < report["dcore"] <= X.F32_UNITS
    X.assert_every_window_counts(X.eps_window_weights(x, K, dy))
    # the grid: every x entry is 0 or 2^-k (k <= 1), two ones per pixel at most
    assert set(x.unique().tolist()) <= {0.0, 0.5, 1.0} and int((x != 0).sum(-1).max()) <= 2
    # the oracle in float32 on the same inputs equals float64: nothing rounds inside the budget
    assert torch.equal(R.eps_4step(core.float(), x.float()).double(), R.eps_4step(core, x))


def test_budget_check_refuses_what_does_not_fit():
    with pytest.raises(AssertionError, match="budget"):
        X.check_budget({"dcore": torch.tensor([2.0 ** 24 + 1], dtype=torch.float64)}, torch.float32)
    with pytest.raises(AssertionError, match="bf16 budget"):
        X.check_budget({}, torch.float32, {"Z": 257.0})
    with pytest.raises(AssertionError, match="grid"):
        X.grid_exponent(torch.tensor([1.0 / 3.0]))


@pytest.mark.parametrize("C,K,Q,O,B,H,W", [(1, 3, 2, 4, 3, 8, 9), (2, 2, 2, 3, 2, 6, 5), (1, 2, 4, 5, 2, 5, 6),
                                           (3, 1, 3, 2, 2, 4, 4)])
def test_onehot_closed_form_equals_the_oracle(C, K, Q, O, B, H, W):
    x = X.one_hot_pixels(C, B, H, W, Q, seed=C + K + Q)
    core = X.eps_core(Q, K * K * C, O, seed=O)
    dy = X.small_ints((B, H - K + 1, W - K + 1, O), seed=B, vmax=3, nonzero=True)
    assert torch.equal(X.eps_onehot_forward(core, x), R.eps_4step(core, x))
    dcore, _ = R.grads(R.eps_4step, [core, x], dy)
    assert torch.equal(X.eps_onehot_dcore(core.shape, x, dy), dcore)
    if K * K * C <= 4:
        assert torch.equal(X.eps_onehot_forward(core, x), torch.from_numpy(R.eps_definition_numpy(core.numpy(), x.numpy())))
    with pytest.raises(AssertionError, match="one-hot"):
        X.window_rows(x * 0.5, K)


def test_eps_sensitivity_every_window_and_position():
    """Zeroing any single dY entry changes the exact expected dCore (all windows, exhaustively); swapping two adjacent
    output positions changes the expected forward."""
    C, K, Q, O, B, H, W = 1, 2, 2, 2, 2, 5, 6
    x = X.pixels(C, B, H, W, Q, seed=5)
    core = X.eps_core(Q, K * K * C, O, seed=6)
    dy = X.small_ints((B, H - K + 1, W - K + 1, O), seed=7, vmax=3, nonzero=True)
    base = R.grads(R.eps_4step, [core, x], dy)[0]
    for idx in torch.cartesian_prod(*(torch.arange(n) for n in dy.shape)).tolist():
        d2 = dy.clone()
        d2[tuple(idx)] = 0
        assert not torch.equal(R.grads(R.eps_4step, [core, x], d2)[0], base), idx
    y = R.eps_4step(core, x)
    for b in range(B):
        for h in range(y.shape[1]):
            for w in range(y.shape[2] - 1):
                if not torch.equal(y[b, h, w], y[b, h, w + 1]):
                    break
            else:
                continue
            break
    swapped = y.clone()
    swapped[b, h, [w, w + 1]] = y[b, h, [w + 1, w]]
    with pytest.raises(AssertionError, match="differ"):
        X.assert_exact(swapped.float(), y, torch.float32, X.EPS_LAYOUT, "swapped")
    # and the report names the window
    try:
        X.assert_exact(swapped.float(), y, torch.float32, X.EPS_LAYOUT, "swapped")
    except AssertionError as e:
        assert f"sample={b}, row={h}, col={w}" in str(e)


def test_convsbs_sensitivity_every_window():
    spec_pos = [(0, 0), (0, 1), (1, 1)]
    shapes = R.sbs_core_shapes([1, 2, 1], [1, 3, 3], 1, 3)
    cores = X.sbs_cores(shapes, seed=3)
    x = X.pixels(1, 2, 4, 5, 3, seed=4, halves=True)
    dy = X.small_ints((2, 3, 4, 2), seed=5, vmax=2, nonzero=True)
    mags = X.sbs_mags(cores, spec_pos, x, dy)
    X.check_budget(mags, torch.float32)
    X.assert_every_window_counts(X.sbs_window_weights(cores, spec_pos, x, dy))
    fn = lambda xx, *cc: R.convsbs_forward(cc, spec_pos, xx)
    base = R.grads(fn, [x] + cores, dy)
    for idx in torch.cartesian_prod(*(torch.arange(n) for n in dy.shape)).tolist():
        d2 = dy.clone()
        d2[tuple(idx)] = 0
        again = R.grads(fn, [x] + cores, d2)
        assert all(not torch.equal(a, b) for a, b in zip(again[1:], base[1:])), idx


def test_convsbs_budget_cfg4_geometry():
    """The cfg4 string (9-core snake, bond 16, q = 3) on a slice of the full-size batch: +-1 cores keep every state at one
    unit, so the dCore bound grows with the window count only."""
    shapes = R.sbs_core_shapes([1, 1, 1, 1, 2, 1, 1, 1, 1], [1] + [16] * 8, 1, 3)
    cores = X.sbs_cores(shapes, seed=16, p2=0.0)
    x = X.pixels(1, 2, 32, 32, 3, seed=1)
    assert X.sbs_state_bound(cores, list(SNAKE9), x) <= 2 ** 10


def test_assert_exact_reports_the_window():
    want = torch.zeros(2, 3, 4, 2, dtype=torch.float64)
    want[1, 2, 3, 1] = 5
    got = want.clone().float()
    got[1, 2, 3, 1] = 4
    with pytest.raises(AssertionError, match=r"1 of 48 elements differ, largest by 1 grid units.*sample=1, row=2, col=3, o=1"):
        X.assert_exact(got, want, torch.float32, X.EPS_LAYOUT, "y")
    X.assert_exact(want.float(), want, torch.float32, X.EPS_LAYOUT, "y")


def _kernel_names_in_sources():
    names = set()
    for path in glob.glob(os.path.join(ROOT, "dctn_amd", "csrc", "*.hip")):
        src = open(path).read()
        for m in re.finditer(r"dctn_set_last_kernel\((.*?)\);", src, re.S):
            names.update(re.findall(r'"([a-z0-9_]+)"', m.group(1)))
    return {n for n in names if n.startswith(("eps_", "linear_head_", "convsbs_"))}


def test_every_kernel_name_has_an_exact_test():
    tree = ast.parse(open(os.path.join(ROOT, "tests", "test_gpu_exact.py")).read())
    table = next(ast.literal_eval(node.value) for node in tree.body
                 if isinstance(node, ast.Assign) and any(getattr(t, "id", None) == "KERNELS" for t in node.targets))
    found = _kernel_names_in_sources()
    assert len(found) >= 40
    missing = sorted(found - set(table))
    assert not missing, f"kernels without an exact test in tests/test_gpu_exact.py: {missing}"
    tests = {node.name for node in tree.body if isinstance(node, ast.FunctionDef)}
    assert set(table.values()) <= tests
    assert not set(table) - found, f"names in KERNELS the library no longer reports: {sorted(set(table) - found)}"
