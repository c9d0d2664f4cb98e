"""Every kernel held to the buffer contract of include/dctn_amd.h (DESIGN.md "Buffer contract tests"): outputs are
overwritten, a workspace of exactly the queried size is enough and needs nothing of its previous content, `saved` buffers
of exactly the queried size are enough, and nothing outside the buffers is touched.

Each case runs under the guarded arena of tests/guarded_buffers.py - outputs, workspaces and saved buffers of the host
modules exactly sized, between 0xFF guards, pre-filled with a poison pattern - and must then pass the assertions it
already has: for the exact-input runners of tests/test_gpu_exact.py and tests/test_gpu_precision_high.py that is bit
equality with the float64 oracle, so no tolerance is introduced; the families without exact-input generators run the
body of their parity test with its own oracle and tolerance (a NaN anywhere fails those comparisons).  `arena.check()`
then asserts that every guard byte is intact.

* 0xFF (NaN; counters at their maximum): every case of tests/test_gpu_exact.py - the graph-replay half of
  `test_two_calls_and_graph_replays_equal_the_oracle` aside, the arena does not run under capture -, the exact-input
  cases of the bf16x3 family, and every other family;
* 0x7B (large finite stale values), 0x00, and stale mode (workspaces carved from one never-refilled buffer, order
  shuffled with a fixed seed, every case twice in a row): a subset that reports every name of `KERNELS`
  (`test_the_subset_reports_every_kernel_name`), and every other family.

`GUARDED` names, for every kernel the library can report, the test here that runs it
(tests/test_host_buffer_contract.py holds the sources to this table).  Out of scope: the all-reduce (peer memory,
several processes) and anything under graph capture."""
import contextlib
import inspect
import itertools
import random

import pytest
import torch

import dctn_amd
import dctn_amd.eps
from tests import test_gpu_convsbs_wide as WD
from tests import test_gpu_exact as E
from tests import test_gpu_flat_adam as FA
from tests import test_gpu_parity as P
from tests import test_gpu_precision_high as H
from tests import test_gpu_regulariser_init as RI
from tests.guarded_buffers import GuardDamaged, StalePool, guarded

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

_X, _H, _F = "test_exact_suite_under_nan_fill", "test_bf16x3_family_under_the_arena", "test_other_families_under_the_arena"
GUARDED = {
    "eps_fwd_generic": _X, "eps_bwd_generic": _X, "eps_fwd_mfma_q2reg": _X, "eps_bwd_mfma_q2reg": _X,
    "eps_fwd_q2f32": _X, "eps_bwd_q2f32": _X,
    "eps_fwd_mfma_bigcore_f32": _X, "eps_fwd_mfma_bigcore_f32_saving": _X,
    "eps_bwd_mfma_bigcore_f32": _X, "eps_bwd_mfma_bigcore_f32_savedz": _X,
    "eps_fwd_mfma_f64_halves": _X, "eps_fwd_mfma_f64_halves_saving": _X,
    "eps_bwd_mfma_f64_halves": _X, "eps_bwd_mfma_f64_halves_savedz": _X,
    "eps_fwd_mfma_f32_halves": _X, "eps_fwd_mfma_f32_halves_saving": _X,
    "eps_bwd_mfma_f32_halves": _X, "eps_bwd_mfma_f32_halves_savedz": _X,
    "eps_fwd_mfma_bf16_halves": _X, "eps_fwd_mfma_bf16_halves_saving": _X,
    "eps_bwd_mfma_bf16_halves": _X, "eps_bwd_mfma_bf16_halves_savedz": _X,
    "eps_head_fwd_mfma_q2reg": _X, "eps_head_bwd_mfma_q2reg": _X, "eps_head_fwd_q2f32": _X, "eps_head_bwd_q2f32": _X,
    "linear_head_fwd_mfma": _X, "linear_head_fwd_generic": _X, "linear_head_bwd": _X, "linear_head_bwd_generic": _X,
    "convsbs_fwd_reg_f32": _X, "convsbs_bwd_reg_f32": _X, "convsbs_fwd_band_f32": _X, "convsbs_bwd_band_f32": _X,
    "convsbs_fwd_mfma_f32": _X, "convsbs_bwd_mfma_f32": _X, "convsbs_fwd_generic": _X, "convsbs_bwd_generic": _X,
    "convsbs_bwd_wide_f32": _X, "convsbs_bwd_wide_f64": _X, "convsbs_bwd_wide_bf16": _X,
    "convsbs_many_fwd_reg_f32": _X, "convsbs_many_bwd_reg_f32": _X,
    "convsbs_many_fwd_band_f32": _X, "convsbs_many_bwd_band_f32": _X,
    "bf16x3_eps_fwd_bigcore": _H, "bf16x3_eps_fwd_bigcore_saving": _H,
    "bf16x3_eps_bwd_bigcore": _H, "bf16x3_eps_bwd_bigcore_savedz": _H,
    "logmatmulexp_fwd": _F, "logmatmulexp_bwd": _F, "logmatmulexp_fold_fwd": _F, "logmatmulexp_fold_bwd": _F,
    "logmatmulexp_fold_fwd_mfma16": _F, "logmatmulexp_fold_bwd_mfma16": _F,
    "logmatmulexp_fwd_mfma_gemm": _F, "logmatmulexp_bwd_mfma_gemm": _F,
    "tn_fiber_gram": _F, "tn_mode_product": _F, "window_stats": _F, "phi_window_stats": _F, "phi_expand": _F,
}

MODES = ["nan", "big", "zero", "stale"]
FILL = {"nan": 0xFF, "big": 0x7B, "zero": 0x00, "stale": 0xFF}
POOL = StalePool(fill=0x7B)          # stale mode: one pool for the whole module, never refilled
SEEN = {m: set() for m in MODES}     # kernel names the cases asked `dctn_amd.last_kernel()` about, per mode
RAN = {m: set() for m in MODES}


# ------------------------------------------------------------------------------------------------ the cases
def _param_sets(fn):
    """[{argname: value}] of a test function's parametrize marks (their product), in a fixed order."""
    axes = []
    for mark in getattr(fn, "pytestmark", []):
        if mark.name != "parametrize":
            continue
        names = mark.args[0]
        names = [n.strip() for n in names.split(",")] if isinstance(names, str) else list(names)
        rows = []
        for v in mark.args[1]:
            if hasattr(v, "marks") and hasattr(v, "values"):   # a pytest.param
                v = v.values if len(names) > 1 else v.values[0]
            rows.append(dict(zip(names, v)) if len(names) > 1 else {names[0]: v})
        axes.append(rows)
    out = []
    for combo in itertools.product(*axes):
        kw = {}
        for part in combo:
            kw.update(part)
        out.append(kw)
    return out


def _word(v):
    if isinstance(v, torch.dtype):
        return str(v).split(".")[1]
    if isinstance(v, (tuple, list)):
        return "_".join(_word(x) for x in v)
    if callable(v):
        return getattr(v, "__name__", "fn")
    return str(v).replace(" ", "")


def _cases(module, names=None):
    """[(id, test function, kwargs)] for every parametrised case of the module's tests (or of the named ones)."""
    out = []
    for name, fn in inspect.getmembers(module, inspect.isfunction):
        if not name.startswith("test_") or fn.__module__ != module.__name__ or (names is not None and name not in names):
            continue
        for i, kw in enumerate(_param_sets(fn)):
            words = "-".join(_word(v) for v in kw.values())[:70]
            out.append((f"{name[5:]}[{i}:{words}]", fn, kw))
    return out


def _strided(kw):
    return any(v is True and k == "strided" for k, v in kw.items()) or any(
        isinstance(v, tuple) and len(v) in (8, 9, 11) and v[-1] is True for v in kw.values())


EXACT = _cases(E)                                   # every case of tests/test_gpu_exact.py
HIGH_EXACT = _cases(H, {"test_bf16x3_exact_inputs"})
HIGH_OTHER = _cases(H, {"test_high_routes", "test_high_vs_oracle"})


def _subset(cases, seed=20):
    """All cases of the small test functions, and of the large ones the strided cases plus a fixed random half."""
    rng = random.Random(seed)
    by_fn = {}
    for c in cases:
        by_fn.setdefault(c[1].__name__, []).append(c)
    out = []
    for group in by_fn.values():
        if len(group) <= 16:
            out += group
        else:
            pick = set(rng.sample(range(len(group)), (len(group) + 1) // 2))
            out += [c for i, c in enumerate(group) if i in pick or _strided(c[2])]
    return out


SUBSET = _subset(EXACT) + HIGH_EXACT
STALE_ORDER = list(SUBSET)
random.Random(7).shuffle(STALE_ORDER)               # unlike families follow each other


def _score_cases():
    return [dict(dtype=d, B=b, C=c) for d in (torch.float32, torch.bfloat16) for b, c in ((1, 2), (77, 10), (10000, 16))]


OTHER = (   # families without exact-input generators: the body of their parity test, its oracle and its tolerance
    _cases(P, {"test_logmatmulexp_golden", "test_logmatmulexp_fold_and_batched",
               "test_logmatmulexp_fold16_factored_mfma_and_exact_fallback", "test_logmatmulexp_factored_gemm_and_exact_fallback",
               "test_window_statistics_kernel_against_reference_fixture_and_oracle",
               "test_feature_map_and_its_window_statistics_on_the_device", "test_fused_training_tail_matches_torch",
               "test_fused_cross_entropy_invalid_label_poisons_loss_and_gradient",
               "test_linear_head_scalar_kernels_any_dtype_any_feature_count", "test_linear_head_vs_torch_reference",
               "test_eps_f32_bigcore_vs_oracle", "test_eps_bf16_mfma_vs_oracle"})
    + _cases(RI, {"test_inner_product_closed_forms_through_the_alias_package",
                  "test_inner_product_value_and_gradients_match_the_reference", "test_mode_product_and_fiber_gram_shapes_fuzz",
                  "test_forward_statistics_epilogue_equals_the_materialised_output"})
    + _cases(FA, {"test_flat_adam_matches_torch_adam_within_torchs_own_error", "test_state_dict_resumes_bit_identically",
                  "test_score_fused_agrees_with_score"})
    + [(f"score_accumulate[{_word(tuple(kw.values()))}]", FA.test_score_accumulate_matches_torch, kw) for kw in _score_cases()]
)


# ------------------------------------------------------------------------------------------------ running one case
@contextlib.contextmanager
def _recording(mode):
    real = dctn_amd.last_kernel

    def last_kernel():
        name = real()
        SEEN[mode].add(name)
        return name

    dctn_amd.last_kernel = last_kernel
    try:
        yield
    finally:
        dctn_amd.last_kernel = real


def _call(fn, kw):
    if fn is E.test_two_calls_and_graph_replays_equal_the_oracle:
        return E.two_eager_calls(**kw)      # the eager half; the replays stay with tests/test_gpu_exact.py
    if fn.__module__ == H.__name__:         # that module's autouse fixture
        dctn_amd.set_float32_matmul_precision("high")
        try:
            return fn(**kw)
        finally:
            dctn_amd.set_float32_matmul_precision("exact")
    return fn(**kw)


def under(mode, call, must_allocate=True):
    """`call()` under the arena of `mode`, then the guards.  A damaged guard is reported in preference to the assertion
    it probably caused."""
    arena = guarded(fill=FILL[mode], stale=POOL if mode == "stale" else False)
    try:
        with arena, _recording(mode):
            result = call()
    except Exception as failure:
        try:
            arena.check()
        except GuardDamaged as damaged:
            raise damaged from failure
        raise
    arena.check()
    if must_allocate:   # the case did go through the arena
        assert arena.count["empty"] + arena.count["workspace"] + arena.count["zeros"] > 0, arena.count
    arena.release()
    return result


def _ids(cases):
    return [c[0] for c in cases]


# ------------------------------------------------------------------------------------------------ 0xFF: everything
@pytest.mark.parametrize("case", EXACT, ids=_ids(EXACT))
def test_exact_suite_under_nan_fill(case):
    name, fn, kw = case
    under("nan", lambda: _call(fn, kw))
    RAN["nan"].add(name)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", HIGH_EXACT + HIGH_OTHER, ids=_ids(HIGH_EXACT + HIGH_OTHER))
def test_bf16x3_family_under_the_arena(case, mode):
    """The four bf16x3_eps_* names: the exact-input cases (bit equality) and the "high" policy shapes of
    tests/test_gpu_precision_high.py (their own tolerance, reproducibility and comparison with the bf16 policy)."""
    name, fn, kw = case
    for _ in range(2 if mode == "stale" else 1):
        under(mode, lambda: _call(fn, kw))
    RAN[mode].add(name)


# ------------------------------------------------------------------------------------------------ 0x7B, 0x00: the subset
@pytest.mark.parametrize("mode", ["big", "zero"])
@pytest.mark.parametrize("case", _subset(EXACT), ids=_ids(_subset(EXACT)))
def test_exact_subset_under_finite_fills(case, mode):
    name, fn, kw = case
    under(mode, lambda: _call(fn, kw))
    RAN[mode].add(name)


@pytest.mark.parametrize("case", [c for c in STALE_ORDER if c[1].__module__ == E.__name__],
                         ids=_ids([c for c in STALE_ORDER if c[1].__module__ == E.__name__]))
def test_exact_subset_with_stale_workspaces(case):
    """Twice in a row: the second run inherits the first's own flags, tickets and partial records; the first inherits
    those of an unlike family (the order is shuffled with a fixed seed)."""
    name, fn, kw = case
    for _ in range(2):
        under("stale", lambda: _call(fn, kw))
    RAN["stale"].add(name)


# ------------------------------------------------------------------------------------------------ the other families
@pytest.mark.parametrize("mode", ["nan", "big", "stale"])
@pytest.mark.parametrize("case", OTHER, ids=_ids(OTHER))
def test_other_families_under_the_arena(case, mode):
    """logmatmulexp (direct, fold, fold mfma16, mfma gemm - with the windows, tiles and batch elements the existing
    tests send to the exact fall-back), tn_fiber_gram / tn_mode_product, window_stats / phi_window_stats / phi_expand,
    dctn_ce_loss_*, dctn_sgd_l2_step, dctn_adam_l2_step, dctn_ce_score_accumulate, the float64 linear head: the existing
    test's body with its oracle and tolerance.  Optimiser state (momentum, exp_avg, the Adam state block, the score
    accumulators) comes from `zeros`: guarded, not poisoned - the contract says it is read."""
    name, fn, kw = case
    for _ in range(2 if mode == "stale" else 1):
        under(mode, lambda: _call(fn, kw), must_allocate=fn is not FA.test_score_accumulate_matches_torch)


# ------------------------------------------------------------------------------------------------ bit-reproducible kernels
def _adam_run():
    snaps, _ = FA._run_eager(FA._batches(4))
    return snaps[-1]


def _score_run():
    from dctn_amd.evaluation import score_fused

    model = FA._model(torch.float32)
    dl = [(x, y, torch.arange(len(y))) for x, y in FA._batches(3, torch.float32, seed=41, B=64)]
    return score_fused(model, dl, DEV)


def _eps_random(C, B, H_, W, Q, K, O, policy):
    def run():
        torch.manual_seed(5)
        N = K * K * C
        x = torch.randn(C, B, H_, W, Q)
        core = torch.randn(*(Q,) * N, O) * Q ** (-N / 4)
        dy = torch.randn(B, H_ - K + 1, W - K + 1, O)
        dctn_amd.set_float32_matmul_precision(policy)
        try:
            y, gx, gc, kf, kb = H._run(core, x, dy)
        finally:
            dctn_amd.set_float32_matmul_precision("exact")
        assert kf.startswith("bf16x3_" if policy == "high" else "eps_fwd_mfma_bigcore_f32"), kf
        return y, gx, gc
    return run


def _wide_run():
    res = WD.run(WD.snake_spec(18, 10), torch.float32, seed=3)
    assert res[3] == "convsbs_bwd_wide_f32"
    return (res[0].detach(), res[1], *res[2])


REPRODUCIBLE = {   # documented bit-reproducible: the result under every fill is the result on zeroed buffers, bit for bit
    "flat_adam_eager_steps": _adam_run,                                  # FlatAdam (resume / two runs bit-identical)
    "score_fused": _score_run,                                           # dctn_ce_score_accumulate: deterministic launch
    "bigcore_f32_fixed_order_slices": _eps_random(1, 3, 9, 10, 2, 4, 4, "exact"),
    "bigcore_f32_padded_out": _eps_random(1, 2, 6, 7, 4, 3, 6, "exact"),
    "bf16x3_fixed_order_slices": _eps_random(1, 3, 9, 9, 8, 2, 8, "high"),
    "convsbs_wide_f32": _wide_run,                                       # test_two_backward_calls_are_bit_identical
}


def _same(a, b):
    if isinstance(a, torch.Tensor):
        return a.dtype == b.dtype and torch.equal(a, b)
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return a == b


@pytest.mark.parametrize("which", sorted(REPRODUCIBLE))
def test_reproducible_kernels_give_the_bits_of_zeroed_buffers(which):
    run = REPRODUCIBLE[which]
    base = under("zero", run)
    for mode in ("nan", "big", "stale", "stale"):
        assert _same(under(mode, run), base), f"{which}: the result under '{mode}' buffers differs from zeroed buffers"


def test_the_arena_stays_out_of_a_capture():
    """Graph tests stay as they are: entering the arena on a capturing stream raises and patches nothing."""
    from dctn_amd import _lib as L

    real, t = L.workspace, torch.zeros(4, device=DEV)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        t.add_(1.0)
        with pytest.raises(RuntimeError, match="capture"):
            with guarded():
                pass
    assert L.workspace is real and dctn_amd.eps.torch is torch
    graph.replay()
    torch.cuda.synchronize()
    assert t.tolist() == [1.0] * 4


# ------------------------------------------------------------------------------------------------ coverage of the subset
@pytest.mark.parametrize("mode", MODES)
def test_the_subset_reports_every_kernel_name(mode):
    """Holds once the cases above have run in this process (a run narrowed with -k has nothing to say)."""
    want = {c[0] for c in (EXACT if mode == "nan" else _subset(EXACT))} | {c[0] for c in HIGH_EXACT}
    if not want <= RAN[mode]:
        return
    names = set(E.KERNELS) | set(H.KERNELS)
    assert names <= SEEN[mode], f"no case under '{mode}' reported {sorted(names - SEEN[mode])}"
