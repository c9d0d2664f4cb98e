"""The "high" float32 precision policy (DCTN_PREC_SPLIT, bf16x3) on the host: mode names, which family each shape
routes to (`dctn_eps_family` plans without a device), and that every kernel name the bf16x3 family reports has a test
in tests/test_gpu_precision_high.py.  No GPU needed."""
import ast
import glob
import os
import re

import pytest

import dctn_amd
from dctn_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def restore_exact():
    try:
        yield
    finally:
        dctn_amd.set_float32_matmul_precision("exact")


def _family(shape, dtype=L.F32, policy=L.PREC_SPLIT):
    return L.lib().dctn_eps_family(*shape, dtype, policy)


def test_high_selects_split():
    dctn_amd.set_float32_matmul_precision("high")
    assert L.precision() & L.PREC_MASK == 2 == L.PREC_SPLIT


def test_medium_is_bf16():
    dctn_amd.set_float32_matmul_precision("medium")
    medium = L.precision()
    dctn_amd.set_float32_matmul_precision("bf16")
    assert medium == L.precision() and medium & L.PREC_MASK == L.PREC_BF16


def test_exact_names_unchanged():
    for mode in ("exact", "highest"):
        dctn_amd.set_float32_matmul_precision(mode)
        assert L.precision() & L.PREC_MASK == L.PREC_EXACT


def test_unknown_mode_raises():
    with pytest.raises(KeyError):
        dctn_amd.set_float32_matmul_precision("tf32")


@pytest.mark.parametrize("shape", [
    (1, 128, 28, 28, 2, 4, 4),   # cfg3a layer 1
    (1, 128, 25, 25, 4, 3, 6),   # cfg3a layer 2
    (1, 128, 28, 28, 2, 4, 8),   # cfg3b layer 1
    (1, 128, 25, 25, 8, 2, 8),   # cfg3b layer 2
    (1, 128, 32, 32, 4, 3, 6),   # cfg4_eps36
])
def test_split_routes_large_cores_to_bf16x3(shape):
    assert _family(shape, policy=L.PREC_EXACT) == 2
    assert _family(shape) == 5


@pytest.mark.parametrize("shape,dtype,want", [
    ((1, 128, 28, 28, 2, 3, 4), L.F32, 4),    # cfg2 in float32: the register-resident exact family
    ((1, 64, 28, 28, 2, 4, 2), L.F64, 3),     # cfg1 in float64: the two-halves path
    ((1, 2, 7, 7, 16, 2, 4), L.F32, None),    # Q = 16: beyond the bf16x3 plans
    ((1, 128, 28, 28, 3, 3, 4), L.F32, None),  # odd Q
    ((1, 128, 25, 25, 4, 3, 6), L.BF16, None),  # bf16 tensors: the policy is for float32 only
])
def test_split_elsewhere_answers_as_exact(shape, dtype, want):
    got = _family(shape, dtype)
    assert got == _family(shape, dtype, L.PREC_EXACT) and got != 5
    if want is not None:
        assert got == want


def test_split_with_prefer_halves_stays_on_halves():
    shape = (1, 128, 25, 25, 4, 3, 6)
    pol = L.PREC_SPLIT | L.OPT_F32_PREFER_HALVES
    assert _family(shape, policy=pol) == _family(shape, policy=L.PREC_EXACT | L.OPT_F32_PREFER_HALVES) != 5


def test_split_workspace_and_saved_sizes():
    """The bf16x3 family keeps Z in the exact family's layout: the same saved size; its forward needs no more scratch."""
    lib = L.lib()
    for shape in ((1, 128, 28, 28, 2, 4, 4), (1, 128, 25, 25, 4, 3, 6)):
        assert lib.dctn_eps_saved_bytes(*shape, L.F32, L.PREC_SPLIT) == lib.dctn_eps_saved_bytes(*shape, L.F32, L.PREC_EXACT) > 0
        assert lib.dctn_eps_fwd_workspace_bytes(*shape, L.F32, L.PREC_SPLIT) <= lib.dctn_eps_fwd_workspace_bytes(*shape, L.F32, L.PREC_EXACT)
        assert lib.dctn_eps_bwd_workspace_bytes(*shape, L.F32, L.PREC_SPLIT, 1, 1) > 0


def _bf16x3_names_in_sources():
    names = set()
    for path in glob.glob(os.path.join(ROOT, "dctn_amd", "csrc", "*.hip")):
        for m in re.finditer(r"dctn_set_last_kernel\((.*?)\);", open(path).read(), re.S):
            names.update(re.findall(r'"([a-z0-9_]+)"', m.group(1)))
    return {n for n in names if n.startswith("bf16x3_")}


def test_every_bf16x3_kernel_name_has_a_test():
    tree = ast.parse(open(os.path.join(ROOT, "tests", "test_gpu_precision_high.py")).read())
    table = next(ast.literal_eval(node.value) for node in tree.body
                 if isinstance(node, ast.Assign) and any(getattr(t, "id", None) == "KERNELS" for t in node.targets))
    found = _bf16x3_names_in_sources()
    assert len(found) >= 4
    assert not sorted(found - set(table)), f"bf16x3 kernels without a test: {sorted(found - set(table))}"
    assert not set(table) - found, f"names no longer reported: {sorted(set(table) - found)}"
    tests = {node.name for node in tree.body if isinstance(node, ast.FunctionDef)}
    assert set(table.values()) <= tests
