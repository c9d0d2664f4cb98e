"""Host checks of tests/test_gpu_buffer_contract.py: every kernel name the library can report - the all-reduce aside - has
an entry in its `GUARDED` table, the table names nothing the sources no longer report, and its 0xFF pass covers every
collected case of tests/test_gpu_exact.py."""
import ast
import glob
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONTRACT = os.path.join(ROOT, "tests", "test_gpu_buffer_contract.py")


def _kernel_names_in_sources():
    """Like tests/test_host_exact_inputs.py, without the name-prefix filter."""
    names = set()
    for path in glob.glob(os.path.join(ROOT, "dctn_amd", "csrc", "*.hip")):
        src = open(path).read()
        for m in re.finditer(r"dctn_set_last_kernel\((.*?)\);", src, re.S):
            names.update(re.findall(r'"([a-z0-9_]+)"', m.group(1)))
    return names


def _guarded_table():
    tree = ast.parse(open(CONTRACT).read())
    consts = {}
    for node in tree.body:
        if isinstance(node, ast.Assign) and isinstance(node.value, ast.Tuple) and isinstance(node.targets[0], ast.Tuple):
            consts.update({t.id: ast.literal_eval(v) for t, v in zip(node.targets[0].elts, node.value.elts)})
    table = next(node.value for node in tree.body
                 if isinstance(node, ast.Assign) and any(getattr(t, "id", None) == "GUARDED" for t in node.targets))
    out = {ast.literal_eval(k): (consts[v.id] if isinstance(v, ast.Name) else ast.literal_eval(v))
           for k, v in zip(table.keys, table.values)}
    tests = {node.name for node in tree.body if isinstance(node, ast.FunctionDef)}
    return out, tests


def test_every_kernel_name_runs_under_the_arena():
    table, tests = _guarded_table()
    found = {n for n in _kernel_names_in_sources() if not n.startswith("allreduce_")}   # several processes, peer memory
    assert len(found) >= 60
    missing = sorted(found - set(table))
    assert not missing, f"kernels without an entry in GUARDED of tests/test_gpu_buffer_contract.py: {missing}"
    gone = sorted(set(table) - found)
    assert not gone, f"names in GUARDED the library no longer reports: {gone}"
    assert set(table.values()) <= tests


def test_the_nan_pass_covers_every_collected_case_of_the_exact_suite():
    from tests import test_gpu_buffer_contract as C
    from tests import test_gpu_exact as E
    from tests import test_gpu_precision_high as H

    res = subprocess.run([sys.executable, "-m", "pytest", "--collect-only", "-q", "-p", "no:cacheprovider",
                          os.path.join("tests", "test_gpu_exact.py")], cwd=ROOT, capture_output=True, text=True)
    collected = [line for line in res.stdout.splitlines() if "::" in line]
    assert len(collected) >= 330, res.stdout[-2000:] + res.stderr[-2000:]
    assert len(C.EXACT) == len(collected)
    per_fn = {}
    for line in collected:
        name = line.split("::")[1].split("[")[0]
        per_fn[name] = per_fn.get(name, 0) + 1
    mine = {}
    for _, fn, _ in C.EXACT:
        mine[fn.__name__] = mine.get(fn.__name__, 0) + 1
    assert mine == per_fn
    assert len(C.HIGH_EXACT) == 10 and set(H.KERNELS) <= set(C.GUARDED) and set(E.KERNELS) <= set(C.GUARDED)
    # the subset of the other fills keeps every small test function whole and the strided cases of the large ones
    subset = C._subset(C.EXACT)
    assert {c[1].__name__ for c in subset} == set(per_fn)
    assert all(c in subset for c in C.EXACT if C._strided(c[2]))
    assert [c[0] for c in C.STALE_ORDER] != [c[0] for c in C.SUBSET] and sorted(c[0] for c in C.STALE_ORDER) == sorted(
        c[0] for c in C.SUBSET)
    # and the settings the other fills must see: both keep_gemm_result settings, the option flags, blocked4 and row-major
    # features, dCore with and without dX
    from dctn_amd import _lib as L

    def has(fn_name, **kw):
        return any(c[1].__name__ == fn_name and all(c[2].get(k) == v for k, v in kw.items()) for c in subset)

    for keep in (True, False):
        assert has("test_eps_bigcore_f32", keep=keep) and has("test_eps_halves_f64", keep=keep, chunks=L.OPT_SMALL_CHUNKS)
        assert has("test_eps_halves_f32_small_chunks", keep=keep) and has("test_eps_halves_f32_preferred", keep=keep)
        assert has("test_eps_halves_bf16", keep=keep) and has("test_eps_halves_f32", keep=keep)
    for mode in ("fused_blocked4", "fused_rowmajor", "fused_bwd_only", "unfused"):
        assert has("test_head_bf16", mode=mode) and has("test_head_bf16_cfg2_batches", mode=mode)
    for need_dx in (True, False):
        assert has("test_eps_q2reg_bf16", need_dx=need_dx)
    assert has("test_eps_q2reg_bf16", strided=True) and has("test_eps_q2f32", strided=True) and has("test_head_f32", strided=True)

