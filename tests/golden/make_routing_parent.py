"""Record what the dispatch layer's host-only queries answer, from a build of the PARENT commit's library.

    git worktree add ../parent <parent commit> && make -C ../parent/dctn_amd/csrc
    python tests/golden/make_routing_parent.py --lib ../parent/dctn_amd/libdctn_amd.so --commit <parent commit>

writes tests/golden/routing_parent.npz (integers only; compressed, 1/10 of the same rows as text).  tests/test_host_routing_snapshot.py recomputes the same queries with the
library under test and compares: every committed row one by one, the whole EPS grid through one sha256 per
(dtype, policy) bucket.  The queries plan without a device; what they answer depends on `dctn_device_limits`, which
the record stores and the test checks first.

The record is never regenerated from the code under review: a routing change that is meant shows up as a diff of
this file made from the commit that precedes it.
"""
from __future__ import annotations

import argparse
import ctypes
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from dctn_amd import _lib as L   # noqa: E402  (constants and ctypes signatures only; no library is loaded by the import)

RECORD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "routing_parent.npz")

DTYPES = (L.F32, L.F64, L.BF16)
POLICIES = (0, L.PREC_BF16, L.PREC_SPLIT, L.OPT_F32_PREFER_HALVES, L.PREC_SPLIT | L.OPT_F32_PREFER_HALVES,
            L.OPT_GENERIC_KERNELS, L.OPT_SMALL_CHUNKS)
HEAD_COUT = 10
BWD_NEEDS = ((1, 1), (1, 0), (0, 1))   # (need_dx, need_dcore)
# committed one by one: every row of these families; of the others every SAMPLE_EVERY-th row of its bucket
KEPT_FAMILIES = (1, 2, 4, 5)
SAMPLE_EVERY = 41


def load(path: str) -> ctypes.CDLL:
    handle = ctypes.CDLL(path)
    for name, (res, args) in L.SIGNATURES.items():
        fn = getattr(handle, name)
        fn.restype, fn.argtypes = res, args
    return handle


def device_limits(lib) -> list:
    cus, lds = ctypes.c_int(0), ctypes.c_int(0)
    assert lib.dctn_device_limits(ctypes.byref(cus), ctypes.byref(lds)) == 0
    return [cus.value, lds.value]


# ------------------------------------------------------------------------------------------------ EPS
def eps_grid():
    for C in (1, 2, 3):
        for B in (2, 128, 1024):
            for H, W in ((5, 5), (7, 9), (25, 25), (28, 28), (32, 32)):
                for Q in (2, 3, 4, 8, 16):
                    for K in (1, 2, 3, 4):
                        if Q ** (K * K * C) > 2 ** 26:
                            continue
                        for O in (1, 2, 4, 6, 8, 10, 32):
                            yield (C, B, H, W, Q, K, O)


# outside the grid, all committed: kernels larger than the image, and the head's feature-layout flag (which only the
# head entry points accept) on shapes of several families: family -1
EPS_EXTRA = [
    (shape, dtype, policy)
    for shape in ((1, 2, 5, 5, 3, 9, 2), (1, 2, 3, 3, 2, 4, 4), (2, 128, 2, 9, 2, 3, 4), (1, 1024, 28, 28, 2, 3, 4),
                  (1, 128, 28, 28, 2, 4, 4), (2, 3, 7, 9, 3, 2, 3))
    for dtype in DTYPES
    for policy in (0, L.PREC_SPLIT, L.OPT_HEAD_FEATURES_BLOCKED4, L.OPT_HEAD_FEATURES_BLOCKED4 | L.PREC_BF16, 1 << 13)
]


def eps_row(lib, shape, dtype: int, policy: int) -> list:
    """[family, saved bytes, forward ws, statistics ws, backward ws for each of BWD_NEEDS, head backward ws]"""
    a = (*shape, dtype, policy)
    return [lib.dctn_eps_family(*a), lib.dctn_eps_saved_bytes(*a), lib.dctn_eps_fwd_workspace_bytes(*a),
            lib.dctn_eps_fwd_stats_workspace_bytes(*a),
            *(lib.dctn_eps_bwd_workspace_bytes(*a, dx, dc) for dx, dc in BWD_NEEDS),
            lib.dctn_eps_head_bwd_workspace_bytes(*shape, HEAD_COUT, dtype, policy)]


def eps_buckets(lib):
    """{(dtype, policy): (sha256 over every grid row, rows per family -1 .. 5, committed rows [grid index, *row])}"""
    grid = list(eps_grid())
    out = {}
    for dtype in DTYPES:
        for policy in POLICIES:
            digest, kept, hist, others = hashlib.sha256(), [], [0] * 7, 0
            for i, shape in enumerate(grid):
                row = eps_row(lib, shape, dtype, policy)
                digest.update((",".join(map(str, (*shape, *row))) + "\n").encode())
                hist[row[0] + 1] += 1
                if row[0] in KEPT_FAMILIES or (others := others + 1) % SAMPLE_EVERY == 1:
                    kept.append([i, *row])
            out[(dtype, policy)] = (digest.hexdigest(), hist, kept)
    return out


# ------------------------------------------------------------------------------------------------ ConvSBS
SNAKE_A = [(0, 0), (0, 1), (0, 2), (1, 2), (1, 1), (1, 0), (2, 0), (2, 1), (2, 2)]
SNAKE_B = [(0, 0), (1, 0), (2, 0), (2, 1), (1, 1), (0, 1), (0, 2), (1, 2), (2, 2)]
RING_2X2 = [((0, 0), 1), ((0, 1), 3), ((1, 0), 2), ((1, 1), 4)]
SBS_FLAGS = (0, L.SBS_MATRIX_CORE_SWEEP, L.SBS_WIDE_SWEEP, L.SBS_MATRIX_CORE_SWEEP | L.SBS_WIDE_SWEEP)
CLASSIFIER_BONDS = (2, 4, 8, 16, 18)


def _snake(pos, mid):
    return [(p, mid if i == 4 else 1) for i, p in enumerate(pos)]


def sbs_strings():
    """(name, [(position, out size)], bond sizes, C, q, B, H, W): the strings of tests/golden/sbs_*.npz and the three
    layers of tests/sbs_classifier.py (28 x 28 images, batch 128) at several bonds"""
    yield "snake_r4_c1_q2", _snake(SNAKE_A, 2), (1,) + (4,) * 8, 1, 2, 2, 6, 6
    yield "snake_r2_c1_q3", _snake(SNAKE_A, 2), (1,) + (2,) * 8, 1, 3, 2, 5, 6
    yield "snake2_r4_c2_q2", _snake(SNAKE_B, 2), (1,) + (4,) * 8, 2, 2, 2, 5, 5
    yield "snake_ring_r3_c1_q2", _snake(SNAKE_A, 2), (3,) * 9, 1, 2, 2, 5, 5
    yield "2x2_ring_perm0", RING_2X2, (3, 4, 5, 6), 2, 2, 3, 4, 5
    yield "2x2_ring_perm1", [RING_2X2[i] for i in (2, 0, 3, 1)], (3, 4, 5, 6), 2, 2, 3, 4, 5
    for bond in CLASSIFIER_BONDS:
        bonds = (1,) + (bond,) * 8
        yield f"classifier_l1_r{bond}", _snake(SNAKE_A, 2), bonds, 1, 2, 128, 28, 28
        yield f"classifier_l2_r{bond}", _snake(SNAKE_B, 2), bonds, 2, 2, 128, 26, 26
        yield f"classifier_l3_r{bond}", _snake(SNAKE_A, 10), bonds, 2, 2, 128, 24, 24
        yield f"classifier_l1_ring_r{bond}", _snake(SNAKE_A, 2), (bond,) * 9, 1, 2, 128, 28, 28


def many_layers():
    """(name, [strings], bond sizes, C, q, B, H, W): the two-snake ManyConvSBS layers of the classifier"""
    for bond in CLASSIFIER_BONDS:
        two = [_snake(SNAKE_A, 2), _snake(SNAKE_B, 2)]
        yield f"many_l1_r{bond}", two, (1,) + (bond,) * 8, 1, 2, 128, 28, 28
        yield f"many_l2_r{bond}", two, (1,) + (bond,) * 8, 2, 2, 128, 26, 26
        yield f"many_l2_b2_r{bond}", two, (1,) + (bond,) * 8, 2, 2, 2, 7, 9


def _arrays(cores, bonds):
    return (L.int_array([o for _, o in cores]), L.int_array(bonds), L.int_array([p[0] for p, _ in cores]),
            L.int_array([p[1] for p, _ in cores]))


def sbs_rows(lib) -> dict:
    """{name: [value, ...]} in the fixed order of the loops below"""
    out = {}
    for name, cores, bonds, C, q, B, H, W in sbs_strings():
        outs, bnd, ph, pw = _arrays(cores, bonds)
        row = []
        for dtype in DTYPES:
            for flags in SBS_FLAGS:
                for backward in (0, 1):
                    row.append(lib.dctn_convsbs_workspace_bytes(len(cores), outs, bnd, C, B, H, W, q, ph, pw, dtype | flags, backward))
                row.append(lib.dctn_convsbs_saved_states_bytes(len(cores), outs, bnd, C, B, H, W, q, ph, pw, dtype | flags))
        out[name] = row
    for name, strings, bonds, C, q, B, H, W in many_layers():
        cat = [c for s in strings for c in s]
        outs, bnd, ph, pw = _arrays(cat, bonds * len(strings))
        out[name] = [lib.dctn_convsbs_many_workspace_bytes(len(strings), len(strings[0]), outs, bnd, C, B, H, W, q, ph, pw, dtype)
                     for dtype in DTYPES]
    return out


def record(lib, commit: str) -> dict:
    """the arrays of the record; every value is an integer but the commit and the digests"""
    buckets = eps_buckets(lib)
    sbs = sbs_rows(lib)
    return {
        "parent_commit": np.array(commit),
        "device_limits": np.array(device_limits(lib)),
        "eps_buckets": np.array(list(buckets)),                                    # [bucket] (dtype, policy)
        "eps_sha256": np.array([v[0] for v in buckets.values()]),
        "eps_families": np.array([v[1] for v in buckets.values()]),                # [bucket][family + 1] rows of the whole grid
        # [row] dtype, policy, grid index, then eps_row's eight answers
        "eps_rows": np.array([[*key, *row] for key, v in buckets.items() for row in v[2]], dtype=np.int64),
        "eps_extra": np.array([eps_row(lib, *e) for e in EPS_EXTRA], dtype=np.int64),
        "sbs_names": np.array(list(sbs)),
        **{f"sbs_{name}": np.array(row, dtype=np.int64) for name, row in sbs.items()},
    }


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--lib", required=True, help="libdctn_amd.so built from the parent commit")
    ap.add_argument("--commit", required=True, help="hash of the parent commit")
    a = ap.parse_args()
    rec = record(load(a.lib), a.commit)
    np.savez_compressed(RECORD, **rec)
    print(f"{RECORD}: {os.path.getsize(RECORD)} bytes, {len(rec['eps_rows'])} committed EPS rows of "
          f"{int(rec['eps_families'].sum())}, rows per family -1 .. 5: {rec['eps_families'].sum(0).tolist()}")


if __name__ == "__main__":
    main()
