"""Host-side checks of the device learning-rate schedule (no GPU needed): the library's host entry point
`dctn_lr_schedule_value` - the very function the optimizer kernels evaluate - against the numpy mirror
`LRSchedule.value`, bit for bit; the mirror against an independent restatement in `fractions`; validation on both
sides; the interface; the plateau hook.

Steps covered per table: every step from 0 to 20 past the last knot for every table whose last knot lies below 20 000
(the builders' tables, the single knot, the 64 knots, k[0] > 0 and the random tables that happen to be short).  The 200
random tables have gaps up to 10^6 steps - about 5 * 10^8 steps in all, hours of Python - so a long table is covered at
every step within 4 of every knot, every step of every segment shorter than 64, 8 seeded steps inside every longer
segment, and the 20 steps past the end: the places where the segment search and the interpolation's end points can go
wrong, plus a sample of each interior."""
import ctypes
import inspect
import math
import os
import random
import re
import struct
import subprocess
from fractions import Fraction

import numpy as np
import pytest
import torch

from dctn_amd import _lib
from dctn_amd.training import LRSchedule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
c_void, c_i64, c_int, c_size = _lib.c_void, _lib.c_i64, _lib.c_int, _lib.c_size
c_float, c_double = ctypes.c_float, ctypes.c_double
SCALES = (1.0, 0.5, 0.7)   # 0.7: not a power of two, so the product rounds
EXHAUSTIVE_BELOW = 20_000


def lib_value(words: np.ndarray, step: int):
    """(return code, value) of dctn_lr_schedule_value on a host copy of the block"""
    out = c_float(float("nan"))
    words = np.ascontiguousarray(words, dtype=np.int32)
    rc = _lib.lib().dctn_lr_schedule_value(words.ctypes.data, int(step), ctypes.byref(out))
    return rc, out.value


def bits(x: float) -> int:
    return struct.unpack("<I", struct.pack("<f", x))[0]


def steps_to_check(ks, rng):
    last = ks[-1]
    if last < EXHAUSTIVE_BELOW:
        return range(0, last + 21)
    steps = set(range(0, min(ks[0], 8) + 1)) | set(range(last, last + 21))
    for a, b in zip(ks, ks[1:]):
        if b - a < 64:
            steps.update(range(a, b + 1))
        else:
            steps.update(range(a - 4, a + 5))
            steps.update(range(b - 4, b + 5))
            steps.add((a + b) // 2)
            steps.update(rng.randrange(a, b) for _ in range(8))
    return sorted(s for s in steps if s >= 0)


def builder_tables():
    return {
        "constant": LRSchedule.constant("cpu", 3e-4),
        "warmup": LRSchedule.warmup("cpu", 1e-3, 37),
        "warmup from a start": LRSchedule.warmup("cpu", 1e-3, 10, start=1e-5),
        "warmup_cosine": LRSchedule.warmup_cosine("cpu", 2e-3, 25, 400, final=1e-5),
        "warmup_cosine, short decay": LRSchedule.warmup_cosine("cpu", 2e-3, 5, 17),
        "cosine, no warm-up": LRSchedule.warmup_cosine("cpu", 1e-3, 0, 1000),
        "milestones": LRSchedule.milestones("cpu", 1e-2, [30, 60, 90], 0.1),
        "single knot": LRSchedule("cpu", [(5, 1e-3)]),
        "64 knots": LRSchedule("cpu", [(3 * i * i + i, 1e-3 * (1.0 + math.sin(i)) + 1e-6) for i in range(64)],
                               hold=[i % 3 == 0 for i in range(64)]),
        "k[0] > 0": LRSchedule("cpu", [(7, 1e-4), (20, 1e-3), (50, 1e-3), (120, 1e-5)], hold=[0, 1, 0, 0]),
    }


def random_table(seed: int):
    rng = random.Random(seed)
    n = rng.randint(1, 64)
    k, knots = rng.choice((0, 0, rng.randint(1, 1000))), []
    for _ in range(n):
        knots.append((k, 10.0 ** rng.uniform(-7.0, 0.0)))
        k += int(round(10.0 ** rng.uniform(0.0, 6.0)))   # gaps from 1 to 10^6 steps
    return knots, [rng.random() < 0.4 for _ in range(n)]


def check_against_library(schedule: LRSchedule, rng, what: str):
    ks = [k for k, _ in schedule.knots]
    steps = steps_to_check(ks, rng)
    for scale in SCALES:
        schedule.scale = scale
        words = schedule.host_block()
        for s in steps:
            rc, got = lib_value(words, s)
            assert rc == 0, (what, s, rc)
            want = schedule.value(s)
            assert bits(got) == bits(want), f"{what}: step {s} scale {scale}: library {got!r}, mirror {want!r}"
    schedule.scale = 1.0


# ------------------------------------------------------------------ the mirror against the library
def test_the_block_is_784_bytes_and_laid_out_as_documented():
    assert _lib.lib().dctn_lr_schedule_bytes() == 784 == 4 * LRSchedule.WORDS
    s = LRSchedule("cpu", [(2, 0.5), (9, 0.25), (11, 0.125)], hold=[0, 1, 0])
    s.scale = 0.75
    words = s.host_block()
    assert words.dtype == np.int32 and words.size == 196
    assert words[0] == 3 and words.view(np.float32)[1] == 0.75 and words[2] == 0 and words[3] == 0
    assert list(words[4:7]) == [2, 9, 11] and list(words.view(np.float32)[68:71]) == [0.5, 0.25, 0.125]
    assert list(words[132:135]) == [0, 1, 0]
    assert np.array_equal(s._block.numpy(), words)   # the (here: host) block the optimizers are handed
    assert LRSchedule.decode(words) == ([(2, 0.5), (9, 0.25), (11, 0.125)], [0, 1, 0], 0.75)
    header = open(os.path.join(ROOT, "include", "dctn_amd.h")).read()
    for field in ("n_knots", "scale", r"reserved\[2\]", r"k\[64\]", r"lr\[64\]", r"hold\[64\]"):
        assert re.search(r"\*\s+(float|int32)\s+" + field, header), f"the header does not document `{field}`"


@pytest.mark.parametrize("name", sorted(builder_tables()))
def test_library_equals_mirror_on_the_builders_tables(name):
    check_against_library(builder_tables()[name], random.Random(1), name)


@pytest.mark.parametrize("block", range(8))
def test_library_equals_mirror_on_200_random_tables(block):
    for seed in range(25 * block, 25 * block + 25):
        knots, hold = random_table(seed)
        check_against_library(LRSchedule("cpu", knots, hold), random.Random(1000 + seed), f"random table {seed}")


def test_unused_slots_do_not_matter():
    s = LRSchedule("cpu", [(0, 1e-3), (10, 1e-4)])
    words = s.host_block()
    words[4 + 2: 4 + 64] = np.iinfo(np.int32).max
    words.view(np.float32)[68 + 2: 68 + 64] = np.nan
    words[132 + 2:] = 0x7FC00000
    for step in range(0, 31):
        rc, got = lib_value(words, step)
        assert rc == 0 and bits(got) == bits(s.value(step))


# ------------------------------------------------------------------ the mirror against independent arithmetic
def to_f32(x: float) -> float:
    return struct.unpack("<f", struct.pack("<f", x))[0]   # C's double -> float conversion: round to nearest even


def restated(knots, hold, scale, s):
    """The definition with exact rationals, rounded once to float64 per operation (float(Fraction) rounds correctly),
    once to float32, and once more for the product with the scale (exact in float64: 24 x 24 bits)."""
    ks = [k for k, _ in knots]
    lrs = [to_f32(lr) for _, lr in knots]
    n = len(ks)
    if s < ks[0]:
        v = lrs[0]
    elif s >= ks[-1]:
        v = lrs[-1]
    else:
        i = max(j for j in range(n) if ks[j] <= s)
        if hold[i]:
            v = lrs[i]
        else:
            frac = float(Fraction(s - ks[i], ks[i + 1] - ks[i]))
            diff = float(Fraction(lrs[i + 1]) - Fraction(lrs[i]))
            rise = float(Fraction(diff) * Fraction(frac))
            v = to_f32(float(Fraction(lrs[i]) + Fraction(rise)))
    return to_f32(float(Fraction(v) * Fraction(to_f32(scale))))


def test_mirror_equals_the_restatement_in_fractions():
    rng = random.Random(7)
    tables = [(s.knots, s.hold) for s in builder_tables().values()]
    tables += [random_table(seed) for seed in range(15)]
    for knots, hold in tables:
        schedule = LRSchedule("cpu", knots, hold)
        for scale in SCALES:
            schedule.scale = scale
            for s in steps_to_check([k for k, _ in knots], rng):
                want = restated(schedule.knots, schedule.hold, scale, s)
                assert bits(schedule.value(s)) == bits(want), (knots[:3], s, scale)


def test_mirror_is_exact_at_knots_monotone_on_segments_and_constant_past_the_ends():
    rng = random.Random(11)
    tables = [(s.knots, s.hold) for s in builder_tables().values()] + [random_table(seed) for seed in range(200)]
    for knots, hold in tables:
        schedule = LRSchedule("cpu", knots, hold)
        ks, lrs = [k for k, _ in schedule.knots], [lr for _, lr in schedule.knots]
        for k, lr in zip(ks, lrs):
            assert bits(schedule.value(k)) == bits(lr)   # scale 1.0 leaves the bits alone
        for s in list(range(0, min(ks[0], 50) + 1)) + [ks[0] // 2]:
            assert schedule.value(s) == lrs[0]
        for s in (ks[-1], ks[-1] + 1, ks[-1] + 20, ks[-1] + 10 ** 6, 2 ** 31 - 1):
            assert schedule.value(s) == lrs[-1]
        for i in range(len(ks) - 1):
            a, b = ks[i], ks[i + 1]
            inside = range(a, b + 1) if b - a < 200 else sorted({a, a + 1, b - 1, b, *(rng.randrange(a, b) for _ in range(30))})
            values = [schedule.value(s) for s in inside]
            if schedule.hold[i]:
                assert all(v == lrs[i] for v in values[:-1])
            elif lrs[i + 1] >= lrs[i]:
                assert all(x <= y for x, y in zip(values, values[1:])) and values[0] == lrs[i] and values[-1] == lrs[i + 1]
            else:
                assert all(x >= y for x, y in zip(values, values[1:])) and values[0] == lrs[i] and values[-1] == lrs[i + 1]


def test_builders_give_the_shapes_they_name():
    w = LRSchedule.warmup("cpu", 1e-3, 10)
    assert w.value(0) == 0.0 and w.value(10) == w.value(500) == float(np.float32(1e-3))
    assert abs(w.value(5) - 5e-4) < 1e-10
    assert LRSchedule.warmup("cpu", 1e-3, 0).knots == [(0, float(np.float32(1e-3)))]
    c = LRSchedule.warmup_cosine("cpu", 1.0, 100, 10_100, final=0.1)
    assert len(c.knots) == 64 and c.knots[0] == (0, 0.0) and c.knots[1][0] == 100 and c.knots[-1][0] == 10_100
    assert c.value(100) == 1.0 and c.value(10_100) == c.value(99_999) == float(np.float32(0.1))
    # 62 linear pieces of a half cosine f = 0.1 + 0.45 (1 + cos(pi x / T)), T = 10 000: a chord over h steps is within
    # max|f''| h^2 / 8 = 0.45 (pi / T)^2 h^2 / 8 of it, the longest piece has h = ceil(T / 62) = 162 steps
    for s in range(100, 10_101, 37):
        exact = 0.1 + 0.9 * 0.5 * (1.0 + math.cos(math.pi * (s - 100) / 10_000))
        assert abs(c.value(s) - exact) <= 0.45 * (math.pi * 162 / 10_000) ** 2 / 8 + 1e-6
    short = LRSchedule.warmup_cosine("cpu", 1.0, 2, 6)
    assert [k for k, _ in short.knots] == [0, 2, 3, 4, 5, 6]
    m = LRSchedule.milestones("cpu", 0.1, [30, 80], 0.1)
    assert [m.value(s) for s in (0, 29, 30, 79, 80, 1000)] == [float(np.float32(v)) for v in (0.1, 0.1, 0.1 * 0.1, 0.1 * 0.1, 0.1 * 0.1 ** 2, 0.1 * 0.1 ** 2)]
    with pytest.raises(ValueError):
        LRSchedule.warmup_cosine("cpu", 1.0, 10, 10)
    with pytest.raises(ValueError):
        LRSchedule.milestones("cpu", 0.1, list(range(1, 65)), 0.5)   # 65 knots


# ------------------------------------------------------------------ validation
MALFORMED = {
    "no knots": ([], None),
    "65 knots": ([(i, 1e-3) for i in range(65)], None),
    "equal steps": ([(0, 1e-3), (5, 1e-3), (5, 1e-4)], None),
    "decreasing steps": ([(0, 1e-3), (9, 1e-3), (4, 1e-4)], None),
    "negative first step": ([(-1, 1e-3), (4, 1e-4)], None),
    "negative rate": ([(0, 1e-3), (4, -1e-4)], None),
    "NaN rate": ([(0, float("nan"))], None),
    "infinite rate": ([(0, 1e-3), (4, float("inf"))], None),
    "a rate beyond float32": ([(0, 1e39)], None),
}


def raw_block(knots, scale=1.0):
    """A block written field by field, without LRSchedule's validation"""
    words = np.zeros(196, dtype=np.int32)
    words[0] = len(knots)
    words.view(np.float32)[1] = scale
    for i, (k, lr) in enumerate(knots[:64]):
        words[4 + i] = k
        with np.errstate(over="ignore"):
            words.view(np.float32)[68 + i] = np.float32(lr)
    return words


@pytest.mark.parametrize("name", sorted(MALFORMED))
def test_malformed_tables_are_refused_on_both_sides(name):
    knots, hold = MALFORMED[name]
    with pytest.raises(ValueError):
        LRSchedule("cpu", knots, hold)
    good = LRSchedule("cpu", [(0, 1e-3)])
    with pytest.raises(ValueError):
        good.set(knots, hold)
    assert good.knots == [(0, float(np.float32(1e-3)))]   # a refused set() leaves the table alone
    rc, _ = lib_value(raw_block(knots), 3)
    assert rc == _lib.ERR_BAD_SHAPE, name


def test_other_malformed_input():
    with pytest.raises(ValueError):
        LRSchedule("cpu", [(0, 1e-3), (4, 1e-4)], hold=[1])   # one flag per knot
    with pytest.raises(ValueError):
        LRSchedule("cpu", [(0.5, 1e-3)])
    s = LRSchedule("cpu", [(0, 1e-3)])
    for bad in (-0.5, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            s.scale = bad
        assert lib_value(raw_block([(0, 1e-3)], scale=bad), 0)[0] == _lib.ERR_BAD_SHAPE
    assert s.scale == 1.0
    assert lib_value(raw_block([(0, 1e-3)]), -1)[0] == _lib.ERR_BAD_SHAPE
    out = c_float()
    assert _lib.lib().dctn_lr_schedule_value(None, 0, ctypes.byref(out)) == _lib.ERR_NULL
    assert _lib.lib().dctn_lr_schedule_value(raw_block([(0, 1e-3)]).ctypes.data, 0, None) == _lib.ERR_NULL


def test_step_entry_points_validate_their_arguments_without_a_device():
    lib = _lib.lib()
    adam, sgd = lib.dctn_adam_l2_step_scheduled, lib.dctn_sgd_l2_step_scheduled
    tail = (4, 2, 0.9, 0.999, 1e-8, 0.0, 0.0)
    assert adam(None, 8, 8, 8, 8, None, 8, None, None, *tail, _lib.F32, None) == _lib.ERR_NULL    # no schedule
    assert adam(None, None, 8, 8, 8, None, 8, None, 8, *tail, _lib.F32, None) == _lib.ERR_NULL
    assert adam(None, 8, 8, 8, 8, None, None, None, 8, *tail, _lib.F32, None) == _lib.ERR_NULL    # no state
    assert adam(None, 8, 8, 8, 8, None, 8, None, 8, 0, 0, *tail[2:], _lib.F32, None) == _lib.ERR_BAD_SHAPE
    assert adam(None, 8, 8, 8, 8, None, 8, None, 8, 4, 5, *tail[2:], _lib.F32, None) == _lib.ERR_BAD_SHAPE
    assert adam(None, 8, 8, 8, 8, None, 8, None, 8, *tail, _lib.F64, None) == _lib.ERR_BAD_DTYPE
    assert adam(8, 8, 8, 8, 8, None, 8, None, 8, *tail, _lib.F32, None) == _lib.ERR_BAD_DTYPE     # a master of f32 parameters
    stail = (4, 2, 0.9, 0.0)
    assert sgd(None, 8, 8, 8, None, 8, None, None, *stail, _lib.F32, None) == _lib.ERR_NULL       # no schedule
    assert sgd(None, 8, 8, 8, None, None, None, 8, *stail, _lib.F32, None) == _lib.ERR_NULL       # no state
    assert sgd(None, 8, None, 8, None, 8, None, 8, *stail, _lib.F32, None) == _lib.ERR_NULL
    assert sgd(None, 8, 8, 8, None, 8, None, 8, 4, -1, *stail[2:], _lib.F32, None) == _lib.ERR_BAD_SHAPE
    assert sgd(None, 8, 8, 8, None, 8, None, 8, *stail, _lib.F64, None) == _lib.ERR_BAD_DTYPE
    assert sgd(8, 8, 8, 8, None, 8, None, 8, *stail, _lib.F32, None) == _lib.ERR_BAD_DTYPE


# ------------------------------------------------------------------ interface
EXPECTED = {
    "dctn_lr_schedule_bytes": (c_size, []),
    "dctn_lr_schedule_value": (c_int, [c_void, c_i64, ctypes.POINTER(c_float)]),
    "dctn_adam_l2_step_scheduled": (c_int, [c_void] * 9 + [c_i64, c_i64, c_double, c_double, c_float, c_float, c_float,
                                            c_int, c_void]),
    "dctn_sgd_l2_step_scheduled": (c_int, [c_void] * 8 + [c_i64, c_i64, c_float, c_float, c_int, c_void]),
}


def test_entry_points_are_in_header_library_and_bindings():
    header = open(os.path.join(ROOT, "include", "dctn_amd.h")).read()
    declared = set(re.findall(r"\b(dctn_[a-z0-9_]+)\s*\(", header))
    exported = set()
    for line in subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True,
                               check=True).stdout.splitlines():
        parts = line.split()
        if len(parts) == 3 and parts[1] == "T":
            exported.add(parts[2])
    for name, (res, args) in EXPECTED.items():
        assert name in declared, f"{name} is not declared in include/dctn_amd.h"
        assert name in exported, f"{name} is not exported by {_lib.LIB_PATH}"
        assert name in _lib.SIGNATURES, f"{name} is missing from _lib.SIGNATURES"
        got_res, got_args = _lib.SIGNATURES[name]
        assert got_res is res and list(got_args) == args, name
        fn = getattr(_lib.lib(), name)
        assert fn.restype is res and list(fn.argtypes) == args, name
    assert declared == set(_lib.SIGNATURES)
    assert _lib.lib().dctn_version() >= 510
    # the scheduled step is the unscheduled one with master in front and guard + schedule behind the state block
    adam = list(_lib.SIGNATURES["dctn_adam_l2_step"][1])
    assert EXPECTED["dctn_adam_l2_step_scheduled"][1] == [c_void] + adam[:6] + [c_void, c_void] + adam[6:]


def small_optimizers(schedule):
    from dctn_amd import training

    def params():
        return [torch.nn.Parameter(torch.ones(5)), torch.nn.Parameter(torch.ones(3))]

    return training.FlatAdam(params()[:1], params()[1:], schedule=schedule), training.FlatSGD(params(), schedule=schedule)


def test_optimizers_take_a_schedule_and_refuse_an_assigned_rate():
    from dctn_amd import training

    for cls in (training.FlatAdam, training.FlatSGD):
        p = inspect.signature(cls.__init__).parameters["schedule"]
        assert p.default is None and p.kind is inspect.Parameter.KEYWORD_ONLY
    assert list(inspect.signature(training.make_lr_plateau_hook).parameters) == [
        "schedule", "key", "low_is_good", "factor", "patience", "min_scale"]
    assert list(inspect.signature(LRSchedule.__init__).parameters) == ["self", "device", "knots", "hold"]
    for name in ("value", "set", "state_dict", "load_state_dict", "constant", "warmup", "warmup_cosine", "milestones"):
        assert callable(getattr(LRSchedule, name)), name
    assert isinstance(LRSchedule.scale, property)
    schedule = LRSchedule.warmup("cpu", 1e-3, 10)
    for opt in small_optimizers(schedule):
        assert opt.schedule is schedule
        with pytest.raises(RuntimeError, match=r"schedule\.set.*schedule\.scale"):
            opt.lr = 0.5
    sgd = training.FlatSGD([torch.nn.Parameter(torch.ones(4))], lr=0.25)   # without a schedule: what it always was
    assert sgd.schedule is None and sgd._state is None and sgd.lr == 0.25
    sgd.lr = 0.5
    assert sgd.lr == 0.5 and sgd.state_dict()["lr"] == 0.5 and sgd.state_dict()["steps"] == 0
    with pytest.raises(TypeError):
        training.FlatSGD([torch.nn.Parameter(torch.ones(4))], schedule=object())


def test_state_dict_round_trip_and_set():
    a = LRSchedule("cpu", [(0, 1e-4), (10, 1e-3), (50, 1e-3), (90, 1e-5)], hold=[0, 1, 0, 0])
    a.scale = 0.7
    b = LRSchedule.constant("cpu", 1.0)
    b.load_state_dict(a.state_dict())
    assert b.state_dict() == a.state_dict() and np.array_equal(b.host_block(), a.host_block())
    assert np.array_equal(b._block.numpy(), a._block.numpy())
    assert [bits(b.value(s)) for s in range(120)] == [bits(a.value(s)) for s in range(120)]
    import json

    assert json.loads(json.dumps(a.state_dict())) == a.state_dict()
    b.set([(0, 0.5)])
    assert b.scale == float(np.float32(0.7)) and b.value(3) == float(np.float32(0.5) * np.float32(0.7))
    assert b._block.numpy()[0] == 1 and not b._block.numpy()[5:68].any()   # the old knots are gone from the block
    c = LRSchedule.constant("cpu", 1.0)
    c.run_restored(None, {"schedule": a.host_block()})
    assert c.state_dict() == a.state_dict()


# ------------------------------------------------------------------ the plateau hook
def test_plateau_hook_scales_after_patience_bad_evaluations():
    from dctn_amd.training import make_lr_plateau_hook

    s = LRSchedule.constant("cpu", 1e-3)
    hook = make_lr_plateau_hook(s, "val_mean_ce", True, factor=0.5, patience=2, min_scale=0.2)
    seen = []
    for i, v in enumerate([1.0, 0.9, 0.95, 0.9, 0.91, 0.8, 0.8, 0.8, 0.8, 0.8, 0.8, 0.8, 0.8, 0.8, 0.8]):
        hook({}, {"val_mean_ce": v, "num_iters_done": i})
        seen.append(s.scale)
    #        1.0  0.9  bad1 bad2->x0.5 bad1 better bad1 bad2->0.25 bad1 bad2->0.2 (the floor) ... stays
    f02 = float(np.float32(0.2))
    assert seen == [1.0, 1.0, 1.0, 0.5, 0.5, 0.5, 0.5, 0.25, 0.25, f02, f02, f02, f02, f02, f02]
    assert s.value(0) == float(np.float32(np.float32(1e-3) * np.float32(0.2)))
    up = LRSchedule.constant("cpu", 1e-3)
    hook = make_lr_plateau_hook(up, "val_acc", False, factor=0.1, patience=1)
    for v, want in ((0.5, 1.0), (0.6, 1.0), (0.6, 0.1), (0.7, 0.1), (0.1, 0.01)):
        hook({}, {"val_acc": v})
        assert up.scale == pytest.approx(want, rel=1e-6)
    with pytest.raises(ValueError):
        make_lr_plateau_hook(up, "val_acc", False, factor=1.5, patience=1)
    with pytest.raises(ValueError):
        make_lr_plateau_hook(up, "val_acc", False, factor=0.5, patience=0)
