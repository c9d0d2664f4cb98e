"""`checkpoint.RunState`'s file format held to the PARENT commit's (`-m gpu`): tests/golden/run_state_parent.json and the two
snapshot files beside it were written on an MI355X by tests/golden/make_run_state_parent.py from the commit the record
names, through `RunState`'s public surface only.  Here the code under test rebuilds every recorded case, loads the
parent's files into objects built from other seeds and other hyper-parameters, writes them again, and refuses damaged
copies with the parent's messages.  Eager steps on tiny shapes; no graph is captured.  Every comparison is exact."""
import functools
import json
import os

import numpy as np
import pytest
import torch

from tests.golden import make_run_state_parent as M

pytestmark = pytest.mark.gpu

DEV = M.DEV
with open(M.RECORD) as f:
    RECORD = json.load(f)
GOLDEN = os.path.dirname(M.RECORD)


def _bytes(t):
    return t.detach().contiguous().reshape(-1).view(torch.uint8).cpu().numpy()


def test_the_record_names_its_commit_and_holds_every_case():
    assert len(RECORD["parent_commit"]) == 40 and list(RECORD["cases"]) == list(M.CASES)
    assert set(RECORD["files"]) == set(M.FILES)
    for kind in ("adam", "sgd"):   # every option on and off for both optimizers
        flags = np.array([c[1:] for c in M.CASES.values() if c[0] == kind])
        assert flags.any(0).all() and not flags.all(0).any(), kind
    assert sum(c[0] is None for c in M.CASES.values()) == 1


# ------------------------------------------------------------------ 1. the layout of every case
@pytest.mark.parametrize("name", list(M.CASES))
def test_a_case_rebuilds_to_the_recorded_layout(name):
    got, want = M.layout(M.build_case(name).run), RECORD["cases"][name]
    assert got["entries"] == want["entries"]
    assert got["model"] == want["model"]
    assert got["host"] == want["host"]
    assert {slot: list(v) for slot, v in got["host"].items()} == {slot: list(v) for slot, v in want["host"].items()}
    assert got["arena_bytes"] == want["arena_bytes"]


# ------------------------------------------------------------------ 2. the parent's files, loaded
def _file(name):
    from dctn_amd import checkpoint as C

    path = os.path.join(GOLDEN, M.FILES[name])
    manifest, arena = C.read_file(path)
    blocks = {r["name"]: arena[r["offset"]: r["offset"] + r["bytes"]] for r in manifest["regions"]}
    return path, manifest, arena, blocks


@functools.lru_cache(maxsize=None)
def _loaded(name):
    """Fresh objects from other seeds and hyper-parameters with the parent's file loaded: (case, extras)."""
    case = M.build_case(name, variant=1)
    return case, case.run.load(_file(name)[0])


def _mirrors(case):
    """Every host mirror of a case (no device read)."""
    opt, out = case.opt, {}
    out["opt"] = (opt._lr, opt.l2) + ((opt.betas, opt.eps, opt.weight_decay) if case.kind == "adam" else
                                      (opt.momentum, opt._steps))
    if case.guard is not None:
        out["guard"] = case.guard.max_norm
    if case.src is not None:
        out["src"] = case.src.seed
    if case.schedule is not None:
        out["schedule"] = (case.schedule.knots, case.schedule.hold, case.schedule.scale)
    if case.groups is not None:
        out["groups"] = (case.groups.lr_scales, case.groups.weight_decays, case.groups.frozen)
    if case.trace is not None:
        out["trace"] = (case.trace._last_read, case.trace.lost)
    out["p"] = case.model._p_float
    return out


@pytest.mark.parametrize("name", list(M.FILES))
def test_fresh_objects_load_the_parents_file(name):
    from dctn_amd import checkpoint as C
    from dctn_amd.training import LRSchedule, ParamGroups

    path, manifest, arena, blocks = _file(name)
    assert M.layout(M.build_case(name, variant=1).run)["host"] != manifest["host"]   # the objects start elsewhere
    case, extras = _loaded(name)
    assert extras == RECORD["files"][name]["extras"] == M.EXTRAS
    run, opt, host = case.run, case.opt, manifest["host"]
    # every region's device bytes are the file's
    assert run.names == list(blocks)
    for region, t in zip(run.names, run.tensors):
        assert np.array_equal(_bytes(t), blocks[region]), region
    # every host mirror is what the manifest and the blocks say
    saved = host["optimizer"]
    assert opt._lr == saved["lr"] == (M.ADAM if case.kind == "adam" else M.SGD)[0]["lr"] and opt.l2 == saved["l2"]
    assert opt.t == M.STEPS
    if case.kind == "adam":
        assert (list(opt.betas), opt.eps, opt.weight_decay) == (saved["betas"], saved["eps"], saved["weight_decay"])
        assert isinstance(opt.betas, tuple) and opt.betas == M.ADAM[0]["betas"]
    else:
        assert (opt.momentum, opt._steps) == (saved["momentum"], saved["steps"]) == (M.SGD[0]["momentum"], M.STEPS)
    assert case.guard.max_norm == host["guard"]["max_norm"] == M.MAX_NORM[0]
    assert case.src.seed == host["batch_source"]["seed"] == M.SEEDS[0]["batch"]
    assert case.src.state_dict() == {"seed": M.SEEDS[0]["batch"], "batches_done": M.STEPS}
    if case.schedule is None:
        assert opt.lr == saved["lr"]
    else:
        knots, hold, scale = LRSchedule.decode(blocks["optimizer.schedule"])
        assert (case.schedule.knots, case.schedule.hold, case.schedule.scale) == (knots, hold, scale)
        assert [k for k, _ in knots] == [k for k, _ in M.KNOTS[0][0]] and hold == M.KNOTS[0][1] and scale == M.SCALE[0]
        assert opt.lr == case.schedule.value(M.STEPS)
    words = blocks["optimizer.groups"].view("<i4")
    floats, k, G = words.view("<f4"), len(case.groups), ParamGroups
    assert case.groups.lr_scales == [float(x) for x in floats[G._SCALE: G._SCALE + k]] == [*M.GROUP_LR_SCALES[0], 1.0]
    assert case.groups.weight_decays == [float(x) for x in floats[G._WD: G._WD + k]]
    assert case.groups.frozen == [bool(x & 1) for x in words[G._FLAGS: G._FLAGS + k]] == [False, False, True]
    assert case.groups.steps == [int(x) for x in words[G._STEPS: G._STEPS + k]] == [M.STEPS, M.STEPS, 0]
    state = C.read_model_state(path)
    assert case.model._p_float == float(state["p"]) == (float(state["p"].new_tensor(M.KEEP[0])) if case.on.dropout else 1.0)
    if case.on.dropout:
        assert case.model.dropout_state_dict() == {"seed": M.SEEDS[0]["dropout"], "draws_done": M.STEPS}
    if case.trace is not None:
        assert case.trace.read().size == 0 and case.trace.lost == 0
        assert case.trace.state_dict() == {"records_done": M.STEPS, "capacity": M.CAPACITY}


# ------------------------------------------------------------------ 3. and written again
@pytest.mark.parametrize("name", list(M.FILES))
def test_the_loaded_state_saves_to_the_parents_bytes(name, tmp_path):
    from dctn_amd import checkpoint as C

    _, manifest, arena, _ = _file(name)
    case, extras = _loaded(name)
    again = case.run.snapshot(extras).save(str(tmp_path / "again.dctn"))
    manifest2, arena2 = C.read_file(again)
    assert np.array_equal(arena2, arena)
    assert manifest2 == manifest   # parsed: regions, digests, model entries, host scalars, extras
    assert os.path.getsize(again) == RECORD["files"][name]["bytes"]


# ------------------------------------------------------------------ 4. damaged copies
@pytest.mark.parametrize("name", list(M.FILES))
def test_damaged_copies_are_refused_with_the_parents_words_before_anything_is_written(name, tmp_path):
    path = _file(name)[0]
    case = M.build_case(name, variant=1)
    before = [t.clone() for t in case.run.tensors]
    mirrors = _mirrors(case)
    for how in M.REFUSALS:
        bad = M.damaged_copy(path, how, str(tmp_path / f"{how}.dctn"))
        with pytest.raises(ValueError) as e:
            case.run.load(bad)
        assert str(e.value) == RECORD["files"][name]["refusals"][how].replace("{path}", bad), how
        torch.cuda.synchronize(DEV)
        for region, t, b in zip(case.run.names, case.run.tensors, before):
            assert np.array_equal(_bytes(t), _bytes(b)), (how, region)
        assert _mirrors(case) == mirrors, how
