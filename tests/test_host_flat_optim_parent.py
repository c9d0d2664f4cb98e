"""The flat optimizers show on the host what the parent commit's classes showed.

tests/golden/flat_optim_host_parent.json was written by tests/golden/make_flat_optim_host_parent.py from the commit the
record names: per case every key, key order, value and value type of ``state_dict()`` and ``run_host()``, the names of
``run_regions()``, ``lr``, ``t``, the step block's 16 bytes, the descriptor's pointers and ``_what`` - as built, after
``lr`` was assigned, after ``load_state_dict`` and after ``run_restored`` - and the type and text of every refusal that
needs no device.  Every case is rebuilt here with the code under test on CPU tensors and compared for equality.  No GPU.
"""
import functools
import json

import pytest

from tests.golden import make_flat_optim_host_parent as M


@functools.lru_cache(maxsize=None)
def _record():
    with open(M.RECORD) as f:
        return json.load(f)


def test_the_record_holds_exactly_the_cases_of_the_script():
    assert list(_record()["cases"]) == M.all_cases() and len(M.all_cases()) == 21


@pytest.mark.parametrize("name", M.all_cases())
def test_the_optimizer_shows_what_the_parents_showed(name):
    want, got = M.unpacked(_record()["cases"][name]), M.run(name)
    assert list(got) == list(want)
    for moment in want:
        for what in want[moment]:
            assert got[moment][what] == want[moment][what], f"{name}: {moment}: {what}"
        assert list(got[moment]) == list(want[moment])


def test_every_refusal_has_the_parents_type_and_text():
    want, got = _record()["refusals"], M.refusals()
    assert list(got) == list(want)
    for what in want:
        assert got[what] == want[what], what
