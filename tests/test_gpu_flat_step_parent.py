"""The flat optimizers' step kernels leave, in every buffer, the bits the parent commit's kernels left.

tests/golden/flat_step_parent.json was written on an MI355X by tests/golden/make_flat_step_parent.py from the commit the
record names: per case, step and buffer a 64-bit prefix of the SHA-256 of the buffer's bytes.  Every case is rebuilt here
with the code under test; no case is skipped and no difference is tolerated.  The other step-kernel tests compare the
forms of a kernel with each other, and would pass if all of them changed together.
"""
import functools
import json

import pytest

from tests.golden import make_flat_step_parent as M

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _record():
    with open(M.RECORD) as f:
        return json.load(f)


def test_the_record_holds_exactly_the_cases_of_the_script():
    assert list(_record()["cases"]) == M.all_cases() and len(M.all_cases()) == 350


@pytest.mark.parametrize("variant", list(M.VARIANTS))
@pytest.mark.parametrize("optimizer", list(M.OPTIMIZERS))
def test_every_buffer_holds_the_parents_bits(optimizer, variant):
    cases = _record()["cases"]
    wrong = []
    for name in M.case_names(optimizer, variant):
        want, got = cases[name], M.run(name)
        assert got["buffers"] == want["buffers"] and len(got["steps"]) == len(want["steps"]), name
        first = next(((s, b) for s, (g_row, w_row) in enumerate(zip(got["steps"], want["steps"]))
                      for b, g, w in zip(want["buffers"], g_row, w_row) if g != w), None)
        if first is not None:
            same_inputs = got["inputs"] == want["inputs"]
            wrong.append(f"{name}: step {first[0]}, buffer {first[1]!r} differs first; the inputs' digest is "
                         + ("the record's" if same_inputs else "NOT the record's: another torch, not a kernel"))
    assert not wrong, f"{len(wrong)} case(s) differ from the parent's record:\n" + "\n".join(wrong)
