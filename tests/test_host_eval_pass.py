"""The padded sequential draw and the graphed evaluation pass, the parts that need no GPU: the host restatement of the
padded walk, the constants, and the checks a source makes before it touches a device."""
import inspect
import os
import re

import pytest
import torch

from dctn_amd import _lib
from dctn_amd import batches as B


def test_padded_walk_of_ten_samples_in_batches_of_four():
    n, G = 10, 4
    S = B.steps_per_epoch(n, G, drop_last=False)
    assert S == 3
    assert [B.expected_padded_indices(k, n, G) for k in range(S)] == [[0, 1, 2, 3], [4, 5, 6, 7], [8, 9, -1, -1]]
    walked = [i for k in range(S) for i in B.expected_padded_indices(k, n, G) if i >= 0]
    assert walked == list(range(n))


def test_no_padding_when_the_batch_divides_the_set():
    n, G = 12, 4
    for k in range(7):   # S = 3 with and without the remainder: the same walk, wrap included
        assert B.expected_padded_indices(k, n, G) == B.expected_indices(0, k, n, G, shuffle=False)
        assert -1 not in B.expected_padded_indices(k, n, G)


def test_two_ranks_take_fixed_slots_and_one_shard_may_be_all_padding():
    n, G = 10, 4
    assert B.expected_padded_indices(2, n, G, rank=0, world=2) == [8, 9]
    assert B.expected_padded_indices(2, n, G, rank=1, world=2) == [-1, -1]
    for k in range(3):
        halves = [B.expected_padded_indices(k, n, G, rank=r, world=2) for r in range(2)]
        assert halves[0] + halves[1] == B.expected_padded_indices(k, n, G)
    assert B.expected_padded_indices(2, 9, G, rank=0, world=2) == [8, -1]   # half padding


def test_the_counter_wraps_at_the_padded_number_of_batches():
    n, G, S = 10, 4, 3
    for r, w in ((0, 1), (1, 2)):
        assert B.expected_padded_indices(S, n, G, r, w) == B.expected_padded_indices(0, n, G, r, w)
        assert B.expected_padded_indices(2 * S + 2, n, G, r, w) == B.expected_padded_indices(2, n, G, r, w)
    with pytest.raises(ValueError):
        B.expected_padded_indices(0, 3, 4)          # G <= n, as everywhere
    with pytest.raises(ValueError):
        B.expected_padded_indices(0, 10, 4, 0, 3)   # the global batch divides over the ranks


def test_flag_value_and_version():
    assert _lib.BATCH_PAD_TAIL == 2 and _lib.BATCH_IDENTITY_ORDER == 1
    assert _lib.lib().dctn_version() >= 504
    # the header defines the flag as a macro (it says why): the same value, once, and distinct from the enum's flag
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "dctn_amd.h")).read()
    defined = re.findall(r"^#define\s+DCTN_BATCH_PAD_TAIL\s+(\d+)\s*$", header, re.M)
    assert [int(v) for v in defined] == [_lib.BATCH_PAD_TAIL]
    identity = re.findall(r"DCTN_BATCH_IDENTITY_ORDER\s*=\s*(\d+)", header)
    assert [int(v) for v in identity] == [_lib.BATCH_IDENTITY_ORDER] and _lib.BATCH_PAD_TAIL & _lib.BATCH_IDENTITY_ORDER == 0


def test_the_flag_is_refused_without_the_identity_order_before_any_launch():
    P = 64   # any non-null address: nothing is launched
    draw = _lib.lib().dctn_batch_draw

    def d(flags):
        return draw(P, P, P, P, P, P, P, 37, 8, 8, 0, 25, 2, _lib.BATCH_SRC_U8_TABLE, flags, _lib.F32, None)

    assert d(_lib.BATCH_PAD_TAIL) == _lib.ERR_BAD_SHAPE
    assert d(4) == _lib.ERR_BAD_SHAPE and d(_lib.BATCH_IDENTITY_ORDER | _lib.BATCH_PAD_TAIL | 4) == _lib.ERR_BAD_SHAPE


def _plan(shuffle, drop_last=True, n=10, G=4):
    """A source with its host-side plan only: what the constructors compute before they look for a device."""
    src = B.DeviceBatches.__new__(B.DeviceBatches)
    src._plan(n, torch.zeros(n, dtype=torch.int64), G, 1, shuffle, drop_last, 0, 1)
    return src


def test_padded_draw_of_a_shuffled_plan_raises_before_it_touches_a_device():
    with pytest.raises(ValueError, match="shuffle=False"):
        _plan(shuffle=True).draw_padded_into(None, None, None)
    src = _plan(shuffle=False)
    assert src.padded_steps == 3 and src.steps == 2
    assert src.expected_padded_indices(2) == [8, 9, -1, -1]
    assert _plan(shuffle=False, drop_last=False).padded_steps == 3
    assert _plan(shuffle=False, n=12).padded_steps == 3


def test_graphed_score_and_the_hook_exist_with_their_signatures():
    from dctn_amd import evaluation as E

    params = inspect.signature(E.GraphedScore.__init__).parameters
    assert list(params) == ["self", "model", "src", "warmup"] and params["warmup"].default == 1
    for name in ("launch", "read", "__call__"):
        assert callable(getattr(E.GraphedScore, name))
    with pytest.raises(ValueError, match="shuffle=False"):
        E.GraphedScore(torch.nn.Identity(), _plan(shuffle=True))

    class Scorer:
        def __init__(self, log, name, result):
            self.log, self.name, self.result = log, name, result

        def launch(self):
            self.log.append(("launch", self.name))

        def read(self):
            self.log.append(("read", self.name))
            return self.result

    log = []
    hook = E.make_evaluation_hook(Scorer(log, "train", (1.25, 0.5)), Scorer(log, "val", (2.0, 0.25)))
    st_it = {"num_iters_done": 3}
    hook({}, st_it)
    assert log == [("launch", "train"), ("launch", "val"), ("read", "train"), ("read", "val")]
    assert st_it == {"num_iters_done": 3, "train_mean_ce": 1.25, "train_acc": 0.5, "val_mean_ce": 2.0, "val_acc": 0.25}
    from dctn_amd.training import _checkpoint_tag

    assert _checkpoint_tag(st_it) == "nitd=0000003_tracc=0.5000_vacc=0.2500_trmce=1.2500_vmce=2.0000"
