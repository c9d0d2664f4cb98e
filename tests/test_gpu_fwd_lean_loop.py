"""The step loop of eps_fwd_head_q2reg_t_k (eps_mfma.hip) as it stands behind the DCTN_FWD_* switches of common.h:

* a step takes its lane's offsets from a table of all npg * 64 (position group, lane) pairs that the workgroup fills
  once in LDS, and splits its ticket into (sample, position group) by a multiply-shift;
* the first group's tickets are set in front of the barrier that publishes the core, and a wave's first window goes out
  behind the core's loads;
* the parameter block is read once at entry.

Exact inputs (tests/exact_inputs.py, one-hot pixels: closed-form oracle): every sum is exact in any order, so a wrong
table entry, ticket or window shows as a bit difference in logits, features or gradients (run_head asserts logits,
dCore, dW, dBias and the kernel names; dW is formed from the features the forward left).  The oracle of a shape is
computed once and shared by the two feature layouts.

N = 8 (C = 2, K = 2) runs on 5 x 5 and 11 x 11 images (16 and 100 positions): the fused bf16 head takes F = positions x O
that are multiples of 8."""
import functools

import pytest
import torch

from tests.test_gpu_exact import HEAD_MODES, head_operands, head_oracle, run_head

pytestmark = pytest.mark.gpu
MODES = ["fused_blocked4", "fused_rowmajor"]
FWD, BWD = "eps_head_fwd_mfma_q2reg", "eps_head_bwd_mfma_q2reg"


@functools.lru_cache(maxsize=None)
def case(C, K, size, B, cout):
    ops = head_operands(C, K, size, size, B, 4, cout, torch.bfloat16, seed=C + K + size + B + cout, two_hot=False)
    return ops, head_oracle(*ops, closed_form=True)


def check(C, K, size, B, cout, mode):
    (core, x, w, bias, g), oracle = case(C, K, size, B, cout)
    fused, ffwd, blocked = HEAD_MODES[mode]
    run_head(core, x, w, bias, g, torch.bfloat16, fused=fused, fused_fwd=ffwd, blocked=blocked, oracle=oracle, fwd=FWD, bwd=BWD,
             tag=f"N={C * K * K} {size}x{size} B={B} classes={cout} {mode}")


# ---- position table
# N = 9: 6 x 6 (16 live lanes of one group), 10 x 10 (64 positions: exactly one full group), 12 x 12 (two groups, 36 live
# lanes in the second), 28 x 28 (eleven groups, 36 live lanes in the last).  N = 8: one and two groups.  B = 5: every
# sample slot of a group and a second workgroup.
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("C,K,size", [(1, 3, 6), (1, 3, 10), (1, 3, 12), (1, 3, 28), (2, 2, 5), (2, 2, 11)])
def test_position_table(C, K, size, mode):
    check(C, K, size, 5, 10, mode)


# ---- ticket -> (sample, position group); waves that run 0, 1, 2 and 3 steps
# 28 x 28 at B = 1 .. 4: 11, 22, 33 and 44 steps for 16 waves: static tickets only, then the first drawn ones.
# 12 x 12 at B = 4: 8 steps, half the first tickets dead.
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("size,B", [(28, 1), (28, 2), (28, 3), (28, 4), (12, 4)])
def test_tickets_and_step_counts(size, B, mode):
    check(1, 3, size, B, 10, mode)


# ---- group loop and the reset of the step counter
# 12 x 12 at B = 1028: two groups per workgroup, the last ragged.  6 x 6 at B = 2052: three groups.  6 x 6 at B = 5: a
# second workgroup with one sample.
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("size,B", [(12, 1028), (6, 2052), (6, 5)])
def test_group_loop_and_counter_reset(size, B, mode):
    check(1, 3, size, B, 10, mode)


# ---- 2 and 16 classes: the head product behind the loop is indexed by class
@pytest.mark.parametrize("size,B,cout", [(12, 5, 2), (28, 3, 16)])
def test_other_class_counts(size, B, cout):
    check(1, 3, size, B, cout, "fused_blocked4")
