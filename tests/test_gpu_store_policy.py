"""The two buffers a register-family step hands from one kernel to the next, and the stores that write them
(DCTN_WT_FEATURES / DCTN_WT_TILES in common.h; eps_mfma.hip and eps_q2f32.hip):

* the dCore kernels' partial tiles: thread t sums elements 4 t .. 4 t + 3 of the workgroup's tile and writes them with one
  16-byte buffer store (MT = 2: every dCore thread, MT = 1: the first half of them); eps_head_reduce_k /
  eps_bwd_dcore_reduce_k / eps_q2f32_finish_k sum the tiles of EVERY workgroup of the grid, empty ones included;
* the forward's feature buffer (the blocked4 block store in bf16, the 16-byte row store in float32), read by the dW
  product of the backward: a block that did not reach memory shows in dW.

Under a write-through policy the consumer reads both from the memory side, so the same cases hold whichever value the
library was built with.  Exact inputs (tests/exact_inputs.py, one-hot pixels: closed-form oracle): every sum is exact in
any order, so logits, dCore, dW and dBias are compared bit for bit (run_head asserts all four and the kernel names).  The
oracle of a shape is computed once and shared by the modes.

The fused bf16 head takes F = positions x O that are multiples of 8, which N = 8 (C = 2, K = 2) does not give on 6 x 6
and 12 x 12 images (25 and 121 positions); its one- and two-position-group shapes are 5 x 5 (16 positions) and 11 x 11
(100).  N = 8 runs the kernel's other join (A = 16: not the LDST path), which is unchanged and stays covered here."""
import functools

import pytest
import torch

from tests.guarded_buffers import guarded
from tests.test_gpu_exact import HEAD_MODES, head_operands, head_oracle, run_head

pytestmark = pytest.mark.gpu
BF16_FWD, BF16_BWD = "eps_head_fwd_mfma_q2reg", "eps_head_bwd_mfma_q2reg"
F32_FWD, F32_BWD = "eps_head_fwd_q2f32", "eps_head_bwd_q2f32"
# (C, K, size of the one-group image, size of the two-group image)
LAYERS = {9: (1, 3, 6, 12), 8: (2, 2, 5, 11)}
BATCHES = [(1, 10), (5, 16), (47, 10), (49, 16)]   # (B, classes)


@functools.lru_cache(maxsize=None)
def case(C, K, size, B, O, cout):
    ops = head_operands(C, K, size, size, B, O, cout, torch.bfloat16, seed=C + K + size + B + O + cout, two_hot=False)
    return ops, head_oracle(*ops, closed_form=True)


def check_bf16(C, K, size, B, O, cout, mode, arena=None):
    (core, x, w, bias, g), oracle = case(C, K, size, B, O, cout)
    fused, ffwd, blocked = HEAD_MODES[mode]
    fwd, bwd = (BF16_FWD, BF16_BWD) if fused else ("linear_head_fwd_mfma", "eps_bwd_mfma_q2reg")
    run_head(core, x, w, bias, g, torch.bfloat16, fused=fused, fused_fwd=ffwd, blocked=blocked, oracle=oracle, fwd=fwd, bwd=bwd,
             tag=f"N={C * K * K} {size}x{size} B={B} O={O} classes={cout} {mode}", arena=arena)


def check_f32(size, B, cout, arena=None):
    (core, x, w, bias, g), oracle = case(1, 3, size, B, 4, cout)
    run_head(core, x, w, bias, g, torch.float32, fused=True, fused_fwd=True, blocked=False, oracle=oracle, fwd=F32_FWD,
             bwd=F32_BWD, tag=f"float32 {size}x{size} B={B} classes={cout}", arena=arena)


# ---- partial tiles
# O = 4: MT = 2, every dCore thread stores 16 bytes; O = 2: MT = 1, threads 0-255 do.  One and two position groups.
# B = 1: one live wave; 5; 47 and 49: one sample per wave, the last chunk block partly empty.  "unfused": the same join
# in front of eps_bwd_dcore_reduce_k (no head: HEADC = 0).
@pytest.mark.parametrize("mode", ["fused_blocked4", "fused_rowmajor", "unfused"])
@pytest.mark.parametrize("groups", [1, 2])
@pytest.mark.parametrize("O", [4, 2])
@pytest.mark.parametrize("N", [9, 8])
def test_partial_tiles(N, O, groups, mode):
    C, K = LAYERS[N][:2]
    for B, cout in BATCHES:
        check_bf16(C, K, LAYERS[N][1 + groups], B, O, cout, mode)


@pytest.mark.parametrize("mode", ["fused_blocked4", "fused_rowmajor"])
@pytest.mark.parametrize("O", [4, 2])
def test_tiles_of_empty_workgroups_are_written(O, mode):
    """12 x 12, B = 47: 6 chunk blocks x 2 position groups = 12 live workgroups in a grid rounded up to 16; the finishing
    kernel sums 16 tiles.  Every buffer, the workspace included, starts as NaN (0xFF bytes) between intact guards."""
    with guarded(fill=0xFF) as arena:
        check_bf16(1, 3, 12, 47, O, 10, mode, arena=arena)
    arena.check()


# ---- feature block
# 6 x 6: F = 64, ng < 4 at B = 1, 3 and 5 (the second block holds one sample and three of zeros); 28 x 28: B = 5, and
# B = 1028 with two groups per workgroup.  The backward behind it forms dW from the block.
@pytest.mark.parametrize("size,B", [(6, 1), (6, 3), (6, 5), (28, 5), (28, 1028)])
def test_feature_block(size, B):
    check_bf16(1, 3, size, B, 4, 10, "fused_blocked4")


# ---- float32 (eps_q2f32.hip): one case of each kind
def test_partial_tiles_f32():
    with guarded(fill=0xFF) as arena:
        check_f32(12, 47, 10, arena=arena)
    arena.check()


def test_feature_rows_f32():
    check_f32(28, 5, 10)
