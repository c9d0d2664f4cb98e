"""CPU tests (no GPU) of the fused head's sample-blocked feature layout option: the header and the binding agree on
the bit, and the host-side validation of the entry points treats it as documented in include/dctn_amd.h."""
import os
import re

import torch

from dctn_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_enum(name):
    header = open(os.path.join(ROOT, "include", "dctn_amd.h")).read()
    m = re.search(rf"\b{name}\s*=\s*([^,/]+)", header)
    assert m, name
    return eval(m.group(1).replace("|", " | "))   # "1 << 12", "(1 << 8) | ..."


def test_blocked_features_bit_matches_the_header():
    assert header_enum("DCTN_OPT_HEAD_FEATURES_BLOCKED4") == _lib.OPT_HEAD_FEATURES_BLOCKED4 == 1 << 12
    assert header_enum("DCTN_OPT_ALL") & _lib.OPT_HEAD_FEATURES_BLOCKED4
    for other in (_lib.OPT_F32_PREFER_HALVES, _lib.OPT_SMALL_CHUNKS, _lib.OPT_MAIN_KERNEL_ONLY, _lib.OPT_GENERIC_KERNELS):
        assert other & _lib.OPT_HEAD_FEATURES_BLOCKED4 == 0 and header_enum("DCTN_OPT_ALL") & other


def test_only_the_fused_head_takes_the_blocked_features_bit():
    lib, blk = _lib.lib(), _lib.OPT_HEAD_FEATURES_BLOCKED4
    bf16 = _lib._DTYPE_CODE[torch.bfloat16]
    cfg2 = (1, 1024, 28, 28, 2, 3, 4)
    # host-only queries of the other entry points decline it (-1 / 0 bytes) ...
    assert lib.dctn_eps_family(*cfg2, bf16, 0) == 1 and lib.dctn_eps_family(*cfg2, bf16, blk) == -1
    assert lib.dctn_eps_bwd_workspace_bytes(*cfg2, bf16, blk, 0, 1) == 0
    # ... the fused head's workspace query sizes the same workspace with and without it
    want = lib.dctn_eps_head_bwd_workspace_bytes(*cfg2, 10, bf16, 0)
    assert want > 0 and lib.dctn_eps_head_bwd_workspace_bytes(*cfg2, 10, bf16, blk) == want
