"""Host-side checks of the colour batch source (no GPU needed): the two entry points are declared, exported and bound,
they validate their arguments before any launch, the kernel names come from a table, `colour_table` indexed by the bytes
is bit for bit the reference's colour pipeline applied to the expanded tensor, `channel_moments` meets torch's float64
mean and population std, and `DeviceBatches.from_colour` raises what the other constructors raise."""
import os
import re
import subprocess

import pytest
import torch

from dctn_amd import _lib
from dctn_amd import batches as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dctn_batch_draw_cols", "dctn_batch_gather_cols")
DTYPES = [torch.float32, torch.bfloat16, torch.float64]


def test_new_entry_points_are_in_header_library_and_bindings():
    header = open(os.path.join(ROOT, "include", "dctn_amd.h")).read()
    declared = set(re.findall(r"\b(dctn_[a-z0-9_]+)\s*\(", header))
    exported = set()
    for line in subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True,
                               check=True).stdout.splitlines():
        parts = line.split()
        if len(parts) == 3 and parts[1] == "T":
            exported.add(parts[2])
    for name in NEW:
        assert name in declared, f"{name} is not declared in include/dctn_amd.h"
        assert name in exported, f"{name} is not exported by {_lib.LIB_PATH}"
        assert name in _lib.SIGNATURES, f"{name} is missing from _lib.SIGNATURES"
    # the same argument lists as the grey-scale calls, the source kind replaced by the second width
    assert _lib.SIGNATURES["dctn_batch_draw_cols"] == _lib.SIGNATURES["dctn_batch_draw"]
    assert _lib.SIGNATURES["dctn_batch_gather_cols"] == _lib.SIGNATURES["dctn_batch_gather"]
    assert _lib.BATCH_SRC_COLOUR not in (_lib.BATCH_SRC_U8_TABLE, _lib.BATCH_SRC_ROWS)


def test_version():
    assert _lib.lib().dctn_version() >= 506


def test_entry_points_validate_their_arguments_without_a_device():
    L = _lib
    draw, gather = L.lib().dctn_batch_draw_cols, L.lib().dctn_batch_gather_cols
    IDENTITY, PAD = L.BATCH_IDENTITY_ORDER, L.BATCH_PAD_TAIL
    P = 64   # any non-null address: nothing is launched

    def d(src=P, table=P, labels=P, x=P, y=P, idx=P, state=P, n=37, G=8, Bl=8, off=0, pixels=25, C=3, W=4, flags=0,
          dtype=L.F32):
        return draw(src, table, labels, x, y, idx, state, n, G, Bl, off, pixels, C, W, flags, dtype, None)

    def g(src=P, table=P, labels=P, sample=P, x=P, y=P, idx=P, n=37, count=8, pixels=25, C=3, W=4, dtype=L.F32):
        return gather(src, table, labels, sample, x, y, idx, n, count, pixels, C, W, dtype, None)

    for name in ("src", "table", "labels", "x", "y", "idx", "state"):
        assert d(**{name: None}) == L.ERR_NULL, name
    for name in ("src", "table", "labels", "sample", "x", "y", "idx"):
        assert g(**{name: None}) == L.ERR_NULL, name
    assert d(n=0) == L.ERR_BAD_SHAPE and g(n=0) == L.ERR_BAD_SHAPE
    assert d(n=1 << 31, G=8) == L.ERR_BAD_SHAPE and g(n=1 << 31) == L.ERR_BAD_SHAPE
    assert d(n=7, G=8) == L.ERR_BAD_SHAPE                     # G > n
    assert d(G=0, Bl=0) == L.ERR_BAD_SHAPE
    assert d(Bl=0) == L.ERR_BAD_SHAPE and g(count=0) == L.ERR_BAD_SHAPE
    assert d(Bl=4, off=5) == L.ERR_BAD_SHAPE                  # the shard ends beyond the global batch
    assert d(Bl=4, off=-1) == L.ERR_BAD_SHAPE
    assert d(pixels=0) == L.ERR_BAD_SHAPE and g(pixels=0) == L.ERR_BAD_SHAPE
    assert d(pixels=1 << 31) == L.ERR_BAD_SHAPE
    # the widths: 1 <= C <= 4, W = C or C + 1, W <= 4
    assert d(C=0, W=1) == L.ERR_BAD_SHAPE and g(C=0, W=1) == L.ERR_BAD_SHAPE
    assert d(C=3, W=0) == L.ERR_BAD_SHAPE and g(C=-1, W=1) == L.ERR_BAD_SHAPE
    assert d(C=5, W=5) == L.ERR_UNSUPPORTED and g(C=5, W=5) == L.ERR_UNSUPPORTED
    assert d(C=5, W=4) == L.ERR_UNSUPPORTED
    assert d(C=3, W=2) == L.ERR_UNSUPPORTED and g(C=3, W=2) == L.ERR_UNSUPPORTED          # width < src_channels
    assert d(C=2, W=4) == L.ERR_UNSUPPORTED and g(C=1, W=3) == L.ERR_UNSUPPORTED          # width > src_channels + 1
    assert d(C=4, W=5) == L.ERR_UNSUPPORTED and g(C=4, W=5) == L.ERR_UNSUPPORTED          # width = 5
    # the flags
    assert d(flags=4) == L.ERR_BAD_SHAPE and d(flags=IDENTITY | PAD | 4) == L.ERR_BAD_SHAPE
    assert d(flags=PAD) == L.ERR_BAD_SHAPE                    # PAD_TAIL without IDENTITY_ORDER
    assert d(dtype=7) == L.ERR_BAD_DTYPE and g(dtype=3) == L.ERR_BAD_DTYPE and d(dtype=-1) == L.ERR_BAD_DTYPE
    # the order of the checks: shape before dtype before the supported widths
    assert d(n=0, dtype=7, W=5) == L.ERR_BAD_SHAPE and d(dtype=7, W=5) == L.ERR_BAD_DTYPE


def test_kernel_names_come_from_a_table():
    """tests/test_host_buffer_contract.py asks for a GUARDED entry for every LITERAL name in a dctn_set_last_kernel call;
    the colour kernels report theirs through a table, as the batch kernels do, and tests/test_gpu_colour_source.py holds
    them to the buffer contract."""
    src = open(os.path.join(ROOT, "dctn_amd", "csrc", "colour_source.hip")).read()
    assert "dctn_set_last_kernel" not in src
    call = open(os.path.join(ROOT, "dctn_amd", "csrc", "batch_call.hip")).read()   # the one table of all batch kernels
    calls = re.findall(r"dctn_set_last_kernel\((.*?)\);", call, re.S)
    assert len(calls) == 1 and '"' not in calls[0] and "BATCH_KERNEL_NAMES[" in calls[0]
    names = set(re.findall(r'"(colour_[a-z0-9_]+)"', call))
    assert names == {f"colour_{op}_{dt}" for op in ("draw", "gather") for dt in ("f32", "f64", "bf16")}
    # the order has one definition: both sources take it from the shared header, and neither restates it
    batch = open(os.path.join(ROOT, "dctn_amd", "csrc", "batch_source.hip")).read()
    for text in (src, batch):
        assert '#include "draw_order.h"' in text and "perm_once(unsigned" not in text and "struct BatchState" not in text
    assert "draw_order.h" in open(os.path.join(ROOT, "dctn_amd", "csrc", "Makefile")).read()


# ------------------------------------------------------------------ the table against the reference's pipeline
MU = torch.tensor([0.4914, 0.4822, 0.4465], dtype=torch.float64)
SIGMA = torch.tensor([0.2470, 0.2435, 0.2616], dtype=torch.float64)
NU = (1.46, 0.83, 1.21)
VARIANTS = {
    "normalised_with_constant": dict(mean=MU, std=SIGMA, constant_channel=0.75),
    "nu_only": dict(),
    "normalised": dict(mean=MU, std=SIGMA),
    "constant": dict(constant_channel=-1.5),
}


def _bytes():
    g = torch.Generator().manual_seed(0)
    images = torch.randint(0, 256, (50, 6, 6, 3), dtype=torch.uint8, generator=g)
    images[0, 0, 0] = torch.tensor([0, 255, 0], dtype=torch.uint8)
    images[1, 0, 0] = torch.tensor([255, 0, 255], dtype=torch.uint8)
    return images


def _pipeline(images, nu, mean=None, std=None, constant_channel=None):
    """The published formula on the WHOLE expanded tensor, in the reference's order (dataset_loading.py:349-375):
    to_tensor's float32 u8 / 255 as (1, n, H, W, C); in place, minus the float64 channel means and over the float64 channel
    deviations; a concatenated constant channel; in place, times the float32 nu (with 1.0 for the constant channel)."""
    x = images.float().div(255).unsqueeze(0)
    if mean is not None:
        x -= mean
        x /= std
    if constant_channel is not None:
        x = torch.cat((x, constant_channel * torch.ones_like(x[:, :, :, :, :1])), dim=4)
        nu = nu + (1.0,)
    x *= torch.tensor(nu)
    return x


def _lookup(table, images):
    """x[0, s, h, w, c] = table[c][byte] for the source channels, table[c][0] for a constant one."""
    C = images.shape[-1]
    cols = [table[c][images[..., c].long()] for c in range(C)]
    cols += [table[c][torch.zeros_like(images[..., 0]).long()] for c in range(C, table.shape[0])]
    return torch.stack(cols, dim=-1).unsqueeze(0)


def _bits(t):
    return t.contiguous().view(torch.uint8)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16", "f64"])
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_colour_table_is_the_reference_pipeline_per_byte(variant, dtype):
    images, kw = _bytes(), VARIANTS[variant]
    assert int(images.min()) == 0 and int(images.max()) == 255
    table = B.colour_table(3, nu=NU, dtype=dtype, **kw)
    W = 3 + ("constant_channel" in kw)
    assert table.shape == (W, 256) and table.dtype == dtype and table.is_contiguous()
    full = _pipeline(images, NU, **kw)
    assert full.dtype == torch.float32 and full.shape == (1, 50, 6, 6, W)
    want = full.to(dtype)   # the model dtype is a cast of the float32 pipeline
    assert torch.equal(_bits(_lookup(table, images)), _bits(want))
    if "constant_channel" in kw:
        assert len(set(table[3].tolist())) == 1 and float(table[3, 0]) == float(torch.tensor(kw["constant_channel"]).to(dtype))


def test_colour_table_arguments():
    assert B.colour_table(1, nu=2.0, dtype=torch.float32).shape == (1, 256)
    assert torch.equal(B.colour_table(2, nu=2.0, dtype=torch.float32), B.colour_table(2, nu=(2.0, 2.0), dtype=torch.float32))
    assert B.colour_table(4, nu=1.0, dtype=torch.float64).shape == (4, 256)
    with pytest.raises(NotImplementedError):
        B.colour_table(5, nu=1.0, dtype=torch.float32)
    with pytest.raises(NotImplementedError):
        B.colour_table(4, nu=1.0, constant_channel=1.0, dtype=torch.float32)     # five columns
    with pytest.raises(ValueError):
        B.colour_table(3, nu=(1.0, 2.0), dtype=torch.float32)
    with pytest.raises(ValueError):
        B.colour_table(3, nu=NU, mean=MU, dtype=torch.float32)                   # mean without std
    with pytest.raises(ValueError):
        B.colour_table(3, nu=NU, mean=MU[:2], std=SIGMA[:2], dtype=torch.float32)
    with pytest.raises(TypeError):
        B.colour_table(3, nu=NU, dtype=torch.float16)


def test_channel_moments_meet_the_float64_mean_and_population_std():
    """Both sides are float64 sums of values in [0, 1]: the histogram form has 256 terms per channel, torch's pairwise sum
    log2(N) levels, so each is within 1e-13 of the exact value; the bound is relative 1e-12."""
    images = _bytes()
    mean, std = B.channel_moments(images)
    x = images.float().div(255).unsqueeze(0)
    mu = x.double().mean(dim=(0, 1, 2, 3))
    sigma = x.double().std(dim=(0, 1, 2, 3), unbiased=False)
    assert mean.dtype == std.dtype == torch.float64 and mean.shape == std.shape == (3,)
    rel = max(float(((mean - mu) / mu).abs().max()), float(((std - sigma) / sigma).abs().max()))
    print(f"channel_moments: largest relative difference {rel:.3e}, bound 1e-12")
    assert rel <= 1e-12
    one = torch.full((4, 2, 2, 1), 51, dtype=torch.uint8)             # a constant channel: 0.2, no spread
    m1, s1 = B.channel_moments(one)
    assert float(m1) == pytest.approx(0.2, rel=1e-7) and float(s1) <= 1e-9
    with pytest.raises(TypeError):
        B.channel_moments(images.float())


def test_from_colour_errors_come_before_the_device():
    images = torch.zeros(37, 5, 5, 3, dtype=torch.uint8)
    labels = torch.zeros(37, dtype=torch.int64)
    kw = dict(dtype=torch.float32, seed=1, nu=NU)
    with pytest.raises(TypeError):
        B.DeviceBatches.from_colour(images.float(), labels, 8, **kw)
    with pytest.raises(TypeError):
        B.DeviceBatches.from_colour(images[..., 0], labels, 8, **kw)                    # (n, H, W): the grey-scale form
    with pytest.raises(TypeError):
        B.DeviceBatches.from_colour(images, labels, 8, dtype=torch.float16, seed=1, nu=NU)
    with pytest.raises(NotImplementedError):
        B.DeviceBatches.from_colour(torch.zeros(37, 5, 5, 5, dtype=torch.uint8), labels, 8, dtype=torch.float32, seed=1,
                                    nu=1.0)
    with pytest.raises(NotImplementedError):
        B.DeviceBatches.from_colour(torch.zeros(37, 5, 5, 4, dtype=torch.uint8), labels, 8, dtype=torch.float32, seed=1,
                                    nu=1.0, constant_channel=1.0)
    with pytest.raises(ValueError):
        B.DeviceBatches.from_colour(images, labels, 38, **kw)                            # S = 0
    with pytest.raises(ValueError):
        B.DeviceBatches.from_colour(images, labels, 9, rank=0, world=2, **kw)            # 9 does not divide over 2 ranks
    with pytest.raises(ValueError):
        B.DeviceBatches.from_colour(images, labels[:5], 8, **kw)
    with pytest.raises(ValueError):
        B.DeviceBatches.from_colour(images, labels, 8, shuffle=True, drop_last=False, **kw)
    with pytest.raises(ValueError):
        B.DeviceBatches.from_colour(images, labels, 8, dtype=torch.float32, seed=1 << 64, nu=NU)


@pytest.mark.skipif(torch.cuda.is_available(), reason="with a GPU the source is built (tests/test_gpu_colour_source.py)")
def test_a_colour_source_without_a_gpu_raises():
    images = torch.zeros(37, 5, 5, 3, dtype=torch.uint8)
    labels = torch.zeros(37, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        B.DeviceBatches.from_colour(images, labels, 8, dtype=torch.float32, seed=1, nu=NU)
