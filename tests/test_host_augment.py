"""Host-side checks of the on-device augmentation (no GPU needed): the parameters of a slot against known answers, their
range and coverage, `augment_bytes` against pad / crop / flip in torch, the two entry points declared, exported and bound,
their argument checks and the order of those checks, the kernel names, and the Python errors, all before any device."""
import os
import re
import subprocess
from collections import Counter

import pytest
import torch
import torch.nn.functional as F

from dctn_amd import _lib
from dctn_amd import batches as B
from dctn_amd.dropout import philox4x32_10

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dctn_batch_draw_aug", "dctn_batch_draw_cols_aug")
SEED = 0x1234567890ABCDEF


# ------------------------------------------------------------------ the parameters
def test_known_answer():
    words = philox4x32_10((16, 0, 1, 0x41554731), (SEED & 0xFFFFFFFF, SEED >> 32))
    assert B.AUG_TAG == 0x41554731 and B.AUG_TAG != B.TAG and B.AUG_TAG >= 8
    assert tuple(words) == (0xB6CF4FEC, 0xCD5954F5, 0x01740A7B, 0x8F03CC94)
    # m = 1: (w * 3) >> 32 is 2 for both words (they are above 2/3 of 2^32), minus 1; the top bit of w[2] is clear
    assert (0xB6CF4FEC * 3 >> 32, 0xCD5954F5 * 3 >> 32, 0x01740A7B >> 31) == (2, 2, 0)
    assert B.augment_params(SEED, 1, 16, 1, True) == (1, 1, 0)


def test_draw_6_of_37_samples_in_batches_of_8():
    """Draw 6 with S = 4: epoch 1, positions 16 .. 23."""
    got = [B.augment_params(SEED, 1, g, 2, True) for g in range(16, 24)]
    assert got == [(1, 2, 0), (0, 2, 1), (0, 0, 0), (-2, -2, 1), (0, 2, 1), (1, -2, 0), (1, -2, 0), (-2, -2, 0)]
    assert [B.augment_params(SEED, 1, g, 2, False) for g in range(16, 24)] == [(dy, dx, 0) for dy, dx, _ in got]
    m4 = [B.augment_params(SEED, 1, g, 4, True) for g in range(16, 24)]
    assert m4[3][0] == -4 and m4[7][0] == -4
    # the epoch is part of the counter: the same positions get other parameters in epoch 0
    assert [B.augment_params(SEED, 0, g, 2, True) for g in range(16, 24)] != got


def test_range_and_coverage():
    seen = Counter(B.augment_params(SEED, 0, g, 2, True) for g in range(4096))
    assert set(seen) == {(dy, dx, f) for dy in range(-2, 3) for dx in range(-2, 3) for f in (0, 1)} and len(seen) == 50
    seen = Counter(B.augment_params(SEED, 3, g, 4, False) for g in range(8192))
    assert set(seen) == {(dy, dx, 0) for dy in range(-4, 5) for dx in range(-4, 5)} and len(seen) == 81
    assert all(B.augment_params(SEED, 2, g, 0, False) == (0, 0, 0) for g in range(256))
    assert {B.augment_params(SEED, 2, g, 0, True)[:2] for g in range(256)} == {(0, 0)}
    big = [B.augment_params(SEED, 5, g, B.AUG_MAX_SHIFT, True) for g in range(512)]
    assert all(-B.AUG_MAX_SHIFT <= v <= B.AUG_MAX_SHIFT for dy, dx, _ in big for v in (dy, dx))


# ------------------------------------------------------------------ augment_bytes against pad, crop, flip
def _pad_crop_flip(images, params, fill):
    """An independent formulation: torch's constant pad by m on every side per channel, an H x Wd window at
    (m + dy, m + dx), torch's flip."""
    grey = images.ndim == 3
    full = images.unsqueeze(-1) if grey else images
    count, H, Wd, C = full.shape
    fills = [fill] * C if isinstance(fill, int) else list(fill)
    m = max([1] + [max(abs(dy), abs(dx)) for dy, dx, _ in params])
    out = []
    for i, (dy, dx, flip) in enumerate(params):
        chans = [F.pad(full[i, :, :, c].int(), (m, m, m, m), value=fills[c])[m + dy : m + dy + H, m + dx : m + dx + Wd]
                 for c in range(C)]
        img = torch.stack(chans, dim=-1).to(torch.uint8)
        out.append(torch.flip(img, dims=(1,)) if flip else img)
    out = torch.stack(out)
    return out[..., 0] if grey else out


PARAMS = [(0, 0, 0), (0, 0, 1), (1, 2, 0), (-1, -2, 1), (2, -3, 1), (-4, 0, 0), (0, 6, 1), (5, 0, 0), (0, -7, 0), (9, 9, 1),
          (-6, 1, 1), (4, 3, 0), (-4, -6, 1), (3, -3, 0)]


def test_augment_bytes_is_pad_crop_flip():
    g = torch.Generator().manual_seed(0)
    grey = torch.randint(0, 256, (len(PARAMS), 5, 7), dtype=torch.uint8, generator=g)
    colour = torch.randint(0, 256, (len(PARAMS), 6, 4, 3), dtype=torch.uint8, generator=g)
    for fill in (0, 77):
        assert torch.equal(B.augment_bytes(grey, PARAMS, fill), _pad_crop_flip(grey, PARAMS, fill))
    for fill in (0, 200, (3, 130, 255)):
        got = B.augment_bytes(colour, PARAMS, fill)
        assert got.shape == colour.shape and got.dtype == torch.uint8
        assert torch.equal(got, _pad_crop_flip(colour, PARAMS, fill))
    # a sample shifted out entirely is the fill alone, channel by channel
    out = B.augment_bytes(colour[:1], [(6, 0, 1)], (3, 130, 255))
    assert torch.equal(out[0], torch.tensor([3, 130, 255], dtype=torch.uint8).expand(6, 4, 3))
    # the definition, element by element
    dy, dx, flip = PARAMS[3]
    got = B.augment_bytes(grey, PARAMS, 9)[3]
    for h in range(5):
        for w in range(7):
            hs, ws = h + dy, (6 - w if flip else w) + dx
            assert int(got[h, w]) == (int(grey[3, hs, ws]) if 0 <= hs < 5 and 0 <= ws < 7 else 9)
    with pytest.raises(ValueError):
        B.augment_bytes(grey, PARAMS[:3], 0)
    with pytest.raises(ValueError):
        B.augment_bytes(colour, PARAMS, (1, 2))
    with pytest.raises(ValueError):
        B.augment_bytes(grey.float(), PARAMS, 0)


# ------------------------------------------------------------------ the bindings
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
    assert re.search(r"DCTN_AUG_HFLIP\s*=\s*(\d+)", header).group(1) == str(_lib.AUG_HFLIP)
    assert int(re.search(r"#define\s+DCTN_AUG_TAG\s+(0x[0-9A-Fa-f]+)", header).group(1), 16) == B.AUG_TAG
    assert _lib.lib().dctn_version() >= 507
    # one argument more than the grey call: the source channels
    grey, cols = _lib.SIGNATURES["dctn_batch_draw_aug"][1], _lib.SIGNATURES["dctn_batch_draw_cols_aug"][1]
    assert len(cols) == len(grey) + 1 == 21


def test_entry_points_validate_their_arguments_without_a_device():
    L = _lib
    IDENTITY, PAD = L.BATCH_IDENTITY_ORDER, L.BATCH_PAD_TAIL
    P = 64   # any non-null address: nothing is launched

    def grey(src=P, table=P, labels=P, x=P, y=P, idx=P, state=P, n=37, G=8, Bl=8, off=0, H=5, Wd=7, W=2, flags=0,
             dtype=L.F32, m=2, aug=L.AUG_HFLIP, fill=0):
        return L.lib().dctn_batch_draw_aug(src, table, labels, x, y, idx, state, n, G, Bl, off, H, Wd, W, flags, dtype, m,
                                           aug, fill, None)

    def cols(src=P, table=P, labels=P, x=P, y=P, idx=P, state=P, n=37, G=8, Bl=8, off=0, H=5, Wd=7, C=3, W=4, flags=0,
             dtype=L.F32, m=2, aug=L.AUG_HFLIP, fill=0):
        return L.lib().dctn_batch_draw_cols_aug(src, table, labels, x, y, idx, state, n, G, Bl, off, H, Wd, C, W, flags,
                                                dtype, m, aug, fill, None)

    for d in (grey, cols):
        for name in ("src", "table", "labels", "x", "y", "idx", "state"):
            assert d(**{name: None}) == L.ERR_NULL, name
        assert d(n=0) == L.ERR_BAD_SHAPE and d(n=1 << 31) == L.ERR_BAD_SHAPE
        assert d(n=7, G=8) == L.ERR_BAD_SHAPE and d(G=0, Bl=0) == L.ERR_BAD_SHAPE and d(Bl=0) == L.ERR_BAD_SHAPE
        assert d(Bl=4, off=5) == L.ERR_BAD_SHAPE and d(Bl=4, off=-1) == L.ERR_BAD_SHAPE
        assert d(H=0) == L.ERR_BAD_SHAPE and d(Wd=0) == L.ERR_BAD_SHAPE and d(H=-3) == L.ERR_BAD_SHAPE
        assert d(H=1 << 31) == L.ERR_BAD_SHAPE and d(Wd=1 << 31) == L.ERR_BAD_SHAPE
        assert d(H=1 << 16, Wd=1 << 15) == L.ERR_BAD_SHAPE                   # H * Wd = 2^31
        assert d(W=0) == L.ERR_BAD_SHAPE
        # the flags: the identity order only; an evaluation pass is not augmented
        assert d(flags=PAD) == L.ERR_BAD_SHAPE and d(flags=IDENTITY | PAD) == L.ERR_BAD_SHAPE
        assert d(flags=4) == L.ERR_BAD_SHAPE and d(flags=IDENTITY | 8) == L.ERR_BAD_SHAPE
        # the augmentation's own arguments
        assert d(m=-1) == L.ERR_BAD_SHAPE and d(m=1 << 15) == L.ERR_BAD_SHAPE
        assert d(aug=2) == L.ERR_BAD_SHAPE and d(aug=L.AUG_HFLIP | 4) == L.ERR_BAD_SHAPE
        assert d(dtype=7) == L.ERR_BAD_DTYPE and d(dtype=-1) == L.ERR_BAD_DTYPE
        assert d(W=5) == L.ERR_UNSUPPORTED
        # the order of the checks: null, shape, dtype, unsupported
        assert d(src=None, n=0, dtype=7, W=5) == L.ERR_NULL
        assert d(n=0, dtype=7, W=5) == L.ERR_BAD_SHAPE and d(m=-1, dtype=7, W=5) == L.ERR_BAD_SHAPE
        assert d(flags=PAD, dtype=7, W=5) == L.ERR_BAD_SHAPE and d(aug=2, dtype=7, W=5) == L.ERR_BAD_SHAPE
        assert d(dtype=7, W=5) == L.ERR_BAD_DTYPE and d(dtype=7, H=128, Wd=128) == L.ERR_BAD_DTYPE
    # fill bits above the source channels
    assert grey(fill=0x100) == L.ERR_BAD_SHAPE and grey(fill=0x80000000) == L.ERR_BAD_SHAPE
    assert cols(fill=0x01000000) == L.ERR_BAD_SHAPE and cols(C=1, W=2, fill=0xFF00) == L.ERR_BAD_SHAPE
    assert cols(fill=0x01000000, dtype=7) == L.ERR_BAD_SHAPE
    # the widths of the colour form
    assert cols(C=0, W=1) == L.ERR_BAD_SHAPE and cols(C=-1, W=1) == L.ERR_BAD_SHAPE
    assert cols(C=5, W=5) == L.ERR_UNSUPPORTED and cols(C=3, W=2) == L.ERR_UNSUPPORTED
    assert cols(C=2, W=4) == L.ERR_UNSUPPORTED and cols(C=4, W=5) == L.ERR_UNSUPPORTED
    # the sample-size limit: 13 KiB a sample; 64 x 64 x 3 is inside it (its other arguments are wrong on purpose: no launch)
    assert grey(H=128, Wd=128) == L.ERR_UNSUPPORTED and cols(H=128, Wd=128) == L.ERR_UNSUPPORTED
    assert grey(H=1, Wd=B.AUG_MAX_SAMPLE_BYTES + 1) == L.ERR_UNSUPPORTED
    assert cols(H=67, Wd=67) == L.ERR_UNSUPPORTED                            # 13 467 bytes
    assert cols(H=64, Wd=64, dtype=7) == L.ERR_BAD_DTYPE and cols(H=64, Wd=64, W=5) == L.ERR_UNSUPPORTED
    assert cols(H=64, Wd=64, C=5, W=5) == L.ERR_UNSUPPORTED


def test_kernel_names_come_from_a_table():
    """tests/test_host_buffer_contract.py asks for a GUARDED entry for every LITERAL name in a dctn_set_last_kernel call;
    the augmented draws report theirs through a table, and tests/test_gpu_augment.py holds them to the buffer contract."""
    src = open(os.path.join(ROOT, "dctn_amd", "csrc", "augment_source.hip")).read()
    assert "dctn_set_last_kernel" not in src
    call = open(os.path.join(ROOT, "dctn_amd", "csrc", "batch_call.hip")).read()   # the one table of all batch kernels
    calls = re.findall(r"dctn_set_last_kernel\((.*?)\);", call, re.S)
    assert len(calls) == 1 and '"' not in calls[0] and "BATCH_KERNEL_NAMES[" in calls[0]
    names = set(re.findall(r'"(aug_[a-z0-9_]+)"', call))
    assert names == {f"aug_draw_{kind}_{dt}" for kind in ("u8", "cols") for dt in ("f32", "f64", "bf16")}
    # the order has one definition: the shared header, not restated
    assert '#include "draw_order.h"' in src and "perm_once(unsigned" not in src and "struct BatchState" not in src
    assert "struct BatchHead" not in src and "struct BatchGroup" not in src
    make = open(os.path.join(ROOT, "dctn_amd", "csrc", "Makefile")).read()
    assert "augment_source.hip" in make and re.search(r"augment_source\.o[^\n]*:\s*draw_order\.h", make)


# ------------------------------------------------------------------ the Python errors
def test_augment_validates_on_construction():
    a = B.Augment()
    assert (a.max_shift, a.hflip, a.fill, a.flags) == (0, False, 0, 0)
    a = B.Augment(4, True, (1, 2, 3))
    assert a.flags == _lib.AUG_HFLIP and a.packed_fill(3) == 0x030201 and a.fill_bytes(3) == (1, 2, 3)
    assert B.Augment(fill=200).packed_fill(3) == 0xC8C8C8 and B.Augment(fill=200).packed_fill(1) == 200
    for bad in (dict(max_shift=-1), dict(max_shift=1 << 15), dict(max_shift=1.5), dict(max_shift=True), dict(hflip=1),
                dict(fill=256), dict(fill=-1), dict(fill=(1, 2, 300)), dict(fill=()), dict(fill=(1, 2, 3, 4, 5)),
                dict(fill=0.5)):
        with pytest.raises(ValueError):
            B.Augment(**bad)
    with pytest.raises(ValueError):
        B.Augment(fill=(1, 2)).packed_fill(3)


def test_constructor_errors_come_before_the_device():
    labels = torch.zeros(37, dtype=torch.int64)
    grey, colour = torch.zeros(37, 5, 7, dtype=torch.uint8), torch.zeros(37, 5, 7, 3, dtype=torch.uint8)
    aug = B.Augment(2, True)
    gkw, ckw = dict(dtype=torch.float32, seed=1), dict(dtype=torch.float32, seed=1, nu=1.0)
    with pytest.raises(TypeError):
        B.DeviceBatches(grey, labels, 8, augment=(2, True), **gkw)
    with pytest.raises(TypeError):
        B.DeviceBatches.from_colour(colour, labels, 8, augment="shift", **ckw)
    with pytest.raises(ValueError):   # evaluation is not augmented
        B.DeviceBatches(grey, labels, 8, shuffle=False, drop_last=False, augment=aug, **gkw)
    with pytest.raises(ValueError):
        B.DeviceBatches.from_colour(colour, labels, 8, shuffle=False, drop_last=False, augment=aug, **ckw)
    with pytest.raises(ValueError):   # one fill byte per SOURCE channel
        B.DeviceBatches.from_colour(colour, labels, 8, augment=B.Augment(fill=(1, 2)), **ckw)
    with pytest.raises(ValueError):
        B.DeviceBatches(grey, labels, 8, augment=B.Augment(fill=(1, 2, 3)), **gkw)
    with pytest.raises(ValueError):
        B.DeviceBatches.from_colour(colour, labels, 8, constant_channel=1.0, augment=B.Augment(fill=(1, 2, 3, 4)), **ckw)
    with pytest.raises(NotImplementedError):   # more than a wave's LDS region
        B.DeviceBatches(torch.zeros(9, 128, 128, dtype=torch.uint8), labels[:9], 8, augment=aug, **gkw)
    with pytest.raises(NotImplementedError):
        B.DeviceBatches.from_colour(torch.zeros(9, 67, 67, 3, dtype=torch.uint8), labels[:9], 8, augment=aug, **ckw)
    with pytest.raises(ValueError):   # the unaugmented constructors' own errors still come first
        B.DeviceBatches(grey, labels, 38, augment=aug, **gkw)
    with pytest.raises(TypeError):    # from_features has no height or width: no such argument
        B.DeviceBatches.from_features(torch.zeros(1, 37, 5, 7, 2), labels, 8, seed=1, augment=aug)


@pytest.mark.skipif(torch.cuda.is_available(), reason="with a GPU the source is built (tests/test_gpu_augment.py)")
def test_an_augmented_source_without_a_gpu_raises():
    labels = torch.zeros(37, dtype=torch.int64)
    aug = B.Augment(2, True, 7)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        B.DeviceBatches(torch.zeros(37, 5, 7, dtype=torch.uint8), labels, 8, dtype=torch.float32, seed=1, augment=aug)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        B.DeviceBatches.from_colour(torch.zeros(37, 64, 64, 3, dtype=torch.uint8), labels, 8, dtype=torch.float32, seed=1,
                                    nu=1.0, shuffle=False, augment=aug)
