"""Exact inputs for bit-exact parity tests ("Exact-input tests").

Every operand lies on a power-of-two grid: pixels are one-hot (rarely two-hot) Q-vectors of 1 or 2^-1, cores, head
weights and biases small integers, incoming gradients small integers.  Every product and every partial sum that a kernel
forms is then an integer number of grid units, bounded by the same contraction over absolute values ("mag").  While mag
fits the accumulator (2^24 units for float32, 2^53 for float64) and every intermediate a family rounds to bf16 fits 2^8
units, the kernel's result does not depend on summation order, tiling, split count or atomics: it equals the float64
oracle after the one final rounding to the storage dtype.  A dropped, duplicated or misplaced window, sample, tile or
column is then a mismatch at any batch size.

Host-side only (no GPU): generators, budget and non-degeneracy checks, `assert_exact`, and a closed form of the EPS
oracle for one-hot pixels that the full-size tests use (tests/test_host_exact_inputs.py ties it to the oracle)."""
from __future__ import annotations

import math
from typing import Dict, Optional, Sequence, Tuple

import torch

from oracle import ref_cpu as R

F32_UNITS = 2 ** 24     # float32 accumulators: exact while every partial sum is at most this many grid units
F64_UNITS = 2 ** 53     # float64: exact below this
BF16_UNITS = 2 ** 8     # an intermediate rounded to bf16: exact while its own bound is at most this many units
SMALLEST = 2.0 ** -60   # every nonzero magnitude stays far above the subnormals

EPS_LAYOUT = ("sample", "row", "col", "o")
CORE_LAYOUT = ("core row", "o")


# ------------------------------------------------------------------------------------------------ generators
def _gen(seed: int) -> torch.Generator:
    return torch.Generator().manual_seed(int(seed) % (2 ** 63))


def small_ints(shape, seed: int, vmax: int, nonzero: bool = False) -> torch.Tensor:
    """float64 integers in [-vmax, vmax]; with ``nonzero`` none is zero."""
    g = _gen(seed)
    if not nonzero:
        return torch.randint(-vmax, vmax + 1, tuple(shape), generator=g).double()
    mag = torch.randint(1, vmax + 1, tuple(shape), generator=g)
    sign = torch.randint(0, 2, tuple(shape), generator=g) * 2 - 1
    return (mag * sign).double()


def pixels(C: int, B: int, H: int, W: int, Q: int, seed: int, two_hot: bool = True, halves: bool = False) -> torch.Tensor:
    """x (C, B, H, W, Q), float64.  Every pixel is a one-hot Q-vector (a 1 at a random q).  With ``two_hot``, pixels on
    the lattice h % 4 == 0, w % 4 == 0 carry, with probability 1/2, a second 1 (Q = 2: the vector (1, 1)); a window of
    up to 4 x 4 pixels holds at most one of them, so a Khatri-Rao row of any window has at most two ones per channel.
    With ``halves`` (the float32 / float64 paths) a quarter of the pixels hold 2^-1 instead of 1."""
    g = _gen(seed)
    hot = torch.randint(0, Q, (C, B, H, W), generator=g)
    x = torch.nn.functional.one_hot(hot, Q).double()
    if two_hot and Q > 1:
        lattice = torch.zeros(H, W, dtype=torch.bool)
        lattice[::4, ::4] = True
        pick = (torch.rand(C, B, H, W, generator=g) < 0.5) & lattice
        other = (hot + torch.randint(1, Q, (C, B, H, W), generator=g)) % Q
        x = x + torch.nn.functional.one_hot(other, Q).double() * pick.unsqueeze(-1)
    if halves:
        x = x * torch.where(torch.rand(C, B, H, W, 1, generator=g) < 0.25, 0.5, 1.0).double()
    return x


def one_hot_pixels(C: int, B: int, H: int, W: int, Q: int, seed: int) -> torch.Tensor:
    """Strictly one-hot pixels of value 1: the input of the closed-form oracle (`eps_onehot_forward`)."""
    return pixels(C, B, H, W, Q, seed, two_hot=False)


def eps_core(Q: int, N: int, O: int, seed: int, vmax: int = 8) -> torch.Tensor:
    return small_ints((Q,) * N + (O,), seed, vmax)


def head_operands(cout: int, F: int, B: int, seed: int):
    """(W, bias, dLogits) of a linear head, integers: bias in [-8, 8], dLogits nonzero in [-2, 2] with column 0 odd,
    W row 0 odd in [-3, 3], the other rows even in [-2, 2].  dFeat = dLogits . W is then odd - never zero - for every
    sample and feature, so every window of the layer below adds to dCore; |dFeat| <= 3 + 4 (Cout - 1)."""
    w = small_ints((cout, F), seed, 1) * 2
    w[0] = small_ints((F,), seed + 3, 1, nonzero=True) * (1 + 2 * (small_ints((F,), seed + 4, 1) != 0).double())
    g = small_ints((B, cout), seed + 2, 2, nonzero=True)
    g[:, 0] = small_ints((B,), seed + 5, 1, nonzero=True)
    return w, small_ints((cout,), seed + 1, 8), g


def sbs_cores(shapes: Sequence[Tuple[int, ...]], seed: int, p2: float = 0.125) -> list:
    """ConvSBS cores (o, l, r, q, ..., q), float64.  Every (o, q...) slice is an l x r matrix in which every row and
    every column holds a nonzero (a random map of rows to columns, onto the larger side), values +-1 and, with
    probability ``p2``, +-2; a one-row or one-column slice (the open ends) is dense.  Chain states then stay sparse and
    small whatever the bond, and no window's chain dies: every window contributes to every core's gradient."""
    g = _gen(seed)
    out = []
    for shape in shapes:
        o, l, r = shape[:3]
        nq = math.prod(shape[3:])
        core = torch.zeros(o, nq, l, r, dtype=torch.float64)
        for a in range(o):
            for q in range(nq):
                if l == 1 or r == 1:
                    mask = torch.ones(l, r, dtype=torch.bool)
                else:
                    mask = torch.zeros(l, r, dtype=torch.bool)
                    big, small = max(l, r), min(l, r)
                    onto = torch.cat([torch.randperm(small, generator=g),
                                      torch.randint(0, small, (big - small,), generator=g)])[torch.randperm(big, generator=g)]
                    for i in range(big):
                        if l >= r:
                            mask[i, onto[i]] = True
                        else:
                            mask[onto[i], i] = True
                vals = torch.where(torch.rand(l, r, generator=g) < p2, 2.0, 1.0).double()
                vals = vals * (torch.randint(0, 2, (l, r), generator=g) * 2 - 1)
                core[a, q] = vals * mask
        out.append(core.permute(0, 2, 3, 1).reshape(shape).contiguous())
    return out


# ------------------------------------------------------------------------------------------------ grid and budgets
def grid_exponent(t: torch.Tensor) -> int:
    """Smallest k >= 0 with t * 2^k integral everywhere (t on a power-of-two grid no finer than 2^-24: every double is
    dyadic, so a finer "grid" means the operand is not an exact input)."""
    t = t.double()
    nz = t[t != 0].abs()
    assert nz.numel() == 0 or float(nz.min()) >= SMALLEST, "a nonzero magnitude below 2^-60"
    for k in range(25):
        s = t * 2.0 ** k
        if torch.equal(s, s.round()):
            return k
    raise AssertionError("operand is not on a power-of-two grid")


def to_grid(t: torch.Tensor) -> torch.Tensor:
    """t scaled to integer grid units (exact: a power-of-two scale)."""
    return t.double() * 2.0 ** grid_exponent(t)


def eps_mags(core: torch.Tensor, x: torch.Tensor, dy: torch.Tensor) -> Dict[str, torch.Tensor]:
    """Bounds in grid units of every partial sum of the forward, dCore and dX: the oracle on the absolute values of
    the integer-scaled operands."""
    c, xx, g = to_grid(core).abs(), to_grid(x).abs(), to_grid(dy).abs()
    fwd = R.eps_4step(c, xx)
    dcore, dx = R.grads(R.eps_4step, [c, xx], g)
    return {"forward": fwd, "dcore": dcore, "dx": dx}


def khatri_rao_halves(x: torch.Tensor, K: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """The two Khatri-Rao halves (B, H', W', Q^n0) and (B, H', W', Q^n1) of the two-halves / register families."""
    views = R.align(x, K)
    n0 = math.ceil(len(views) / 2)
    return R._khatri_rao(views[:n0]), R._khatri_rao(views[n0:]) if len(views) > n0 else None


def eps_bf16_intermediates(core: torch.Tensor, x: torch.Tensor, dy: Optional[torch.Tensor], family: str) -> Dict[str, float]:
    """Largest magnitude, in grid units, of every intermediate that an EPS family rounds to bf16 (operands aside):
      q2reg  (eps_mfma.hip)  : P0 / P1 rows (built in f32, v_cvt_pk_bf16_f32); backward Z = P1 . dY
      halves (eps_halves.hip): "scaled" operands = a half-row times one dY scalar (scale8); Z' = core . half0 (zstore)
    The bf16 operands themselves (x, core, dY) are exact by construction.  The bf16 paths take pixels of 0 / 1 (one
    grid for every factor, so grid units measure the bits a value needs)."""
    assert bool(((x == 0) | (x == 1)).all()), "bf16 paths: pixels of 0 and 1 only"
    K = math.isqrt((core.ndim - 1) // x.shape[0])
    h0, h1 = khatri_rao_halves(to_grid(x).abs(), K)
    out = {"P0": float(h0.max()), "P1": float(h1.max()) if h1 is not None else 0.0}
    g = to_grid(dy).abs() if dy is not None else None
    if family == "q2reg" and g is not None and h1 is not None:
        out["Z = P1 dY"] = float(h1.max()) * float(g.max())
    if family == "halves":
        if g is not None:
            out["half-row x dY"] = max(float(h0.max()), out["P1"]) * float(g.max())
        if h1 is not None:
            z = torch.tensordot(h0, to_grid(core).abs().reshape(h0.shape[-1], -1), dims=1)
            out["Z' = core half0"] = float(z.max())
    return out


def check_budget(mags: Dict[str, torch.Tensor], accumulator: torch.dtype, bf16: Optional[Dict[str, float]] = None) -> Dict[str, float]:
    """Asserts every mag fits the accumulator and every bf16 intermediate fits 2^8 units; returns the largest of each
    (the headroom report)."""
    limit = F64_UNITS - 1 if accumulator == torch.float64 else F32_UNITS
    report = {}
    for name, m in mags.items():
        top = float(m.max()) if m.numel() else 0.0
        assert top <= limit, f"budget: {name} reaches {top:.0f} grid units > {limit}"
        report[name] = top
    for name, top in (bf16 or {}).items():
        assert top <= BF16_UNITS, f"bf16 budget: {name} reaches {top:.0f} grid units > 2^8"
        report["bf16 " + name] = top
    return report


# ------------------------------------------------------------------------------------------------ non-degeneracy
def eps_window_weights(x: torch.Tensor, K: int, dy: torch.Tensor) -> torch.Tensor:
    """Per window (B, H', W'): the absolute size of its term in dCore, prod_n sum|x_n| * sum_o |dY|."""
    w = None
    for v in R.align(x.double().abs(), K):
        s = v.sum(-1)
        w = s if w is None else w * s
    return w * dy.double().abs().sum(-1)


def assert_every_window_counts(weights: torch.Tensor, what: str = "") -> None:
    dead = (weights == 0).nonzero()
    assert dead.shape[0] == 0, f"{what}: {dead.shape[0]} windows add nothing to dCore, first {dead[:4].tolist()}"


def assert_nonzero(**tensors: torch.Tensor) -> None:
    for name, t in tensors.items():
        assert bool((t != 0).any()), f"expected {name} is all zero"


# ------------------------------------------------------------------------------------------------ comparison
def expected(want64: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """The one final rounding: float64 -> float32 is exact within budget, then RNE to the storage dtype."""
    want64 = want64.detach().cpu().double()
    return want64 if dtype == torch.float64 else want64.float().to(dtype)


def assert_exact(got: torch.Tensor, want64: torch.Tensor, dtype: torch.dtype, layout: Sequence[str] = (), what: str = "") -> None:
    """torch.equal(got, want64 rounded once to dtype).  On mismatch: the count of differing elements, the first few
    indices decoded along ``layout`` (e.g. (sample, row, col, o) or (core row, o)) and the largest difference in grid
    units of the expected value."""
    want = expected(want64, dtype)
    got = got.detach().cpu()
    assert got.dtype == dtype, f"{what}: got {got.dtype}, want {dtype}"
    assert tuple(got.shape) == tuple(want.shape), f"{what}: shape {tuple(got.shape)} != {tuple(want.shape)}"
    if torch.equal(got, want):
        return
    g, w = got.double(), want.double()
    bad = (g != w) & ~(g.isnan() & w.isnan())
    idx = bad.nonzero()
    k = grid_exponent(want64.detach().cpu().double())
    diff = float((g - w).abs()[bad].max()) * 2.0 ** k
    lines = []
    for row in idx[:6].tolist():
        if len(layout) == want.ndim:
            pos = ", ".join(f"{n}={i}" for n, i in zip(layout, row))
        else:
            pos = ", ".join(map(str, row))
        lines.append(f"({pos}): got {float(g[tuple(row)])!r} want {float(w[tuple(row)])!r}")
    raise AssertionError(f"{what}: {idx.shape[0]} of {want.numel()} elements differ, largest by {diff:.6g} grid units; "
                         + "; ".join(lines))


def decode_core_layout(core_shape: Sequence[int]) -> Tuple[int, ...]:
    """A core gradient viewed as (core row, o): the shape to pass `assert_exact` with CORE_LAYOUT."""
    return (math.prod(core_shape[:-1]), core_shape[-1])


# ------------------------------------------------------------------------------------------------ closed form (one-hot x)
def window_rows(x: torch.Tensor, K: int) -> torch.Tensor:
    """For strictly one-hot pixels of value 1: the core row every window selects, (B, H', W') int64.  Factor
    n = position * C + channel, position row-major, the first factor most significant (R.eps_definition_numpy)."""
    C, B, H, W, Q = x.shape
    assert bool(((x == 0) | (x == 1)).all()) and bool((x.sum(-1) == 1).all()), "closed form: one-hot pixels only"
    digit = x.argmax(-1)   # (C, B, H, W)
    Ho, Wo = H - K + 1, W - K + 1
    rows = torch.zeros(B, Ho, Wo, dtype=torch.int64)
    for dh in range(K):
        for dw in range(K):
            for ch in range(C):
                rows = rows * Q + digit[ch, :, dh : dh + Ho, dw : dw + Wo]
    return rows


def eps_onehot_forward(core: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
    """eps_4step for one-hot x: a gather of core rows, (B, H', W', O)."""
    C = x.shape[0]
    K = math.isqrt((core.ndim - 1) // C)
    O = core.shape[-1]
    return core.reshape(-1, O).double()[window_rows(x, K)]


def eps_onehot_dcore(core_shape: Sequence[int], x: torch.Tensor, dy: torch.Tensor) -> torch.Tensor:
    """dCore of eps_4step for one-hot x: an index_add of dY over the selected rows."""
    C = x.shape[0]
    K = math.isqrt((len(core_shape) - 1) // C)
    O = core_shape[-1]
    rows = window_rows(x, K).reshape(-1)
    out = torch.zeros(math.prod(core_shape[:-1]), O, dtype=torch.float64)
    out.index_add_(0, rows, dy.double().reshape(-1, O))
    return out.reshape(tuple(core_shape))


# ------------------------------------------------------------------------------------------------ ConvSBS
def _sbs_mats(cores: Sequence[torch.Tensor], positions, x: torch.Tensor):
    C = x.shape[0]
    views = R.align_with_positions(x, positions)
    mats = []
    for c, core in enumerate(cores):
        f = R._khatri_rao(views[c * C : (c + 1) * C])
        o, l, r = core.shape[:3]
        mats.append(torch.einsum("bhwq,olrq->bhwolr", f, core.reshape(o, l, r, -1)))
    return mats


def sbs_state_bound(cores: Sequence[torch.Tensor], positions, x: torch.Tensor, chunk: int = 8) -> float:
    """Largest entry, in grid units, of every prefix and suffix chain state of every window: the chain of
    R.convsbs_forward over absolute values, both directions (batch slices of ``chunk`` images)."""
    cs = [to_grid(c).abs() for c in cores]
    xg = to_grid(x).abs()
    top = 0.0
    for b0 in range(0, x.shape[1], chunk):
        mats = _sbs_mats(cs, positions, xg[:, b0 : b0 + chunk])
        acc = mats[0]
        top = max(top, float(acc.max()))
        for m in mats[1:]:
            acc = torch.einsum("bhwalr,bhwors->bhwaols", acc, m)
            acc = acc.reshape(*acc.shape[:3], -1, acc.shape[-2], acc.shape[-1])
            top = max(top, float(acc.max()))
        acc = mats[-1]
        for m in reversed(mats[:-1]):
            acc = torch.einsum("bhwolr,bhwars->bhwoals", m, acc)
            acc = acc.reshape(*acc.shape[:3], -1, acc.shape[-2], acc.shape[-1])
            top = max(top, float(acc.max()))
    return top


def sbs_mags(cores: Sequence[torch.Tensor], positions, x: torch.Tensor, dy: torch.Tensor) -> Dict[str, torch.Tensor]:
    """Grid-unit bounds of the ConvSBS forward, dX, every dCore and every chain state."""
    cs = [to_grid(c).abs() for c in cores]
    xg, g = to_grid(x).abs(), to_grid(dy).abs()
    pos = list(positions)
    fwd = R.convsbs_forward(cs, pos, xg)
    gr = R.grads(lambda xx, *cc: R.convsbs_forward(cc, pos, xx), [xg] + cs, g)
    mags = {"forward": fwd, "dx": gr[0], "states": torch.tensor([sbs_state_bound(cores, pos, x)])}
    for i, gc in enumerate(gr[1:]):
        mags[f"dcore{i}"] = gc
    return mags


def sbs_window_weights(cores: Sequence[torch.Tensor], positions, x: torch.Tensor, dy: torch.Tensor) -> torch.Tensor:
    """Per window: prod over the cores of sum |M_c| (the core contracted with its pixels) times sum |dY|.  The cores of
    `sbs_cores` hold a nonzero in every row and every column of every slice, so every product of them does too (over
    absolute values): a window whose matrices are all nonzero adds a nonzero term to every core's gradient, in open
    chains and rings alike."""
    w = dy.double().abs().sum(-1)
    for m in _sbs_mats([c.abs() for c in cores], list(positions), x.abs()):
        w = w * m.flatten(3).sum(-1)
    return w
