"""The drop-in boundary with CPU tensors (SURVEY 8b "dtype/device": f32 and f64 on CPU must be accepted).

The reference's own tests build CPU float64 tensors and call ``dctn.eps`` / ``dctn.conv_sbs`` directly
(/root/reference/tests/test_eps.py:9-61, tests/test_conversion_of_convsbs_to_eps.py:13-56,
tests/test_epses_composition.py:7-41).  Here their assertions are RESTATED (not copied) and run through the alias
package ``dctn`` exactly as a user of the reference would: CPU tensors in, CPU tensors out, gradients on the CPU
leaves — with the arithmetic on the MI355X (CPU tensors are staged to the device, `dctn_amd._lib.placement`; the
last-kernel name proves the HIP path ran).  Nothing here touches the oracle: the expected values are the
independent einsum definitions the reference's tests use.
"""
import functools
import itertools
import string

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _definition(core, factors):
    """sum over i_0..i_{N-1} of core[i_0, .., i_{N-1}, o] * prod_n factors[n][..., i_n]: one einsum, the formulation
    the reference's tests hand to opt_einsum ("01234567θ,b0,...,b7->bθ")."""
    n = len(factors)
    letters = string.ascii_lowercase[:n]
    batched = factors[0].ndim == 2
    lhs = ",".join(("z" + l) if batched else l for l in letters)
    return torch.einsum(f"{letters}y,{lhs}->{'zy' if batched else 'y'}", core, *factors)


def test_eps_single_pixel_output_cpu_f64():
    # restated from tests/test_eps.py:9-26: C=2, K=2 on a 2x2 image, factor index = position * C + channel
    import dctn.eps
    import dctn_amd

    x = torch.randn((2, 3, 2, 2, 2), dtype=torch.float64)
    core = torch.rand((2,) * 8 + (4,), dtype=torch.float64)
    got = dctn.eps.eps_one_by_one(core, x)
    assert got.device.type == "cpu" and got.dtype == torch.float64 and got.shape == (3, 1, 1, 4)
    assert dctn_amd.last_kernel().startswith("eps_fwd")   # the HIP library computed it
    factors = [x[ch, :, h, w] for h in range(2) for w in range(2) for ch in range(2)]
    assert torch.allclose(got.reshape(3, 4), _definition(core, factors))
    assert torch.allclose(dctn.eps.eps(core, x), got)


def test_eps_two_pixels_output_cpu_f64():
    # restated from tests/test_eps.py:29-61: K=3 on a 4x3 image -> two windows, one below the other
    import dctn.eps

    x = torch.randn((1, 1, 4, 3, 2), dtype=torch.float64)
    core = torch.rand((2,) * 9 + (4,), dtype=torch.float64)
    got = dctn.eps.eps_one_by_one(core, x)
    assert got.shape == (1, 2, 1, 4) and got.device.type == "cpu"
    for top in (0, 1):
        factors = [x[0, 0, top + dh, dw] for dh in range(3) for dw in range(3)]
        assert torch.allclose(got[0, top, 0], _definition(core, factors))


def test_cpu_gradients_arrive_on_the_cpu_leaves():
    import dctn.eps

    x = torch.randn((1, 2, 5, 5, 3), dtype=torch.float32, requires_grad=True)
    core = torch.randn((3,) * 4 + (5,), dtype=torch.float32, requires_grad=True)
    out = dctn.eps.eps(core, x)
    out.square().sum().backward()
    assert x.grad is not None and x.grad.device.type == "cpu" and core.grad.device.type == "cpu"
    factors = [x.detach()[0, :, h, w] for h in range(2) for w in range(2)]   # the top-left window of each sample
    assert torch.allclose(out.detach()[:, 0, 0], _definition(core.detach(), factors), rtol=1e-4, atol=1e-5)


def test_convsbs_equals_eps_for_all_orders_cpu_f64():
    # restated from tests/test_conversion_of_convsbs_to_eps.py:13-56: ring bonds (3,4,5,6), outs (1,3,2,4), every
    # order of the four cores of a 2x2 window; CPU float64 module and input, as the reference builds them
    from dctn.conv_sbs import ConvSBS
    from dctn.conv_sbs_spec import SBSSpecCore, SBSSpecString
    from dctn.eps import eps
    from dctn.pos2d import Pos2D
    import dctn_amd

    cores = (SBSSpecCore(Pos2D(0, 0), 1), SBSSpecCore(Pos2D(0, 1), 3), SBSSpecCore(Pos2D(1, 0), 2),
             SBSSpecCore(Pos2D(1, 1), 4))
    for order in itertools.permutations(cores):
        sbs = ConvSBS(SBSSpecString(order, (3, 4, 5, 6), 2, 2)).double()
        with torch.no_grad():
            dense = sbs.as_eps()
        assert dense.shape == (2,) * 8 + (24,)
        assert torch.all(dense == sbs.as_eps())
        x = torch.randn(2, 3, 4, 5, 2, dtype=torch.float64, requires_grad=True)
        y_sbs = sbs(x)
        assert y_sbs.device.type == "cpu" and dctn_amd.last_kernel().startswith("convsbs_fwd")
        seed = torch.randn_like(y_sbs)
        y_sbs.backward(seed)
        g_sbs = x.grad.clone()
        x.grad.zero_()
        y_eps = eps(dense, x)
        assert torch.allclose(y_eps, y_sbs)
        y_eps.backward(seed)
        assert torch.allclose(x.grad, g_sbs)


def test_model_on_cpu_runs_on_the_device():
    """EPSesPlusLinear built with device=cpu (what `EPS.__init__` / a CPU-side user gets): forward and backward
    are staged once per call; parameters' gradients land on the CPU parameters."""
    from dctn.eps_plus_linear import EPSesPlusLinear, UnitTheoreticalOutputStd

    torch.manual_seed(3)
    cpu_model = EPSesPlusLinear(((2, 3), (2, 4)), UnitTheoreticalOutputStd(), 1.0, torch.device("cpu"), torch.float64,
                                image_size=6)
    gpu_model = EPSesPlusLinear(((2, 3), (2, 4)), UnitTheoreticalOutputStd(), 1.0, torch.device("cuda"), torch.float64,
                                image_size=6)
    gpu_model.load_state_dict(cpu_model.state_dict())
    x = torch.rand(1, 4, 6, 6, 2, dtype=torch.float64)
    out = cpu_model(x)
    assert out.device.type == "cpu" and out.shape == (4, 10)
    out.logsumexp(1).sum().backward()
    ref = gpu_model(x.cuda())
    ref.logsumexp(1).sum().backward()
    assert torch.allclose(out, ref.cpu(), rtol=1e-12, atol=1e-14)
    for a, b in zip(cpu_model.parameters(), gpu_model.parameters()):
        assert a.grad.device.type == "cpu" and torch.allclose(a.grad, b.grad.cpu(), rtol=1e-10, atol=1e-13)


def test_logmatmulexp_cpu_inputs():
    from dctn.logmatmulexp import logmatmulexp, logmatmulexp_lowmem

    a = torch.randn(5, 7, dtype=torch.float64, requires_grad=True)
    b = torch.randn(7, 3, dtype=torch.float64, requires_grad=True)
    got = logmatmulexp(a, b)
    want = (a.detach().exp() @ b.detach().exp()).log()   # the reference's docstring definition (logmatmulexp.py:6-7)
    assert got.device.type == "cpu" and torch.allclose(got, want)
    assert torch.allclose(logmatmulexp_lowmem(a, b), want)
    got.sum().backward()
    assert a.grad.device.type == "cpu" and b.grad.device.type == "cpu"


def test_mixed_placement_raises():
    import dctn.eps

    with pytest.raises(RuntimeError, match="one device"):
        dctn.eps.eps(torch.randn(2, 2, 2, 2, 3), torch.randn(1, 2, 4, 4, 2, device="cuda"))


# ------------------------------------------------------------------ the device geometry the plans assume
# The library asks the device for its CU count and LDS per CU once (dctn_device_limits); DCTN_DEVICE_LIMITS="cus,lds"
# can only lower them.  Each family runs once at reduced size in a child process: on the card as it is, with a quarter
# of its CUs (every family must still run, on the same kernels, and match the oracle) and with 64 KiB of LDS (a shape
# that no longer fits must be declined - NotImplementedError - and never fail at the launch).
def _limits_cases():
    import dctn_amd
    import dctn_amd.eps_plus_linear as EPL
    from dctn_amd.conv_sbs import ConvSBS, DumbNormalInitialization, ManyConvSBS
    from dctn_amd.conv_sbs_spec import SBSSpecCore, SBSSpecString
    from dctn_amd.eps import eps
    from dctn_amd.logmatmulexp import logmatmulexp_fold
    from dctn_amd.pos2d import Pos2D
    from dctn_amd.tn_inner import gram_over_input_dims
    from dctn_amd.window_stats import apply_feature_map, window_mean_var
    from oracle import ref_cpu as R
    from tests.test_gpu_parity import bf16_close, close

    dev = torch.device("cuda:0")
    snake = [(0, 0), (0, 1), (0, 2), (1, 2), (1, 1), (1, 0), (2, 0), (2, 1), (2, 2)]

    def run_eps(C, B, H, W, Q, K, O, dtype, x_grad):
        N = K * K * C
        if Q == 2:
            u = torch.rand(C, B, H, W)
            x = torch.stack((torch.sin(u * torch.pi / 2) ** 2, torch.cos(u * torch.pi / 2) ** 2), dim=-1).to(dtype)
        else:
            x = torch.randn(C, B, H, W, Q, dtype=dtype)
        core = (torch.randn(*(Q,) * N, O, dtype=torch.float64) * Q ** (-N / 4)).to(dtype)
        xd, cd = x.to(dev).requires_grad_(x_grad), core.to(dev).requires_grad_(True)
        y = eps(cd, xd)
        names = [dctn_amd.last_kernel()]
        want = R.eps_4step(core.double(), x.double())
        dy = torch.randn(*want.shape, dtype=torch.float64).to(dtype)
        y.backward(dy.to(dev))
        names.append(dctn_amd.last_kernel())
        dcore, dx = R.grads(R.eps_4step, [core.double(), x.double()], dy.double())
        if dtype == torch.bfloat16:
            ok = bf16_close(y, want) and bf16_close(cd.grad, dcore)
        else:
            ok = close(y, want, dtype) and close(cd.grad, dcore, dtype) and (not x_grad or close(xd.grad, dx, dtype))
        return ok, names

    def run_head(dtype):
        torch.manual_seed(5)
        B, size, cout = 5, 12, 10
        core = (torch.randn(*(2,) * 9, 4) * 2.0 ** (-3.5)).to(dtype).to(dev).requires_grad_(True)
        w = (torch.randn(cout, 10 * 10 * 4) * 0.05).to(dtype).to(dev).requires_grad_(True)
        bias = torch.randn(cout).to(dtype).to(dev).requires_grad_(True)
        u = torch.rand(1, B, size, size)
        x = torch.stack([torch.sin(u * 1.5707963) ** 2, torch.cos(u * 1.5707963) ** 2], dim=-1).to(dtype).to(dev)
        assert EPL._EpsLinearHeadFunction.supported(core, x, w, bias)
        out = EPL._EpsLinearHeadFunction.apply(core, x, w, bias)
        names = [dctn_amd.last_kernel()]
        g = torch.randn(B, cout).to(dtype)
        out.backward(g.to(dev))
        names.append(dctn_amd.last_kernel())
        leaves = [t.detach().cpu().double().requires_grad_(True) for t in (core, w, bias)]
        want = R.eps_plus_linear_forward([leaves[0]], leaves[1], leaves[2], x.cpu().double())
        want.backward(g.double())
        pairs = [(out, want.detach())] + [(t.grad, r.grad) for t, r in zip((core, w, bias), leaves)]
        if dtype == torch.bfloat16:
            return all(bf16_close(a, b) for a, b in pairs), names
        return all(close(a, b, dtype) for a, b in pairs), names

    def run_sbs(module, x, pos_of_strings):
        ys = module(x)
        ys = ys if isinstance(ys, (tuple, list)) else (ys,)
        names = [dctn_amd.last_kernel()]
        dys = [torch.randn_like(y) for y in ys]
        torch.autograd.backward(list(ys), dys)
        names.append(dctn_amd.last_kernel())
        x64 = x.detach().cpu().double()
        strings = module.strings if hasattr(module, "strings") else [module]
        gx = torch.zeros_like(x64)
        ok = True
        for s, pos, y, dy in zip(strings, pos_of_strings, ys, dys):
            cores64 = [c.detach().cpu().double() for c in s.cores]
            ok = ok and close(y, R.convsbs_forward(cores64, pos, x64), x.dtype)
            gr = R.grads(lambda xx, *cc: R.convsbs_forward(cc, pos, xx), [x64] + cores64, dy.cpu().double())
            gx += gr[0]
            ok = ok and all(close(c.grad, gc, x.dtype) for c, gc in zip(s.cores, gr[1:]))
        return ok and close(x.grad, gx, x.dtype), names

    def snake_sbs(r, q, C, B, HW, dtype=torch.float32):
        spec = (tuple(SBSSpecCore(Pos2D(*p), 2 if i == 4 else 1) for i, p in enumerate(snake)),)
        many = ManyConvSBS(C, q, r, False, spec, (DumbNormalInitialization((q**C * r) ** -0.5),)).to(dev).to(dtype)
        x = torch.randn(C, B, HW, HW, q, device=dev, dtype=dtype, requires_grad=True)
        return run_sbs(many, x, [snake])

    def band_many():
        snake_b = [(0, 0), (1, 0), (2, 0), (2, 1), (1, 1), (0, 1), (0, 2), (1, 2), (2, 2)]
        outs = (1, 1, 1, 1, 2, 1, 1, 1, 1)
        specs = tuple(tuple(SBSSpecCore(Pos2D(h, w), o) for (h, w), o in zip(sn, outs)) for sn in (snake, snake_b))
        init = DumbNormalInitialization((4 * 16) ** -0.5 * 1.2)
        many = ManyConvSBS(2, 2, 16, False, specs, (init, init)).to(dev)
        x = torch.randn(2, 3, 7, 8, 2, device=dev, requires_grad=True)
        return run_sbs(many, x, [snake, snake_b])

    def sbs_ring():
        cores = (SBSSpecCore(Pos2D(0, 0), 1), SBSSpecCore(Pos2D(0, 1), 3), SBSSpecCore(Pos2D(1, 0), 2), SBSSpecCore(Pos2D(1, 1), 4))
        m = ConvSBS(SBSSpecString(cores, (3, 4, 5, 6), 2, 2)).to(dev)
        x = torch.randn(2, 3, 4, 5, 2, device=dev, requires_grad=True)
        return run_sbs(m, x, [[(c.position.h, c.position.w) for c in cores]])

    def fold():
        m = torch.randn(70, 9, 16, 16)
        md = m.to(dev).requires_grad_(True)
        y = logmatmulexp_fold(md)
        names = [dctn_amd.last_kernel()]
        dy = torch.randn(70, 16, 16)
        y.backward(dy.to(dev))
        names.append(dctn_amd.last_kernel())
        want = R.logmatmulexp_fold_batched(m.double())
        (gm,) = R.grads(R.logmatmulexp_fold_batched, [m.double()], dy.double())
        ok = torch.allclose(y.cpu().double(), want, rtol=5e-5, atol=5e-5)
        return ok and torch.allclose(md.grad.cpu().double(), gm, rtol=1e-4, atol=1e-4 * float(gm.abs().max())), names

    def window_stats():
        x = apply_feature_map(torch.rand(40, 28, 28))
        mean, var = window_mean_var(x.to(dev), 3)
        ref = R.window_mean_var_factor(x, 3)
        ok = np.isclose(float(mean), float(ref[0]), rtol=1e-6) and np.isclose(float(var), float(ref[1]), rtol=1e-5)
        return ok, [dctn_amd.last_kernel()]

    def tn_inner():
        a = torch.randn(4, 4, 4, 5, dtype=torch.float64)
        b = torch.randn(4, 4, 4, 6, dtype=torch.float64)
        ad, bd = a.to(dev).requires_grad_(True), b.to(dev).requires_grad_(True)
        g = gram_over_input_dims(ad, bd)
        names = [dctn_amd.last_kernel()]
        dg = torch.randn(5, 6, dtype=torch.float64)
        g.backward(dg.to(dev))
        names.append(dctn_amd.last_kernel())
        want = torch.einsum("ijko,ijkp->op", a, b)
        ok = close(g, want, torch.float64)
        ok = ok and close(ad.grad, torch.einsum("ijkp,op->ijko", b, dg), torch.float64)
        return ok and close(bd.grad, torch.einsum("ijko,op->ijkp", a, dg), torch.float64), names

    return {
        "eps_q2reg_bf16": lambda: run_eps(1, 3, 10, 10, 2, 3, 4, torch.bfloat16, False),
        "eps_q2f32": lambda: run_eps(1, 3, 10, 10, 2, 3, 4, torch.float32, False),
        "eps_bigcore_f32": lambda: run_eps(1, 2, 6, 7, 4, 3, 6, torch.float32, True),
        "eps_halves_f64": lambda: run_eps(1, 2, 28, 28, 2, 4, 2, torch.float64, True),
        "eps_generic": lambda: run_eps(2, 2, 7, 6, 2, 2, 3, torch.float64, True),
        "head_f32": lambda: run_head(torch.float32),
        "head_bf16": lambda: run_head(torch.bfloat16),
        "sbs_reg_r4": lambda: snake_sbs(4, 3, 1, 3, 12),
        "sbs_band_r8": lambda: snake_sbs(8, 3, 1, 2, 10),
        "sbs_band_r16": lambda: snake_sbs(16, 3, 1, 2, 8),
        "sbs_band_many": band_many,
        "sbs_mfma": sbs_ring,
        "sbs_generic": lambda: snake_sbs(3, 2, 1, 2, 7, torch.float64),
        "fold": fold,
        "window_stats": window_stats,
        "tn_inner": tn_inner,
    }


def _limits_child():
    """Child process: every case once; one JSON line {case: {ok, kernels} or {declined} or {error}} plus the limits."""
    import ctypes
    import json

    from dctn_amd import _lib

    out = {}
    for name, case in _limits_cases().items():
        torch.manual_seed(sum(map(ord, name)))
        try:
            ok, names = case()
            out[name] = {"ok": bool(ok), "kernels": names}
        except NotImplementedError as e:
            out[name] = {"declined": str(e)[:200]}
        except Exception as e:   # a launch error or anything else: reported, the parent fails on it
            out[name] = {"error": f"{type(e).__name__}: {str(e)[:300]}"}
        torch.cuda.synchronize()
    cus, lds = ctypes.c_int(), ctypes.c_int()
    assert _lib.lib().dctn_device_limits(ctypes.byref(cus), ctypes.byref(lds)) == 0
    print(json.dumps({"limits": [cus.value, lds.value], "cases": out}))


def _run_limits_child(limits):
    import json
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ)
    env.pop("DCTN_DEVICE_LIMITS", None)
    if limits:
        env["DCTN_DEVICE_LIMITS"] = limits
    code = f"import sys; sys.path.insert(0, {root!r}); from tests.test_gpu_boundary import _limits_child; _limits_child()"
    res = subprocess.run([sys.executable, "-c", code], cwd=root, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                         text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    return json.loads(res.stdout.strip().splitlines()[-1])


@functools.lru_cache(maxsize=None)
def _limits_run(limits):
    return _run_limits_child(limits)


def test_device_limits_are_the_mi355x_as_it_is():
    import ctypes

    from dctn_amd import _lib

    cus, lds = ctypes.c_int(), ctypes.c_int()
    assert _lib.lib().dctn_device_limits(ctypes.byref(cus), ctypes.byref(lds)) == 0
    assert cus.value == torch.cuda.get_device_properties(0).multi_processor_count
    if "gfx950" in torch.cuda.get_device_properties(0).gcnArchName:
        assert lds.value == 160 * 1024   # the plans of every family were written for it: on it the helper changes nothing


def test_fewer_cus_still_run_every_family_on_the_same_kernels():
    full = _limits_run(None)
    assert all(r.get("ok") for r in full["cases"].values()), full
    few = _limits_run("64,163840")
    assert few["limits"] == [64, full["limits"][1]]
    for name, r in few["cases"].items():
        assert r.get("ok"), (name, r)
        assert r["kernels"] == full["cases"][name]["kernels"], (name, r, full["cases"][name])


def test_less_lds_declines_cleanly():
    full = _limits_run(None)
    small = _limits_run("256,65536")
    assert small["limits"] == [full["limits"][0], 65536]
    handed = set()
    for name, r in small["cases"].items():
        assert "error" not in r, (name, r)
        assert "declined" in r or r["ok"], (name, r)
        if "declined" in r or r["kernels"] != full["cases"][name]["kernels"]:
            handed.add(name)
    assert {"sbs_band_r8", "sbs_band_r16", "eps_bigcore_f32", "eps_q2f32"} <= handed, small
