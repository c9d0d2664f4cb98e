#!/usr/bin/env python3
"""Device time of the ConvSBS calls of the reference's classifier (mnist.py:189-222) at the bonds the wide backward
(convsbs_wide.hip) serves, B = 128 in the MNIST geometry (28 x 28 -> 26 x 26 -> 24 x 24 -> 22 x 22), graph-timed like
tools/time_convsbs_calls.py:

  1. forward and backward (dX + dCores) of every string of the three layers at bonds 24 and 32, float32;
  2. the same-shape A/B of the backward, the wide family forced (DCTN_SBS_WIDE_SWEEP) against the generic sweep, at the
     largest bonds the generic sweep still takes: final string r = 17, middle string r = 24;
  3. per wide backward, the share of the float32 matrix peak (157.3 TFLOP/s) on algorithmic flops: the dCore GEMM
     2 (q^C l)(o r)(windows oacc) plus the two sweeps' state products (forward 2 windows oacc o l r, adjoint twice that).

    python tools/time_convsbs_wide.py [B]
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from dctn_amd import _lib as L  # noqa: E402

SNAKE_A = [(0, 0), (0, 1), (0, 2), (1, 2), (1, 1), (1, 0), (2, 0), (2, 1), (2, 2)]   # mnist.py:190-199
SNAKE_B = [(0, 0), (1, 0), (2, 0), (2, 1), (1, 1), (0, 1), (0, 2), (1, 2), (2, 2)]   # mnist.py:201-210
PEAK_F32_MATRIX = 157.3e12
dev = torch.device("cuda:0")
B = int(sys.argv[1]) if len(sys.argv) > 1 else 128


def graph_time(fn, iters=10, per=2):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(per):
            fn()
    g.replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters / per * 1e3


class Call:
    """One string's forward and backward through the C ABI (float32), buffers allocated once."""

    def __init__(self, snake, mid, r, C, HW, flags=0):
        self.n, self.C, self.HW, self.q = 9, C, HW, 2
        self.outs_l = [mid if i == 4 else 1 for i in range(9)]
        self.bonds_l = [1] + [r] * 8
        self.outs, self.bonds = L.int_array(self.outs_l), L.int_array(self.bonds_l)
        self.ph, self.pw = L.int_array([p[0] for p in snake]), L.int_array([p[1] for p in snake])
        torch.manual_seed(r)
        self.cores = [torch.randn(o, self.bonds_l[c], self.bonds_l[(c + 1) % 9], *(2,) * C, device=dev) * (4 * r) ** -0.5
                      for c, o in enumerate(self.outs_l)]
        self.x = torch.rand(C, B, HW, HW, 2, device=dev)
        self.out = torch.empty(B, HW - 2, HW - 2, mid, device=dev)
        self.dy = torch.randn_like(self.out)
        self.dx = torch.empty_like(self.x)
        self.dcs = [torch.empty_like(c) for c in self.cores]
        self.code = L.F32 | flags
        lib = L.lib()
        args = (9, self.outs, self.bonds, C, B, HW, HW, 2, self.ph, self.pw, self.code)
        self.wsb = torch.empty(max(256, lib.dctn_convsbs_workspace_bytes(*args, 1)), dtype=torch.uint8, device=dev)
        self.wsf = torch.empty(max(256, lib.dctn_convsbs_workspace_bytes(*args, 0)), dtype=torch.uint8, device=dev)
        self.cp, self.dcp, self.xs = L.ptr_array(self.cores), L.ptr_array(self.dcs), L.strides5(self.x)

    def fwd(self):
        L.check(L.lib().dctn_convsbs_fwd(self.x.data_ptr(), self.xs, self.cp, self.out.data_ptr(), 9, self.outs, self.bonds, self.ph,
                                         self.pw, self.C, B, self.HW, self.HW, 2, self.wsf.data_ptr(), self.wsf.numel(), self.code,
                                         L.stream_ptr(dev)), "forward")

    def bwd(self):
        L.check(L.lib().dctn_convsbs_bwd(self.x.data_ptr(), self.xs, self.cp, self.dy.data_ptr(), self.dx.data_ptr(), self.dcp, 9,
                                         self.outs, self.bonds, self.ph, self.pw, self.C, B, self.HW, self.HW, 2, self.wsb.data_ptr(),
                                         self.wsb.numel(), self.code, L.stream_ptr(dev)), "backward")

    def flops(self):
        """algorithmic flops of the backward (see the module doc)"""
        W = B * (self.HW - 2) ** 2
        qc, oacc, total = 2 ** self.C, 1, 0
        for c in range(9):
            o, l, r = self.outs_l[c], self.bonds_l[c], self.bonds_l[(c + 1) % 9]
            total += 2 * (qc * l) * (o * r) * (W * oacc)   # dCore GEMM
            total += 3 * 2 * W * oacc * o * l * r           # forward sweep + adjoint sweep (two products)
            oacc *= o
        return total


def timed(call):
    f = graph_time(call.fwd)
    b = graph_time(call.bwd)
    return f, b, L.last_kernel()


print(f"B = {B}, float32, device time per call (us), graph-timed", flush=True)
LAYERS = [("layer 1", 1, 28, [(SNAKE_A, 2), (SNAKE_B, 2)]), ("layer 2", 2, 26, [(SNAKE_A, 2), (SNAKE_B, 2)]),
          ("final", 2, 24, [(SNAKE_A, 10)])]
for r in (24, 32):
    tot_f = tot_b = 0.0
    for name, C, HW, strings in LAYERS:
        for k, (snake, mid) in enumerate(strings):
            call = Call(snake, mid, r, C, HW)
            f, b, kern = timed(call)
            tot_f += f
            tot_b += b
            share = ""
            if kern.startswith("convsbs_bwd_wide"):
                share = f"  {call.flops() / (b * 1e-6) / 1e12:6.2f} TFLOP/s = {call.flops() / (b * 1e-6) / PEAK_F32_MATRIX:6.2%} of f32 matrix peak"
            print(f"r = {r:2d} {name} string {k}: fwd {f:9.1f}  bwd {b:9.1f}  [{kern}]{share}", flush=True)
            del call
            torch.cuda.empty_cache()
    print(f"r = {r:2d} classifier (all strings): fwd {tot_f:9.1f}  bwd {tot_b:9.1f}  fwd + bwd {tot_f + tot_b:9.1f}", flush=True)

print("A/B of the backward, same shape: generic sweep vs the wide family forced", flush=True)
for name, C, HW, mid, r in (("final", 2, 24, 10, 17), ("middle (layer 2)", 2, 26, 2, 24)):
    res = []
    for flags in (0, L.SBS_WIDE_SWEEP):
        call = Call(SNAKE_A, mid, r, C, HW, flags)
        _, b, kern = timed(call)
        res.append((b, kern, call.flops()))
        del call
        torch.cuda.empty_cache()
    (bg, kg, fl), (bw, kw, _) = res
    print(f"{name} r = {r}: {kg} {bg:9.1f} us | {kw} {bw:9.1f} us ({bw / bg:5.2f} x)  wide at "
          f"{fl / (bw * 1e-6) / PEAK_F32_MATRIX:6.2%} of f32 matrix peak", flush=True)
