"""A/B of the fused head's feature layout (eps_plus_linear.BLOCKED_FEATURES: row-major against "blocked4") on the bf16
headline model (python tools/blocked_features_ab.py [B] [repeats]): the model's forward + backward step, replayed from a
HIP graph (bench.device_time), alternating the two settings in one process, and whether the gradients agree bit for bit."""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import bench
import dctn_amd.eps_plus_linear as EPL
from dctn_amd.eps_plus_linear import EPSesPlusLinear, UnitTheoreticalOutputStd

dev = torch.device("cuda:0")
B = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
REP = int(sys.argv[2]) if len(sys.argv) > 2 else 3
torch.manual_seed(0)
model = EPSesPlusLinear(((3, 4),), UnitTheoreticalOutputStd(), 1.0, dev, torch.bfloat16, image_size=28)
params = list(model.parameters())
x = bench.synthetic_input(B, 28, 2, torch.bfloat16, dev, 1)
g = torch.randn(B, 10, device=dev).bfloat16()


def step():
    for p in params:
        p.grad = None
    model(x).backward(g)


grads = {}
for blocked in (False, True):
    EPL.BLOCKED_FEATURES = blocked
    step()
    grads[blocked] = [p.grad.clone() for p in params]
same = all(torch.equal(a, b) for a, b in zip(grads[False], grads[True]))
print(f"B = {B}: gradients bit-identical across layouts: {same}")
for _ in range(REP):
    for blocked in (False, True):
        EPL.BLOCKED_FEATURES = blocked
        t = bench.device_time(step, dev, 50) * 1e6
        print(f"{'blocked4' if blocked else 'row-major':9s} {t:7.2f} us/step")
EPL.BLOCKED_FEATURES = True
