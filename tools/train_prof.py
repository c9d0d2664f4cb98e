#!/usr/bin/env python3
"""The complete cfg2 bf16 training iteration with the fused tail, replayed from its HIP graph (for rocprofv3)."""
import argparse, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from dctn_amd.eps_plus_linear import EPSesPlusLinear, UnitTheoreticalOutputStd
from dctn_amd.training import FlatAdam, FlatSGD, GraphedTrainStep, fused_cross_entropy

ap = argparse.ArgumentParser()
ap.add_argument("--optimizer", choices=("sgd", "adam", "torch_adam", "torch_adam_fused"), default="sgd")
args = ap.parse_args()

dev = torch.device("cuda:0")
torch.manual_seed(0)
model = EPSesPlusLinear(((3, 4),), UnitTheoreticalOutputStd(), 1.0, dev, torch.bfloat16)
u = torch.rand(1, 1024, 28, 28)
x = torch.stack((torch.sin(u * torch.pi / 2) ** 2, torch.cos(u * torch.pi / 2) ** 2), dim=-1).to(torch.bfloat16).to(dev)
y = torch.randint(0, 10, (1024,), device=dev)
flat, reg = (list(model.epses) + [model.linear.weight], [model.linear.bias]), {}
if args.optimizer == "sgd":
    opt = FlatSGD(*flat, lr=1e-3, momentum=0.9, l2=1e-2)
elif args.optimizer == "adam":
    opt = FlatAdam(*flat, lr=1e-3, weight_decay=1e-4, l2=1e-2)
else:   # the library optimizer: the regulariser goes through autograd
    opt = torch.optim.Adam(model.parameters(), lr=1e-3, weight_decay=1e-4, capturable=True,
                           fused=True if args.optimizer == "torch_adam_fused" else None)
    reg = dict(reg_fn=lambda m: m.epswise_l2_regularizer(), reg_coeff=1e-2)
step = GraphedTrainStep(model, x, y, fused_cross_entropy, opt, warmup=2, **reg)
for _ in range(200):
    step(x, y)
torch.cuda.synchronize()
