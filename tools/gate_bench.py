#!/usr/bin/env python3
"""Gate forward / backward of layer 3 (config_energy, l_max 2) in isolation, HIP-event timed, in both output layouts, next to a
float4 copy that moves the same number of bytes as the backward: python tools/gate_bench.py [molecules]"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "equivariant-nn-zoo_amd"))
import torch
from e3_layers_amd.backend import ops
from e3_layers_amd.configs import config_energy
from e3_layers_amd.utils import build
dev = torch.device("cuda:0")
B = int(sys.argv[1]) if len(sys.argv) > 1 else 256
n = 18 * B
model = build(config_energy.get_config(l_max=2).model_config).to(dev)
gate = model.layer3.equivariant_nonlin
spec = gate._spec
x = torch.randn(n, spec.in_dim, device=dev)
gy = torch.randn(n, spec.out_dim, device=dev)
def timeit(fn, reps=50):
    for _ in range(5): fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps): fn()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps
mb_f = 4e-6 * n * (spec.in_dim + spec.out_dim)          # MB the forward moves
mb_b = 4e-6 * n * (2 * spec.in_dim + spec.out_dim)      # ... and the backward
# the yardstick: an elementwise float4 kernel (torch's vectorised negation) that reads and writes mb_b between them
src = torch.randn(int(mb_b * 1e6 / 8), device=dev)
dst = torch.empty_like(src)
copy = timeit(lambda: torch.neg(src, out=dst))
print(f"float4 copy of {mb_b:.1f} MB: {copy:.1f} us ({mb_b / copy:.2f} TB/s)")
for cf in (True, False):
    fwd = timeit(lambda: ops._gate_fwd_raw(x, spec, cf))
    bwd = timeit(lambda: ops._gate_bwd_raw(x, gy, spec, cf))
    bwd2 = timeit(lambda: ops._gate_bwd_raw(x, gy, spec, cf, gy))
    print(f"gate rows {n} in {spec.in_dim} out {spec.out_dim} {'cf' if cf else 'e3nn'} output: fwd {fwd:.1f} us ({mb_f / fwd:.2f} TB/s), "
          f"bwd {bwd:.1f} us ({mb_b / bwd:.2f} TB/s, {bwd / copy:.2f} x the copy), bwd with g_y2 {bwd2:.1f} us")
