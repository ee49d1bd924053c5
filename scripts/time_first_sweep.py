#!/usr/bin/env python3
"""First and second smoothing sweep of a fresh engine at the headline size (d = dy = 4, T = 10⁵, 1024 chains of one model): create,
set_data_device, run_async, sync — five fresh engines, after a throwaway one that loads the code objects.  The first sweep of a handle stores
the per-chain covariance array, later ones do not; run it from the root of each build's tree to compare two builds
(profiles/r12/first_sweep.txt)."""
import os
import sys
import time

sys.path.insert(0, os.path.join(os.getcwd(), "rxinfer.jl_amd"))
import torch

import rxhip
from rxhip import workloads

mdl = workloads.c1_model()
T, C = 100000, 1024
args = (mdl["A"], mdl["B"], mdl["P"], mdl["Q"], mdl["m0"], mdl["V0"])
torch.manual_seed(0)
y = torch.randn(T, C, 4, dtype=torch.float64, device="cuda:0")   # the timing does not depend on the values
ys = y[:4096].contiguous()
torch.cuda.synchronize()
with rxhip.LGSSMEngine(*args, T=4096, n_chains=C, device=0) as w:
    w.set_data_device(ys.data_ptr(), ys.numel(), keepalive=ys)
    w.run_async(1, True)
    w.sync()
ms = []
for _ in range(5):
    eng = rxhip.LGSSMEngine(*args, T=T, n_chains=C, device=0)
    eng.set_data_device(y.data_ptr(), y.numel(), keepalive=y)
    eng.sync()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    eng.run_async(1, True)
    eng.sync()
    t1 = time.perf_counter()
    eng.run_async(1, True)
    eng.sync()
    t2 = time.perf_counter()
    ms.append(((t1 - t0) * 1e3, (t2 - t1) * 1e3))
    eng.close()
first, second = [a for a, _ in ms], [b for _, b in ms]
print("first_sweep_ms", " ".join(f"{a:.3f}" for a in first), "min", f"{min(first):.3f}", "spread", f"{max(first) - min(first):.3f}")
print("second_sweep_ms", " ".join(f"{b:.3f}" for b in second), "min", f"{min(second):.3f}")
