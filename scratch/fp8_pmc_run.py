"""One fp8 top-k at 1024 x 20 000 x 1030 after a warm-up: the workload of the counter pass of DESIGN.md §4.5
(rocprofv3 --pmc ... --kernel-include-regex maxsim_fwd8 -- python scratch/fp8_pmc_run.py; counters only, no tracing)."""
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fp8_bench as B  # noqa: E402

dev = torch.device("cuda:0")
cb, c8 = B.build(20000, 1030, dev)
del cb
Q = F.normalize(torch.randn((1024, B.LQ, B.D), generator=torch.Generator(device=dev).manual_seed(3), device=dev), dim=-1)
for _ in range(2):
    c8.topk(Q, None, B.K)
torch.cuda.synchronize()
print("ok")
