"""Workload for a kernel trace of the differentiable MaxSim scores (profiles/maxsim_scores.txt):
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/maxsim_trace.py
The shapes of the reference's ColBERT / TCT recipe (24 queries x 8 passages per device on 1, 4 and 8 ranks; 31 query and 149 passage tokens
after the CLS token, 128 dims), fp16; 3 forward + backward calls per shape."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from dhr_amd import maxsim_scores as MS  # noqa: E402

Lq, Lp, D = 31, 149, 128
for A, B in ((24, 192), (96, 768), (192, 1536)):
    q = (torch.rand((A, Lq, D), device="cuda") - 0.5).half().requires_grad_(True)
    p = (torch.rand((B, Lp, D), device="cuda") - 0.5).half().requires_grad_(True)
    G = torch.randn((A, B), device="cuda")
    for _ in range(3):
        q.grad = p.grad = None
        MS.listwise_maxsim(q, p).backward(G)
    torch.cuda.synchronize()
    print("A=%d B=%d done" % (A, B))
    del q, p, G
