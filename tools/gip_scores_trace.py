"""Workload for a kernel trace of the differentiable gated-inner-product scores (profiles/gip_scores.txt):
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/gip_scores_trace.py
Forward + backward of listwise_gip_scores from fp32 [B, 30522] reps at the three training shapes; 3 steps per shape."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from dhr_amd import gip_scores as GS  # noqa: E402

V = 30522
for n_q, n_p in ((24, 192), (96, 768), (192, 1536)):
    q = (torch.rand((n_q, V), device="cuda") * (torch.rand((n_q, V), device="cuda") < 0.02)).requires_grad_(True)
    p = (torch.rand((n_p, V), device="cuda") * (torch.rand((n_p, V), device="cuda") < 0.05)).requires_grad_(True)
    G = torch.randn((n_q, n_p), device="cuda")
    for _ in range(3):
        q.grad = p.grad = None
        GS.listwise_gip_scores(q, p, n_q).backward(G)
    torch.cuda.synchronize()
    print("n_q=%d n_p=%d done" % (n_q, n_p))
