"""Workload for a kernel trace of the fused training loss (profiles/train_loss.txt):
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/train_loss_trace.py
The score matrices of the reference's DHR recipe (24 queries x 8 passages per device on 1, 4 and 8 ranks with cross-device negatives), fp32,
with teacher scores (--tct) and with hard labels; 5 forward + backward calls per shape and form."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from dhr_amd import train_loss as TL  # noqa: E402

for R, C in ((24, 192), (96, 768), (192, 1536)):
    lex = (torch.randn((R, C), device="cuda") * 4).requires_grad_(True)
    sem = (torch.randn((R, C), device="cuda") * 4).requires_grad_(True)
    tea = torch.randn((R, C), device="cuda") * 4
    for teacher in (tea, None):
        for _ in range(5):
            lex.grad = sem.grad = None
            loss, _scores = TL.dhr_loss(lex, sem, teacher, train_n_passages=8, lamb=1.0)
            loss.backward()
        torch.cuda.synchronize()
        print("R=%d C=%d %s done, loss %.6f" % (R, C, "tct" if teacher is not None else "hard labels", loss.item()))
    del lex, sem, tea
