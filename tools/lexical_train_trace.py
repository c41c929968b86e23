"""Workload for a kernel trace of the differentiable lexical head (profiles/lexical_train.txt):
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/lexical_train_trace.py
The shapes of the reference's training recipe (24 queries x 8 passages per device, p_max_len 150, q_max_len 32, BERT vocabulary), fp16
logits, skip_tokens=1; 3 forward + backward calls per shape."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from dhr_amd import lexical_train as LT  # noqa: E402

V = 30522
for B, L in ((192, 150), (24, 32)):
    lg = torch.randn((B, L, V), device="cuda", dtype=torch.float16).requires_grad_(True)
    w = torch.randn((B, L - 1, 1), device="cuda", dtype=torch.float16).requires_grad_(True)
    mask = torch.ones((B, L - 1), dtype=torch.long, device="cuda")
    G = torch.randn((B, V), device="cuda")
    for _ in range(3):
        lg.grad = w.grad = None
        LT.lexical_reps(lg, w, mask, skip_tokens=1).backward(G)
    torch.cuda.synchronize()
    print("B=%d L=%d done" % (B, L))
    del lg, w, G
