"""Workload for a kernel trace of the fused lexical head (profiles/lexical_head.txt):
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/lexical_trace.py
B=128 passages of fp16 logits (BERT vocabulary), L=128 and L=32, densify mode into fp16 / uint8 records; 3 calls per shape."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from dhr_amd import lexical as LX  # noqa: E402

V, dims, remove = 30522, 768, 570
for B, L in ((128, 128), (128, 32)):
    lg = torch.randn((B, L, V), device="cuda", dtype=torch.float16)[:, 1:]
    w = torch.randn((B, L - 1, 1), device="cuda", dtype=torch.float16)
    mask = torch.ones((B, L - 1), dtype=torch.long, device="cuda")
    rv = torch.empty((B, dims), dtype=torch.float16, device="cuda")
    ri = torch.empty((B, dims), dtype=torch.uint8, device="cuda")
    for _ in range(3):
        LX.densify_lexical_into(lg, w, mask, rv, ri, dims, remove)
    torch.cuda.synchronize()
    print("B=%d L=%d done" % (B, L))
