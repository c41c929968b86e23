"""Workloads behind profiles/lexical_proj.txt: the lexical head with the vocabulary projection fused in (a) against the parent composition,
torch.nn.functional.linear in fp16 followed by dhr_amd.lexical (b), on the same inputs.

    python tools/lexical_proj_profile.py time                     call times (device events, 3 warm-ups, median of 10) and peak memory
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/lexical_proj_profile.py trace fused      3 calls per shape, one path per run
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/lexical_proj_profile.py trace parent

B = 128 passages, H = 768, BERT vocabulary, L = 128 and L = 32 read through the [:, 1:] view, densify mode into fp16 / uint8 records; every
shape once with all tokens unmasked and once with per-passage lengths uniform in [L/4, L]."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from dhr_amd import lexical as LX  # noqa: E402
from dhr_amd import lexical_proj as LP  # noqa: E402

V, H, dims, remove, B = 30522, 768, 768, 570, 128


def workloads():
    gen = torch.Generator(device="cuda").manual_seed(1)
    W = (torch.randn((V, H), generator=gen, device="cuda") * 0.02).half()
    bias = (torch.randn((V,), generator=gen, device="cuda") * 0.1).half()
    for L in (128, 32):
        for ragged in (False, True):
            hidden = torch.randn((B, L, H), generator=gen, device="cuda").half()[:, 1:]
            w = torch.randn((B, L - 1), generator=gen, device="cuda").half()
            lens = torch.randint(L // 4, L + 1, (B, 1), generator=gen, device="cuda") - 1 if ragged else torch.full((B, 1), L - 1, device="cuda")
            mask = (torch.arange(L - 1, device="cuda")[None] < lens).long()
            rv = torch.empty((B, dims), dtype=torch.float16, device="cuda")
            ri = torch.empty((B, dims), dtype=torch.uint8, device="cuda")

            def fused(hidden=hidden, w=w, mask=mask, rv=rv, ri=ri):
                LP.densify_lexical_into(hidden, W, bias, w, mask, rv, ri, dims, remove)

            def parent(hidden=hidden, w=w, mask=mask, rv=rv, ri=ri):
                LX.densify_lexical_into(torch.nn.functional.linear(hidden, W, bias), w, mask, rv, ri, dims, remove)

            yield "L=%d %s (%d of %d tokens)" % (L, "ragged" if ragged else "full", int(mask.sum()), B * (L - 1)), fused, parent


def median_ms(fn):
    for _ in range(3):
        fn()
    times = []
    for _ in range(10):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    return float(np.median(times))


def peak_mb(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - before) / 1e6


if sys.argv[1] == "time":
    for name, fused, parent in workloads():
        a, b = median_ms(fused), median_ms(parent)
        print("%-40s fused %.3f ms  linear + head %.3f ms  ratio %.2fx  peak memory over the inputs: fused %.1f MB, parent %.1f MB"
              % (name, a, b, b / a, peak_mb(fused), peak_mb(parent)), flush=True)
else:
    for name, fused, parent in workloads():
        for _ in range(3):
            (fused if sys.argv[2] == "fused" else parent)()
        torch.cuda.synchronize()
        print(name, "done", flush=True)
