"""Workloads behind profiles/lexical_proj_train.txt: forward + backward of the differentiable lexical head with the vocabulary projection
fused in (a) against the parent composition (b), torch.nn.functional.linear in fp16 followed by dhr_amd.lexical_train.lexical_reps and
.backward(), in the same process on the same inputs.

    python tools/lexical_proj_train_profile.py time                  forward + backward times (device events, 3 warm-ups, median of 10), peak memory
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/lexical_proj_train_profile.py trace fused      3 steps per shape, one path per run
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/lexical_proj_train_profile.py trace parent

B = 128 passages, H = 768, BERT vocabulary, fp16 hidden states, weight, bias and term weights, skip_tokens = 1: L = 128 with every token
unmasked, L = 128 with per-passage lengths uniform in [32, 128], L = 32 with every token unmasked.  Gradients of hidden, weight, bias and
the term weights are all computed."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from dhr_amd import lexical_proj_train as LPT  # noqa: E402
from dhr_amd import lexical_train as LT  # noqa: E402

V, H, B = 30522, 768, 128


def workloads():
    gen = torch.Generator(device="cuda").manual_seed(1)
    W = (torch.randn((V, H), generator=gen, device="cuda") * 0.07).half().requires_grad_(True)
    bias = (torch.randn((V,), generator=gen, device="cuda") * 0.1).half().requires_grad_(True)
    for L, ragged in ((128, False), (128, True), (32, False)):
        hidden = torch.randn((B, L, H), generator=gen, device="cuda").half().requires_grad_(True)
        w = torch.randn((B, L - 1, 1), generator=gen, device="cuda").half().requires_grad_(True)
        lens = torch.randint(32, L + 1, (B, 1), generator=gen, device="cuda") - 1 if ragged else torch.full((B, 1), L - 1, device="cuda")
        mask = (torch.arange(L - 1, device="cuda")[None] < lens).long()
        G = torch.randn((B, V), generator=gen, device="cuda")

        def clear(hidden=hidden, w=w):
            hidden.grad = w.grad = W.grad = bias.grad = None

        def fused(hidden=hidden, w=w, mask=mask, G=G, clear=clear):
            clear()
            LPT.lexical_reps(hidden, W, bias, w, mask, skip_tokens=1).backward(G)

        def parent(hidden=hidden, w=w, mask=mask, G=G, clear=clear):
            clear()
            LT.lexical_reps(torch.nn.functional.linear(hidden, W, bias), w, mask, skip_tokens=1).backward(G)

        yield "L=%d %s (%d of %d tokens)" % (L, "ragged" if ragged else "full", int(mask.sum()), B * (L - 1)), fused, parent, clear


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


def peak_mb(fn, clear):
    clear()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - before) / 1e6


if sys.argv[1] == "time":
    for name, fused, parent, clear in workloads():
        a, b = median_ms(fused), median_ms(parent)
        print("%-40s fused %.3f ms  linear + head + backward %.3f ms  ratio %.2fx  peak memory over the inputs: fused %.1f MB, parent %.1f MB"
              % (name, a, b, b / a, peak_mb(fused, clear), peak_mb(parent, clear)), flush=True)
        clear()
else:
    for name, fused, parent, clear in workloads():
        for _ in range(3):
            (fused if sys.argv[2] == "fused" else parent)()
        torch.cuda.synchronize()
        clear()
        print(name, "done", flush=True)
