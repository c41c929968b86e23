#!/usr/bin/env python
"""What one k-means assignment and one full round (assignment + update) cost at the size of the MS MARCO training queries (N = 808 731,
K = 2 000), at d = 768 and at d = 128 (the documented CLSDIM), against eager torch on the same device in the same process, the two legs
alternating inside every round:

    fused   dhr_amd.cluster.assign / assign + update           (csrc/kmeans.hip: no [N, K] array, no atomics)
    eager   argmax(x @ c.T - |c|^2 / 2) over chunks of rows sized to a 1 GiB fp32 temporary, then index_add_ and a division

Both read the same fp16 rows and fp32 centroids (eager multiplies in fp16 x fp16(c): the product torch would take on this data; it is the
baseline for time, not for the bits).  After a warm-up every leg is repeated until a window of at least --window seconds is full, between
device events; medians and ranges over --rounds windows.  Workspace is the peak of torch's allocator over a leg (eager) and the library's own
layout (fused: the two fp16 images and the norms; for the update the sort buffers).

    python tools/kmeans_time.py [--n 808731] [--k 2000] [--dims 768,128] [--rounds 5] [--window 1.0] [--out profiles/kmeans.txt]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=808_731)
    ap.add_argument("--k", type=int, default=2000)
    ap.add_argument("--dims", default="768,128")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_outputs", "kmeans_time.txt"))
    args = ap.parse_args()
    import torch
    from dhr_amd import cluster
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    logf = open(args.out, "a")

    def log(*a):
        print(*a, flush=True)
        print(*a, file=logf, flush=True)
    dev = torch.device("cuda", 0)
    n, K = args.n, args.k
    log("# %s, N = %d, K = %d, %d windows of >= %.1f s per leg after a warm-up, legs alternating" % (torch.cuda.get_device_name(0), n, K, args.rounds, args.window))

    def window(fn):
        """calls of fn until the window is full -> ms per call (device events around the whole window)"""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        reps = max(1, int(np.ceil(args.window * 1e3 / max(e0.elapsed_time(e1), 1e-3))))
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps, reps

    for d in (int(x) for x in args.dims.split(",")):
        g = torch.Generator(device=dev).manual_seed(1)
        x = (torch.randn((n, d), generator=g, device=dev) * 0.1).half()
        c = x[torch.randperm(n, generator=g, device=dev)[:K]].float().contiguous()
        chunk = max(1, (1 << 30) // (4 * K))

        def eager_assign():
            c16 = c.half()
            hn = 0.5 * (c * c).sum(1)
            out = torch.empty(n, dtype=torch.int64, device=dev)
            for lo in range(0, n, chunk):
                out[lo:lo + chunk] = ((x[lo:lo + chunk] @ c16.T).float() - hn).argmax(1)
            return out

        def eager_round():
            a = eager_assign()
            s = torch.zeros((K, d), dtype=torch.float32, device=dev).index_add_(0, a, x.float())
            cnt = torch.bincount(a, minlength=K)
            return torch.where(cnt[:, None] > 0, s / cnt.clamp(min=1)[:, None], c)

        def fused_assign():
            return cluster.assign(x, c)

        def fused_round():
            a, _ = cluster.assign(x, c)
            return cluster.update(x, a, c)

        a_f = fused_assign()[0]
        a_e = eager_assign()
        log("d = %4d  rows on which eager (fp16 centroids) and fused disagree: %d of %d" % (d, int((a_f.long() != a_e).sum()), n))
        legs = {"assign fused": fused_assign, "assign eager": eager_assign, "round  fused": fused_round, "round  eager": eager_round}
        peak = {}
        for name, fn in legs.items():                                   # warm-up, and the allocator's peak over one call
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            fn()
            torch.cuda.synchronize()
            peak[name] = torch.cuda.max_memory_allocated() - base
        rec = {name: [] for name in legs}
        for _ in range(args.rounds):
            for name, fn in legs.items():
                rec[name].append(window(fn))
        flop = 2.0 * n * d * K
        d_pad, k_pad = (d + 127) // 128 * 128, (K + 31) // 32 * 32
        fused_ws = {"assign fused": 2 * k_pad * d_pad * 2 + k_pad * 4, "round  fused": 2 * k_pad * d_pad * 2 + k_pad * 4 + 4 * n * 4 + (K + 1) * 4}
        for name, xs in rec.items():
            ms = np.array([v[0] for v in xs])
            extra = ""
            if name.startswith("assign"):
                extra = "  %.1f Tflop/s of the %.3g algorithmic flop" % (flop / np.median(ms) / 1e9, flop)
            ws = "workspace %.1f MB (library layout, without the sort's own scratch; outputs %.1f MB)" % (fused_ws[name] / 1e6, peak[name] / 1e6) \
                if name in fused_ws else "workspace + outputs %.1f MB (allocator peak)" % (peak[name] / 1e6)
            log("d = %4d  %s  ms per call median %9.3f [%9.3f, %9.3f] over %d windows of %d calls%s  %s" %
                (d, name, np.median(ms), ms.min(), ms.max(), len(ms), xs[-1][1], extra, ws))
        med = {name: float(np.median([v[0] for v in xs])) for name, xs in rec.items()}
        log("d = %4d  fused / eager: assign %.2f x, round %.2f x (below 1: fused is faster)" %
            (d, med["assign fused"] / med["assign eager"], med["round  fused"] / med["round  eager"]))
        del x, c


if __name__ == "__main__":
    main()
