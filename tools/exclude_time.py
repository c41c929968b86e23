#!/usr/bin/env python
"""What per-query row exclusion costs on the bench corpus (hybrid = config 3: 8.8 M rows, 6 980 queries, top-1000), at E = 1 and E = 16
excluded rows per query (each query's own best E rows: positives rank high).  One process, one box, the legs alternating inside every round:

    (a)  dhr_search at k and at k + E          on --parent-lib, a library built from the commit before the feature (and on this build, beside it)
    (b)  dhr_search_excluding at k             on this build
    (c)  the filter kernel alone               dhr_exclude_rows on device lists [Q, k + E], device events around 20 calls

Step times are the host clock around a call that ends in a stream synchronise, and the library's own total_ms (device events); medians and
ranges over the rounds after one warm-up round.  (b) - (a at k + E) is what the feature adds to a search that is E deeper anyway.

    python tools/exclude_time.py [--parent-lib PATH] [--rounds 7] [--n-docs N] [--n-queries Q] [--out FILE]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--n-docs", type=int, default=0)
    ap.add_argument("--n-queries", type=int, default=0)
    ap.add_argument("--topk", type=int, default=1000)
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_outputs", "exclude_time.txt"))
    args = ap.parse_args()
    import torch
    import bench
    from dhr_amd import _lib, synth
    from dhr_amd.retrieval.gip_retrieval import GipIndex
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    logf = open(args.out, "a")

    def log(*a):
        print(*a, flush=True)
        print(*a, file=logf, flush=True)
    dev = torch.device("cuda", 0)
    n, nq, k = args.n_docs or bench.N_MSMARCO, args.n_queries or bench.Q_DEV, args.topk
    cv, ci = bench.gen_rows(torch, synth, dev, 1237, 0, n, 768, 768, 30, 90, False, dup=True)
    qv, qi = bench.gen_rows(torch, synth, dev, 1237 + 999_983, 0, nq, 768, 768, 4, 12, False, hot_frac=synth.HOT_FRAC)
    new_lib = _lib.load()
    _lib.check(new_lib.dhr_set_option(_lib.OPT_DENSE_I8, -1), "opt")
    handles = {"this": GipIndex(cv, ci)}
    if args.parent_lib:                               # a second library in the process, with an index of its own built from the same rows
        os.environ["DHR_HIP_LIB"] = os.path.abspath(args.parent_lib)
        _lib._lib = None
        par = _lib.load()
        assert par is not new_lib and not hasattr(par, "dhr_search_excluding"), "--parent-lib is not a library from before the feature"
        _lib.check(par.dhr_set_option(_lib.OPT_DENSE_I8, -1), "opt")
        handles["parent"] = GipIndex(cv, ci)
        _lib._lib = new_lib
        del os.environ["DHR_HIP_LIB"]
    del cv, ci
    torch.cuda.empty_cache()
    for ix in handles.values():
        ix.set_param(_lib.PARAM_PROFILE, 1)
    log("# corpus %d rows, %d queries, k = %d, rounds %d (+1 warm-up), libraries: %s" % (n, nq, k, args.rounds, ", ".join(handles)))

    def timed(fn, ix):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3, ix.stats()["total_ms"], out

    _, r_plain = handles["this"].search(qv, qi, k, out_device=True)
    for E in (1, 16):
        ptr = np.arange(nq + 1, dtype=np.int64) * E
        ex = r_plain[:, :E].contiguous().reshape(-1)
        legs = {}
        for name, ix in handles.items():
            legs["a: %s dhr_search k" % name] = (ix, lambda ix=ix: ix.search(qv, qi, k, out_device=True))
            legs["a: %s dhr_search k+E" % name] = (ix, lambda ix=ix: ix.search(qv, qi, k + E, out_device=True))
        legs["b: this dhr_search_excluding k"] = (handles["this"], lambda: handles["this"].search(qv, qi, k, out_device=True, exclude=(ptr, ex)))
        rec = {name: [] for name in legs}
        out = {}
        for rd in range(args.rounds + 1):
            for name, (ix, fn) in legs.items():
                wall, total, out[name] = timed(fn, ix)
                if rd:
                    rec[name].append((wall, total))
        for name, xs in rec.items():
            w, t = np.array([x[0] for x in xs]), np.array([x[1] for x in xs])
            log("E = %2d  %-36s wall ms median %8.3f [%8.3f, %8.3f]   total_ms median %8.3f [%8.3f, %8.3f]" % (E, name, np.median(w), w.min(), w.max(), np.median(t), t.min(), t.max()))
        med = {name: float(np.median([x[0] for x in xs])) for name, xs in rec.items()}
        base = "a: parent dhr_search k+E" if "parent" in handles else "a: this dhr_search k+E"
        step = med["a: parent dhr_search k" if "parent" in handles else "a: this dhr_search k"]
        log("E = %2d  (b) - (a at k + E, %s) = %+.3f ms = %+.2f %% of the step at k (%.3f ms); (a at k + E) - (a at k) = %+.3f ms" %
            (E, base.split()[1], med["b: this dhr_search_excluding k"] - med[base], 100 * (med["b: this dhr_search_excluding k"] - med[base]) / step, step, med[base] - step))
        # the filtered lists are the deeper plain lists without the excluded rows: same rows as the parent's own k + E search gives
        s_deep, r_deep = out[base]
        s_b, r_b = out["b: this dhr_search_excluding k"]
        keep = (r_deep.unsqueeze(2) != r_plain[:, :E].unsqueeze(1)).all(2)
        assert bool((keep.sum(1) >= k).all())
        pos = keep.cumsum(1) - 1
        want_r = torch.full_like(r_b, -1)
        want_s = torch.full_like(s_b, float("-inf"))
        sel = keep & (pos < k)
        qq = torch.arange(nq, device=dev).unsqueeze(1).expand_as(r_deep)
        want_r[qq[sel], pos[sel]] = r_deep[sel]
        want_s[qq[sel], pos[sel]] = s_deep[sel]
        log("E = %2d  lists of (b) equal the k + E lists of (%s) without the excluded rows: rows %s, scores %s" %
            (E, base.split()[1], bool((want_r == r_b).all()), bool((want_s == s_b).all())))
        # (c) the kernel alone
        s_in, r_in = out["a: this dhr_search k+E"]
        handles["this"].exclude_rows(s_in, r_in, (ptr, ex), k)
        reps = 20
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ms = []
        for _ in range(args.rounds):
            torch.cuda.synchronize()
            e0.record()
            for _ in range(reps):
                handles["this"].exclude_rows(s_in, r_in, (ptr, ex), k)
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1) / reps * 1e3)
        byt = nq * ((k + E) * 12 + k * 12 + E * 8)
        log("E = %2d  c: dhr_exclude_rows [%d, %d] -> [%d, %d], per call (device events over %d calls, allocation of the offsets included): median %.1f us [%.1f, %.1f], %.1f MB moved -> %.0f GB/s" %
            (E, nq, k + E, nq, k, reps, np.median(ms), min(ms), max(ms), byt / 1e6, byt / 1e3 / np.median(ms)))
    for ix in handles.values():
        ix.close()


if __name__ == "__main__":
    main()
