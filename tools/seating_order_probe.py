#!/usr/bin/env python
"""Does the ORDER of the queries in the batch change the bound GEMM's time?  The premise of the seating of the main pass,
measured without it (DHR_PARAM_SEAT_QUERIES = 0): the bench corpus
(config 3; `dense`: config 2), the same batch searched in the given order and with its rows permuted on the host, descending and ascending by
per-query bound-candidate totals (bound scores of a 100 k-row slice against the final thresholds) -> bench_outputs/seating_probe*.
usage: python tools/seating_order_probe.py [hybrid|dense] [rounds]; profiles/query_seating.txt has the figures."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "bench_outputs")          # git-ignored, as the outputs of bench.py --dump-outputs
os.makedirs(OUT, exist_ok=True)


def log(*a):
    print(*a, flush=True)
    with open(os.path.join(OUT, "seating_probe.log"), "a") as f:
        print(*a, file=f)


def main():
    import torch
    import bench
    from dhr_amd import _lib, synth
    from dhr_amd.retrieval.gip_retrieval import GipIndex
    workload = sys.argv[1] if len(sys.argv) > 1 else "hybrid"
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    d_dlr = 768 if workload == "hybrid" else 0
    dev = torch.device("cuda", 0)
    n, nq, k, m = bench.N_MSMARCO, bench.Q_DEV, 1000, 100_000
    t0 = time.time()
    cv, ci = bench.gen_rows(torch, synth, dev, 1237, 0, n, d_dlr, 768, 30, 90, False, dup=True)
    qv, qi = bench.gen_rows(torch, synth, dev, 1237 + 999_983, 0, nq, d_dlr, 768, 4, 12, False, hot_frac=synth.HOT_FRAC)
    torch.cuda.synchronize()
    log("%s: data %.1f s" % (workload, time.time() - t0))
    _lib.check(_lib.load().dhr_set_option(_lib.OPT_DENSE_I8, -1), "opt")
    ix = GipIndex(cv, ci)
    del cv, ci
    torch.cuda.empty_cache()
    torch.cuda.synchronize()
    log("index %.1f s, kernel id %d" % (time.time() - t0, int(ix.info(_lib.INFO_GEMM_KERNEL))))
    ix.set_param(_lib.PARAM_PROFILE, 1)
    ix.set_param(_lib.PARAM_OVERLAP_AUX, 0)
    ix.set_param(_lib.PARAM_SEAT_QUERIES, 0)          # every query computes where the permuted batch puts it

    def run(perm):
        a = qv[perm].contiguous()
        b = None if qi is None else qi[perm].contiguous()
        torch.cuda.synchronize()
        t = time.perf_counter()
        s, r = ix.search(a, b, k, out_device=True)
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t) * 1e3
        return s, r, ix.stats(), wall, (a, b)

    ident = torch.arange(nq, device=dev)
    s0, r0, st, _, _ = run(ident)
    log("checksum", bench.result_checksum(torch, s0, r0))
    # per-query bound-candidate totals: bound scores of a 100k-row slice against the final k-th score minus the filter margin
    kth = s0[:, k - 1]
    qb, keep = _lib.make_query_batch(qv, qi)
    mg = np.zeros(nq, np.float32)
    _lib.check(ix._lib.dhr_debug_query_margins(ix._h, C.byref(qb), mg.ctypes.data, None), "margins")
    thr = kth - torch.from_numpy(mg).to(dev)
    cnt = torch.zeros(nq, device=dev, dtype=torch.float64)
    step = 25_000
    U = torch.empty((nq, step), dtype=torch.float32, device=dev)
    for lo in range(0, m, step):
        _lib.check(ix._lib.dhr_debug_bound_scores(ix._h, C.byref(qb), lo, lo + step, U.data_ptr(), None), "bound_scores")
        cnt += (U >= thr[:, None]).sum(1)
    del U
    c = cnt.cpu().numpy() * (n / m)
    np.save(os.path.join(OUT, "seating_totals_%s.npy" % workload), c.astype(np.float32))
    srt = np.sort(c)[::-1]
    log("bound candidates per query (slice estimate, final thresholds): mean %.0f median %.0f p99 %.0f max %.0f; top 1 %% hold %.1f %%, top 10 %% hold %.1f %%" %
        (c.mean(), np.median(c), np.percentile(c, 99), c.max(), 100 * srt[:nq // 100].sum() / c.sum(), 100 * srt[:nq // 10].sum() / c.sum()))
    # modelled share of four-accumulator blocks entered per wave column (32 queries x 8 accumulators)
    p = np.clip(c / n, 0, 1)

    def blocks(order):
        pp = p[order]
        pad = (-len(pp)) % 32
        pp = np.concatenate([pp, np.zeros(pad)]).reshape(-1, 32)
        return float((1 - np.prod((1 - pp) ** 8, axis=1)).mean())
    cn = torch.from_numpy(c).to(dev)
    desc = torch.argsort(-cn, stable=True)
    asc = torch.argsort(cn, stable=True)
    orders = {"given": ident, "desc": desc, "asc": asc}
    for nm, o in orders.items():
        log("  modelled taken-block share, %s order: %.3f" % (nm, blocks(o.cpu().numpy())))

    rec = {nm: [] for nm in orders}
    for rd in range(rounds + 1):          # round 0 warms every order
        for nm, o in orders.items():
            s, r, st, wall, qq = run(o)
            same = bool(torch.equal(s, s0[o])) and bool(torch.equal(r, r0[o]))
            # the kernel alone over the whole shard with the final thresholds of this search (DHR_GEMM_TIME_OPEN)
            os.environ["DHR_GEMM_TIME_OPEN"] = "1"
            qb2, keep2 = _lib.make_query_batch(qq[0], qq[1])
            ms, fl = C.c_double(), C.c_double()
            _lib.check(ix._lib.dhr_debug_gemm_time(ix._h, C.byref(qb2), 1, C.byref(ms), C.byref(fl), None), "gemm_time")
            os.environ["DHR_GEMM_TIME_OPEN"] = "0"
            if rd:
                rec[nm].append(dict(gemm_ms=st["gemm_ms"], total_ms=st["total_ms"], wall_ms=wall, cb=st["candidates_bound"], ce=st["candidates_exact"],
                                    phases=st["phases"], gemm_rows=st["gemm_rows"], same=same, open_whole_ms=ms.value,
                                    refine_ms=st["refine_ms"], rescore_ms=st["rescore_ms"]))
            log(rd, nm, "gemm %.3f total %.3f wall %.3f cb %d ce %d phases %d rows %d same %s | whole-shard open launch %.3f ms" %
                (st["gemm_ms"], st["total_ms"], wall, st["candidates_bound"], st["candidates_exact"], st["phases"], st["gemm_rows"], same, ms.value))
    for nm, rs in rec.items():
        g = np.array([x["gemm_ms"] for x in rs]); t = np.array([x["total_ms"] for x in rs]); w = np.array([x["open_whole_ms"] for x in rs])
        log("%-6s gemm_ms median %.3f min %.3f max %.3f | total_ms median %.3f min %.3f max %.3f | open whole-shard launch median %.3f min %.3f max %.3f | cb %s ce %s same %s" %
            (nm, np.median(g), g.min(), g.max(), np.median(t), t.min(), t.max(), np.median(w), w.min(), w.max(),
             sorted({x["cb"] for x in rs}), sorted({x["ce"] for x in rs}), all(x["same"] for x in rs)))
    with open(os.path.join(OUT, "seating_probe_%s.json" % workload), "w") as f:
        json.dump(rec, f)
    ix.close()


if __name__ == "__main__":
    main()
