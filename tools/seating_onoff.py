#!/usr/bin/env python
"""In-process A/B of DHR_PARAM_SEAT_QUERIES (the seating of the main pass) on the bench corpus (hybrid = config 3, dense = config 2): alternating searches with the switch off
and at its default, serial (OVERLAP_AUX = 0: every kernel alone, candidate counts reproducible) and overlapped."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "bench_outputs")          # git-ignored, as the outputs of bench.py --dump-outputs
os.makedirs(OUT, exist_ok=True)


def main():
    import torch
    import bench
    from dhr_amd import _lib, synth
    from dhr_amd.retrieval.gip_retrieval import GipIndex
    workload = sys.argv[1] if len(sys.argv) > 1 else "hybrid"
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    logf = open(os.path.join(OUT, "seating_onoff_%s.log" % workload), "a")

    def log(*a):
        print(*a, flush=True)
        print(*a, file=logf, flush=True)
    d_dlr = 768 if workload == "hybrid" else 0
    dev = torch.device("cuda", 0)
    n, nq, k = bench.N_MSMARCO, bench.Q_DEV, 1000
    cv, ci = bench.gen_rows(torch, synth, dev, 1237, 0, n, d_dlr, 768, 30, 90, False, dup=True)
    qv, qi = bench.gen_rows(torch, synth, dev, 1237 + 999_983, 0, nq, d_dlr, 768, 4, 12, False, hot_frac=synth.HOT_FRAC)
    _lib.check(_lib.load().dhr_set_option(_lib.OPT_DENSE_I8, -1), "opt")
    ix = GipIndex(cv, ci)
    del cv, ci
    torch.cuda.empty_cache()
    ix.set_param(_lib.PARAM_PROFILE, 1)
    res = {}
    for overlap in (0, -1):
        ix.set_param(_lib.PARAM_OVERLAP_AUX, overlap)
        rec = {0: [], -1: []}
        for rd in range(rounds + 1):
            for seat in (0, -1):
                ix.set_param(_lib.PARAM_SEAT_QUERIES, seat)
                torch.cuda.synchronize()
                t = time.perf_counter()
                s, r = ix.search(qv, qi, k, out_device=True)
                torch.cuda.synchronize()
                wall = (time.perf_counter() - t) * 1e3
                st = ix.stats()
                st["wall_ms"] = wall
                st["checksum"] = bench.result_checksum(torch, s, r)
                if rd:
                    rec[seat].append(st)
        for seat in (0, -1):
            rs = rec[seat]
            med = lambda f: float(np.median([x[f] for x in rs]))
            rng_ = lambda f: (min(x[f] for x in rs), max(x[f] for x in rs))
            log("%s overlap %2d seat %2d: gemm_ms median %.3f [%.3f, %.3f]  total_ms median %.3f [%.3f, %.3f]  wall median %.3f  refine %.3f rescore %.3f select %.3f prep %.3f | "
                "kernel %d phases %s gemm_rows %s cb %s ce %s retries %s fallback %s checksum %s" %
                (workload, overlap, seat, med("gemm_ms"), *rng_("gemm_ms"), med("total_ms"), *rng_("total_ms"), med("wall_ms"), med("refine_ms"), med("rescore_ms"), med("select_ms"),
                 med("prep_ms"), int(ix.info(_lib.INFO_GEMM_KERNEL)), sorted({x["phases"] for x in rs}), sorted({x["gemm_rows"] for x in rs}), sorted({x["candidates_bound"] for x in rs}),
                 sorted({x["candidates_exact"] for x in rs}), sorted({x["overflow_retries"] for x in rs}), sorted({x["sample_fallback_queries"] for x in rs}),
                 sorted({json.dumps(x["checksum"]) for x in rs})))
        res[overlap] = {str(s_): [{f: v for f, v in x.items() if not isinstance(v, dict)} for x in rs_] for s_, rs_ in rec.items()}
    with open(os.path.join(OUT, "seating_onoff_%s.json" % workload), "w") as f:
        json.dump(res, f)
    ix.close()


if __name__ == "__main__":
    main()
