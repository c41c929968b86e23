#!/usr/bin/env python
"""Epilogue cycles of gemm_filter_g8_kernel by query tile, for the given and the sorted query order, open and closed filter (-DG8_TRACE=1 build
of the library: tools/ab_build.sh trace "-DG8_TRACE=1", DHR_HIP_LIB=dhr_amd/csrc/_ab/libdhr_hip_trace.so).  First 1 M rows of the bench
corpus, bench queries, final thresholds; the order is read from bench_outputs/seating_totals_hybrid.npy (tools/seating_order_probe.py)."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "bench_outputs")          # git-ignored, as the outputs of bench.py --dump-outputs
os.makedirs(OUT, exist_ok=True)


def log(*a):
    print(*a, flush=True)
    with open(os.path.join(OUT, "seating_trace.log"), "a") as f:
        print(*a, file=f)


def main():
    import torch
    import bench
    from dhr_amd import _lib, synth
    from dhr_amd.retrieval.gip_retrieval import GipIndex
    dev = torch.device("cuda", 0)
    n, nq, k = 1_000_000, bench.Q_DEV, 1000
    cv, ci = bench.gen_rows(torch, synth, dev, 1237, 0, n, 768, 768, 30, 90, False, dup=True)
    qv, qi = bench.gen_rows(torch, synth, dev, 1237 + 999_983, 0, nq, 768, 768, 4, 12, False, hot_frac=synth.HOT_FRAC)
    ix = GipIndex(cv, ci)
    del cv, ci
    lib = ix._lib
    tr = getattr(lib, "dhr_debug_g8_trace", None)
    if tr is None:
        raise SystemExit("this library was not built with -DG8_TRACE=1")
    tr.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_uint)]
    ix.set_param(_lib.PARAM_OVERLAP_AUX, 0)
    totals = torch.from_numpy(np.load(os.path.join(OUT, "seating_totals_hybrid.npy")).astype(np.float64)).to(dev)
    orders = {"given": torch.arange(nq, device=dev), "desc": torch.argsort(-totals, stable=True)}
    cap = 1 << 18
    for closed in (False, True):
        for nm, o in orders.items():
            a, b = qv[o].contiguous(), qi[o].contiguous()
            ix.search(a, b, k, out_device=True)
            os.environ["DHR_GEMM_TIME_OPEN"] = "0" if closed else "1"
            qb, keep = _lib.make_query_batch(a, b)
            ms, fl = C.c_double(), C.c_double()
            nrec = C.c_uint()
            torch.cuda.synchronize()
            assert tr(None, 0, C.byref(nrec)) == 0
            _lib.check(lib.dhr_debug_gemm_time(ix._h, C.byref(qb), 1, C.byref(ms), C.byref(fl), None), "gemm_time")
            torch.cuda.synchronize()
            buf = np.zeros((cap, 8), dtype=np.uint64)
            assert tr(buf.ctypes.data, cap, C.byref(nrec)) == 0
            r = buf[:min(nrec.value, cap)].astype(np.int64)
            r = r[np.argsort(r[:, 0])][-(len(r) // 2):]          # the timed launch
            epi = r[:, 6] - r[:, 5]
            whole = r[:, 6] - r[:, 1]
            qt = (r[:, 7] >> 40) & 0xff
            ok = (epi > 0) & (epi < 1_000_000) & (whole > 0) & (whole < 10_000_000)
            log("%s filter, %s order: launch %.3f ms, %d tile records; epilogue mean %.0f cycles, whole tile mean %.0f" %
                ("closed" if closed else "open", nm, ms.value, len(r), epi[ok].mean(), whole[ok].mean()))
            line = []
            for t in range(int(qt.max()) + 1):
                sel = ok & (qt == t)
                line.append("%d:%.1fk" % (t, epi[sel].mean() / 1e3))
            log("   epilogue cycles by query tile  " + " ".join(line))
    ix.close()


if __name__ == "__main__":
    main()
