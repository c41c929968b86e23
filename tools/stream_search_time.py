#!/usr/bin/env python
"""What one `add` of the streamed exact search costs at the size of the reference's un-densified BEIR route: 16 384 passages x (30 522 lexical +
128 semantic) fp32 columns against Q = 1 024 and Q = 6 980 queries, k = 1 000, the lists warm from a previous chunk of the same size -- against
the route's own op sequence on the same device in the same process, the two legs alternating inside every round:

    fused   dhr_amd.stream_search.StreamSearch.add     (csrc/stream_search.hip: split fp16 products, float64 fold, threshold filter, select)
    torch   torch.mm in fp32 -> torch.topk(k) -> cat with the running lists -> torch.topk(k)          (materialises [Q, 16 384] scores)

Every timed call starts from the same state, the lists after chunk 0: the fused leg builds a fresh search and adds chunk 0 outside the timed
region.  Times are between device events around the one call, medians and ranges over --reps calls after a warm-up of both legs.  Also printed:
the workspace of each leg (the library's own device_bytes(), of which the query images; torch's allocator peak over a call), the share of the
chunk's scores that pass the filter (score above the query's k-th after chunk 0, counted from the torch scores), the algorithmic Tflop/s of the
whole add (2 Q N D over its time: exponent pass, scoring kernel and select together) against the two ceilings, and how far the two legs' answers
agree.

    python tools/stream_search_time.py [--queries 1024,6980] [--rows 16384] [--k 1000] [--reps 7] [--out bench_outputs/stream_search_time.txt]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

V, DS = 30522, 128
PEAK_F16_DENSE, PEAK_F32_MFMA = 2500.0, 157.0          # Tflop/s


def rows_like_the_route(n, lo, hi, seed, dev):
    """[n, V] lexical reps (a softmax leak around e^-14 under `lo`..`hi` real term weights per row, Zipf columns) and [n, DS] semantic reps"""
    import torch
    g = torch.Generator(device=dev).manual_seed(seed)
    lex = torch.exp(torch.randn((n, V), generator=g, device=dev) * 2.0 - 14.0)
    p = 1.0 / torch.arange(1, V + 1, device=dev, dtype=torch.float64) ** 1.1
    perm = torch.randperm(V, generator=g, device=dev)
    cols = perm[torch.multinomial(p, n * hi, replacement=True, generator=g).view(n, hi)]
    vals = torch.rand((n, hi), generator=g, device=dev) * 1.95 + 0.05
    keep = torch.arange(hi, device=dev)[None, :] < torch.randint(lo, hi + 1, (n, 1), generator=g, device=dev)
    rows = torch.arange(n, device=dev)[:, None].expand(n, hi)
    lex[rows[keep], cols[keep]] = vals[keep]
    return lex, torch.randn((n, DS), generator=g, device=dev) * 0.1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", default="1024,6980")
    ap.add_argument("--rows", type=int, default=16384)
    ap.add_argument("--k", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_outputs", "stream_search_time.txt"))
    args = ap.parse_args()
    import torch
    from dhr_amd.stream_search import StreamSearch
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    logf = open(args.out, "a")

    def log(*a):
        print(*a, flush=True)
        print(*a, file=logf, flush=True)
    dev = torch.device("cuda", 0)
    n, k, D = args.rows, args.k, V + DS
    log("# %s, one add of %d rows x (%d + %d) fp32, k = %d, lists warm from a chunk of the same size; %d timed calls per leg after a warm-up, legs alternating"
        % (torch.cuda.get_device_name(0), n, V, DS, k, args.reps))
    chunks = [rows_like_the_route(n, 20, 80, 2 + i, dev) for i in range(2)]
    cat = [torch.cat(c, 1) for c in chunks]                  # the route scores one concatenated matrix per text

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), out

    for Q in (int(x) for x in args.queries.split(",")):
        q_lex, q_sem = rows_like_the_route(Q, 4, 12, 1, dev)
        q_cat = torch.cat([q_lex, q_sem], 1)
        s0 = torch.mm(q_cat, cat[0].T)
        run_s, run_r = torch.topk(s0, k, dim=1)
        share = float((torch.mm(q_cat, cat[1].T) > run_s[:, -1:]).float().mean())
        del s0

        def torch_add():
            s = torch.mm(q_cat, cat[1].T)
            top_s, top_r = torch.topk(s, k, dim=1)
            both_s, both_r = torch.cat([run_s, top_s], 1), torch.cat([run_r, top_r + n], 1)
            out_s, at = torch.topk(both_s, k, dim=1)
            return out_s, torch.gather(both_r, 1, at)

        def fused_add():
            """-> (ms of the add of chunk 1, the search)"""
            s = StreamSearch(q_lex, q_sem, k=k)
            s.add(*chunks[0])
            ms, _ = timed(lambda: s.add(*chunks[1]))
            return ms, s

        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        _, (t_s, t_r) = timed(torch_add)
        torch_ws = torch.cuda.max_memory_allocated() - base
        _, s = fused_add()
        f_s, f_r = s.result()
        fused_ws = s.device_bytes()
        images = 2 * ((Q + 127) // 128 * 128) * ((V + 127) // 128 * 128 + DS) * 2
        same = sum(len(np.intersect1d(a, b)) for a, b in zip(f_r.cpu().numpy(), t_r.cpu().numpy())) / float(Q * k)
        log("Q = %5d  answers: %.4f %% of the listed rows agree with the torch route, largest score difference %.3e" % (Q, 100 * same, float((f_s - t_s).abs().max())))
        s.close()
        del s, f_s, f_r, t_s, t_r
        rec = {"fused": [], "torch": []}
        for _ in range(args.reps):
            ms, s = fused_add()
            s.close()
            rec["fused"].append(ms)
            rec["torch"].append(timed(torch_add)[0])
        flop = 2.0 * Q * n * D
        for name, xs in rec.items():
            ms = np.array(xs)
            tf = flop / np.median(ms) / 1e9
            ws = "workspace %.0f MB (device_bytes; %.0f MB of it the two fp16 images of the queries)" % (fused_ws / 1e6, images / 1e6) if name == "fused" \
                else "workspace + outputs %.0f MB (allocator peak)" % (torch_ws / 1e6)
            log("Q = %5d  %s  ms per add median %9.3f [%9.3f, %9.3f] over %d calls  %.1f Tflop/s of the %.3g algorithmic flop (%.1f %% of %.0f = 2 500 / 3 for three "
                "fp16 products, %.1f %% of the %.0f of an fp32 MFMA)  %s" % (Q, name, np.median(ms), ms.min(), ms.max(), len(ms), tf, flop, 100 * tf / (PEAK_F16_DENSE / 3),
                                                                      PEAK_F16_DENSE / 3, 100 * tf / PEAK_F32_MFMA, PEAK_F32_MFMA, ws))
        log("Q = %5d  share of the chunk's scores above the running k-th entry: %.4f %%;  fused / torch: %.2f x (below 1: fused is faster)"
            % (Q, 100 * share, np.median(rec["fused"]) / np.median(rec["torch"])))
        del q_lex, q_sem, q_cat, run_s, run_r


if __name__ == "__main__":
    main()
