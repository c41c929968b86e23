#!/usr/bin/env python
"""What the search controller PLANS, pinned to the commit before the controller was rewritten around one search plan (search_plan.h):
the ranks the four exported rank queries report, the phase / row / flop / candidate counters of plain searches, and counters plus results of
the three staged call sequences on two half-corpus shards.  Everything recorded is an integer (flop counts are exactly representable sums of
integers; result arrays are recorded as SHA-256 digests of their bytes), so tests/test_controller_plan.py compares for equality.

Needs the GPU.  Run at the commit whose behaviour is to be pinned:   python tests/golden/make_golden_controller_plan.py
A run that finds tests/golden/controller_plan.json keeps only the fields that come out equal to the file's: run it twice.  What is known to
differ from build to build is not recorded in the first place (IMAGES below).  tests/test_controller_plan.py imports collect() from here."""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
PATH = os.path.join(HERE, "controller_plan.json")

D_DLR, D_CLS, NQ = 64, 8, 32
# rows -> [(DHR_PARAM_SAMPLE_PERIOD or None = default, DHR_PARAM_SAMPLE_SHARE, k)], the default period first (a handle keeps what was set)
RANK_CASES = {
    5_000: [(None, 1, 10), (None, 1, 100), (4, 2, 100)],
    40_000: [(None, 1, 10), (None, 1, 100), (None, 8, 1000), (4, 2, 100)],
    80_000: [(None, 1, 100), (None, 2, 1000), (4, 8, 100)],
    300_000: [(None, 1, 100), (None, 8, 1000), (4, 2, 100), (4, 8, 1000)],
}
# plain searches: (rows, period or None) -- unsampled, S = 4, the default period
STAT_CASES = [(5_000, None), (40_000, 4), (300_000, None)]
K_STATS = 100
GEOMETRY = ("phases", "gemm_rows", "gemm_flops", "gemm_flops_alg", "overflow_retries")
FALLBACKS = ("sample_fallback_queries",)
COUNTS = ("candidates_bound", "candidates_exact") + FALLBACKS
STAGED_ROWS, STAGED_K = 300_000, 100


def _pick(st, fields):
    return {f: int(st[f]) for f in fields}


def _digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _pair(n):
    from dhr_amd import synth
    cv, ci, qv, qi = synth.make_pair(7000 + n % 1000, n, NQ, D_DLR, D_CLS)
    return cv, ci, qv.astype(np.float32), qi


def collect_ranks(G, _lib):
    out = {}
    for n, cases in RANK_CASES.items():
        cv, ci, _, _ = _pair(n)
        ix = G.GipIndex(cv, ci)
        try:
            for period, share, k in cases:
                if period is not None:
                    ix.set_param(_lib.PARAM_SAMPLE_PERIOD, period)
                ix.set_param(_lib.PARAM_SAMPLE_SHARE, share)
                out["n%d_period%s_share%d_k%d" % (n, period or "default", share, k)] = {
                    "sample_rank": ix.sample_rank(k), "union_rank": ix.union_rank(k),
                    "mid_ranks": list(ix.mid_ranks(k)), "pre_ranks": list(ix.pre_ranks(k))}
        finally:
            ix.close()
    return out


# Two images of every index.  "default": what the library builds by default -- two index buckets per gated slice, dealt by a value-mass
# histogram that the build accumulates with floating-point atomics (idx_hist_kernel): the order of the additions, and with it a near-tie in
# the greedy deal, differs from build to build, so the BOUND of a row does, and with it how many rows pass the filter.  What such a search
# returns above its thresholds does not depend on that; its candidate counts, and the entries of a shard's list BELOW the agreed threshold, do.
# "one_bucket" (idx_buckets = 1: every index value in bucket 0, no histogram): the same controller over a bound that is the same in every
# build, so that the candidate counts are pinned too.  (Measured at the parent: four builds of the 40 000-row index gave 182 534 / 182 580 /
# 182 536 / 182 579 bound candidates on the default image -- the same in two searches of one build -- and 593 467 every time on this one.)
IMAGES = {"default": 0, "one_bucket": 1}
SERIAL_FIELDS = {"default": GEOMETRY + FALLBACKS, "one_bucket": GEOMETRY + COUNTS}      # what the serial configurations record per image


def collect_search_stats(G, _lib):
    out = {}
    for n, period in STAT_CASES:
        cv, ci, q, qi = _pair(n)
        for image, buckets in IMAGES.items():
            ix = G.GipIndex(cv, ci, idx_buckets=buckets)
            try:
                if period is not None:
                    ix.set_param(_lib.PARAM_SAMPLE_PERIOD, period)
                name = "n%d_period%s_%s" % (n, period or "default", image)
                ix.search(q, qi, K_STATS)
                out[name + "_overlapped"] = _pick(ix.stats(), GEOMETRY)
                ix.set_param(_lib.PARAM_OVERLAP_AUX, 0)
                ix.search(q, qi, K_STATS)
                out[name + "_serial"] = _pick(ix.stats(), SERIAL_FIELDS[image])
                ix.set_param(_lib.PARAM_ASYNC_CONTROLLER, 0)
                ix.search(q, qi, K_STATS)
                out[name + "_serial_host"] = _pick(ix.stats(), SERIAL_FIELDS[image])
            finally:
                ix.close()
    return out


def _determined(outs, tau, k):
    """What the shards' results DETERMINE whatever their bounds are worth: per shard the counts and the entries that reach the agreed
    threshold (a list is sorted, so those are its first count entries; below the threshold a list holds whatever passed the filter), and the
    merged top-k of the union where the counts say that it is complete."""
    scores = [o[0].cpu().numpy() for o in outs]
    rows = [o[1].cpu().numpy() for o in outs]
    counts = [o[2].cpu().numpy() for o in outs]
    t = tau.cpu().numpy()
    rec = {"count_sha256": [_digest(c) for c in counts], "scores_sha256": [], "rows_sha256": []}
    for s, r, c in zip(scores, rows, counts):
        assert all((s[i, :max(c[i], 0)] >= t[i]).all() and (c[i] < 0 or c[i] >= k or not (s[i, c[i]:] >= t[i]).any()) for i in range(len(c)))
        keep = np.arange(s.shape[1])[None, :] < np.minimum(np.maximum(c, 0), k)[:, None]
        rec["scores_sha256"].append(_digest(np.where(keep, s, np.float32(0))))
        rec["rows_sha256"].append(_digest(np.where(keep, r, np.int64(-1))))
    total = sum(np.maximum(c, 0) for c in counts)
    complete = (total >= k) & np.all([c >= 0 for c in counts], axis=0)
    ms, mr = np.concatenate(scores, 1), np.concatenate(rows, 1)
    order = np.lexsort((mr, -ms.astype(np.float64)), axis=1)[:, :k]
    ms, mr = np.take_along_axis(ms, order, 1), np.take_along_axis(mr, order, 1)
    rec["complete_queries"] = int(complete.sum())
    rec["merged_scores_sha256"] = _digest(ms[complete])
    rec["merged_rows_sha256"] = _digest(mr[complete])
    return rec


def collect_staged(G, _lib):
    """begin -> finish, begin -> mid -> finish, pre -> begin_rest -> finish on two half-corpus handles (share 2, period 4), the collectives
    replaced by in-process tensor operations; counters summed over the shards, of the results what _determined keeps."""
    import torch
    from dhr_amd import dist as D
    cv, ci, q, qi = _pair(STAGED_ROWS)
    k, ns = STAGED_K, 2
    out = {}
    for image, buckets in IMAGES.items():
        shards = []
        try:
            for sh in range(ns):
                lo, hi = G.shard_bounds(STAGED_ROWS, ns, sh)
                shards.append(G.GipIndex(cv[lo:hi], ci[lo:hi], row_offset=lo, idx_buckets=buckets))
                shards[-1].set_param(_lib.PARAM_SAMPLE_PERIOD, 4)
                shards[-1].set_param(_lib.PARAM_SAMPLE_SHARE, ns)
                shards[-1].set_param(_lib.PARAM_OVERLAP_AUX, 0)
            for config in ("serial", "serial_host"):
                if config == "serial_host":
                    for s in shards:
                        s.set_param(_lib.PARAM_ASYNC_CONTROLLER, 0)
                ru = shards[0].union_rank(k)
                mid = [s.mid_ranks(k) for s in shards]
                pre = [s.pre_ranks(k) for s in shards]
                assert ru > 0 and all(a > 0 for a, _ in mid) and all(a > 0 for a, _ in pre), (ru, mid, pre)
                for seq in ("begin_finish", "begin_mid_finish", "pre_rest_finish"):
                    if seq == "pre_rest_finish":
                        rl, rup = max(a for a, _ in pre), max(b for _, b in pre)
                        firsts = [s.search_pre(q, qi, k, rl) for s in shards]
                        tau0 = D.common_threshold(torch.stack(firsts), min(rup, ns * rl))
                        samples = [s.search_begin_rest(tau0) for s in shards]
                    else:
                        samples = [s.search_begin(q, qi, k) for s in shards]
                    tau = D.common_threshold(torch.stack(samples), ru)
                    if seq == "begin_mid_finish":
                        rl, rum = max(a for a, _ in mid), max(b for _, b in mid)
                        seen = [s.search_mid(tau, rl) for s in shards]
                        tau = torch.maximum(tau, D.common_threshold(torch.stack(seen), min(rum, ns * rl)))
                    outs = [s.search_finish(tau) for s in shards]
                    stats = [s.stats() for s in shards]
                    rec = {f: int(sum(st[f] for st in stats)) for f in SERIAL_FIELDS[image]}
                    rec["tau_sha256"] = _digest(tau.cpu().numpy())
                    rec.update(_determined(outs, tau, k))
                    out["%s_%s_%s" % (image, config, seq)] = rec
        finally:
            for s in shards:
                s.close()
    return out


def collect():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from dhr_amd import _lib
    from dhr_amd.retrieval import gip_retrieval as G
    _lib.load()
    return {"ranks": collect_ranks(G, _lib), "search_stats": collect_search_stats(G, _lib), "staged": collect_staged(G, _lib)}


def keep_equal(a, b):
    """the fields of a that b holds with the same value (nested dicts)"""
    out = {}
    for key, va in a.items():
        if key not in b:
            continue
        if isinstance(va, dict):
            out[key] = keep_equal(va, b[key])
        elif va == b[key]:
            out[key] = va
    return out


def main():
    got = collect()
    ranks = got["ranks"].values()
    for what in ("mid_ranks", "pre_ranks"):          # the set must show the step both present and absent
        assert sum(1 for r in ranks if r[what][0] > 0) >= 2 and sum(1 for r in ranks if r[what][0] == 0) >= 2, what
    if os.path.exists(PATH):
        with open(PATH) as f:
            before = json.load(f)
        kept = keep_equal(got, before)
        print("fields that differ from the file (dropped):", json.dumps({k: [f for f in got[k] if got[k][f] != kept.get(k, {}).get(f)] for k in got}))
        got = kept
    with open(PATH, "w") as f:
        json.dump(got, f, indent=1, sort_keys=True)
        f.write("\n")
    print(os.path.getsize(PATH), "bytes")


if __name__ == "__main__":
    main()
