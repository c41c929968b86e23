"""The running top-k merge at the end of every search phase, key by key, on all four paths of launch_select (dhr_debug_select_merge: a SelectArgs
filled from the arguments and handed to the searches' own launcher):

  kp <= 1024          select_kernel<4>       LDS: the list + one round of `room` new keys, bitonic sort of the round, merge by rank
  kp <= 4096          select_kernel<16>      the same with 16 list entries per thread
  kp <= 16384         select_big_kernel      in place in global memory, rounds of 2048 new keys, the list swept tile by tile from its tail
  kp >  16384         launch_select_global   [list | new keys] through one segmented radix sort

The reference is plain numpy in this file and shares no code with the library: per query the non-zero keys of slots [0, keep) plus the first
min(cnt, cap) input keys (count_all without cnt), sorted descending as uint64; the first keep = k_keep or k of them are the expected list, zeros
behind the last; tau = score of slot k - 1, -inf while it is empty, max(old tau, that) with monotone; thr = tau - margin in float32.  Slots
[0, keep), tau and thr are compared BIT FOR BIT: no tolerance anywhere.  What stands past keep is asserted per path (SelectArgs, dhr_internal.h).

The key encoding is restated here (keys_of / score_of); test_key_order_is_the_librarys_tie_rule (CPU) holds it against dhr_merge_topk_host, so
that a wrong restatement cannot agree with itself.  Scores come from a grid of 12 values, so a query holds hundreds of exact ties at different
rows; rows are scattered over [0, 2^32 - 1) and distinct, which keeps the keys unique.  Each case prints "[select_merge] ..." with what it ran."""
import numpy as np
import pytest

KPS_OF_PATH = {"select_kernel<4>": (64, 1024), "select_kernel<16>": (2048, 4096), "select_big_kernel": (8192, 16384), "select_global": (32768,)}
ALL_KP = [kp for kps in KPS_OF_PATH.values() for kp in kps]
ODD_K = {64: 37, 1024: 1000, 2048: 1500, 4096: 4000, 8192: 5000, 16384: 10000, 32768: 20000}      # not a power of two, past the half of kp
GRID = np.array([-np.inf, -7.5, -1.25, -2.0 ** -140, -0.0, 0.0, 2.0 ** -140, 0.5, 1.0, 1.0 + 2.0 ** -23, 3.0e38, np.inf], np.float32)
SELECT_BIG_BATCH = 2048                      # new keys per round of select_big_kernel (kernels.hip)
U32 = np.uint64(0xFFFFFFFF)


def path_of(kp):
    return next(name for name, kps in KPS_OF_PATH.items() if kp in kps)


def kp_id(kp):
    return "%s-kp%d" % (path_of(kp), kp)


# ------------------------------------------------------------------------------------------------ the key, restated
def ordered_of(scores):
    """fp32 -> u32, order preserving: a non-negative score gets its sign bit set, a negative one every bit flipped; both zeros -> 0x80000000"""
    u = np.ascontiguousarray(scores, np.float32).view(np.uint32)
    o = np.where(u >> np.uint32(31), ~u, u | np.uint32(0x80000000))
    return np.where((u << np.uint32(1)) == 0, np.uint32(0x80000000), o).astype(np.uint32)


def keys_of(scores, rows):
    """make_key: score image in the high word, 0xFFFFFFFF - row in the low one (equal scores order by ascending row); rows < 2^32 - 1"""
    return (ordered_of(scores).astype(np.uint64) << np.uint64(32)) | (U32 - np.asarray(rows).astype(np.uint64))


def score_of(keys):
    o = (np.asarray(keys, np.uint64) >> np.uint64(32)).astype(np.uint32)
    return np.where(o >> np.uint32(31), o & np.uint32(0x7FFFFFFF), ~o).astype(np.uint32).view(np.float32)


def test_key_order_is_the_librarys_tie_rule():
    """(score, row) pairs sorted by the numpy keys come out in the order of dhr_merge_topk_host (score descending, row ascending; +0.0 and
    -0.0 tie): ties, both zeros, negative scores and both infinities in the input"""
    from dhr_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(4101)
    nq, n = 3, 400
    scores = GRID[rng.integers(0, len(GRID), (nq, n))]
    scores[:, :len(GRID)] = GRID                                    # every grid value in every query, each many times over
    rows = (np.stack([rng.permutation(n) for _ in range(nq)]).astype(np.int64) + 1) * 10737418 + np.arange(nq)[:, None]      # distinct, up to 2^32 - 96
    rows[0, 0], rows[0, 1] = 0, 2 ** 32 - 2                           # ... and both ends of the row range
    assert rows.max() < 2 ** 32 - 1 and all(len(set(r)) == n for r in rows.tolist())
    keys = keys_of(scores, rows)
    assert all(len(set(k)) == n for k in keys.tolist()) and keys.min() > 0
    assert np.array_equal(score_of(keys), scores) and np.array_equal(U32 - (keys & U32), rows.astype(np.uint64))      # (== : the zeros tie)
    assert score_of(keys_of(np.float32([-0.0]), [5])).view(np.uint32)[0] == 0       # a zero comes back as +0.0
    order = np.argsort(keys, axis=1)[:, ::-1]
    for k in (1, 37, n):
        out_s, out_r = np.full((nq, k), 9.0, np.float32), np.full((nq, k), 9, np.int64)
        assert lib.dhr_merge_topk_host(nq, n, scores.ctypes.data, rows.ctypes.data, k, out_s.ctypes.data, out_r.ctypes.data) == 0
        assert np.array_equal(out_r, np.take_along_axis(rows, order, 1)[:, :k])
        assert np.array_equal(out_s, np.take_along_axis(scores, order, 1)[:, :k])
    tied = np.take_along_axis(scores, order, 1)
    assert (tied[:, 1:] == tied[:, :-1]).sum() > nq * n // 2          # the input is mostly ties


def test_the_hook_is_declared_exported_and_bound():
    import os
    from dhr_amd import _lib
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "dhr_hip.h")).read()
    name = "dhr_debug_select_merge"
    assert name + "(" in header and name in _lib.EXPORTS and hasattr(_lib.load(), name)
    assert len(_lib.load().dhr_debug_select_merge.argtypes) == 18


# ------------------------------------------------------------------------------------------------ the reference
def sort_desc(keys):
    return np.sort(keys, axis=1)[:, ::-1]


def reference(lists_keep, in_keys, counts, k, monotone, tau_old, margin):
    """-> (expected slots [0, keep) [nq, keep] u64, tau [nq] f32, thr [nq] f32)"""
    keep = lists_keep.shape[1]
    taken = np.where(np.arange(in_keys.shape[1])[None, :] < np.asarray(counts)[:, None], in_keys, np.uint64(0))
    want = sort_desc(np.concatenate([lists_keep, taken], axis=1))[:, :keep]
    kth = want[:, k - 1]
    tau = np.where(kth != 0, score_of(kth), np.float32(-np.inf)).astype(np.float32)
    if monotone:
        assert not np.any((tau == 0) & (tau_old == 0))            # (the maximum of two zeros of different sign is not pinned)
        tau = np.maximum(tau_old, tau)
    with np.errstate(invalid="raise", over="ignore"):         # (-3e38 - 3e38 = -inf is wanted; a NaN would be a mistake of the case)
        thr = tau.astype(np.float32) - margin.astype(np.float32)   # float32 - float32: one rounding, in float32
    return want, tau, thr


def room_of(sort_n, kps):
    """new keys per round of select_kernel, recomputed from its arguments: the largest power of two that fits behind the kps list slots in
    sort_n keys of LDS, between 64 and 2048"""
    room = 64
    while room * 2 <= sort_n - kps and room < 2048:
        room *= 2
    return room


def round_of(kp, sort_n, kps):
    return room_of(sort_n, kps) if kp <= 4096 else SELECT_BIG_BATCH          # (the global path has no rounds: the in-place kernel's size serves)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------ inputs
def draw_keys(rng, nq, n, grid=GRID):
    """[nq, n] unique keys: scores from the grid, rows distinct over the whole array and scattered over [0, 2^32 - 1)"""
    rows = np.unique(rng.integers(0, 2 ** 32 - 1, size=nq * n + nq * n // 8 + 64, dtype=np.uint64))
    assert len(rows) >= nq * n
    rows = rng.permutation(rows)[:nq * n].reshape(nq, n)
    return keys_of(grid[rng.integers(0, len(grid), (nq, n))], rows)


def list_of(keys, kp, fill):
    """[nq, kp] running lists: the `fill[q]` greatest of keys[q] (all of them where fill is None), sorted, zeros behind"""
    nq = keys.shape[0]
    out = np.zeros((nq, kp), np.uint64)
    s = sort_desc(keys)
    for q in range(nq):
        f = s.shape[1] if fill is None else int(fill[q])
        out[q, :f] = s[q, :f]
    return out


class Lists:
    """running lists, tau, thr and margin of one launch geometry on the device; merge() makes one call and checks everything it left behind"""

    def __init__(self, kp, lists, margin, tau=None, thr=None):
        import torch
        from dhr_amd import _lib
        self.lib, self._lib, self.torch = _lib.load(), _lib, torch
        self.kp, self.nq = kp, lists.shape[0]
        assert lists.shape == (self.nq, kp) and lists.dtype == np.uint64 and self.nq <= 64
        self.path = path_of(kp)
        self.d_list = torch.from_numpy(lists.view(np.int64).copy()).cuda()
        self.h_list = lists.copy()
        self.tau = np.full(self.nq, -np.inf, np.float32) if tau is None else np.asarray(tau, np.float32).copy()
        self.thr = np.full(self.nq, 7.0, np.float32) if thr is None else np.asarray(thr, np.float32).copy()       # thr is output only: 7.0 must not survive
        self.margin = np.asarray(margin, np.float32).copy()
        self.d_tau, self.d_thr, self.d_margin = (torch.from_numpy(a.copy()).cuda() for a in (self.tau, self.thr, self.margin))
        self.calls = 0

    def merge(self, in_keys, k, k_keep=0, kps=None, sort_n=None, monotone=0, cnt=None, count_all=0, cap=None, tail_rule=True):
        torch = self.torch
        kp, nq = self.kp, self.nq
        kps = kp if kps is None else kps
        sort_n = 2 * kp if sort_n is None else sort_n
        keep = k_keep or k
        ld = in_keys.shape[1]
        assert in_keys.shape[0] == nq and ld <= 32768 and in_keys.dtype == np.uint64
        cap = ld if cap is None else cap
        d_in = torch.from_numpy(in_keys.view(np.int64).copy()).cuda()
        d_cnt = None if cnt is None else torch.from_numpy(np.asarray(cnt, np.int64).astype(np.uint32).view(np.int32).copy()).cuda()
        rc = self.lib.dhr_debug_select_merge(0, nq, k, k_keep, kp, kps, sort_n, monotone, self.d_list.data_ptr(), d_in.data_ptr(), ld,
                                             None if d_cnt is None else d_cnt.data_ptr(), count_all, cap, self.d_margin.data_ptr(), self.d_tau.data_ptr(),
                                             self.d_thr.data_ptr(), None)
        self._lib.check(rc, "dhr_debug_select_merge")
        self.calls += 1
        got = self.d_list.cpu().numpy().view(np.uint64)
        got_tau, got_thr = self.d_tau.cpu().numpy(), self.d_thr.cpu().numpy()
        counts = np.full(nq, count_all, np.int64) if cnt is None else np.minimum(np.asarray(cnt, np.int64), cap)
        before = self.h_list
        want, tau, thr = reference(before[:, :keep], in_keys, counts, k, monotone, self.tau, self.margin)
        where = "%s kp %d call %d" % (self.path, kp, self.calls)
        bad = np.flatnonzero((got[:, :keep] != want).any(axis=1))
        assert bad.size == 0, "%s: slots [0, %d) differ for queries %s (counts %s); query %d first at slot %d" % (
            where, keep, bad.tolist(), counts[bad].tolist(), bad[0], int(np.flatnonzero(got[bad[0], :keep] != want[bad[0]])[0]))
        assert np.array_equal(bits(got_tau), bits(tau)), "%s: tau %s, expected %s" % (where, got_tau.tolist(), tau.tolist())
        assert np.array_equal(bits(got_thr), bits(thr)), "%s: thr %s, expected %s" % (where, got_thr.tolist(), thr.tolist())
        # slots [keep, kp): nobody's input, defined per path
        if kp <= 4096:
            assert not got[:, keep:kps].any(), where + ": the LDS kernels zero slots [keep, kps)"
            assert np.array_equal(got[:, kps:], before[:, kps:]), where + ": the LDS kernels leave slots [kps, kp) alone"
        elif kp <= 16384:
            assert np.array_equal(got[:, keep:], before[:, keep:]), where + ": the in-place kernel leaves slots [keep, kp) alone"
        else:
            taken = np.where(np.arange(ld)[None, :] < counts[:, None], in_keys, np.uint64(0))
            assert np.array_equal(got, sort_desc(np.concatenate([before, taken], axis=1))[:, :kp]), where + ": the global path keeps the next-best keys in [keep, kp)"
        if tail_rule and keep < kp:
            assert (got[:, keep:].max(axis=1) <= got[:, keep - 1]).all(), where + ": a key past keep beats slot keep - 1"
        self.h_list, self.tau, self.thr = got, tau, thr
        return got, tau, thr


def fills_of(states, k):
    return [{"empty": 0, "part": k // 3, "full": k}[s] for s in states]


# ------------------------------------------------------------------------------------------------ the rounds
def _rounds_case(kp, k, sort_n, use_cnt, seed):
    """one launch mixes counts around the round size with the three list states; the same through count_all, one launch per count"""
    rng = np.random.default_rng(seed)
    kps = kp
    R = round_of(kp, sort_n, kps)
    cap = 4 * R
    ld = cap + 64
    counts = [0, 1, R - 1, R, R + 1, 2 * R, 3 * R + 5, cap, cap + 7]          # the last one is clamped to cap
    states = ["empty", "part", "full"]
    margin_pool = np.float32([0.0, 0.25, 1.0e-3, 1.0e30])
    if use_cnt:
        cnt = np.repeat(counts, len(states))
        fill = fills_of(states * len(counts), k)
    else:
        cnt, fill = None, fills_of(states, k)
    nq = len(fill)
    pool = draw_keys(rng, nq, k + ld)
    lists = list_of(pool[:, :k], kp, fill)
    in_keys = pool[:, k:].copy()
    # behind cap: keys that would win if they were read (+inf at low rows); in front of it every slot holds a live key, so a count read too
    # long shows as well
    in_keys[:, cap:] = keys_of(np.full((nq, 64), np.inf, np.float32), np.arange(nq * 64).reshape(nq, 64))
    L = Lists(kp, lists, margin_pool[np.arange(nq) % len(margin_pool)])
    if use_cnt:
        L.merge(in_keys, k, kps=kps, sort_n=sort_n, cnt=cnt, cap=cap)
    else:
        for c in counts[:-1]:
            L = Lists(kp, lists, margin_pool[np.arange(nq) % len(margin_pool)])
            L.merge(in_keys, k, kps=kps, sort_n=sort_n, count_all=c, cap=cap)
    print("[select_merge] %s kp %d k %d sort_n %d: round size %d (recomputed from sort_n and kps on the LDS paths), counts %s, %s, %d queries" % (
        path_of(kp), kp, k, sort_n, R, counts, "cnt per query" if use_cnt else "count_all", nq))


ROUNDS = [pytest.param(kp, k_kind, budget, source, id="%s-%s-sort_n%dkp-%s" % (kp_id(kp), k_kind, budget, source))
          for kp in ALL_KP for k_kind in ("k1", "k_odd", "k_kp") for budget in ((2, 4) if kp <= 4096 else (2,))      # sort_n is an argument of the LDS kernels only
          for source in ("cnt", "count_all")]


@pytest.mark.gpu
@pytest.mark.parametrize("kp,k_kind,budget,source", ROUNDS)
def test_rounds_and_list_states(kp, k_kind, budget, source):
    """k = 1, a k that is no power of two and k = kp; empty, part-filled (k / 3) and full lists; 0, 1, one below / at / one above the round
    size, several rounds, cap and cnt > cap with sentinel keys behind cap; both LDS budgets (2 kp: the searches, 4 kp: the PQ search)"""
    k = {"k1": 1, "k_odd": ODD_K[kp], "k_kp": kp}[k_kind]
    _rounds_case(kp, k, budget * kp, source == "cnt", seed=kp + k + budget)


# ------------------------------------------------------------------------------------------------ kps < kp
@pytest.mark.gpu
@pytest.mark.parametrize("budget", [2, 4])
@pytest.mark.parametrize("kp,kps,k,k_keep", [(1024, 128, 100, 0), (1024, 256, 37, 200), (2048, 128, 100, 0), (4096, 1024, 37, 1000), (4096, 64, 64, 0)])
def test_live_prefix_shorter_than_the_list(kp, kps, k, k_keep, budget):
    """kps < kp on both select_kernel instantiations (a sampled run sizes the LDS sort by k, not by the list): three calls on the same lists;
    slots [kps, kp) hold keys of their own that no call may touch -- or read: they would win"""
    rng = np.random.default_rng(kp + kps + budget)
    sort_n = budget * kp
    R = room_of(sort_n, kps)
    keep = k_keep or k
    nq, ld = 8, 3 * R + 5
    counts = np.array([0, 1, R - 1, R, R + 1, 3 * R + 5, 2 * R, min(keep, ld)])
    pool = draw_keys(rng, nq, keep + 3 * ld)
    lists = list_of(pool[:, :keep], kp, fills_of(["empty", "part", "full", "part"] * 2, keep))
    lists[:, kps:] = keys_of(np.full((nq, kp - kps), np.inf, np.float32), np.arange(nq * (kp - kps)).reshape(nq, -1))
    L = Lists(kp, lists, np.full(nq, 0.125, np.float32))
    for call in range(3):
        L.merge(np.ascontiguousarray(pool[:, keep + call * ld:keep + (call + 1) * ld]), k, k_keep=k_keep, kps=kps, sort_n=sort_n, cnt=np.roll(counts, call), tail_rule=False)
        assert np.array_equal(L.h_list[:, kps:], lists[:, kps:])
    print("[select_merge] %s kp %d kps %d k %d keep %d sort_n %d: round size %d, 3 calls" % (path_of(kp), kp, kps, k, keep, sort_n, R))


# ------------------------------------------------------------------------------------------------ feed sequences
@pytest.mark.gpu
@pytest.mark.parametrize("order", ["ascending", "descending", "random"])
@pytest.mark.parametrize("kp", ALL_KP, ids=kp_id)
def test_feed_sequences(kp, order):
    """four calls on the same lists, the state checked after every call: ascending by key (every key enters, the whole list shifts, and the
    list runs full on the way), descending (nothing enters once the list is full), random"""
    rng = np.random.default_rng(kp + len(order))
    k, calls, nq = ODD_K[kp], 4, 6
    per_call = min(kp, 8192) + 77                # several rounds on every path; 4 calls bring more than kp keys
    pool = draw_keys(rng, nq, calls * per_call)
    if order == "ascending":
        pool = np.sort(pool, axis=1)
    elif order == "descending":
        pool = sort_desc(pool)
    L = Lists(kp, np.zeros((nq, kp), np.uint64), np.linspace(0.0, 2.0, nq).astype(np.float32))
    entered = []
    for c in range(calls):
        before = L.h_list[:, :k].copy()
        got, _, _ = L.merge(np.ascontiguousarray(pool[:, c * per_call:(c + 1) * per_call]), k, cnt=np.full(nq, per_call))
        entered.append(int((~np.isin(got[0, :k], before[0])).sum()))
    if order == "ascending":
        assert entered == [min(k, per_call)] * calls
    if order == "descending":
        assert entered[0] == min(k, per_call) and entered[-1] == max(0, min(per_call, k - (calls - 1) * per_call))
    print("[select_merge] %s kp %d k %d %s feed: %d keys per call, keys of query 0 that entered per call %s" % (path_of(kp), kp, k, order, per_call, entered))


# ------------------------------------------------------------------------------------------------ sampled-run arguments
@pytest.mark.gpu
@pytest.mark.parametrize("monotone", [1, 0])
@pytest.mark.parametrize("kp", ALL_KP, ids=kp_id)
def test_sampled_run_arguments(kp, monotone):
    """k = 37 of k_keep = 1000 (scaled with kp): the threshold rank is not the list length.  Old tau above the new k-th score for half of the
    queries: with monotone it stands, without it tau follows the list; the list keeps k_keep keys either way"""
    rng = np.random.default_rng(kp + monotone)
    keep = ODD_K[kp]
    k = max(3, keep * 37 // 1000)
    nq, n = 8, min(keep + keep // 2 + 11, 32768)
    finite = GRID[1:-1]
    tau_old = np.where(np.arange(nq) % 2 == 0, np.float32(2.0e38), np.float32(-3.0)).astype(np.float32)      # above / below every k-th score below
    L = Lists(kp, np.zeros((nq, kp), np.uint64), np.full(nq, 0.5, np.float32), tau=tau_old)
    pool = draw_keys(rng, nq, 2 * n, grid=finite[:-1])          # scores up to 1 + 2^-23: far below 2e38
    for call in range(2):
        keys = np.ascontiguousarray(pool[:, call * n:(call + 1) * n])
        got, tau, _ = L.merge(keys, k, k_keep=keep, monotone=monotone, cnt=np.full(nq, n))
        assert (got[:, keep - 1] != 0).all() and (got[:, k - 1] != 0).all()        # the list holds keep keys, not k
        kth = score_of(got[:, k - 1])
        if monotone:
            assert np.array_equal(bits(tau[0::2]), bits(tau_old[0::2])) and np.array_equal(bits(tau[1::2]), bits(kth[1::2]))
        else:
            assert np.array_equal(bits(tau), bits(kth)) and (tau[0::2] < tau_old[0::2]).all()
    print("[select_merge] %s kp %d k %d k_keep %d monotone %d: 2 calls of %d keys" % (path_of(kp), kp, k, keep, monotone, n))


# ------------------------------------------------------------------------------------------------ threshold arithmetic
@pytest.mark.gpu
@pytest.mark.parametrize("kp", ALL_KP, ids=kp_id)
def test_threshold_arithmetic(kp):
    """the score at rank k chosen per query (+0.0, -0.0, the smallest denormals, negative, huge) inside a run of ties, against margins that are
    zero, tiny, larger than |tau| and large enough to overflow; an under-full list publishes -inf - margin = -inf"""
    rng = np.random.default_rng(kp)
    k = ODD_K[kp]
    at_rank = np.float32([0.0, -0.0, 2.0 ** -149, -2.0 ** -149, -1.25, -7.5, 1.0 + 2.0 ** -23, 3.0e38, -3.0e38, 0.5, 0.5, 0.5])
    margin = np.float32([0.5, 0.5, 2.0 ** -149, 0.0, 100.0, 1.0e-3, 2.0 ** -24, 3.0e38, 3.0e38, 0.75, 1.0e-9, 0.5])
    nq, ties = len(at_rank), 9
    under_full = nq - 1                                              # the last query keeps fewer than k keys
    n = k + 40
    rows = np.unique(rng.integers(0, 2 ** 32 - 1, size=2 * nq * n, dtype=np.uint64))
    rows = rng.permutation(rows)[:nq * n].reshape(nq, n)
    scores = np.empty((nq, n), np.float32)
    for q in range(nq):
        above = np.nextafter(at_rank[q], np.float32(np.inf), dtype=np.float32) if at_rank[q] != 0 else np.float32(2.0 ** -149)
        below = np.nextafter(at_rank[q], np.float32(-np.inf), dtype=np.float32) if at_rank[q] != 0 else np.float32(-2.0 ** -149)
        hi = k - 1 - ties // 2                                        # keys that beat the run of ties: rank k lies inside the run
        scores[q, :hi] = np.where(rng.integers(0, 2, hi) == 1, above, np.float32(np.inf))
        scores[q, hi:hi + ties] = at_rank[q]
        scores[q, hi + ties:] = np.where(rng.integers(0, 2, n - hi - ties) == 1, below, np.float32(-np.inf))
    if at_rank[0] == 0:
        scores[0, k - 1 - ties // 2:k - 1 - ties // 2 + ties:2] = -0.0       # query 0: the run mixes both zeros
    keys = keys_of(scores, rows)
    keys = np.take_along_axis(keys, np.stack([rng.permutation(n) for _ in range(nq)]), 1)
    cnt = np.full(nq, n)
    cnt[under_full] = k - 1
    L = Lists(kp, np.zeros((nq, kp), np.uint64), margin, tau=np.full(nq, 5.0, np.float32))
    _, tau, thr = L.merge(keys, k, cnt=cnt)
    want_tau = np.where(at_rank == 0, np.float32(0.0), at_rank).astype(np.float32)
    want_tau[under_full] = -np.inf
    assert np.array_equal(bits(tau), bits(want_tau))
    assert np.isneginf(thr[under_full]) and thr[7] == 0.0 and np.isneginf(thr[8]) and thr[4] == np.float32(-101.25)
    print("[select_merge] %s kp %d k %d: tau %s thr %s" % (path_of(kp), kp, k, tau.tolist(), thr.tolist()))


# ------------------------------------------------------------------------------------------------ the rank switch
@pytest.mark.gpu
@pytest.mark.parametrize("kp", ALL_KP, ids=kp_id)
def test_rank_switch_on_an_under_full_list(kp):
    """The state behind a sampled run at a lower rank: fewer than k keys in the list, a finite tau and thr.  main_pass switches to rank k with
    monotone = 0; a batch that leaves the list under-full must publish tau = thr = -inf on every path (SelectArgs: the LDS and in-place kernels
    always did, the global path kept the sampled values until this test).  What the controller needs is only that thr never exceeds a valid
    threshold: raise_thr_main_kernel takes max(thr_hat, thr) and thr_hat starts from the sampled thr, so -inf means "no news".  With monotone
    the old tau stands, as in the sampled run itself."""
    rng = np.random.default_rng(kp)
    k = ODD_K[kp]
    r = max(2, k // 8)                                               # the sampled rank: the list holds r + 3 < k keys
    nq, have, more = 4, r + 3, max(1, (k - r - 3) // 2)
    assert have + more < k
    pool = draw_keys(rng, nq, have + more + k, grid=GRID[1:-1])
    lists = list_of(pool[:, :have], kp, None)
    tau_s = score_of(lists[:, r - 1])                                # what the sampled run published: the r-th best
    margin = np.full(nq, 0.25, np.float32)
    for monotone in (0, 1):
        L = Lists(kp, lists, margin, tau=tau_s, thr=tau_s - margin)
        got, tau, thr = L.merge(np.ascontiguousarray(pool[:, have:have + more]), k, monotone=monotone, cnt=np.full(nq, more))
        assert (got[:, have + more - 1] != 0).all() and not got[:, have + more:k].any()
        if monotone:
            assert np.array_equal(bits(tau), bits(tau_s)) and np.array_equal(bits(thr), bits(tau_s - margin))
        else:
            assert np.isneginf(tau).all() and np.isneginf(thr).all()
    # ... and the batch that fills slot k - 1 publishes its score
    L = Lists(kp, lists, margin, tau=tau_s, thr=tau_s - margin)
    got, tau, _ = L.merge(np.ascontiguousarray(pool[:, have + more:]), k, cnt=np.full(nq, k))
    assert np.array_equal(bits(tau), bits(score_of(got[:, k - 1]))) and np.isfinite(tau).all()
    print("[select_merge] %s kp %d: %d keys at the sampled rank %d, %d more, k %d: tau -inf, thr -inf (monotone: kept)" % (path_of(kp), kp, have, r, more, k))
