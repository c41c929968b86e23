"""The bounds of the filter levels BEHIND the bound GEMM, pair by pair, against float64 scores (dhr_debug_refine_bounds: the bound GEMM into
the candidate lists, then launch_refine on those lists, both lists scattered into dense [Q, n] arrays; NaN = the row is not in that list).

The search is exact only if every level keeps an upper bound of the exact score.  End to end a bound that is slightly too low hides behind
thresholds that are lower estimates of the final one, and `candidates_exact` cannot tell which entry a level lost; here every pair is checked:

  3a  safety and monotonicity      exact_f64 - margin_q <= U2 <= U for every pair, the list U == the GEMM's dump bit for bit
  3b  collapse on short rows       a row whose non-zero gated values all fit its record, under ONE bucket: U2 comes down to the exact score
  3c  restatement                  U - U2 == oracle/refine_oracle.py, given the device's U (and, int8 image, its unit)
  3d  survivor sets                finite thresholds, grid and flat launches: exactly {row of the GEMM list : U2 >= thr}, ties included
  3e  residual level               dense-only int8 indexes, all four instantiations of dense_refine_kernel

Margins come from dhr_debug_query_margins, exact scores from oracle.gip_oracle.gip_scores_f64; every other tolerance is derived where it is
used.  Each case prints its minimum head room and the largest observed value of every toleranced quantity ("[refine_bounds] ..." lines;
profiles/refine_bounds.txt keeps those of one run on an MI355X).  Corpora: tests/refine_cases.py (their conditions: tests/test_refine_oracle.py)."""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import gip_oracle as O
from oracle import refine_oracle as R
from tests import refine_cases as RC

pytestmark = pytest.mark.gpu

N, Q = RC.N, RC.Q            # 1500 rows = three refine workgroups of 512 with a partial last one, whose last round of 64 is not full


# ------------------------------------------------------------------------------------------------ the hooks
def _index(cv, ci, **kw):
    from dhr_amd.retrieval.gip_retrieval import GipIndex
    return GipIndex(cv, ci, **kw)


def _batch(qv, qi):
    from dhr_amd import _lib
    return _lib.make_query_batch(np.ascontiguousarray(qv, np.float32), None if qi is None else np.ascontiguousarray(qi))


def _refine(ix, qv, qi, n, tau=None, flat=0):
    """-> (U [Q, n], U2 [Q, n], thr [Q], unit [Q]) as float64 / float32 numpy arrays (U, U2 keep their float32 values exactly)."""
    import torch
    from dhr_amd import _lib
    qb, keep = _batch(qv, qi)
    nq = qv.shape[0]
    u = torch.zeros((nq, n), dtype=torch.float32, device="cuda")
    u2 = torch.zeros((nq, n), dtype=torch.float32, device="cuda")
    thr, unit = np.zeros(nq, np.float32), np.zeros(nq, np.float32)
    tau32 = None if tau is None else np.ascontiguousarray(tau, np.float32)
    _lib.check(ix._lib.dhr_debug_refine_bounds(ix._h, C.byref(qb), 0, n, None if tau32 is None else tau32.ctypes.data, flat, u.data_ptr(), u2.data_ptr(),
                                               thr.ctypes.data, unit.ctypes.data, None), "dhr_debug_refine_bounds")
    del keep
    return u.cpu().numpy(), u2.cpu().numpy(), thr, unit


def _dump(ix, qv, qi, n):
    import torch
    from dhr_amd import _lib
    qb, keep = _batch(qv, qi)
    out = torch.zeros((qv.shape[0], n), dtype=torch.float32, device="cuda")
    _lib.check(ix._lib.dhr_debug_bound_scores(ix._h, C.byref(qb), 0, n, out.data_ptr(), None), "dhr_debug_bound_scores")
    del keep
    return out.cpu().numpy()


def _margins(ix, qv, qi):
    from dhr_amd import _lib
    qb, keep = _batch(qv, qi)
    m = np.zeros(qv.shape[0], np.float32)
    _lib.check(ix._lib.dhr_debug_query_margins(ix._h, C.byref(qb), m.ctypes.data, None), "dhr_debug_query_margins")
    del keep
    return m.astype(np.float64)


def _exact(cv, ci, qv, qi):
    c32 = cv.astype(np.float32)
    return np.stack([O.gip_scores_f64(qv[q], None if qi is None else qi[q], c32, None if qi is None else ci) for q in range(qv.shape[0])])


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _image_is(ix, gated_image):
    from dhr_amd import _lib
    assert ix.info(_lib.INFO_GATED_I8) == (1 if gated_image == "gated_i8" else 0)


# ------------------------------------------------------------------------------------------------ 3a
@functools.lru_cache(maxsize=None)
def _case(name):
    """-> (cv, ci, qv fp32, qi or None, idx_buckets)"""
    from dhr_amd import synth

    def synth_pair(seed, n, d_dlr, d_cls):
        cv, ci, qv, qi = synth.make_pair(seed, n, Q, d_dlr, d_cls)
        return cv, ci, RC.adversarial_queries(qv, d_dlr), qi.astype(np.int16)

    if name == "synth_768_64":
        return synth_pair(5101, N, 768, 64) + (0,)
    if name == "synth_128_0":
        return synth_pair(5102, N, 128, 0) + (0,)
    if name == "synth_104_27":
        return synth_pair(5103, N, 104, 27) + (0,)
    if name == "wide_2048":            # heavy_build_kernel<64>, 16 KB of query words per refine workgroup
        return synth_pair(5104, 700, 2048, 64) + (0,)
    if name == "wide_4096":            # ... and slice ids that use all 12 key bits
        return synth_pair(5105, 700, 4096, 64) + (0,)
    if name == "abs_mode":             # negative gated values on both sides: the index is built in abs mode
        cv, ci, qv, qi = synth_pair(5106, N, 768, 64)
        rng = np.random.default_rng(5106)
        cv = cv.copy()
        cv[:, :768] *= rng.choice([-1, 1], size=(N, 768)).astype(np.float16)
        qv[:, :768] *= rng.choice([-1, 1], size=(Q, 768)).astype(np.float32)
        return cv, ci, qv, qi, 0
    if name == "ungated_batch":        # plain inner product (--IP stage 1): refined on the int8 image of the gated half only
        cv, ci, qv, qi = synth_pair(5107, N, 768, 64)
        return cv, ci, qv, None, 0
    if name == "int16_alias":
        c = RC.int16_alias(5108)
        return c["cv"], c["ci"], RC.adversarial_queries(c["qv"], RC.D), c["qi"], 0
    if name == "short_rows":           # rows with 0 .. 128 non-zero gated values, one bucket (such an index keeps the fp16 image of its gated half)
        c = RC.short_rows(11)
        return c["cv"], c["ci"], c["qv"], c["qi"], 1
    if name == "short_rows_parity":    # ... and with 16-bit index values: two buckets by the parity of the value
        c = RC.short_rows(11, idx_dtype=np.int16)
        return c["cv"], c["ci"], c["qv"], c["qi"], 0
    raise ValueError(name)


CASES_3A = ["synth_768_64", "synth_128_0", "synth_104_27", "wide_2048", "wide_4096", "abs_mode", "ungated_batch", "int16_alias", "short_rows", "short_rows_parity"]


@pytest.mark.parametrize("name", CASES_3A)
def test_refined_bound_is_safe_and_monotone(name, gated_image):
    """tau = null (thr = -inf: every row passes both levels), all pairs:  U2 >= exact_f64 - margin_q,  U2 <= U,  and the U of the list entries
    the filter epilogue appends equals the GEMM's dump bit for bit (one conversion of the same accumulator: nothing may differ).
    Default buckets (two) except `short_rows`; the bucket test of the refine level is covered here only (see 3c)."""
    from dhr_amd import _lib
    cv, ci, qv, qi, nb = _case(name)
    n = cv.shape[0]
    ix = _index(cv, ci, idx_buckets=nb)
    image = "gated_fp16" if nb == 1 else gated_image                     # (the int8 image needs the two bucket columns: index_layout.h)
    try:
        _image_is(ix, image)
        if name == "ungated_batch" and gated_image == "gated_fp16":      # such a batch rescores its bound lists directly
            with pytest.raises(_lib.DhrError) as ei:
                _refine(ix, qv, qi, n)
            assert ei.value.status == _lib.ERR_UNSUPPORTED
            return
        margin = _margins(ix, qv, qi)
        dump = _dump(ix, qv, qi, n)
        U, U2, thr, unit = _refine(ix, qv, qi, n)
    finally:
        ix.close()
    exact = _exact(cv, ci, qv, qi)
    assert np.all(np.isneginf(thr)) and np.all(np.isfinite(margin))
    assert not np.isnan(U).any() and not np.isnan(U2).any()               # every row is in both lists, once
    assert np.array_equal(_bits(U), _bits(dump))
    U, U2 = U.astype(np.float64), U2.astype(np.float64)
    head = U2 - (exact - margin[:, None])
    q, r = np.unravel_index(int(head.argmin()), head.shape)
    print("\n[refine_bounds] 3a %-17s %-10s min head room U2 - (exact - margin) %.3e (query %d row %d; margins %.3e .. %.3e)  min U2 - exact %.3e  min U - U2 %.3e  mean (U - U2) / (U - exact) %.3f"
          % (name, image, head.min(), q, r, margin.min(), margin.max(), (U2 - exact).min(), (U - U2).min(), float((U - U2).sum() / max((U - exact).sum(), 1e-30))))
    assert np.all(head >= 0.0), (q, r, head.min())
    assert np.all(U2 <= U), float((U - U2).min())


# ------------------------------------------------------------------------------------------------ 3b, 3c: images and bucket rules
# one_bucket: idx_buckets = 1, 8-bit index values -- the fp16 image only (an index with one bucket keeps it: the int8 image needs the two bucket
# columns).  parity: the default two buckets with 16-bit index values, which have no bucket map: bucket = value % 2 (index_build.hip), a rule
# the restatement can state.  Index values 0 .. 3: a listed entry shares the query's bucket without sharing its index value in a quarter of
# the (entry, query) pairs -- the entries whose whole product the level must take off.
SETUPS = [("gated_fp16", "one_bucket"), ("gated_fp16", "parity"), ("gated_i8", "parity")]


def _short_rows(seed, kind, buckets):
    """-> (case, idx_buckets, bucket_q, bucket_d)"""
    if buckets == "one_bucket":
        return RC.short_rows(seed, kind), 1, None, None
    c = RC.short_rows(seed, kind, idx_dtype=np.int16)
    return c, 0, c["qi"] % 2, c["ci"] % 2


@pytest.mark.parametrize("gated_image,buckets", SETUPS)
def test_collapse_on_short_rows(gated_image, buckets, monkeypatch):
    """No ungated columns, non-negative values, fp16-representable queries, rows with 0, 1, 4, 5, 6, 19, 20, 21, 31, 63 and 64 non-zero gated
    values: every entry is listed, so the level sees everything the bound counted (the entries of the query's bucket) and the refined bound
    must come down to the exact score -- under one bucket and under any bucket rule.  An entry of the query's bucket that no lane reads (the
    twentieth of line 1, a lane's eleventh of level 2, ...) leaves a whole product >= 1 in the bound unless its index value agrees; every
    tolerance below is under a tenth of that (asserted; tests/test_refine_oracle.py: every record position holds such an entry).

    int8 image:  0 <= U2 - exact <= 8 ulp32(U).  With every entry listed, U2 = roundup32(U - S unit + exact) where S unit is the integer sum
    the GEMM converted: U = fl(x + |x| 2.4e-7), x = fl(float(S) mul) (g8_score: "rounded up"; S < 2^24 converts exactly, mul == unit without
    ungated columns).  Two roundings to nearest and the 2.4e-7 put U within (2 x 2^-24 + 2.4e-7) S unit < (2 + 4.03) ulp32(U) above S unit
    (S unit <= U < 2^24 ulp32(U)) and never below it; the one round-up of bound_g8 adds less than ulp32(U): 7.1, rounded up to 8.
    fp16 image:  |U2 - exact| <= margin_q + 64 2^-24 sum |q d|  (what the GEMM's U may be off by; the fp32 sum of up to 64 corrections)."""
    monkeypatch.setenv("DHR_GATED_I8", "1" if gated_image == "gated_i8" else "0")
    c, nb, _, _ = _short_rows(11, "distinct", buckets)
    cv, ci, qv, qi = c["cv"], c["ci"], c["qv"], c["qi"]
    ix = _index(cv, ci, idx_buckets=nb)
    try:
        _image_is(ix, gated_image)
        margin = _margins(ix, qv, qi)
        U, U2, _, unit = _refine(ix, qv, qi, N)
    finally:
        ix.close()
    exact = _exact(cv, ci, qv, qi)
    short = c["nnz"] <= RC.COLLAPSE_MAX_NNZ
    U, U2 = U.astype(np.float64), U2.astype(np.float64)
    off = (U2 - exact)[:, short]
    prod_min = float(qv.min()) * float(cv[cv > 0].astype(np.float64).min())
    if gated_image == "gated_i8":
        tol = 8.0 * RC.ulp32(U)[:, short]
        print("\n[refine_bounds] 3b short_rows parity     gated_i8   U2 - exact in ulp32(U): min %.2f max %.2f (bound 0 .. 8); rows with > 64 values keep %.3e .. %.3e"
              % ((off / RC.ulp32(U)[:, short]).min(), (off / RC.ulp32(U)[:, short]).max(), (U2 - exact)[:, ~short].min(), (U2 - exact)[:, ~short].max()))
        assert prod_min > 10 * tol.max()
        assert np.all(off >= 0.0) and np.all(off <= tol), (float(off.min()), float((off / RC.ulp32(U)[:, short]).max()))
    else:
        sum_abs = np.abs(qv.astype(np.float64)) @ np.abs(cv.astype(np.float64)).T
        tol = (margin[:, None] + 64 * 2.0 ** -24 * sum_abs)[:, short]
        print("\n[refine_bounds] 3b short_rows %-10s gated_fp16 |U2 - exact| / (margin + 64 2^-24 sum |q d|): max %.3f (bound 1); margins %.3e .. %.3e; rows with > 64 values keep %.3e .. %.3e"
              % (buckets, (np.abs(off) / tol).max(), margin.min(), margin.max(), (U2 - exact)[:, ~short].min(), (U2 - exact)[:, ~short].max()))
        assert prod_min > 10 * tol.max()
        assert np.all(np.abs(off) <= tol), float((np.abs(off) / tol).max())


# ------------------------------------------------------------------------------------------------ 3c
@pytest.mark.parametrize("gated_image,buckets", SETUPS)
@pytest.mark.parametrize("kind", ["distinct", "ties"])
def test_refine_equals_the_restatement(kind, gated_image, buckets, monkeypatch):
    """U - U2 of the device == U - U2_ref of oracle/refine_oracle.py, given the device's U, on the short-rows corpus (rows with 65 and 128 values
    included: the 64-entry cut of a record) with fp16-representable queries, under one bucket and under the parity buckets of 16-bit index
    values.  `distinct`: magnitudes distinct within a row; `ties`: the rows with 128 values hold 48 equal ones across the cut, of which the
    record must take the 24 in the lowest slices.  No oracle module restates build_bucket_map (8-bit index values, two buckets): the bucket
    test against such a map is covered by 3a only.

    fp16 image: |diff| <= 64 2^-24 corr_ref + ulp32(U) (an fp32 sum of up to 64 exact products; one rounded subtraction).
    int8 image: the rule in force is the strict one -- exact up to ulp32(U).  The generator redraws every value within 1e-4 relative of a
    rounding boundary of its int8 level, so the restated levels are the device's; the unit is the device's own (the hook hands it out, as it
    hands out U: the device derives it in fp32 with ~1e-6 of deliberate head room, which no float64 restatement reproduces to an ulp; 3b pins
    that unit against the GEMM's).  What remains is bound_g8's one round-up of the fp64 expression."""
    monkeypatch.setenv("DHR_GATED_I8", "1" if gated_image == "gated_i8" else "0")
    c, nb, bq, bd = _short_rows(11 if kind == "distinct" else 12, kind, buckets)
    cv, ci, qv, qi = c["cv"], c["ci"], c["qv"], c["qi"]
    ix = _index(cv, ci, idx_buckets=nb)
    try:
        _image_is(ix, gated_image)
        U, U2, _, unit = _refine(ix, qv, qi, N)
    finally:
        ix.close()
    U, U2 = U.astype(np.float64), U2.astype(np.float64)
    got = U - U2
    if gated_image == "gated_i8":
        ref, taken, back = R.corr_g8(qv, qi, None, cv.astype(np.float32), ci, None, bucket_q=bq, bucket_d=bd, unit=unit.astype(np.float64))
        _, unit_ref = R.query_levels(qv, None, cv.astype(np.float32), None)
        tol = RC.ulp32(U)
        print("\n[refine_bounds] 3c %-8s parity     gated_i8   |(U - U2) - ref| in ulp32(U): max %.3f (bound 1); device unit / restated unit - 1: %.2e .. %.2e"
              % (kind, (np.abs(got - ref) / tol).max(), (unit / unit_ref - 1).min(), (unit / unit_ref - 1).max()))
        assert np.all(np.abs(unit / unit_ref - 1.0) <= 1e-5)              # the head room of the device's unit (g8_bound_oracle's header)
    else:
        ref = R.corr_fp16(qv, qi, cv.astype(np.float32), ci, bucket_q=bq, bucket_d=bd)
        tol = 64 * 2.0 ** -24 * ref + RC.ulp32(U)
        print("\n[refine_bounds] 3c %-8s %-10s gated_fp16 |(U - U2) - ref| / (64 2^-24 ref + ulp32(U)): max %.3f (bound 1)" % (kind, buckets, (np.abs(got - ref) / tol).max()))
    bad = np.abs(got - ref) > tol
    assert not bad.any(), [(int(q), int(r), int(c["nnz"][r]), float(got[q, r]), float(ref[q, r])) for q, r in zip(*np.nonzero(bad))][:5]


# ------------------------------------------------------------------------------------------------ 3d
def _tau_for_tie(u2r, m):
    """An fp32 tau with fl32(tau - m) == u2r (make_thr_kernel's subtraction), or None."""
    u2r, m = np.float32(u2r), np.float32(m)
    lo = hi = np.float32(u2r + m)
    for _ in range(16):
        for cand in (lo, hi):
            if np.float32(cand - m) == u2r:
                return cand
        lo, hi = np.nextafter(lo, np.float32(-np.inf)), np.nextafter(hi, np.float32(np.inf))
    return None


@pytest.mark.parametrize("flat", [0, 1, 2])
def test_survivor_sets_at_finite_thresholds(flat, gated_image):
    """768 + 64 columns, tau_q per query one of: below every score (every candidate survives, all 512 slots of every block fill), above every
    bound (nobody survives), the median exact score, exactly the exact score of one row, and the tau whose thr EQUALS one row's U2 (the tie of
    the final `>=`); the five settings rotate over the queries in five calls.  The rows the level returns must be exactly
    {row of the GEMM list : U2_dump[row] >= thr_q} with U2_dump from the tau = null call: level 1's early test drops nothing the final test
    keeps, the compaction loses and duplicates nothing, a tie stays.  U2 of a surviving row is bit-equal to the tau = null call's, between two
    calls, and between the launch forms (list order differs from call to call: a row's value must not depend on its slot).  flat: 0 = grid of
    (block, query), 1 = flat launch over the block offsets with the grid of the controller that only enqueues, 2 = the same on two workgroups
    (every workgroup walks several blocks of several queries by grid stride).  The GEMM list itself must hold every row whose exact score reaches tau."""
    from dhr_amd import synth
    cv, ci, qv, qi = synth.make_pair(5101, N, Q, 768, 64)
    qv, qi = qv.astype(np.float32), qi.astype(np.int16)
    exact = _exact(cv, ci, qv, qi)
    ix = _index(cv, ci)
    try:
        _image_is(ix, gated_image)
        margin32 = _margins(ix, qv, qi).astype(np.float32)
        U0, U20, _, _ = _refine(ix, qv, qi, N, flat=0)
        assert not np.isnan(U0).any() and not np.isnan(U20).any()
        Ua, U2a, _, _ = _refine(ix, qv, qi, N, flat=flat)
        assert np.array_equal(_bits(U0), _bits(Ua)) and np.array_equal(_bits(U20), _bits(U2a))      # between two calls and between the launch forms
        ties = kept_total = unlisted_above = 0
        for shift in range(5):
            tau = np.zeros(Q, np.float32)
            tie_row = {}
            for q in range(Q):
                setting = (q + shift) % 5
                if setting == 0:
                    tau[q] = np.float32(exact[q].min() - 1.0)                     # thr = tau - margin <= exact - margin <= U2 for every row
                elif setting == 1:
                    tau[q] = np.float32(float(U0[q].max()) + float(margin32[q]) + 1.0)
                elif setting == 2:
                    tau[q] = np.float32(np.median(exact[q]))
                elif setting == 3:
                    tau[q] = np.float32(exact[q][np.argsort(exact[q])[(3 * N) // 4]])
                else:
                    r = int(np.argsort(U20[q])[(2 * N) // 3])
                    t = _tau_for_tie(U20[q, r], margin32[q])
                    tau[q] = t if t is not None else np.float32(U20[q, r] + margin32[q])
                    if t is not None:
                        tie_row[q] = r
            U, U2, thr, _ = _refine(ix, qv, qi, N, tau=tau, flat=flat)
            assert np.array_equal(thr, (tau - margin32).astype(np.float32))         # make_thr_kernel
            listed = ~np.isnan(U)
            assert np.all(listed | (exact < tau.astype(np.float64)[:, None]))         # the filter drops no row whose exact score reaches tau
            unlisted_above += int((~listed & (U0 >= thr[:, None])).sum())             # (it may test in accumulator units, conservatively: printed)
            assert np.array_equal(_bits(U)[listed], _bits(U0)[listed])
            want = listed & (U20 >= thr[:, None])
            got = ~np.isnan(U2)
            assert np.array_equal(got, want), [(int(q), int(r), float(U20[q, r]), float(thr[q])) for q, r in zip(*np.nonzero(got != want))][:5]
            assert np.array_equal(_bits(U2)[got], _bits(U20)[got])
            for q in range(Q):
                setting = (q + shift) % 5
                if setting == 0:
                    assert got[q].all()
                elif setting == 1:
                    assert not got[q].any()
            for q, r in tie_row.items():
                assert thr[q] == U20[q, r] and got[q, r]
            ties += len(tie_row)
            kept_total += int(got.sum())
        print("\n[refine_bounds] 3d flat %d %-10s survivor sets exact in 5 x %d queries (%d pairs kept), %d exact ties U2 == thr kept; rows with U >= thr outside the GEMM list: %d" % (flat, gated_image, Q, kept_total, ties, unlisted_above))
        assert ties >= Q // 2                                                      # the tie is pinned, not merely attempted
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------------ 3e
def _dense_case(d_cls, kind):
    rng = np.random.default_rng(6000 + d_cls + {"gauss": 0, "outlier_columns": 1, "spiky_rows": 2}[kind])
    cv = (rng.standard_normal((N, d_cls)) * 0.1).astype(np.float32)
    qv = (rng.standard_normal((Q, d_cls)) * 0.1).astype(np.float32)
    if kind == "outlier_columns":
        cv[:, ::7] *= 30.0
        qv[:, ::7] *= 0.2
    elif kind == "spiky_rows":
        cv[::11] = 0
        cv[np.arange(0, N, 11), rng.integers(0, d_cls, len(range(0, N, 11)))] = 6.0
    qv[0] = 0; qv[0, rng.integers(0, d_cls)] = 1.5                                # a one-hot query
    qv[1:4] = qv[1:4] * np.float32(1.0001) + np.float32(1e-5)                     # fp32 values that are not fp16-representable
    return cv.astype(np.float16), qv.astype(np.float32)


@pytest.mark.parametrize("kind", ["gauss", "outlier_columns", "spiky_rows"])
@pytest.mark.parametrize("d_cls", [27, 128, 300, 768, 1000])
def test_residual_level_of_dense_int8_indexes(d_cls, kind):
    """dense_refine_kernel<16 | 32 | 48 | 64> (27 / 128, 300, 768, 1000 columns; 27 and 300 are no multiples of 16) on Gaussian data, outlier
    columns and spiky rows, with a one-hot query and queries that are not fp16-representable.
    Safety without knowing the level's internal threshold shift (thr + thr_raise - 7 sd): from the tau = null dump take, per query,
    r* = argmin(U2 - exact); with tau_q the largest fp32 <= exact(r*) every row with exact >= tau_q must be returned -- r* at its own border is
    the worst case of its query.  The rows the level returns are an upper set in U2_dump among the rows of the GEMM list (the two levels
    compare with different thresholds, so a row the FILTER dropped may have a larger U2 than a kept one: that figure is printed, not asserted).
    Two-sided sanity: |U2 - exact| <= margin_q."""
    from dhr_amd import _lib
    lib = _lib.load()
    cv, qv = _dense_case(d_cls, kind)
    exact = _exact(cv, None, qv, None)
    _lib.check(lib.dhr_set_option(_lib.OPT_DENSE_I8, 1), "set_option")
    try:
        ix = _index(cv, None)
    finally:
        _lib.check(lib.dhr_set_option(_lib.OPT_DENSE_I8, -1), "set_option")
    try:
        assert int(ix.info(_lib.INFO_DENSE_I8)) == 1
        margin = _margins(ix, qv, None)
        dump = _dump(ix, qv, None, N)
        U0, U20, _, _ = _refine(ix, qv, None, N)
        assert not np.isnan(U0).any() and not np.isnan(U20).any() and np.array_equal(_bits(U0), _bits(dump))
        u2 = U20.astype(np.float64)
        rstar = (u2 - exact).argmin(axis=1)
        tau = np.array([exact[q, rstar[q]] for q in range(Q)]).astype(np.float32)
        tau = np.where(tau.astype(np.float64) > exact[np.arange(Q), rstar], np.nextafter(tau, np.float32(-np.inf)), tau).astype(np.float32)
        U, U2, thr, _ = _refine(ix, qv, None, N, tau=tau, flat=1)
    finally:
        ix.close()
    got, listed = ~np.isnan(U2), ~np.isnan(U)
    must = exact >= tau.astype(np.float64)[:, None]
    assert np.all(got[must]), [(int(q), int(r)) for q, r in zip(*np.nonzero(must & ~got))][:5]
    assert np.all(got[np.arange(Q), rstar])
    assert np.array_equal(_bits(U2)[got], _bits(U20)[got])
    gap_listed, gap_all = np.inf, np.inf
    for q in range(Q):
        if got[q].any():
            lowest_kept = u2[q][got[q]].min()
            dropped = listed[q] & ~got[q]
            if dropped.any():
                gap_listed = min(gap_listed, lowest_kept - u2[q][dropped].max())
            if (~got[q]).any():
                gap_all = min(gap_all, lowest_kept - u2[q][~got[q]].max())
    two_sided = np.abs(u2 - exact) / margin[:, None]
    print("\n[refine_bounds] 3e d_cls %4d %-15s min head room U2 - (exact - margin) %.3e  max |U2 - exact| / margin %.3f (bound 1)  kept %d of %d listed of %d pairs; "
          "lowest kept U2 - highest dropped U2: %.3e among listed rows, %.3e among all rows"
          % (d_cls, kind, (u2 - exact + margin[:, None]).min(), two_sided.max(), int(got.sum()), int(listed.sum()), got.size, gap_listed, gap_all))
    assert gap_listed >= 0.0
    assert np.all(two_sided <= 1.0), float(two_sided.max())
