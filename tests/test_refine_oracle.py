"""The restatement of the refine level (oracle/refine_oracle.py) pinned on the CPU, on the generators that tests/test_refine_bounds.py
runs on the device (tests/refine_cases.py): fed with the nominal bound U of its image (g8_bound_oracle.bound_scores; for the fp16 image
the plain sum of the bucket-matching operand products) the refined bound keeps  exact - margin <= U2 <= U  for every pair, it collapses to
the exact score on rows that a record holds completely, and the generators meet the conditions the device tests rely on: products far
above the tolerances, no int8 level on a rounding boundary, no tie (or a deliberate one) at the 64-entry cut of a record."""
import numpy as np
import pytest

from oracle import g8_bound_oracle as G8
from oracle import gip_oracle as O
from oracle import refine_oracle as R
from tests import refine_cases as RC


def _exact(c, ungated=False):
    cv = c["cv"].astype(np.float32)
    return np.stack([O.gip_scores_f64(c["qv"][q], None if ungated else c["qi"][q], cv, None if ungated else c["ci"]) for q in range(c["qv"].shape[0])])


def _split(c, d):
    cv = c["cv"].astype(np.float32)
    return c["qv"][:, :d], c["qv"][:, d:], cv[:, :d], cv[:, d:]


def _u_fp16(qg, cg, bucket_q, bucket_d, abs_mode):
    """Nominal bound of the fp16 image: every slice whose buckets agree counts its operand product."""
    q16 = R._operand(qg, abs_mode).astype(np.float16).astype(np.float64)
    return np.stack([((bucket_d == bucket_q[q][None, :]) * np.abs(cg.astype(np.float64))) @ q16[q] for q in range(qg.shape[0])])


def _synth_case(seed, abs_mode=False):
    from dhr_amd import synth
    cv, ci, qv, qi = synth.make_pair(seed, 400, 9, 128, 64)
    c = dict(cv=cv.copy(), ci=ci, qv=RC.adversarial_queries(qv, 128), qi=qi.astype(np.int16))
    if abs_mode:
        rng = np.random.default_rng(seed)
        c["cv"][:, :128] *= rng.choice([-1, 1], size=(400, 128)).astype(np.float16)
        c["qv"][:, :128] *= rng.choice([-1, 1], size=(9, 128)).astype(np.float32)
    return c


CASES = {
    "short_rows": lambda: (RC.short_rows(11), 128, False),
    "short_rows_ties": lambda: (RC.short_rows(12, "ties"), 128, False),
    "synth_128_64": lambda: (_synth_case(13), 128, False),
    "synth_abs_mode": lambda: (_synth_case(14, True), 128, True),
    "int16_alias": lambda: (RC.int16_alias(15, 400), 128, False),
}


@pytest.mark.parametrize("buckets", [1, 2])
@pytest.mark.parametrize("name", sorted(CASES))
def test_refined_bound_between_exact_and_bound(name, buckets):
    c, d, abs_mode = CASES[name]()
    qg, qd, cg, cd = _split(c, d)
    exact = _exact(c)
    # one bucket, or two per slice by the parity of the index value (the device's maps are some such function of the index value)
    bq, bd = (np.zeros_like(c["qi"]), np.zeros_like(c["ci"])) if buckets == 1 else (c["qi"] % 2, c["ci"] % 2)
    eps = 1e-9 * max(1.0, float(np.abs(exact).max()))
    # int8 image
    U, margin = G8.bound_scores(qg, c["qi"], qd, cg, c["ci"], cd, bq, bd, abs_mode)
    corr, taken, back = R.corr_g8(qg, c["qi"], qd, cg, c["ci"], cd, abs_mode=abs_mode, bucket_q=bq, bucket_d=bd)
    assert np.all(corr >= -eps) and np.all(U - corr >= exact - margin[:, None] - eps), float((U - corr - exact + margin[:, None]).min())
    # ... and a plain inner-product batch on it: every listed entry counts and every one matches
    z = np.zeros_like(c["ci"])
    Uu, margin_u = G8.bound_scores(qg, z[:qg.shape[0]], qd, cg, z, cd, abs_mode=abs_mode)
    corr_u, _, _ = R.corr_g8(qg, None, qd, cg, c["ci"], cd, abs_mode=abs_mode, ungated=True)
    exact_u = _exact(c, ungated=True)
    if abs_mode:
        exact_u = np.abs(qg).astype(np.float64) @ np.abs(cg).astype(np.float64).T + qd.astype(np.float64) @ cd.astype(np.float64).T
    assert np.all(corr_u >= -eps) and np.all(Uu - corr_u >= exact_u - margin_u[:, None] - eps)
    # fp16 image (the nominal sum has no rounding: no margin but the fp16 rounding of the query operand, |q - q16| |d| summed)
    U16 = _u_fp16(qg, cg, bq, bd, abs_mode)
    c16 = R.corr_fp16(qg, c["qi"], cg, c["ci"], abs_mode=abs_mode, bucket_q=bq, bucket_d=bd)
    q16 = R._operand(qg, abs_mode).astype(np.float16).astype(np.float64)
    m16 = np.abs(R._operand(qg, abs_mode) - q16) @ np.abs(cg).astype(np.float64).T
    exact_g = exact - qd.astype(np.float64) @ cd.astype(np.float64).T
    assert np.all(c16 >= 0) and np.all(U16 - c16 >= exact_g - m16 - eps), float((U16 - c16 - exact_g + m16).min())


@pytest.mark.parametrize("buckets", ["one_bucket", "parity"])
@pytest.mark.parametrize("kind", ["distinct", "ties"])
def test_collapse_and_generator_conditions(kind, buckets):
    """one_bucket: idx_buckets = 1 (the fp16 image); parity: 16-bit index values, which the device deals into two buckets by value % 2."""
    c = RC.short_rows(11 if kind == "distinct" else 12, kind, idx_dtype=np.uint8 if buckets == "one_bucket" else np.int16)
    bq, bd = (np.zeros_like(c["qi"]), np.zeros_like(c["ci"])) if buckets == "one_bucket" else (c["qi"] % 2, c["ci"] % 2)
    cv, qv = c["cv"].astype(np.float64), c["qv"].astype(np.float64)
    assert np.array_equal((cv > 0).sum(axis=1), c["nnz"]) and set(c["nnz"].tolist()) == set(RC.NNZ)
    assert np.array_equal(qv.astype(np.float16).astype(np.float64), qv)                    # fp16-representable queries
    exact = _exact(c)
    listed = R.select_records(cv)
    short = c["nnz"] <= RC.COLLAPSE_MAX_NNZ
    assert np.array_equal((listed >= 0).sum(axis=1), np.minimum(c["nnz"], R.HEAVY))
    # ---- collapse: every non-zero entry of a short row is listed, the level sees all the bound counted -> the refined bound IS the exact score
    U, margin = G8.bound_scores(qv, c["qi"], None, cv, c["ci"], None, bq, bd)
    corr, taken, back = R.corr_g8(qv, c["qi"], None, cv, c["ci"], None, bucket_q=bq, bucket_d=bd)
    scale = float(np.abs(U).max())
    assert np.abs((U - corr) - exact)[:, short].max() <= 1e-12 * scale
    assert np.abs(back - exact)[:, short].max() <= 1e-12 * scale
    U16 = _u_fp16(qv, cv, bq, bd, False)
    c16 = R.corr_fp16(qv, c["qi"], cv, c["ci"], bucket_q=bq, bucket_d=bd)
    assert np.abs((U16 - c16) - exact)[:, short].max() <= 1e-12 * scale
    assert np.all((U - corr)[:, ~short] >= exact[:, ~short]) and np.any((U16 - c16)[:, ~short] > exact[:, ~short] + 1.0)   # longer rows keep slack
    # ---- a missed entry cannot hide: every product of a listed entry with every query is above ten times the device tests' tolerances.
    # int8 image: 8 ulp32(U) (test_refine_bounds.py derives the 8); fp16 image: margin + 64 2^-24 sum |q d|, the margin bounded from
    # query_prep_kernel's expression with a padded width of at most 4096 columns and no fp16 rounding of the query
    prod_min = float(qv.min() * cv[cv > 0].min())
    tol_i8 = 8.0 * float(RC.ulp32(U).max())
    sum_abs = np.abs(qv) @ np.abs(cv).T
    margin16 = 1.05 * (4096 + 256) * 2.0 ** -24 * np.linalg.norm(qv, axis=1) * float(cv.max())
    tol_16 = float((margin16[:, None] + 64 * 2.0 ** -24 * sum_abs).max())
    assert prod_min >= 1.0 and prod_min > 10 * tol_i8 and prod_min > 10 * tol_16, (prod_min, tol_i8, tol_16)
    # every record position is reached, in rows of every length that holds it, by an entry of the query's bucket whose index value differs
    # (its whole product must come off the bound) and by one whose index value agrees
    at = np.maximum(listed, 0)
    for length in sorted(set(c["nnz"].tolist())):
        rows = c["nnz"] == length
        differs = np.zeros(R.HEAVY, bool); agrees = np.zeros(R.HEAVY, bool)
        for q in range(qv.shape[0]):
            live = (listed >= 0) & rows[:, None] & (bq[q][at] == np.take_along_axis(bd, at, axis=1))
            ne = c["qi"][q].astype(np.int64)[at] != np.take_along_axis(c["ci"].astype(np.int64), at, axis=1)
            differs |= (live & ne).any(axis=0); agrees |= (live & ~ne).any(axis=0)
        held = np.arange(R.HEAVY) < min(length, R.HEAVY)
        assert np.array_equal(differs, held) and np.array_equal(agrees, held), length
    # ---- no int8 level on a rounding boundary (1e-4 relative), on either side
    assert not R.borderline_corpus(cv).any() and not R.borderline_queries(qv, None, cv, None).any()
    # ---- the 64-entry cut
    mag = np.sort(np.abs(cv), axis=1)[:, ::-1]
    full = c["nnz"] > R.HEAVY
    if kind == "distinct":
        nz = mag > 0
        assert np.all((np.diff(mag, axis=1) < 0) | ~nz[:, 1:])                              # distinct magnitudes within a row
    else:
        tied = full & (c["nnz"] == RC.D)
        assert tied.any() and np.all(mag[tied, R.HEAVY - 1] == mag[tied, R.HEAVY])          # a tie across the cut ...
        for r in np.nonzero(tied)[0]:                                                       # ... resolved toward the lower slices
            v = mag[r, R.HEAVY]
            run = np.nonzero(np.abs(cv[r]) == v)[0]
            kept = np.intersect1d(listed[r], run)
            assert len(run) == 48 and np.array_equal(kept, run[:len(kept)]) and len(kept) == 24
            assert np.array_equal(listed[r][40:64], run[:24])                               # heaviest first, the run in slice order


def test_record_selection_rules():
    cg = np.zeros((4, 200), np.float32)
    cg[0, [5, 9, 150]] = [1.0, -3.0, 2.0]                     # magnitudes rank, signs do not
    cg[1, :] = 1.0                                            # all equal: the 64 lowest slices
    cg[2, 10:90] = np.arange(80, 0, -1)
    cg[2, 3] = 70.0                                           # ties with slice 20: the lower slice first
    cg[3, 7] = np.float32(1e-9)                               # below fp16: the record ranks the fp16 image, where it is zero
    L = R.select_records(cg)
    assert L[0].tolist()[:4] == [9, 150, 5, -1] and np.all(L[0][3:] == -1)
    assert L[1].tolist() == list(range(64))
    assert L[2].tolist()[:13] == list(range(10, 20)) + [3, 20, 21] and len(set(L[2].tolist())) == 64
    assert np.all(L[3] == -1)
    # index values are compared in 12 bits: a pair that differs only above bit 11 counts as equal
    qg = np.ones((1, 200), np.float32); qi = np.full((1, 200), 5, np.int16); ci = np.full((4, 200), 5 + 4096, np.int16)
    assert np.all(R.corr_fp16(qg, qi, cg, ci) == 0)
    ci[:] = 6
    assert R.corr_fp16(qg, qi, cg, ci)[0, 0] == 6.0
