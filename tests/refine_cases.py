"""Corpora and query batches of the refine-bound tests, shared by tests/test_refine_oracle.py (CPU: the conditions below can be met and
hold) and tests/test_refine_bounds.py (GPU).  Everything is deterministic in its seed.

collapse / restatement cases: 128 gated columns, no ungated ones, ONE index bucket, non-negative fp16 values from the grid
1 + k / 1024 (k < 1024) on both sides, index values 0 .. 3.  Every query value is non-zero, so every listed entry of a row has a product
q_j d_j >= 1 with every query, far above any tolerance the tests apply (asserted there).  Row r holds NNZ[r % len(NNZ)] non-zero values
in random slices, their magnitudes distinct within the row (the 64-entry cut of a record then has no tie); kind "ties" gives the rows
with 128 values a run of 48 equal ones across the cut instead.  Values whose int8 level (g8_bound_oracle) lies within 1e-4 relative
of a rounding boundary are redrawn, on both sides, so that a restated level cannot differ from the device's."""
import numpy as np

from oracle import refine_oracle as R

D, N, Q = 128, 1500, 9
NNZ = (0, 1, 4, 5, 6, 19, 20, 21, 31, 63, 64, 65, 128)
COLLAPSE_MAX_NNZ = 64                    # rows with more non-zero values than a record holds do not collapse to the exact score


def ulp32(x):
    """Spacing of float32 at |x| (float64 array)."""
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)


def _grid(rng, shape):
    return 1.0 + rng.integers(0, 1024, shape) / 1024.0


def short_rows(seed: int, kind: str = "distinct", idx_dtype=np.uint8):
    """-> dict(cv fp16 [N, D], ci [N, D], qv fp32 [Q, D], qi int16 [Q, D], nnz [N])."""
    assert kind in ("distinct", "ties")
    rng = np.random.default_rng(seed)
    nnz = np.array([NNZ[r % len(NNZ)] for r in range(N)])
    cv = np.zeros((N, D))
    run = np.zeros((N, D), bool)                                                  # kind "ties": the equal values of a row
    lo, hi = np.ones((N, D)), np.full((N, D), 2.0)                                # the range [lo, hi) an entry is (re)drawn from
    for r in range(N):
        sl = rng.permutation(D)[:nnz[r]]
        cv[r, sl] = 1.0 + rng.permutation(1024)[:nnz[r]] / 1024.0                # distinct within the row
        if kind == "ties" and nnz[r] == D:
            # 40 values above the run, 48 equal ones, 40 below: the cut takes the 24 of the run that sit in the lowest slices
            order = rng.permutation(D)
            cv[r, order[:40]] = 1.75 + rng.permutation(256)[:40] / 1024.0
            cv[r, order[40:88]] = 1.5
            cv[r, order[88:]] = 1.0 + rng.permutation(256)[:40] / 1024.0
            run[r, order[40:88]] = True
            lo[r, order[:40]], hi[r, order[88:]] = 1.75, 1.25
            lo[r, order[40:88]], hi[r, order[40:88]] = 1.45, 1.55
    qv = _grid(rng, (Q, D))
    ci = rng.integers(0, 4, (N, D)).astype(idx_dtype)
    qi = rng.integers(0, 4, (Q, D)).astype(np.int16)

    def draw(r, c):
        return lo[r, c] + int(rng.integers(0, round((hi[r, c] - lo[r, c]) * 1024))) / 1024.0

    for _ in range(200):                                                          # redraw what sits on a level boundary
        bad = R.borderline_corpus(cv)
        if not bad.any():
            break
        for r in np.nonzero((bad & run).any(axis=1))[0]:                          # a run moves as a whole
            cv[r, run[r]] = draw(r, np.nonzero(run[r])[0][0])
        for r, c in zip(*np.nonzero(bad & ~run)):
            v = draw(r, c)
            while v in cv[r]:
                v = draw(r, c)
            cv[r, c] = v
    else:
        raise AssertionError("corpus values still on a level boundary")
    for _ in range(100):
        bad = R.borderline_queries(qv, None, cv, None)
        if not bad.any():
            break
        qv[bad] = _grid(rng, int(bad.sum()))
    else:
        raise AssertionError("query values still on a level boundary")
    return dict(cv=cv.astype(np.float16), ci=ci, qv=qv.astype(np.float32), qi=qi, nnz=nnz)


def int16_alias(seed: int, n: int = N, d_cls: int = 64):
    """128 gated columns with int16 index values above 4095, negative ones, and pairs that differ only above bit 11 (they alias in the
    refine level's 12-bit compare: the bound may get looser and must stay safe); d_cls ungated columns."""
    rng = np.random.default_rng(seed)
    pool = np.array([5, 5 + 4096, 5 + 8192, -3, -3 + 4096, 300, 300 - 4096, 32767, 32767 - 4096, -32768], np.int16)
    cv = np.where(rng.random((n, D)) < 0.6, rng.uniform(0.05, 3.0, (n, D)), 0.0)
    qv = np.where(rng.random((Q, D)) < 0.5, rng.uniform(0.05, 3.0, (Q, D)), 0.0)
    ci = pool[rng.integers(0, len(pool), (n, D))]
    qi = pool[rng.integers(0, len(pool), (Q, D))]
    cd = rng.standard_normal((n, d_cls)) * 0.1
    qd = rng.standard_normal((Q, d_cls)) * 0.1
    return dict(cv=np.concatenate([cv, cd], axis=1).astype(np.float16), ci=ci, qv=np.concatenate([qv, qd], axis=1).astype(np.float16).astype(np.float32), qi=qi)


def adversarial_queries(qv: np.ndarray, d: int) -> np.ndarray:
    """The query edits of test_bound_never_below_exact_minus_margin on a batch of at least 7 queries [Q, d gated + ungated]: one-hot
    (gated; ungated where there are such columns), zero, x 300 gated, x 300 ungated, fp32 values that are not fp16-representable,
    negative gated values."""
    q = qv.astype(np.float32).copy()
    q[0] = 0; q[0, min(17, d - 1)] = 2.5
    if q.shape[1] > d:
        q[1] = 0; q[1, d + min(9, q.shape[1] - d - 1)] = 1.5
        q[4, d:] *= 300
    q[2] = 0
    q[3, :d] *= 300
    q[5] *= np.float32(0.3)
    q[6, :d] = -np.abs(q[6, :d])
    return q
