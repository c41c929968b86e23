"""TEST INFRASTRUCTURE ONLY (see oracle/gip_oracle.py's header): numpy float64 restatement of the refine level of a gated index
(dhr_amd/csrc/kernels.hip: heavy_build_kernel writes a row's record, refine_kernel reads it), written from the comments of
kernels.hip and dhr_internal.h, not from the device code's arithmetic.  It has no counterpart in the reference
(retrieval/gip_retrieval.py:115-126 scores every row exactly): the search result never depends on it, only the number of rows
that reach the exact rescoring does.  What the level must keep is  exact score - margin <= U2 <= U.

Record of a row: its HEAVY = 64 gated entries of largest |fp16 value|, heaviest first, ties toward the lower slice; a row with
fewer non-zero entries is padded.  Each listed entry carries its slice, its bucket, its index value and its value.

fp16 image of the gated half:   U2 = U - sum over the listed entries of the query's bucket whose index values differ of |q16_j d_j|
    (the bound counted every slice whose BUCKETS agree; a listed entry of the same bucket with another index value contributes
    nothing to the exact score).  q16_j: the query's bound operand, fp16(max(q_j, 0)), fp16(|q_j|) in abs mode.
int8 image (gated_i8):          U2 = U - unit_q * sum over the listed entries of the query's bucket with level > 0 of q8_j level_j
                                       + sum over those of them whose index values agree of q_j d_j       (|d_j| in abs mode)
    (the bound counted such an entry as q8_j level_j units; the entries whose index values agree contribute their real product,
    the others nothing).  q_j: the bound operand rounded UP to fp16, so that what is put back never falls below the real product.
    A plain inner-product batch (ungated): every listed entry counts and every one matches.
Index values are compared in their low 12 bits: values that differ only above bit 11 count as equal, which only loosens the bound.

U is an input (the device's own bound), so its rounding cancels in U - U2; levels, steps and the unit come from g8_bound_oracle
(the unit may be handed in instead: the device's carries ~1e-6 of deliberate head room, see that module's header).
"""
import numpy as np

from . import g8_bound_oracle as G8
from . import i8_bound_oracle as I8

HEAVY = 64


def select_records(cg: np.ndarray) -> np.ndarray:
    """cg: [N, D] gated values (any float dtype; their fp16 images are ranked) -> slices [N, HEAVY] int64, heaviest first, ties
    toward the lower slice, -1 where the row has fewer non-zero entries."""
    mag = np.abs(cg.astype(np.float16).astype(np.float64))
    n, d = mag.shape
    order = np.argsort(-mag, axis=1, kind="stable")[:, :HEAVY]                    # stable: equal magnitudes keep slice order
    if order.shape[1] < HEAVY:
        order = np.concatenate([order, np.zeros((n, HEAVY - order.shape[1]), np.int64)], axis=1)
    live = np.arange(HEAVY)[None, :] < (mag > 0).sum(axis=1)[:, None]           # the non-zero entries come first
    return np.where(live, order, -1)


def _half_up(x: np.ndarray) -> np.ndarray:
    """Non-negative float32 / float64 values rounded up to fp16 (as float64)."""
    h = x.astype(np.float16)
    low = h.astype(np.float64) < x.astype(np.float64)
    return np.where(low, np.nextafter(h, np.float16(np.inf)), h).astype(np.float64)


def _low12(idx) -> np.ndarray:
    return np.asarray(idx).astype(np.int64) & 0xFFF


def _operand(qg: np.ndarray, abs_mode: bool) -> np.ndarray:
    q = qg.astype(np.float64)
    return np.abs(q) if abs_mode else np.maximum(q, 0.0)


def _gather(a: np.ndarray, listed: np.ndarray) -> np.ndarray:
    return np.take_along_axis(a, np.maximum(listed, 0), axis=1)


def corr_fp16(qg, qi, cg, ci, *, abs_mode=False, bucket_q=None, bucket_d=None, listed=None) -> np.ndarray:
    """[Q, N] what the refine level of the fp16 image takes off the bound.  bucket_q [Q, D] / bucket_d [N, D]: the bucket of every
    (query, slice) / (row, slice); default: one bucket."""
    listed = select_records(cg) if listed is None else listed
    live = listed >= 0
    d = _gather(cg.astype(np.float16).astype(np.float64), listed)
    ci12 = _gather(_low12(ci), listed)
    out = np.empty((qg.shape[0], cg.shape[0]))
    for q in range(qg.shape[0]):
        q16 = _operand(qg[q], abs_mode).astype(np.float16).astype(np.float64)
        use = live & (_low12(qi[q])[np.maximum(listed, 0)] != ci12)
        if bucket_q is not None:
            use &= bucket_q[q][np.maximum(listed, 0)] == _gather(bucket_d, listed)
        out[q] = (np.abs(q16[np.maximum(listed, 0)] * d) * use).sum(axis=1)
    return out


def corpus_levels(cg: np.ndarray):
    """-> (level [N, D], step [D], w [D], s_ref): the int8 operand level of every gated corpus entry (g8_bound_oracle)."""
    step, w, s_ref = G8.corpus_steps(cg)
    return G8.corpus_image(cg, step), step, w, s_ref


def query_levels(qg, qd, cg, cd, *, abs_mode=False):
    """-> (q8 [Q, D], unit [Q]): the int8 operand levels of the gated query values and the score units of one operand product."""
    _, _, w, s_ref = corpus_levels(cg)
    has_u = cd is not None and cd.shape[1] > 0
    if has_u:
        _, cs, sc, _, _ = I8.corpus_image(cd)
    q8, unit = np.empty(qg.shape), np.empty(qg.shape[0])
    for q in range(qg.shape[0]):
        r = G8.query_units(qg[q], qd[q] if has_u else None, w, s_ref, cs if has_u else None, sc if has_u else 0.0, abs_mode)
        q8[q], unit[q] = r["q8"], r["u"]
    return q8, unit


def corr_g8(qg, qi, qd, cg, ci, cd, *, abs_mode=False, ungated=False, bucket_q=None, bucket_d=None, unit=None, listed=None):
    """[Q, N] U - U2 of the int8 image: (taken * unit - back, taken [Q, N] integer units, back [Q, N]).  unit [Q]: the score units
    of one operand product where the caller knows the device's; default: g8_bound_oracle's."""
    listed = select_records(cg) if listed is None else listed
    live = listed >= 0
    level, _, _, _ = corpus_levels(cg)
    q8, unit_ref = query_levels(qg, qd, cg, cd, abs_mode=abs_mode)
    unit = unit_ref if unit is None else np.asarray(unit, np.float64)
    lv = _gather(level, listed)
    d16 = cg.astype(np.float16).astype(np.float64)
    d = _gather(np.abs(d16) if abs_mode else d16, listed)
    ci12 = _gather(_low12(ci), listed)
    taken, back = np.empty((qg.shape[0], cg.shape[0])), np.empty((qg.shape[0], cg.shape[0]))
    at = np.maximum(listed, 0)
    for q in range(qg.shape[0]):
        counts = live & (lv > 0)
        if not ungated and bucket_q is not None:
            counts &= bucket_q[q][at] == _gather(bucket_d, listed)
        agree = counts if ungated else counts & (_low12(qi[q])[at] == ci12)
        taken[q] = (q8[q][at] * lv * counts).sum(axis=1)
        back[q] = (_half_up(_operand(qg[q], abs_mode).astype(np.float32))[at] * d * agree).sum(axis=1)
    return taken * unit[:, None] - back, taken, back


def borderline_corpus(cg: np.ndarray, rel: float = 1e-4) -> np.ndarray:
    """[N, D] bool: entries whose |d| / step lies within `rel` (relative) of a rounding boundary of the int8 level, so that an
    arithmetic with ~1e-6 of head room may come out one level apart.  (A boundary beyond the last level is none: both sides clamp.)"""
    step, _, _ = G8.corpus_steps(cg)
    x = np.abs(cg.astype(np.float64)) / step[None, :] * (1.0 + 1e-6)
    return np.minimum(np.ceil(x * (1.0 - rel)), 127.0) != np.minimum(np.ceil(x * (1.0 + rel)), 127.0)


def borderline_queries(qg, qd, cg, cd, *, abs_mode=False, rel: float = 1e-4) -> np.ndarray:
    """[Q, D] bool: the same for the query's int8 levels."""
    _, _, w, s_ref = corpus_levels(cg)
    _, unit = query_levels(qg, qd, cg, cd, abs_mode=abs_mode)
    x = _operand(qg, abs_mode) * w[None, :] / (unit[:, None] / s_ref) * (1.0 + 1e-6)
    return np.minimum(np.ceil(x * (1.0 - rel)), 255.0) != np.minimum(np.ceil(x * (1.0 + rel)), 255.0)
