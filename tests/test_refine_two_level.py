"""The two-level refine kernel (kernels.hip: level 1 reads line 1 of a row's heavy record = its 20 heaviest entries, compacts the
survivors in LDS, level 2 reads lines 2-3 for those only) against the oracle, on the shapes that reach every branch of it: both images
of the gated half, an abs_mode corpus, a gated half wider than 1 024 slices, and rows with fewer than 20 / fewer than 64 non-zero gated
values (padded records, padding inside line 1).

Results equal the oracle as in test_gpu_parity.py.  Besides, the refine level must keep what the one-level kernel kept and no more:
`candidates_exact` (the rows that reach exact rescoring) is compared with the figure of the SAME call measured on the parent commit
(one-level kernel, all 64 entries in one pass), recorded below as constants.

The survivor SET is meant to be the same.  What can differ is the rounding of a borderline bound: the one-level kernel summed a
candidate's corrections as 8 lanes x 8 entries and a 3-step butterfly, the two-level kernel sums 4 x 5 and 4 x 11 entries and adds the two
levels.  gated_i8: the sums are fp64 (products of two fp16 values are exact there, a sum of 64 of them in this value range almost always
is), and the result is rounded up to fp32 once, so a difference needs a tie within 2^-53 relative: not expected at all.  gated_fp16:
`corr` is an fp32 sum of up to 64 terms, the order of which moves u2 by an ulp or two, so a candidate within ~2^-22 relative of the
threshold can change sides.  With thresholds in the bulk of a smooth score distribution that is a few per million candidates, in either
direction.  The bound used for both images: 5 per million bound candidates, rounded up -- it is not loosened further."""
import math

import numpy as np
import pytest

from oracle import gip_oracle as O

pytestmark = pytest.mark.gpu

# stats()["candidates_exact"] of each call below on the parent commit (one-level refine_kernel), measured on an MI355X with this file's own
# corpora; not computed by the code under test.
PARENT_CANDIDATES_EXACT = {
    ("big", "gated_i8"): 15220,
    ("big", "gated_fp16"): 11336,
    ("abs_mode", "gated_i8"): 60685,
    ("abs_mode", "gated_fp16"): 57228,
    ("wide", "gated_i8"): 20123,
    ("wide", "gated_fp16"): 15629,
    ("short_rows", "gated_i8"): 14655,
    ("short_rows", "gated_fp16"): 14157,
}
PER_MILLION = 5


def _corpus(kind):
    from dhr_amd import synth
    if kind == "big":              # at least 200 k rows x 768 + 768
        cv, ci, qv, qi = synth.make_pair(4242, 200_000, 24, 768, 768)
        return cv, ci, qv.astype(np.float32), qi, 100, range(0, 24, 4)
    if kind == "abs_mode":         # negative gated values on both sides: the index is built in abs_mode
        cv, ci, qv, qi = synth.make_pair(4243, 30_000, 16, 768, 64)
        rng = np.random.default_rng(1)
        cv = cv.copy(); qv = qv.copy()
        cv[:, :768] *= rng.choice([-1, 1], size=(30_000, 768)).astype(np.float16)
        qv[:, :768] *= rng.choice([-1, 1], size=(16, 768)).astype(np.float16)
        return cv, ci, qv.astype(np.float32), qi, 50, range(16)
    if kind == "wide":             # gated half wider than 1 024 slices (heavy_build_kernel<64>, 16 KB of query words per workgroup)
        cv, ci, qv, qi = synth.make_pair(4244, 20_000, 12, 2048, 64)
        return cv, ci, qv.astype(np.float32), qi, 100, range(12)
    if kind == "short_rows":       # a third of the rows with 0 .. 19 non-zero gated values, a third with 20 .. 63, a third full
        n = 30_000
        cv, ci, qv, qi = synth.make_pair(4245, n, 16, 768, 64)
        rng = np.random.default_rng(2)
        keep = np.where(np.arange(n) % 3 == 0, rng.integers(0, 20, n), np.where(np.arange(n) % 3 == 1, rng.integers(20, 64, n), 768))
        g = cv[:, :768].astype(np.float32)
        rank = np.argsort(np.argsort(-g, axis=1, kind="stable"), axis=1, kind="stable")
        cv = cv.copy()
        cv[:, :768] = np.where(rank < keep[:, None], g, 0).astype(np.float16)
        return cv, ci, qv.astype(np.float32), qi, 50, range(16)
    raise ValueError(kind)


@pytest.mark.parametrize("kind", ["big", "abs_mode", "wide", "short_rows"])
def test_two_level_refine(kind, gated_image):
    from dhr_amd import _lib
    from dhr_amd.retrieval.gip_retrieval import GipIndex
    cv, ci, q32, qi, k, queries = _corpus(kind)
    ix = GipIndex(cv, ci)
    assert ix.info(_lib.INFO_GATED_I8) == (1 if gated_image == "gated_i8" else 0)
    ix.set_param(_lib.PARAM_PROFILE, 1)
    # refine / rescoring of a chunk behind its own bound GEMM, not beside the next one: the running thresholds that later chunks filter
    # with, and with them both candidate counts, then do not depend on how the two streams happen to interleave
    ix.set_param(_lib.PARAM_OVERLAP_AUX, 0)
    scores, rows = ix.search(q32, qi, k)
    st = ix.stats()
    ix.close()
    parent = PARENT_CANDIDATES_EXACT[(kind, gated_image)]
    print("refine_two_level %s %s: candidates_bound %d candidates_exact %d (parent %s)" % (kind, gated_image, st["candidates_bound"], st["candidates_exact"], parent))
    c32 = cv.astype(np.float32)
    for i in queries:
        ex = O.gip_scores_f64(q32[i], qi[i], c32, ci)
        O.check_topk(rows[i, :k], scores[i, :k], ex, k)
        np.testing.assert_allclose(scores[i, :k], ex[rows[i, :k]].astype(np.float32), rtol=0, atol=1e-6 * max(1.0, np.abs(ex).max()))
    if kind == "big":            # the refine level ran and pruned (small corpora: several phases, rows counted once per phase)
        assert st["candidates_exact"] < st["candidates_bound"] // 2
    assert st["candidates_exact"] <= parent + math.ceil(PER_MILLION * 1e-6 * st["candidates_bound"])
