"""Exact rescoring of wide rows (rescore_fast_kernel and its whole-row-in-flight instances, kernels.hip): the VALUE of every score, bit for bit,
against a numpy float64 restatement of the sum that shares no code with the library.

The sum of a (query, row) pair is defined by its order: the row is cut into chunks of 8 columns; lane l of a 64-lane wave adds, in float64, the
products of the chunks l, l + 64, l + 128, ... in that order and inside a chunk in column order (products of two fp16 values are exact in
float32 and in float64); the 64 partial sums are combined by the xor butterfly v = v + v[lane ^ o] for o = 32, 16, ..., 1; lane 0 is rounded
to float32 once.  A gated column (the first d_dlr) counts only where the corpus and the query index values agree.

The restatement stands on its own: test_restatement_is_the_exact_sum (CPU) holds it against math.fsum of the same products on fp16 values with
exponents spread over 2^-14 ... 2^14 -- the float32 result is the correctly rounded exact sum in every pair, although the float64 sum itself
depends on the chunk order there.  So the comparison pins the value on every shape with no pair left out and no tolerance; it cannot tell
two summation orders apart (that is what the checksum comparisons between builds are for).

score_rows reaches the kernel through the rows32 list and the 2-D grid; the candidate-list / flat form is what every search test runs."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def restated_scores(qv, qi, cv, ci, rows):
    """float32 [Q, m]: the sum spelled out above for query i against corpus rows rows[i, :] (all inside the corpus)."""
    nq, m = rows.shape
    k = qv.shape[1]
    d_dlr = 0 if ci is None else ci.shape[1]
    assert k % 8 == 0 and d_dlr % 8 == 0
    nch = k // 8
    passes = (nch + 63) // 64
    d = cv[rows].astype(np.float64)                                   # [Q, m, k]
    prod = d * qv.astype(np.float64)[:, None, :]                      # exact: 22 significant bits at most
    if d_dlr:
        agree = ci[rows].astype(np.int64) == qi.astype(np.int64)[:, None, :]
        prod[:, :, :d_dlr] = np.where(agree, prod[:, :, :d_dlr], 0.0)
    prod = prod.reshape(nq, m, nch, 8)
    acc = np.zeros((nq, m, 64), np.float64)
    for t in range(passes):
        live = min(64, nch - 64 * t)                                  # lanes past the row's end add nothing
        for e in range(8):
            acc[:, :, :live] = acc[:, :, :live] + prod[:, :, 64 * t:64 * t + live, e]
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[:, :, lanes ^ o]
    return acc[:, :, 0].astype(np.float32)


def _synth_case(seed, n, nq, d_dlr, d_cls, idx_dtype):
    from dhr_amd import synth
    cv, ci, qv, qi = synth.make_pair(seed, n, nq, d_dlr, d_cls)
    if idx_dtype == np.int8:                                          # the same bytes read as signed: agreement is unchanged
        ci, qi = ci.view(np.int8), qi.view(np.int8)
    return cv, ci, qv, qi


def _wide_exponent_case(seed, n, nq, d_dlr, d_cls):
    """fp16 values with exponents spread over 2^-14 ... 2^14 and random signs (finite in fp16; a score is below 1536 * 2^30, finite in fp32),
    index values 0 / 1 so that about half of the gated columns count."""
    rng = np.random.Generator(np.random.PCG64(seed))
    k = d_dlr + d_cls

    def vals(rows):
        mant = rng.uniform(1.0, 2.0, (rows, k))
        return (np.ldexp(mant, rng.integers(-14, 15, (rows, k))) * rng.choice([-1.0, 1.0], (rows, k))).astype(np.float16)
    cv, qv = vals(n), vals(nq)
    assert np.isfinite(cv).all() and np.isfinite(qv).all()
    return cv, rng.integers(0, 2, (n, d_dlr)).astype(np.uint8), qv, rng.integers(0, 2, (nq, d_dlr)).astype(np.uint8)


# (d_dlr, d_cls, index dtype): chunks per lane / gated passes of the kernel instance the width selects
SHAPES = [
    pytest.param(768, 768, np.uint8, id="768+768-u8"),         # 192 chunks: 3 per lane; chunk pass 1 gated in lanes 0-31 only
    pytest.param(768, 320, np.uint8, id="768+320-u8"),         # 136 chunks: 3 per lane, lanes 8-63 idle in the last pass
    pytest.param(1024, 768, np.int8, id="1024+768-i8"),        # 224 chunks: 4 per lane, two full gated passes
    pytest.param(320, 1024, np.int8, id="320+1024-i8"),        # 168 chunks; 40 gated chunks: a gated half that is no multiple of 512 columns
    pytest.param(1000, 768, np.uint8, id="1000+768-u8"),       # 221 chunks: 4 per lane with idle lanes; 125 gated chunks
    pytest.param(768, 1536, np.uint8, id="768+1536-u8"),       # 288 chunks: 5 per lane -> the loop form of the kernel
]


def _rows_for(rng, n, nq, m):
    rows = rng.integers(0, n, (nq, m)).astype(np.int64)
    rows[:, -1] = n - 1                                               # the last rows of the corpus
    rows[:, -2] = n - 2
    rows[0, 0] = n - 1
    return rows


def _check(cv, ci, qv, qi, m, seed):
    from dhr_amd.retrieval.gip_retrieval import GipIndex
    n, nq = cv.shape[0], qv.shape[0]
    rows = _rows_for(np.random.Generator(np.random.PCG64(seed)), n, nq, m)
    want = restated_scores(qv, qi, cv, ci, rows)
    assert np.isfinite(want).all()
    ask = rows.copy()
    ask[1, 3] = n + 5                                                 # a row number outside the index: -inf, no memory touched
    want[1, 3] = -np.inf
    ix = GipIndex(cv, ci)
    try:
        got = ix.score_rows(qv.astype(np.float32), qi, ask)           # fp32 queries that are fp16-representable: the fast kernels take them
    finally:
        ix.close()
    fin = np.isfinite(want) & np.isfinite(got)
    print("pairs %d  differing %d  max |got - want| %g" % (want.size, int((got != want).sum()), float(np.abs(got[fin].astype(np.float64) - want[fin]).max())))
    np.testing.assert_array_equal(got, want)


@pytest.mark.gpu
@pytest.mark.parametrize("d_dlr,d_cls,idx_dtype", SHAPES)
@pytest.mark.parametrize("m", [41, 7])                                # pairs per query: no multiple of 32 (a block), of 4 (the waves) or of the rows in flight
def test_scores_bit_for_bit(d_dlr, d_cls, idx_dtype, m):
    cv, ci, qv, qi = _synth_case(4242, 2000, 8, d_dlr, d_cls, idx_dtype)
    _check(cv, ci, qv, qi, m, 99)


@pytest.mark.gpu
@pytest.mark.parametrize("d_dlr,d_cls", [(768, 768), (1024, 768), (768, 320)])
def test_scores_wide_exponents(d_dlr, d_cls):
    cv, ci, qv, qi = _wide_exponent_case(777, 2000, 8, d_dlr, d_cls)
    _check(cv, ci, qv, qi, 41, 100)


def test_restatement_is_the_exact_sum():
    """CPU: the restatement against math.fsum of the same products (the exact sum, rounded once), so the GPU test leans on nothing but it."""
    import math
    cv, ci, qv, qi = _wide_exponent_case(778, 64, 4, 768, 768)
    rows = _rows_for(np.random.Generator(np.random.PCG64(5)), 64, 4, 9)
    got = restated_scores(qv, qi, cv, ci, rows)
    for i in range(4):
        for j in range(9):
            p = cv[rows[i, j]].astype(np.float64) * qv[i].astype(np.float64)
            p[:768] = np.where(ci[rows[i, j]] == qi[i], p[:768], 0.0)
            assert got[i, j] == np.float32(math.fsum(p))


def test_wide_instances_use_no_scratch():
    """CPU: compile kernels.hip to gfx950 assembly and read the kernels' metadata: no instance of the wide fast kernel spills, and the one the
    768 + 768 layout runs fits the 72 registers of 7 waves per SIMD."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "kernels.s")
        csrc = os.path.join(ROOT, "dhr_amd", "csrc")
        subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", "-I" + os.path.join(ROOT, "include"), "-I" + csrc,
                        os.path.join(csrc, "kernels.hip"), "-o", out], check=True, stderr=subprocess.DEVNULL)
        text = open(out).read()
    found = {}
    for blk in text.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        if "rescore_fast_kernel" in name:
            found[name] = (int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1)), int(re.search(r"\.vgpr_count:\s+(\d+)", blk).group(1)),
                           int(re.search(r"\.vgpr_spill_count:\s+(\d+)", blk).group(1)))
    wide = {k: v for k, v in found.items() if "rescore_fast_kernel_wide" in k}
    assert len(wide) == 9 and len(found) == 10, sorted(found)
    for name, (scratch, vgprs, spills) in found.items():
        assert scratch == 0 and spills == 0 and vgprs <= 128, (name, scratch, vgprs, spills)
    (cfg3,) = [v for k, v in wide.items() if "ILi3ELi2E" in k]
    assert cfg3[1] <= 72, cfg3
