"""The fused lexical head (dhr_amd/lexical.py, dhr_amd/csrc/lexical.hip) against the reference's own encoder code (tests/golden/lexical_golden.npz,
made by tests/golden/make_golden_lexical.py), a float64 restatement kept here, and the torch composition on the same device.

Tolerance rule (every comparison below):
  - fp32 reps: within 1e-5 * |ref| + 1e-30 of the torch composition (and of the float64 truth);
  - fp16 record values: bit-equal, except where the fp32 reference lies within that tolerance of an fp16 rounding midpoint;
  - group indices: equal, except where the two best candidates of a slice lie within the tolerance;
  - exemptions are counted: zero on the goldens, below 5e-4 of the entries on random data.  (Two fp32 evaluations that differ by one ulp
    round to different fp16 values with probability ulp32 / ulp16 = 2^-13 .. 2^-12, 1.2e-4 .. 2.4e-4 per ulp: the torch composition sums
    the softmax normaliser in its own order, so a bound of 1e-4 would sit below that floor -- measured: 7 in 45 448 entries, 1.5e-4);
  - signs of zero are compared bit for bit wherever every contribution is zero.
CPU part: the fixture agrees with the float64 restatement; the new entry points return statuses, not crashes, on bad arguments and without
a device.  GPU part (-m gpu): goldens, random shapes / strided [:, 1:] views / fp16 and fp32 inputs / all three modes into wider record
rows, top-k parity of searches over records built both ways, one timing printout."""
import os

import numpy as np
import pytest

from dhr_amd import _lib
from dhr_amd import lexical as LX

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lexical_golden.npz")
CASES = ("prod", "small", "neg", "pad")
RTOL, ATOL = 1e-5, 1e-30


# ------------------------------------------------------------------------------------------ float64 restatement
def _first_max(stack):
    """max over axis 1 of [B, n, ...], the first entry on ties (torch.max on the device / the reference on the CPU)."""
    r = stack[:, 0].copy()
    for i in range(1, stack.shape[1]):
        r = np.where(stack[:, i] > r, stack[:, i], r)
    return r


def _first_argmax(stack):
    r, a = stack[:, 0].copy(), np.zeros(stack[:, 0].shape, np.int64)
    for i in range(1, stack.shape[1]):
        up = stack[:, i] > r
        r, a = np.where(up, stack[:, i], r), np.where(up, i, a)
    return r, a


def contributions_f64(logits, w, mask):
    """[B, T, V] float64 (softmax(logits) * w) * mask; softmax over the whole vocabulary."""
    x = logits.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        x = x - x.max(-1, keepdims=True)
        e = np.exp(x)
        p = e / e.sum(-1, keepdims=True)
    p = np.where(np.isnan(p), 0.0, p)                   # (masked rows may be all -inf; they never reach the max with a non-zero)
    return (p * w.astype(np.float64)[..., None]) * mask.astype(np.float64)[..., None]


def reps_f64(logits, w, mask):
    c = contributions_f64(logits, w, mask)
    return _first_max(c), np.all(c == 0, axis=1)        # reps, "every contribution is zero"


def densify_f64(reps, dims, remove):
    B = reps.shape[0]
    return _first_argmax(reps[:, remove:].reshape(B, -1, dims))


def aggregate_f64(reps, dims, full):
    B, V = reps.shape
    if full:
        remove = LX.cal_remove_dim(2 * dims)
        r = np.concatenate([reps, np.zeros((B, -remove), reps.dtype)], 1) if remove < 0 else reps[:, remove:]
        tok = _first_max(r.reshape(B, -1, 2 * dims))
        pos, neg = tok[:, 0::2], tok[:, 1::2]
        return pos * (pos > neg) - neg * (pos <= neg)
    return _first_max(reps[:, LX.cal_remove_dim(dims):].reshape(B, -1, dims))


# ------------------------------------------------------------------------------------------ tolerance rule
def _tol(ref):
    return RTOL * np.abs(ref.astype(np.float64)) + ATOL


def check_f32(got, ref, what):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    bad = ~(np.abs(got - ref) <= _tol(ref))
    assert not bad.any(), f"{what}: {bad.sum()} entries outside the tolerance, e.g. {got[bad][:4]} vs {ref[bad][:4]}"


def check_zero_signs(got, ref, zero, what):
    g, r = np.asarray(got, np.float32)[zero], np.asarray(ref, np.float32)[zero]
    assert np.array_equal(g.view(np.uint32), r.view(np.uint32)), f"{what}: signs of zero differ"


def fp16_exemptions(got16, ref32, what):
    """-> exempt entries; fails on a difference that is not within the tolerance of an fp16 rounding midpoint."""
    got16 = np.asarray(got16, np.float16)
    ref = np.asarray(ref32, np.float32).astype(np.float64)
    want = ref.astype(np.float16)
    diff = got16.view(np.uint16) != want.view(np.uint16)
    lo, hi = (ref - _tol(ref)).astype(np.float16), (ref + _tol(ref)).astype(np.float16)
    near = lo.view(np.uint16) != hi.view(np.uint16)
    ok = (got16.view(np.uint16) == lo.view(np.uint16)) | (got16.view(np.uint16) == hi.view(np.uint16))
    bad = diff & ~(near & ok)
    assert not bad.any(), f"{what}: {bad.sum()} fp16 values differ, e.g. {got16[bad][:4]} vs {want[bad][:4]}"
    return int((diff & near).sum())


def index_exemptions(got, ref_reps, dims, remove, what):
    groups = np.asarray(ref_reps, np.float64)[:, remove:].reshape(ref_reps.shape[0], -1, dims)
    _, want = _first_argmax(groups)
    diff = np.asarray(got, np.int64) != want
    top2 = -np.sort(-groups, axis=1)[:, :2] if groups.shape[1] > 1 else np.concatenate([groups, groups - np.inf], 1)
    near = np.abs(top2[:, 0] - top2[:, 1]) <= _tol(top2[:, 0])
    bad = diff & ~near
    assert not bad.any(), f"{what}: {bad.sum()} group indices differ"
    return int(diff.sum())


def _golden():
    return np.load(GOLDEN)


# ------------------------------------------------------------------------------------------ CPU part
def test_fixture_matches_float64_restatement():
    g = _golden()
    for name in CASES:
        lg, w, m = g[name + "_logits"][:, 1:], g[name + "_w"], g[name + "_mask"][:, 1:]
        ref, zero = reps_f64(lg, w, m)
        rep = g[name + "_reps"]
        check_f32(rep, ref, name)
        assert zero.any() or name in ("prod", "pad")
        check_zero_signs(rep, ref, zero, name)
        # the epilogues are selections: exact on the reference's own reps
        if name + "_dval" in g:
            dims, remove, _ = (int(v) for v in g[name + "_geom"])
            v, i = densify_f64(rep.astype(np.float64), dims, remove)
            assert np.array_equal(v.astype(np.float32).view(np.uint32), g[name + "_dval"].view(np.uint32))
            assert np.array_equal(i, g[name + "_didx"])
        agg = 640 if name == "prod" else 700 if name == "pad" else 8
        for full, tag in ((True, "_afull"), (False, "_asemi")):
            a = aggregate_f64(rep.astype(np.float64), agg, full).astype(np.float32)
            assert np.array_equal(a.view(np.uint32), g[name + tag].view(np.uint32)), (name, tag)
    # the cases cover what the issue lists
    assert (g["small_mask"][3, 1:] == 0).all() and (g["neg_w"] < 0).all() and np.isneginf(g["small_logits"]).any()


def test_cal_remove_dim_and_aggregate_errors_match_reference():
    assert [LX.cal_remove_dim(d) for d in (768, 640, 512, 256, 128)] == [570, 442, 314, 58, 58]
    assert [LX.cal_remove_dim(2 * d) for d in (768, 640)] == [-198, -198]
    errs = [str(e) for e in _golden()["errors"]]
    with pytest.raises(ValueError) as e:
        LX.densify_lexical_into(np.zeros((2, 1, 30), np.float16), np.zeros((2, 1)), np.ones((2, 1)), np.zeros((2, 7), np.float16),
                                np.zeros((2, 7), np.uint8), dims=7, remove_dims=1)
    assert "ValueError: " + str(e.value) == errs[0]
    for (V, dims, full), want in zip(((1000, 640, True), (1000, 8, True), (1000, 8, False), (5, 8, False)), errs[1:]):
        with pytest.raises(RuntimeError) as e:
            LX.aggregate(np.zeros((2, V), np.float32), dims, full=full)
        assert "RuntimeError: " + str(e.value) == want
    with pytest.raises(ValueError, match="negative"):                   # cal_remove_dim(1400) = -278: the semi view never exists
        LX.aggregate(np.zeros((2, 1400), np.float32), 1400, full=False)


def _head(lib, **kw):
    a = dict(device=0, mem_kind=_lib.MEM_HOST, mode=_lib.LEX_DENSIFY, logits=None, value_dtype=_lib.VAL_F16, batch=2, n_tokens=3, vocab=32,
             ld_batch=96, ld_token=32, w=None, ld_w=3, m=None, ld_m=3, dims=8, remove=0, val=None, val_dtype=_lib.VAL_F16, ld_val=8, idx=None,
             idx_dtype=_lib.IDX_U8, ld_idx=8, cls=None, cls_dtype=_lib.VAL_F16, ld_cls=0, cls_dim=0, ws=None, stream=None)
    a.update(kw)
    return lib.dhr_lexical_head(*a.values())


def test_entry_points_return_statuses():
    import torch
    lib = _lib.load()
    lg = np.zeros((2, 3, 32), np.float16)
    w, m = np.ones((2, 3), np.float32), np.ones((2, 3), np.float32)
    val, idx = np.zeros((2, 8), np.float16), np.zeros((2, 8), np.uint8)
    good = dict(logits=lg.ctypes.data, w=w.ctypes.data, m=m.ctypes.data, val=val.ctypes.data, idx=idx.ctypes.data)
    bad = [dict(logits=None), dict(mem_kind=7), dict(mode=9), dict(value_dtype=5), dict(n_tokens=0), dict(ld_token=31), dict(ld_batch=60),
           dict(ld_w=2), dict(dims=7), dict(dims=0), dict(remove=-2), dict(ld_val=7), dict(idx=None), dict(idx_dtype=_lib.IDX_I8), dict(ld_idx=4),
           dict(cls_dim=4), dict(batch=-1)]
    for b in bad:
        assert _head(lib, **{**good, **b}) == _lib.ERR_INVALID, b
    assert _head(lib, **{**good, "dims": 7}) == _lib.ERR_INVALID and b"densified" in lib.dhr_last_error()
    assert _head(lib, **{**good, "batch": 0}) == _lib.DHR_OK
    reps, out = np.zeros((2, 32), np.float32), np.zeros((2, 8), np.float32)
    assert lib.dhr_aggregate(0, _lib.MEM_HOST, None, _lib.VAL_F32, 32, 2, 32, 8, 0, 1, out.ctypes.data, _lib.VAL_F32, 8, None) == _lib.ERR_INVALID
    assert lib.dhr_aggregate(0, _lib.MEM_HOST, reps.ctypes.data, _lib.VAL_F32, 32, 2, 32, 8, 1, 1, out.ctypes.data, _lib.VAL_F32, 8, None) == _lib.ERR_INVALID
    assert lib.dhr_aggregate(0, _lib.MEM_HOST, reps.ctypes.data, _lib.VAL_F32, 32, 2, 32, 8, -8, 0, out.ctypes.data, _lib.VAL_F32, 8, None) == _lib.ERR_INVALID
    # valid calls: a status without a device, the result with one
    rc_h = _head(lib, **good)
    rc_a = lib.dhr_aggregate(0, _lib.MEM_HOST, reps.ctypes.data, _lib.VAL_F32, 32, 2, 32, 8, 0, 1, out.ctypes.data, _lib.VAL_F32, 8, None)
    want = _lib.DHR_OK if torch.cuda.is_available() else _lib.ERR_HIP
    assert rc_h == want and rc_a == want, (rc_h, rc_a)
    if not torch.cuda.is_available():
        with pytest.raises(_lib.DhrError, match="dhr_lexical_head failed"):
            LX.lexical_reps(lg, w, m)


# ------------------------------------------------------------------------------------------ GPU part
def _torch_reps(logits, w, mask):
    """The reference's composition on the device, with autocast's dtypes: fp32 softmax, fp16/fp32 weights [B, T, 1], integer mask [B, T, 1]."""
    import torch
    p = torch.softmax(logits.float(), dim=-1)
    return torch.max((p * w) * mask, dim=-2).values


def _torch_densify(reps, dims, remove):
    B = reps.shape[0]
    return reps[:, remove:].reshape(B, -1, dims).max(1)


def _torch_aggregate(reps, dims, full):
    import torch
    B = reps.shape[0]
    if full:
        remove = LX.cal_remove_dim(2 * dims)
        r = torch.cat([reps, reps.new_zeros(B, -remove)], 1) if remove < 0 else reps[:, remove:]
        tok = r.reshape(B, -1, 2 * dims).max(1).values
        pos, neg = tok[:, 0::2], tok[:, 1::2]
        return pos * (pos > neg) - neg * (pos <= neg)
    return reps[:, LX.cal_remove_dim(dims):].reshape(B, -1, dims).max(1).values


@pytest.mark.gpu
def test_goldens_on_gpu():
    import torch
    g = _golden()
    for name in CASES:
        full_lg, w, mk = g[name + "_logits"], g[name + "_w"], g[name + "_mask"]
        ref, zero = g[name + "_reps"], reps_f64(full_lg[:, 1:], w, mk[:, 1:])[1]
        cls = g[name + "_cls"]
        B, V = ref.shape
        dl = torch.from_numpy(full_lg).cuda()[:, 1:]                       # the strided view of the model's [B, L, V] logits
        dw, dm = torch.from_numpy(w).cuda(), torch.from_numpy(mk).cuda()[:, 1:]
        for tag, lg_in, w_in, m_in in (("device", dl, dw, dm), ("host", full_lg[:, 1:], w, mk[:, 1:])):
            rep = LX.lexical_reps(lg_in, w_in, m_in)
            rep = rep.cpu().numpy() if tag == "device" else rep
            check_f32(rep, ref, f"{name} reps ({tag})")
            check_zero_signs(rep, ref, zero, f"{name} reps ({tag})")
        if name + "_dval" in g:
            dims, remove, _ = (int(v) for v in g[name + "_geom"])
            rv = torch.full((B, dims + cls.shape[1] + 5), 7.0, dtype=torch.float16, device="cuda")
            ri = torch.full((B, dims + 3), 99, dtype=torch.uint8, device="cuda")
            LX.densify_lexical_into(dl, dw, dm, rv[:, :dims + cls.shape[1]], ri[:, :dims], dims, remove, semantic_reps=torch.from_numpy(cls).cuda())
            ref32 = np.concatenate([g[name + "_dval"], cls], 1)
            assert fp16_exemptions(rv[:, :dims + cls.shape[1]].cpu().numpy(), ref32, name) == 0
            assert np.array_equal(ri[:, :dims].cpu().numpy(), g[name + "_drec_i"])
            assert (rv[:, dims + cls.shape[1]:] == 7).all() and (ri[:, dims:] == 99).all()   # nothing beyond the record columns
            hv, hi = np.zeros((B, dims + cls.shape[1]), np.float16), np.zeros((B, dims), np.uint8)
            LX.densify_lexical_into(full_lg[:, 1:], w, mk[:, 1:], hv, hi, dims, remove, semantic_reps=cls)
            assert np.array_equal(hv.view(np.uint16), g[name + "_drec_v"].view(np.uint16)) and np.array_equal(hi, g[name + "_drec_i"])
        agg = 640 if name == "prod" else 700 if name == "pad" else 8
        for full, key in ((True, "_afull"), (False, "_asemi")):
            rec = g[name + key + "_rec"]
            av = torch.zeros((B, agg + cls.shape[1]), dtype=torch.float16, device="cuda")
            LX.aggregate_lexical_into(dl, dw, dm, av, agg, full=full, semantic_reps=torch.from_numpy(cls).cuda())
            assert np.array_equal(av.cpu().numpy().view(np.uint16), rec.view(np.uint16)), (name, key)
            a32 = LX.aggregate(torch.from_numpy(ref).cuda(), agg, full=full).cpu().numpy()     # the standalone twin on the same kernel
            assert np.array_equal(a32.view(np.uint32), g[name + key].view(np.uint32)), (name, key)
            assert np.array_equal(LX.aggregate(ref, agg, full=full).view(np.uint32), g[name + key].view(np.uint32))


@pytest.mark.gpu
def test_random_shapes_views_dtypes_and_modes():
    import torch
    gen = torch.Generator(device="cuda").manual_seed(7)
    entries = exempt = 0
    shapes = [(3, 9, 1082, 64, 58, 64, torch.float16, torch.float16), (4, 17, 4026, 64, 58, 64, torch.float32, torch.float32),
              (12, 9, 30522, 768, 570, 640, torch.float16, torch.float16), (5, 3, 202, 8, 2, 8, torch.float32, torch.float16)]
    for B, L, V, dims, remove, agg, ldt, wdt in shapes:
        full_lg = (torch.randn((B, L, V + 3), generator=gen, device="cuda") * 3).to(ldt)[:, :, 1:V + 1]   # batch, token AND column offsets
        lg = full_lg[:, 1:]
        w = torch.randn((B, L - 1, 1), generator=gen, device="cuda").to(wdt)
        mask = torch.ones((B, L - 1), dtype=torch.int32, device="cuda")
        mask[0, (L - 1) // 2:] = 0
        mask[-1, :] = 0
        zero = torch.zeros((B, V), dtype=torch.bool, device="cuda")
        zero[-1] = True
        ref = _torch_reps(lg, w, mask[..., None])
        rep = LX.lexical_reps(lg, w, mask)
        check_f32(rep.cpu().numpy(), ref.cpu().numpy(), f"reps {B}x{L}x{V} {ldt}")
        check_zero_signs(rep.cpu().numpy(), ref.cpu().numpy(), zero.cpu().numpy(), "reps")
        if V <= 4100:
            truth, _ = reps_f64(lg.float().cpu().numpy(), w[..., 0].float().cpu().numpy(), mask.cpu().numpy())
            check_f32(rep.cpu().numpy(), truth, "reps vs float64")
        refn = ref.cpu().numpy()
        cls = torch.randn((B, 24), generator=gen, device="cuda").to(wdt)
        for vdt in (torch.float16, torch.float32):
            rv = torch.zeros((B, dims + 24 + 8), dtype=vdt, device="cuda")
            ri = torch.zeros((B, dims + 8), dtype=torch.uint8, device="cuda")
            LX.densify_lexical_into(lg, w, mask, rv, ri, dims, remove, semantic_reps=cls)
            v, i = _torch_densify(ref, dims, remove)
            got = rv.cpu().numpy()
            if vdt == torch.float16:
                exempt += fp16_exemptions(got[:, :dims], v.cpu().numpy(), "densify values")
                entries += got[:, :dims].size
            else:
                check_f32(got[:, :dims], v.cpu().numpy(), "densify values fp32")
            assert np.array_equal(got[:, dims:dims + 24], cls.to(vdt).cpu().numpy())
            exempt += index_exemptions(ri[:, :dims].cpu().numpy(), refn, dims, remove, "densify groups")
            entries += B * dims
            for full in (True, False):
                av = torch.zeros((B, agg + 24), dtype=vdt, device="cuda")
                try:
                    want = _torch_aggregate(ref, agg, full)
                except RuntimeError:
                    with pytest.raises(RuntimeError):
                        LX.aggregate_lexical_into(lg, w, mask, av, agg, full=full, semantic_reps=cls)
                    continue
                LX.aggregate_lexical_into(lg, w, mask, av, agg, full=full, semantic_reps=cls)
                got = av.cpu().numpy()[:, :agg]
                if vdt == torch.float16:
                    exempt += fp16_exemptions(got, want.cpu().numpy(), "aggregate")
                    entries += got.size
                else:
                    check_f32(got, want.cpu().numpy(), "aggregate fp32")
    print(f"random: {exempt} exemptions in {entries} entries")
    assert exempt < 5e-4 * entries


@pytest.mark.gpu
def test_records_search_like_the_torch_composition():
    """Synthetic corpus + queries: records built by the fused op and by the torch composition followed by densify / aggregate give the same
    top-k rows through GipIndex (hybrid with --lamda 0.5, and --IP over aggregated records)."""
    import torch
    from dhr_amd import densify as DZ
    from dhr_amd.retrieval.gip_retrieval import GipIndex
    from oracle import gip_oracle as O
    gen = torch.Generator(device="cuda").manual_seed(11)
    V, dims, remove, agg, H = 4026, 64, 58, 64, 32

    def records(n, L):
        lg = (torch.randn((n, L, V), generator=gen, device="cuda") * 4).half()[:, 1:]
        w = torch.randn((n, L - 1, 1), generator=gen, device="cuda").half()
        mask = (torch.arange(L - 1, device="cuda")[None] < torch.randint(2, L, (n, 1), generator=gen, device="cuda")).long()
        cls = torch.randn((n, H), generator=gen, device="cuda").half()
        fv = torch.zeros((n, dims + H), dtype=torch.float16, device="cuda")
        fi = torch.zeros((n, dims), dtype=torch.uint8, device="cuda")
        LX.densify_lexical_into(lg, w, mask, fv, fi, dims, remove, semantic_reps=cls)
        fa = torch.zeros((n, agg), dtype=torch.float16, device="cuda")
        LX.aggregate_lexical_into(lg, w, mask, fa, agg, full=True)
        reps = _torch_reps(lg, w, mask[..., None])
        tv, ti = DZ.densify(reps, dims, remove_dims=remove)
        tvr = torch.cat([tv.half(), cls], 1)
        ta = _torch_aggregate(reps, agg, True).half()
        return (fv.cpu().numpy(), fi.cpu().numpy(), fa.cpu().numpy()), (tvr.cpu().numpy(), ti.to(torch.uint8).cpu().numpy(), ta.cpu().numpy())

    (cv, ci, ca), (tcv, tci, tca) = records(512, 24)
    (qv, qi, qa), (tqv, tqi, tqa) = records(16, 8)
    for a, b in ((cv, tcv), (ci, tci), (ca, tca), (qv, tqv), (qi, tqi), (qa, tqa)):
        assert (a != b).mean() < 1e-3
    k = 10
    q32, _ = O.prepare_queries(qv, qi, dims, 0.5)
    tq32, _ = O.prepare_queries(tqv, tqi, dims, 0.5)
    ix, tix = GipIndex(cv, ci), GipIndex(tcv, tci)
    s1, r1 = ix.search(q32, qi, k)
    s2, r2 = tix.search(tq32, tqi, k)
    ix.close(), tix.close()
    assert np.array_equal(r1, r2)
    ex = O.gip_scores_f64(q32[0], qi[0], cv.astype(np.float32), ci)
    O.check_topk(r1[0], s1[0], ex, k)
    ia, tia = GipIndex(ca), GipIndex(tca)
    s3, r3 = ia.search(qa.astype(np.float32), None, k)
    s4, r4 = tia.search(tqa.astype(np.float32), None, k)
    ia.close(), tia.close()
    assert np.array_equal(r3, r4)


@pytest.mark.gpu
def test_timing_printout():
    """Fused head (densify mode into fp16 records) vs the torch composition on the same fp16 logits: device events, warm-up, median of 10.
    A printout, not a threshold."""
    import torch
    V, dims, remove = 30522, 768, 570
    for B, L in ((128, 128), (128, 32)):
        full = torch.randn((B, L, V), device="cuda", dtype=torch.float16)
        lg = full[:, 1:]
        w = torch.randn((B, L - 1, 1), device="cuda", dtype=torch.float16)
        mask = torch.ones((B, L - 1), dtype=torch.long, device="cuda")
        rv = torch.empty((B, dims), dtype=torch.float16, device="cuda")
        ri = torch.empty((B, dims), dtype=torch.uint8, device="cuda")

        def fused():
            LX.densify_lexical_into(lg, w, mask, rv, ri, dims, remove)

        def composed():
            reps = _torch_reps(lg, w, mask[..., None])
            v, i = _torch_densify(reps, dims, remove)
            rv.copy_(v)
            ri.copy_(i)

        res = {}
        for name, fn in (("fused", fused), ("torch", composed)):
            for _ in range(3):
                fn()
            times = []
            for _ in range(10):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                times.append(e0.elapsed_time(e1))
            res[name] = float(np.median(times))
        nbytes = B * (L - 1) * V * 2
        print(f"lexical head B={B} L={L} fp16: fused {res['fused']:.3f} ms ({nbytes / res['fused'] / 1e9:.2f} TB/s of logits), "
              f"torch {res['torch']:.3f} ms ({nbytes / res['torch'] / 1e9:.2f} TB/s), {res['torch'] / res['fused']:.2f}x")
        del full
        torch.cuda.empty_cache()


@pytest.mark.gpu
def test_host_arrays_with_strides_match_the_device_path():
    """B = 2, T = 3, V = 32 logits as base[:, 1:, :32] of a [2, 4, 40] base (token stride > V), records and reps in wider rows: the staged host
    paths of dhr_lexical_head (all modes) and dhr_aggregate give the bits of the same views on the device."""
    import torch
    lib = _lib.load()
    rng = np.random.default_rng(11)
    base = (rng.standard_normal((2, 4, 40)) * 3).astype(np.float16)
    w, mk = rng.uniform(0.5, 2, (2, 3)).astype(np.float32), np.array([[1, 1, 0], [1, 1, 1]], np.int64)
    cls = rng.standard_normal((2, 7)).astype(np.float32)[:, :4]
    h_in = (base[:, 1:, :32], w, mk)
    d_in = (torch.from_numpy(base).cuda()[:, 1:, :32], torch.from_numpy(w).cuda(), torch.from_numpy(mk).cuda())
    reps = LX.lexical_reps(*h_in)
    assert np.array_equal(reps, LX.lexical_reps(*d_in).cpu().numpy())
    hv, hi = np.full((2, 15), 7, np.float16), np.full((2, 11), 99, np.uint8)
    dv, di = torch.from_numpy(hv).cuda(), torch.from_numpy(hi).cuda()
    LX.densify_lexical_into(*h_in, hv[:, :12], hi[:, :8], 8, 0, semantic_reps=cls)
    LX.densify_lexical_into(*d_in, dv[:, :12], di[:, :8], 8, 0, semantic_reps=torch.from_numpy(cls).cuda())
    assert np.array_equal(hv.view(np.uint16), dv.cpu().numpy().view(np.uint16)) and np.array_equal(hi, di.cpu().numpy())
    assert (hv[:, 12:] == 7).all() and (hi[:, 8:] == 99).all() and not (hv[:, :12] == 7).all()
    for agg, full in ((1, True), (2, False)):                              # cal_remove_dim(2 * 1) = cal_remove_dim(2) = 0: 32 columns fold whole
        ha = np.full((2, agg + 6), 7, np.float32)
        da = torch.from_numpy(ha).cuda()
        LX.aggregate_lexical_into(*h_in, ha[:, :agg + 4], agg, full=full, semantic_reps=cls)
        LX.aggregate_lexical_into(*d_in, da[:, :agg + 4], agg, full=full, semantic_reps=torch.from_numpy(cls).cuda())
        assert np.array_equal(ha.view(np.uint32), da.cpu().numpy().view(np.uint32)) and (ha[:, agg + 4:] == 7).all()
        # dhr_aggregate on reps cut from a 40-column base, into a wider output
        wide, out = np.zeros((2, 40), np.float32), np.full((2, agg + 3), 7, np.float32)
        wide[:, :32] = reps
        d_wide, d_out = torch.from_numpy(wide).cuda(), torch.from_numpy(out).cuda()
        for kind, src, dst in ((_lib.MEM_HOST, wide.ctypes.data, out.ctypes.data), (_lib.MEM_DEVICE, d_wide.data_ptr(), d_out.data_ptr())):
            assert lib.dhr_aggregate(0, kind, src, _lib.VAL_F32, 40, 2, 32, agg, 0, int(full), dst, _lib.VAL_F32, agg + 3,
                                     torch.cuda.current_stream().cuda_stream if kind == _lib.MEM_DEVICE else None) == _lib.DHR_OK, lib.dhr_last_error()
        assert np.array_equal(out.view(np.uint32), d_out.cpu().numpy().view(np.uint32)) and (out[:, agg:] == 7).all()
        assert np.array_equal(out[:, :agg], LX.aggregate(reps, agg, full=full))
