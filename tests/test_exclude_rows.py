"""dhr_exclude_rows (dhr_amd/csrc/exclude.hip): per query, the first k_out pairs of a ranked list whose row is not in the query's exclusion
list, in their input order.

GPU part: the kernel against a numpy restatement written here (`restate`), bit for bit, from host arrays and from device arrays, with
out_valid checked in every case and every case run twice (two calls on the same arguments are bit-identical).  The shapes are the ones at
which the kernel takes another path: lists of 0 / 1 / 64 / 65 rows (64 is the last length compared row by row, 65 the first that is sorted
and searched), a list longer than one LDS chunk and one longer than two (the chunk length comes from dhr_debug_exclude_chunk), n_in around the
wave and workgroup sizes and beyond one workgroup's LDS merge, one and several workgroups.
CPU part: every argument check returns its status with a message before any device call (no GPU needed)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from dhr_amd import _build, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def restate(scores, rows, ptr, ex, k):
    out_s = np.full((rows.shape[0], k), -np.inf, np.float32)
    out_r = np.full((rows.shape[0], k), -1, np.int64)
    valid = np.zeros(rows.shape[0], np.int32)
    for q in range(rows.shape[0]):
        keep = np.nonzero((rows[q] >= 0) & ~np.isin(rows[q], ex[ptr[q]:ptr[q + 1]]))[0][:k]
        out_s[q, :len(keep)], out_r[q, :len(keep)], valid[q] = scores[q, keep], rows[q, keep], len(keep)
    return out_s, out_r, valid


def make_case(seed, Q, n_in, lengths, all_excluded=()):
    """Ranked lists with runs of equal scores, padding at the end of some and in the middle of others, rows above 2^32 in every other query;
    exclusion list q has lengths[q % len(lengths)] rows: rows of the list (about a third of it where the length allows), rows that occur in
    no list, negative rows (-1 among them) and repeats, shuffled.  Queries in all_excluded list every row they have."""
    rng = np.random.default_rng(seed)
    scores = -np.sort(-np.round(rng.standard_normal((Q, n_in)) * 3, 1).astype(np.float32), axis=1) + np.float32(0)
    rows = np.empty((Q, n_in), np.int64)
    lists = []
    for q in range(Q):
        r = (rng.permutation(n_in) * 50 + rng.integers(0, 50, n_in)).astype(np.int64)       # distinct
        if q % 2:
            r += (1 << 32) + 12345
        if q % 3 == 1 and n_in > 4:                  # a padded tail, as a search deeper than the corpus leaves it
            fill = int(rng.integers(1, n_in))
            r[fill:], scores[q, fill:] = -1, -np.inf
        if q % 3 == 2 and n_in > 4:                  # padding between real entries, as a merge's input may hold it
            r[rng.choice(n_in, n_in // 5, replace=False)] = -1
        rows[q] = r
        want = lengths[q % len(lengths)]
        real = r[r >= 0]
        if q in all_excluded:                        # every row it has, with repeats up to the asked length
            e = np.concatenate([real, real[: max(0, want - len(real))]])
        else:
            n_hit = min(len(real), want // 3 if want >= 3 else want)
            hits = rng.choice(real, n_hit, replace=False) if n_hit else real[:0]
            absent = -rng.integers(1, 1 << 40, size=want) if q % 4 == 0 else rng.integers(1 << 50, 1 << 51, size=want)
            e = np.concatenate([hits, np.array([-1, -7], np.int64), hits[: len(hits) // 2], absent.astype(np.int64)])[:want]
        lists.append(rng.permutation(e))
    ptr, ex, _, _ = _lib.make_exclusions(lists)
    return scores, rows, ptr, ex


def call_host(lib, scores, rows, ptr, ex, k):
    Q, n_in = rows.shape
    out_s, out_r, out_v = np.full((Q, k), 7, np.float32), np.full((Q, k), 7, np.int64), np.full(Q, -3, np.int32)
    rc = lib.dhr_exclude_rows(0, _lib.MEM_HOST, Q, n_in, scores.ctypes.data, rows.ctypes.data, ptr.ctypes.data, ex.ctypes.data, k,
                              out_s.ctypes.data, out_r.ctypes.data, out_v.ctypes.data, None)
    assert rc == 0, lib.dhr_last_error()
    return out_s, out_r, out_v


def call_device(lib, scores, rows, ptr, ex, k):
    import torch
    Q, n_in = rows.shape
    d_s, d_r, d_e = torch.from_numpy(scores).cuda(), torch.from_numpy(rows).cuda(), torch.from_numpy(ex).cuda()
    out_s = torch.full((Q, k), 7, dtype=torch.float32, device="cuda")
    out_r = torch.full((Q, k), 7, dtype=torch.int64, device="cuda")
    out_v = torch.full((Q,), -3, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    rc = lib.dhr_exclude_rows(0, _lib.MEM_DEVICE, Q, n_in, d_s.data_ptr(), d_r.data_ptr(), ptr.ctypes.data, d_e.data_ptr(), k,
                              out_s.data_ptr(), out_r.data_ptr(), out_v.data_ptr(), None)
    assert rc == 0, lib.dhr_last_error()
    torch.cuda.synchronize()
    return out_s.cpu().numpy(), out_r.cpu().numpy(), out_v.cpu().numpy()


def same_bits(got, want, what):
    for g, w, name in zip(got, want, ("scores", "rows", "valid")):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name)
        assert np.array_equal(g.view(np.uint8), w.view(np.uint8)), (what, name, np.argwhere(g != w)[:5])


def check_case(lib, scores, rows, ptr, ex, ks, what):
    """-> the expected (scores, rows, valid) of the first k of ks"""
    wants = []
    for k in ks:
        want = restate(scores, rows, ptr, ex, k)
        wants.append(want)
        for call in (call_host, call_device):
            got = call(lib, scores, rows, ptr, ex, k)
            same_bits(got, want, (what, k, call.__name__))
            same_bits(call(lib, scores, rows, ptr, ex, k), got, (what, k, call.__name__, "second call"))
    return wants[0]


def _ks(n_in):
    return sorted({n_in, max(1, (2 * n_in) // 3), 1})


@pytest.mark.gpu
@pytest.mark.parametrize("Q", [1, 3, 257])
@pytest.mark.parametrize("n_in", [1, 63, 64, 65, 1000, 16385])
def test_shapes_against_numpy(n_in, Q):
    """every n_in x Q; the lists of a batch take the lengths 0, 1, 64, 65, 7 and (Q = 257: some queries) more than one chunk in turn"""
    lib = _lib.load()
    chunk = lib.dhr_debug_exclude_chunk()
    lengths = [[65], [0, 64, 1], [0, 1, 64, 65, 7, 3, 200] + ([chunk + 37] if n_in <= 1000 else [])][[1, 3, 257].index(Q)]
    scores, rows, ptr, ex = make_case(1000 * Q + n_in, Q, n_in, lengths)
    want = check_case(lib, scores, rows, ptr, ex, _ks(n_in) if Q < 257 else [n_in, max(1, n_in // 2)], (n_in, Q))
    assert all(-1 not in want[1][q, : want[2][q]] for q in range(Q))


@pytest.mark.gpu
@pytest.mark.parametrize("length", ["0", "1", "64", "65", "chunk", "chunk+1", "2*chunk+5"])
def test_list_lengths(length):
    """one length for every list of the batch: both sides of the row-by-row / sorted threshold and of the chunk boundary, three chunks"""
    lib = _lib.load()
    n = int(eval(length, {"chunk": lib.dhr_debug_exclude_chunk()}))
    for n_in, seed in ((1000, 5), (16385, 6)):
        scores, rows, ptr, ex = make_case(seed + n, 3, n_in, [n])
        assert np.all(np.diff(ptr) == n)
        want = check_case(lib, scores, rows, ptr, ex, [n_in, 100], (length, n_in))
        if n >= 3:                                     # the case does exclude something, and k_out = n_in leaves a padded tail
            assert np.all(want[2] < (rows >= 0).sum(1)) and np.all(want[1][:, -1] == -1)


@pytest.mark.gpu
def test_every_entry_excluded_and_lists_of_all_kinds():
    """queries whose every entry is excluded (by a short list, a sorted list and a list of several chunks) beside ordinary ones"""
    lib = _lib.load()
    chunk = lib.dhr_debug_exclude_chunk()
    for n_in in (40, 3000, 2 * chunk + 300):
        scores, rows, ptr, ex = make_case(77 + n_in, 5, n_in, [n_in + 9, 5, n_in + 9, 70, 0], all_excluded=(0, 2))
        want = check_case(lib, scores, rows, ptr, ex, [n_in, 7], n_in)
        assert want[2][0] == 0 and want[2][2] == 0 and np.all(want[1][0] == -1) and np.all(np.isneginf(want[0][2]))
        assert want[2][4] == (rows[4] >= 0).sum()


@pytest.mark.gpu
def test_equal_scores_keep_their_order_and_minus_one_never_matches_padding():
    lib = _lib.load()
    Q, n_in = 2, 300
    scores = np.repeat(np.array([[3.0], [-0.0]], np.float32), n_in, axis=1)        # one run of equal scores per query
    rows = np.stack([np.arange(n_in, dtype=np.int64)[::-1] * 3, (1 << 40) + np.arange(n_in, dtype=np.int64)])
    rows[1, 10:20] = -1
    ptr, ex, _, _ = _lib.make_exclusions([[-1, 6, 6, 297 * 3, 5], [-1, (1 << 40) + 5, 17]])
    check_case(lib, scores, rows, ptr, ex, [n_in, 50], "ties")
    got = call_host(lib, scores, rows, ptr, ex, n_in)
    assert got[2].tolist() == [n_in - 2, n_in - 10 - 1]
    assert got[1][0, :3].tolist() == [299 * 3, 298 * 3, 296 * 3] and np.signbit(got[0][1, 0])


def test_chunk_constant_build_list_and_exports():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "dhr_hip.h")).read()
    assert lib.dhr_debug_exclude_chunk() == int(re.search(r"#define DHR_EXCLUDE_CHUNK (\d+)", header).group(1)) > 64
    assert "exclude.hip" in _build.SOURCES
    for name in ("dhr_exclude_rows", "dhr_search_excluding", "dhr_debug_exclude_chunk"):
        assert name + "(" in header and name in _lib.EXPORTS and hasattr(lib, name)


def test_argument_checks_answer_before_the_device():
    """Each check returns its status and leaves a message; none of them reaches a device call (this runs on hosts without a GPU)."""
    lib = _lib.load()
    Q, n, k = 2, 4, 3
    s, r = np.zeros((Q, n), np.float32), np.arange(Q * n, dtype=np.int64).reshape(Q, n)
    ptr, ex = np.array([0, 1, 3], np.int64), np.array([1, 2, 3], np.int64)
    os_, or_, ov = np.zeros((Q, k), np.float32), np.zeros((Q, k), np.int64), np.zeros(Q, np.int32)

    def call(**kw):
        a = dict(device=0, kind=_lib.MEM_HOST, Q=Q, n=n, s=s.ctypes.data, r=r.ctypes.data, ptr=ptr.ctypes.data, ex=ex.ctypes.data, k=k,
                 os=os_.ctypes.data, orow=or_.ctypes.data, ov=ov.ctypes.data)
        a.update(kw)
        rc = lib.dhr_exclude_rows(a["device"], a["kind"], a["Q"], a["n"], a["s"], a["r"], a["ptr"], a["ex"], a["k"], a["os"], a["orow"], a["ov"], None)
        return rc, lib.dhr_last_error().decode()

    bad_first = np.array([1, 1, 3], np.int64)
    decreasing = np.array([0, 2, 1], np.int64)
    cases = [(dict(s=None), "null"), (dict(r=None), "null"), (dict(os=None), "null"), (dict(orow=None), "null"), (dict(ptr=None), "excl_ptr_host"),
             (dict(ex=None), "excl_rows"), (dict(ptr=bad_first.ctypes.data), "excl_ptr_host[0]"), (dict(ptr=decreasing.ctypes.data), "decreases"),
             (dict(n=0), "n_in"), (dict(n=-4), "n_in"), (dict(k=0), "k_out"), (dict(k=-1), "k_out"), (dict(k=n + 1), "k_out"),
             (dict(kind=2), "mem_kind"), (dict(kind=-1), "mem_kind"), (dict(Q=-1), "n_queries")]
    for kw, word in cases:
        rc, msg = call(**kw)
        assert rc == _lib.ERR_INVALID and word in msg, (kw, rc, msg)
    big = np.array([0, 0, lib.dhr_debug_exclude_chunk() + 1], np.int64)
    rc, msg = call(ptr=big.ctypes.data, n=(1 << 20) + 1, k=1)          # (refused before any array is read)
    assert rc == _lib.ERR_UNSUPPORTED and "1048576" in msg
    # the allocation hook reaches the entry checkpoint on a host without a GPU too
    lib.dhr_debug_fail_alloc(1)
    rc, msg = call()
    lib.dhr_debug_fail_alloc(0)
    assert rc == _lib.ERR_NOMEM and "memory" in msg
    # dhr_search_excluding validates its handle and batch first, as dhr_search does
    qb, keep = _lib.make_query_batch(np.zeros((Q, 64), np.float32), None)
    assert lib.dhr_search_excluding(None, C.byref(qb), 1, ptr.ctypes.data, ex.ctypes.data, _lib.MEM_HOST, os_.ctypes.data, or_.ctypes.data,
                                    _lib.MEM_HOST, None) == _lib.ERR_INVALID and lib.dhr_last_error()
    del keep


@pytest.mark.gpu
def test_make_exclusions_keeps_device_rows_on_the_device():
    import torch
    rows = torch.tensor([4, 9, 2], dtype=torch.int64, device="cuda")
    ptr, got, kind, _ = _lib.make_exclusions((np.array([0, 1, 3]), rows))
    assert kind == _lib.MEM_DEVICE and got.data_ptr() == rows.data_ptr() and ptr.tolist() == [0, 1, 3]
    with pytest.raises(_lib.DhrError):
        _lib.make_exclusions((np.array([0, 3]), rows.to(torch.int32)))
