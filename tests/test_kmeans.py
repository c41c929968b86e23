"""k-means over whole fp16 rows (dhr_amd/cluster.py on dhr_kmeans_assign / dhr_kmeans_update / dhr_kmeans, csrc/kmeans.hip).

Truth is the float64 restatement below: t64(i, j) = <x_i, c_j> - |c_j|^2 / 2, a first-wins argmax, means and objectives in float64.

The assignment bound is derived from the arithmetic that was built, not measured.  A centroid value c is used as hi + 2^-11 lo' with
hi = fp16(c) (0 where that is subnormal) and lo' = fp16((c - hi) 2^11): c - hi is exact in fp32, |c - hi| <= 2^-11 |c|, so rounding lo' leaves
at most 2^-11 * 2^-11 |c| = 2^-22 |c|, or, where lo' is subnormal (or flushed), at most 2^-25.  Every product x_k hi_k and x_k lo'_k of two
fp16 numbers is exact in fp32; the 2d products are added in fp32 (two accumulators, then one fma and one subtraction), each addition with a
relative error of at most 2^-24 of the partial sum: (2d + 2) 2^-24 sum_k |x_k c_k| in all.  |c_j|^2 / 2 is summed in float64 and rounded once:
2^-24 |c_j|^2 / 2.  Hence, per pair,

    b(i, j) = (2d + 2) 2^-24 sum_k |x_k c_k| + sum_k |x_k| (2^-22 |c_k| + 2^-25) + 2^-24 |c_j|^2 / 2 .

A row's chosen j must be within 2 max_j b(i, j) of the float64 best, and must BE the float64 argmax where the float64 gap between best and
second best exceeds that; at most 5 % of a case's rows may fall under that exemption, asserted from the float64 values alone.  dist[i] must
equal |x_i|^2 - 2 t64(i, assign[i]) within 2 b plus (d + 2) 2^-24 |x_i|^2 (|x_i|^2 is d exact products added in fp32).

CPU part (-m "not gpu"): the symbols, the statuses that are decided before a device is touched.  GPU part: everything else."""
import ctypes as C
import fnmatch
import functools
import os
import re
import time
from types import SimpleNamespace

import numpy as np
import pytest

from dhr_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
NEW = ("dhr_kmeans_assign", "dhr_kmeans_update", "dhr_kmeans")


# ------------------------------------------------------------------------------------------ float64 restatement
def t64_of(x, c):
    """x [n, d], c [K, d] float64 -> t64 [n, K], b [n, K]"""
    d = x.shape[1]
    hn = 0.5 * (c * c).sum(1)
    t = x @ c.T - hn[None, :]
    A = np.abs(x) @ np.abs(c).T
    b = ((2 * d + 2) * U + 2.0 ** -22) * A + 2.0 ** -25 * np.abs(x).sum(1)[:, None] + U * hn[None, :]
    return t, b


def make_case(seed, N, d, K):
    """the inputs of the issue, drawn in its order -> x fp16 [N, d], c fp32 [K, d]"""
    rng = np.random.Generator(np.random.PCG64(seed))
    x = (rng.normal(0, 1, (N, d)) * 0.1).astype(np.float16)
    p = np.sort(rng.permutation(N)[:K])
    c = x[p].astype(np.float32) + rng.normal(0, 1, (K, d)).astype(np.float32) * np.float32(1e-3)
    return x, c


@functools.lru_cache(maxsize=None)
def case(seed, N, d, K):
    x, c = make_case(seed, N, d, K)
    t, b = t64_of(x.astype(np.float64), c.astype(np.float64))
    best = t.argmax(1)                                         # numpy's argmax returns the first maximum
    top = t.max(1)
    if K > 1:
        second = np.partition(t, K - 2, axis=1)[:, K - 2]
    else:
        second = np.full(N, -np.inf)
    for a in (x, c, t, b, best, top, second):
        a.setflags(write=False)
    return SimpleNamespace(x=x, c=c, t=t, b=b, best=best, top=top, gap=top - second, bmax=b.max(1), nx=(x.astype(np.float64) ** 2).sum(1))


def check_assignment(k, a, dist, what):
    """the three rules of the module docstring for a device answer (a, dist) on case k"""
    N, d = k.x.shape
    rows = np.arange(N)
    assert a.dtype == np.int32 and a.min() >= 0 and a.max() < k.c.shape[0], what
    loss = k.top - k.t[rows, a]
    worst = (loss - 2 * k.bmax).max()
    print(f"{what}: largest loss / (2 max b) = {(loss / (2 * k.bmax)).max():.3e}, rows off the float64 argmax: {(a != k.best).sum()}")
    assert worst <= 0, f"{what}: a row chose a centroid {loss.max():.3e} below the float64 best"
    clear = k.gap > 2 * k.bmax
    assert np.array_equal(a[clear], k.best[clear].astype(np.int32)), f"{what}: {(a[clear] != k.best[clear]).sum()} unambiguous rows off the float64 argmax"
    if dist is not None:
        want = k.nx - 2 * k.t[rows, a]
        tol = 2 * k.b[rows, a] + (d + 2) * U * k.nx
        err = np.abs(dist.astype(np.float64) - want)
        print(f"{what}: largest dist error / tolerance = {(err / tol).max():.3e}")
        assert (err <= tol).all(), f"{what}: dist off by {err.max():.3e}"


# ------------------------------------------------------------------------------------------ CPU part
def test_new_symbols_are_declared_mapped_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "dhr_hip.h")).read()
    vmap = open(os.path.join(ROOT, "dhr_amd", "csrc", "libdhr.map")).read()
    globs = re.findall(r"^\s*([a-z_*]+);", vmap.split("local:")[0], re.M)
    lib = _lib.load()
    for name in NEW:
        assert name + "(" in header and name in _lib.EXPORTS and hasattr(lib, name)
        assert getattr(lib, name).argtypes is not None
        assert any(fnmatch.fnmatch(name, p) for p in globs), globs
        m = re.search(r"^int\s+%s\s*\(([^;]*?)\)\s*;" % name, header, re.S | re.M)
        assert m and " ".join(m.group(1).split(",")[-1].split()) == "void* stream" and len(m.group(1).split(",")) == len(getattr(lib, name).argtypes)
    from dhr_amd import _build, cluster
    assert "kmeans.hip" in _build.SOURCES
    for fn in ("assign", "update", "kmeans"):
        assert callable(getattr(cluster, fn))
    assert cluster.KMeans._fields == ("centroids", "assign", "counts", "objective", "changed")


def _host_args(n=8, d=4, K=3):
    x = np.zeros((n, d), np.float16)
    c = np.zeros((K, d), np.float32)
    a = np.zeros(n, np.int32)
    dist = np.zeros(n, np.float32)
    counts = np.zeros(K, np.int64)
    obj, chg = np.zeros(4, np.float64), np.zeros(4, np.int64)
    return SimpleNamespace(x=x, c=c, a=a, dist=dist, counts=counts, obj=obj, chg=chg, n=n, d=d, K=K)


def _bad_argument_calls(lib, kind_ok):
    """(what, call, text of dhr_last_error) for every bad argument of the three entry points; all are refused before a device is touched"""
    h = _host_args()
    p = lambda a: a.ctypes.data                                # noqa: E731

    def assign(x=p(h.x), ld=h.d, n=h.n, d=h.d, c=p(h.c), K=h.K, a=p(h.a), dist=p(h.dist), kind=kind_ok):
        return lib.dhr_kmeans_assign(0, kind, x, ld, n, d, c, K, a, dist, None)

    def update(x=p(h.x), ld=h.d, n=h.n, d=h.d, a=p(h.a), K=h.K, c=p(h.c), counts=p(h.counts), kind=kind_ok):
        return lib.dhr_kmeans_update(0, kind, x, ld, n, d, a, K, c, counts, None)

    def kmeans(x=p(h.x), ld=h.d, n=h.n, d=h.d, K=h.K, iters=3, c=p(h.c), a=p(h.a), counts=p(h.counts), obj=p(h.obj), chg=p(h.chg), kind=kind_ok):
        return lib.dhr_kmeans(0, kind, x, ld, n, d, K, iters, c, a, counts, obj, chg, None)

    bad = np.zeros(h.n, np.int32)
    bad[5] = h.K
    neg = np.zeros(h.n, np.int32)
    neg[2] = -1
    out = []
    for name, fn, ptrs in (("assign", assign, ("x", "c", "a")), ("update", update, ("x", "a", "c", "counts")),
                           ("kmeans", kmeans, ("x", "c", "a", "counts", "obj", "chg"))):
        for q in ptrs:
            out.append((f"{name}: null {q}", lambda fn=fn, q=q: fn(**{q: None}), "null pointer"))
        out += [(f"{name}: ld < d", lambda fn=fn: fn(ld=h.d - 1), "ld is shorter"),
                (f"{name}: n = 0", lambda fn=fn: fn(n=0), "n must be"),
                (f"{name}: n = 2^31", lambda fn=fn: fn(n=1 << 31), "n must be"),
                (f"{name}: d = 0", lambda fn=fn: fn(d=0, ld=0), "d must be"),
                (f"{name}: d = 4097", lambda fn=fn: fn(d=4097, ld=4097), "d must be"),
                (f"{name}: K = 0", lambda fn=fn: fn(K=0), "K must be"),
                (f"{name}: K = 65537", lambda fn=fn: fn(K=65537), "K must be"),
                (f"{name}: mem_kind 7", lambda fn=fn: fn(kind=7), "bad mem_kind")]
    out += [("kmeans: iters < 0", lambda: kmeans(iters=-1), "iters must be"),
            ("update: assign entry = K", lambda: update(a=p(bad)), "assign[5] = 3 is outside [0, 3)"),
            ("update: assign entry < 0", lambda: update(a=p(neg)), "assign[2] = -1 is outside [0, 3)")]
    return out, (h, bad, neg)


def test_bad_arguments_are_refused_before_a_device_is_touched():
    lib = _lib.load()
    calls, keep = _bad_argument_calls(lib, _lib.MEM_HOST)
    for what, call, text in calls:
        assert call() == _lib.ERR_INVALID, what
        assert text in lib.dhr_last_error().decode(), (what, lib.dhr_last_error())
    del keep


def test_wrapper_errors():
    from dhr_amd import cluster
    x = np.zeros((8, 6), np.float16)
    with pytest.raises(ValueError, match="2-D"):
        cluster.assign(x[0], np.zeros((2, 6), np.float32))
    with pytest.raises(ValueError, match="columns"):
        cluster.assign(x, np.zeros((2, 6), np.float32), columns=(4, 9))
    with pytest.raises(ValueError, match="centroids must have shape"):
        cluster.assign(x, np.zeros((2, 5), np.float32))
    with pytest.raises(ValueError, match="assign must have shape"):
        cluster.update(x, np.zeros(7, np.int32), np.zeros((2, 6), np.float32))
    with pytest.raises(ValueError, match="need an `init`"):
        cluster.kmeans(x, 9)
    with pytest.raises(ValueError, match="iters"):
        cluster.kmeans(x, 2, iters=-1)
    with pytest.raises(ValueError, match="outside"):
        cluster.kmeans(x, 2, init=np.asarray([0, 8]))
    assert np.array_equal(cluster.initial_rows(50, 7, 3), np.random.Generator(np.random.PCG64(3)).permutation(50)[:7])


# ------------------------------------------------------------------------------------------ GPU part
def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(t):
    return t.detach().cpu().numpy() if not isinstance(t, np.ndarray) else t


# (N, d, K, record width, first column): the shapes of the issue -- one chunk and several, K below and beyond a tile, rows of 16-byte multiples
# and not, a last row block and a last centroid tile that are not full -- and one more of this file: several chunks read element by element
SHAPES = [(4099, 100, 67, None, 0), (3001, 160, 257, None, 0), (5000, 72, 2000, None, 0), (4099, 768, 2000, None, 0), (2048, 1536, 40, None, 0),
          (4099, 100, 67, 131, 3), (515, 200, 33, 203, 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [1, 2])
@pytest.mark.parametrize("N, d, K, width, col0", SHAPES)
def test_assignment_against_float64(seed, N, d, K, width, col0):
    from dhr_amd import cluster
    k = case(seed, N, d, K)
    exempt = (k.gap <= 2 * k.bmax).mean()
    print(f"seed {seed} {N}x{d}x{K}: {100 * exempt:.2f} % of the rows have a float64 gap inside 2 max b")
    assert exempt <= 0.05                                      # from the float64 values alone, before the device is asked
    if width is None:
        a, dist = cluster.assign(_dev(k.x), _dev(k.c))
    else:
        wide = np.full((N, width), 7.0, np.float16)
        wide[:, col0:col0 + d] = k.x
        t = _dev(wide)
        assert (t.data_ptr() + 2 * col0) % 16 != 0 and width > d
        a, dist = cluster.assign(t, _dev(k.c), columns=(col0, col0 + d))
    check_assignment(k, _np(a), _np(dist), f"seed {seed} {N}x{d}x{K}" + ("" if width is None else f" in {width} columns"))


@pytest.mark.gpu
def test_ties_go_to_the_lowest_centroid():
    from dhr_amd import cluster
    k = case(1, 4099, 100, 67)
    base, _ = cluster.assign(_dev(k.x), _dev(k.c))
    base = _np(base)
    c = k.c.copy()
    c[5] = c[40] = c[2]
    c[66] = c[33]
    got, dist = cluster.assign(_dev(k.x), _dev(c))
    got = _np(got)
    assert not np.isin(got, (5, 40, 66)).any()
    kept = ~np.isin(base, (5, 40, 66))
    assert np.array_equal(got[kept], base[kept])
    assert (base == 2).any() and (base == 33).any()
    one, dist1 = cluster.assign(_dev(k.x), _dev(k.c[:1]))
    assert not _np(one).any()
    tol = 2 * k.b[:, 0] + (100 + 2) * U * k.nx
    assert (np.abs(_np(dist1).astype(np.float64) - (k.nx - 2 * k.t[:, 0])) <= tol).all()


@pytest.mark.gpu
def test_update_means_counts_and_empty_clusters():
    from dhr_amd import cluster
    rng = np.random.Generator(np.random.PCG64(5))
    N, d, K = 3001, 259, 70                                     # two column blocks of the mean kernel, the second one partial
    x = (rng.normal(0, 1, (N, d)) * 0.3).astype(np.float16)
    a = rng.integers(0, K, N).astype(np.int32)
    a[np.isin(a, (0, 17, 69))] = 3                              # three empty clusters, the first and the last among them
    a[a == 41] = 40
    a[7] = 41                                                   # ... and a cluster of one
    c0 = rng.normal(0, 1, (K, d)).astype(np.float32)
    wide = np.full((N, d + 5), 9.0, np.float16)
    wide[:, 2:2 + d] = x
    for values, cols in ((_dev(x), None), (_dev(wide), (2, 2 + d)), (x, None)):
        c_in = c0 if isinstance(values, np.ndarray) else _dev(c0)
        c1, counts = cluster.update(values, a if isinstance(values, np.ndarray) else _dev(a), c_in, columns=cols)
        assert np.array_equal(_np(c_in), c0)                    # the input centroids are not written
        c1, counts = _np(c1), _np(counts)
        want_n = np.bincount(a, minlength=K)
        assert counts.dtype == np.int64 and np.array_equal(counts, want_n)
        x64 = x.astype(np.float64)
        for j in range(K):
            if want_n[j] == 0:
                assert np.array_equal(c1[j].view(np.uint32), c0[j].view(np.uint32)), j
                continue
            m = want_n[j]
            mem = x64[a == j]
            tol = (m + 2) * U * np.abs(mem).sum(0) / m
            assert (np.abs(c1[j].astype(np.float64) - mem.mean(0)) <= tol).all(), j
        assert (want_n == 0).sum() == 3 and want_n[41] == 1


@pytest.mark.gpu
def test_update_is_exact_on_a_grid():
    from dhr_amd import cluster
    rng = np.random.Generator(np.random.PCG64(6))
    sizes = [1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1, 64]      # member counts: powers of two
    K, d = len(sizes), 72
    a = rng.permutation(np.repeat(np.arange(K), sizes)).astype(np.int32)
    x = (rng.integers(-64, 65, (len(a), d)) / 64.0).astype(np.float16)          # multiples of 2^-6: every partial sum is exact in fp32
    c1, counts = cluster.update(_dev(x), _dev(a), _dev(np.zeros((K, d), np.float32)))
    want = np.stack([x[a == j].astype(np.float64).mean(0) for j in range(K)]).astype(np.float32)
    assert np.array_equal(_np(c1).view(np.uint32), want.view(np.uint32))
    assert np.array_equal(_np(counts), np.asarray(sizes))


def _planted():
    rng = np.random.Generator(np.random.PCG64(7))
    K, d, N = 16, 96, 2000
    centres = rng.normal(0, 1, (K, d)) * 0.1
    labels = rng.integers(0, K, N)
    labels[:K] = rng.permutation(K)                             # every label occurs
    x = (centres[labels] + rng.normal(0, 1, (N, d)) * 0.005).astype(np.float16)
    init = np.asarray([np.flatnonzero(labels == j)[0] for j in range(K)], np.int64)
    return x, labels, init


@pytest.mark.gpu
def test_whole_run_on_planted_clusters():
    from dhr_amd import cluster
    x, labels, init = _planted()
    res = cluster.kmeans(_dev(x), 16, iters=3, init=init)
    assert np.array_equal(_np(res.assign), labels.astype(np.int32))
    changed, obj = _np(res.changed), _np(res.objective)
    assert changed[0] == len(x) and not changed[1:].any()
    assert np.array_equal(_np(res.counts), np.bincount(labels, minlength=16))
    assert len(obj) == 4 and len(set(obj[1:].tolist())) == 1 and obj[1] < obj[0]
    means = np.stack([x[labels == j].astype(np.float64).mean(0) for j in range(16)])
    assert np.abs(_np(res.centroids) - means).max() < 1e-5


@pytest.mark.gpu
def test_objective_is_monotone_within_the_bound():
    """case (3001, 160, 257), init=None, seed=0, iters=6: the rounds are replayed with assign / update to have the centroids of every round;
    dhr_kmeans must give the same bits as the replay."""
    from dhr_amd import cluster
    N, d, K, iters = 3001, 160, 257, 6
    x, _ = make_case(1, N, d, K)
    xd = _dev(x)
    res = cluster.kmeans(xd, K, iters=iters, seed=0)
    obj = _np(res.objective)
    x64 = x.astype(np.float64)
    c = _dev(x[cluster.initial_rows(N, K, 0)].astype(np.float32))
    slack, prev_a = [], None
    for t in range(iters + 1):
        a, dist = cluster.assign(xd, c)
        a_np, c64 = _np(a), _np(c).astype(np.float64)
        _, b = t64_of(x64, c64)
        slack.append((2 * b.max(1)).sum())
        exact = ((x64 - c64[a_np]) ** 2).sum()
        print(f"round {t}: objective {obj[t]:.9f}, float64 of the same assignment {exact:.9f}, allowed {slack[t]:.3e}")
        assert abs(obj[t] - exact) <= slack[t]
        assert int(_np(res.changed)[t]) == (N if prev_a is None else int((a_np != prev_a).sum()))
        prev_a = a_np
        if t < iters:
            assert obj[t + 1] <= obj[t] + slack[t]
            c, counts = cluster.update(xd, a, c)
    assert np.array_equal(_np(res.assign), prev_a)
    assert np.array_equal(_np(res.centroids).view(np.uint32), _np(c).view(np.uint32))
    assert np.array_equal(_np(res.counts), np.bincount(prev_a, minlength=K))


@pytest.mark.gpu
def test_two_runs_and_both_memory_kinds_give_the_same_bits():
    from dhr_amd import cluster
    x, _ = make_case(2, 3001, 160, 257)
    wide = np.full((3001, 170), 3.0, np.float16)
    wide[:, 5:165] = x
    runs = [cluster.kmeans(_dev(x), 257, iters=4, seed=3), cluster.kmeans(_dev(x), 257, iters=4, seed=3), cluster.kmeans(x, 257, iters=4, seed=3),
            cluster.kmeans(_dev(wide), 257, iters=4, seed=3, columns=(5, 165)), cluster.kmeans(wide, 257, iters=4, seed=3, columns=(5, 165))]
    assert isinstance(runs[2].assign, np.ndarray) and runs[0].assign.is_cuda
    first = [_np(f).tobytes() for f in runs[0]]
    assert len(first) == 5
    for r in runs[1:]:
        assert [_np(f).tobytes() for f in r] == first
    assert (_np(runs[0].counts) == 0).sum() >= 0 and _np(runs[0].changed)[0] == 3001


@pytest.mark.gpu
def test_statuses_with_a_device_present():
    import torch
    lib = _lib.load()
    torch.cuda.init()
    calls, keep = _bad_argument_calls(lib, _lib.MEM_HOST)
    for what, call, text in calls:
        assert call() == _lib.ERR_INVALID, what
        assert text in lib.dhr_last_error().decode(), (what, lib.dhr_last_error())
    # ... and on device arrays: the size checks come before anything is launched
    x, c = torch.zeros((8, 4), dtype=torch.float16, device="cuda"), torch.zeros((3, 4), dtype=torch.float32, device="cuda")
    a, dist = torch.zeros(8, dtype=torch.int32, device="cuda"), torch.zeros(8, dtype=torch.float32, device="cuda")
    cnt, obj, chg = torch.zeros(3, dtype=torch.int64, device="cuda"), torch.zeros(4, dtype=torch.float64, device="cuda"), torch.zeros(4, dtype=torch.int64, device="cuda")
    p = lambda t: t.data_ptr()                                 # noqa: E731
    D = _lib.MEM_DEVICE
    assert lib.dhr_kmeans_assign(0, D, p(x), 3, 8, 4, p(c), 3, p(a), p(dist), None) == _lib.ERR_INVALID
    assert lib.dhr_kmeans_assign(0, D, p(x), 4, 8, 4, p(c), 0, p(a), p(dist), None) == _lib.ERR_INVALID
    assert lib.dhr_kmeans(0, D, p(x), 4, 8, 4, 3, -1, p(c), p(a), p(cnt), p(obj), p(chg), None) == _lib.ERR_INVALID
    assert lib.dhr_kmeans_update(0, 5, p(x), 4, 8, 4, p(a), 3, p(c), p(cnt), None) == _lib.ERR_INVALID
    # an out-of-range entry of a DEVICE assignment is not read back: the row joins no cluster, nothing is written out of bounds
    a[3], a[4] = 3, -7
    x[:] = 1.0
    assert lib.dhr_kmeans_update(0, D, p(x), 4, 8, 4, p(a), 3, p(c), p(cnt), None) == 0
    torch.cuda.synchronize()
    assert cnt.tolist() == [6, 0, 0] and c[0].tolist() == [1.0] * 4 and not c[1:].any()
    del keep


# ------------------------------------------------------------------------------------------ stream order (the method of tests/test_stream_order.py)
STREAM_LAST = NEW
MIN_BLOCK_MS, HOST_FACTOR, MAX_BLOCK_MS, ROUNDS = 100.0, 20.0, 2000.0, 3


class _Spy:
    """the loaded library with every dhr_* call recorded"""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("dhr_"):
            return fn

        def recorded(*args):
            self.calls.append((name, args))
            return fn(*args)
        return recorded


class _Blocker:
    """Plain torch work on the current stream that lasts a requested time: torch.cuda._sleep, or a chain of matmuls where that does not spin."""

    def __init__(self):
        import torch
        self.eye = None
        torch.cuda._sleep(1000)
        cycles = 20_000_000
        ms = self._time(lambda: torch.cuda._sleep(cycles))
        if ms >= 1.0:
            self.per_ms = cycles / ms
        else:
            self.eye = torch.eye(4096, device="cuda")
            self._matmuls(2)
            self.per_ms = 20 / self._time(lambda: self._matmuls(20))

    @staticmethod
    def _time(fn):
        import torch
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    def _matmuls(self, n):
        x = self.eye
        for _ in range(n):
            x = x @ self.eye

    def enqueue(self, ms):
        import torch
        n = int(ms * 1.3 * self.per_ms) + 1
        if self.eye is None:
            torch.cuda._sleep(n)
        else:
            self._matmuls(n)


@pytest.fixture(scope="module")
def blocker():
    return _Blocker()


def _runs_beside_null(s, blocker):
    """a short blocker on s, then a fill on the null stream: the fill must finish while the blocker still runs"""
    import torch
    null = torch.cuda.default_stream()
    probe = torch.empty(64, device="cuda")
    torch.cuda.synchronize()
    behind = torch.cuda.Event()
    with torch.cuda.stream(s):
        blocker.enqueue(20.0)
        behind.record()
    with torch.cuda.stream(null):
        probe.fill_(1.0)
    null.synchronize()
    concurrent = not behind.query()
    s.synchronize()
    return concurrent


def _side_stream(blocker):
    import torch
    for _ in range(8):
        s = torch.cuda.Stream()
        if _runs_beside_null(s, blocker):
            return s
    pytest.fail("no side stream runs concurrently with the null stream: a wrong stream cannot be observed here")


def _bits(t):
    return t.detach().contiguous().cpu().numpy().reshape(-1).view(np.uint8)


def _round(real, poison, call, blocker, monkeypatch):
    import torch
    s = _side_stream(blocker)
    with torch.cuda.stream(s):
        bufs = {k: v.to("cuda") for k, v in poison.items()}
        staged = {k: v.to("cuda") for k, v in real.items()}
        on_poison = tuple(t.detach().clone() for t in call(bufs))      # warm-up: kernels loaded, the allocators hold every block the call takes
        s.synchronize()
        host_ms = float("inf")
        for _ in range(3):
            t0 = time.perf_counter()
            call(bufs)
            host_ms = min(host_ms, (time.perf_counter() - t0) * 1e3)
            s.synchronize()
    spy = _Spy(_lib.load())
    monkeypatch.setattr(_lib, "load", lambda: spy)
    need_ms = max(MIN_BLOCK_MS, HOST_FACTOR * host_ms)
    e0, e1, e_in = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True), torch.cuda.Event()
    with torch.cuda.stream(s):
        e0.record()
        blocker.enqueue(min(need_ms, MAX_BLOCK_MS))
        e1.record()
        for k in bufs:
            bufs[k].copy_(staged[k])
        e_in.record()
        got = call(bufs)
        returned_early = not e_in.query()
    s.synchronize()
    monkeypatch.undo()
    block_ms = e0.elapsed_time(e1)
    if block_ms < need_ms:
        blocker.per_ms *= 1.2 * need_ms / max(block_ms, 1.0)
    beside = _runs_beside_null(s, blocker)
    return SimpleNamespace(got=got, on_poison=on_poison, returned_early=returned_early, calls=spy.calls, stream=s.cuda_stream, need_ms=need_ms,
                           block_ms=block_ms, host_ms=host_ms, beside=beside, decisive=need_ms <= MAX_BLOCK_MS and block_ms >= need_ms and beside)


def _stream_inputs(seed):
    import torch
    x, c = make_case(seed, 3001, 160, 257)
    return dict(x=torch.from_numpy(x), c=torch.from_numpy(c))


@pytest.mark.gpu
@pytest.mark.parametrize("op", ["assign", "kmeans"])
def test_runs_in_stream_order_without_waiting(op, blocker, monkeypatch):
    """Real inputs are copied into buffers of poison (another seed) behind a blocker on a side stream, then the op is called: it must see the real
    inputs (bit-equal to a run on the default stream), every library call must carry that stream, and the call must return while the
    blocker still runs.  Up to ROUNDS rounds, until one is decisive (tests/test_stream_order.py)."""
    import torch
    from dhr_amd import cluster
    if op == "assign":
        call = lambda d: cluster.assign(d["x"], d["c"])                               # noqa: E731
    else:
        call = lambda d: tuple(cluster.kmeans(d["x"], 257, iters=2, init=d["c"]))     # noqa: E731
    real, poison = _stream_inputs(1), _stream_inputs(2)
    ref = call({k: v.to("cuda") for k, v in real.items()})
    torch.cuda.synchronize()
    rounds = []
    while len(rounds) < ROUNDS:
        rounds.append(_round(real, poison, call, blocker, monkeypatch))
        if rounds[-1].decisive and rounds[-1].returned_early:
            break
    for n, r in enumerate(rounds):
        print(f"stream order {op} round {n + 1}: blocker {r.block_ms:.1f} ms (needed {r.need_ms:.1f}), warmed host call {r.host_ms:.3f} ms, returned early: "
              f"{r.returned_early}, beside the null stream afterwards: {r.beside}, library calls: {[c[0] for c in r.calls]}")
        assert r.stream not in (None, 0) and len(r.got) == len(ref) == len(r.on_poison)
        for i, (g, w) in enumerate(zip(r.got, ref)):
            assert g.shape == w.shape and g.dtype == w.dtype, (op, i)
            assert np.array_equal(_bits(g), _bits(w)), f"{op}: result {i} differs from the default-stream run: the op did not run in stream order"
        assert any(not np.array_equal(_bits(g), _bits(w)) for g, w in zip(r.on_poison, ref)), f"{op}: poison and real inputs give the same result"
        assert r.calls, op
        for name, args in r.calls:
            if name == "dhr_last_error":
                continue
            assert name in STREAM_LAST, f"{op}: {name} is not expected here"
            assert args[-1] is not None and args[-1] != 0 and args[-1] == r.stream, f"{op}: {name} got stream {args[-1]}, torch's current stream is {r.stream}"
    last = rounds[-1]
    assert last.need_ms <= MAX_BLOCK_MS, f"{op}: the call takes {last.host_ms:.1f} ms on the host"
    assert last.block_ms >= last.need_ms, f"{op}: the blocker lasted {last.block_ms:.1f} ms, {last.need_ms:.1f} ms were needed"
    assert last.beside, f"{op}: in none of {len(rounds)} rounds did the side stream stay beside the null stream"
    assert last.returned_early, f"{op}: documented as not waiting, but in {len(rounds)} rounds the call returned only after its stream had caught up"
