"""Stream order of every torch-facing op: the op runs on torch's CURRENT stream, and the ops documented as not waiting do not wait.

Every other numerical test runs on torch's default stream, which on ROCm is the legacy null stream: there an op enqueued on the wrong stream
still passes, and so does an op that waits although its documentation says it does not.  Here one harness (`run`) makes both visible:

    ref = call(real inputs) on the default stream
    bufs = device buffers holding POISON: make_inputs(seed + 1), valid inputs of the same shapes, dtypes and distribution
    on a fresh side stream s that does not share a hardware queue with the null stream (`_side_stream`):
                         a blocker (plain torch work of >= 100 ms and >= 20 x the host time of the call), then the copies real inputs -> bufs,
                         then got = call(bufs)

An op that runs on s sees the real inputs and returns `ref`, bit for bit (every op here is bit-reproducible).  An op that runs on another
stream -- torch's side streams do not wait for the null stream, nor it for them -- reads the poison while the blocker still runs: a bit
mismatch on readable memory, no fault.  A spy on the loaded library checks the same thing at the C ABI: every dhr_* call made inside `call`
received s as its stream argument (the last parameter of these entry points; `test_stream_is_the_last_parameter` checks that against
include/dhr_hip.h).  An op that returns before the event recorded behind the copies has completed did not wait for its stream.
`test_control_wrong_stream_reads_poison` runs the harness on a stand-in op that clones its inputs on the default stream and asserts that it
gets the poison: the arrangement can fail.  Timing on a shared machine can make one round inconclusive (`run`): it is then repeated on another
side stream, at most twice; what a round must show whatever its timing is asserted in every round.

Each case's comment names the launch sites (kernel launches, memsets, copies in the host code of its entry points) that its shape reaches."""
import os
import re
import time
from types import SimpleNamespace

import numpy as np
import pytest

from dhr_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(os.path.dirname(HERE), "include", "dhr_hip.h")

# entry points whose last parameter is `void* stream` ...
STREAM_LAST = ("dhr_densify", "dhr_lexical_head", "dhr_aggregate", "dhr_lexical_proj_head", "dhr_gip_scores", "dhr_gip_scores_backward",
               "dhr_densify_backward", "dhr_lexical_head_train", "dhr_lexical_head_backward", "dhr_lexical_proj_train", "dhr_lexical_proj_backward",
               "dhr_maxsim_scores", "dhr_maxsim_scores_backward", "dhr_aggregate_train", "dhr_aggregate_backward", "dhr_term_weight_head",
               "dhr_term_weight_head_backward", "dhr_merge_topk", "dhr_merge_topk_lists", "dhr_pq_train_nbits", "dhr_pq_encode_nbits",
               "dhr_pq_decode_nbits")
# ... and the host-only ones the wrappers also call (sizes, the error string): anything else a wrapper calls fails the case
NO_STREAM = ("dhr_gip_scores_workspace", "dhr_lexical_head_train_workspace", "dhr_lexical_proj_workspace", "dhr_lexical_proj_train_workspace",
             "dhr_last_error")

_DECL = r"^(?:int|int64_t|const char\*)\s+{}\s*\(([^;]*?)\)\s*;"      # a prototype of include/dhr_hip.h, its parameter list captured
MIN_BLOCK_MS, HOST_FACTOR, MAX_BLOCK_MS = 100.0, 20.0, 2000.0


def test_stream_is_the_last_parameter():
    with open(HEADER) as f:
        text = f.read()
    for name in STREAM_LAST:
        m = re.search(_DECL.format(name), text, re.S | re.M)
        assert m, name
        assert " ".join(m.group(1).split(",")[-1].split()) == "void* stream", name
    for name in NO_STREAM:
        m = re.search(_DECL.format(name), text, re.S | re.M)
        assert m and "stream" not in m.group(1), name


# ------------------------------------------------------------------------------------------ the harness
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
    """Plain torch work on the current stream that lasts a requested time: torch.cuda._sleep, or a chain of matmuls where that does not
    spin.  Calibrated once with device events; `run` measures every use again."""

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
        self.calibrated_ms = ms

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
    """A fresh side stream that the hardware runs concurrently with the null stream.  The runtime maps its streams onto a few hardware queues
    (four by default), and a queue runs its packets in order: a side stream that shares the null stream's queue serialises with it whatever
    its flags say, and work on the wrong stream would then see the right data.  Which of torch's pool streams do depends on how many streams
    the process has made so far, so each candidate is probed.  -> (stream, candidates tried)"""
    import torch
    for attempt in range(1, 9):
        s = torch.cuda.Stream()
        if _runs_beside_null(s, blocker):
            return s, attempt
    pytest.fail("no side stream runs concurrently with the null stream: a wrong stream cannot be observed here")


def _upload(cpu):
    return {k: v.detach().to("cuda").requires_grad_(v.requires_grad) for k, v in cpu.items()}


def _write(dst, src):
    import torch
    with torch.no_grad():
        for k in dst:
            dst[k].detach().copy_(src[k].detach())


def _bits(t):
    return t.detach().contiguous().cpu().numpy().reshape(-1).view(np.uint8)


ROUNDS = 3


def _round(real, poison, call, blocker, monkeypatch):
    """Steps 2-4 of the module docstring on one side stream.  `decisive` says whether the round could have shown a wrong stream: the blocker
    lasted as long as it had to, and the side stream ran beside the null stream before the round and after it."""
    import torch
    s, tried = _side_stream(blocker)
    delayed = [k for k in real if not k.startswith("out_")]
    with torch.cuda.stream(s):                       # (everything the blocked call touches lives in s's part of the caching allocator)
        bufs, staged = _upload(poison), _upload(real)
        on_poison = tuple(t.detach().clone() for t in call(bufs))     # warm-up: kernels loaded, the allocator holds every block the call takes
        s.synchronize()
        host_ms = float("inf")
        for _ in range(3):                           # host wall time of the warmed-up call: the least of three, a preempted host is not the call
            t0 = time.perf_counter()
            call(bufs)
            host_ms = min(host_ms, (time.perf_counter() - t0) * 1e3)
            s.synchronize()
        _write(bufs, _upload(poison))                # poison and sentinels again
        s.synchronize()
    spy = _Spy(_lib.load())
    monkeypatch.setattr(_lib, "load", lambda: spy)
    need_ms = max(MIN_BLOCK_MS, HOST_FACTOR * host_ms)
    e0, e1, e_in = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True), torch.cuda.Event()
    with torch.cuda.stream(s):
        e0.record()
        blocker.enqueue(min(need_ms, MAX_BLOCK_MS))
        e1.record()
        _write({k: bufs[k] for k in delayed}, staged)
        e_in.record()
        got = call(bufs)
        returned_early = not e_in.query()
    s.synchronize()
    monkeypatch.undo()
    block_ms = e0.elapsed_time(e1)
    if block_ms < need_ms:                           # the clock the blocker counts in has changed: take the new rate
        blocker.per_ms *= 1.2 * need_ms / max(block_ms, 1.0)
    beside = _runs_beside_null(s, blocker)
    return SimpleNamespace(got=got, on_poison=on_poison, returned_early=returned_early, calls=spy.calls, stream=s.cuda_stream, need_ms=need_ms,
                           block_ms=block_ms, host_ms=host_ms, tried=tried, beside=beside,
                           decisive=need_ms <= MAX_BLOCK_MS and block_ms >= need_ms and beside)


def run(make_inputs, call, blocker, monkeypatch, no_wait, seed=1):
    """make_inputs(seed) -> dict of CPU tensors (floating leaves that take a gradient have requires_grad set; keys that start with "out_" are
    output buffers of an "into" form, filled with a sentinel); call(dict of device tensors) -> tuple of tensors, the forward results and, for
    differentiable ops, the gradients.

    Up to ROUNDS rounds, each on a side stream of its own, until one is decisive and, for an op documented as not waiting, has returned
    early.  The timing of a round depends on a shared machine: a blocker cut short by a clock change, a stream that the runtime moved onto the
    null stream's queue, or a host thread that was preempted between two lines make a round inconclusive, not wrong.  What every round must
    show is checked in every round (`check`).  For the wait check one early return is proof, since a call that waits for its stream can never
    return before the event behind the blocker; a call that does wait returns late in all rounds."""
    import torch
    real, poison = make_inputs(seed), make_inputs(seed + 1)
    assert real.keys() == poison.keys() and all(real[k].shape == poison[k].shape and real[k].dtype == poison[k].dtype for k in real)
    ref = call(_upload(real))
    torch.cuda.synchronize()
    rounds = []
    while len(rounds) < ROUNDS:
        rounds.append(_round(real, poison, call, blocker, monkeypatch))
        if rounds[-1].decisive and (rounds[-1].returned_early or not no_wait):
            break
    return SimpleNamespace(ref=ref, poison=poison, rounds=rounds)


def check(res, what, no_wait):
    for n, r in enumerate(res.rounds):
        print(f"stream order {what} round {n + 1}: blocker {r.block_ms:.1f} ms (needed {r.need_ms:.1f}), warmed host call {r.host_ms:.3f} ms, "
              f"returned early: {r.returned_early}, side stream: candidate {r.tried}, beside the null stream afterwards: {r.beside}, "
              f"library calls: {[c[0] for c in r.calls]}")
    ref = res.ref
    for r in res.rounds:                             # in every round: the result of stream order, and the stream at the C ABI
        assert r.stream not in (None, 0)
        assert len(r.got) == len(ref) == len(r.on_poison)
        for i, (g, w) in enumerate(zip(r.got, ref)):
            assert g.shape == w.shape and g.dtype == w.dtype, (what, i)
            assert np.array_equal(_bits(g), _bits(w)), f"{what}: result {i} differs from the default-stream run: the op did not run in stream order"
        # the case can tell the two inputs apart: on the poison the op gives something else
        assert any(not np.array_equal(_bits(g), _bits(w)) for g, w in zip(r.on_poison, ref)), f"{what}: poison and real inputs give the same result"
        assert r.calls, what
        for name, args in r.calls:
            if name in NO_STREAM:
                continue
            assert name in STREAM_LAST, f"{what}: {name} is not in this file's tables"
            assert args[-1] is not None and args[-1] != 0 and args[-1] == r.stream, f"{what}: {name} got stream {args[-1]}, torch's current stream is {r.stream}"
    last = res.rounds[-1]
    # the conditions that make the check decisive (not performance thresholds)
    assert last.need_ms <= MAX_BLOCK_MS, f"{what}: the call takes {last.host_ms:.1f} ms on the host, no blocker up to {MAX_BLOCK_MS} ms is 20 x that"
    assert last.block_ms >= last.need_ms, f"{what}: the blocker lasted {last.block_ms:.1f} ms, {last.need_ms:.1f} ms were needed"
    assert last.beside, f"{what}: in none of {len(res.rounds)} rounds did the side stream stay beside the null stream"
    if no_wait:
        assert last.returned_early, f"{what}: documented as not waiting, but in {len(res.rounds)} rounds the call returned only after its stream had caught up"


# ------------------------------------------------------------------------------------------ inputs
def _gen(seed):
    import torch
    return torch.Generator().manual_seed(seed)


def _randn(g, shape, dtype, scale=1.0, grad=False):
    import torch
    return (torch.randn(shape, generator=g) * scale).to(getattr(torch, dtype)).requires_grad_(grad)


def _ragged_mask(g, B, T, dtype="int32"):
    """0/1, row b keeps its first n_b tokens, 1 <= n_b <= T"""
    import torch
    n = torch.randint(1, T + 1, (B,), generator=g)
    return (torch.arange(T)[None, :] < n[:, None]).to(getattr(torch, dtype))


def _full(shape, value, dtype):
    import torch
    return torch.full(shape, value, dtype=getattr(torch, dtype))


def _backward(d, out, leaves, g="G"):
    for k in leaves:
        d[k].grad = None
    out.backward(d[g])
    return (out.detach(),) + tuple(d[k].grad for k in leaves)


def _into(op, d, *outs):
    """an "into" form: run it, the results are the whole output buffers (the sentinel columns beyond the record included)"""
    op()
    return tuple(d[k] for k in outs)


CASES = []


def case(name, no_wait):
    def add(fn):
        CASES.append(pytest.param(fn, no_wait, id=name))
        return fn
    return add


# ---- dhr_amd.lexical: dhr_lexical_head launches lexical_stats_kernel, lexical_fold_kernel<mode> and, with semantic reps, lexical_cls_kernel;
# ---- dhr_aggregate launches lexical_fold_kernel<AGG_FULL / AGG_SEMI> alone.  Nothing else depends on the shape.  Both wait: ordering only.
def _lexical_inputs(dtype, V, outs):
    def make(seed):
        g = _gen(seed)
        d = dict(logits=_randn(g, (3, 10, V), dtype, 3.0), w=_randn(g, (3, 9, 1), dtype), mask=_ragged_mask(g, 3, 9), cls=_randn(g, (3, 24), dtype))
        d.update({k: _full(*v) for k, v in outs.items()})
        return d
    return make


def _lexical_cases():
    from dhr_amd import lexical as LX
    for dtype, V in (("float16", 1082), ("float32", 4026)):          # dims 64 after 58 removed; aggregate(64): 58 removed, full and semi
        vdt = "float16" if dtype == "float16" else "float32"

        @case(f"lexical.lexical_reps-{dtype}", False)                  # stats, fold<RAW>
        def _(dtype=dtype, V=V):
            return _lexical_inputs(dtype, V, {}), lambda d: (LX.lexical_reps(d["logits"][:, 1:], d["w"], d["mask"]),)

        for cls in (False, True):                                      # stats, fold<DENSIFY> (+ cls)
            @case(f"lexical.densify_lexical_into-{dtype}-{'cls' if cls else 'nocls'}", False)
            def _(dtype=dtype, V=V, cls=cls, vdt=vdt):
                outs = dict(out_value=((3, 64 + 24 + 5), 7.0, vdt), out_index=((3, 64 + 3), 99, "uint8"))
                return _lexical_inputs(dtype, V, outs), lambda d: _into(lambda: LX.densify_lexical_into(
                    d["logits"][:, 1:], d["w"], d["mask"], d["out_value"][:, :64 + (24 if cls else 0)], d["out_index"][:, :64], 64, 58,
                    semantic_reps=d["cls"] if cls else None), d, "out_value", "out_index")

            for full in (True, False):                                 # stats, fold<AGG_FULL> / fold<AGG_SEMI> (+ cls)
                @case(f"lexical.aggregate_lexical_into-{'full' if full else 'semi'}-{dtype}-{'cls' if cls else 'nocls'}", False)
                def _(dtype=dtype, V=V, cls=cls, full=full, vdt=vdt):
                    outs = dict(out_value=((3, 64 + 24 + 5), 7.0, vdt))
                    return _lexical_inputs(dtype, V, outs), lambda d: _into(lambda: LX.aggregate_lexical_into(
                        d["logits"][:, 1:], d["w"], d["mask"], d["out_value"][:, :64 + (24 if cls else 0)], 64, full,
                        semantic_reps=d["cls"] if cls else None), d, "out_value")

        for full in (True, False):                                     # fold<AGG_FULL> / fold<AGG_SEMI> on [B, V] reps
            @case(f"lexical.aggregate-{'full' if full else 'semi'}-{dtype}", False)
            def _(dtype=dtype, V=V, full=full):
                return (lambda seed: dict(reps=_randn(_gen(seed), (3, V), dtype))), lambda d: (LX.aggregate(d["reps"], 64, full=full),)


# ---- dhr_amd.densify: dhr_densify launches densify_kernel<float / _Float16>; the index dtype is a kernel argument.  Enqueues and returns.
def _densify_cases():
    from dhr_amd import densify as DZ
    for dtype, dims, groups, remove, idt in (("float32", 64, 16, 58, "uint8"), ("float16", 8, 300, 2, "int16")):     # 300 groups: the int16 index
        V = remove + groups * dims

        @case(f"densify.densify-{dtype}-{idt}", True)
        def _(dtype=dtype, V=V, dims=dims, remove=remove):
            return (lambda seed: dict(reps=_randn(_gen(seed), (5, V), dtype))), lambda d: DZ.densify(d["reps"], dims, remove_dims=remove)

        @case(f"densify.densify_into-{dtype}-{idt}", True)
        def _(dtype=dtype, V=V, dims=dims, remove=remove, idt=idt):
            def make(seed):
                return dict(reps=_randn(_gen(seed), (5, V), dtype), out_value=_full((5, dims + 9), 7.0, "float16"), out_index=_full((5, dims + 3), 99, idt))
            return make, lambda d: _into(lambda: DZ.densify_into(d["reps"], d["out_value"], d["out_index"], dims, remove), d, "out_value", "out_index")


# ---- dhr_amd.lexical_proj: dhr_lexical_proj_head launches proj_count, proj_scan, proj_fill, proj_stats, proj_combine, proj_fold<false>, then
# ---- (lexical_record_from_reps) lexical_fold_kernel<mode> unless raw, and lexical_cls_kernel with semantic reps.  The host code has no slab
# ---- path of its own (one launch of each whatever H), so no H > 768 shape is added.  Enqueues and returns.
def _proj_inputs(B, L, V, H, outs, bias=True, grad=False, wdt="float16"):
    def make(seed):
        g = _gen(seed)
        d = dict(hidden=_randn(g, (B, L, H), "float16", 1.0, grad), weight=_randn(g, (V, H), "float16", 2.0 / H ** 0.5, grad),
                 w=_randn(g, (B, L - 1, 1), wdt, 1.0, grad), mask=_ragged_mask(g, B, L - 1), cls=_randn(g, (B, 24), "float16"))
        if bias:
            d["bias"] = _randn(g, (V,), "float32", 0.5, grad)
        if grad:
            d["G"] = _randn(g, (B, V), "float32")
        d.update({k: _full(*v) for k, v in outs.items()})
        return d
    return make


def _lexical_proj_cases():
    from dhr_amd import lexical_proj as LP
    # (B, L, V, H) of tests/test_lexical_proj_train.py::RANDOM; densify dims / remove; aggregate dims full / semi
    for (B, L, V, H), dims, remove, agg_full, agg_semi in (((5, 70, 762, 72), 64, 58, 32, 64), ((2, 9, 202, 24), 8, 2, 8, 8)):
        tag = f"{B}x{L}x{V}x{H}"

        @case(f"lexical_proj.lexical_reps-{tag}", True)                # the six proj kernels (raw: the fold writes the output itself)
        def _(B=B, L=L, V=V, H=H):
            return _proj_inputs(B, L, V, H, {}), lambda d: (LP.lexical_reps(d["hidden"][:, 1:], d["weight"], d["bias"], d["w"], d["mask"]),)

        @case(f"lexical_proj.densify_lexical_into-{tag}", True)        # + lexical_fold_kernel<DENSIFY>, lexical_cls_kernel
        def _(B=B, L=L, V=V, H=H, dims=dims, remove=remove):
            outs = dict(out_value=((B, dims + 24 + 5), 7.0, "float16"), out_index=((B, dims + 3), 99, "uint8"))
            return _proj_inputs(B, L, V, H, outs), lambda d: _into(lambda: LP.densify_lexical_into(
                d["hidden"][:, 1:], d["weight"], d["bias"], d["w"], d["mask"], d["out_value"][:, :dims + 24], d["out_index"][:, :dims], dims, remove,
                semantic_reps=d["cls"]), d, "out_value", "out_index")

        @case(f"lexical_proj.aggregate_lexical_into-full-{tag}", True)  # + lexical_fold_kernel<AGG_FULL>, lexical_cls_kernel
        def _(B=B, L=L, V=V, H=H, agg=agg_full):
            outs = dict(out_value=((B, agg + 24 + 5), 7.0, "float32"))
            return _proj_inputs(B, L, V, H, outs), lambda d: _into(lambda: LP.aggregate_lexical_into(
                d["hidden"][:, 1:], d["weight"], d["bias"], d["w"], d["mask"], d["out_value"][:, :agg + 24], agg, True, semantic_reps=d["cls"]), d, "out_value")

        @case(f"lexical_proj.aggregate_lexical_into-semi-nobias-{tag}", True)   # + lexical_fold_kernel<AGG_SEMI>; no bias, no cls
        def _(B=B, L=L, V=V, H=H, agg=agg_semi):
            outs = dict(out_value=((B, agg + 5), 7.0, "float16"))
            return _proj_inputs(B, L, V, H, outs, bias=False), lambda d: _into(lambda: LP.aggregate_lexical_into(
                d["hidden"][:, 1:], d["weight"], None, d["w"], d["mask"], d["out_value"][:, :agg], agg, False), d, "out_value")


# ---- dhr_amd.lexical_train: forward lexical_stats_kernel, lexical_fold_tok_kernel; backward lexical_route_sum_kernel<RT_SMALL> or <RT_BIG>
# ---- (ceil(T / 16) * B >= 512), then lexical_dx_kernel<vec> or <not vec> (rows of V values at multiples of 4 bytes or not).  Enqueue and return.
def _lexical_train_cases():
    from dhr_amd import lexical_train as LT
    for B, L, V, dtype, view, sites in ((3, 9, 1082, "float16", False, "route_sum<SMALL>, dx<vec>"),        # rows of tests/test_lexical_train.py::RANDOM
                                        (3, 12, 203, "float16", True, "route_sum<SMALL>, dx<not vec>"),    # 406-byte rows, the [:, 1:] view
                                        (520, 2, 203, "float32", False, "route_sum<BIG>, dx<vec>")):       # 520 single-token passages: RT_BIG
        @case(f"lexical_train.lexical_reps-{B}x{L}x{V}-{dtype}", True)
        def _(B=B, L=L, V=V, dtype=dtype, view=view):
            def make(seed):
                g = _gen(seed)
                return dict(logits=_randn(g, (B, L, V), dtype, 3.0, True), w=_randn(g, (B, L - 1, 1), dtype, 1.0, True), mask=_ragged_mask(g, B, L - 1),
                            G=_randn(g, (B, V), "float32"))

            def call(d):
                x = d["logits"][:, 1:] if view else d["logits"]
                return _backward(d, LT.lexical_reps(x, d["w"], d["mask"], skip_tokens=0 if view else 1), ("logits", "w"))
            return make, call


# ---- dhr_amd.lexical_proj_train: forward the six proj kernels (fold<true>); backward proj_route_sum_kernel<RT_SMALL / RT_BIG>, proj_zero_rows,
# ---- proj_grad_kernel<2, NC> once per slab of H (NC = 2, 6 or 12 chunk registers), proj_grad_combine_kernel where dhidden is split over the
# ---- vocabulary, proj_grad_kernel<3, NC> once per slab for the weight (the first slab writes dbias).  Enqueue and return.
def _lexical_proj_train_cases():
    from dhr_amd import lexical_proj_train as LPT
    for (B, L, V, H), bias, sites in (((5, 70, 762, 72), True, "route_sum<SMALL>, grad<.,2>, split dhidden + combine"),
                                      ((5, 70, 762, 72), False, "the same without bias: no dbias"),
                                      ((130, 64, 515, 64), True, "route_sum<BIG>, unsplit dhidden: no combine"),
                                      ((6, 50, 1030, 136), True, "grad<.,6>"),
                                      ((3, 20, 515, 776), True, "two slabs: grad<.,12> twice per pass"),
                                      ((4, 40, 1030, 1024), True, "two launches and one combine")):
        @case(f"lexical_proj_train.lexical_reps-{B}x{L}x{V}x{H}-{'bias' if bias else 'nobias'}", True)
        def _(B=B, L=L, V=V, H=H, bias=bias):
            leaves = ("hidden", "weight", "w") + (("bias",) if bias else ())
            return _proj_inputs(B, L, V, H, {}, bias=bias, grad=True, wdt="float32"), lambda d: _backward(d, LPT.lexical_reps(
                d["hidden"], d["weight"], d.get("bias"), d["w"], d["mask"], skip_tokens=1), leaves)


# ---- dhr_amd.gip_scores.  dhr_gip_scores: group > 0 gip_pair_fwd_kernel; group = 0 gip_fwd_kernel<1, 1> (16 x 16 tiles) or <2, 4> (32 x 64
# ---- tiles, from 256 tile steps), and gip_fold_kernel when dims are split (a workspace).  dhr_gip_scores_backward: gip_pair_bwd_kernel, or
# ---- gip_bwd_kernel once per side.  The fused forms add dhr_densify per side in front and dhr_densify_backward per side behind.  None waits.
def _reps(g, rows, dims, groups, remove, dtype):
    import torch
    x = torch.rand((rows, remove + groups * dims), generator=g) * 3 + 0.05
    x = x * (torch.rand(x.shape, generator=g) < 0.5) * (torch.randint(0, 2, x.shape, generator=g) * 2 - 1)
    return x.to(getattr(torch, dtype)).requires_grad_(True)


def _gip_cases():
    import torch
    from dhr_amd import gip_scores as GS
    # gip_scores on densified arrays: (n_q, n_p, group, dims, groups, dtype, sites)
    for n_q, n_p, group, dims, groups, dtype, sites in ((1, 7, 0, 96, 5, "float32", "fwd<1,1> over 3 slices + fold: the smallest workspace"),
                                                        (5, 11, 0, 24, 5, "float16", "fwd<1,1>, one slice: no workspace"),
                                                        (9, 36, 4, 33, 4, "float16", "pair_fwd, pair_bwd")):
        @case(f"gip_scores.gip_scores-{n_q}x{n_p}-g{group}-d{dims}-{dtype}", True)
        def _(n_q=n_q, n_p=n_p, group=group, dims=dims, groups=groups, dtype=dtype):
            def make(seed):
                g = _gen(seed)
                return dict(qv=_randn(g, (n_q, dims), dtype, 1.0, True), qi=torch.randint(0, groups, (n_q, dims), generator=g, dtype=torch.uint8),
                            pv=_randn(g, (n_p, dims), dtype, 1.0, True), pi=torch.randint(0, groups, (n_p, dims), generator=g, dtype=torch.uint8),
                            G=_randn(g, (n_q, group if group else n_p), "float32"))
            return make, lambda d: _backward(d, GS.gip_scores(d["qv"], d["qi"], d["pv"], d["pi"], group), ("qv", "pv"))

    # the fused forms on [B, V] reps: (form, n_q, n_p, dims, groups, remove, dtype, sites)
    for form, n_q, n_p, dims, groups, remove, dtype, sites in (
            ("listwise", 1, 7, 96, 5, 10, "float32", "densify x 2, fwd<1,1> + fold (workspace), bwd x 2, densify_bwd x 2"),
            ("listwise", 5, 11, 24, 5, 2, "float16", "no workspace"),
            ("listwise", 100, 200, 520, 2, 570, "float32", "fwd<2,4> over 17 slices + fold"),
            ("pairwise", 9, 36, 33, 4, 1, "float16", "pair_fwd, pair_bwd"),
            ("pairwise", 65, 130, 70, 300, 3, "float32", "300 groups: the int16 index through densify, the pair kernels and densify_bwd"),
            ("paired", 13, 13, 50, 6, 570, "float16", "group = 1: the pair kernels"),
            ("paired", 1, 19, 50, 6, 570, "float32", "one query broadcast: group = 0, two slices + fold")):
        @case(f"gip_scores.{form}_gip_scores-{n_q}x{n_p}-d{dims}-{dtype}", True)
        def _(form=form, n_q=n_q, n_p=n_p, dims=dims, groups=groups, remove=remove, dtype=dtype):
            shape = {"listwise": (n_q, n_p), "pairwise": (n_q, n_p // n_q), "paired": (max(n_q, n_p),)}[form]

            def make(seed):
                g = _gen(seed)
                return dict(q=_reps(g, n_q, dims, groups, remove, dtype), p=_reps(g, n_p, dims, groups, remove, dtype),
                            G=_randn(g, tuple(n for n in shape if n != 1) if form != "paired" else shape, "float32"))

            def call(d):
                if form == "listwise":
                    s = GS.listwise_gip_scores(d["q"], d["p"], n_q, dims, remove)
                elif form == "pairwise":
                    s = GS.pairwise_gip_scores(d["q"], d["p"], n_q, n_p // n_q, dims, remove)
                else:
                    s = GS.paired_gip_scores(d["q"], d["p"], dims, remove)
                return _backward(d, s, ("q", "p"))
            return make, call


# ---- dhr_amd.maxsim_scores: forward maxsim_fwd_kernel<T, 1, multi> (one chunk of D or several; two queries per wave only from 512 workgroups);
# ---- backward maxsim_bwd_q_kernel, maxsim_bwd_p_kernel.  The only memset of the entry point (zeros for a side when the other side has no rows)
# ---- is not reachable through the wrapper, which answers an empty side itself.  Enqueue and return.
def _maxsim_cases():
    from dhr_amd import maxsim_scores as MS
    for (A, n, Lq, Lp, D), dtype in (((3, 8, 31, 149, 128), "float16"), ((5, 5, 7, 300, 24), "float32")):
        for group in (0, n):
            @case(f"maxsim_scores.maxsim_scores-{A}x{n}x{Lq}x{Lp}x{D}-{dtype}-g{group}", True)
            def _(A=A, n=n, Lq=Lq, Lp=Lp, D=D, dtype=dtype, group=group):
                def make(seed):
                    g = _gen(seed)
                    return dict(q=_randn(g, (A, Lq, D), dtype, 1.0, True), p=_randn(g, (A * n, Lp, D), dtype, 1.0, True),
                                G=_randn(g, (A, group if group else A * n), "float32"))
                return make, lambda d: _backward(d, MS.maxsim_scores(d["q"], d["p"], group), ("q", "p"))


# ---- dhr_amd.aggretriever_train: one launch per entry point: aggregate_route_kernel<T, full>, aggregate_backward_kernel,
# ---- term_weight_head_kernel, term_weight_head_backward_kernel.  Enqueue and return.
def _aggretriever_cases():
    import torch
    from dhr_amd import aggretriever_train as AT
    for V, dims, full, dtype in ((186, 16, True, "float16"), (57, 9, False, "float32")):        # the small shapes of tests/test_aggretriever_train.py
        @case(f"aggretriever_train.aggregate-{'full' if full else 'semi'}-{V}-{dtype}", True)
        def _(V=V, dims=dims, full=full, dtype=dtype):
            def make(seed):
                g = _gen(seed)
                return dict(reps=_randn(g, (5, V), dtype, 1.0, True), G=_randn(g, (5, dims), dtype))
            return make, lambda d: _backward(d, AT.aggregate(d["reps"], dims, full), ("reps",))

    for idt, wdt in (("int64", "float32"), ("int32", "float16")):
        @case(f"aggretriever_train.term_weight_reps-{idt}-{wdt}", True)
        def _(idt=idt, wdt=wdt):
            def make(seed):
                g = _gen(seed)                                           # ids inside the vocabulary, repeats within a row
                return dict(ids=torch.randint(0, 203, (4, 12), generator=g).to(getattr(torch, idt)), w=_randn(g, (4, 11, 1), wdt, 1.0, True),
                            G=_randn(g, (4, 203), "float32"))
            return make, lambda d: _backward(d, AT.term_weight_reps(d["ids"], d["w"], 203, 1), ("w",))


# ---- dhr_amd.dist: dhr_merge_topk launches merge_topk_kernel (up to 16 384 entries per query, in the LDS) or, beyond, mg_init / mg_score /
# ---- mg_emit kernels around two hipcub segmented sorts with stream-ordered allocations; dhr_merge_topk_lists launches merge_lists_kernel<NL>;
# ---- lists beyond the LDS go to merge_topk.  Both enqueue and return.
def _lists(g, n_lists, q, ll):
    """[n_lists, q, ll] lists sorted (score desc, row asc) with many ties, ragged (-inf, -1) tails"""
    import torch
    s = (torch.randn((n_lists, q, ll), generator=g) * 4).round() / 4 + 0.0
    r = torch.randperm(n_lists * q * ll * 3, generator=g)[:n_lists * q * ll].reshape(n_lists, q, ll)
    r = r.sort(-1).values
    s = s.sort(-1, descending=True).values                               # rows ascend along the list, so also within equal scores
    fill = torch.randint(0, ll + 1, (n_lists, q, 1), generator=g)
    pad = torch.arange(ll)[None, None, :] >= fill
    return s.masked_fill(pad, float("-inf")), r.masked_fill(pad, -1)


def _dist_cases():
    import torch
    from dhr_amd import dist as DI
    for q, n_in, k, sites in ((3, 200, 10, "merge_topk_kernel"), (2, 16500, 50, "mg_init, sort, mg_score, sort, mg_emit")):
        @case(f"dist.merge_topk-{q}x{n_in}", True)
        def _(q=q, n_in=n_in, k=k):
            def make(seed):
                g = _gen(seed)
                rows = torch.stack([torch.randperm(n_in * 2, generator=g)[:n_in] for _ in range(q)])
                rows[torch.rand((q, n_in), generator=g) < 0.1] = -1
                return dict(scores=(torch.randn((q, n_in), generator=g) * 4).round() / 4 + 0.0, rows=rows)
            return make, lambda d: DI.merge_topk(d["scores"], d["rows"], k)

    for n_lists, q, ll, k, rows, sites in ((4, 3, 50, 20, True, "merge_lists_kernel<4>"), (2, 3, 50, 20, False, "merge_lists_kernel<2>, scores only"),
                                           (4, 2, 4000, 30, True, "16 000 entries of 12 bytes: beyond the LDS, merge_topk_kernel")):
        @case(f"dist.merge_sorted_lists-{n_lists}x{q}x{ll}-{'rows' if rows else 'norows'}", True)
        def _(n_lists=n_lists, q=q, ll=ll, k=k, rows=rows):
            def make(seed):
                s, r = _lists(_gen(seed), n_lists, q, ll)
                return dict(scores=s, rows=r) if rows else dict(scores=s)
            return make, lambda d: tuple(t for t in DI.merge_sorted_lists(d["scores"], d.get("rows"), k) if t is not None)


# ---- dhr_amd.retrieval.quantize_index on torch CUDA tensors: dhr_pq_train_nbits launches pq_init_kernel, then per iteration three memsets,
# ---- pq_assign_kernel<0> and pq_update_kernel, and copies the error to the host; dhr_pq_encode_nbits launches pq_assign_kernel<0>;
# ---- dhr_pq_decode_nbits launches pq_decode_kernel.  All three wait: ordering only.
# ---- The k-means sums are float atomics, whose order is free: the values are multiples of 1/8 in [-4, 4], so every partial sum of up to
# ---- 2 000 of them is exact in fp32 and the codebooks do not depend on the order.  (The returned error does, and is not compared.)
def _pq_values(g, n, d):
    import torch
    return (torch.randint(-32, 33, (n, d), generator=g) / 8.0).to(torch.float16)


def _pq_cases():
    import torch
    from dhr_amd.retrieval import quantize_index as QI
    n, d, M, nbits = 2000, 32, 4, 4

    @case("quantize_index.train_and_encode", False)
    def _():
        return (lambda seed: dict(values=_pq_values(_gen(seed), n, d))), lambda d_: QI.train_and_encode(d_["values"], M, nbits, iters=3)[:2]

    @case("quantize_index.encode", False)
    def _():
        def make(seed):
            g = _gen(seed)
            return dict(values=_pq_values(g, n, d), cb=_randn(g, (M, 1 << nbits, d // M), "float32", 2.0))
        return make, lambda d_: (QI.encode(d_["values"], d_["cb"], nbits),)

    @case("quantize_index.decode", False)
    def _():
        def make(seed):
            g = _gen(seed)
            return dict(cb=_randn(g, (M, 1 << nbits, d // M), "float32", 2.0), codes=torch.randint(0, 1 << nbits, (n, M), generator=g, dtype=torch.uint8))
        return make, lambda d_: (QI.decode(d_["cb"], d_["codes"]),)


for _register in (_lexical_cases, _densify_cases, _lexical_proj_cases, _lexical_train_cases, _lexical_proj_train_cases, _gip_cases, _maxsim_cases,
                  _aggretriever_cases, _dist_cases, _pq_cases):
    _register()


# ------------------------------------------------------------------------------------------ the tests
@pytest.mark.gpu
def test_control_wrong_stream_reads_poison(blocker, monkeypatch):
    """The harness on a stand-in op that clones its inputs on torch's default stream (no library code): it must see the POISON, not the real
    inputs.  This shows on the machine at hand that the blocker is long enough and that a side stream and the null stream do not serialise;
    without it the cases below could not observe a wrong stream."""
    import torch

    def make(seed):
        g = _gen(seed)
        return dict(a=_randn(g, (64, 1000), "float32"), b=torch.randint(0, 1000, (64, 100), generator=g))

    def wrong_stream_clone(d):
        with torch.cuda.stream(torch.cuda.default_stream()):
            return tuple(d[k].clone() for k in sorted(d))

    res = run(make, wrong_stream_clone, blocker, monkeypatch, True)
    for n, r in enumerate(res.rounds):
        print(f"control round {n + 1}: blocker {r.block_ms:.1f} ms (calibration run {blocker.calibrated_ms:.1f} ms, "
              f"{'torch.cuda._sleep' if blocker.eye is None else 'matmul chain'}), warmed host call {r.host_ms:.3f} ms, returned early: "
              f"{r.returned_early}, side stream: candidate {r.tried}, beside the null stream afterwards: {r.beside}")
    r = res.rounds[-1]
    assert r.decisive and r.need_ms >= MIN_BLOCK_MS and r.returned_early
    for got, ref, k in zip(r.got, res.ref, sorted(res.poison)):
        assert np.array_equal(_bits(got), _bits(res.poison[k])), f"{k}: a clone on the default stream did not see the poison"
        assert not np.array_equal(_bits(got), _bits(ref))


@pytest.mark.gpu
@pytest.mark.parametrize("build, no_wait", CASES)
def test_op_runs_in_stream_order(build, no_wait, blocker, monkeypatch, request):
    make_inputs, call = build()
    check(run(make_inputs, call, blocker, monkeypatch, no_wait), request.node.callspec.id, no_wait)
