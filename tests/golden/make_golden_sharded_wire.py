"""Records tests/golden/sharded_wire.json: what every rank of a sharded step puts on the wire.  Recorded at the commit BEFORE
dhr_amd/csrc/sharded.hip was rewritten around one step plan (sharded_plan.h); tests/test_sharded_wire.py replays the same cases with this
module's own functions and asserts equality, so the rewrite is pinned byte for byte: the sequence of exchanges, their sizes, and the block
each rank sends (payload, padding and status record).

Ranks are spawned over local gloo like tests/test_dist_gloo.py, and drive dhr_search_sharded_host (dhr_amd.dist.sharded_search_host) with that
module's _FakeShard classes on INTEGER-valued data: every score is exact, so every byte is.  dist._host_allgather is wrapped in the worker:
each call logs its byte count and the SHA-256 of the block this rank sends.  Per case and rank: that sequence, the shard's `calls`, the
status, and the returned rows.  (The allocation-failure cases of test_dist_gloo.py are not pinned: their sequences depend on the step's
allocation count, which is free to change.)

    python tests/golden/make_golden_sharded_wire.py        # rewrites sharded_wire.json"""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
PATH = os.path.join(HERE, "sharded_wire.json")
WORLDS = (2, 3, 5)
# where the failing rank's callback raises -> (shard class, method)
FAIL_POINTS = {"begin": ("plain", "search_begin"), "finish": ("plain", "search_finish"), "mid": ("mid", "search_mid"),
               "pre": ("pre", "search_pre"), "rest": ("pre", "search_begin_rest"), "search": ("plain", "search")}


def cases(world):
    """(name, shard kind, layout, failing callback or None) in the order the worker runs them."""
    out = [("plain", "plain", "random", None), ("mid", "mid", "random", None), ("pre", "pre", "random", None),
           ("mismatch", "plain", "random", None),          # the last rank reports another union rank: local thresholds for the whole batch
           ("repair", "plain", "adversarial", None)]       # query 0's best rows sit on sample positions: threshold too high, the query is redone
    if world == 5:
        out.append(("prefix", "pre", "big", None))         # k = 300: prefix_len gives kk = 256 < k, the lists travel as prefixes
    for where, (kind, _name) in FAIL_POINTS.items():       # (a failure in the repair step needs a repair step first)
        out.append(("fail_" + where, kind, "adversarial" if where == "search" else "random", where))
    return out


def _data(layout, world):
    from dhr_amd import dist as D
    rng = np.random.default_rng(7)
    n, k, nq = (6001, 300, 3) if layout == "big" else (4000, 60, 5)
    cv = rng.integers(-3, 4, (n, 16)).astype(np.float32)
    q = rng.integers(-2, 3, (nq, 16)).astype(np.float32)
    if layout == "adversarial":
        for r_ in range(world):
            lo_ = D.shard_bounds(n, world, r_)[0]
            cv[lo_:lo_ + 80:4] += 3.0 * q[0]
    return cv, q, k


def _worker(rank, world, port, tmp):
    sys.path.insert(0, ROOT)
    import ctypes as C
    import torch.distributed as dist
    from dhr_amd import _lib, dist as D
    from tests import test_dist_gloo as T
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    wire = []
    plain_allgather = D._host_allgather

    def logging_allgather(group, device=None):
        inner = plain_allgather(group, device)

        def fn(user, send, recv, nbytes):
            wire.append([int(nbytes), hashlib.sha256(C.string_at(send, nbytes)).hexdigest()])
            return inner(user, send, recv, nbytes)
        return _lib.ALLGATHER_FN(fn)
    D._host_allgather = logging_allgather
    try:
        kinds = {"plain": T._FakeShard, "mid": T._FakeShardMid, "pre": T._FakeShardPre}
        record = {}
        for name, kind, layout, fail in cases(world):
            cv, q, k = _data(layout, world)
            lo, hi = D.shard_bounds(cv.shape[0], world, rank)
            cls = kinds[kind]
            if fail is not None and rank == world - 1:
                def boom(self, *a):
                    raise RuntimeError("injected shard failure")
                cls = type("Failing", (cls,), {FAIL_POINTS[fail][1]: boom})
            shard = cls(cv[lo:hi], lo, r_skew=(3 if name == "mismatch" and rank == world - 1 else 0))
            del wire[:]
            dist.barrier()
            status, rows = 0, None
            try:
                rows = D.sharded_search_host(shard, q, None, k)[1].tolist()
            except _lib.DhrError as e:
                status = int(e.status)
            record[name] = {"wire": [list(w) for w in wire], "calls": list(shard.calls), "status": status, "rows": rows}
        with open(os.path.join(tmp, "rank%d.json" % rank), "w") as f:
            json.dump(record, f)
    finally:
        D._host_allgather = plain_allgather
        dist.destroy_process_group()


def record_world(world, tmp, port):
    """-> {case: [one record per rank]}"""
    import torch.multiprocessing as mp
    mp.spawn(_worker, args=(world, port, str(tmp)), nprocs=world, join=True)
    per_rank = [json.load(open(os.path.join(str(tmp), "rank%d.json" % r))) for r in range(world)]
    return {name: [per_rank[r][name] for r in range(world)] for name, *_ in cases(world)}


def main():
    import tempfile
    sys.path.insert(0, ROOT)
    out = {}
    for world in WORLDS:
        with tempfile.TemporaryDirectory() as tmp:
            got = record_world(world, tmp, 25100 + (os.getpid() % 1500) + world)
        assert "search5" not in got["plain"][0]["calls"] and got["repair"][0]["calls"][-1].startswith("search"), got["repair"][0]["calls"]
        assert got["mismatch"][0]["calls"] == ["search5"], got["mismatch"][0]["calls"]
        out[str(world)] = got
        for name, recs in got.items():
            print(world, name, [w[0] for w in recs[0]["wire"]], recs[0]["calls"], [r["status"] for r in recs])
    with open(PATH, "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")
    print(PATH, os.path.getsize(PATH), "bytes")


if __name__ == "__main__":
    main()
