"""Host-visible time of one sharded step (profiles/sharded_refactor_timing.txt), one process per measurement:

    DHR_HIP_LIB=<libdhr_hip.so> python tools/sharded_step_time.py <tag>     -> one JSON line, milliseconds

local:   dhr_search_sharded_local (dist.search_sharded_local) on 4 shards of the 400 000-row hybrid pair of
         tests/test_gpu_parity.py::test_search_sharded_local_c_abi, k = 1000, sample period 4;
world1:  dhr_search_sharded (dist.sharded_search) at world size 1 on the first of those shards.
Wall clock around the call (both entry points return with the result delivered), 2 warm-ups, then 6 timed runs each.  DHR_HIP_LIB
(dhr_amd/_lib.py) picks the library, so a build of another commit is timed with the same script in the same session: alternate the two."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from dhr_amd import _lib, dist as D, synth  # noqa: E402
from dhr_amd.retrieval import gip_retrieval as G  # noqa: E402

N, NS, K, WARM, REPS = 400_000, 4, 1000, 2, 6


def timed(fn):
    for _ in range(WARM):
        fn()
    out = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        fn()
        out.append(round((time.perf_counter() - t0) * 1e3, 3))
    return out


def main(tag):
    cv, ci, qv, qi = synth.make_pair(22, N, 12, 768, 64)
    q32 = qv.astype(np.float32)
    shards = []
    for sh in range(NS):
        lo, hi = G.shard_bounds(N, NS, sh)
        shards.append(G.GipIndex(cv[lo:hi], ci[lo:hi], row_offset=lo))
        shards[-1].set_param(_lib.PARAM_SAMPLE_PERIOD, 4)
    try:
        local = timed(lambda: D.search_sharded_local(shards, q32, qi, K))
        world1 = timed(lambda: D.sharded_search(shards[0], q32, qi, K))
        rows = D.search_sharded_local(shards, q32, qi, K)[1].cpu().numpy()
    finally:
        for s in shards:
            s.close()
    print(json.dumps({"tag": tag, "lib": os.environ.get("DHR_HIP_LIB", "in-tree"), "local_ms": local, "world1_ms": world1,
                      "local_median_ms": float(np.median(local)), "world1_median_ms": float(np.median(world1)),
                      "rows_checksum": int(rows.astype(np.uint64).sum())}))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "lib")
