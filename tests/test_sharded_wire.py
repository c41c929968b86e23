"""What a sharded step puts on the wire, pinned to the commit before dhr_amd/csrc/sharded.hip was rewritten around one step plan:
tests/golden/sharded_wire.json was recorded there by tests/golden/make_golden_sharded_wire.py, and this module replays the same cases with the
generator's own worker.  Per case and per rank the sequence of exchanges (byte count and SHA-256 of the block the rank sends: payload,
padding and status record), the shard callbacks that ran, the status and the returned rows must equal the recording: clean steps with
plain / second-agreement / two-round shards, a rank mismatch (local path), a repair step, list prefixes shorter than k (world 5, k = 300),
and a failing callback at each of six points, where the sequence ends at the first gather that carries the status."""
import importlib
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def _generator():
    """The recording script as a module the spawned ranks can import too (they inherit sys.path and unpickle its worker by module name)."""
    golden = os.path.join(HERE, "golden")
    if golden not in sys.path:
        sys.path.insert(0, golden)
    return importlib.import_module("make_golden_sharded_wire")


@pytest.mark.parametrize("world", [2, 3, 5])
def test_sharded_wire_equals_recording(tmp_path, world):
    gen = _generator()
    want = json.load(open(gen.PATH))[str(world)]
    got = gen.record_world(world, tmp_path, 24100 + (os.getpid() % 1500) + world)
    assert list(got) == list(want) == [name for name, *_ in gen.cases(world)]
    for name in want:
        for rank in range(world):
            g, w = got[name][rank], want[name][rank]
            assert [x[0] for x in g["wire"]] == [x[0] for x in w["wire"]], (name, rank, "byte counts")
            assert g["wire"] == w["wire"], (name, rank, "sent blocks")
            assert g["calls"] == w["calls"], (name, rank)
            assert g["status"] == w["status"], (name, rank)
            assert g["rows"] == w["rows"], (name, rank)
