"""What the search controller plans, pinned to the commit before it was rewritten around one search plan: tests/golden/controller_plan.json
was recorded there by tests/golden/make_golden_controller_plan.py, and this module recomputes it with the generator's own collect functions.
Everything compared is an integer, an exactly representable count or a digest of an array that the search determines: equality is exact.
Candidate counts are pinned on the one-bucket image of the indexes only: the default image deals index values to two buckets by a histogram
that the build sums with floating-point atomics, so its bounds -- never its results above the thresholds -- differ from build to build
(the generator's comment at IMAGES); of the staged results only what reaches the agreed thresholds is compared, and the merged top-k."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def gen():
    spec = importlib.util.spec_from_file_location("make_golden_controller_plan", os.path.join(HERE, "golden", "make_golden_controller_plan.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def pinned(gen):
    with open(gen.PATH) as f:
        want = json.load(f)
    assert len(want["ranks"]) == sum(len(c) for c in gen.RANK_CASES.values()) and len(want["search_stats"]) == 3 * len(gen.STAT_CASES) * len(gen.IMAGES) and len(want["staged"]) == 6 * len(gen.IMAGES)
    return want


@pytest.fixture(scope="module")
def lib(gen):
    import sys
    if gen.ROOT not in sys.path:
        sys.path.insert(0, gen.ROOT)
    from dhr_amd import _lib
    from dhr_amd.retrieval import gip_retrieval as G
    _lib.load()
    return G, _lib


def _assert_pinned(gen, got, want):
    """every field of the file, with the file's value"""
    for case, fields in want.items():
        assert fields, case
        assert gen.keep_equal(fields, got[case]) == fields, (case, {f: (got[case].get(f), v) for f, v in fields.items() if got[case].get(f) != v})


def test_rank_queries_equal_the_parent(gen, pinned, lib):
    _assert_pinned(gen, gen.collect_ranks(*lib), pinned["ranks"])


def test_search_stats_equal_the_parent(gen, pinned, lib):
    _assert_pinned(gen, gen.collect_search_stats(*lib), pinned["search_stats"])


def test_staged_sequences_equal_the_parent(gen, pinned, lib):
    _assert_pinned(gen, gen.collect_staged(*lib), pinned["staged"])
