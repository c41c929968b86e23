"""How the entry points of api.hip and pq_adc.hip answer bad arguments, and what the two host merges return: tests/golden/entry_points.json was
recorded by tests/golden/make_golden_entry_points.py at the commit before their host code was rewritten (one staging vocabulary, one error style),
and this module recomputes it with the recorder's own collect_checks().  Every case is a validation exit that is reached before the library
touches the device -- (status, exact dhr_last_error text) -- so no GPU is needed; the cases whose name says "beats" violate two rules at once
and pin which of them answers."""
import importlib.util
import json
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def gen():
    spec = importlib.util.spec_from_file_location("make_golden_entry_points", os.path.join(HERE, "golden", "make_golden_entry_points.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def pinned(gen):
    with open(gen.PATH_CHECKS) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def got(gen):
    return gen.collect_checks()


def test_the_table_covers_every_touched_entry_point(pinned):
    exits = pinned["exits"]
    for prefix in ("densify_", "pq_train_", "pq_train_plain_", "pq_encode_", "pq_encode_plain_", "pq_decode_", "pq_decode_plain_", "pq_create_", "pq_search_null",
                   "pq_adc_scores_null", "pq_last_scan_null", "merge_", "merge_host_", "lists_", "lists_host_", "search_mid_", "search_begin_rest_", "search_finish_",
                   "search_begin_", "search_pre_", "search_async_mid_", "search_async_pre_", "search_async_begin_rest_", "search_async_begin_", "search_async_finish_",
                   "sample_rank_", "union_rank_", "mid_ranks_", "pre_ranks_", "select_merge_"):
        assert any(name.startswith(prefix) for name in exits), prefix
    assert sum("beats" in name for name in exits) >= 20
    statuses = {v[0] for name, v in exits.items() if len(v) == 2 and isinstance(v[1], str)}
    assert statuses == {0, -1, -2}, statuses          # DHR_OK (an empty batch), DHR_ERR_INVALID, DHR_ERR_UNSUPPORTED


def test_validation_exits_equal_the_parent(pinned, got):
    assert sorted(got["exits"]) == sorted(pinned["exits"])
    wrong = {name: (got["exits"][name], want) for name, want in pinned["exits"].items() if got["exits"][name] != want}
    assert not wrong, wrong


def test_host_merges_equal_the_parent(pinned, got):
    assert got["host_merges"] == pinned["host_merges"]
    assert all(v[0] == 0 for v in pinned["host_merges"].values())
