"""What the entry points of api.hip and pq_adc.hip compute, pinned to the commit before their host code was rewritten around one staging
vocabulary and one error style: tests/golden/entry_points_gpu.json was recorded there, twice, by tests/golden/make_golden_entry_points.py, and
this module recomputes it with the recorder's own collect().  dhr_search, dhr_search_rerank, dhr_score_rows and the debug hooks on a 1000-row
shard with a row offset (fp16 and int8 gated image), dhr_densify, PQ training / encoding / decoding, the dhr_pq_* handle over 40 000 rows (several
blocks, a workspace that regrows) and the device merges, each from host and from device memory.  Everything compared is an integer, the hex form
of a float or a digest of an output array, so equality is exact.  A field is missing from the file only where the two recordings at the parent
disagreed; the file names each one under "_dropped" and only the float-atomic sum of the PQ training error may stand there."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def gen():
    spec = importlib.util.spec_from_file_location("make_golden_entry_points", os.path.join(HERE, "golden", "make_golden_entry_points.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def pinned(gen):
    with open(gen.PATH) as f:
        want = json.load(f)
    dropped = want.pop("_dropped")
    assert all(path.split(".")[-1] in gen.ALLOWED_TO_DIFFER for path in dropped), dropped
    return want, set(dropped)


@pytest.fixture(scope="module")
def computed(gen):
    return gen.collect()


def test_the_file_holds_every_field_but_the_named_ones(gen, pinned, computed):
    want, dropped = pinned
    assert set(gen.leaves(computed)) == set(gen.leaves(want)) | dropped
    assert computed["search"]["gated_fp16"]["info_GATED_I8"] == 0 and computed["search"]["gated_i8"]["info_GATED_I8"] == 1


@pytest.mark.parametrize("group", ["search", "densify", "pq", "pq_handle", "merges"])
def test_entry_points_equal_the_parent(gen, pinned, computed, group):
    want, dropped = pinned
    got = gen.leaves(gen.drop(computed, dropped)[group])
    assert got == gen.leaves(want[group]), {f: (got.get(f), v) for f, v in gen.leaves(want[group]).items() if got.get(f) != v}


def test_host_and_device_memory_give_the_same(pinned):
    """one call, its arrays in host or in device memory: the same bytes come back"""
    want, _ = pinned
    for image in want["search"].values():
        for field, v in image.items():
            if "_host_" in field and field.endswith("sha256"):
                assert image[field.replace("_host_", "_device_")] == v, field
    for name, case in want["densify"].items():
        if name.endswith("_host"):
            assert want["densify"][name[:-5] + "_device"] == case, name
    for group in ("pq", "pq_handle"):
        for name, case in want[group].items():
            if name.endswith("_host"):
                other = want[group][name[:-5] + "_device"]
                assert {f: v for f, v in case.items() if f != "out_error"} == {f: v for f, v in other.items() if f != "out_error"}, name
