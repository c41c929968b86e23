"""What the index build produces, pinned to the commit before dhr_index_create was rewritten around one layout plan: tests/golden/index_build.json
was recorded there by tests/golden/make_golden_index_build.py, and this module recomputes it with the recorder's own collect().  Every branch of
the build has a case (fp16 / int8 gated image, abs_mode, zero-slice padding from host memory, device memory and an index file, 16-bit indices,
one bucket, dense-only fp16 / int8 with and without the residual image, the dense-only trial kept and rejected); everything compared is an
integer, the hex form of a float or a digest of an array that the build determines, so equality is exact and every field of the file counts."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FIELDS = 19      # of a gated case; a dense-only one has no gated batch (two digests fewer)


@pytest.fixture(scope="module")
def gen():
    spec = importlib.util.spec_from_file_location("make_golden_index_build", os.path.join(HERE, "golden", "make_golden_index_build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def pinned(gen):
    with open(gen.PATH) as f:
        want = json.load(f)
    assert sorted(want) == sorted(gen.CASES)
    for name, case in want.items():          # the file holds every field of every case: none was dropped as irreproducible
        assert len(case) == (FIELDS if "gated_bound_sha256" in case else FIELDS - 2), name
    gen.check_coverage(want)
    return want


@pytest.fixture(scope="module")
def built(gen):
    got = gen.collect()
    gen.check_coverage(got)
    return got


@pytest.mark.parametrize("case", ["g64_gated_fp16", "g64_gated_i8", "g64_abs_gated_i8", "pad100_host", "pad100_device", "pad100_file", "i16_value_mod_2", "one_bucket",
                                  "dense128_fp16", "dense128_i8_residual", "dense1100_i8_no_residual", "trial_keeps_i8", "trial_falls_back"])
def test_index_build_equals_the_parent(pinned, built, case):
    assert built[case] == pinned[case], {f: (built[case].get(f), v) for f, v in pinned[case].items() if built[case].get(f) != v}
