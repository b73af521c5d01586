"""The forward pass, bit for bit, on every route it can take: each case of tests/golden/make_forward_routes.py is
recomputed and compared with the record in tests/golden/forward_routes.json (SHA-256 of the logits and of the written KV
range, launch counts per profile class, prefill-attention launch counters).  The record was made by that script at the
commit before the forward pass's host code was restructured around a per-pass route; host-side changes that keep every
launch as it is keep every digest."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
with open(os.path.join(GOLDEN, "forward_routes.json")) as f:
    RECORD = json.load(f)


@pytest.fixture(scope="module")
def routes():
    spec = importlib.util.spec_from_file_location("make_forward_routes", os.path.join(GOLDEN, "make_forward_routes.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert sorted(mod.CASES) == sorted(RECORD), "the record and the script's cases differ: regenerate the record"
    return mod


@pytest.mark.parametrize("name", sorted(RECORD))
def test_forward_route_is_bit_identical_to_the_record(routes, name):
    got = routes.run_case(name)
    print(name, got)
    assert got["counts"] == RECORD[name]["counts"]
    assert got["prefill"] == RECORD[name]["prefill"]
    assert got["logits"] == RECORD[name]["logits"]
    assert got["kv"] == RECORD[name]["kv"]
