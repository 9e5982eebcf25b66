"""CPU tier: what every wrapper of api.py hands to the render library, compared with tests/golden/binding_calls.json — the record of
the same driver (tests/binding_model.py drive()) against the commit the file names, written by tools/record_binding_calls.py.  A
recorder stands in for render_lib(); the host library is the real one and needs no device.  Per call the record shows every scalar, and
for every pointer whether it was NULL: opt_stats above all, which chooses between the counting and the counter-free kernels."""
import json
import os

import pytest

import binding_model as bm

FIXTURE = os.path.join(bm.ROOT, "tests", "golden", "binding_calls.json")
COUNTERS = ["flagged", "instance_enters", "kernel_ms", "node_tests", "planar_tests", "rays", "rng_words", "sphere_tests"]
# the wrappers that hand the library an rl_stats whether or not the caller asked for counters: always the counting, reference-order kernels
ALWAYS_COUNTING = {"Camera.render", "Camera.render_rows", "Camera.render_independent",
                   "Camera.render_independent_rows", "Camera.render_multi", "Camera.render_moments", "Camera.render_adaptive",
                   "Camera.render_features", "RtcWorld.render", "RtcWorld.render_multi", "RtcWorld.render_pixels", "RtcWorld.intersect_rays",
                   "RtcWorld.color_at_rays"}


@pytest.fixture(scope="module")
def recorded(rl):
    mp = pytest.MonkeyPatch()
    try:
        return json.loads(json.dumps(bm.drive(rl.api, mp.setattr)))  # through JSON: tuples and lists compare as the file holds them
    finally:
        mp.undo()


@pytest.fixture(scope="module")
def fixture():
    with open(FIXTURE) as f:
        head, *entries = json.load(f)
    assert head["recorded_from"]
    return entries


def test_every_wrapper_hands_c_what_it_did(recorded, fixture):
    assert [e["wrapper"] for e in recorded] == [e["wrapper"] for e in fixture]
    for got, want in zip(recorded, fixture):
        assert got == want, got["wrapper"]


def test_the_driver_reaches_every_wrapper(rl, recorded):
    driven = {e["wrapper"].split("[")[0] for e in recorded}
    missing = [w for w in bm.covered_wrappers(rl.api) if w not in driven]
    assert missing == []


def _stats_arg(call):
    return call[1][-1]


def test_opt_stats_is_null_exactly_where_it_was(recorded):
    """The routing decision, stated outright beside the fixture: without stats= only the always-counting wrappers pass an rl_stats; with a
    dict every wrapper does."""
    seen = set()
    for e in recorded:
        if "stats" not in e:
            continue
        name = e["wrapper"].split("[")[0]
        plain = [c for c in e["plain"]["calls"] if isinstance(_stats_arg(c), dict) or _stats_arg(c) == "null"][-1]
        counted = [c for c in e["stats"]["calls"] if c[0] == plain[0]][-1]
        assert (_stats_arg(plain) != "null") == (name in ALWAYS_COUNTING), e["wrapper"]
        assert isinstance(_stats_arg(counted), dict), e["wrapper"]
        seen.add(name)
    assert ALWAYS_COUNTING <= seen


def test_every_stats_dict_holds_the_counters_and_rc(recorded):
    for e in recorded:
        if "stats" in e:
            assert e["stats"]["keys"] == sorted(COUNTERS + ["rc"]), e["wrapper"]
            assert e["degenerate"]["outcome"] == "RLError(-5)" and e["degenerate"]["keys"] == [], e["wrapper"]  # refused before the dict is touched
        if "allowed" in e:
            assert e["allowed"]["outcome"] == "ok", e["wrapper"]
            if "keys" in e["allowed"]:
                assert e["allowed"]["rc"] == bm.RL_E_DEGENERATE, e["wrapper"]
