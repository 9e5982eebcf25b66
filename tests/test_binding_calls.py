"""CPU tier: what every wrapper of api.py, ao.py, direct.py, nee.py, occlusion.py and entry_table.py hands to the render library (and
the cpp_mirror_probe* to the host library's probes), compared with tests/golden/binding_calls.json — the record of the same driver
(tests/binding_model.py drive()) against the commit the file names, written by tools/record_binding_calls.py.  A recorder stands in for
render_lib(), a second one for the rlh_*_probe symbols of host_lib(); the rest of the host library is the real one and needs no device.
Per wrapper the record shows its signature, and per call every scalar and for every pointer whether it was NULL: opt_stats above all,
which chooses between the counting and the counter-free kernels."""
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
                   "RtcWorld.color_at_rays", "ao.render_ao", "direct.render_direct", "nee.render_nee", "nee.render_nee_mis"}
# what binding_model.names_render_lib yields at 366aa9a: the driver must reach at least these of api.py, whatever their text names now
API_WRAPPERS = (
    "Camera.render_rgb8", "Camera.render_denoised_rgb8", "Camera.render_independent_rows", "Camera.render_independent_device", "Camera.get_rays",
    "Camera.get_rays_device", "Camera.render_multi", "Camera.render_multi_device", "Camera.render_device", "Camera.render_pixels",
    "Camera.render_pixels_device", "Camera.render_moments", "Camera.render_moments_device", "Camera.render_pixels_moments",
    "Camera.render_pixels_moments_device", "Camera.render_adaptive", "Camera.render_adaptive_device", "Camera.render_features",
    "Camera.render_features_device", "Camera.render_pixels_features", "Camera.render_pixels_features_device", "World.device", "World.hit_rays",
    "World.hit_rays_device", "World.hit_rays_seeded", "World.hit_rays_seeded_device", "World.ray_color_rays", "World.ray_color_rays_device",
    "World.scatter_rays", "World.scatter_rays_device", "World.texture_values", "World.texture_values_device", "RtcWorld.device", "RtcWorld.render",
    "RtcWorld.render_rgb8", "RtcWorld.render_multi", "RtcWorld.render_device", "RtcWorld.render_pixels", "RtcWorld.render_pixels_device",
    "RtcWorld.intersect_rays", "RtcWorld.intersect_rays_device", "RtcWorld.color_at_rays", "RtcWorld.color_at_rays_device", "RtcWorld.prepare_rays",
    "RtcWorld.prepare_rays_device", "RtcWorld.shade_hits", "RtcWorld.shade_hits_device", "RtcWorld.shadow_attenuation",
    "RtcWorld.shadow_attenuation_device", "RtcWorld.lighting", "RtcWorld.lighting_device", "init", "init_multi", "render_status", "render_progress",
    "set_fast_traversal", "set_coop", "set_lpt", "set_coop_pixels_max", "set_steal", "set_indep_cap", "set_indep_k", "set_fastg_one_wave",
    "set_pixel_entry", "set_pixel_entry_sphere", "pixel_entry_table", "fast_tree", "set_status_gap", "live_buffers", "set_query_pass_cap", "last_query",
    "set_denoise_route", "last_denoise_route", "set_denoise_blocks", "last_denoise_launch", "last_rtc_launch", "rtiow_launch_total", "rtiow_launches",
    "steal_record", "rtc_program", "material_query_max_lanes", "features_max_lanes", "set_rtiow_variant", "denoise_atrous",
    "denoise_atrous_pass_device", "denoise_prepare_device", "denoise_finish_device", "denoise_render_work_bytes", "denoise_render_device",
    "denoise_render_gpu")


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
        head, *lines = json.load(f)
    assert head["recorded_from"]
    signatures = {e["signature_of"]: e["signature"] for e in lines if "signature_of" in e}
    return [dict(e, signature=signatures[e["wrapper"].split("[")[0]]) for e in lines if "wrapper" in e]


def test_every_wrapper_hands_c_what_it_did(recorded, fixture):
    assert [e["wrapper"] for e in recorded] == [e["wrapper"] for e in fixture]
    for got, want in zip(recorded, fixture):
        assert got == want, got["wrapper"]


def test_the_driver_reaches_every_wrapper(rl, recorded):
    driven = {e["wrapper"].split("[")[0] for e in recorded}
    wanted = bm.covered_wrappers(rl.api, API_WRAPPERS)
    assert len(wanted) >= len(API_WRAPPERS) + 27  # the 27 of the family modules at 366aa9a
    missing = [w for w in wanted if w not in driven]
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
