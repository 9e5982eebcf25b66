"""GPU tier: the status accounting of concurrent asynchronous renders of ONE scene (include/rl_render.h rl_render_status, csrc/rl_scene.h).

rl_render_status must report `flagged` = the panic sites reached by every pending render (none is lost or counted twice) and `rays` = the
ray count of the render enqueued last, while every frame stays the bits of the same render issued alone.  The scenes below flag on one
camera and not on another, so a render whose status copy reads a neighbour's counters shows up as a wrong total.  The windows in which
that could happen are microseconds wide; rl_debug_set_status_gap widens them to milliseconds (a wait kernel before each status copy, a
host sleep before a multi-GPU frame's status post) so that a lost count fails every run, not by luck.

No flagging scene reaches the fast general kernel (variant 1031): its structure is only built where build_fast_general proves that
no sphere normal can miss unit length (rl_fast_bvh.cpp r_safe), and the cooperative kernel only runs scenes of the fast sphere tree,
which excludes such spheres too.  Those kernels are covered here with frames and rays (and flagged == 0)."""
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTERS = ("rays", "node_tests", "sphere_tests", "planar_tests", "instance_enters", "rng_words", "flagged")
GAP_US = 3000


@pytest.fixture(autouse=True)
def _gap(rl):
    rl.api.set_status_gap(GAP_US, 0)
    try:
        yield
    finally:
        rl.api.set_status_gap(0, 0)
        rl.api.set_indep_cap(0)


def _far_sphere(rl, width=33, spp=16):
    """test_gpu_timed_kernels.py::test_async_render_surfaces_reference_panic_sites: a unit sphere at x = 1e12 trips vec3.rs:219 on
    thousands of hits; a second camera at the same spot that looks the other way sees only sky."""
    api = rl.api
    tex = np.zeros(1, dtype=api.TEXTURE)
    tex[0]["kind"], tex[0]["color"] = api.TEX_SOLID, (0.5, 0.4, 0.3)
    mats = np.zeros(1, dtype=api.MATERIAL)
    mats[0]["kind"], mats[0]["texture"] = api.MAT_LAMBERTIAN, 0
    sph = np.zeros(1, dtype=api.SPHERE)
    sph[0]["center0"], sph[0]["radius"] = (1e12, 0.0, -1.0), 1.0
    world = rl.World.from_spheres(sph, mats, tex, False)
    common = dict(aspect_ratio=1.0, image_width=width, samples_per_pixel=spp, max_depth=5, lookfrom=(1e12, 0, 3), vfov=40.0)
    flag = rl.Camera(rl.CameraParams(**common, lookat=(1e12, 0, -1)))
    quiet = rl.Camera(rl.CameraParams(**common, lookat=(1e12, 0, 7), seed=3))
    return world, flag, quiet


def _buf(cam, nan=True):
    import torch
    return torch.full((cam.c.image_height, cam.c.image_width, 3), float("nan") if nan else 0.0, dtype=torch.float64, device="cuda:0")


def _alone(rl, world, cam, issue):
    """The render issued alone, asynchronously: (frame, rays, flagged)."""
    import torch
    b = _buf(cam, nan=False)
    issue(cam, b, torch.cuda.current_stream().cuda_stream)
    st = rl.api.render_status(world, allow_degenerate=True)
    return b.cpu().numpy(), st["rays"], st["flagged"]


def _rtiow_device(world):
    return lambda cam, b, s: cam.render_device(world, b.data_ptr(), stream=s)


def _rtiow_indep(world):
    return lambda cam, b, s: cam.render_independent_device(world, b.data_ptr(), stream=s, allow_degenerate=True)


def _alternate(rl, world, cams, refs, issue, n, n_streams=3):
    """n renders, cams[i % len(cams)] on stream i % n_streams, no host sync between them; then one rl_render_status.  Three streams:
    which hardware queue a stream lands on is the runtime's choice, and two of them may share one."""
    import torch
    streams = [torch.cuda.Stream() for _ in range(n_streams)]
    torch.cuda.synchronize()
    bufs = []
    for i in range(n):
        c = i % len(cams)
        b = _buf(cams[c])
        torch.cuda.synchronize()  # the NaN fill, before any render is enqueued
        bufs.append((c, b))
    for i, (c, b) in enumerate(bufs):
        issue(cams[c], b, streams[i % n_streams].cuda_stream)
    st = rl.api.render_status(world, allow_degenerate=True)
    torch.cuda.synchronize()
    for i, (c, b) in enumerate(bufs):
        assert np.array_equal(b.cpu().numpy(), refs[c][0], equal_nan=True), (i, c)
    want = sum(refs[c][2] for c, _ in bufs)
    assert st["flagged"] == want, ("flagged", st["flagged"], want)
    assert st["rc"] == (rl.api.RL_E_DEGENERATE if want else rl.api.RL_OK)
    assert st["rays"] == refs[bufs[-1][0]][1], ("rays", st["rays"], refs[bufs[-1][0]][1])


@pytest.mark.parametrize("entry", ["device", "device_large", "independent"])
def test_alternating_flagged_and_quiet_renders_on_several_streams(rl, entry):
    """(a) flagging and quiet renders alternate over three streams: flagged = k * F exactly, rays of the last render, every frame bit-equal."""
    width = 256 if entry == "device_large" else 33  # 256 x 256: above the small-frame threshold (wave-scheduled kernel with its tiles)
    world, flag, quiet = _far_sphere(rl, width=width, spp=2 if entry == "device_large" else 16)
    issue = _rtiow_indep(world) if entry == "independent" else _rtiow_device(world)
    gs, qs = {}, {}
    flag._render(0, world, stats=gs, allow_degenerate=True) if entry != "independent" else flag.render_independent_rows(world, 0, 1, stats=gs, allow_degenerate=True)
    quiet._render(0, world, stats=qs) if entry != "independent" else quiet.render_independent_rows(world, 0, 1, stats=qs)
    assert gs["flagged"] > 1000 and qs["flagged"] == 0
    refs = [_alone(rl, world, flag, issue), _alone(rl, world, quiet, issue)]
    assert refs[0][2] == gs["flagged"] and refs[0][1] == gs["rays"] and refs[1][2] == 0 and refs[1][1] == qs["rays"]
    _alternate(rl, world, [flag, quiet], refs, issue, 6)
    _alternate(rl, world, [quiet, flag], [refs[1], refs[0]], issue, 5)  # a flagging render last


def test_small_frames_and_fast_general_renders_account_rays_on_several_streams(rl):
    """(a) the kernels no flagging scene reaches: the cooperative kernel (small frames of a sphere scene) and the fast general kernel
    (quads, media, textures): frames and rays of renders alternating over three streams, flagged = 0."""
    import dataclasses
    for world, width in ((rl.World.bouncing_spheres(1), 40), (rl.World.example_scene("cornell_box"), 48), (rl.World.example_scene("cornell_smoke"), 48),
                         (rl.World.perlin_spheres(), 48)):
        p = world.params
        p.max_depth = min(p.max_depth, 20)
        a = rl.Camera(dataclasses.replace(p, image_width=width, samples_per_pixel=8))
        b = rl.Camera(dataclasses.replace(p, image_width=width, samples_per_pixel=3, seed=p.seed + 7))
        for issue in (_rtiow_device(world), _rtiow_indep(world)):
            refs = [_alone(rl, world, a, issue), _alone(rl, world, b, issue)]
            assert refs[0][2] == 0 and refs[1][2] == 0 and refs[0][1] != refs[1][1]
            _alternate(rl, world, [a, b], refs, issue, 5)


def test_status_ring_wraps_with_flagged_renders_on_three_streams(rl):
    """(b) 14 renders in flight against a status ring of N_STATUS = 8 slots, over three streams: the flagged total stays exact."""
    world, flag, quiet = _far_sphere(rl)
    issue = _rtiow_device(world)
    refs = [_alone(rl, world, flag, issue), _alone(rl, world, quiet, issue)]
    assert refs[0][2] > 1000
    _alternate(rl, world, [flag, quiet, flag, quiet, quiet], [refs[0], refs[1], refs[0], refs[1], refs[1]], issue, 14)


def test_threads_streams_and_counting_renders_of_one_flagging_scene(rl):
    """(c) two threads issue asynchronous flagging / quiet renders on their own streams while a third interleaves counting renders:
    every counting render's seven counters are its alone render's, the asynchronous totals are exact, every frame bit-equal."""
    import torch
    world, flag, quiet = _far_sphere(rl)
    issue = _rtiow_device(world)
    refs = [_alone(rl, world, flag, issue), _alone(rl, world, quiet, issue)]
    counted = []
    for cam in (flag, quiet):
        st = {}
        cam._render(0, world, stats=st, allow_degenerate=True)
        counted.append(st)
    assert counted[0]["flagged"] == refs[0][2] > 1000 and counted[1]["flagged"] == 0
    streams = [torch.cuda.Stream() for _ in range(2)]
    bufs = [[_buf(flag if (t + k) % 2 == 0 else quiet) for k in range(4)] for t in range(2)]
    torch.cuda.synchronize()
    errors, seen = [], []

    def asynchronous(t):
        try:
            for k in range(4):
                issue(flag if (t + k) % 2 == 0 else quiet, bufs[t][k], streams[t].cuda_stream)
        except Exception as e:  # noqa: BLE001
            errors.append((t, repr(e)))

    def counting():
        try:
            for k in range(4):
                st = {}
                (flag if k % 2 == 0 else quiet)._render(0, world, stats=st, allow_degenerate=True)
                seen.append((k % 2, st))
        except Exception as e:  # noqa: BLE001
            errors.append(("counting", repr(e)))
    ts = [threading.Thread(target=asynchronous, args=(t,)) for t in range(2)] + [threading.Thread(target=counting)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors
    st = rl.api.render_status(world, allow_degenerate=True)
    torch.cuda.synchronize()
    for c, s in seen:
        for k in COUNTERS:
            assert s[k] == counted[c][k], (c, k, s[k], counted[c][k])
    for t in range(2):
        for k in range(4):
            c = (t + k) % 2
            assert np.array_equal(bufs[t][k].cpu().numpy(), refs[c][0], equal_nan=True), (t, k)
    assert st["flagged"] == 4 * refs[0][2], (st["flagged"], 4 * refs[0][2])
    assert st["rays"] in (refs[0][1], refs[1][1])


@pytest.mark.parametrize("name", ["bouncing_spheres", "cornell_box"])
def test_independent_and_chained_renders_of_one_scene_on_two_streams(rl, name):
    """(d) the sample-parallel entry (its pass buffer, and on the fast general kernel the two-slot parameter ring: 4 passes here) and
    chained renders of one scene, alternating over three streams: every frame the bits of the same render issued alone."""
    import dataclasses
    world = rl.World.bouncing_spheres(1) if name == "bouncing_spheres" else rl.World.example_scene(name)
    p = world.params
    p.max_depth = min(p.max_depth, 20)
    width = 64 if name == "bouncing_spheres" else 48
    ind = rl.Camera(dataclasses.replace(p, image_width=width, samples_per_pixel=10))
    chn = rl.Camera(dataclasses.replace(p, image_width=width, samples_per_pixel=6, seed=p.seed + 1))
    rl.api.set_indep_cap(ind.c.image_height * ind.c.image_width * 3 * 8 * 3)  # 3 samples per pass: 4 passes
    ii, ic = _rtiow_indep(world), _rtiow_device(world)
    refs = [_alone(rl, world, ind, ii), _alone(rl, world, chn, ic)]
    both = lambda cam, b, s: (ii if cam is ind else ic)(cam, b, s)
    _alternate(rl, world, [ind, chn], refs, both, 6)
    _alternate(rl, world, [chn, ind], [refs[1], refs[0]], both, 5)


def _rtc_stack(rl):
    """30 unit spheres in a row along +z: a ray down the row meets 60 intersections, more than the full kernel keeps (RL_RTC_K = 48),
    and each overflow is flagged; a camera at the same spot that looks sideways meets none (Ray::intersect keeps the roots behind the origin too)."""
    api = rl.api
    n = 30
    mats = np.zeros(1, dtype=api.RTC_MATERIAL)
    mats["color"], mats["ambient"], mats["diffuse"], mats["specular"], mats["shininess"], mats["refractive_index"] = (0.8, 0.5, 0.3), 0.1, 0.9, 0.9, 200.0, 1.0
    shapes = np.zeros(n, dtype=api.RTC_SHAPE)
    shapes["kind"], shapes["material"] = api.O_SPHERE, 0
    tr = np.array([api.rtc_transformed(np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 3.0 * i], [0, 0, 0, 1]], dtype=float), api.O_SPHERE, i)
                   for i in range(n)], dtype=api.RTC_TRANSFORMED)
    objs = np.zeros(n, dtype=api.HREF)
    objs["kind"], objs["index"] = api.O_TRANSFORMED, np.arange(n)
    lights = np.zeros(1, dtype=api.RTC_LIGHT)
    lights["position"], lights["intensity"] = (-5, 8, -8), (1, 1, 1)
    flag = api.rtc_camera(24, 20, 0.3, (0, 0, -10), (0, 0, 0), (0, 1, 0))
    quiet = api.rtc_camera(24, 20, 0.3, (0, 0, -10), (10, 0, -10), (0, 1, 0))  # along +x: the row is neither ahead nor behind
    world = rl.RtcWorld.from_arrays(np.zeros(0, dtype=api.RTC_TRIANGLE), mats, objs, lights, transformeds=tr, shapes=shapes, camera=flag)
    return world, flag, quiet


def test_rtc_alternating_flagged_and_quiet_renders_on_several_streams(rl):
    """(e) the same as (a) through rl_rtc_render_device, on a world that overflows the full kernel's intersection list."""
    world, flag, quiet = _rtc_stack(rl)
    gs, qs = {}, {}
    world.render(1, camera=flag, stats=gs, allow_degenerate=True)
    world.render(1, camera=quiet, stats=qs)
    assert gs["flagged"] > 0 and qs["flagged"] == 0

    class Cam:  # the helpers read c.image_height / image_width for the buffers
        def __init__(self, rc):
            self.rc = rc
            self.c = type("C", (), {"image_height": rc.vsize, "image_width": rc.hsize})
    cams = [Cam(flag), Cam(quiet)]
    issue = lambda cam, b, s: world.render_device(b.data_ptr(), 1, camera=cam.rc, stream=s)
    refs = [_alone(rl, world, c, issue) for c in cams]
    assert refs[0][2] == gs["flagged"] and refs[0][1] == gs["rays"] and refs[1][2] == 0
    _alternate(rl, world, cams, refs, issue, 6)
    _alternate(rl, world, cams[::-1], refs[::-1], issue, 5)


BODY = r'''
import importlib, sys, threading
import numpy as np
import torch  # BEFORE the product library: torch bundles its own HIP runtime, and a process must not end up with two of them
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
rl = importlib.import_module("rendering-learning_amd")
api = rl.api
from test_gpu_status_accounting import _far_sphere

api.init(0)
world, flag, quiet = _far_sphere(rl)
refs = []
for cam in (flag, quiet):
    gs = {}
    refs.append((cam.render(world, stats=gs, allow_degenerate=True).data, gs["flagged"], gs["rays"]))
assert refs[0][1] > 1000 and refs[1][1] == 0
del world
for G in (2, 3):
    assert api.init_multi(emulate=G) == G
    api.set_status_gap(0, 5000)
    world, flag, quiet = _far_sphere(rl)
    n = (3, 5)  # unequal: a status post that reads the next frame's counters must not be evened out by a later one
    bufs = [[torch.full((33, 33, 3), float("nan"), dtype=torch.float64, device="cuda:0") for _ in range(n[t])] for t in range(2)]
    torch.cuda.synchronize()
    errors = []
    def work(t):
        try:
            for k in range(n[t]):
                (flag if t == 0 else quiet).render_multi_device(world, bufs[t][k].data_ptr())
        except Exception as e:
            errors.append((t, repr(e)))
    ts = [threading.Thread(target=work, args=(t,)) for t in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors
    st = api.render_status(world, allow_degenerate=True)
    torch.cuda.synchronize()
    for t in range(2):
        for k in range(n[t]):
            assert np.array_equal(bufs[t][k].cpu().numpy(), refs[t][0], equal_nan=True), (G, t, k)
    assert st["flagged"] == n[0] * refs[0][1], ("G", G, "flagged", st["flagged"], "want", n[0] * refs[0][1])
    assert st["rays"] in (refs[0][2], refs[1][2]), (G, st["rays"])
    # progress of a multi-GPU scene: refused, never a silent zero or a stale total
    try:
        api.render_progress(world)
        raise AssertionError("render_progress on a multi-GPU scene did not raise")
    except api.RLError as e:
        assert e.code == api.RL_E_UNSUPPORTED, (G, e.code)
    api.set_status_gap(0, 0)
    del world
print("STATUS_MULTI_OK")
'''


def test_multi_device_renders_from_two_threads_account_every_flag():
    """(f) emulated multi-GPU contexts (G = 2, 3) in a fresh child process: two threads issue rl_rtiow_render_multi_device with the
    flagging and the quiet camera; rl_render_status gives the exact flagged sum and every frame is the single render's."""
    r = subprocess.run([sys.executable, "-c", BODY % {"root": ROOT, "tests": os.path.join(ROOT, "tests")}], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0 and "STATUS_MULTI_OK" in r.stdout, r.stdout[-4000:]
