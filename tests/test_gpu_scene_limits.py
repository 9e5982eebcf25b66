"""GPU tier: the scene compilers' limits at their edge, on the device.  tests/test_scene_desc_refusals.py (CPU tier) establishes what
a description ends as; here the deepest worlds the fixed-size device stacks accept are traced and compared, and refusals are taken
through the C ABI.  Nothing reaches the device from this module that the CPU tier has not shown to be refused or to compile to a program
that passes its checker: the accepted worlds are B.instances.8 and B.checker.32 in shape, the refused ones rows of its table made with
the same edit of the same example scene."""
import ctypes as C

import numpy as np
import pytest

import test_rtiow_geometry_model as M
from test_scene_desc_refusals import A, B, CASES

pytestmark = pytest.mark.gpu
INF = float("inf")


# ----------------------------------------------------------------------------- instances nested 8 deep
def _nested_instances(rl, depth):
    """Translate and rotate-Y Transform alternating around a list of one sphere and one quad.  The translations are along y and the
    sphere sits on the y axis, so whatever the turns it ends at (0, 0.5 * translations, 0); the quad is a horizontal square below it."""
    def fn(b):
        red, grey = b.lambertian(b.solid((0.8, 0.2, 0.2))), b.lambertian(b.solid((0.5, 0.5, 0.5)))
        node = b.list([b.sphere((0.0, 0.0, 0.0), 1.0, red), b.quad((-3.0, -1.5, -3.0), (6.0, 0.0, 0.0), (0.0, 0.0, 6.0), grey)])
        for k in range(depth):
            node = b.translate(node, (0.0, 0.5, 0.0)) if k % 2 == 0 else b.rotate_y(node, 17.0 * (k + 1))
        return node
    return rl.World.build(fn)


def _rays_at(centre, n, seed):
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(n, 3))
    o = centre + 8.0 * v / np.linalg.norm(v, axis=1, keepdims=True)
    target = centre + np.array([0.0, -0.5, 0.0]) + rng.uniform(-1.5, 1.5, size=(n, 3)) * np.array([1.0, 0.5, 1.0])
    return o, target - o


def test_instances_nested_exactly_8_equal_the_oracle_and_9_are_refused(rl, oracle):
    rl.init(0)
    assert CASES["B.instances.8"][0] == 0 and CASES["B.instances.9"][1] == "instances nested deeper than 8"
    world = _nested_instances(rl, 8)
    assert world.counts()["translates"] == 4 and world.counts()["transforms"] == 4
    n = 64
    o, d = _rays_at(np.array([0.0, 2.0, 0.0]), n, 808)
    st = {}
    counted = world.hit_rays(o, d, stats=st)  # the reference-order fold
    assert rl.api.last_query()["kernel"] == "reference", rl.api.last_query()
    print("counters", {k: st[k] for k in ("rays", "node_tests", "sphere_tests", "planar_tests", "instance_enters", "rng_words", "flagged")})
    free = world.hit_rays(o, d)  # the fast walk: its instance chain is 8 long here
    assert rl.api.last_query()["kernel"] == "fast", rl.api.last_query()
    assert counted.tobytes() == free.tobytes()
    # a list of two primitives under eight instances and no box: the reference enters every instance and tests both primitives for every ray
    assert st["rays"] == n and st["instance_enters"] == 8 * n and st["sphere_tests"] == n and st["planar_tests"] == n and st["node_tests"] == 0, st
    assert st["rng_words"] == 0 and st["flagged"] == 0, st
    materials = set()
    for i in range(n):
        ref = oracle.rtiow_hit(world.desc, o[i], d[i], 0.0, 1e-10, INF)
        h = counted[i]
        if ref is None:
            assert h["hit"] == 0 and h["t"] == INF, i
            continue
        materials.add(int(h["material"]))
        assert h["hit"] == 1 and h["material"] == ref["mat"] and bool(h["front_face"]) == ref["front"], (i, h, ref)
        assert h["t"] == ref["t"] and np.array_equal(h["p"], ref["p"]) and np.array_equal(h["normal"], ref["normal"]), (i, h, ref)
    assert int((counted["hit"] == 1).sum()) >= 40 and len(materials) == 2, (int((counted["hit"] == 1).sum()), materials)  # sphere and quad
    with pytest.raises(rl.api.RLError) as e:
        _nested_instances(rl, 9).hit_rays(o, d)
    assert e.value.code == rl.api.RL_E_INVALID and "instances nested deeper than 8" in str(e.value), str(e.value)


# ----------------------------------------------------------------------------- checkers nested 32 deep
LEAVES = [(0.9, 0.1, 0.1), (0.1, 0.9, 0.1), (0.1, 0.1, 0.9), (0.9, 0.9, 0.1)]


def _checker_ladder(depth):
    """Two checkers per level, A_k = Checker(even: A_k+1, odd: B_k+1) and B_k = Checker(even: B_k+1, odd: A_k+1) with scales of their own;
    four colours below the last level.  Every walk from A_1 is `depth` steps long and its colour depends on every one of its choices."""
    a, b = ((0.37 + 0.05 * depth,), LEAVES[0], LEAVES[1]), ((0.53 + 0.03 * depth,), LEAVES[2], LEAVES[3])
    for k in range(depth - 1, 0, -1):
        a, b = ((0.37 + 0.05 * k,), a, b), ((0.53 + 0.03 * k,), b, a)
    return a


def _ladder_world(rl, tree):
    def fn(b):
        ids = {}

        def tex(t):  # shared nodes once: the ladder is 2 * depth checkers, not 2^depth
            if id(t) not in ids:
                ids[id(t)] = b.solid(t) if isinstance(t[0], float) else b.checker(t[0][0], tex(t[1]), tex(t[2]))
            return ids[id(t)]
        return b.list([b.sphere((0.0, 0.0, 0.0), 1.0, b.lambertian(tex(tree)))])
    return rl.World.build(fn)


def _choices(tree, p):
    """the even (0) / odd (1) choice of every level of the walk M.checker_leaf takes"""
    out = []
    while not isinstance(tree[0], float):
        s = sum(int(np.floor(c * (1.0 / tree[0][0]))) for c in p)
        out.append(abs(s) % 2)
        tree = tree[1 + out[-1]]
    return out


def test_a_checker_nested_exactly_32_deep_equals_the_restatement_and_33_is_refused(rl):
    rl.init(0)
    assert CASES["B.checker.32"][0] == 0 and CASES["B.checker.33"][1] == "checker textures nest cyclically or deeper than 32"
    tree = _checker_ladder(32)
    world = _ladder_world(rl, tree)
    assert world.counts()["textures"] == 63 + 4  # B_1 is never reached
    root = int(world.materials()["texture"][0])
    pts = np.random.default_rng(3232).uniform(-8.0, 8.0, size=(65, 3))
    choices = np.array([_choices(tree, p) for p in pts])
    assert choices.shape == (65, 32) and (choices.min(axis=0) == 0).all() and (choices.max(axis=0) == 1).all()  # both children, at every level
    want = np.array([M.checker_leaf(tree, p) for p in pts])
    assert len({tuple(w) for w in want.tolist()}) == 4
    got = world.texture_values(np.full(65, root, dtype=np.uint32), np.zeros((65, 2)), pts)
    assert np.array_equal(got, want), (got, want)
    with pytest.raises(rl.api.RLError) as e:
        deeper = _ladder_world(rl, _checker_ladder(33))
        deeper.texture_values(np.zeros(1, dtype=np.uint32), np.zeros((1, 2)), np.zeros((1, 3)))
    assert e.value.code == rl.api.RL_E_INVALID and "checker textures nest cyclically or deeper than 32" in str(e.value), str(e.value)


# ----------------------------------------------------------------------------- refusals through the C ABI
def _golden_bytes(rl):
    world = rl.World.golden_test_scene()
    p = world.params
    p.image_width, p.samples_per_pixel, p.max_depth = 48, 2, 8
    return rl.Camera(p).render(world).data.tobytes()


def _rtiow_rows(rl):
    """(row of the CPU tier's table, description, what it keeps alive): the edits of tests/host/scene_desc_check.cpp on checkered_spheres"""
    api = rl.api
    world = rl.World.example_scene("checkered_spheres")
    base = api.RtiowSceneDesc.from_address(world.desc)

    def edit(name, field=None, dtype=None, change=None, desc_change=None):
        d = api.RtiowSceneDesc.from_buffer_copy(base)
        keep = [world]
        if field is not None:
            table = world._table(field, dtype)
            change(table)
            keep.append(table)
            setattr(d, field, table.ctypes.data)
        if desc_change is not None:
            desc_change(d)
        return name, d, keep

    def checker_cycle(t):
        k = int(np.flatnonzero(t["kind"] == api.TEX_CHECKER)[0])
        t["even"][k] = k

    def material_texture(m):
        m["texture"][int(np.flatnonzero(m["kind"] == api.MAT_LAMBERTIAN)[0])] = len(world.textures())

    def root_kind(d):
        d.root[0] = 0

    return [edit("A.rtiow.null.spheres", desc_change=lambda d: setattr(d, "spheres", None)),
            edit("A.rtiow.too_many_spheres", desc_change=lambda d: setattr(d, "n_spheres", 0x3FFFFFFF + 1)),
            edit("A.rtiow.hittable_kind.none", desc_change=root_kind),
            edit("A.rtiow.sphere_material", "spheres", api.SPHERE, lambda s: s["material"].__setitem__(0, len(world.materials()))),
            edit("A.rtiow.material_texture", "materials", api.MATERIAL, material_texture),
            edit("A.rtiow.texture_kind", "textures", api.TEXTURE, lambda t: t["kind"].__setitem__(0, api.TEX_NOISE + 1)),
            edit("A.rtiow.checker_cycle", "textures", api.TEXTURE, checker_cycle)]


def _rtc_rows(rl):
    """... on the mirror and CSG scenes"""
    api = rl.api
    rows = []
    for name, scene, field, dtype, change in [
            ("A.rtc.shape_material", "mirror", "shapes", api.RTC_SHAPE, lambda t, d: t["material"].__setitem__(0, d.n_materials)),
            ("A.rtc.pattern_kind.none", "mirror", "patterns", api.RTC_PATTERN, lambda t, d: t["kind"].__setitem__(0, 0)),
            ("A.rtc.material_pattern", "mirror", "materials", api.RTC_MATERIAL, lambda t, d: t["pattern"].__setitem__(0, d.n_patterns + 1)),
            ("A.rtc.csg_operation", "csg", "csgs", api.RTC_CSG, lambda t, d: t["operation"].__setitem__(0, api.CSG_DIFFERENCE + 1)),
            ("B.reflection_depth.8.full_kernel", "mirror", None, None, lambda t, d: setattr(d, "max_reflection_depth", 8))]:
        world = rl.RtcWorld.test_mirror_scene(30, 20) if scene == "mirror" else rl.RtcWorld.test_csg_scene(30, 20)
        d = api.RtcSceneDesc.from_buffer_copy(api.RtcSceneDesc.from_address(world.desc))
        keep = [world]
        if field is None:
            change(None, d)
        else:
            n = getattr(d, "n_" + field)
            table = np.frombuffer((C.c_char * (n * dtype.itemsize)).from_address(getattr(d, field)), dtype=dtype).copy()
            change(table, d)
            keep.append(table)
            setattr(d, field, table.ctypes.data)
        rows.append((name, d, keep))
    return rows


def test_refusals_through_the_c_abi_create_nothing_and_disturb_nothing(rl):
    rl.init(0)
    api = rl.api
    L = api.render_lib()
    before_bytes = _golden_bytes(rl)
    before = api.live_buffers()
    rows = [(L.rl_rtiow_scene_create, r) for r in _rtiow_rows(rl)] + [(L.rl_rtc_scene_create, r) for r in _rtc_rows(rl)]
    assert len(rows) == 12
    for create, (name, desc, keep) in rows:
        code, message = {**A, **B}[name]
        assert code < 0 and message
        handle = create(C.addressof(desc))
        assert not handle, name
        assert L.rl_last_error().decode() == message, (name, L.rl_last_error().decode())
        assert api.live_buffers() == before, name
    assert _golden_bytes(rl) == before_bytes
