"""CPU tier: the reject-only box trees build_rtc_guards (csrc/rl_scene_host.cpp) lays over the RTC triangle ranges, read back through
api.rtc_program (no device) and checked in numpy and binary64 on every world tests/test_gpu_rtc_meshes.py renders: the skip links close,
a depth-first walk meets each triangle of a range once and in index order, every leaf box holds its triangle and every parent box its
children (float(box) <= double(vertex), exactly), boxes are NaN exactly on the path from a vertex beyond 1e30 to the root, and the scene
size the launch compares with 64 KB is 64 n_ops + 160 n_tris + 32 n_guards.  The directed rays of the hard guard cases are checked here
too, on the oracle alone: at least half hit and at least a tenth miss, so the GPU tier compares both answers."""
import numpy as np
import pytest

import rtc_mesh_worlds as mw


def _worlds(rl):
    """(name, build) of every world of the GPU tier"""
    out = [(f"route {n}", lambda n=n: mw.route_world(rl, n)) for n in (7, 8, 292, 293, 1024)]
    out.append(("full 1024", lambda: mw.route_world(rl, 1024, reflective=(3,))))
    out += [(f"ranges depth {depth} same {same}", lambda depth=depth, same=same: mw.multi_range_world(rl, depth, same)) for depth in (2, 8) for same in (False, True)]
    out += [(name, build) for name, (build, _) in mw.hard_cases(rl).items()]
    out.append(("axis 293", lambda: mw.axis_world(rl, 293)))
    return out


def _holds(box, lo, hi):
    """float box >= the double interval [lo, hi] on every axis, exactly; a box of NaNs holds everything"""
    b = box.astype(np.float64)
    if np.isnan(b).all():
        return True
    return bool((b[0::2] <= lo).all() and (hi <= b[1::2]).all())


def check_program(api, prog):
    """-> (guarded ranges, unguarded ranges, deepest tree) after asserting every structural property of the program's guard trees"""
    ops, tris, guards = prog["ops"], prog["tris"], prog["guards"]
    assert prog["scene_bytes"] == 64 * len(ops) + 160 * len(tris) + 32 * len(guards)
    verts = mw.vertices(tris)
    huge = ~(np.abs(verts).max(axis=(1, 2)) <= 1e30)
    used = np.zeros(len(guards), dtype=bool)
    n_guarded = n_plain = deepest = 0
    for op in ops[ops["code"] == api.ROP_TRIS]:
        a, b = int(op["a"]), int(op["b"])
        if b < 8:
            assert op["skip"] == 0
            n_plain += 1
            continue
        n_guarded += 1
        root = int(op["skip"]) - 1
        end = int(guards["skip"][root])
        assert 0 <= root < end <= len(guards) and end - root == 2 * b - 1 and not used[root:end].any()
        used[root:end] = True
        leaves = []

        def walk(g, depth):
            """the subtree at node g -> (its end, whether its box must be NaN: a leaf below holds a vertex beyond 1e30)"""
            nonlocal deepest
            deepest = max(deepest, depth)
            nd = guards[g]
            if nd["tri"] != 0xFFFFFFFF:
                t = int(nd["tri"])
                leaves.append(t)
                assert nd["skip"] == g + 1 and a <= t < a + b
                assert _holds(nd["box"], verts[t].min(axis=0), verts[t].max(axis=0)), (g, t, nd["box"], verts[t])
                assert np.isnan(nd["box"]).all() == bool(huge[t]) and (np.isnan(nd["box"]).all() or not np.isnan(nd["box"]).any())
                return g + 1, bool(huge[t])
            left_end, left_nan = walk(g + 1, depth + 1)
            right_end, right_nan = walk(left_end, depth + 1)
            assert nd["skip"] == right_end, (g, nd["skip"], right_end)
            nan = np.isnan(nd["box"]).all()
            assert nan == (left_nan or right_nan) and (nan or not np.isnan(nd["box"]).any())  # NaN on the ancestors of a huge leaf, and on nothing else
            for child in (g + 1, left_end):
                cb = guards["box"][child].astype(np.float64)
                if not np.isnan(cb).all():
                    assert _holds(nd["box"], cb[0::2], cb[1::2]), (g, child, nd["box"], cb)
            return right_end, bool(nan)

        assert walk(root, 1)[0] == end
        assert leaves == list(range(a, a + b))
    assert used.all()  # no node outside every range
    return n_guarded, n_plain, deepest


def test_every_world_of_the_gpu_tier_has_sound_guard_trees(rl):
    api = rl.api
    seen = {}
    for name, build in _worlds(rl):
        prog = api.rtc_program(build())
        seen[name] = check_program(api, prog) + (prog["scene_bytes"], len(prog["tris"]))
    assert seen["route 7"][:2] == (0, 1) and seen["route 8"][:3] == (1, 0, 4)
    assert seen["route 1024"][2] == 11 and seen["route 1024"][3] == 96 + 224 * 1024  # deeper than any tree the suite walked before
    assert seen["route 292"][3] == 65504 and seen["route 293"][3] > 65536
    for depth in (2, 8):
        assert seen[f"ranges depth {depth} same False"][:2] == (2, 1) and seen[f"ranges depth {depth} same True"][:2] == (2, 1)
    for name, (_, _) in mw.hard_cases(rl).items():
        assert 64 <= seen[name][4] <= 300 and seen[name][0] >= 1, name


def test_second_and_third_ranges_start_where_the_previous_tree_ends(rl):
    api = rl.api
    prog = api.rtc_program(mw.multi_range_world(rl, 2, True))
    tr = prog["ops"][prog["ops"]["code"] == api.ROP_TRIS]
    assert [(int(o["a"]), int(o["b"]), int(o["skip"])) for o in tr] == [(0, 300, 1), (0, 300, 600), (300, 7, 0)]  # two trees over the same triangles
    prog = api.rtc_program(mw.multi_range_world(rl, 8, False))
    tr = prog["ops"][prog["ops"]["code"] == api.ROP_TRIS]
    assert [(int(o["a"]), int(o["b"]), int(o["skip"])) for o in tr] == [(0, 300, 1), (300, 40, 600), (340, 7, 0)]
    assert (prog["ops"]["code"] == api.ROP_ENTER).sum() == 8 and len(prog["guards"]) == 599 + 79


def test_a_vertex_beyond_1e30_makes_nan_boxes_on_its_path_only(rl):
    api = rl.api
    build, _ = mw.hard_cases(rl)["degenerate: zero area, needles, a vertex at 1e31"]
    prog = api.rtc_program(build())
    check_program(api, prog)  # asserts NaN exactly on the leaf and its ancestors
    g = prog["guards"]
    nan = np.isnan(g["box"]).all(axis=1)
    assert nan.sum() == 9 and nan[0] and (g["tri"][nan] == 120).sum() == 1  # 200 triangles: the leaf and the eight nodes above it
    # zero-area triangles and needles keep finite boxes, padded outwards on every axis
    verts = mw.vertices(prog["tris"])
    for t in (13, 30, 77, 99):
        leaf = g[g["tri"] == t][0]
        b = leaf["box"].astype(np.float64)
        assert (b[0::2] < verts[t].min(axis=0)).all() and (verts[t].max(axis=0) < b[1::2]).all(), (t, b, verts[t])


def test_boxes_are_padded_strictly_outwards_at_every_magnitude(rl):
    """The pad of box_of, 1e-6 (|min| + |max| + extent), is what keeps a float box outside its triangle after rounding: at coordinates of
    order 1e6 a float's spacing is 0.06, so without the pad a rounded-to-nearest box cuts into the triangle.  Every leaf box must lie
    strictly outside its triangle's, by at least a quarter of the pad."""
    api = rl.api
    cases = mw.hard_cases(rl)
    for name in ("offset 1e4", "offset 1e6, reflective", "extent 1e-4", "extent 1e4", "uniform scale 1e5"):
        prog = api.rtc_program(cases[name][0]())
        verts, g = mw.vertices(prog["tris"]), prog["guards"]
        leaves = g[g["tri"] != 0xFFFFFFFF]
        lo, hi = verts[leaves["tri"]].min(axis=1), verts[leaves["tri"]].max(axis=1)
        b = leaves["box"].astype(np.float64)
        pad = 1e-6 * (np.abs(lo) + np.abs(hi) + (hi - lo))
        assert (lo - b[:, 0::2] >= 0.25 * pad).all() and (b[:, 1::2] - hi >= 0.25 * pad).all(), name


@pytest.mark.parametrize("name", mw.CASE_NAMES)
def test_directed_rays_hit_and_miss_on_the_oracle(rl, oracle, name):
    """What the GPU tier relies on, from the oracle alone: of the directed rays at least half hit something and at least a tenth miss."""
    w = mw.hard_cases(rl)[name][0]()
    o, d = mw.directed_rays(w, 7)
    assert 200 <= len(o) <= 600
    hits = sum(len(oracle.rtc_intersect(w.desc, o[i], d[i], cap=64)[0]) > 0 for i in range(len(o)))
    print(name, "rays", len(o), "hit", hits)
    assert 2 * hits >= len(o) and 10 * (len(o) - hits) >= len(o), (name, hits, len(o))
