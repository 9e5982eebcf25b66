"""CPU tier: the host scene compiler (csrc/rl_scene_host.cpp over rl_program.cpp and rl_fast_bvh.cpp) as a stand-alone program under
AddressSanitizer and UndefinedBehaviorSanitizer.  tests/host/scene_host_check.cpp compiles the example scenes and three hand-made ones
and prints one line per scene; this module builds it once with g++, runs the executable as it is (nothing preloaded, no sanitizer
options) and compares the lines with a table recorded from rl_debug_host_structures of the commit BEFORE the compiler left
rl_render.hip (profiles/scene_host_split.txt): the sanitizers must stay silent and the moved code must report what it reported."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "rendering-learning_amd")
SOURCES = [os.path.join(ROOT, "tests", "host", "scene_host_check.cpp")] + [os.path.join(PKG, "csrc", f + ".cpp") for f in ("rl_program", "rl_fast_bvh", "rl_scene_host")]
FLAGS = ["-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]

# name: the 16 words of the structure report (flags, items, binary_nodes, quad_nodes, leaves, dups, missing, box_violations, quad_depth,
# s_inner, s_leaves, s_bad_reach, s_box_violations, s_depth, media, media_shapes)
RTIOW = {
    "golden_test_scene": (1, 0, 0, 0, 0, 0, 0, 0, 0, 4, 5, 0, 0, 4, 0, 0),
    "bouncing_spheres": (1, 0, 0, 0, 0, 0, 0, 0, 0, 487, 488, 0, 0, 13, 0, 0),
    "checkered_spheres": (1, 0, 0, 0, 0, 0, 0, 0, 0, 1, 2, 0, 0, 2, 0, 0),
    "quads": (2, 5, 4, 2, 5, 0, 0, 0, 3, 0, 0, 0, 0, 0, 0, 0),
    "flat_world": (2, 5, 3, 1, 5, 0, 0, 0, 2, 0, 0, 0, 0, 0, 0, 0),
    "cornell_box": (2, 18, 17, 7, 18, 0, 0, 0, 4, 0, 0, 0, 0, 0, 0, 0),
    "cornell_smoke": (2, 6, 4, 4, 6, 0, 0, 0, 3, 0, 0, 0, 0, 0, 2, 0x1111),
    "perlin_spheres": (2, 2, 1, 1, 2, 0, 0, 0, 2, 0, 0, 0, 0, 0, 0, 0),
    "simple_light": (2, 4, 3, 1, 4, 0, 0, 0, 2, 0, 0, 0, 0, 0, 0, 0),
}
# name: (guards, ops, return code)
RTC = {"rtc_mirror": (0, 32, 0), "rtc_csg": (0, 19, 0), "rtc_teapot": (479, 5, 0)}


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++ on PATH")
    out = tmp_path_factory.mktemp("scene_host")
    objs, jobs = [], []
    for src in SOURCES:  # the four compiles side by side
        objs.append(str(out / (os.path.basename(src) + ".o")))
        jobs.append(subprocess.Popen([gxx, *FLAGS, "-I", PKG, "-c", "-o", objs[-1], src], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    for src, job in zip(SOURCES, jobs):
        log = job.communicate()[0]
        assert job.returncode == 0, f"{src}:\n{log}"
    exe = str(out / "scene_host_check")
    r = subprocess.run([gxx, *FLAGS, "-o", exe, *objs], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "teapot-low.obj")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stderr == "", r.stderr
    table = {}
    for line in r.stdout.splitlines():
        name, *words = line.split()
        assert name not in table, line
        table[name] = tuple(int(w) for w in words)
    return table


def test_example_scenes_report_what_the_parent_commit_reported(lines):
    for name, want in RTIOW.items():
        assert lines[name] == want, name
    for name, want in RTC.items():
        assert lines[name] == want, name
    assert set(lines) == set(RTIOW) | set(RTC) | {"twice_named_sphere", "radius_zero", "one_sphere"}


def test_hand_made_scenes(lines):
    keys = ("flags", "items", "binary_nodes", "quad_nodes", "leaves", "dups", "missing", "box_violations", "quad_depth",
            "s_inner", "s_leaves", "s_bad_reach", "s_box_violations", "s_depth", "media", "media_shapes")
    twice, zero, one = (dict(zip(keys, lines[n])) for n in ("twice_named_sphere", "radius_zero", "one_sphere"))
    # a sphere named twice: no guards, hence no fast tree (the program itself checks cops, lops and fast_root); a sphere-only world has
    # no general structure either, so every count stays zero
    assert twice["flags"] == 0 and not any(twice.values())
    assert zero["flags"] == 0  # a radius-0 sphere: its reject-only box cannot be padded, the scene stays on the reference-order layouts
    # one sphere: a tree without an inner node whose root is the leaf
    assert one["flags"] == 1 and one["s_inner"] == 0 and one["s_leaves"] == 1 and one["s_bad_reach"] == 0 and one["s_box_violations"] == 0 and one["s_depth"] == 1
