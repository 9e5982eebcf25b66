"""CPU tier: the two expressions behind the entry table's time slices (csrc/rl_pixel_entry_slices.h: which slice a sample's time falls into, and
the ball that holds a moving sphere during a slice), as a stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer.
tests/host/pixel_entry_time_check.cpp says what it checks; this module builds it once with g++, runs the executable as it is (nothing
preloaded, no sanitizer options) and reads its lines:
  * over more than 2^20 values of time, every k / T and its two neighbours among them, the slice index is the exact floor of time * T;
  * for 4096 spheres with centres and motions of magnitudes 1e-3 .. 1e3, every T in {2, 4, 8}, every slice and five times of it, the exact
    centre at that time lies within R_k - r - pad of the rounded slice centre, with room left for the kernel's own rounding of the centre."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "rendering-learning_amd")
SOURCES = [os.path.join(ROOT, "tests", "host", "pixel_entry_time_check.cpp")] + [os.path.join(PKG, "csrc", f + ".cpp") for f in ("rl_program", "rl_fast_bvh", "rl_scene_host")]
FLAGS = ["-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++ on PATH")
    out = tmp_path_factory.mktemp("pixel_entry_time")
    objs, jobs = [], []
    for src in SOURCES:  # the four compiles side by side
        objs.append(str(out / (os.path.basename(src) + ".o")))
        jobs.append(subprocess.Popen([gxx, *FLAGS, "-I", PKG, "-c", "-o", objs[-1], src], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    for src, job in zip(SOURCES, jobs):
        log = job.communicate()[0]
        assert job.returncode == 0, f"{src}:\n{log}"
    exe = str(out / "pixel_entry_time_check")
    r = subprocess.run([gxx, *FLAGS, "-o", exe, *objs], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    print(r.stdout)
    assert r.stderr == "", r.stderr
    lines = {}
    for line in r.stdout.splitlines():
        words = line.split()
        if words and words[0] in ("slices", "balls"):
            assert words[0] not in lines, line
            lines[words[0]] = dict(zip(words[1::2], words[2::2]))
    return r.returncode, r.stdout, lines


def test_the_program_found_nothing(report):
    rc, out, _ = report
    assert rc == 0 and "FAIL" not in out and "WRONG" not in out and out.rstrip().endswith("ok"), out


def test_the_slice_index_is_the_exact_floor(report):
    s = report[2]["slices"]
    assert int(s["times"]) >= 2 ** 20 + 3 * 7 + 3
    assert int(s["wrong"]) == 0


def test_a_slice_ball_holds_its_sphere_for_the_whole_slice(report):
    b = report[2]["balls"]
    assert int(b["spheres"]) == 4096
    assert int(b["checks"]) == 4096 * (2 + 4 + 8) * 5
    assert int(b["wrong"]) == 0
    assert float(b["margin"]) > 0.0
