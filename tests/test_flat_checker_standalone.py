"""CPU tier: which spheres flatten_sphere_materials (csrc/rl_scene_host.cpp) gives the flat form of a Checker of two Solid colours, as a
stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer.  tests/host/flat_checker_check.cpp compiles a world with a
flat checker on a Lambertian, on a DiffuseLight and on one material shared by two spheres, nested and half-nested checkers, a Solid, a
Metal and a Dielectric, and checks flag, colours and inv_scale of every sphere's records bit for bit: the GPU test
(tests/test_gpu_flat_checker.py) compares a flat scene with a nested one, and this is what says that the two take different paths."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "rendering-learning_amd")
SOURCES = [os.path.join(ROOT, "tests", "host", "flat_checker_check.cpp")] + [os.path.join(PKG, "csrc", f + ".cpp") for f in ("rl_program", "rl_fast_bvh", "rl_scene_host")]
FLAGS = ["-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def test_flat_checker_records(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++ on PATH")
    objs, jobs = [], []
    for src in SOURCES:  # the four compiles side by side
        objs.append(str(tmp_path / (os.path.basename(src) + ".o")))
        jobs.append(subprocess.Popen([gxx, *FLAGS, "-I", PKG, "-c", "-o", objs[-1], src], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    for src, job in zip(SOURCES, jobs):
        log = job.communicate()[0]
        assert job.returncode == 0, f"{src}:\n{log}"
    exe = str(tmp_path / "flat_checker_check")
    r = subprocess.run([gxx, *FLAGS, "-o", exe, *objs], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stderr == "", r.stderr
    assert r.stdout.strip().endswith("10 spheres checked, 0 failures"), r.stdout
