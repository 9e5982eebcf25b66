"""CPU tier: the host scene compilers on BAD descriptions, as a stand-alone program under AddressSanitizer and
UndefinedBehaviorSanitizer.  Every kernel trusts the program build_host_rtiow / build_host_rtc compile from the caller's description,
so what they refuse — and that they refuse it without crashing, hanging or throwing — is checked here, before any device sees it.
tests/host/scene_desc_check.cpp holds the cases (its head describes the five parts and the program checker); this module builds it the
way test_scene_host_standalone.py builds its program, runs the executable as it is (nothing preloaded, no sanitizer options) and compares
its lines with the table below.  A second build WITHOUT sanitizers runs the allocation-failure cases under a 1 GiB address-space limit
(AddressSanitizer reserves terabytes of address space, which rules a limit out there)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "rendering-learning_amd")
LIBRARY = [os.path.join(PKG, "csrc", f + ".cpp") for f in ("rl_program", "rl_fast_bvh", "rl_scene_host")]
SOURCES = [os.path.join(ROOT, "tests", "host", "scene_desc_check.cpp")] + LIBRARY
PLAIN = ["-std=c++17", "-O1", "-g", "-ffp-contract=off"]
FLAGS = PLAIN + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
TIMEOUT = 120  # seconds for the whole executable (it needs about twenty): only so that a regression fails instead of hanging the suite

OK, INVALID, UNSUPPORTED, NOMEM = 0, -1, -4, -6

# case: (return code, message).  A refusal leaves `out` null, an acceptance sets it and the program passed the checker (the executable
# asserts both for every case and every mutation; the `out is null` column is compared here as well).
NULLS_RTIOW = ("spheres", "planars", "translates", "transforms", "bvh_nodes", "lists", "list_items", "materials", "textures", "images", "perlins", "media")
NULLS_RTC = ("triangles", "groups", "group_items", "boundeds", "transformeds", "materials", "objects", "lights", "shapes", "csgs", "patterns")
MEDIUM = "a ConstantMedium boundary must not contain another medium"
CHECKER = "checker textures nest cyclically or deeper than 32"
A = {
    **{f"A.base.{n}": (OK, "") for n in ("cornell_smoke", "checkered_spheres", "perlin_spheres", "image", "rtc_csg", "rtc_mirror", "rtc_mixed", "rtc_mesh")},
    **{f"A.rtiow.null.{n}": (INVALID, f"null array: {n}") for n in NULLS_RTIOW},
    "A.rtiow.too_many_spheres": (INVALID, "too many spheres"),
    "A.rtiow.perlin_permutation": (INVALID, "perlin permutation entry out of range"),
    "A.rtiow.image_no_data.width": (INVALID, "Image has no data"),
    "A.rtiow.image_no_data.pixels": (INVALID, "Image has no data"),
    "A.rtiow.checker_child": (INVALID, "checker texture child out of range"),
    "A.rtiow.image_index": (INVALID, "image index out of range"),
    "A.rtiow.perlin_index": (INVALID, "perlin index out of range"),
    "A.rtiow.texture_kind": (INVALID, "unknown texture kind"),
    "A.rtiow.checker_cycle": (INVALID, CHECKER),
    "A.rtiow.material_kind": (INVALID, "unknown material kind"),
    "A.rtiow.material_texture": (INVALID, "material texture out of range"),
    "A.rtiow.sphere_material": (INVALID, "sphere material out of range"),
    "A.rtiow.planar_material": (INVALID, "planar material out of range"),
    "A.rtiow.planar_kind": (INVALID, "unknown planar kind"),
    "A.rtiow.sphere_index": (INVALID, "sphere index out of range"),
    "A.rtiow.planar_index": (INVALID, "planar index out of range"),
    "A.rtiow.translate_index": (INVALID, "translate index out of range"),
    "A.rtiow.transform_index": (INVALID, "transform index out of range"),
    "A.rtiow.bvh_index": (INVALID, "bvh node index out of range"),
    "A.rtiow.list_index": (INVALID, "list index out of range"),
    "A.rtiow.medium_index": (INVALID, "medium index out of range"),
    "A.rtiow.hittable_kind.none": (INVALID, "unknown hittable kind"),
    "A.rtiow.hittable_kind.above": (INVALID, "unknown hittable kind"),
    "A.rtiow.cycle_list": (INVALID, "cycle through a list"),
    "A.rtiow.cycle_bvh": (INVALID, "cycle through a bvh node"),
    "A.rtiow.cycle_instance": (INVALID, "cycle through an instance"),
    "A.rtiow.medium_in_medium": (INVALID, MEDIUM),
    "A.rtiow.medium_in_itself": (INVALID, MEDIUM),
    "A.rtiow.list_range": (INVALID, "list range out of bounds"),
    "A.rtiow.bvh_children.none": (INVALID, "bvh node must have 1 or 2 children"),
    "A.rtiow.bvh_children.three": (INVALID, "bvh node must have 1 or 2 children"),
    "A.rtiow.medium_material": (INVALID, "medium material out of range"),
    **{f"A.rtc.null.{n}": (INVALID, f"null array: {n}") for n in NULLS_RTC},
    "A.rtc.triangle_material": (INVALID, "triangle material out of range"),
    "A.rtc.shape_material": (INVALID, "shape material out of range"),
    "A.rtc.pattern_kind.none": (INVALID, "unknown pattern kind"),
    "A.rtc.pattern_kind.above": (INVALID, "unknown pattern kind"),
    "A.rtc.material_pattern": (INVALID, "material pattern out of range"),
    "A.rtc.triangle_index": (INVALID, "triangle index out of range"),
    "A.rtc.group_index": (INVALID, "group index out of range"),
    "A.rtc.bounded_index": (INVALID, "bounded index out of range"),
    "A.rtc.transformed_index": (INVALID, "transformed index out of range"),
    "A.rtc.shape_index": (INVALID, "shape index out of range"),
    "A.rtc.csg_index": (INVALID, "csg index out of range"),
    "A.rtc.shape_kind_mismatch": (INVALID, "shape kind does not match its reference"),
    "A.rtc.object_kind.none": (INVALID, "unknown object kind"),
    "A.rtc.object_kind.above": (INVALID, "unknown object kind"),
    "A.rtc.cycle_group": (INVALID, "cycle through a group"),
    "A.rtc.cycle_bounded": (INVALID, "cycle through a bounded"),
    "A.rtc.cycle_transformed": (INVALID, "cycle through a transformed"),
    "A.rtc.cycle_csg": (INVALID, "cycle through a csg"),
    "A.rtc.csg_operation": (INVALID, "unknown csg operation"),
    "A.rtc.group_range": (INVALID, "group range out of bounds"),
}
# the refusals that are caps: each with the case at the cap beside it
B = {
    "B.instances.8": (OK, ""),
    "B.instances.9": (INVALID, "instances nested deeper than 8"),
    "B.checker.32": (OK, ""),
    "B.checker.33": (INVALID, CHECKER),
    "B.transformed.8": (OK, ""),
    "B.transformed.9": (INVALID, "Transformed nesting deeper than 8"),
    "B.csg.4": (OK, ""),
    "B.csg.5": (INVALID, "CSG nesting deeper than 4"),
    "B.lights.65535": (OK, ""),
    "B.lights.65536": (UNSUPPORTED, "too many lights"),
    "B.reflection_depth.7.full_kernel": (OK, ""),
    "B.reflection_depth.8.full_kernel": (UNSUPPORTED, "max_reflection_depth above 7 is not supported by the device kernel"),
    "B.reflection_depth.8.reduced_kernel": (OK, ""),
    "B.spheres.above_index_field": (INVALID, "too many spheres"),
    "B.list_range.at_end": (OK, ""),
    "B.list_range.past_end": (INVALID, "list range out of bounds"),
    "B.list_range.wraps": (INVALID, "list range out of bounds"),
    "B.group_range.at_end": (OK, ""),
    "B.group_range.past_end": (INVALID, "group range out of bounds"),
    "B.group_range.wraps": (INVALID, "group range out of bounds"),
}
# depth (each on a thread with a 1 MiB stack) and sharing
DEEP = "scene graph too deep"
C = {
    **{f"C.{g}.at_max_nest": (OK, "") for g in ("lists", "bvh", "groups", "boundeds")},
    **{f"C.{g}.one_deeper": (INVALID, DEEP) for g in ("lists", "bvh", "groups", "boundeds")},
    "C.checkers.2000000": (INVALID, CHECKER),
}
D = {
    "D.rtiow.ops_at_limit": (INVALID, "program too large"),
    "D.rtiow.60_levels.sphere": (INVALID, "program too large"),
    "D.rtc.60_levels.sphere": (INVALID, "program too large"),
    "D.rtiow.60_levels.empty": (OK, ""),  # a graph that expands to nothing is an empty world: the program is its end op alone
    "D.rtc.60_levels.empty": (OK, ""),
    "D.rtiow.20_levels.sphere": (OK, ""),
    "D.rtc.20_levels.sphere": (OK, ""),
    # children that expand to nothing, and lists of one item, under 2^20 expansions of their parent: compiled in time proportional to the ops
    "D.rtiow.20_levels.sphere_and_empties": (OK, ""),
    "D.rtc.20_levels.sphere_and_empties": (OK, ""),
    "D.rtiow.20_levels.wrappers": (OK, ""),
    "D.rtc.20_levels.wrappers": (OK, ""),
}
NOMEM_MESSAGE = "out of memory while compiling the scene"
D_NOMEM = {n: (NOMEM, NOMEM_MESSAGE) for n in ("D.nomem.rtiow.27_levels", "D.nomem.rtc.27_levels", "D.nomem.rtiow.ops_below_limit")}
CASES = {**A, **B, **C, **D}
E_SCENES = ("cornell_smoke", "checkered_spheres", "perlin_spheres", "image", "rtc_csg", "rtc_mirror", "rtc_mixed", "rtc_mesh")

# a message of the code that no description can trigger, with the reason
NOT_FROM_A_DESCRIPTION = {"scene compiler: ": "prefix of an exception other than std::bad_alloc: the compilers throw none themselves",
                          "scene compiler: unknown exception": "the catch-all behind it"}


def _compile(gxx, out, tag, flags):
    objs, jobs = [], []
    for src in SOURCES:
        objs.append(str(out / (tag + os.path.basename(src) + ".o")))
        jobs.append((src, subprocess.Popen([gxx, *flags, "-I", PKG, "-c", "-o", objs[-1], src], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)))
    return objs, jobs


def _parse(stdout):
    cases, other = {}, []
    for line in stdout.splitlines():
        if line.startswith("case "):
            name, rc, out_null, message, facts = (f.strip() for f in line[5:].split("|"))
            assert name not in cases, line
            cases[name] = (int(rc), message, int(out_null), facts)
        else:
            other.append(line)
    return cases, other


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++ on PATH")
    out = tmp_path_factory.mktemp("scene_desc")
    builds = {"asan": _compile(gxx, out, "asan_", FLAGS), "plain": _compile(gxx, out, "plain_", PLAIN)}  # the eight compiles side by side
    exe = {}
    for tag, (objs, jobs) in builds.items():
        for src, job in jobs:
            log = job.communicate()[0]
            assert job.returncode == 0, f"{src}:\n{log}"
        exe[tag] = str(out / ("scene_desc_check_" + tag))
        r = subprocess.run([gxx, *(FLAGS if tag == "asan" else PLAIN), "-o", exe[tag], *objs, "-lpthread"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, r.stdout
    result = {}
    for tag, args in (("asan", []), ("plain", ["nomem"])):
        r = subprocess.run([exe[tag], *args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=TIMEOUT)
        assert r.stderr == "", r.stderr
        assert r.returncode == 0, r.stdout[-4000:]
        result[tag] = _parse(r.stdout)
    return result


def _compare(got, want):
    assert set(got) == set(want), sorted(set(got) ^ set(want))
    for name, (rc, message) in want.items():
        g_rc, g_message, g_null, g_facts = got[name]
        assert (g_rc, g_message) == (rc, message), name
        assert g_null == (0 if rc == OK else 1), name
        assert (g_facts.endswith(" checked") if rc == OK else g_facts == ""), (name, g_facts)


def test_every_case_ends_as_the_table_says(runs):
    cases, other = runs["asan"]
    assert not [l for l in other if l.startswith("FAIL")], other
    _compare(cases, CASES)


def test_running_out_of_memory_is_a_return_code(runs):
    cases, other = runs["plain"]
    assert not [l for l in other if l.startswith("FAIL")], other
    _compare(cases, D_NOMEM)


def test_every_single_field_mutation_is_refused_or_compiles_to_a_checked_program(runs):
    """The executable fails a mutation whose outcome is neither (and a class that was never refused, or an index class never accepted);
    here: every base scene was mutated, and in numbers that show the enumeration ran."""
    _, other = runs["asan"]
    counts = {}
    for line in other:
        m = re.match(r"E (\w+): (\d+) mutations, (.*)", line)
        if m:
            counts[m.group(1)] = (int(m.group(2)), {k: (int(a), int(r)) for k, a, r in re.findall(r"(\w+) (\d+) \((\d+) refused\)", m.group(3))})
    assert set(counts) == set(E_SCENES)
    for scene, (total, by_class) in counts.items():
        assert total == sum(a for a, _ in by_class.values()) and total >= 90, scene
        for cls in ("index_too_large", "kind_unknown", "null_array"):
            applied, refused = by_class[cls]
            assert applied > 0 and refused == applied, (scene, cls)
        applied, refused = by_class["index_other_valid"]
        assert 0 <= refused < applied, scene


def refusal_sites():
    """message -> the files that hold it, for every fail("...") / err = "..." / need(..., "...") of the compiler sources"""
    found = {}
    for path in LIBRARY + [os.path.join(PKG, "csrc", "rl_program.h"), os.path.join(PKG, "csrc", "rl_scene_host.h")]:
        text = open(path).read()
        messages = re.findall(r'\bfail\("([^"]+)"\)', text) + re.findall(r'\berr = (?:std::string\()?"([^"]+)"', text)
        messages += ["null array: " + what for what in re.findall(r'\bneed\([^;{}"]*?"(\w+)"\)', text)]
        for m in messages:
            found.setdefault(m, set()).add(os.path.basename(path))
    return found


def test_every_refusal_in_the_sources_has_a_row():
    """A new refusal cannot arrive untested: each message the sources can put into `err` is the message of a row above (or the head of
    one, where the code appends a number)."""
    found = refusal_sites()
    assert len(found) >= 75, sorted(found)  # the search itself still finds the sites (12 + 11 null arrays, 50-odd others)
    rows = {message for _, message in {**CASES, **D_NOMEM}.values() if message}
    missing = [m for m in found if m not in NOT_FROM_A_DESCRIPTION and m != "null array: " and not any(r == m or (m.endswith(" ") and r.startswith(m)) for r in rows)]
    assert not missing, missing
    stale = [r for r in rows if not any(r == m or (m.endswith(" ") and r.startswith(m)) for m in found)]
    assert not stale, stale
