"""CPU tier: tools/wave_codegen.py on this tree, for the end of a walk in the fast wave kernels (csrc/rl_rtiow_wave_body.inc).  A miss is
left to GEN instead of being resolved inside the TRAV step, and SHADE writes the next ray over the old one, so the step body is shorter
than the 74 VALU instructions it had with the miss resolved in place, SHADE's pick path copies less than the 100 registers it copied with
two rays alive (both figures: profiles/wave_state_inplace.txt), and the headline kernel needs at most 120 of its 128 VGPRs."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAST = ("headline", "steal", "indep", "moments")


@pytest.fixture(scope="module")
def report():
    spec = importlib.util.spec_from_file_location("wave_codegen", os.path.join(ROOT, "tools", "wave_codegen.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    hipcc = tool.makefile_flags(ROOT)[0]
    if not os.path.exists(hipcc):
        pytest.fail(f"{hipcc} not found: the report compiles the kernels")
    return tool.report(ROOT, FAST)


@pytest.mark.parametrize("name", FAST)
def test_trav_step_is_shorter_than_with_the_miss_resolved_in_it(report, name):
    t = report[name]["paths"]["TRAV"]
    print(name, "TRAV", t)
    assert t["step"] < 74, (name, t)


def test_shade_copies_fewer_registers_than_with_two_rays_alive(report):
    s = report["headline"]["paths"]["SHADE"]
    print("headline SHADE", s)
    assert s["mov"] < 100, s


def test_headline_kernel_frees_registers(report):
    k = report["headline"]["kernel"]
    print("headline", k)
    assert k["vgpr_count"] <= 120 and k["agpr_count"] == 0, k
    assert k["vgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0, k
