"""CPU tier: tools/wave_codegen.py on this tree.  The headline wave kernel must keep the register budget its occupancy rests on (one more
VGPR costs a wave per SIMD, a spill puts scratch traffic into the scheduler loop), and the report must find the scheduler loop's five
pick paths in every instantiation — a body whose marks no longer reach the assembly would make the report silently useless.
No instruction count is pinned here: those are recorded in profiles/wave_state_inplace.txt against the parent commit."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def report():
    spec = importlib.util.spec_from_file_location("wave_codegen", os.path.join(ROOT, "tools", "wave_codegen.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    hipcc = tool.makefile_flags(ROOT)[0]
    if not os.path.exists(hipcc):
        pytest.fail(f"{hipcc} not found: the report compiles the kernels")
    return tool, tool.report(ROOT)


def test_headline_kernel_register_budget(report):
    _, rep = report
    k = rep["headline"]["kernel"]
    assert k["vgpr_count"] <= 128 and k["agpr_count"] == 0, k
    assert k["vgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0, k


def test_report_lists_all_five_pick_paths_for_every_instantiation(report):
    tool, rep = report
    assert set(rep) == set(tool.INSTANCES) == {"headline", "steal", "indep", "moments", "counting"}
    for name, r in rep.items():
        assert set(r["paths"]) == set(tool.BLOCKS) == {"TRAV", "LEAF", "SHADE", "GEN", "FILL"}, name
        for blk, p in r["paths"].items():
            assert p["insts"] >= p["valu"] >= p["mov"] + p["lane"] and p["valu"] > 0, (name, blk, p)
        t = r["paths"]["TRAV"]
        assert 0 < 2 * t["step"] <= t["valu"], (name, t)  # the path runs two steps
