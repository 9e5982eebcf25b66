"""CPU tier: the status-gap test hook (rl_debug_set_status_gap, not part of the ABI) behind tests/test_gpu_status_accounting.py is
exported, wrapped in api.py, and fails LOUDLY (RL_E_NO_DEVICE) when no GPU is present instead of arming nothing silently."""
import os

import pytest
from pixel_family_abi import gpu_present

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_status_gap_hook_is_exported_and_wrapped(rl):
    lib = rl.api.render_lib()
    for s in ("rl_debug_set_status_gap", "rl_debug_set_fastg_one_wave"):
        assert hasattr(lib, s), s
        assert s not in rl.api.RENDER_SYMBOLS, s  # test switches, not part of the ABI
    assert callable(rl.api.set_status_gap) and callable(rl.api.set_fastg_one_wave)
    assert "rl_debug_set_status_gap" not in open(os.path.join(ROOT, "include", "rl_render.h")).read()


@pytest.mark.skipif(gpu_present(), reason="GPU present: the failure path is not reachable")
def test_status_gap_hook_without_a_device_fails_loudly(rl):
    api = rl.api
    assert api.render_lib().rl_init(-1) == api.RL_E_NO_DEVICE
    with pytest.raises(rl.RLError) as e:
        api.set_status_gap(1000, 1000)
    assert e.value.code == api.RL_E_NO_DEVICE
    assert api.render_lib().rl_debug_set_status_gap(0, 0) == api.RL_E_NO_DEVICE
