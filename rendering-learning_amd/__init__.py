"""MI355X-native back end for the per-pixel / per-ray hot path of marcantony/rendering-learning.

Product = csrc/ (hand-written HIP for gfx950 behind the C ABI of include/rl_render.h) + host/ (C++
mirror of the reference's scene-building API).  `api` is the ctypes plumbing used by tests and bench.
"""
from . import api  # noqa: F401
from .api import (Adaptive, AtrousParams, Camera, CameraParams, Canvas, Features, Moments, RLError, RtcWorld, World, atrous_params, canvas_ppm,  # noqa: F401
                  denoise_atrous, denoise_atrous_pass_device, denoise_render, init, output_ppm, rtc_camera)
from .api import (DenoiseInputs, denoise_finish_device, denoise_inputs, denoise_prepare_device, denoise_render_device, denoise_render_gpu,  # noqa: F401
                  denoise_render_work_bytes)
from . import occlusion  # noqa: F401
from .occlusion import occluded_rays, occluded_rays_device  # noqa: F401
from . import ao  # noqa: F401
from .ao import AmbientOcclusion, render_ao, render_ao_device, render_pixels_ao, render_pixels_ao_device  # noqa: F401
from . import direct  # noqa: F401
from .direct import DirectLight, pack_lights, render_direct, render_direct_device, render_pixels_direct, render_pixels_direct_device  # noqa: F401
from . import nee  # noqa: F401
from .nee import PathNEE, render_nee, render_nee_device, render_pixels_nee, render_pixels_nee_device  # noqa: F401
from .nee import render_nee_mis, render_nee_mis_device, render_pixels_nee_mis, render_pixels_nee_mis_device  # noqa: F401
from .nee import pack_sphere_lights  # noqa: F401
from . import entry_table  # noqa: F401
