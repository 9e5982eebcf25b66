// RTIOW all-primitives kernel in wave-scheduled form: the schedule of rl_rtiow_wave.h (per-lane state
// machine, the wave runs the most populated state, path regeneration, two-block ChaCha ring in LDS,
// filtered AABB test) with the primitive coverage of rl_rtiow_general.h (planes / quads / triangles,
// Translate / Transform scopes, Image textures).  The scene program is read from HBM through L1 / L2 /
// Infinity Cache (cfg 4: 2 MB; cfg 5: ~150 MB), LDS holds the RNG rings only.
//
// States: GEN, TRAV (one box op), LEAF (1-2 sphere or planar tests with a full HitRecord), XF (enter /
// leave an instance scope), FILL, SHADE.  Instance scopes stay stackless exactly as in the nested-loop
// kernel: PUSH transforms the ray, POP transforms the hit found inside and restores the parent ray by
// replaying the enclosing PUSH chain from the world ray.
#pragma once
#include "rl_rtiow_general.h"
#include "rl_rtiow_wave.h"

namespace rl {

enum : uint32_t { ST_XF = 6 };

// TRANS: the scene needs the transcendental texture code (Noise, or Image textures on spheres -> get_sphere_uv); without it
// the kernel fits 168 VGPRs (3 waves per SIMD) instead of 256 (2 waves per SIMD)
// MEDIA: the scene holds ConstantMedium hittables (constant_medium.rs:27-80, the deterministic variant of include/rl_render.h rl_medium).
// A medium is a SCOPE of the threaded program, like an instance: OP_MEDIUM_BEGIN parks the closest hit found so far in LDS and walks the
// boundary's ops with ray_t = universe; OP_MEDIUM_END either restarts the walk with ray_t = (t1 + 0.0001, inf) (first pass found a hit)
// or closes the scope: the parked record comes back, and with both boundary hits the free path is drawn from the pixel's stream exactly
// where the reference's traversal evaluates the medium.  Boxes inside the scope are tested with the reference's divisions (the
// filtered test is derived for [1e-10, closest]).  Media do not nest (rl_program.cpp).
static const int MEDIA_SAVE_WORDS = 12;  // parked Rec: t, p, normal, u, v, w, {mat, pc}, flags
// INDEP: the sample-parallel mode, as in rtiow_wave_indep_kernel (rl_rtiow_wave.h; the body is included into both kernels for the same reason); rng_words are counted at every sample end
template <int NT, bool TRANS, bool STATS, bool MEDIA = false>
__global__ void RL_KERNEL_ALIGN __launch_bounds__(NT) rtiow_wave_general_kernel(RtiowParams P) {
  constexpr bool INDEP = false, RAYS = false, PIXELS = false, MOMENTS = never_v<NT>;
#include "rl_rtiow_wave_general_body.inc"
}
template <int NT, bool TRANS, bool STATS, bool MEDIA>
__global__ void RL_KERNEL_ALIGN __launch_bounds__(NT) rtiow_wave_general_indep_kernel(RtiowParams P) {
  constexpr bool INDEP = true, RAYS = false, PIXELS = false, MOMENTS = never_v<NT>;
#include "rl_rtiow_wave_general_body.inc"
}
// RAYS (rl_rtiow_ray_color_rays*): the reference-order form of the ray-buffer path query — counting calls, scenes without a
// fast tree, RL_FAST=0.  A slot is one ray with its own RNG cursor; rng_words counts the words each path consumed.
template <int NT, bool TRANS, bool STATS, bool MEDIA>
__global__ void RL_KERNEL_ALIGN __launch_bounds__(NT) rtiow_wave_general_rays_kernel(RtiowParams P) {
  constexpr bool INDEP = false, RAYS = true, PIXELS = false, MOMENTS = never_v<NT>;
#include "rl_rtiow_wave_general_body.inc"
}
// PIXELS (rl_rtiow_render_pixels*): a slot is one element of the caller's (x, y) list; the lane reads the pair once, runs the
// pixel's whole chained sample loop and stores the sums at the element's own index.  No tile order, no resume, no tile costs.  Serves the
// counting calls of every scene (sphere-only ones too: reference order, the counters of rtiow_wave_kernel's counting layouts) and the
// counter-free calls that have no fast path.
template <int NT, bool TRANS, bool STATS, bool MEDIA>
__global__ void RL_KERNEL_ALIGN __launch_bounds__(NT) rtiow_wave_general_pixels_kernel(RtiowParams P) {
  constexpr bool INDEP = false, RAYS = false, PIXELS = true, MOMENTS = never_v<NT>;
#include "rl_rtiow_wave_general_body.inc"
}
// MOMENTS (rl_rtiow_render_moments* / rl_rtiow_render_pixels_moments*): the frame and the list kernel once more, keeping the
// sum of the squared sample colours (P.out_sq) beside the sum.  The reference-order form: every counting moments call, every scene without
// a fast tree, and every moments call that would otherwise land in a kernel that has no MOMENTS flavour.  With P.out_count set
// (rl_rtiow_render_adaptive*) a pixel of the frame kernel also ends at the first checkpoint rtiow_adaptive_stop accepts.
template <int NT, bool TRANS, bool STATS, bool MEDIA>
__global__ void RL_KERNEL_ALIGN __launch_bounds__(NT) rtiow_wave_general_moments_kernel(RtiowParams P) {
  constexpr bool INDEP = false, RAYS = false, PIXELS = false, MOMENTS = true;
#include "rl_rtiow_wave_general_body.inc"
}
template <int NT, bool TRANS, bool STATS, bool MEDIA>
__global__ void RL_KERNEL_ALIGN __launch_bounds__(NT) rtiow_wave_general_pixels_moments_kernel(RtiowParams P) {
  constexpr bool INDEP = false, RAYS = false, PIXELS = true, MOMENTS = true;
#include "rl_rtiow_wave_general_body.inc"
}

}  // namespace rl
