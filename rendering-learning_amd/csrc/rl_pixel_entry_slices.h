// Time slices of the per-pixel entry table (rl_pixel_entry.h, "Time slices"): the two expressions the table kernel and the render kernels'
// GEN block share — which slice a sample's time falls into, and the ball that holds a moving sphere during a slice.  Plain C++ as well as
// HIP: tests/host/pixel_entry_time_check.cpp compiles this file with g++ and checks both against exact arithmetic.
#pragma once
#include <cstdint>

#ifdef __HIPCC__
#define RL_SLICE_FN __host__ __device__ __forceinline__
#else
#define RL_SLICE_FN inline
#endif

namespace rl {

// How many time slices the table has by default (RL_PIXEL_ENTRY_TIME / rl_debug_set_pixel_entry_time: 1, 2, 4 or 8; 1 = the one word for all times)
static constexpr int PIXEL_ENTRY_TIME_DEFAULT = 4;
inline int pixel_entry_slices(int asked) { return asked == 1 || asked == 2 || asked == 4 || asked == 8 ? asked : PIXEL_ENTRY_TIME_DEFAULT; }

// The slice a sample's time falls into, of T = 1 << log2T.  T is a power of two and 0 <= time < 1 (gen_f64), so time * T is exact and the
// conversion truncates: this is floor(time T) exactly, for every time.  The clamp is for form.
RL_SLICE_FN uint32_t time_slice(double time, uint32_t log2T) {
  const uint32_t T = 1u << log2T, k = (uint32_t)(time * (double)T);
  return k < T - 1u ? k : T - 1u;
}

// The same slice from the draw itself: gen_f64 makes time = (u >> 11) 2^-53 of a 64-bit draw u, so floor(time T) is the top log2T bits of u,
// i.e. of its high word.  What GEN uses: one shift of a register the conversion reads anyway, where time * T asks for a binary64 temporary at
// the kernel's register peak (tools/kernel_regs.py: 120 VGPRs instead of 118).  (Two shifts: log2T = 0 would shift by the word's width.)
RL_SLICE_FN uint32_t time_slice_bits(uint32_t draw_hi, uint32_t log2T) { return (draw_hi >> 1) >> (31u - log2T); }

// The ball of slice k of T: ball = {c(1/2), R} of fast_leaf_balls (rl_fast_bvh.cpp), mo = {dc, h = |dc| / 2} beside it.  The centre at the
// middle of the slice, c(1/2) + dc s with s = (k + 1/2) / T - 1/2, and R_k = R - h (1 - 1 / T): s and 1 - 1 / T are exact (T a power of
// two), so each centre coordinate carries two roundings and the radius two: the form without contraction, which is how the library is
// built (-ffp-contract=off, csrc/Makefile) and how the host check builds it; a fused multiply-add would only drop one of the two.
RL_SLICE_FN void slice_ball(const double *ball, const double *mo, uint32_t k, uint32_t T, double *out) {
  const double inv = 1.0 / (double)T, s = ((double)k + 0.5) * inv - 0.5;
  out[0] = ball[0] + mo[0] * s, out[1] = ball[1] + mo[1] * s, out[2] = ball[2] + mo[2] * s;
  out[3] = ball[3] - mo[3] * (1.0 - inv);
}

}  // namespace rl
