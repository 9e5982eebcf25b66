// The stopping rule of the adaptive renders (include/rl_render.h "Adaptive renders"): the one statement that the GEN blocks
// of rl_rtiow_wave_body.inc, rl_rtiow_fastgen_body.inc and rl_rtiow_wave_general_body.inc (their MOMENTS instantiations) decide with, at a
// sample boundary, whether a pixel is finished before it has taken all its samples.  The counts are equal through every kernel because
// they inline this text, and equal to a numpy evaluation of the header's formula because it is multiplies, adds and one comparison in
// binary64, each rounded on its own (the library is built with -ffp-contract=off).
#pragma once
#include "rl_rtiow_kernel.h"

namespace rl {

// one channel: n * sq - sum^2 <= (n - 1) * (abs * n^2 + rel * sum^2), i.e. variance of the mean <= abs + rel * mean^2 multiplied through by
// n^2 (n - 1).  A NaN anywhere compares false: the pixel runs on.
__device__ __forceinline__ bool rtiow_adaptive_ok(double nd, double sum, double sq, double abs_variance, double rel_variance) {
  const double s2 = sum * sum;
  const double lhs = (nd * sq) - s2;
  const double rhs = (nd - 1.0) * ((abs_variance * (nd * nd)) + (rel_variance * s2));
  return lhs <= rhs;
}

// n = the samples of this call that sum and sq hold.  True when n is a checkpoint (min_samples + k * check_every) short of the call's
// samples_per_pixel (`total`) at which all three channels pass.
__device__ __forceinline__ bool rtiow_adaptive_stop(const rl_rtiow_adaptive &rule, uint32_t total, uint32_t n, const D3 &sum, const D3 &sq) {
  if (n >= total || n < rule.min_samples || (n - rule.min_samples) % rule.check_every != 0u) return false;
  const double nd = (double)n;
  return rtiow_adaptive_ok(nd, sum.x, sq.x, rule.abs_variance, rule.rel_variance) && rtiow_adaptive_ok(nd, sum.y, sq.y, rule.abs_variance, rule.rel_variance) &&
         rtiow_adaptive_ok(nd, sum.z, sq.z, rule.abs_variance, rule.rel_variance);
}

}  // namespace rl
