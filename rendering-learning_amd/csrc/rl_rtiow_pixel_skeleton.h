// What every pixel-render kernel is built around (rtiow_features_kernel, rtiow_ao_kernel, rtiow_direct_kernel, rtiow_nee_kernel; DESIGN.md
// §3.24): one pixel per lane, grid-stride over the slots of a shard's rows or of a pixel list, per lane a loop over the samples
// F .. F + S - 1, each sample a ChaCha stream of its own in an LDS ring.  Here: the pieces of that skeleton the four kernels CALL.  A piece
// is here only if every instantiation of every kernel that calls it came out with the instructions it had with the text written out
// (DESIGN.md §3.24 has the comparison).  The other repeated texts failed that test as functions — the slot decode, the sample start
// (reset_stream, Camera::get_ray, the time draw), the closest-hit statement, the any-hit segment statement, the counters as one struct —
// and stay written out in each kernel, which says so at the place.  rl_rtiow_features.h includes this file.
#pragma once

namespace rl {

// The dynamic LDS of a pixel-render kernel, the plan rl_pixel_render_api.h sizes, and (FAST) the tree's top staged by the whole
// workgroup: every thread of the block calls this once, before anything else.
template <int NT, bool FAST, int SD>
__device__ __forceinline__ void pixel_lds(unsigned char *smem, const RtiowParams &P, int tid, unsigned long long *&s_rng, uint32_t *&s_stack, uint4 *&s_top) {
  s_rng = (unsigned long long *)smem;                                           // [16][NT] ChaCha ring
  s_stack = (uint32_t *)(smem + (size_t)16 * NT * sizeof(unsigned long long));  // FAST: [SD][NT], the closest-hit and the any-hit walk in turn
  s_top = (uint4 *)(s_stack + (size_t)NT * SD);                                 // FAST: [fg_top] FastNodeQ
  if (FAST && P.fg_top) {
    for (uint32_t i = (uint32_t)tid; i < P.fg_top * 8u; i += (uint32_t)NT) s_top[i] = ((const uint4 *)P.fg_nodes)[i];
    __syncthreads();
  }
}

// A lane's counters into P.stats, one wave sum and one atomic per wave and counter: [0] rays, [5] words drawn, [6] flagged, FAST: [7] rays
// the fast walks handed to general_trace, STATS: [1..4].  Every thread of the block, behind the lanes' loops (wave-wide operations).
// By value: the kernels keep eight locals (one struct of them changed the code of all fifteen instantiations).
template <bool STATS, bool FAST>
__device__ __forceinline__ void pixel_flush_counters(unsigned long long *stats, int tid, unsigned long long rays, unsigned long long words, unsigned long long flag,
                                                     unsigned long long slow, unsigned long long nodes, unsigned long long sph, unsigned long long pl,
                                                     unsigned long long inst) {
  unsigned long long v;
  v = wave_sum(rays);
  if ((tid & 63) == 0 && v) atomicAdd(&stats[0], v);
  v = wave_sum(words);
  if ((tid & 63) == 0 && v) atomicAdd(&stats[5], v);
  v = wave_sum(flag);
  if ((tid & 63) == 0 && v) atomicAdd(&stats[6], v);
  if (FAST) {
    v = wave_sum(slow);
    if ((tid & 63) == 0 && v) atomicAdd(&stats[7], v);
  }
  if (STATS) {
    v = wave_sum(nodes);
    if ((tid & 63) == 0) atomicAdd(&stats[1], v);
    v = wave_sum(sph);
    if ((tid & 63) == 0) atomicAdd(&stats[2], v);
    v = wave_sum(pl);
    if ((tid & 63) == 0) atomicAdd(&stats[3], v);
    v = wave_sum(inst);
    if ((tid & 63) == 0) atomicAdd(&stats[4], v);
  }
}

}  // namespace rl
