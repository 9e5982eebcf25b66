// Material queries (include/rl_render.h rl_rtiow_scatter_rays*, rl_rtiow_texture_values*): the kernels whose input is a buffer of hit
// records instead of a ray to trace.
//
//   rtiow_scatter_rays_kernel    Material::scatter(&mut rng, &ray, &hit_record) and Material::emitted(u, v, &p) (material.rs:11-20) for
//                                every element, the draws taken from the element's own cursor
//   rtiow_texture_values_kernel  Texture::value(u, v, &p) (texture.rs) for a buffer of (texture id, uv, p)
//
// The material arithmetic is material_texture + material_scatter (rl_rtiow_scatter.h), the same inlined statement the general renders' SHADE
// blocks use: a host loop of rl_rtiow_hit_rays + rl_rtiow_scatter_rays reproduces rl_rtiow_ray_color_rays bit for bit
// (tests/test_gpu_material_query.py).  What is this kernel's own is the record packing, the cursors and the lazy stream start; the render
// kernels carry none of that.  One element per lane, grid-stride over the batch;
// the lane's ChaCha8 blocks live in a Ring column (ODD: a cursor may stand at any word), regenerated for every element that draws.
// Records move as whole 8-byte words.  MATERIAL_QUERY_MAX_BLOCKS_PER_CU bounds the grid: a batch beyond it puts several elements, each
// on its own stream, through one lane.
#pragma once
#include "rl_rtiow_scatter.h"
#include "rl_rtiow_wave.h"

namespace rl {

static constexpr int MATERIAL_QUERY_NT = 256;
static constexpr int MATERIAL_QUERY_MAX_BLOCKS_PER_CU = 8;

struct MaterialQuery {
  unsigned long long n;
  uint32_t n_materials, n_textures;
  // scatter
  const rl_ray *rays;
  const rl_rtiow_hit *hits;
  const rl_rng_cursor *cursors;
  rl_rtiow_scatter *out;
  rl_rng_cursor *out_cursors;  // null: not wanted (may be `cursors`: a lane reads its element's cursor before it writes it)
  // texture values
  const uint32_t *tex_ids;
  const double *uv;  // [n][2]
  const double *p;   // [n][3]
  double *rgb;       // [n][3]
};

// The query's draws for material_scatter: the element's two blocks are generated just before its first draw, so an element that draws
// nothing generates none
template <class RingT>
struct LazyDraws {
  RingT &rng;
  uint64_t stream;
  bool started;
  __device__ __forceinline__ void start() {
    if (!started) rng.reset_stream(stream), started = true;
  }
  __device__ __forceinline__ D3 unit_sphere() {
    start();
    return rng.unit_sphere();
  }
  __device__ __forceinline__ double gen_f64() {
    start();
    return rng.gen_f64();
  }
};

// P: the scene's material / texture / image / Perlin tables, key (expanded from the call's seed) and stats ([0] elements with a hit,
// [5] words consumed, [6] flagged)
template <int NT>
__global__ void RL_KERNEL_ALIGN __launch_bounds__(NT) rtiow_scatter_rays_kernel(RtiowParams P, MaterialQuery Q) {
  __shared__ unsigned long long s_rng[16 * NT];
  const int tid = threadIdx.x;
  Ring<NT, true, true> rng{P.key, s_rng, tid, 0ull, 0u, 0u, 0u};
  unsigned long long c_rays = 0, c_flag = 0, c_words = 0;
  for (unsigned long long idx = (unsigned long long)blockIdx.x * NT + tid; idx < Q.n; idx += (unsigned long long)gridDim.x * NT) {
    const uint64_t *cur = (const uint64_t *)(Q.cursors + idx);
    const uint64_t stream = cur[0], word_pos = cur[1];
    const double *h = (const double *)(Q.hits + idx);
    const uint64_t hw9 = ((const uint64_t *)h)[9], hw10 = ((const uint64_t *)h)[10];  // hit | front_face << 32, material | _pad << 32
    const uint32_t mat = (uint32_t)hw10;
    double *out = (double *)(Q.out + idx);
    if ((uint32_t)hw9 == 0u || mat >= Q.n_materials) {  // None, or an index outside the table (device form; the host form refuses it): zeros
#pragma unroll
      for (int i = 0; i < 13; i++) out[i] = 0.0;
      ((uint64_t *)out)[13] = 0ull;
      if (Q.out_cursors) {
        uint64_t *oc = (uint64_t *)(Q.out_cursors + idx);
        oc[0] = stream, oc[1] = word_pos;
      }
      continue;
    }
    c_rays++;
    const bool front = (uint32_t)(hw9 >> 32) != 0u;
    const D3 p = d3(h[1], h[2], h[3]);
    const DevMaterial &m = P.materials[mat];
    // (acos / atan2 are the caller's already: hit.u, hit.v)
    const D3 texc = material_texture<true>(m, [&](uint32_t tex) { return texture_value<2>(P, tex, h[7], h[8], p); });
    const D3 normal = d3(h[4], h[5], h[6]);
    const double *r = (const double *)(Q.rays + idx);
    const D3 wd = d3(r[3], r[4], r[5]);
    const double time = r[6];
    rng.stream = stream, rng.pos = (uint32_t)word_pos, rng.nres = 0;
    LazyDraws<decltype(rng)> draws{rng, stream, false};
    const Scatter s = material_scatter<true>(m, wd, normal, front, [&] { return texc; }, draws);  // (an absorbed reflection has consumed its draws all the same)
    if (s.flagged) c_flag++;  // on with the renders' value
    const bool some = s.what == SCATTER_RAY;
    const D3 att = s.att, emitted = s.emitted, nd = s.dir;  // (att, emitted: zeros unless a ray was scattered / light emitted; nd is written only if `some`)
    c_words += rng.pos - (uint32_t)word_pos;
    out[0] = att.x, out[1] = att.y, out[2] = att.z;
    out[3] = emitted.x, out[4] = emitted.y, out[5] = emitted.z;
    if (some) {
      out[6] = p.x, out[7] = p.y, out[8] = p.z, out[9] = nd.x, out[10] = nd.y, out[11] = nd.z, out[12] = time;
    } else {
#pragma unroll
      for (int i = 6; i < 13; i++) out[i] = 0.0;
    }
    ((uint64_t *)out)[13] = some ? 1ull : 0ull;
    if (Q.out_cursors) {
      uint64_t *oc = (uint64_t *)(Q.out_cursors + idx);
      oc[0] = stream, oc[1] = (uint64_t)rng.pos;
    }
  }
  unsigned long long v;
  v = wave_sum(c_rays);
  if ((tid & 63) == 0 && v) atomicAdd(&P.stats[0], v);
  v = wave_sum(c_words);
  if ((tid & 63) == 0 && v) atomicAdd(&P.stats[5], v);
  v = wave_sum(c_flag);
  if ((tid & 63) == 0 && v) atomicAdd(&P.stats[6], v);
}

// out_rgb[3i ..] = textures[tex_ids[i]].value(uv[2i], uv[2i + 1], p[3i ..]); an id outside the table gives zeros
template <int NT>
__global__ void RL_KERNEL_ALIGN __launch_bounds__(NT) rtiow_texture_values_kernel(RtiowParams P, MaterialQuery Q) {
  const int tid = threadIdx.x;
  for (unsigned long long idx = (unsigned long long)blockIdx.x * NT + tid; idx < Q.n; idx += (unsigned long long)gridDim.x * NT) {
    const uint32_t tex = Q.tex_ids[idx];
    D3 c = d3(0.0, 0.0, 0.0);
    if (tex < Q.n_textures) {
      const double *uv = Q.uv + idx * 2, *p = Q.p + idx * 3;
      c = texture_value<2>(P, tex, uv[0], uv[1], d3(p[0], p[1], p[2]));
    }
    double *o = Q.rgb + idx * 3;
    o[0] = c.x, o[1] = c.y, o[2] = c.z;
  }
}

}  // namespace rl
