// RTIOW hot path on gfx950: Camera::_render's per-pixel loop (camera.rs:145-199), get_ray (:203-230),
// ray_color (:232-260), Bvh/slice/Sphere hit (bvh.rs:79-95, hittable/mod.rs:88-105, sphere.rs:32-75,
// aabb.rs:123-152), the materials (material.rs) and textures (texture.rs), ChaCha8 stream RNG
// (rand_chacha 0.3.1 as used at camera.rs:161-170).
//
// This header holds what every RTIOW kernel shares: the parameter block, the ChaCha8 block function and
// per-lane RNG, the exact AABB and sphere tests, Perlin noise and the textures.  The kernels themselves are
// in rl_rtiow_general.h, rl_rtiow_wave.h, rl_rtiow_wave_general.h, rl_rtiow_fastgen.h and rl_rtiow_coop.h.
// Parallel unit = the pixel: samples of one pixel are sequentially dependent (set_stream keeps the
// ChaCha word position), pixels are independent.
#pragma once
#ifndef RL_KERNEL_ALIGN
// Every big kernel starts on a 64 KB boundary of the code object.  Measured (round 3): the stealing instantiation of rtiow_wave_kernel (77 KB of
// code: main loop + cooperative body, more than the 64 KB instruction cache two CUs share) ran the 1/8 shard in 174 or in 189 ms depending on
// nothing but where the linker happened to put it (0x...ad00 against 0x...d600 after unrelated kernels grew); aligned, the placement is fixed.
#define RL_KERNEL_ALIGN __attribute__((aligned(65536)))
#endif
#include "rl_device.h"

namespace rl {

struct RtiowParams {
  const DevOp *ops;
  const DevSphere *spheres;
  const uint32_t *sphere_material;
  const DevPlanar *planars;
  const rl_translate *translates;
  const rl_transform *transforms;
  const DevMaterial *materials;
  const DevTexture *textures;
  const DevImage *images;
  const float *image_pool;
  const rl_perlin *perlins;
  const rl_medium *media;
  uint32_t n_ops, n_spheres;
  const DevMaterial *sphere_flat;  // wave kernel: per-sphere flattened material (see flatten_sphere_materials)
  const DevOp *lops;  // wave kernel: ops with {code, skip} replaced by linked successor words (state << 29 | op index), see rl_scene_host.cpp link_ops
  uint32_t entry0;    // linked word of op 0: where (and in which state) a new ray starts
  const CompactOp *cops;    // wave kernel LDS_SCENE = 3: guarded compact ops (n_ops originals + one guard per sphere)
  const uint32_t *movbits;  // ... one bit per sphere: Center::Moving
  uint32_t n_cops, centry0;
  const FastNode *fast_nodes;  // wave kernel LDS_SCENE = 4: the fast traversal structure (n_fast_inner nodes; entry ids, rl_program.h)
  const FastNodeCH *fast_nodes_ch;  // ... the same nodes as centre / half-extent boxes: what the wave kernels stage into LDS and step through
  uint32_t n_fast_inner, fast_root;
  const FastNodeQ *fg_nodes;  // rl_rtiow_fastgen.h: fast traversal structure of a general scene (rl_fast_bvh.cpp build_fast_general)
  const DevSphere *fg_spheres;  // [item] sphere record of sphere items
  const uint32_t *fg_material;   // [item] material index
  const FastItem *fg_items;
  uint32_t fg_root;
  float fg_center[3], fg_rsafe2;  // r_safe squared
  float fg_radius, fg_pad_k;      // far-origin rays: box growth = fg_pad_k * (distance + fg_radius)^2 (rl_rtiow_fastgen.h start_ray)
  rl_rtiow_camera cam;
  uint32_t key[8];
  uint64_t first_sample;
  uint32_t row_first, row_step, nrows;
  uint32_t tiles_x, n_slots;
  uint32_t *work_counter;
  double *out;
  uint32_t sample_begin, sample_end, resume;  // wave kernel: this launch renders samples [begin, end); resume = continue saved pixels
  uint32_t *pos_state;                         // per-pixel ChaCha word position (saved at pixel end when non-null)
  const uint32_t *tile_order;                  // slot>>6 -> tile (LPT order) or null
  uint32_t *tile_cost;                         // per-tile ray count accumulated at pixel end, or null
  double k8u;                 // 8 * 2^-53, passed as a kernel argument so it lives in SGPRs (one v_fma instead of v_mov + v_fmac with a literal)
  uint32_t tune[4];           // wave kernel: [0] max TRAV steps per scheduling round, [1] leave-TRAV population floor in 1/16ths
  // work stealing on small shards (rl_rtiow_wave.h STEAL instantiation): a wave whose lanes have all run out of pixels takes over pixels
  // other lanes are still rendering, at a sample boundary, and continues them with the cooperative one-wave-per-pixel body.
  // steal_state[pix]: 0 queued / running, 1 take-over requested, 2 released (P.out, pos_state and steal_n hold the state), 3 finished
  uint32_t *steal_state, *steal_n, *steal_counter;
  const float *coop_leaf_boxes;  // ... the spheres' padded leaf boxes, which that body scans (rl_rtiow_coop.h)
  uint32_t *pix_rays;         // debug (tools/): per-pixel ray counts, accumulated at pixel end by the counting wave kernel, or null
  unsigned long long *stats;  // [0]=rays [1]=node_tests [2]=sphere_tests [3]=planar [4]=instance [5]=rng_words [6]=flagged
  // (appended last: the by-value kernels' kernarg offsets of everything above stay where they were)
  const uint32_t *fg_seg_roots;  // rl_rtiow_fastgen.h MEDIA: root entry of every program segment (FastGeneral::seg_roots)
  const FastMedium *fg_media;    // ... and the media between them
  uint32_t fg_n_seg;
  uint32_t fg_top;  // the first fg_top nodes of fg_nodes (the tree's top, breadth first) are copied into LDS by every workgroup (0: none)
  // sample-parallel mode (INDEP instantiations, rl_rtiow_render_independent*): a slot is (sample group, pixel); groups of indep_k samples,
  // sample-major (slot / indep_tile_slots = group); each sample's colour goes to indep_buf[sample - sample_begin][nrows * W][3]
  double *indep_buf;
  uint32_t indep_k, indep_tile_slots;
  // fast traversal (LDS_SCENE = 4): per-pixel entry words of this render's camera rays, [nrows * W] (rl_pixel_entry.h); null: every ray starts at fast_root
  const uint32_t *pixel_entry;
  // ray-buffer mode (RAYS instantiations, rl_rtiow_ray_color_rays*): a slot is one ray of the caller's batch, q_first + slot its index.
  // cam holds what the call gives instead of a camera: background and max_depth; key is expanded from the call's seed.
  const rl_ray *q_rays;
  const rl_rng_cursor *q_cursors;
  double *q_rgb;                  // [n][3]
  rl_rng_cursor *q_out_cursors;   // [n] or null
  uint32_t *q_ray_counts;         // [n] or null
  uint64_t q_first;
  // pixel-list mode (PIXELS instantiations, rl_rtiow_render_pixels*): a slot is element i of the caller's list, pixel (pix_xs[i], pix_ys[i]) of
  // the whole frame (row_first = 0, row_step = 1); its sums go to out[i], never to out[y * W + x].  n_slots = the list's length.
  const uint32_t *pix_xs, *pix_ys;
  // second moments (MOMENTS instantiations, rl_rtiow_render_moments* / rl_rtiow_render_pixels_moments*): per channel the
  // sum of the squared sample colours, laid out as `out` and stored / re-loaded wherever `out` is.  Read by no other instantiation.
  // (appended last, as everything since `stats`: the by-value kernels' kernarg offsets of everything above stay where they were)
  double *out_sq;
  // adaptive renders (rl_rtiow_render_adaptive*; a runtime mode of the MOMENTS frame kernels): out_count non-null = a pixel
  // stops at the first checkpoint of `adapt` that rtiow_adaptive_stop (rl_rtiow_adaptive.h) accepts, and its sample count goes to
  // out_count[pix], laid out as the pixels of `out`.  adapt_total = the call's samples_per_pixel, whatever [sample_begin, sample_end) this
  // launch renders.  Null: today's moments render.  Read by no other instantiation.
  uint32_t *out_count;
  rl_rtiow_adaptive adapt;
  uint32_t adapt_total;
  // wave kernels (rl_rtiow_wave.h Ring::coop_blocks): non-zero = thin block passes run four lanes to a block and FILL generates wave-wide;
  // 0 (RL_COOP_QUAD=0) = lane-per-block passes only, FILL per lane.  Same blocks in the same ring slots either way.
  uint32_t coop_quad;
  // wave kernels' SHADE: beside sphere_flat, one 32-byte record per sphere — the odd colour and inv_scale of a Checker of two Solid colours
  // (MAT_TEX_CHECKER; zeros otherwise), fetched by sphere index in the same round trip as the flattened material
  const DevChecker *sphere_checker;
  // fast traversal: the entry words by time slice, [nrows * W][1 << pixel_entry_log2t] (rl_pixel_entry.h, time slices): a camera ray takes the
  // word of its pixel and of the slice its time falls into.  Null: the one word of pixel_entry.
  const uint32_t *pixel_entry_t;
  uint32_t pixel_entry_log2t;
};

// MOMENTS, the compile-time flavour of the chained render kernels that keeps second moments (P.out_sq), is `false` in every kernel without
// it — spelled as a value that DEPENDS on a template parameter.  The bodies add a sample's colour under `if constexpr (MOMENTS) { name it,
// add it, add its square } else { the statement the kernel has always had }`, and only a dependent condition makes the first branch a
// discarded statement: nothing in it is instantiated, and the lambdas it stands in do not capture sq.  Measured with a plain `false` (and
// with the colour named in both flavours): the headline kernel <1024, 4, false> came out with another register assignment (or three
// instructions shorter), rtiow_fast_general_rays_kernel<768, 20, false, false> with one more spilled VGPR — and they stay exactly what they were.
template <int>
constexpr bool never_v = false;

// RAYS: the path's colour, the cursor behind it and its ray count to the ray's own index
__device__ __forceinline__ void rtiow_rays_store(const RtiowParams &P, uint64_t idx, const D3 &c, uint64_t stream, uint32_t pos, uint32_t rays) {
  double *b = P.q_rgb + idx * 3;
  b[0] = c.x, b[1] = c.y, b[2] = c.z;
  if (P.q_out_cursors) {
    uint64_t *q = (uint64_t *)(P.q_out_cursors + idx);
    q[0] = stream, q[1] = (uint64_t)pos;
  }
  if (P.q_ray_counts) P.q_ray_counts[idx] = rays;
}

// INDEP: the colour of sample `rel` (relative to the pass's sample_begin) of shard pixel (pr, px) into the pass buffer
__device__ __forceinline__ void rtiow_indep_store(const RtiowParams &P, uint32_t rel, uint32_t pr, uint32_t px, const D3 &c) {
  const size_t W = P.cam.image_width;
  double *b = P.indep_buf + ((size_t)rel * ((size_t)P.nrows * W) + (size_t)pr * W + px) * 3;
  b[0] = c.x, b[1] = c.y, b[2] = c.z;
}

// The ordered fold of one pass: out = (((A + c_0) + c_1) + ... ) + c_{np-1} per component, left to right, A = out (accumulate) or 0.0.
// (No special case for the first sample: 0.0 + c is what Canvas::merge of a fresh canvas computes, -0.0 included.)
__global__ void rtiow_indep_fold(double *__restrict__ out, const double *__restrict__ buf, unsigned long long n_vals, uint32_t np, uint32_t accumulate) {
  const unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_vals) return;
  double acc = accumulate ? out[i] : 0.0;
  for (uint32_t p = 0; p < np; p++) acc = acc + buf[(size_t)p * n_vals + i];
  out[i] = acc;
}

// ---------------------------------------------------------------- ChaCha8
__device__ __forceinline__ uint32_t rotl32(uint32_t x, int r) { return __builtin_rotateleft32(x, r); }

#define RL_QR(a, b, c, d)   \
  a += b, d ^= a, d = rotl32(d, 16); \
  c += d, b ^= c, b = rotl32(b, 12); \
  a += b, d ^= a, d = rotl32(d, 8);  \
  c += d, b ^= c, b = rotl32(b, 7);

// Generates block (key, ctr, stream) and stores its 16 words as 8 u64 into the lane's LDS column.
// ROLLED: the four double rounds as a loop (a quarter of the code).  A block is ~420 instructions (2 KB) unrolled, and inlined at every
// gen_f64 call site the copies made up half of the wave kernels' code — 37 of the 77 KB of the stealing instantiation, more than the 64 KB
// instruction cache two CUs share.  The wave-scheduled kernels (rl_rtiow_wave.h Ring) use the rolled form everywhere: main kernel 7292 ->
// 4728 instructions and no spills left, stealing instantiation 13943 -> 8986 and 38 -> 6 spilled VGPRs; 6709 -> 6770 Mrays/s, 1/8 shard
// 174 -> 163 ms.  The cooperative one-wave-per-pixel body keeps the unrolled form: there a block is on the pixel's critical path.
// (A real function call for the rare mid-SHADE refill was measured too: its register convention spills 36 more VGPRs in the main loop, 4940 Mrays/s.)
// (chacha8_block_to_lds_job: the same block function with its inputs {counter, stream, destination} produced by `job()`, which it
// calls twice — before the rounds and again for the feed-forward and the stores — so that a job that can re-derive its inputs
// cheaply (rl_rtiow_wave.h Ring::coop_blocks: a few lane permutes) does not hold them in registers through the rounds; a lane
// whose job has store = false computes a block and discards it)
struct ChachaJob {
  uint32_t ctr_lo;
  uint64_t stream;
  unsigned long long *s_rng;
  int tid;
  bool store;
};
template <int NT, bool ROLLED, class Job>
__device__ __forceinline__ void chacha8_block_to_lds_job(const uint32_t *key, Job job) {
  const uint32_t c0 = 0x61707865u, c1 = 0x3320646eu, c2 = 0x79622d32u, c3 = 0x6b206574u;
  const ChachaJob in = job();
  uint32_t x0 = c0, x1 = c1, x2 = c2, x3 = c3, x4 = key[0], x5 = key[1], x6 = key[2], x7 = key[3], x8 = key[4], x9 = key[5], x10 = key[6],
           x11 = key[7], x12 = in.ctr_lo, x13 = 0u, x14 = (uint32_t)in.stream, x15 = (uint32_t)(in.stream >> 32);
#pragma unroll(ROLLED ? 1 : 4)
  for (int r = 0; r < 4; r++) {
    RL_QR(x0, x4, x8, x12) RL_QR(x1, x5, x9, x13) RL_QR(x2, x6, x10, x14) RL_QR(x3, x7, x11, x15)
    RL_QR(x0, x5, x10, x15) RL_QR(x1, x6, x11, x12) RL_QR(x2, x7, x8, x13) RL_QR(x3, x4, x9, x14)
  }
  const ChachaJob j = job();
  x0 += c0, x1 += c1, x2 += c2, x3 += c3;
  x4 += key[0], x5 += key[1], x6 += key[2], x7 += key[3], x8 += key[4], x9 += key[5], x10 += key[6], x11 += key[7];
  x12 += j.ctr_lo, x14 += (uint32_t)j.stream, x15 += (uint32_t)(j.stream >> 32);
  unsigned long long *s_rng = j.s_rng;
  const int tid = j.tid;
  if (!j.store) return;
  s_rng[0 * NT + tid] = (unsigned long long)x0 | ((unsigned long long)x1 << 32);
  s_rng[1 * NT + tid] = (unsigned long long)x2 | ((unsigned long long)x3 << 32);
  s_rng[2 * NT + tid] = (unsigned long long)x4 | ((unsigned long long)x5 << 32);
  s_rng[3 * NT + tid] = (unsigned long long)x6 | ((unsigned long long)x7 << 32);
  s_rng[4 * NT + tid] = (unsigned long long)x8 | ((unsigned long long)x9 << 32);
  s_rng[5 * NT + tid] = (unsigned long long)x10 | ((unsigned long long)x11 << 32);
  s_rng[6 * NT + tid] = (unsigned long long)x12 | ((unsigned long long)x13 << 32);
  s_rng[7 * NT + tid] = (unsigned long long)x14 | ((unsigned long long)x15 << 32);
}
// Four lanes to a block (rl_rtiow_wave.h Ring::coop_blocks, a thin pass: at most a quarter of the wave's lanes have a job).  Lane
// q = lane & 3 of a quad holds column q of the state, a = x[q], b = x[4 + q], c = x[8 + q], d = x[12 + q], so the column round is ONE
// quarter round per lane; the diagonal round is the same quarter round with rows b, c, d turned by 1, 2, 3 lanes inside the quad
// (DPP quad_perm, no LDS traffic), and turned back after it.  A double round is 24 + 6 instructions before the compiler folds turns into
// the adds and xors that read them, against 96 of the lane-per-block form: a pass costs about a third and serves 16 blocks instead of 64.
// MUST run with all four lanes of every quad enabled (the callers run it with full exec; a quad without a job computes and discards).
// `job()` as above, but called once; d_in is the lane's word of the last row: {counter, 0, stream low, stream high}[q].  Word w of the
// block goes where the lane-per-block form puts it: u64 slot w >> 1, half w & 1 of the requester's column `tid` in s_rng.
struct ChachaQuadJob {
  uint32_t q;     // lane & 3
  uint32_t d_in;  // input word 12 + q
  unsigned long long *s_rng;
  int tid;
  bool store;
};
template <int CTRL>
__device__ __forceinline__ uint32_t quad_perm(uint32_t v) {  // CTRL = s0 | s1 << 2 | s2 << 4 | s3 << 6: lane k of a quad reads lane s_k
  return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, CTRL, 0xF, 0xF, true);
}
template <int NT, bool ROLLED, class Job>
__device__ __forceinline__ void chacha8_quad_block_to_lds_job(const uint32_t *key, Job job) {
  auto column = [&](uint32_t q, uint32_t &a, uint32_t &b, uint32_t &c) {  // input words q, 4 + q, 8 + q
    // (the four words pass through an empty asm as scalars: a plain select of key[..] compiles to a VECTOR load from the kernel
    // arguments at a selected address, and plain constants are held in four VGPRs through the whole scheduler loop)
    auto sel4 = [&](uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3) {
      asm volatile("" : "+s"(w0), "+s"(w1), "+s"(w2), "+s"(w3));
      return (q & 2u) ? ((q & 1u) ? w3 : w2) : ((q & 1u) ? w1 : w0);
    };
    a = sel4(0x61707865u, 0x3320646eu, 0x79622d32u, 0x6b206574u);
    b = sel4(key[0], key[1], key[2], key[3]);
    c = sel4(key[4], key[5], key[6], key[7]);
  };
  // the job is derived ONCE and its four input words are held through the rounds for the feed-forward: with four state words instead of
  // sixteen the pass still needs eight registers fewer than the lane-per-block form, and a second derivation is a third of the pass
  const ChachaQuadJob j = job();
  uint32_t ia, ib, ic;
  column(j.q, ia, ib, ic);
  uint32_t a = ia, b = ib, c = ic, d = j.d_in;
#pragma unroll(ROLLED ? 1 : 4)
  for (int r = 0; r < 4; r++) {
    RL_QR(a, b, c, d)
    b = quad_perm<0x39>(b), c = quad_perm<0x4E>(c), d = quad_perm<0x93>(d);  // lane q now holds x[4 + (q+1)%4], x[8 + (q+2)%4], x[12 + (q+3)%4]
    RL_QR(a, b, c, d)
    b = quad_perm<0x93>(b), c = quad_perm<0x4E>(c), d = quad_perm<0x39>(d);
  }
  a += ia, b += ib, c += ic, d += j.d_in;
  if (!j.store) return;
  uint32_t *w = (uint32_t *)(j.s_rng + (size_t)(j.q >> 1) * NT + j.tid) + (j.q & 1u);  // word q; word 4 i + q is 2 i slots on
  w[0 * 4 * NT] = a;
  w[1 * 4 * NT] = b;
  w[2 * 4 * NT] = c;
  w[3 * 4 * NT] = d;
}
template <int NT, bool ROLLED = false>
__device__ __forceinline__ void chacha8_block_to_lds(const uint32_t *key, uint32_t ctr_lo, uint64_t stream, unsigned long long *s_rng, int tid) {
  chacha8_block_to_lds_job<NT, ROLLED>(key, [&] { return ChachaJob{ctr_lo, stream, s_rng, tid, true}; });
}

// per-lane RNG state: stream + word position; the current block lives in LDS
struct Rng {
  uint64_t stream;
  uint32_t pos;      // u32 word position since the pixel started (set_stream keeps it, camera.rs:170)
  uint32_t buf_ctr;  // block counter of the block held in LDS, 0xFFFFFFFF = none
};

template <int NT>
struct RngCtx {
  const uint32_t *key;
  unsigned long long *s_rng;
  int tid;
  __device__ __forceinline__ uint64_t next_u64(Rng &r) const {
    uint32_t ctr = r.pos >> 4;
    if (ctr != r.buf_ctr) {
      chacha8_block_to_lds<NT>(key, ctr, r.stream, s_rng, tid);
      r.buf_ctr = ctr;
    }
    uint64_t v = s_rng[((r.pos & 15u) >> 1) * NT + tid];
    r.pos += 2;
    return v;
  }
  // rand 0.8.5 Standard for f64: 53 random bits * 2^-53
  __device__ __forceinline__ double gen_f64(Rng &r) const { return (double)(next_u64(r) >> 11) * 0x1.0p-53; }
  // rand 0.8.5 Uniform::new(-1.0, 1.0): (value1_2 - 1.0) * scale + low, scale = 2
  __device__ __forceinline__ double uniform_m1_1(Rng &r) const {
    double v = __longlong_as_double((long long)((next_u64(r) >> 12) | 0x3FF0000000000000ull));
    return (v - 1.0) * 2.0 + (-1.0);
  }
  // rand_distr 0.4.3 UnitSphere (Marsaglia 1972): reject s >= 1
  __device__ __forceinline__ D3 unit_sphere(Rng &r) const {
    for (;;) {
      double x1 = uniform_m1_1(r), x2 = uniform_m1_1(r);
      double s = x1 * x1 + x2 * x2;
      if (s >= 1.0) continue;
      double f = 2.0 * sqrt(1.0 - s);
      return D3{x1 * f, x2 * f, 1.0 - 2.0 * s};
    }
  }
  // rand_distr 0.4.3 UnitDisc: accept s <= 1
  __device__ __forceinline__ void unit_disc(Rng &r, double &a, double &b) const {
    for (;;) {
      a = uniform_m1_1(r);
      b = uniform_m1_1(r);
      if (a * a + b * b <= 1.0) return;
    }
  }
};

// ---------------------------------------------------------------- AABB (aabb.rs:123-152)
__device__ __forceinline__ void intersect_axis(double mn, double mx, double origin, double speed, double &lo, double &hi) {
  double t0 = (mn - origin) / speed;
  double t1 = (mx - origin) / speed;
  bool lt = t0 < t1;
  lo = lt ? t0 : t1;
  hi = lt ? t1 : t0;
}
__device__ __forceinline__ bool aabb_hit(const double *b, D3 o, D3 d, double tmin_, double tmax_) {
  double xl, xh, yl, yh, zl, zh;
  intersect_axis(b[0], b[1], o.x, d.x, xl, xh);
  intersect_axis(b[2], b[3], o.y, d.y, yl, yh);
  intersect_axis(b[4], b[5], o.z, d.z, zl, zh);
  // f64::max / f64::min ignore NaN == fmax / fmin
  double tmin = fmax(fmax(fmax(xl, yl), zl), tmin_);
  double tmax = fmin(fmin(fmin(xh, yh), zh), tmax_);
  return tmin < tmax;
}

struct Hit {  // what the traversal keeps: enough to rebuild the HitRecord afterwards
  double t;
  uint32_t prim;  // sphere payload (index | SPH_MOVING) or NONE
};

// Sphere::hit (sphere.rs:32-75). Updates `h` when the sphere is hit inside [tmin, h.t]; returns true
// if the reference's NormalizedVec3::from_normalized assert (vec3.rs:219-222) would have fired.
__device__ __forceinline__ bool sphere_hit(const DevSphere &s, uint32_t payload, D3 o, D3 d, double time, double tmin, Hit &h) {
  D3 c0 = ld3(s.c0);
  D3 center = (payload & SPH_MOVING) ? c0 + ld3(s.dc) * time : c0;  // sphere.rs:24-29
  D3 oc = o - center;
  double a = len2(d);
  double half_b = dot(oc, d);
  double c = len2(oc) - s.r2;
  double disc = half_b * half_b - a * c;
  if (disc < 0.0) return false;
  double sq = sqrt(disc);
  double r_l = (-half_b - sq) / a;
  double r_u = (-half_b + sq) / a;
  double t;
  if (tmin <= r_l && r_l <= h.t) t = r_l;
  else if (tmin <= r_u && r_u <= h.t) t = r_u;
  else return false;
  h.t = t;
  h.prim = payload;
  D3 p = o + d * t;
  D3 outward = (p - center) * s.inv_r;
  double l2 = len2(outward);
  return !(l2 == 1.0 || fabs(l2 - 1.0) <= 1e-5);
}

// Rust `f64 as i32`: saturating, NaN -> 0
__device__ __forceinline__ int f64_as_i32(double x) {
  return x != x ? 0 : (x >= 2147483647.0 ? 2147483647 : (x <= -2147483648.0 ? (int)(-2147483647 - 1) : (int)x));
}

// perlin.rs:39-66,101-125: Perlin::noise = trilinear Hermite blend of dot(randvec[hash], offset) over the cell's 8 corners
__device__ __forceinline__ double perlin_noise(const rl_perlin &pn, D3 p) {
  double fx = floor(p.x), fy = floor(p.y), fz = floor(p.z);
  double u = p.x - fx, v = p.y - fy, w = p.z - fz;
  uint32_t i = (uint32_t)f64_as_i32(fx), j = (uint32_t)f64_as_i32(fy), k = (uint32_t)f64_as_i32(fz);
  double uu = u * u * (3.0 - 2.0 * u);
  double vv = v * v * (3.0 - 2.0 * v);
  double ww = w * w * (3.0 - 2.0 * w);
  double accum = 0.0;
  // deliberately NOT unrolled: eight live corner vectors cost the all-primitives kernels ~70 VGPRs (and with them their
  // occupancy or scratch spills); one corner at a time accumulates in the reference's order just the same
#pragma unroll 1
  for (uint32_t di = 0; di < 2; di++)
#pragma unroll 1
    for (uint32_t dj = 0; dj < 2; dj++)
#pragma unroll 1
      for (uint32_t dk = 0; dk < 2; dk++) {
        uint32_t h = pn.perm_x[(i + di) & 255u] ^ pn.perm_y[(j + dj) & 255u] ^ pn.perm_z[(k + dk) & 255u];
        D3 c = ld3(pn.randvec[h & 255u]);
        double i_f = (double)di, j_f = (double)dj, k_f = (double)dk;
        D3 weight_v = d3(u - i_f, v - j_f, w - k_f);
        accum += (i_f * uu + (1.0 - i_f) * (1.0 - uu)) * (j_f * vv + (1.0 - j_f) * (1.0 - vv)) * (k_f * ww + (1.0 - k_f) * (1.0 - ww)) * dot(c, weight_v);
      }
  return accum;
}

// perlin.rs:68-80
__device__ __forceinline__ double perlin_turb(const rl_perlin &pn, D3 p, uint32_t depth) {
  double accum = 0.0, weight = 1.0;
  D3 temp_p = p;
#pragma unroll 1
  for (uint32_t it = 0; it < depth; it++) {
    accum += weight * perlin_noise(pn, temp_p);
    weight *= 0.5;
    temp_p = temp_p * 2.0;
  }
  return fabs(accum);
}

// sphere.rs:91-99 get_sphere_uv (acos / atan2 are the device libm's: colour-only)
__device__ __forceinline__ void sphere_uv(D3 p, double &u, double &v) {
  const double PI = 3.14159265358979323846;
  double theta = acos(-p.y);
  double phi = atan2(-p.z, p.x) + PI;
  u = phi / (2.0 * PI);
  v = theta / PI;
}

// texture.rs: value(u, v, p).  MODE 0 = Solid / Checker only (the sphere-only kernels: scenes with Image / Noise textures
// are routed to the all-primitives kernels by rl_rtiow_render_device), 1 = + Image, 2 = + Noise.  The branches are
// compiled out, not just skipped: sin() and the Perlin code cost the kernels that carry them ~70 VGPRs.
template <int MODE = 0>
__device__ __forceinline__ D3 texture_value(const RtiowParams &P, uint32_t tex, double u, double v, D3 p) {
  for (int guard = 0; guard < 64; guard++) {
    const DevTexture &t = P.textures[tex];
    if (t.kind == RL_TEX_SOLID) return ld3(t.color);
    if (t.kind == RL_TEX_CHECKER) {  // texture.rs:41-55
      // floor() as i64, saturating, summed wrapping (the release build; a debug build panics on the overflow); Rust's % keeps the
      // sign, so `sum % 2 == 0` asks for the low bit alone
      uint32_t odd = f64_as_i64_low_bit(floor(p.x * t.inv_scale)) ^ f64_as_i64_low_bit(floor(p.y * t.inv_scale)) ^
                     f64_as_i64_low_bit(floor(p.z * t.inv_scale));
      tex = odd ? t.odd : t.even;
      continue;
    }
    if (MODE == 0) return D3{0.0, 0.0, 0.0};
    if (MODE == 2 && t.kind == RL_TEX_NOISE) {  // texture.rs:84-94: Color(0.5,0.5,0.5) * (1 + sin(scale * p.z + 10 * turb(p, 7)))
      double sv = 1.0 + sin(t.inv_scale * p.z + 10.0 * perlin_turb(P.perlins[t.image], p, 7u));
      return D3{0.5 * sv, 0.5 * sv, 0.5 * sv};
    }
    // RL_TEX_IMAGE (texture.rs:62-82): nearest texel, f32 linear RGB
    const DevImage &im = P.images[t.image];
    double uu = u < 0.0 ? 0.0 : (u > 1.0 ? 1.0 : u);
    double vc = v < 0.0 ? 0.0 : (v > 1.0 ? 1.0 : v);
    double vv = 1.0 - vc;
    double fi = uu * (double)(im.width - 1), fj = vv * (double)(im.height - 1);
    uint32_t i = !(fi > 0.0) ? 0u : (fi >= 4294967295.0 ? 4294967295u : (uint32_t)fi);
    uint32_t j = !(fj > 0.0) ? 0u : (fj >= 4294967295.0 ? 4294967295u : (uint32_t)fj);
    const float *px = P.image_pool + im.offset + ((size_t)j * im.width + i) * 3;
    return D3{(double)px[0], (double)px[1], (double)px[2]};
  }
  return D3{0.0, 0.0, 0.0};
}

}  // namespace rl
