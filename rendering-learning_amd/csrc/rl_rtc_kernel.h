// RTC hot path on gfx950: Camera::render / rays_for_pixel (scene/camera.rs:63-124), World::color_at
// (world.rs:89-102), World::intersect + hit (world.rs:46-55, intersect.rs:159-172), Transformed /
// Bounded / Group / Triangle intersect (object/{transformed,bounded,group,triangle}.rs),
// prepare_computations (intersect.rs:48-115), shade_hit + shadow_attenuation (world.rs:57-126).
// lighting (material.rs:54-90) is rtc_lighting of rl_rtc_shading.h, the function the full kernel and the
// shading queries call; this kernel's prepare_computations is its own text (no under_point, no reflect_v:
// neither is read here, and the shared function's reflect_v fallback counts `flagged`).
//
// The reference gathers every intersection into a Vec, stable-sorts by t and picks the lowest t >= 0
// with "later wins" on ties.  That selection equals a single pass in evaluation order that replaces
// the best hit whenever t >= 0 and t <= best.t — no list, no sort (the sorted list itself is only
// needed for refraction, which this kernel does not cover: scenes with reflective or transparent
// materials are rejected with RL_E_UNSUPPORTED at scene creation).
// One lane per pixel; the n x n anti-aliasing grid is summed in the reference's order.
#pragma once
#ifndef RL_KERNEL_ALIGN
// Every big kernel starts on a 64 KB boundary of the code object.  Measured (round 3): the stealing instantiation of rtiow_wave_kernel (77 KB of
// code: main loop + cooperative body, more than the 64 KB instruction cache two CUs share) ran the 1/8 shard in 174 or in 189 ms depending on
// nothing but where the linker happened to put it (0x...ad00 against 0x...d600 after unrelated kernels grew); aligned, the placement is fixed.
#define RL_KERNEL_ALIGN __attribute__((aligned(65536)))
#endif
#include "rl_device.h"
#include "rl_rtc_shading.h"  // mag, norm, reflect; rtc_lighting and the other pointwise steps of color_at

namespace rl {

struct RtcParams {
  const DevOp *ops;
  const DevTri *tris;
  const rl_rtc_transformed *xforms;
  const rl_rtc_material *materials;
  const rl_rtc_light *lights;
  const RtcGuard *guards;  // reject-only box trees of the ROP_TRIS ops (op.skip = root + 1), or null
  uint32_t n_guards;
  uint32_t n_ops, n_tris, n_xforms, n_lights;
  rl_rtc_camera cam;
  uint32_t aa;
  uint32_t row_first, row_step, nrows;
  double void_color[3];
  double *out;
  unsigned long long *stats;
};

// 4x4 (row-major) * point (w = 1) / vector (w = 0): 4-term sums accumulated from 0.0
// (math/matrix.rs:192-210, point.rs:89-96, vector.rs:115-122)
__device__ __forceinline__ D3 mul_point(const double *m, D3 p) {
  double o[3];
#pragma unroll
  for (int n = 0; n < 3; n++) {
    double sum = 0.0;
    sum += m[4 * n + 0] * p.x;
    sum += m[4 * n + 1] * p.y;
    sum += m[4 * n + 2] * p.z;
    sum += m[4 * n + 3] * 1.0;
    o[n] = sum;
  }
  return D3{o[0], o[1], o[2]};
}
__device__ __forceinline__ D3 mul_vec(const double *m, D3 p) {
  double o[3];
#pragma unroll
  for (int n = 0; n < 3; n++) {
    double sum = 0.0;
    sum += m[4 * n + 0] * p.x;
    sum += m[4 * n + 1] * p.y;
    sum += m[4 * n + 2] * p.z;
    sum += m[4 * n + 3] * 0.0;
    o[n] = sum;
  }
  return D3{o[0], o[1], o[2]};
}

struct RtcCounters {
  unsigned long long rays, nodes, tris, enters, flagged;
};

struct RtcHit {
  double t;
  uint32_t tri;  // NONE = no hit
  uint32_t pc;   // op index where it was found (scope test at ROP_EXIT)
  D3 normal;
};

// ---- reject-only binary32 box test for the guard trees (same error analysis as aabb_fast32 in rl_rtiow_wave.h, u = 2^-24):
// with inv32 = RN32(1/d), oi32 = RN32(o/d) each slab parameter is off by <= 3.2u|t| + 3.3u max|o/d|.  The Group of a mesh has
// no acceleration structure in the reference (every ray tests every triangle, group.rs); a triangle whose padded box the ray
// certainly misses inside the parameter range that can still matter ([0, best.t], shadow rays (0, distance)) certainly has no
// intersection the reference would keep, so its (binary64) test is skipped — the counter still counts it.
struct RtcAux32 {
  float invx, invy, invz, oix, oiy, oiz, slack;
};
__device__ __forceinline__ RtcAux32 rtc_aux32(D3 o, D3 d) {
  RtcAux32 r;
  double ix = 1.0 / d.x, iy = 1.0 / d.y, iz = 1.0 / d.z;
  r.invx = (float)ix, r.invy = (float)iy, r.invz = (float)iz;
  r.oix = (float)(o.x * ix), r.oiy = (float)(o.y * iy), r.oiz = (float)(o.z * iz);
  float m = fmaxf(fmaxf(fabsf(r.oix), fabsf(r.oiy)), fabsf(r.oiz));
  float imin = fminf(fminf(fabsf(r.invx), fabsf(r.invy)), fabsf(r.invz)), imax = fmaxf(fmaxf(fabsf(r.invx), fabsf(r.invy)), fabsf(r.invz));
  bool ok = imin >= 1e-30f && imax <= 1e30f && m <= 1e30f;                        // NaN compares false
  r.slack = ok ? fmaf(m, 9.5367431640625e-07f, 1e-30f) : __int_as_float(0x7F800000);  // 16u max|oi|, or +inf: never reject
  return r;
}
__device__ __forceinline__ bool guard_reject32(const float *b, const RtcAux32 &ra, float tbound) {
  float t0x = fmaf(b[0], ra.invx, -ra.oix), t1x = fmaf(b[1], ra.invx, -ra.oix);
  float t0y = fmaf(b[2], ra.invy, -ra.oiy), t1y = fmaf(b[3], ra.invy, -ra.oiy);
  float t0z = fmaf(b[4], ra.invz, -ra.oiz), t1z = fmaf(b[5], ra.invz, -ra.oiz);
  float tmin = fmaxf(fmaxf(fmaxf(fminf(t0x, t1x), fminf(t0y, t1y)), fminf(t0z, t1z)), 0.0f);
  float tmax = fminf(fminf(fminf(fmaxf(t0x, t1x), fmaxf(t0y, t1y)), fmaxf(t0z, t1z)), tbound);
  float thresh = fmaf(tmin + fabsf(tmax), 4.76837158203125e-07f, ra.slack);  // 8u(|tmin|+|tmax|) + slack
  return (tmin - tmax) > thresh;                                            // false for NaN / inf arithmetic
}

// One pass over the program. SHADOW=false: closest hit (lowest t >= 0, later wins).
// SHADOW=true: product of transparency over hits with 0 < t < distance (world.rs:104-126).
template <bool SHADOW>
__device__ __forceinline__ double rtc_traverse(const RtcParams &P, const DevOp *ops, const DevTri *tris, const RtcGuard *guards, D3 wo, D3 wd, double distance,
                                               RtcHit &best, RtcCounters &cnt) {
  D3 o = wo, d = wd;
  double atten = 1.0;
  uint32_t pc = 0;
  for (;;) {
    const DevOp &op = ops[pc];
    uint32_t code = op.code;
    if (code == ROP_END) break;
    if (code == ROP_TRIS) {
      uint32_t first = op.a, count = op.b;
      auto test_triangle = [&](uint32_t ti) {  // triangle.rs:63-101
        const DevTri &t = tris[ti];
        D3 e1 = ld3(t.e1), e2 = ld3(t.e2);
        D3 dir_cross_e2 = cross(d, e2);
        double det = dot(e1, dir_cross_e2);
        if (fabs(det) < 1e-8) return;
        double f = 1.0 / det;
        D3 p1_to_origin = o - ld3(t.p1);
        double u = f * dot(p1_to_origin, dir_cross_e2);
        if (!(0.0 <= u && u <= 1.0)) return;
        D3 origin_cross_e1 = cross(p1_to_origin, e1);
        double v = f * dot(d, origin_cross_e1);
        if (v < 0.0 || (u + v) > 1.0) return;
        double tt = f * dot(e2, origin_cross_e1);
        if (SHADOW) {
          if (tt > 0.0 && tt < distance) atten = atten * P.materials[t.material].transparency;
        } else if (tt >= 0.0 && !(best.t < tt)) {  // intersect.rs:159-168: `lowest.t < i.t ? lowest : i`
          best.t = tt;
          best.tri = ti;
          best.pc = pc;
          if (t.smooth) {
            D3 n = (ld3(t.n2) * u + ld3(t.n3) * v) + ld3(t.n1) * (1.0 - u - v);
            D3 nn;
            if (!norm(n, nn)) {
              cnt.flagged++;
              nn = d3(0.0, 0.0, 0.0);
            }
            best.normal = nn;
          } else
            best.normal = ld3(t.n1);
        }
      };
      if (guards && op.skip != 0u) {  // walk the reject-only box tree; its leaves come in triangle order, so ties resolve as in the loop
        cnt.tris += count;             // the reference tests every triangle of the group
        const RtcAux32 ax = rtc_aux32(o, d);
        uint32_t g = op.skip - 1u;
        const uint32_t gend = guards[g].skip;
        while (g < gend) {
          const RtcGuard &nd = guards[g];
          const float bx[6] = {nd.box[0], nd.box[1], nd.box[2], nd.box[3], nd.box[4], nd.box[5]};
          const uint32_t nskip = nd.skip, ntri = nd.tri;
          const float tbound = SHADOW ? (float)distance : (float)best.t;
          if (guard_reject32(bx, ax, tbound)) g = nskip;
          else if (ntri == NONE) g++;
          else {
            test_triangle(ntri);
            g = nskip;
          }
        }
      } else {
        for (uint32_t k = 0; k < count; k++) {
          cnt.tris++;
          test_triangle(first + k);
        }
      }
      pc++;
      continue;
    }
    if (code == ROP_BOUNDS) {  // bounded.rs:100-139: swap if tmin > tmax; pass iff tmin <= tmax; NaN-ignoring max/min
      cnt.nodes++;
      double lo[3], hi[3];
      const double oo[3] = {o.x, o.y, o.z}, dd[3] = {d.x, d.y, d.z};
#pragma unroll
      for (int a = 0; a < 3; a++) {
        double tmin = (op.box[2 * a] - oo[a]) / dd[a];
        double tmax = (op.box[2 * a + 1] - oo[a]) / dd[a];
        bool sw = tmin > tmax;
        lo[a] = sw ? tmax : tmin;
        hi[a] = sw ? tmin : tmax;
      }
      double tmin = fmax(fmax(lo[0], lo[1]), lo[2]);
      double tmax = fmin(fmin(hi[0], hi[1]), hi[2]);
      pc = (tmin <= tmax) ? pc + 1 : op.skip;
      continue;
    }
    if (code == ROP_ENTER) {  // transformed.rs:39-51: local ray = inverse * ray
      cnt.enters++;
      const rl_rtc_transformed &x = P.xforms[op.a];
      D3 no = mul_point(x.inverse, o), nd = mul_vec(x.inverse, d);
      o = no, d = nd;
      pc++;
      continue;
    }
    // ROP_EXIT: a = xform, skip = pc of the matching ENTER, b = offset into the enclosing-chain table (-> restore parent ray)
    {
      if (!SHADOW && best.tri != NONE && best.pc > op.skip) {  // hit found inside this scope: normal <- unit(inverse_transpose * n)
        const rl_rtc_transformed &x = P.xforms[op.a];
        D3 wn = mul_vec(x.inverse_transpose, best.normal), nn;
        if (!norm(wn, nn)) {
          cnt.flagged++;
          nn = best.normal;
        }
        best.normal = nn;
      }
      // parent-space ray: replay the enclosing ENTERs from the world ray (bit-identical to the first pass)
      o = wo, d = wd;
      uint32_t chain = op.b;  // ops index list encoded as a linked list: each ENTER op stores its parent ENTER pc in .b
      // walk outermost -> innermost: collect up to 8 parents
      uint32_t stack[8];
      int n = 0;
      while (chain != NONE && n < 8) {
        stack[n++] = chain;
        chain = ops[chain].b;
      }
      for (int i = n - 1; i >= 0; i--) {
        const rl_rtc_transformed &x = P.xforms[ops[stack[i]].a];
        D3 no = mul_point(x.inverse, o), nd = mul_vec(x.inverse, d);
        o = no, d = nd;
      }
      pc++;
      continue;
    }
  }
  return atten;
}

// LIST (rl_rtc_render_pixels*): the grid-stride index picks element idx of the caller's pixel list, (xs[idx], ys[idx]) of the
// whole frame, instead of pixel (idx / W, idx % W) of the shard; the colour goes to out[idx] either way.  An element outside the image is
// written as zeros and traces nothing.  Everything after ray generation is the frame's code.
template <int NT, bool LDS_SCENE>
__global__ void RL_KERNEL_ALIGN __launch_bounds__(NT) rtc_kernel(RtcParams P) {
  constexpr bool LIST = false;
  const uint32_t *const xs = nullptr, *const ys = nullptr;
  const uint64_t n_list = 0;
#include "rl_rtc_render_body.inc"
}
template <int NT, bool LDS_SCENE>
__global__ void RL_KERNEL_ALIGN __launch_bounds__(NT) rtc_pixels_kernel(RtcParams P, const uint32_t *xs, const uint32_t *ys, uint64_t n_list) {
  constexpr bool LIST = true;
#include "rl_rtc_render_body.inc"
}

}  // namespace rl
