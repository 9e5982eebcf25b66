// RTIOW sphere/BVH kernel, wave-scheduled form ("v2").
//
// Same arithmetic and same per-pixel / per-sample / per-ray order as the reference (and as the nested-loop
// kernel of rl_rtiow_general.h), different *schedule*: each lane is a small state machine
//     GEN  (claim pixel / start next sample: new ChaCha stream, camera ray)
//     TRAV (ONE box op of the threaded scene program per step)
//     LEAF (the 1-2 Sphere::hit tests of a BVH leaf whose box passed)
//     FILL (top the lane's ChaCha ring up by one block)
//     SHADE(miss -> background; hit -> rebuild HitRecord, scatter, next ray)
// and the 64-wide wave repeatedly runs the state that has the most lanes waiting in it.  A lane
// whose path ends starts its pixel's next sample at once (path regeneration; legal because the
// per-pixel sample order is preserved), so no lane idles while another finishes a long path, and
// ChaCha block generation always runs for many lanes at once instead of lane-by-lane inside
// rejection loops.
//
// AABB test: the reference divides six times per box ((min-o)/d, (max-o)/d per axis, aabb.rs:143-152).
// Here each ray carries inv = 1.0/d (three IEEE divisions per ray) and oi = o*inv, and a box test uses
// t'' = fma(b, inv, -oi), one instruction per bound.  The DECISION tmin < tmax is taken from the
// approximations only when |tmax''-tmin''| exceeds a rigorous error margin (see RayAux); otherwise — and for non-finite boxes or rays with a zero / tiny / huge
// direction component — the lane re-evaluates the reference's exact divisions.  Decisions are
// therefore bit-identical to the reference (tests assert equal AABB/sphere/ray/RNG-word counters).
#pragma once
#include <type_traits>

#include "rl_rtiow_kernel.h"
#include "rl_rtiow_adaptive.h"  // the adaptive renders' stopping rule, the one statement
#include "rl_pixel_entry.h"     // time_slice: which of its pixel's entry words a camera ray takes; the instrumented kernel's census repeats the table's tests

namespace rl {

// (RL_PK_FMA, the lo / hi slab test's plane pairs as v_pk_fma_f32, went with that form of the step: measured 6750 -> 6600 Mrays/s — the
// broadcast operand pairs cost moves, one VGPR spilled)
#ifndef RL_SPLIT_LEAF
#define RL_SPLIT_LEAF false
#endif
// GEN's stream resets through Ring::coop_blocks: 0 = per lane, two blocks one after the other (the old path); 1 = one wave-wide pass;
// 2 = as 1, and lanes waiting in FILL take the pass's spare job slots (when that adds no pass): measured 775.6 against 774.0 ms per step, not kept
#ifndef RL_COOP_GEN
#define RL_COOP_GEN 1
#endif
// A/B: the unit-sphere draw of SHADE in at most this many tries per visit (0 = unbounded: the rejection loop runs to its end); a lane without
// an accepted draw stays in ST_SHADE and draws on at its next pick.  Measured and lost, like SPLIT_SHADE and SPLIT_LEAF (the extra SHADE
// visits thin the other blocks, and the colour's loads become a second round behind the draw): 483.2 ms per step unbounded, 534.5 with
// one try, 492.3 with two, the parent 494.4; 121 VGPRs in the headline kernel instead of 118 (profiles/shade_tail.txt section 7)
#ifndef RL_SHADE_TRIES
#define RL_SHADE_TRIES 0
#endif
// tools/wave_codegen.py finds the scheduler loop's header, its blocks and the TRAV step in a kernel's assembly by these comment lines (no code)
#define RL_CG_MARK(name) asm volatile("; rl_cg " name)
// (the scheduler states ST_GEN .. ST_LEAF2: rl_program.h, beside the successor words that encode them)

// two-block ChaCha ring in LDS: 16 u64 slots per lane, slot-major ([slot][lane]) => conflict-free
// ROLL_HOT: also the block generations on the hot paths (stream reset, FILL) use the rolled block function (rl_rtiow_kernel.h
// chacha8_block_to_lds<NT, true>); the refill in the middle of a SHADE block (rare: long rejection streaks) always does.
// ODD (the ray-buffer kernels, rl_rng_cursor): the word position may be odd — a caller's cursor may stand anywhere in the stream, and a
// draw is words pos, pos + 1 (rand_core BlockRng::next_u64), so an odd position reads the halves of two neighbouring u64 slots, the
// second one possibly in the next block.  A render's positions are always even: its kernels keep the plain form.
// QUAD = false: coop_blocks runs lane-per-block passes only, whatever the runtime switch says (an instantiation that would spill more
// with the four-lanes-per-block pass in it: rtiow_wave_moments_kernel<1024, 0>, rl_rtiow_wave_body.inc COOP_QUAD).
template <int NT, bool ROLL_HOT = true, bool ODD = false, bool QUAD = true>
struct Ring {
  const uint32_t *key;
  unsigned long long *s_rng;  // [16][NT]
  int tid;
  uint64_t stream;
  uint32_t pos;     // u32 word position within the pixel
  uint32_t blk_lo;  // lowest resident block counter
  uint32_t nres;    // resident blocks: blk_lo .. blk_lo+nres-1 (0..2); block c lives in half (c & 1)

  __device__ __forceinline__ void gen_block(uint32_t c) { chacha8_block_to_lds<NT, ROLL_HOT>(key, c, stream, s_rng + (size_t)(c & 1u) * 8 * NT, tid); }
  __device__ __forceinline__ void reset_stream(uint64_t s) {  // set_stream keeps pos; both resident blocks become stale
    stream = s;
    blk_lo = pos >> 4;
#pragma unroll 1
    for (uint32_t k = 0; k < 2u; k++) gen_block(blk_lo + k);  // (rolled: one copy of the block function's 2 KB, not two)
    nres = 2;
  }
  __device__ __forceinline__ bool low() const {  // reading from the newest block
    // ODD too goes by the draw's FIRST word: top_up drops the oldest block, and at pos = 16 b + 15 with blocks b, b + 1 resident that is
    // the block of the draw's first word (going by the second word, b + 1, dropped it, and the draw then took its low half from the
    // stale slot: seen only where a colour depends continuously on the path, e.g. a Noise texture after a medium's 2-word draw).  The
    // second word's block, when it is not resident yet, is generated by next_u64_any itself, which never drops the first word's.
    return (pos >> 4) >= blk_lo + nres - 1u;
  }
  __device__ __forceinline__ void top_up() {  // make block (newest+1) resident, dropping the oldest
    uint32_t c = blk_lo + nres;
    gen_block(c);
    top_up_done();
  }
  __device__ __forceinline__ void top_up_done() {  // bookkeeping of top_up once block (newest+1) is resident
    if (nres == 2) blk_lo++;
    else nres++;
  }
  // Wave-cooperative block generation (RL_COOP_GEN).  Called by ALL 64 lanes of the wave (full exec).  A lane with nb = 1 or 2 needs
  // blocks first .. first + nb - 1 of its `stream` in its own ring column.  The wave's requests become a job list — [every lane with
  // nb >= 1: block first][every lane with nb == 2: block first + 1] — and lane l runs job l (then l + 64) of it, writing the block
  // into the REQUESTER's column: 2 x 25 stream resets of a GEN block are one pass of the block function instead of two passes at
  // 40 % lane use.  Same blocks, same LDS slots as per-lane generation.  Cross-lane traffic is permutes only (no LDS allocation).
  // ONES: some lanes may want one block (else nb is 0 or 2 and one compaction serves both halves of the job list).
  // TWOS = false: no lane wants two (FILL: nb is 0 or 1, the job list is its first half only).
  // The pass plan (`quad`, wave-uniform: RtiowParams::coop_quad): full passes of 64 jobs, one lane per block, while more than
  // COOP_QUAD_MAX jobs are left, and the rest in quad passes of 16 jobs, four lanes per block (chacha8_quad_block_to_lds_job).  A
  // quad pass costs about a third of a full one (tools/wave_codegen.py prints both counts of the built kernel and the bound that
  // follows), so a remainder of up to two quad passes is cheaper than one more full pass.  quad = false: full passes only.
  static constexpr uint32_t COOP_QUAD_MAX = 32u;
  // Returns the passes it ran, full | quad << 16 (wave-uniform; the STATS census counts them, nothing else reads it).
  template <bool ONES, bool TWOS = true>
  __device__ __forceinline__ uint32_t coop_blocks(uint32_t nb, uint32_t first, bool quad) {
    const unsigned long long m1 = __ballot(nb != 0u), m2 = !TWOS ? 0ull : ONES ? __ballot(nb == 2u) : m1;
    const uint32_t n1 = (uint32_t)__popcll(m1), jobs = n1 + (uint32_t)__popcll(m2);
    // compaction (a forward permute): lane r receives the id of the r-th lane of mask m; the lanes outside it all send to lane 63,
    // which is then never read (it is the mask's last member only when all 64 lanes are in it)
    auto compact = [](unsigned long long m, uint32_t lane) {
      const uint32_t r = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
      return (uint32_t)__builtin_amdgcn_ds_permute((int)((((m >> lane) & 1ull) ? r : 63u) << 2), (int)lane);
    };
    __builtin_amdgcn_wave_barrier();  // every lane has finished reading the blocks about to be overwritten
    uint32_t j0 = 0;
    // the job of lane l: j0 + l in a full pass, j0 + (l >> 2) in a quad pass.  Requester, counter, stream and destination, all derived
    // from the wave-uniform masks and the lane id — in a full pass twice (chacha8_block_to_lds_job; the empty asm makes the second
    // derivation a new one), so that nothing but the block's 16 words is held through the rounds: the headline kernel stays within its
    // 128 VGPRs; a quad pass holds four words and derives once
    struct Derived {
      uint32_t lane, c, slo, shi;
      int tid;
      bool store;
    };
    auto derive = [&](uint32_t shift) {
      uint32_t lane = (uint32_t)tid & 63u;
      asm volatile("" : "+v"(lane));
      const uint32_t j = j0 + (lane >> shift);
      const bool second = TWOS && j >= n1;
      const int k4 = (int)((second ? j - n1 : j) << 2);
      uint32_t req = (uint32_t)__builtin_amdgcn_ds_bpermute(k4, (int)compact(m1, lane));
      if (ONES && TWOS) {
        const uint32_t r2 = (uint32_t)__builtin_amdgcn_ds_bpermute(k4, (int)compact(m2, lane));
        req = second ? r2 : req;
      }
      const int r4 = (int)((req & 63u) << 2);
      const uint32_t slo = (uint32_t)__builtin_amdgcn_ds_bpermute(r4, (int)(uint32_t)stream);
      const uint32_t shi = (uint32_t)__builtin_amdgcn_ds_bpermute(r4, (int)(uint32_t)(stream >> 32));
      const uint32_t c = (uint32_t)__builtin_amdgcn_ds_bpermute(r4, (int)first) + (second ? 1u : 0u);
      return Derived{lane, c, slo, shi, (tid & ~63) | (r4 >> 2), j < jobs};
    };
    const uint32_t quad_max = QUAD && quad ? COOP_QUAD_MAX : 0u;
    uint32_t passes = 0;
#pragma unroll 1
    for (; j0 + quad_max < jobs; j0 += 64u) {  // full passes while more than quad_max jobs are left (two of them: launch start, more than 64 blocks wanted)
      RL_CG_MARK("FULL_B");
      auto job = [&] {
        const Derived v = derive(0u);
        return ChachaJob{v.c, ((uint64_t)v.shi << 32) | v.slo, s_rng + (size_t)(v.c & 1u) * 8 * NT, v.tid, v.store};
      };
      chacha8_block_to_lds_job<NT, ROLL_HOT>(key, job);  // all 64 lanes (the permutes read from lanes that have no job)
      RL_CG_MARK("FULL_E");
      passes += 1u;
    }
#pragma unroll 1
    for (; QUAD && j0 < jobs; j0 += 16u) {  // the remainder of at most COOP_QUAD_MAX jobs (none without `quad`: the loop above has passed `jobs`)
      RL_CG_MARK("QUAD_B");
      auto job = [&] {
        const Derived v = derive(2u);
        const uint32_t q = v.lane & 3u;
        const uint32_t d_in = (q & 2u) ? ((q & 1u) ? v.shi : v.slo) : ((q & 1u) ? 0u : v.c);
        return ChachaQuadJob{q, d_in, s_rng + (size_t)(v.c & 1u) * 8 * NT, v.tid, v.store};
      };
      chacha8_quad_block_to_lds_job<NT, ROLL_HOT>(key, job);  // all 64 lanes: the quad permutes of the rounds need every quad whole
      RL_CG_MARK("QUAD_E");
      passes += 1u << 16;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    return passes;
  }
  __device__ __forceinline__ uint64_t next_u64() {
    if (ODD) return next_u64_any();
    uint32_t c = pos >> 4;
    if (__builtin_expect(c - blk_lo >= nres, 0)) {  // rare inline path (long rejection streaks): always the rolled block function, a quarter of the code per call site
      const uint32_t nc = blk_lo + nres;
      chacha8_block_to_lds<NT, true>(key, nc, stream, s_rng + (size_t)(nc & 1u) * 8 * NT, tid);
      if (nres == 2) blk_lo++;
      else nres++;
    }
    uint64_t v = s_rng[((size_t)(c & 1u) * 8 + ((pos & 15u) >> 1)) * NT + tid];
    pos += 2;
    return v;
  }
  // ODD: words pos, pos + 1 from any position.  An odd one takes the high half of its u64 slot and the low half of the next slot,
  // which may lie in the next block: residency is checked for the block of the draw's SECOND word (the first one's is resident).
  __device__ __forceinline__ uint64_t next_u64_any() {
    const uint32_t p1 = pos + (pos & 1u);
    const uint32_t c = p1 >> 4;
    if (__builtin_expect(c - blk_lo >= nres, 0)) {
      const uint32_t nc = blk_lo + nres;
      chacha8_block_to_lds<NT, true>(key, nc, stream, s_rng + (size_t)(nc & 1u) * 8 * NT, tid);
      if (nres == 2) blk_lo++;
      else nres++;
    }
    uint64_t v = s_rng[((size_t)((pos >> 4) & 1u) * 8 + ((pos & 15u) >> 1)) * NT + tid];
    if (pos & 1u) v = (v >> 32) | (s_rng[((size_t)(c & 1u) * 8 + ((p1 & 15u) >> 1)) * NT + tid] << 32);
    pos += 2;
    return v;
  }
  __device__ __forceinline__ double gen_f64() { return (double)(next_u64() >> 11) * 0x1.0p-53; }
  __device__ __forceinline__ double uniform_m1_1() {
    double v = __longlong_as_double((long long)((next_u64() >> 12) | 0x3FF0000000000000ull));
    return (v - 1.0) * 2.0 + (-1.0);
  }
  __device__ __forceinline__ D3 unit_sphere() {
    for (;;) {
      double x1 = uniform_m1_1(), x2 = uniform_m1_1();
      double s = x1 * x1 + x2 * x2;
      if (s >= 1.0) continue;
      double f = 2.0 * sqrt(1.0 - s);
      return D3{x1 * f, x2 * f, 1.0 - 2.0 * s};
    }
  }
  // unit_sphere() with the point formed BEHIND the loop, which only finds the accepted (x1, x2, s): the wave kernels' SHADE
  // (rl_rtiow_wave_body.inc).  Returned from inside the loop, the accepted draw's arithmetic (the correctly rounded sqrt's expansion:
  // 24 VALU instructions, 20 of them binary64) sits in the loop's accept branch, and a wave runs that branch in every iteration in which
  // any of its lanes accepts — about three times per SHADE block where once will do.  Same operations in the same order on the same
  // accepted values.  (The other kernels that draw from a Ring keep the form above: with this one some rtiow_fast_general instantiations
  // spill up to 8 more VGPRs, tools/kernel_regs.py.)
  __device__ __forceinline__ D3 unit_sphere_tail() {
    double x1, x2, s;
    do {
      x1 = uniform_m1_1(), x2 = uniform_m1_1();
      s = x1 * x1 + x2 * x2;
    } while (s >= 1.0);
    double f = 2.0 * sqrt(1.0 - s);
    return D3{x1 * f, x2 * f, 1.0 - 2.0 * s};
  }
  // unit_sphere_tail() in at most TRIES tries: false when none was accepted (the tried words are consumed; the caller draws on later)
  template <int TRIES>
  __device__ __forceinline__ bool unit_sphere_tries(D3 &out) {
    double x1 = 0.0, x2 = 0.0, s = 1.0;
#pragma unroll 1
    for (int k = 0; k < TRIES && s >= 1.0; k++) {
      x1 = uniform_m1_1(), x2 = uniform_m1_1();
      s = x1 * x1 + x2 * x2;
    }
    if (s >= 1.0) return false;
    double f = 2.0 * sqrt(1.0 - s);
    out = D3{x1 * f, x2 * f, 1.0 - 2.0 * s};
    return true;
  }
  __device__ __forceinline__ void unit_disc(double &a, double &b) {
    for (;;) {
      a = uniform_m1_1();
      b = uniform_m1_1();
      if (a * a + b * b <= 1.0) return;
    }
  }
};

// per-ray reciprocal + eligibility for the filtered AABB test
__device__ __forceinline__ bool ray_fast_ok(D3 o, D3 d) {
  auto okd = [](double v) { double a = fabs(v); return a >= 1e-100 && a <= 1e100; };
  auto oko = [](double v) { return fabs(v) <= 1e100; };
  return okd(d.x) && okd(d.y) && okd(d.z) && oko(o.x) && oko(o.y) && oko(o.z);
}

// Per-ray constants of the filtered AABB test.
//   inv = 1/d (IEEE), oi = o*inv, slack = 4u * max|oi|.
// A box test evaluates t'' = fma(b, inv, -oi) ~ (b-o)/d with ONE instruction per bound.  Against the
// reference's q^ = RN(RN(b-o)/d):  |t'' - q^| <= 4.1u|t''| + 1.1u|oi|  (u = 2^-53; three roundings in
// t'', two in q^, plus the cancellation term of b*inv - o*inv).  min/max commute with the relative part
// and are 1-Lipschitz in the absolute part, so |tmin'' - tmin| <= 4.2u|tmin''| + 1.1u max|oi| and the
// same for tmax: the decision is certain whenever |tmax''-tmin''| > 8u(|tmin''|+|tmax''|) + slack.
struct RayAux {
  D3 inv, oi;
  double slack;
  bool fast_ok;
};
__device__ __forceinline__ RayAux ray_aux(D3 o, D3 d) {
  RayAux a;
  a.inv = d3(1.0 / d.x, 1.0 / d.y, 1.0 / d.z);
  a.oi = d3(o.x * a.inv.x, o.y * a.inv.y, o.z * a.inv.z);
  a.slack = fmax(fmax(fabs(a.oi.x), fabs(a.oi.y)), fabs(a.oi.z)) * 4.4408920985006262e-16;  // 4u
  a.fast_ok = ray_fast_ok(o, d);
  return a;
}

// Filtered AABB::hit. tmin_ is the kernel constant 1e-10 (> 0), tmax_ the closest hit so far.
// `certain` = false: the caller must evaluate the reference's divisions (aabb_hit).
__device__ __forceinline__ bool aabb_fast(const double *b, const RayAux &ra, double tmax_, bool &certain, double k8u = 8.8817841970012523e-16) {
  const double tmin_ = 1e-10;
  double t0x = fma(b[0], ra.inv.x, -ra.oi.x), t1x = fma(b[1], ra.inv.x, -ra.oi.x);
  double t0y = fma(b[2], ra.inv.y, -ra.oi.y), t1y = fma(b[3], ra.inv.y, -ra.oi.y);
  double t0z = fma(b[4], ra.inv.z, -ra.oi.z), t1z = fma(b[5], ra.inv.z, -ra.oi.z);
  double tmin = fmax(fmax(fmax(fmin(t0x, t1x), fmin(t0y, t1y)), fmin(t0z, t1z)), tmin_);
  double tmax3 = fmin(fmin(fmax(t0x, t1x), fmax(t0y, t1y)), fmax(t0z, t1z)), tmax;
  // = fmin(tmax3, tmax_): v_min_f64 is IEEE minNum (quiets a signalling NaN itself); written as asm because the
  // compiler otherwise spends a v_max_f64 x,x canonicalisation on the loop-carried tmax_ in every step
  asm("v_min_f64 %0, %1, %2" : "=v"(tmax) : "v"(tmax3), "v"(tmax_));
  double diff = tmax - tmin;
  double thresh = fma(tmin + fabs(tmax), k8u, ra.slack);  // 8u(|tmin|+|tmax|) + slack
  certain = fabs(diff) > thresh;                                            // false also for NaN / inf arithmetic
  return diff > 0.0;
}

// Single-precision form of the filter, for LDS-resident ops whose box has been re-stored as six floats (round to nearest).
//   inv32 = RN32(1/d), oi32 = RN32(o * (1/d)), t'' = fmaf(b32, inv32, -oi32), everything in binary32, u = 2^-24.
// |b32*inv32 - b/d| <= 2.1u|b/d| <= 2.1u(|t| + |o/d|), |oi32 - o/d| <= 1.1u|o/d|, one more rounding in the fma, and the
// clamp closest32 = RN32(closest) moves tmax by <= u|tmax|: each end of [tmin, tmax] is off by <= 3.2u|t| + 3.3u max|o/d|.
// The decision tmin < tmax is therefore certain when |tmax''-tmin''| > 8u(|tmin''|+|tmax''|) + 16u max|oi32| (twice the
// bound, which also absorbs the roundings of this comparison itself); otherwise, and whenever anything is non-finite, the
// lane evaluates the reference's divisions in binary64.  About 1 test in 10^5 falls back.
struct RayAux32 {
  float invx, invy, invz, oix, oiy, oiz, slack;
  // ray_aux32_direct only: max_k |o_k / d_k|, the coordinate scale of this ray in units of t (slack = 24u * that; +inf stays +inf)
  __device__ __forceinline__ float oimax() const { return slack * 699050.6875f; }
};
__device__ __forceinline__ RayAux32 ray_aux32(const RayAux &a) {
  RayAux32 r;
  r.invx = (float)a.inv.x, r.invy = (float)a.inv.y, r.invz = (float)a.inv.z;
  r.oix = (float)a.oi.x, r.oiy = (float)a.oi.y, r.oiz = (float)a.oi.z;
  float m = fmaxf(fmaxf(fabsf(r.oix), fabsf(r.oiy)), fabsf(r.oiz));
  // the bound above needs every product and sum to stay a NORMAL binary32 number: 1/d within [1e-30, 1e30] and |o/d| <= 1e30
  // (a zero, denormal-scale or huge direction component, or a far-away origin, makes the lane use the exact path always)
  float imin = fminf(fminf(fabsf(r.invx), fabsf(r.invy)), fabsf(r.invz)), imax = fmaxf(fmaxf(fabsf(r.invx), fabsf(r.invy)), fabsf(r.invz));
  bool ok = a.fast_ok && imin >= 1e-30f && imax <= 1e30f && m <= 1e30f;  // NaN compares false
  r.slack = ok ? m * 9.5367431640625e-07f : __int_as_float(0x7F800000);  // 16u, or +inf: never certain
  return r;
}
__device__ __forceinline__ bool aabb_fast32(const float *b, const RayAux32 &ra, float closest32, bool &certain) {
  float t0x = fmaf(b[0], ra.invx, -ra.oix), t1x = fmaf(b[1], ra.invx, -ra.oix);
  float t0y = fmaf(b[2], ra.invy, -ra.oiy), t1y = fmaf(b[3], ra.invy, -ra.oiy);
  float t0z = fmaf(b[4], ra.invz, -ra.oiz), t1z = fmaf(b[5], ra.invz, -ra.oiz);
  float tmin = fmaxf(fmaxf(fmaxf(fminf(t0x, t1x), fminf(t0y, t1y)), fminf(t0z, t1z)), 1e-10f);
  float tmax = fminf(fminf(fminf(fmaxf(t0x, t1x), fmaxf(t0y, t1y)), fmaxf(t0z, t1z)), closest32);
  float diff = tmax - tmin;
  float thresh = fmaf(tmin + fabsf(tmax), 4.76837158203125e-07f, ra.slack);  // 8u(|tmin|+|tmax|) + slack
  certain = fabsf(diff) > thresh;                                            // false also for NaN / inf arithmetic
  return diff > 0.0f;
}

// Per-ray constants of the FAST traversal's reject-only test, computed in binary32 from the start (no binary64 division):
//   d32 = RN32(d), inv32 = v_rcp_f32(d32) (<= 1 ulp), o32 = RN32(o), oi32 = RN32(o32 * inv32), u = 2^-24.
// inv32 = (1/d)(1 + e), |e| <= 3u;  b32 * inv32 is off by <= 4u|b/d| <= 4u(|t| + |o/d|) (the node boxes are stored exactly, rounded
// OUTWARDS);  oi32 by <= 5u|o/d|;  one more rounding in the fma and the clamp closest32 = RN32(closest): each end of [tmin, tmax] is
// off by <= 6u|t| + 9u max|o/d|.  A box is therefore CERTAINLY missed when tmin'' - tmax'' > 12u(|tmin''| + |tmax''|) + 24u max|oi32|
// (the bound for both ends together, plus room for the roundings of this comparison itself).  Rays with a zero, denormal-scale or
// huge direction component or a far-away origin get slack = +inf: nothing is ever certain for them, and start_ray() sends them
// to the reference-order fold.
//
// The wave kernels' TRAV step (LDS_SCENE = 4) reads its boxes as centre c and half-extent h (FastNodeCH) and forms per axis
//   t_c'' = fma(c, inv32, -oi32),  t_near'' = fma(-h, |inv32|, t_c''),  t_far'' = fma(h, |inv32|, t_c''),
// tmin'' = max(t_near'' of the three axes, 1e-10f), tmax'' = min(t_far'' of the three, closest32), with the same decision.  The bound
// above does not carry over as it stands: it rests on every plane's t'' being off by a multiple of |t''| ITSELF (and of max|o/d|), which
// survives min and max, whereas t_near'' inherits the rounding of t_c'', a multiple of |t_c| that can be far larger than |t_near|.
// Per axis, with t_c = (c - o)/d, t_near = t_c - h/|d| (exact values for the STORED box) and oi32 = o32 inv32 (1 + e), |e| <= u:
//   c inv32 - oi32 = inv32 (c - o) + inv32 (o - o32) - o32 inv32 e: off from t_c by <= 3u|t_c| + 2.01u|o/d|, and <= u|t_c''| more in the fma;
//   h |inv32| is off from h/|d| by <= 3u h/|d|, and the second fma adds <= u|t_near''|:
//   |t_near'' - t_near| <= 4.01u|t_c| + 3u h/|d| + 2.01u|o/d| + u|t_near''| <= (4.01u|c| + 3u h)/|d| + 6.02u|o/d| + u|t_near''|
// by |t_c| <= |c|/|d| + |o/d|; the same for t_far''.  The first term is a length, (4.01u|c| + 3u h), over |d|: moving the slab's planes
// outwards by that length changes t_near and t_far by exactly that much.  So the host stores every box with c - h <= lo - delta and
// c + h >= hi + delta, delta = 8u(|c| + hi - lo) per node, child and axis (rl_fast_bvh.cpp fast_node_ch: twice the |c| term, five times
// the h term), where [lo, hi] is the FastNode's outward-rounded box, and then against the planes of [lo, hi] itself
//   t_near'' <= t_near[lo] + 6.02u max|o/d| + u|t_near''|,   t_far'' >= t_far[hi] - 6.02u max|o/d| - u|t_far''|:
// errors relative to the value itself again, which max and min preserve; the clamps 1e-10f and closest32 add u of themselves.  A ray
// that touches [lo, hi] inside [1e-10, closest] therefore has tmin'' - tmax'' <= 1.01u(|tmin''| + |tmax''|) + 12.04u max|o/d|, and the
// decision keeps its constants, 12u(|tmin''| + |tmax''|) + 24u max|oi32|: twice the per-ray part (max|oi32| >= (1 - 5u) max|o/d|) and
// far more than the relative part, with room for the roundings of the subtraction, of the threshold and of the comparison.  No
// per-ray constant is added.  As before all of this needs NORMAL binary32 results (an fma that underflows is off by <= 2^-126, far
// below 12u * 1e-10, the smallest threshold); an infinite or NaN t'' makes the comparison false, and the child is visited.
__device__ __forceinline__ RayAux32 ray_aux32_direct(D3 o, D3 d) {
  RayAux32 r;
  float dx = (float)d.x, dy = (float)d.y, dz = (float)d.z;
  r.invx = __builtin_amdgcn_rcpf(dx), r.invy = __builtin_amdgcn_rcpf(dy), r.invz = __builtin_amdgcn_rcpf(dz);
  r.oix = (float)o.x * r.invx, r.oiy = (float)o.y * r.invy, r.oiz = (float)o.z * r.invz;
  float m = fmaxf(fmaxf(fabsf(r.oix), fabsf(r.oiy)), fabsf(r.oiz));
  float imin = fminf(fminf(fabsf(r.invx), fabsf(r.invy)), fabsf(r.invz)), imax = fmaxf(fmaxf(fabsf(r.invx), fabsf(r.invy)), fabsf(r.invz));
  float omax = fmaxf(fmaxf(fabsf((float)o.x), fabsf((float)o.y)), fabsf((float)o.z));
  // every product and sum must stay a NORMAL binary32 number: 1/d within [1e-30, 1e30], |o| and |o/d| <= 1e30 (NaN compares false)
  bool ok = imin >= 1e-30f && imax <= 1e30f && m <= 1e30f && omax <= 1e30f;
  r.slack = ok ? m * 1.430511474609375e-06f : __int_as_float(0x7F800000);  // 24u, or +inf: never certain
  return r;
}
// The decision's threshold, the ONE statement of it: a box with tmax'' - tmin'' < -fast_miss_thresh is certainly missed.
__device__ __forceinline__ float fast_miss_thresh(const RayAux32 &ra32, float tmin, float tmax) {
  return fmaf(tmin + fabsf(tmax), 7.152557373046875e-07f, ra32.slack);  // 12u(|tmin|+|tmax|) + slack (ray_aux32_direct)
}
// Two accepted roots closer than this are treated as a tie (the ray is re-traced in the reference's order).  The reference's own
// decisions that involve two different primitives — `tmin < closest` on its boxes, `t <= closest` in Sphere::hit — compare values
// whose rounding errors are a few u (2^-53) times the SCALES involved: the far root of the sphere (cancellation in -half_b -+ sqrt),
// and the coordinates of origin and boxes over the direction (max |o/d|).  4e-12 is ~4e4 u.
__device__ __forceinline__ double fast_tie_band(double scale_t, float oimax) { return 4e-12 * (scale_t + (double)oimax); }

// LDS_SCENE: 0 = scene read from HBM / L2, 1 = linked ops + spheres staged in LDS, 2 = linked ops in LDS, spheres from L2,
// 3 = compact (32-byte) guarded ops in LDS (P.cops: the n_ops originals + one guard op per sphere), spheres from L2,
// 4 = FAST traversal (counter-free renders only): P.fast_nodes in LDS — see below
typedef __attribute__((address_space(3))) CompactOp LdsCompactOp;
typedef float Float4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) const Float4 LdsFloat4;
typedef __attribute__((address_space(3))) const uint32_t LdsU32;

// ---- FAST traversal (LDS_SCENE = 4).  The reference's fold over its BVH visits ~40 boxes and ~4.7 spheres per ray because its tree
// is a median split walked in stored order.  For the RESULT of the fold only the smallest accepted root matters (rl_fast_bvh.cpp), so
// the timed kernel walks its own surface-area-heuristic binary tree instead: one TRAV step fetches a 64-byte node with BOTH children's
// boxes, tests the two with the binary32 filter in reject-only form (a box is skipped only when it is CERTAINLY missed inside
// [1e-10, closest]), descends into the nearer child and pushes the farther one on a 16-entry stack held in five VGPRs (ten-bit entry
// ids, v_alignbit shifts) — ~12 steps and ~1.9 Sphere::hit per ray.  Whenever the visiting ORDER could influence the reference's answer
// the ray is flagged and re-traced by fast_slow_trace, the reference's own fold with exact divisions:
//   * two roots within a few 1e4 ulps of the scales involved (fast_tie_band; exact ties go to the LAST sphere in the reference's
//     order; `tmin < closest` pruning on the reference's boxes),
//   * a grazing hit (chord below 1e-6 relative: the reference's unpadded leaf box may or may not be passed), or a hit next to one
//     of the sphere's axis poles, where it touches its own box (fast_near_box_face),
//   * (a hit whose outward normal trips the from_normalized assert, vec3.rs:219, would make the panic-site count order dependent:
//     scenes in which that assert is reachable do not get a fast structure at all, rl_fast_bvh.cpp normals_safe),
//   * a ray outside the filter's range (zero / denormal-scale / huge direction component, far-away origin).
static const uint32_t FAST_SLOW = 0xFFFFFFFFu;  // pc of a lane in ST_LEAF that must re-trace its ray in the reference's order
// pc of a lane in ST_GEN whose walk ended without a hit: GEN adds thr * background and counts the sample before anything else it does.
// No walk can produce the value: a pc is an LDS address, an entry id below 1024, or FAST_SLOW.
static const uint32_t FAST_MISSED = 0xFFFFFFFEu;

// A sphere touches its own bounding box (and every ancestor box it is extremal in) at its six axis poles.  The ROUNDED root can sit a
// little past the point where the ray leaves that box — e.g. the self-intersection root ~1e-10 of a ray that starts on top of a huge
// ground sphere, whose cancellation error is as large as the root itself — and then the reference's exact slab test (aabb.rs:123-152)
// prunes a sphere that Sphere::hit would have accepted.  The hit is order-sensitive when its point is closer to a face of
// [centre - r, centre + r] than the root's error bound moves it along the ray.
// Bound on the error of Sphere::hit's rounded roots, in units of t: the discriminant carries ~16u a |oc|^2 of rounding (cancellation in
// |oc|^2 - r^2 and half_b^2 - a c), i.e. 8u |oc|^2 / sqrt(disc) in the root, plus a few u of the roots' magnitudes and of the coordinate
// scale max |o/d|; times 64.  (The tie band above is far wider; this one decides how close to a box face a hit may lie.)
__device__ __forceinline__ double fast_root_error(double len2_oc, double sq, double r_l, double r_u, float oimax) {
  float q = (float)len2_oc * __builtin_amdgcn_rcpf((float)sq);  // a tolerance: binary32 is plenty; sq = 0 -> +inf
  return 64.0 * (1.8e-15 * (double)q + 4.5e-16 * (fabs(r_l) + fabs(r_u) + (double)oimax));
}
__device__ __forceinline__ bool fast_near_box_face(D3 o, D3 d, double t, D3 center, double r, double band) {
  D3 q = (o + d * t) - center;
  return r - fabs(q.x) <= band * fabs(d.x) || r - fabs(q.y) <= band * fabs(d.y) || r - fabs(q.z) <= band * fabs(d.z);
}

// Grazing hits and hits next to an axis pole, for an ACCEPTED root t (rl_rtiow_fastgen.h: for the winning hit).  A binary32 pre-filter
// on what Sphere::hit has already computed lets all but ~3 hits in 10^4 skip the exact test: |q_k| < 0.9999 r for q = oc + t d (not
// within 1e-4 r of a face), sqrt(disc) > 1e-3 |d|_max r (not grazing), and the root's error bound below half of that 1e-4 r.
__device__ __forceinline__ bool fast_hit_is_order_sensitive(D3 oc, D3 d, double t, double r, double half_b, double sq, double r_l, double r_u, float oimax) {
  float dx = (float)d.x, dy = (float)d.y, dz = (float)d.z, t32 = (float)t, r32 = (float)r, sq32 = (float)sq;
  float ox = (float)oc.x, oy = (float)oc.y, oz = (float)oc.z;
  float qm = fmaxf(fmaxf(fabsf(fmaf(dx, t32, ox)), fabsf(fmaf(dy, t32, oy))), fabsf(fmaf(dz, t32, oz)));
  float dmax = fmaxf(fmaxf(fabsf(dx), fabsf(dy)), fabsf(dz));
  float l2 = fmaf(ox, ox, fmaf(oy, oy, oz * oz));
  // eps |d_k| <= 64 * 1.8e-15 |oc|^2 / sqrt(disc) * max |d_k| (+ lower-order terms) must stay below 5e-5 r
  bool quiet = 2.4e-13f * l2 * dmax < 5e-5f * r32 * sq32 && qm < 0.9999f * r32 && sq32 > 1e-3f * dmax * r32;
  if (__builtin_expect(quiet, 1)) return false;
  D3 q = oc + d * t;
  double eps = fast_root_error(len2(oc), sq, r_l, r_u, oimax);
  bool grazing = sq <= 1e-6 * fabs(half_b);
  bool pole = r - fabs(q.x) <= eps * fabs(d.x) || r - fabs(q.y) <= eps * fabs(d.y) || r - fabs(q.z) <= eps * fabs(d.z);
  return grazing || pole || !(eps * (double)dmax < 5e-5 * r);
}

// the first lines of Sphere::hit (sphere.rs:32-47): true when the discriminant is negative (same arithmetic as fast_sphere_hit below)
__device__ __forceinline__ bool fast_sphere_misses(const DevSphere &s, uint32_t payload, D3 o, D3 d, double time) {
  D3 c0 = ld3(s.c0);
  D3 center = (payload & SPH_MOVING) ? c0 + ld3(s.dc) * time : c0;
  D3 oc = o - center;
  double a = len2(d);
  double half_b = dot(oc, d);
  double c = len2(oc) - s.r2;
  return half_b * half_b - a * c < 0.0;
}

// Sphere::hit (sphere.rs:32-75) with the acceptance window widened by the tie band; same arithmetic, same root values.
__device__ __forceinline__ void fast_sphere_hit(const DevSphere &s, uint32_t payload, D3 o, D3 d, double time, float oimax, double &closest, uint32_t &hit_prim,
                                                bool &amb) {
  D3 c0 = ld3(s.c0);
  D3 center = (payload & SPH_MOVING) ? c0 + ld3(s.dc) * time : c0;
  D3 oc = o - center;
  double a = len2(d);
  double half_b = dot(oc, d);
  double c = len2(oc) - s.r2;
  double disc = half_b * half_b - a * c;
  if (disc < 0.0) return;
  double sq = sqrt(disc);
  double r_l = (-half_b - sq) / a;
  double r_u = (-half_b + sq) / a;
  const double band = fast_tie_band(fabs(r_l) + fabs(r_u), oimax);
  const double hi = closest + band;  // +inf stays +inf
  double t;
  if (1e-10 <= r_l && r_l <= hi) t = r_l;
  else if (1e-10 <= r_u && r_u <= hi) t = r_u;
  else return;
  // no from_normalized check here: build_fast_bvh only accepts scenes whose frame makes that assert unreachable (GuardFrame::normals_safe)
  amb = amb || (hit_prim != NONE && fabs(t - closest) <= band) || fast_hit_is_order_sensitive(oc, d, t, s.r2 * s.inv_r, half_b, sq, r_l, r_u, oimax);
  if (t <= closest) closest = t, hit_prim = payload;
}

// The self test of a scattered ray.  A ray that leaves a sphere starts at p, the rounded hit point, so its origin lies inside that sphere's
// padded box and the reject-only box test can never drop the sphere: without this every secondary ray pays a LEAF visit on the sphere it
// just left, which almost always returns nothing.  SHADE proves that here and the TRAV step then skips that one child entry.
// With o = p, oc = p - center is the value fast_sphere_hit would form (same time, same expressions), and so are a = len2(d),
// half_b = dot(oc, d) and c = len2(oc) - r2.  The visit accepts nothing when both ROUNDED roots are below 1e-10 (u = 2^-53, sqrt
// faithful: one rounding of <= 2u):
//   r_l:  half_b > 0  =>  -half_b - sq < 0  =>  r_l < 0.
//   r_u:  disc = RN(RN(half_b^2) - RN(a c)) differs from half_b^2 by <= 2.01u half_b^2 + 1.01 a|c|.  If disc <= half_b^2, sq <= (1 + 2u) half_b;
//         else sqrt(disc) - half_b = (disc - half_b^2) / (sqrt(disc) + half_b) < (2.01u half_b^2 + 1.01 a|c|) / (2 half_b).  Either way
//         sq - half_b <= 3.01u half_b + 0.51 a|c| / half_b, and the subtraction and the division add two roundings:
//         r_u <= (3.02u half_b^2 + 0.52 a|c|) / (a half_b).
// So the test is  4u half_b^2 + 0.6 a|c| < 1e-10 a half_b  (its own roundings, a few u, sit far inside the 4 / 3.02 and 0.6 / 0.52 headroom)
// together with  1e-270 <= 1e-10 a half_b <= DBL_MAX.  The lower end asks half_b > 0 and a > 0 and keeps underflow out of it: the products
// of disc that go subnormal add <= 1.5e-323 to it, i.e. <= 1.5e-323 / (a half_b) < 1e-60 to r_u.  The upper end keeps overflow out (an
// infinite right-hand side would pass any finite left-hand side).  A NaN anywhere fails a comparison: no skip.  The reference's
// Sphere::hit on this sphere then returns None for every window that starts at 1e-10 — so the fold's answer, the tie and order checks
// (amb) and the panic-site count cannot change.  An inward ray (refraction into the sphere, half_b < 0) and a camera ray never skip.
__device__ __forceinline__ bool fast_self_miss(const DevSphere &s, D3 oc, D3 d) {
  const double a = len2(d);
  const double half_b = dot(oc, d);
  const double c = len2(oc) - s.r2;
  const double rhs = 1e-10 * (a * half_b);
  return rhs >= 1e-270 && rhs <= 1.7976931348623157e308 && 4.4408920985006262e-16 * (half_b * half_b) + 0.6 * (a * fabs(c)) < rhs;  // 4u
}

// The reference's fold, verbatim: threaded program in stored order, exact divisions, Sphere::hit with ray_t.max = closest so far
// (bvh.rs:79-95, hittable/mod.rs:88-111).  Returns the number of from_normalized asserts tripped on the way.
__device__ __forceinline__ uint32_t fast_slow_trace(const DevOp *ops, const DevSphere *spheres, D3 o, D3 d, double time, double &closest, uint32_t &hit_prim) {
  Hit h{__longlong_as_double(0x7FF0000000000000ll), NONE};
  uint32_t flags = 0, pc = 0;
#pragma unroll 1
  for (;;) {
    const DevOp &op = ops[pc];
    uint32_t code = op.code & 0xFFu;
    if (code == OP_END) break;
    uint32_t a = op.a, b = NONE, next = pc + 1;
    if (code != OP_SPHERE) {  // OP_BOX / OP_BOX_SPH
      double bx[6] = {op.box[0], op.box[1], op.box[2], op.box[3], op.box[4], op.box[5]};
      if (!aabb_hit(bx, o, d, 1e-10, h.t)) {
        pc = op.skip;
        continue;
      }
      if (code == OP_BOX) {
        pc = next;
        continue;
      }
      b = op.b, next = op.skip;
    }
#pragma unroll 1
    for (int k = 0; k < 2; k++) {
      uint32_t payload = k == 0 ? a : b;
      if (payload != NONE && sphere_hit(spheres[payload & SPH_INDEX], payload, o, d, time, 1e-10, h)) flags++;
    }
    pc = next;
  }
  closest = h.t, hit_prim = h.prim;
  return flags;
}

// The instrumented fast kernel's census of wasted LEAF visits (tools/sched.py; the STATS instantiation, verify build) repeats the entry table's
// tests on the visits it counts: leaf boxes, balls and motion as the table kernel reads them, set by the host ahead of such a launch (all null
// otherwise: no census).  A device symbol, not kernel arguments: nothing a product kernel receives is for the tool alone.
struct CensusTables {
  const float *boxes;
  const double *balls, *motion;
  rl_rtiow_camera cam;  // the launch's camera: the census builds the pixel's beam from here
};
__device__ CensusTables g_census;
// What the entry table says of sphere `sidx` for pixel (px, y) and a sample at `time` (rl_pixel_entry.h, the same tests): bit 0 the leaf is in
// the all-times table's leaf set (else it only lies below one of its entries); bit 1 + i, for a moving sphere in that set, the ball of the
// sample's slice of 2 << i leaves it out.  (Inlined: out of line the instrumented kernel spills more, 292 VGPRs against 233.)
__device__ __forceinline__ uint32_t census_leaf(uint32_t px, uint32_t y, uint32_t sidx, double time, bool moving) {
  PixelBeam B;
  double t_lo, t_hi;
  const bool sph = pixel_beam(g_census.cam, px, y, B);
  const double *ball = g_census.balls + (size_t)sidx * 4;
  if (!beam_touches(B, g_census.boxes + (size_t)sidx * 8, t_lo, t_hi) || (sph && !beam_may_touch_ball(B, ball, t_lo, t_hi))) return 0u;
  uint32_t r = 1u;
  for (uint32_t lg = 1; lg <= 3u; lg++) {
    double sb[4];
    slice_ball(ball, g_census.motion + (size_t)sidx * 4, time_slice(time, lg), 1u << lg, sb);
    if (moving && sph && !beam_may_touch_ball(B, sb, t_lo, t_hi)) r |= 1u << lg;
  }
  return r;
}

#ifdef RL_FASTG_VERIFY  // debug build (make verify, tools/verify_fastg.py): every ray of the fast kernels is ALSO traced in the reference's order
__device__ unsigned int g_vcount;                                 // rays whose two answers differ
__device__ double g_vlog[64][12];                                  // the first 64 of them
__device__ unsigned long long g_vstats[4];                         // general kernel: TRAV steps, LEAF visits, far-origin rays; [3] rays verified by the sphere kernels
__device__ __forceinline__ void fast_verify_ray(const DevOp *ops, const DevSphere *spheres, D3 o, D3 d, double time, double closest, uint32_t hit_prim, double who) {
  double c2;
  uint32_t h2;
  fast_slow_trace(ops, spheres, o, d, time, c2, h2);
  const bool same = (hit_prim == NONE) == (h2 == NONE) && (h2 == NONE || ((h2 & SPH_INDEX) == (hit_prim & SPH_INDEX) && c2 == closest));
  if (!same) {
    unsigned k = atomicAdd(&g_vcount, 1u);
    if (k < 64) {
      double *L = g_vlog[k];
      L[0] = o.x, L[1] = o.y, L[2] = o.z, L[3] = d.x, L[4] = d.y, L[5] = d.z, L[6] = time, L[7] = hit_prim == NONE ? -1.0 : closest;
      L[8] = (double)(hit_prim & SPH_INDEX), L[9] = h2 == NONE ? -1.0 : c2, L[10] = (double)(h2 & SPH_INDEX), L[11] = who;
    }
  }
}
#endif
// rl_rtiow_coop.h (included after this header): what a wave of the STEAL instantiation runs once all its lanes have run out of pixels
template <int NT>
__device__ __forceinline__ void rtiow_steal_loop(const RtiowParams &P, unsigned long long *s_rng);

// STEAL (LDS_SCENE = 4, counter-free, the cost-sorted resume launch of a small shard): lanes hand a pixel over, at a sample boundary, to
// a wave that asks for it (P.steal_state), and a wave without work left asks — see rtiow_steal_loop
// (The parameter block arrives BY VALUE.  Measured in round 3: reading it from a device copy instead — scalar loads where a field is needed —
// removes every spill of the <1024, 4, false> instantiation (5 VGPRs / 75 SGPRs / 20 B of scratch -> 0 / 0 / 0) and is 1.2 % SLOWER
// (6625 against 6707 Mrays/s; the work-stealing instantiation 212 against 178 ms on the 1/8 shard): the v_readlane restores sit in block
// preambles, the scalar loads would sit in the blocks.)
// INDEP (rl_rtiow_render_independent*, counter-free LDS_SCENE = 4 and the counting layouts): a slot is (sample group, pixel) instead of a
// pixel — P.indep_k consecutive samples of one pixel, each from ChaCha word 0 on its own stream and from (0,0,0) — and every sample's colour
// goes to the pass buffer P.indep_buf[sample - sample_begin][pixel] (the ordered fold, rtiow_indep_fold, adds them up).
// The body (rl_rtiow_wave_body.inc) is written into both kernels, textually: behind a shared inline function the existing kernels compile to
// different code (measured: other register assignment, 4995 -> 4984 instructions for <1024, 4, false>), and they stay exactly what they were.
template <int NT, int LDS_SCENE, bool STATS, bool STEAL = false>
__global__ void RL_KERNEL_ALIGN __launch_bounds__(NT) rtiow_wave_kernel(RtiowParams P) {
  constexpr bool INDEP = false, MOMENTS = never_v<NT>;
#include "rl_rtiow_wave_body.inc"
}
// the sample-parallel mode (rl_rtiow_render_independent*): the same body, one (sample group, pixel) per slot
template <int NT, int LDS_SCENE, bool STATS>
__global__ void RL_KERNEL_ALIGN __launch_bounds__(NT) rtiow_wave_indep_kernel(RtiowParams P) {
  constexpr bool INDEP = true, STEAL = false, MOMENTS = never_v<NT>;
#include "rl_rtiow_wave_body.inc"
}
// MOMENTS (rl_rtiow_render_moments*): the same body; next to a pixel's sum of sample colours it keeps the sum of their
// squares, sq = sq + c * c per channel in sample order (the product rounded, then added), stored to and resumed from P.out_sq wherever
// the sum is stored to and resumed from P.out.  Counter-free, never stealing: a small shard's resume launch runs without it.
// With P.out_count set (rl_rtiow_render_adaptive*) a pixel also ends at the first checkpoint rtiow_adaptive_stop accepts.
template <int NT, int LDS_SCENE>
__global__ void RL_KERNEL_ALIGN __launch_bounds__(NT) rtiow_wave_moments_kernel(RtiowParams P) {
  constexpr bool INDEP = false, STEAL = false, STATS = false, MOMENTS = true;
#include "rl_rtiow_wave_body.inc"
}

}  // namespace rl
