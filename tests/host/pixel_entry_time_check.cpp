// Stand-alone check of the two expressions behind the entry table's time slices (csrc/rl_pixel_entry_slices.h; argument in the header of
// csrc/rl_pixel_entry.h, "Time slices"): no HIP, no Python.
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -I rendering-learning_amd \
//       tests/host/pixel_entry_time_check.cpp rendering-learning_amd/csrc/{rl_program,rl_fast_bvh,rl_scene_host}.cpp -o pixel_entry_time_check
// 1. The slice index.  For T = 2, 4, 8 and more than 2^20 values of time in [0, 1) — multiples of 2^-53 as gen_f64 makes them: random ones,
//    every k / T, its two neighbours, 0 and the largest value below 1 — time_slice, and time_slice_bits on the draw's high word (the form
//    GEN uses), equal floor(time T) computed in integers from the 53-bit numerator.  One line:   slices times N wrong W
// 2. The slice ball.  Spheres with random c0 and dc, magnitudes 1e-3 .. 1e3 independently per sphere (and a radius of 1e-3 .. 1e3), go
//    through guard_frame and fast_leaf_balls as a world's do.  For every T, slice k and times of the slice (both ends, the middle, random
//    ones), in long double: the distance from the exact centre c0 + dc time to the slice centre AS ROUNDED by slice_ball, plus r + pad,
//    plus the kernel's own rounding of c0 + dc time (2u |c|_max), is at most R_k.  pad is recomputed here by fast_leaf_balls' formula.
//    `margin` is the least (R_k - that sum) / R_k seen: positive, the room the 1e-12 terms of R leave.  One line:
//        balls spheres N checks C wrong W margin M
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "csrc/rl_pixel_entry_slices.h"
#include "csrc/rl_scene_host.h"

extern "C" int rl_bvh_build(const double *, const rl_href *, uint32_t, uint32_t, rl_bvh_node *, uint32_t, uint32_t *) { return RL_E_NO_DEVICE; }
extern "C" const char *rl_last_error(void) { return "no device: stand-alone host check"; }

static int failures = 0;

static void check_slices() {
  std::mt19937_64 gen(0x51CE5ull);
  unsigned long long n = 0, wrong = 0;
  auto one = [&](uint64_t num) {  // time = num 2^-53
    const double time = std::ldexp((double)num, -53);
    for (uint32_t lg = 1; lg <= 3; lg++) {
      const uint32_t want = (uint32_t)(num >> (53 - lg));  // floor(num 2^-53 2^lg)
      const uint32_t hi = (uint32_t)(num >> 21);  // the high word of the 64-bit draw u with num = u >> 11: what GEN takes the slice from
      if (rl::time_slice(time, lg) != want || rl::time_slice_bits(hi, lg) != want) {
        if (wrong < 10) std::printf("WRONG slice: time %a T %u got %u / %u want %u\n", time, 1u << lg, rl::time_slice(time, lg), rl::time_slice_bits(hi, lg), want);
        wrong++;
      }
    }
    if (rl::time_slice(time, 0) != 0u || rl::time_slice_bits((uint32_t)(num >> 21), 0) != 0u) wrong++;  // one slice: always word 0
    n++;
  };
  const uint64_t top = (1ull << 53) - 1;
  one(0), one(1), one(top);
  for (uint32_t k = 1; k < 8; k++) {
    const uint64_t b = (uint64_t)k << 50;  // k / 8: every boundary of T = 2, 4, 8
    one(b - 1), one(b), one(b + 1);
  }
  for (int i = 0; i < (1 << 20); i++) one(gen() >> 11);
  for (int i = 0; i < (1 << 16); i++) {  // near a boundary: k / 8 +- a few ulps
    const uint64_t b = (uint64_t)(1 + gen() % 7) << 50;
    one(b + (gen() % 65) - 32);
  }
  std::printf("slices times %llu wrong %llu\n", n, wrong);
  if (wrong || n < (1ull << 20)) failures++;
}

static void check_balls() {
  std::mt19937_64 gen(0xBA115ull);
  std::uniform_real_distribution<double> unit(-1.0, 1.0), expo(-3.0, 3.0), u01(0.0, 1.0);
  const uint32_t N = 4096;
  std::vector<rl_sphere> sph(N);
  for (uint32_t i = 0; i < N; i++) {
    rl_sphere &s = sph[i];
    const double mc = std::pow(10.0, expo(gen)), md = std::pow(10.0, expo(gen));
    s.radius = std::pow(10.0, expo(gen));
    s.moving = 1, s.material = 0;
    for (int ax = 0; ax < 3; ax++) s.center0[ax] = mc * unit(gen), s.center1[ax] = s.center0[ax] + md * unit(gen);
    if (i % 64 == 0)
      for (int ax = 1; ax < 3; ax++) s.center1[ax] = s.center0[ax];  // motion along one axis
  }
  rl_rtiow_scene_desc d{};
  d.spheres = sph.data(), d.n_spheres = N;
  const rl::GuardFrame f = rl::guard_frame(d);
  std::vector<double> balls, motion;
  if (!rl::fast_leaf_balls(d, f, balls, motion)) std::printf("FAIL balls: finite input reported as not finite\n"), failures++;
  unsigned long long checks = 0, wrong = 0;
  long double margin = 1.0L;
  const long double u = 0x1.0p-53L;
  for (uint32_t i = 0; i < N; i++) {
    const rl_sphere &s = sph[i];
    long double r = std::fabs(s.radius), pad = rl::guard_pad(f, (double)r), cmax = 0.0L;
    for (int ax = 0; ax < 3; ax++) {
      const double c0 = s.center0[ax], c1 = s.center1[ax];
      pad = std::fmax((double)pad, 1e-9 * (std::fabs(std::fmin(c0, c1) - (double)r) + std::fabs(std::fmax(c0, c1) + (double)r) + (double)r));
      cmax = std::fmax((double)cmax, std::fmax(std::fabs(c0), std::fabs(c1)));
    }
    for (uint32_t lg = 1; lg <= 3; lg++) {
      const uint32_t T = 1u << lg;
      for (uint32_t k = 0; k < T; k++) {
        double sb[4];
        rl::slice_ball(&balls[(size_t)i * 4], &motion[(size_t)i * 4], k, T, sb);
        const long double lo = (long double)k / T, hi = (long double)(k + 1) / T;
        const long double times[5] = {lo, hi, 0.5L * (lo + hi), lo + (hi - lo) * (long double)u01(gen), lo + (hi - lo) * (long double)u01(gen)};
        for (long double t : times) {
          long double d2 = 0.0L;
          for (int ax = 0; ax < 3; ax++) {  // the kernel's centre: c0 + RN(c1 - c0) time, exact here but for the difference the device holds too
            const long double c = (long double)s.center0[ax] + (long double)motion[(size_t)i * 4 + ax] * t;
            d2 += (c - (long double)sb[ax]) * (c - (long double)sb[ax]);
          }
          const long double need = std::sqrt(d2) + r + pad + 2.0L * u * cmax;
          checks++;
          if (!(need <= (long double)sb[3])) {
            if (wrong < 10) std::printf("WRONG ball: sphere %u T %u k %u t %Lg need %.20Lg R_k %.20g\n", i, T, k, t, need, sb[3]);
            wrong++;
          }
          margin = std::fmin(margin, ((long double)sb[3] - need) / (long double)sb[3]);
        }
      }
    }
  }
  std::printf("balls spheres %u checks %llu wrong %llu margin %.3Le\n", N, checks, wrong, margin);
  if (wrong || !(margin > 0.0L)) failures++;
}

int main() {
  check_slices();
  check_balls();
  std::printf(failures ? "FAIL %d\n" : "ok\n", failures);
  return failures ? 1 : 0;
}
