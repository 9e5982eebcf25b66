// Stand-alone host check of the RTC shading queries' entry points (include/rl_render.h) on a machine without a GPU: every form must
// return RL_E_NO_DEVICE before it touches a buffer, and n = 0 / NULL arguments must not be dereferenced.  Meant to be built with the
// host sanitizers (the library's host code and this file; no Python involved):
//   cd rendering-learning_amd/csrc && for f in rl_render.hip rl_multi.hip rl_bvh_build.hip rl_program.cpp rl_fast_bvh.cpp; do
//     hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -fPIC -ffp-contract=off -Xarch_host -fsanitize=address,undefined -c -o /tmp/san_${f%.*}.o $f; done
//   clang++ -std=c++17 -g -fsanitize=address,undefined -I../../include -c -o /tmp/san_main.o ../../tools/rtc_shade_query_nodevice.cpp
//   hipcc --offload-arch=gfx950 -fsanitize=address,undefined -o /tmp/rtc_shade_query_nodevice /tmp/san_*.o -ldl && /tmp/rtc_shade_query_nodevice
#include <cstdio>
#include <vector>

#include "rl_render.h"

#define EXPECT(call, want)                                                  \
  do {                                                                      \
    int rc_ = (call);                                                       \
    if (rc_ != (want)) {                                                    \
      std::printf("FAIL %s = %d, expected %d (%s)\n", #call, rc_, (want), rl_last_error()); \
      failures++;                                                           \
    }                                                                       \
  } while (0)

int main() {
  int failures = 0;
  if (rl_init(-1) == RL_OK) {
    std::printf("a device is present: the no-device paths are not reachable, nothing checked\n");
    return 0;
  }
  const uint64_t n = 3;
  std::vector<rl_ray> rays(n);
  std::vector<rl_rtc_comps> comps(n);
  std::vector<rl_rtc_shade> shade(n);
  std::vector<double> v3(n * 3), att(n, 1.0), rgb(n * 3), shadow(n);
  rl_stats st;
  for (int with_stats = 0; with_stats < 2; with_stats++) {
    rl_stats *s = with_stats ? &st : nullptr;
    for (uint64_t m : {n, (uint64_t)0}) {
      EXPECT(rl_rtc_prepare_rays(nullptr, rays.data(), m, comps.data(), s), RL_E_NO_DEVICE);
      EXPECT(rl_rtc_prepare_rays_device(nullptr, rays.data(), m, comps.data(), nullptr, s), RL_E_NO_DEVICE);
      EXPECT(rl_rtc_shade_hits(nullptr, comps.data(), m, shade.data(), shadow.data(), s), RL_E_NO_DEVICE);
      EXPECT(rl_rtc_shade_hits(nullptr, comps.data(), m, shade.data(), nullptr, s), RL_E_NO_DEVICE);
      EXPECT(rl_rtc_shade_hits_device(nullptr, comps.data(), m, shade.data(), shadow.data(), nullptr, s), RL_E_NO_DEVICE);
      EXPECT(rl_rtc_shadow_attenuation(nullptr, v3.data(), v3.data(), m, att.data(), s), RL_E_NO_DEVICE);
      EXPECT(rl_rtc_shadow_attenuation_device(nullptr, v3.data(), v3.data(), m, att.data(), nullptr, s), RL_E_NO_DEVICE);
      EXPECT(rl_rtc_lighting(nullptr, comps.data(), v3.data(), v3.data(), att.data(), m, rgb.data()), RL_E_NO_DEVICE);
      EXPECT(rl_rtc_lighting_device(nullptr, comps.data(), v3.data(), v3.data(), att.data(), m, rgb.data(), nullptr), RL_E_NO_DEVICE);
    }
  }
  EXPECT(rl_rtc_prepare_rays(nullptr, nullptr, n, nullptr, nullptr), RL_E_NO_DEVICE);
  EXPECT(rl_rtc_shade_hits(nullptr, nullptr, n, nullptr, nullptr, nullptr), RL_E_NO_DEVICE);
  EXPECT(rl_rtc_shadow_attenuation(nullptr, nullptr, nullptr, n, nullptr, nullptr), RL_E_NO_DEVICE);
  EXPECT(rl_rtc_lighting(nullptr, nullptr, nullptr, nullptr, nullptr, n, nullptr), RL_E_NO_DEVICE);
  std::printf(failures ? "%d failures\n" : "rtc shading queries, no-device paths: ok\n", failures);
  return failures ? 1 : 0;
}
