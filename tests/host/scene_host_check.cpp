// Stand-alone run of the host scene compiler (csrc/rl_scene_host.cpp over rl_program.cpp and rl_fast_bvh.cpp) on the example scenes
// and three hand-made ones: no HIP, no Python, so that it can be built with the host sanitizers and simply executed
// (tests/test_scene_host_standalone.py does both).  One line per scene — an RTIOW scene's 16 words of host_structures_report, an RTC
// scene's guard count, op count and return code — and a non-zero exit status when a return code or a hand-made scene's fact is wrong.
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -I rendering-learning_amd \
//       tests/host/scene_host_check.cpp rendering-learning_amd/csrc/{rl_program,rl_fast_bvh,rl_scene_host}.cpp -o scene_host_check
// With the path of tests/golden/teapot-low.obj as its argument it also compiles the RTC teapot scene (the one with triangle guards).
#include <cstdio>
#include <fstream>
#include <iterator>
#include <string>

#include "csrc/rl_scene_host.h"
#include "host/scenes.hpp"

// rtiow_host.hpp's DeviceBvh refers to these two; there is no device here
extern "C" int rl_bvh_build(const double *, const rl_href *, uint32_t, uint32_t, rl_bvh_node *, uint32_t, uint32_t *) { return RL_E_NO_DEVICE; }
extern "C" const char *rl_last_error(void) { return "no device: stand-alone host check"; }

static int failures = 0;

static void fail(const char *name, const std::string &what) {
  std::printf("FAIL %s: %s\n", name, what.c_str());
  failures++;
}

// build_host_rtiow + host_structures_report of one flattened world; returns what was built (null on an unexpected return code)
static std::shared_ptr<const rl::HostRtiow> run_rtiow(const char *name, const rtiow::Flattened &f) {
  rl_rtiow_scene_desc d = f.desc();
  std::shared_ptr<const rl::HostRtiow> H;
  std::string err;
  int rc = rl::build_host_rtiow(&d, H, err);
  if (rc != RL_OK) {
    fail(name, "build_host_rtiow = " + std::to_string(rc) + " (" + err + ")");
    return nullptr;
  }
  unsigned long long out[16];
  rl::host_structures_report(&d, *H, out);
  std::printf("%s", name);
  for (unsigned long long w : out) std::printf(" %llu", w);
  std::printf("\n");
  return H;
}
static std::shared_ptr<const rl::HostRtiow> run_rtiow(const char *name, const scenes::RtiowScene &s) {
  rtiow::Flattened f;
  f.root = s.world->flatten(f);
  return run_rtiow(name, f);
}

static void run_rtc(const char *name, const scenes::RtcScene &s, int want) {
  rtc::Flattened f;
  s.world.flatten(f);
  rl_rtc_scene_desc d = f.desc();
  std::shared_ptr<const rl::HostRtc> H;
  std::string err;
  int rc = rl::build_host_rtc(d, H, err);
  if (rc != want) fail(name, "build_host_rtc = " + std::to_string(rc) + " (" + err + "), expected " + std::to_string(want));
  std::printf("%s %zu %zu %d\n", name, H ? H->guards.size() : (size_t)0, H ? H->rc.ops.size() : (size_t)0, rc);
}

static rtiow::HittablePtr ball(double x, double y, double z, double r) {
  using namespace rtiow;
  return std::make_shared<Sphere>(Center::Stationary(Point3(x, y, z)), r, Lambertian(SolidColor(Color(0.5, 0.5, 0.5))));
}

int main(int argc, char **argv) {
  run_rtiow("golden_test_scene", scenes::golden_test_scene());
  run_rtiow("bouncing_spheres", scenes::bouncing_spheres(1));
  run_rtiow("checkered_spheres", scenes::checkered_spheres());
  run_rtiow("quads", scenes::quads_scene(false));
  run_rtiow("flat_world", scenes::quads_scene(true));
  run_rtiow("cornell_box", scenes::cornell_scene(false));
  run_rtiow("cornell_smoke", scenes::cornell_scene(true));
  run_rtiow("perlin_spheres", scenes::perlin_scene(false));
  run_rtiow("simple_light", scenes::perlin_scene(true));
  run_rtc("rtc_mirror", scenes::rtc_test_mirror_scene(), RL_OK);
  run_rtc("rtc_csg", scenes::rtc_test_csg_scene(), RL_OK);
  if (argc > 1) {
    std::ifstream in(argv[1], std::ios::binary);
    run_rtc("rtc_teapot", scenes::rtc_test_obj_scene(std::string(std::istreambuf_iterator<char>(in), std::istreambuf_iterator<char>())), RL_OK);
  }
  {  // a List whose two items are the SAME sphere record (sphere 1 is then in no list at all): no guards, so no compact ops and no fast
     // tree, and the scene renders from the linked ops
    rtiow::Flattened f;
    f.root = rtiow::HittableList({ball(0, 0, -1, 0.5), ball(0, -100.5, -1, 100)}).flatten(f);
    f.list_items[1] = f.list_items[0];
    auto H = run_rtiow("twice_named_sphere", f);
    if (H && !(H->cops.empty() && H->movbits.empty() && H->fast_root == rl::FAST_NONE && H->fast_nodes.empty() && !H->lops.empty() && H->lops.size() == H->rt.ops.size()))
      fail("twice_named_sphere", "guards were not refused: cops " + std::to_string(H->cops.size()) + ", lops " + std::to_string(H->lops.size()) + ", fast_root " + std::to_string(H->fast_root));
  }
  run_rtiow("radius_zero", scenes::RtiowScene{std::make_shared<rtiow::HittableList>(std::vector<rtiow::HittablePtr>{ball(0, 0, -1, 0.0), ball(0, -100.5, -1, 100)}), {}});
  run_rtiow("one_sphere", scenes::RtiowScene{std::make_shared<rtiow::HittableList>(std::vector<rtiow::HittablePtr>{ball(0, 0, -1, 0.5)}), {}});
  return failures ? 1 : 0;
}
