// Stand-alone check of flatten_sphere_materials (csrc/rl_scene_host.cpp): which spheres get the flat form of a Checker of two Solid
// colours (MAT_TEX_CHECKER in the flattened kind, the even colour in albedo, the odd colour and inv_scale in the sphere's DevChecker
// record, every value the texture table's bits) and which keep the generic walk.  No HIP, no Python: built with the host sanitizers and
// executed by tests/test_flat_checker_standalone.py.  Spheres are told apart by their radius.  Exit status 1 when a fact is wrong.
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -I rendering-learning_amd \
//       tests/host/flat_checker_check.cpp rendering-learning_amd/csrc/{rl_program,rl_fast_bvh,rl_scene_host}.cpp -o flat_checker_check
#include <cstdio>
#include <cstring>
#include <string>

#include "csrc/rl_scene_host.h"
#include "host/scenes.hpp"

extern "C" int rl_bvh_build(const double *, const rl_href *, uint32_t, uint32_t, rl_bvh_node *, uint32_t, uint32_t *) { return RL_E_NO_DEVICE; }
extern "C" const char *rl_last_error(void) { return "no device: stand-alone host check"; }

static int failures = 0;
static void fail(double radius, const std::string &what) {
  std::printf("FAIL sphere of radius %g: %s\n", radius, what.c_str());
  failures++;
}
static bool same_bits(const double *a, const double *b, int n) { return std::memcmp(a, b, sizeof(double) * (size_t)n) == 0; }

int main() {
  using namespace rtiow;
  const double A[3] = {-0.0, 0.4, 0.7}, B[3] = {0.8, 0.2, 0.1}, ZERO[4] = {0.0, 0.0, 0.0, 0.0};
  auto solidA = [&] { return SolidColor(Color(A[0], A[1], A[2])); };
  auto solidB = [&] { return SolidColor(Color(B[0], B[1], B[2])); };
  const double scale = 0.32, inv_scale = 1.0 / scale;
  auto flat = [&] { return Checker(scale, solidA(), solidB()); };
  auto nested = [&] { return Checker(scale, Checker(0.07, solidA(), solidA()), Checker(0.07, solidB(), solidB())); };
  auto half = [&] { return Checker(scale, solidA(), Checker(0.07, solidB(), solidB())); };
  auto shared = Lambertian(flat());  // one material, and so one checker texture, on two spheres
  struct Case {
    double radius;
    MaterialPtr mat;
    uint32_t kind;     // the material's kind
    uint32_t tex_flag;  // MAT_TEX_SOLID, MAT_TEX_CHECKER or 0
  };
  const Case cases[] = {
      {0.50, Lambertian(flat()), RL_MAT_LAMBERTIAN, rl::MAT_TEX_CHECKER},
      {0.51, DiffuseLight(flat()), RL_MAT_DIFFUSE_LIGHT, rl::MAT_TEX_CHECKER},
      {0.52, shared, RL_MAT_LAMBERTIAN, rl::MAT_TEX_CHECKER},
      {0.53, shared, RL_MAT_LAMBERTIAN, rl::MAT_TEX_CHECKER},
      {0.54, Lambertian(nested()), RL_MAT_LAMBERTIAN, 0u},
      {0.55, DiffuseLight(nested()), RL_MAT_DIFFUSE_LIGHT, 0u},
      {0.56, Lambertian(half()), RL_MAT_LAMBERTIAN, 0u},
      {0.57, Lambertian(solidA()), RL_MAT_LAMBERTIAN, rl::MAT_TEX_SOLID},
      {0.58, Metal(Color(0.8, 0.7, 0.6), 0.2), RL_MAT_METAL, 0u},
      {0.59, Dielectric(1.5), RL_MAT_DIELECTRIC, 0u},
  };
  std::vector<HittablePtr> items;
  double x = -6.0;
  for (const Case &c : cases) items.push_back(std::make_shared<Sphere>(Center::Stationary(Point3(x += 1.25, c.radius, -1.0)), c.radius, c.mat));
  Flattened f;
  f.root = HittableList(items).flatten(f);
  rl_rtiow_scene_desc d = f.desc();
  std::shared_ptr<const rl::HostRtiow> H;
  std::string err;
  if (int rc = rl::build_host_rtiow(&d, H, err)) {
    std::printf("FAIL build_host_rtiow = %d (%s)\n", rc, err.c_str());
    return 1;
  }
  const size_t n = H->rt.spheres.size();
  if (n != sizeof cases / sizeof cases[0] || H->sphere_flat.size() != n || H->sphere_checker.size() != n) {
    std::printf("FAIL sizes: %zu spheres, %zu flat materials, %zu checker records\n", n, H->sphere_flat.size(), H->sphere_checker.size());
    return 1;
  }
  size_t seen = 0;
  for (size_t i = 0; i < n; i++) {
    const double r = 1.0 / H->rt.spheres[i].inv_r;
    const Case *c = nullptr;
    for (const Case &k : cases)
      if (k.radius - 1e-9 < r && r < k.radius + 1e-9) c = &k;
    if (!c) {
      fail(r, "not one of the cases");
      continue;
    }
    seen++;
    const rl::DevMaterial &m = H->sphere_flat[i];
    const rl::DevChecker &ck = H->sphere_checker[i];
    if ((m.kind & 0xFFu) != c->kind) fail(r, "kind " + std::to_string(m.kind & 0xFFu));
    if ((m.kind & ~0xFFu) != c->tex_flag) fail(r, "texture flags " + std::to_string(m.kind & ~0xFFu) + ", expected " + std::to_string(c->tex_flag));
    if (c->tex_flag == rl::MAT_TEX_CHECKER) {
      if (!same_bits(m.albedo, A, 3)) fail(r, "albedo is not the even colour's bits");
      if (!same_bits(ck.odd, B, 3)) fail(r, "DevChecker::odd is not the odd colour's bits");
      if (!same_bits(&ck.inv_scale, &inv_scale, 1)) fail(r, "DevChecker::inv_scale is not 1 / scale");
    } else {
      if (!same_bits(ck.odd, ZERO, 3) || !same_bits(&ck.inv_scale, ZERO, 1)) fail(r, "a DevChecker record that is not all zero");
      if (c->tex_flag == rl::MAT_TEX_SOLID && !same_bits(m.albedo, A, 3)) fail(r, "albedo is not the Solid colour's bits");
    }
  }
  if (seen != n) fail(0.0, "cases seen: " + std::to_string(seen));
  std::printf("%zu spheres checked, %d failures\n", n, failures);
  return failures ? 1 : 0;
}
