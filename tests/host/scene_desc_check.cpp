// Stand-alone run of the host scene compiler on BAD descriptions: no HIP, no Python, built with the host sanitizers and simply executed
// (tests/test_scene_desc_refusals.py does both, and holds the table of expected outcomes).
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -I rendering-learning_amd \
//       tests/host/scene_desc_check.cpp rendering-learning_amd/csrc/{rl_program,rl_fast_bvh,rl_scene_host}.cpp -o scene_desc_check -lpthread
// Every kernel trusts the program build_host_rtiow / build_host_rtc hand it: skip words are followed unchecked, the instance, CSG and
// pending-ray stacks have fixed sizes, table indices are dereferenced as given.  This program is what stands between a wrong description
// and a device, in five parts:
//   A  one case per refusal of the compilers: the smallest edit of a valid description that must trigger it
//   B  every cap from both sides: accepted at the cap, refused one above it
//   C  depth: chains at RL_SCENE_MAX_NEST and one deeper, each compiled on a thread with a 1 MiB stack
//   D  sharing: doubling graphs whose expansion is 2^60 visits; with the argument `nomem` (a build WITHOUT sanitizers: ASan reserves
//      terabytes of address space) only the allocation-failure cases, under setrlimit(RLIMIT_AS, 1 GiB).  The arguments `lists` and
//      `checkers` run one case of C alone: with `nomem`, the three runs in which the recursive compiler crashed (profiles/scene_desc_check.txt)
//   E  exhaustive single-field mutation of the base descriptions of A, each outcome a refusal or a program that passes the checker
// Output: one line per case, `case <name> | <return code> | <out is null: 1/0> | <message> | <facts>`; `E ...` lines with the mutation
// counts; `FAIL ...` lines and exit status 1 when something this program itself asserts is wrong.
//
// THE PROGRAM CHECKER (check_rtiow / check_rtc below) is written from rl_program.h's comments, not by calling library code.  It states
// what the kernels assume without checking.
//
// Two limits of part E, both for the same reason — a C caller that claims memory it does not own cannot be found out by any callee:
//   * an array count n_* is set to 0, to n + 1 WITH one more (zeroed) record behind the pointer, and to 0xFFFFFFFF only for n_spheres,
//     the one table with a cap to refuse by (every other table would have to be read to be judged);
//   * "count too large" as a class that must be refused therefore applies to the counts the compiler CAN judge: rl_list::count,
//     rl_rtc_group::count, rl_bvh_node::n_children and n_spheres.
// Part B's `n_spheres == SPH_INDEX` (accepted side) would need 2^30 sphere records (77 GB); only the refused side is tested.
#include <pthread.h>
#include <sys/resource.h>

#include <chrono>
#include <cstdio>
#include <cstring>
#include <functional>
#include <map>
#include <string>

#include "csrc/rl_scene_host.h"
#include "host/scenes.hpp"

// rtiow_host.hpp's DeviceBvh refers to these two; there is no device here
extern "C" int rl_bvh_build(const double *, const rl_href *, uint32_t, uint32_t, rl_bvh_node *, uint32_t, uint32_t *) { return RL_E_NO_DEVICE; }
extern "C" const char *rl_last_error(void) { return "no device: stand-alone host check"; }

using RF = rtiow::Flattened;
using CF = rtc::Flattened;
using rl::NONE;

static int failures = 0;
static void fail(const std::string &name, const std::string &what) {
  std::printf("FAIL %s: %s\n", name.c_str(), what.c_str());
  failures++;
}

// ============================================================================================ the program checker
// Returns "" or the first violated assumption.
static std::string check_rtiow(const rl::HostRtiow &H) {
  using namespace rl;
  const RtiowProgram &p = H.rt;
  const std::vector<DevOp> &ops = p.ops;
  const size_t n = ops.size();
  auto at = [](size_t i, const char *what) { return "op " + std::to_string(i) + ": " + what; };
  if (n == 0 || n >= 0x7FFFFFFFu) return "op count";
  if (ops[n - 1].code != OP_END) return "last op is not OP_END";
  auto sphere_ok = [&](uint32_t payload) { return (payload & SPH_INDEX) < p.spheres.size(); };
  std::vector<uint32_t> pushes, depth_at(n, 0);  // open PUSH ops; PUSH depth in front of every op
  uint32_t medium_begin = NONE;
  for (size_t i = 0; i < n; i++) {
    const DevOp &o = ops[i];
    const uint32_t kind = o.code & 0xFFu;
    depth_at[i] = (uint32_t)pushes.size();
    if (o.code & ~(0xFFu | BOX_FINITE)) return at(i, "unknown bits in code");
    if (kind == OP_END) {
      if (i != n - 1) return at(i, "OP_END before the end");
      if (!pushes.empty() || medium_begin != NONE) return at(i, "END inside an instance or a medium");
      continue;
    }
    if (!(o.skip > i && o.skip <= n - 1)) return at(i, "skip outside (i, n_ops)");
    switch (kind) {
      case OP_BOX:
        if (o.a != NONE || o.b != NONE) return at(i, "BOX payload");
        break;
      case OP_BOX_SPH:
        if (!sphere_ok(o.a) || (o.b != NONE && !sphere_ok(o.b)) || o.skip != i + 1) return at(i, "BOX_SPH");
        break;
      case OP_SPHERE:
        if (!sphere_ok(o.a) || o.b != NONE || o.skip != i + 1) return at(i, "SPHERE");
        break;
      case OP_PLANAR:
        if (o.a >= p.planars.size() || o.b != NONE || o.skip != i + 1) return at(i, "PLANAR");
        break;
      case OP_BOX_PLANAR:
        if (o.a >= p.planars.size() || (o.b != NONE && o.b >= p.planars.size()) || o.skip != i + 1) return at(i, "BOX_PLANAR");
        break;
      case OP_PUSH_TRANSLATE:
      case OP_PUSH_TRANSFORM:
        if (o.a >= (kind == OP_PUSH_TRANSLATE ? p.translates.size() : p.transforms.size())) return at(i, "PUSH index");
        if (o.b != (pushes.empty() ? NONE : pushes.back())) return at(i, "PUSH .b is not the enclosing PUSH");
        if (o.skip != i + 1) return at(i, "PUSH skip");
        pushes.push_back((uint32_t)i);
        if (pushes.size() > 8) return at(i, "PUSH depth above 8");
        break;
      case OP_POP_TRANSLATE:
      case OP_POP_TRANSFORM: {
        if (pushes.empty() || o.b != pushes.back()) return at(i, "POP .b is not its matching PUSH");
        const DevOp &pu = ops[o.b];
        if ((pu.code & 0xFFu) != kind - 1u || pu.a != o.a || o.skip != i + 1) return at(i, "POP does not mirror its PUSH");
        pushes.pop_back();
        break;
      }
      case OP_MEDIUM_BEGIN:
        if (o.a >= p.media.size() || medium_begin != NONE) return at(i, "MEDIUM_BEGIN");
        if ((ops[o.skip - 1].code & 0xFFu) != OP_MEDIUM_END || ops[o.skip - 1].b != i) return at(i, "MEDIUM_BEGIN skip - 1 is not its END");
        medium_begin = (uint32_t)i;
        break;
      case OP_MEDIUM_END:
        if (o.b != medium_begin || o.a != ops[medium_begin].a || o.skip != i + 1) return at(i, "MEDIUM_END .b is not its BEGIN");
        if (depth_at[i] != depth_at[medium_begin]) return at(i, "MEDIUM_END at another PUSH depth");
        medium_begin = NONE;
        break;
      default: return at(i, "unknown op code");
    }
  }
  for (size_t i = 0; i + 1 < n; i++) {  // only a PUSH enters an instance; a missed box jumps over whole instances
    const uint32_t kind = ops[i].code & 0xFFu;
    const bool push = kind == OP_PUSH_TRANSLATE || kind == OP_PUSH_TRANSFORM;
    if (depth_at[ops[i].skip] > depth_at[i] + (push ? 1u : 0u)) return at(i, "skip enters an instance");
    if (kind == OP_BOX && depth_at[ops[i].skip] != depth_at[i]) return at(i, "BOX skip changes PUSH depth");
  }
  if (p.max_instance_depth > 8) return "max_instance_depth";
  // ---- tables as lowered
  if (p.sphere_material.size() != p.spheres.size() || p.sphere_uv.size() != p.spheres.size()) return "per-sphere tables";
  for (uint32_t m : p.sphere_material)
    if (m >= p.materials.size()) return "sphere material";
  for (const DevPlanar &pl : p.planars)
    if (pl.material >= p.materials.size() || pl.kind > RL_PLANAR_TRIANGLE) return "planar record";
  for (const rl_medium &m : p.media)
    if (m.material >= p.materials.size()) return "medium material";
  for (const DevMaterial &m : p.materials) {
    if (m.kind > RL_MAT_ISOTROPIC) return "material kind";
    if ((m.kind == RL_MAT_LAMBERTIAN || m.kind == RL_MAT_DIFFUSE_LIGHT || m.kind == RL_MAT_ISOTROPIC) && m.texture >= p.textures.size()) return "material texture";
  }
  for (size_t t = 0; t < p.textures.size(); t++) {
    const DevTexture &tx = p.textures[t];
    if (tx.kind == RL_TEX_CHECKER) {
      if (tx.even >= p.textures.size() || tx.odd >= p.textures.size()) return "checker child";
    } else if (tx.kind == RL_TEX_IMAGE) {
      if (tx.image >= p.images.size()) return "texture image";
    } else if (tx.kind == RL_TEX_NOISE) {
      if (tx.image >= p.perlins.size()) return "texture perlin";
    } else if (tx.kind != RL_TEX_SOLID) return "texture kind";
  }
  {  // every checker walk the device can take ends within 32 steps: longest path by relaxation, 33 rounds
    std::vector<int> len(p.textures.size(), 0);
    for (int round = 0; round < 34; round++) {
      bool changed = false;
      for (size_t t = 0; t < p.textures.size(); t++) {
        if (p.textures[t].kind != RL_TEX_CHECKER) continue;
        int l = 1 + std::max(len[p.textures[t].even], len[p.textures[t].odd]);
        if (l != len[t]) len[t] = l, changed = true;
      }
      if (!changed) break;
      if (round == 33) return "checker nesting does not settle within 32";
    }
    for (int l : len)
      if (l > 32) return "checker nesting above 32";
  }
  for (const DevImage &im : p.images)
    if (im.width == 0 || im.height == 0 || im.offset + (uint64_t)im.width * im.height * 3 > p.image_pool.size()) return "image extent";
  for (const rl_perlin &pn : p.perlins)
    for (int k = 0; k < 256; k++)
      if (pn.perm_x[k] > 255 || pn.perm_y[k] > 255 || pn.perm_z[k] > 255) return "perlin permutation";
  // ---- linked / compact successor words: state << 29 | op index of the SAME array (link_ops); the end marker is ST_SHADE
  auto word_ok = [&](uint32_t w, size_t size) {
    const uint32_t st = w >> 29, idx = w & 0x1FFFFFFFu;
    return (st == ST_TRAV || st == ST_LEAF || st == ST_SHADE) && (idx < size || (st == ST_SHADE && size == 0));
  };
  if (!H.lops.empty()) {
    if (H.lops.size() != n) return "lops size";
    if (!word_ok(H.entry0, n)) return "entry0";
    for (size_t i = 0; i + 1 < n; i++) {
      if (!word_ok(H.lops[i].code, n) || !word_ok(H.lops[i].skip, n)) return at(i, "lops successor word");
      const uint32_t k = ops[i].code & 0xFFu;
      if ((k == OP_BOX_SPH || k == OP_SPHERE) && (!sphere_ok(H.lops[i].a) || (H.lops[i].b != NONE && !sphere_ok(H.lops[i].b)))) return at(i, "lops payload");
    }
    if (H.sphere_flat.size() != p.spheres.size()) return "sphere_flat size";
  }
  if (!H.cops.empty()) {
    if (H.cops.size() != n + p.spheres.size()) return "cops size";
    if (!word_ok(H.centry0, H.cops.size())) return "centry0";
    for (size_t i = 0; i < H.cops.size(); i++) {
      if (i == n - 1) continue;  // the END op keeps its words, nothing leads to them but as a SHADE target
      if (!word_ok(H.cops[i].w_hit, H.cops.size()) || !word_ok(H.cops[i].w_miss, H.cops.size())) return "cops successor word " + std::to_string(i);
    }
    if (H.movbits.size() != 2 * ((p.spheres.size() + 31) / 32 + 1)) return "movbits size";
  }
  return "";
}

static std::string check_rtc(const rl::HostRtc &H) {
  using namespace rl;
  const RtcProgram &p = H.rc;
  const std::vector<DevOp> &ops = p.ops;
  const size_t n = ops.size();
  auto at = [](size_t i, const char *what) { return "op " + std::to_string(i) + ": " + what; };
  if (n == 0 || n >= 0x7FFFFFFFu) return "op count";
  if (ops[n - 1].code != ROP_END) return "last op is not ROP_END";
  struct Open {
    uint32_t pc, kind, mids;
  };
  std::vector<Open> open;  // ENTER and CSG_BEGIN ops not yet closed
  std::vector<uint32_t> enters, open_at(n, 0);
  uint32_t csg_depth = 0;
  for (size_t i = 0; i < n; i++) {
    const DevOp &o = ops[i];
    open_at[i] = (uint32_t)open.size();
    switch (o.code) {
      case ROP_END:
        if (i != n - 1 || !open.empty()) return at(i, "ROP_END early or inside a scope");
        break;
      case ROP_ENTER:
        if (o.a >= p.xforms.size() || o.b != (enters.empty() ? NONE : enters.back())) return at(i, "ENTER");
        enters.push_back((uint32_t)i), open.push_back(Open{(uint32_t)i, ROP_ENTER, 0});
        if (enters.size() > 8) return at(i, "ENTER depth above 8");
        break;
      case ROP_EXIT:
        if (open.empty() || open.back().kind != ROP_ENTER || o.skip != open.back().pc || ops[o.skip].a != o.a) return at(i, "EXIT.skip is not its ENTER");
        enters.pop_back(), open.pop_back();
        if (o.b != (enters.empty() ? NONE : enters.back())) return at(i, "EXIT.b is not the enclosing ENTER");
        break;
      case ROP_BOUNDS:
        if (!(o.skip > i && o.skip < n)) return at(i, "BOUNDS.skip outside (i, n_ops)");
        break;
      case ROP_TRIS:
        if (o.b == 0 || (uint64_t)o.a + o.b > p.tris.size()) return at(i, "TRIS range outside tris");
        if (o.skip != 0 && (o.skip - 1 >= H.guards.size())) return at(i, "TRIS guard root");
        break;
      case ROP_SHAPE:
        if (o.a >= p.shapes.size()) return at(i, "SHAPE index");
        break;
      case ROP_CSG_BEGIN:
        if (o.a >= p.csgs.size()) return at(i, "CSG index");
        open.push_back(Open{(uint32_t)i, ROP_CSG_BEGIN, 0});
        if (++csg_depth > 4) return at(i, "CSG depth above 4");
        break;
      case ROP_CSG_MID:
        if (open.empty() || open.back().kind != ROP_CSG_BEGIN || open.back().mids++ != 0 || ops[open.back().pc].a != o.a) return at(i, "CSG_MID");
        break;
      case ROP_CSG_END:
        if (open.empty() || open.back().kind != ROP_CSG_BEGIN || open.back().mids != 1 || ops[open.back().pc].a != o.a) return at(i, "CSG_END");
        open.pop_back(), csg_depth--;
        break;
      default: return at(i, "unknown op code");
    }
  }
  for (size_t i = 0; i < n; i++)  // a missed box jumps over whole scopes, never into one
    if (ops[i].code == ROP_BOUNDS && open_at[ops[i].skip] != open_at[i]) return at(i, "BOUNDS.skip changes scope");
  if (p.max_xform_depth > 8 || p.max_csg_depth > 4) return "recorded depths";
  for (const DevTri &t : p.tris)
    if (t.material >= p.materials.size()) return "triangle material";
  for (const rl_rtc_shape &s : p.shapes)
    if (s.material >= p.materials.size()) return "shape material";
  for (size_t i = 0; i < n; i++)  // the kernels branch on the kind of a shape an op names (a record nothing names is never read)
    if (ops[i].code == ROP_SHAPE && (p.shapes[ops[i].a].kind < RL_O_SPHERE || p.shapes[ops[i].a].kind > RL_O_CONE)) return at(i, "shape kind");
  for (const rl_rtc_material &m : p.materials)
    if (m.pattern > p.patterns.size()) return "material pattern";
  for (const rl_rtc_pattern &pt : p.patterns)
    if (pt.kind < RL_PAT_STRIPE || pt.kind > RL_PAT_CHECKER3D) return "pattern kind";
  for (size_t i = 0; i < n; i++)  // likewise the operation of a csg an op names
    if (ops[i].code == ROP_CSG_BEGIN && p.csgs[ops[i].a].operation > RL_CSG_DIFFERENCE) return at(i, "csg operation");
  for (size_t g = 0; g < H.guards.size(); g++)
    if (!(H.guards[g].skip > g && H.guards[g].skip <= H.guards.size()) || (H.guards[g].tri != NONE && H.guards[g].tri >= p.tris.size())) return "guard " + std::to_string(g);
  if (p.lights.size() > 0xFFFFu) return "light count";
  if (p.needs_full && p.max_reflection_depth + 1u > RTC_MAX_PENDING) return "pending rays";
  return "";
}

// ============================================================================================ running one description
struct Outcome {
  int rc = 0;
  std::string err, facts;
  bool out_null = true;
  size_t n_ops = 0, n_guards = 0;
};

static Outcome run(const rl_rtiow_scene_desc &d) {
  Outcome o;
  std::shared_ptr<const rl::HostRtiow> H;
  o.rc = rl::build_host_rtiow(&d, H, o.err);
  o.out_null = !H;
  if (H) {
    o.n_ops = H->rt.ops.size();
    std::string bad = check_rtiow(*H);
    o.facts = "ops=" + std::to_string(o.n_ops) + (bad.empty() ? " checked" : " CHECKER: " + bad);
  }
  return o;
}
static Outcome run(const rl_rtc_scene_desc &d) {
  Outcome o;
  std::shared_ptr<const rl::HostRtc> H;
  o.rc = rl::build_host_rtc(d, H, o.err);
  o.out_null = !H;
  if (H) {
    o.n_ops = H->rc.ops.size();
    std::string bad = check_rtc(*H);
    o.facts = "ops=" + std::to_string(o.n_ops) + " guards=" + std::to_string(H->guards.size()) + (bad.empty() ? " checked" : " CHECKER: " + bad);
    o.n_guards = H->guards.size();
  }
  return o;
}
// what every outcome must satisfy, whatever the table says: a refusal has a code, a message and no product; a product passes the checker
static bool well_formed(const Outcome &o) {
  if (o.rc == RL_OK) return !o.out_null && o.err.empty() && o.facts.find("CHECKER") == std::string::npos;
  return o.out_null && !o.err.empty() && (o.rc == RL_E_INVALID || o.rc == RL_E_UNSUPPORTED || o.rc == RL_E_NOMEM);
}
static Outcome report(const std::string &name, const Outcome &o) {
  std::printf("case %s | %d | %d | %s | %s\n", name.c_str(), o.rc, o.out_null ? 1 : 0, o.err.c_str(), o.facts.c_str());
  std::fflush(stdout);
  if (!well_formed(o)) fail(name, "outcome is neither a clean refusal nor a checked program");
  return o;
}
template <class F>
static Outcome run_case(const std::string &name, const F &f) {
  return report(name, run(f.desc()));
}
static void expect_ops(const std::string &name, const Outcome &o, size_t want) {
  if (o.rc != RL_OK || o.n_ops != want) fail(name, "expected " + std::to_string(want) + " ops, got rc " + std::to_string(o.rc) + ", " + std::to_string(o.n_ops));
}

// ============================================================================================ base descriptions
static RF flat(const scenes::RtiowScene &s) {
  RF f;
  f.root = s.world->flatten(f);
  return f;
}
static CF flat(const scenes::RtcScene &s) {
  CF f;
  s.world.flatten(f);
  return f;
}
static rl_sphere raw_sphere(double x, double y, double z, double r, uint32_t material) {
  rl_sphere s{};
  s.center0[0] = x, s.center0[1] = y, s.center0[2] = z, s.radius = r, s.material = material;
  return s;
}
// one Lambertian sphere in a list; `lists` / `list_items` are the caller's to extend
static RF sphere_world() {
  RF f;
  rl_texture t{};
  t.kind = RL_TEX_SOLID, t.color[0] = t.color[1] = t.color[2] = 0.5;
  f.textures.push_back(t);
  rl_material m{};
  m.kind = RL_MAT_LAMBERTIAN, m.texture = 0;
  f.materials.push_back(m);
  f.spheres.push_back(raw_sphere(0, 0, -1, 0.5, 0));
  f.lists.push_back(rl_list{0, 1});
  f.list_items.push_back(rl_href{RL_H_SPHERE, 0});
  f.root = rl_href{RL_H_LIST, 0};
  return f;
}
static RF image_world() {  // an image-textured sphere and a solid one
  RF f = sphere_world();
  auto img = std::make_shared<rtiow::ImageData>();
  img->width = 2, img->height = 2, img->rgb.assign(12, 0.25f);
  f.image_keep.push_back(img);
  f.images.push_back(rl_image{2, 2, img->rgb.data()});
  rl_texture t{};
  t.kind = RL_TEX_IMAGE, t.image = 0;
  f.textures.push_back(t);
  rl_material m{};
  m.kind = RL_MAT_LAMBERTIAN, m.texture = 1;
  f.materials.push_back(m);
  f.spheres.push_back(raw_sphere(1, 0, -1, 0.5, 1));
  f.list_items.push_back(rl_href{RL_H_SPHERE, 1});
  f.lists[0].count = 2;
  return f;
}
static void identity4(double *m) {
  for (int i = 0; i < 16; i++) m[i] = i % 5 == 0 ? 1.0 : 0.0;
}
static rl_rtc_material raw_material(uint32_t pattern = 0) {
  rl_rtc_material m{};
  m.color[0] = m.color[1] = m.color[2] = 1.0, m.ambient = 0.1, m.diffuse = 0.9, m.specular = 0.9, m.shininess = 200.0, m.refractive_index = 1.0, m.pattern = pattern;
  return m;
}
static rl_rtc_triangle raw_triangle(double x) {
  rl_rtc_triangle t{};
  t.p1[0] = x, t.e1[0] = 1.0, t.e2[1] = 1.0, t.n1[2] = t.n2[2] = t.n3[2] = -1.0;
  return t;
}
// triangles only: the world the reduced kernel renders (needs_full stays false)
static CF triangle_world() {
  CF f;
  f.materials.push_back(raw_material());
  f.triangles.push_back(raw_triangle(0.0));
  f.objects.push_back(rl_oref{RL_O_TRIANGLE, 0});
  rl_rtc_light l{};
  l.position[1] = 10.0, l.intensity[0] = l.intensity[1] = l.intensity[2] = 1.0;
  f.lights.push_back(l);
  return f;
}
// two triangles and a Bounded -> Transformed -> patterned sphere in one Group
static CF mixed_world() {
  CF f = triangle_world();
  f.triangles.push_back(raw_triangle(2.0));
  rl_rtc_pattern pt{};
  pt.kind = RL_PAT_STRIPE, pt.a[0] = 1.0, pt.b[1] = 1.0;
  identity4(pt.inverse);
  f.patterns.push_back(pt);
  f.materials.push_back(raw_material(1));
  rl_rtc_shape sh{};
  sh.kind = RL_O_SPHERE, sh.material = 1;
  f.shapes.push_back(sh);
  rl_rtc_transformed tf{};
  identity4(tf.inverse), identity4(tf.inverse_transpose);
  tf.child = rl_oref{RL_O_SPHERE, 0};
  f.transformeds.push_back(tf);
  rl_rtc_bounded b{};
  for (int k = 0; k < 3; k++) b.minimum[k] = -1.0, b.maximum[k] = 1.0;
  b.child = rl_oref{RL_O_TRANSFORMED, 0};
  f.boundeds.push_back(b);
  f.group_items = {rl_oref{RL_O_TRIANGLE, 0}, rl_oref{RL_O_TRIANGLE, 1}, rl_oref{RL_O_BOUNDED, 0}};
  f.groups.push_back(rl_rtc_group{0, 3});
  f.objects = {rl_oref{RL_O_GROUP, 0}};
  return f;
}
// a Group of nine triangles in index order: one ROP_TRIS range long enough (>= 8) for build_rtc_guards to put a guard tree over it
static CF mesh_world() {
  CF f = triangle_world();
  f.triangles.clear();
  for (uint32_t k = 0; k < 9; k++) {
    f.triangles.push_back(raw_triangle(1.5 * k));
    f.group_items.push_back(rl_oref{RL_O_TRIANGLE, k});
  }
  f.groups.push_back(rl_rtc_group{0, 9});
  f.objects = {rl_oref{RL_O_GROUP, 0}};
  return f;
}
static CF shape_world() {  // one plain sphere
  CF f = triangle_world();
  f.triangles.clear();
  rl_rtc_shape sh{};
  sh.kind = RL_O_SPHERE, sh.material = 0;
  f.shapes.push_back(sh);
  f.objects = {rl_oref{RL_O_SPHERE, 0}};
  return f;
}

// every reference a description holds, in a fixed order
static std::vector<rl_href *> hrefs(RF &f) {
  std::vector<rl_href *> r{&f.root};
  for (auto &x : f.list_items) r.push_back(&x);
  for (auto &x : f.translates) r.push_back(&x.child);
  for (auto &x : f.transforms) r.push_back(&x.child);
  for (auto &x : f.bvh_nodes)
    for (uint32_t k = 0; k < x.n_children && k < 2; k++) r.push_back(&x.child[k]);
  for (auto &x : f.media) r.push_back(&x.boundary);
  return r;
}
static std::vector<rl_oref *> orefs(CF &f) {
  std::vector<rl_oref *> r;
  for (auto &x : f.objects) r.push_back(&x);
  for (auto &x : f.group_items) r.push_back(&x);
  for (auto &x : f.boundeds) r.push_back(&x.child);
  for (auto &x : f.transformeds) r.push_back(&x.child);
  for (auto &x : f.csgs) r.push_back(&x.left), r.push_back(&x.right);
  return r;
}
template <class R, class V>
static R *first_ref(V refs, uint32_t kind) {
  for (R *r : refs)
    if (r->kind == kind) return r;
  std::printf("FAIL base scene holds no reference of kind %u\n", kind);
  std::exit(2);
}
static rl_href &href_of(RF &f, uint32_t kind) { return *first_ref<rl_href>(hrefs(f), kind); }
static rl_oref &oref_of(CF &f, uint32_t kind) { return *first_ref<rl_oref>(orefs(f), kind); }
template <class T>
static T &first_of_kind(std::vector<T> &v, uint32_t kind) {
  for (T &x : v)
    if (x.kind == kind) return x;
  std::printf("FAIL base scene holds no record of kind %u\n", kind);
  std::exit(2);
}

struct Bases {
  RF smoke = flat(scenes::cornell_scene(true)), checkered = flat(scenes::checkered_spheres()), perlin = flat(scenes::perlin_scene(false)), image = image_world();
  CF csg = flat(scenes::rtc_test_csg_scene()), mirror = flat(scenes::rtc_test_mirror_scene()), mixed = mixed_world(), mesh = mesh_world();
};

// ============================================================================================ A: one case per refusal
template <class F, class Edit>
static void A(const char *name, const F &base, Edit edit) {
  F f = base;
  auto d = f.desc();
  edit(f, d);
  report(std::string("A.") + name, run(d));
}
// an edit of the records alone: the description is taken afterwards
template <class F, class Edit>
static void Ar(const char *name, const F &base, Edit edit) {
  F f = base;
  edit(f);
  report(std::string("A.") + name, run(f.desc()));
}

static void part_A(const Bases &B) {
  run_case("A.base.cornell_smoke", B.smoke), run_case("A.base.checkered_spheres", B.checkered), run_case("A.base.perlin_spheres", B.perlin);
  run_case("A.base.image", B.image), run_case("A.base.rtc_csg", B.csg), run_case("A.base.rtc_mirror", B.mirror), run_case("A.base.rtc_mixed", B.mixed);
  if (run_case("A.base.rtc_mesh", B.mesh).n_guards != 2 * 9 - 1) fail("A.base.rtc_mesh", "expected the 17 guards of a binary tree over 9 triangles");
  using D = rl_rtiow_scene_desc;
  A("rtiow.null.spheres", B.checkered, [](RF &, D &d) { d.spheres = nullptr; });
  A("rtiow.null.planars", B.smoke, [](RF &, D &d) { d.planars = nullptr; });
  A("rtiow.null.translates", B.smoke, [](RF &, D &d) { d.translates = nullptr; });
  A("rtiow.null.transforms", B.smoke, [](RF &, D &d) { d.transforms = nullptr; });
  A("rtiow.null.bvh_nodes", B.smoke, [](RF &, D &d) { d.bvh_nodes = nullptr; });
  A("rtiow.null.lists", B.smoke, [](RF &, D &d) { d.lists = nullptr; });
  A("rtiow.null.list_items", B.smoke, [](RF &, D &d) { d.list_items = nullptr; });
  A("rtiow.null.materials", B.smoke, [](RF &, D &d) { d.materials = nullptr; });
  A("rtiow.null.textures", B.smoke, [](RF &, D &d) { d.textures = nullptr; });
  A("rtiow.null.images", B.image, [](RF &, D &d) { d.images = nullptr; });
  A("rtiow.null.perlins", B.perlin, [](RF &, D &d) { d.perlins = nullptr; });
  A("rtiow.null.media", B.smoke, [](RF &, D &d) { d.media = nullptr; });
  A("rtiow.too_many_spheres", B.checkered, [](RF &, D &d) { d.n_spheres = rl::SPH_INDEX + 1; });
  Ar("rtiow.perlin_permutation", B.perlin, [](RF &f) { f.perlins[0].perm_y[7] = 256; });
  Ar("rtiow.image_no_data.width", B.image, [](RF &f) { f.images[0].width = 0; });
  Ar("rtiow.image_no_data.pixels", B.image, [](RF &f) { f.images[0].rgb = nullptr; });
  Ar("rtiow.checker_child", B.checkered, [](RF &f) { first_of_kind(f.textures, RL_TEX_CHECKER).odd = (uint32_t)f.textures.size(); });
  Ar("rtiow.image_index", B.image, [](RF &f) { first_of_kind(f.textures, RL_TEX_IMAGE).image = (uint32_t)f.images.size(); });
  Ar("rtiow.perlin_index", B.perlin, [](RF &f) { first_of_kind(f.textures, RL_TEX_NOISE).image = (uint32_t)f.perlins.size(); });
  Ar("rtiow.texture_kind", B.checkered, [](RF &f) { f.textures[0].kind = RL_TEX_NOISE + 1; });
  Ar("rtiow.checker_cycle", B.checkered, [](RF &f) {
    rl_texture &c = first_of_kind(f.textures, RL_TEX_CHECKER);
    c.even = (uint32_t)(&c - f.textures.data());
  });
  Ar("rtiow.material_kind", B.checkered, [](RF &f) { f.materials[0].kind = RL_MAT_ISOTROPIC + 1; });
  Ar("rtiow.material_texture", B.checkered, [](RF &f) { first_of_kind(f.materials, RL_MAT_LAMBERTIAN).texture = (uint32_t)f.textures.size(); });
  Ar("rtiow.sphere_material", B.checkered, [](RF &f) { f.spheres[0].material = (uint32_t)f.materials.size(); });
  Ar("rtiow.planar_material", B.smoke, [](RF &f) { f.planars[0].material = (uint32_t)f.materials.size(); });
  Ar("rtiow.planar_kind", B.smoke, [](RF &f) { f.planars[0].kind = RL_PLANAR_TRIANGLE + 1; });
  Ar("rtiow.sphere_index", B.checkered, [](RF &f) { href_of(f, RL_H_SPHERE).index = (uint32_t)f.spheres.size(); });
  Ar("rtiow.planar_index", B.smoke, [](RF &f) { href_of(f, RL_H_PLANAR).index = (uint32_t)f.planars.size(); });
  Ar("rtiow.translate_index", B.smoke, [](RF &f) { href_of(f, RL_H_TRANSLATE).index = (uint32_t)f.translates.size(); });
  Ar("rtiow.transform_index", B.smoke, [](RF &f) { href_of(f, RL_H_TRANSFORM).index = (uint32_t)f.transforms.size(); });
  Ar("rtiow.bvh_index", B.smoke, [](RF &f) { href_of(f, RL_H_BVH).index = (uint32_t)f.bvh_nodes.size(); });
  Ar("rtiow.list_index", B.smoke, [](RF &f) { href_of(f, RL_H_LIST).index = (uint32_t)f.lists.size(); });
  Ar("rtiow.medium_index", B.smoke, [](RF &f) { href_of(f, RL_H_MEDIUM).index = (uint32_t)f.media.size(); });
  Ar("rtiow.hittable_kind.none", B.checkered, [](RF &f) { f.root.kind = RL_H_NONE; });
  Ar("rtiow.hittable_kind.above", B.checkered, [](RF &f) { f.list_items[0].kind = RL_H_MEDIUM + 1; });
  Ar("rtiow.cycle_list", B.checkered, [](RF &f) { f.list_items[f.lists[f.root.index].first] = f.root; });
  Ar("rtiow.cycle_bvh", B.smoke, [](RF &f) { f.bvh_nodes[f.root.index].child[0] = f.root; });
  Ar("rtiow.cycle_instance", B.smoke, [](RF &f) { f.translates[0].child = rl_href{RL_H_TRANSLATE, 0}; });
  Ar("rtiow.medium_in_medium", B.smoke, [](RF &f) { f.media[0].boundary = rl_href{RL_H_MEDIUM, 1}; });
  Ar("rtiow.medium_in_itself", B.smoke, [](RF &f) { f.media[0].boundary = rl_href{RL_H_MEDIUM, 0}; });
  Ar("rtiow.list_range", B.smoke, [](RF &f) { f.lists[0].first = (uint32_t)f.list_items.size(); });
  Ar("rtiow.bvh_children.none", B.smoke, [](RF &f) { f.bvh_nodes[f.root.index].n_children = 0; });
  Ar("rtiow.bvh_children.three", B.smoke, [](RF &f) { f.bvh_nodes[f.root.index].n_children = 3; });
  Ar("rtiow.medium_material", B.smoke, [](RF &f) { f.media[0].material = (uint32_t)f.materials.size(); });

  using C = rl_rtc_scene_desc;
  A("rtc.null.triangles", B.mixed, [](CF &, C &d) { d.triangles = nullptr; });
  A("rtc.null.groups", B.mixed, [](CF &, C &d) { d.groups = nullptr; });
  A("rtc.null.group_items", B.mixed, [](CF &, C &d) { d.group_items = nullptr; });
  A("rtc.null.boundeds", B.mixed, [](CF &, C &d) { d.boundeds = nullptr; });
  A("rtc.null.transformeds", B.mixed, [](CF &, C &d) { d.transformeds = nullptr; });
  A("rtc.null.materials", B.mixed, [](CF &, C &d) { d.materials = nullptr; });
  A("rtc.null.objects", B.mixed, [](CF &, C &d) { d.objects = nullptr; });
  A("rtc.null.lights", B.mixed, [](CF &, C &d) { d.lights = nullptr; });
  A("rtc.null.shapes", B.mixed, [](CF &, C &d) { d.shapes = nullptr; });
  A("rtc.null.csgs", B.csg, [](CF &, C &d) { d.csgs = nullptr; });
  A("rtc.null.patterns", B.mixed, [](CF &, C &d) { d.patterns = nullptr; });
  Ar("rtc.triangle_material", B.mixed, [](CF &f) { f.triangles[1].material = (uint32_t)f.materials.size(); });
  Ar("rtc.shape_material", B.mirror, [](CF &f) { f.shapes[0].material = (uint32_t)f.materials.size(); });
  Ar("rtc.pattern_kind.none", B.mirror, [](CF &f) { f.patterns[0].kind = 0; });
  Ar("rtc.pattern_kind.above", B.mirror, [](CF &f) { f.patterns[0].kind = RL_PAT_CHECKER3D + 1; });
  Ar("rtc.material_pattern", B.mirror, [](CF &f) { f.materials[0].pattern = (uint32_t)f.patterns.size() + 1; });
  Ar("rtc.triangle_index", B.mixed, [](CF &f) { oref_of(f, RL_O_TRIANGLE).index = (uint32_t)f.triangles.size(); });
  Ar("rtc.group_index", B.mixed, [](CF &f) { oref_of(f, RL_O_GROUP).index = (uint32_t)f.groups.size(); });
  Ar("rtc.bounded_index", B.mixed, [](CF &f) { oref_of(f, RL_O_BOUNDED).index = (uint32_t)f.boundeds.size(); });
  Ar("rtc.transformed_index", B.mixed, [](CF &f) { oref_of(f, RL_O_TRANSFORMED).index = (uint32_t)f.transformeds.size(); });
  Ar("rtc.shape_index", B.mixed, [](CF &f) { oref_of(f, RL_O_SPHERE).index = (uint32_t)f.shapes.size(); });
  Ar("rtc.csg_index", B.csg, [](CF &f) { oref_of(f, RL_O_CSG).index = (uint32_t)f.csgs.size(); });
  Ar("rtc.shape_kind_mismatch", B.mixed, [](CF &f) { oref_of(f, RL_O_SPHERE).kind = RL_O_CUBE; });
  Ar("rtc.object_kind.none", B.mixed, [](CF &f) { f.objects[0].kind = RL_O_NONE; });
  Ar("rtc.object_kind.above", B.mixed, [](CF &f) { f.group_items[0].kind = RL_O_CSG + 1; });
  Ar("rtc.cycle_group", B.mixed, [](CF &f) { f.group_items[0] = rl_oref{RL_O_GROUP, 0}; });
  Ar("rtc.cycle_bounded", B.mixed, [](CF &f) { f.boundeds[0].child = rl_oref{RL_O_BOUNDED, 0}; });
  Ar("rtc.cycle_transformed", B.mixed, [](CF &f) { f.transformeds[0].child = rl_oref{RL_O_TRANSFORMED, 0}; });
  Ar("rtc.cycle_csg", B.csg, [](CF &f) { f.csgs[0].right = rl_oref{RL_O_CSG, 0}; });
  Ar("rtc.csg_operation", B.csg, [](CF &f) { f.csgs[0].operation = RL_CSG_DIFFERENCE + 1; });
  Ar("rtc.group_range", B.mixed, [](CF &f) { f.groups[0].first = (uint32_t)f.group_items.size(); });
}

// ============================================================================================ B: every cap from both sides
static RF instance_chain(uint32_t depth) {  // Translate and Transform alternating around one sphere
  RF f = sphere_world();
  rl_href inner{RL_H_SPHERE, 0};
  for (uint32_t k = 0; k < depth; k++) {
    if (k % 2 == 0) {
      rl_translate t{};
      t.offset[0] = 0.25, t.child = inner;
      f.translates.push_back(t);
      inner = rl_href{RL_H_TRANSLATE, (uint32_t)f.translates.size() - 1};
    } else {
      rl_transform t{};
      for (int i = 0; i < 9; i += 4) t.m[i] = t.inv[i] = t.inv_t[i] = 1.0;
      t.child = inner;
      f.transforms.push_back(t);
      inner = rl_href{RL_H_TRANSFORM, (uint32_t)f.transforms.size() - 1};
    }
  }
  f.list_items[0] = inner;
  return f;
}
static RF checker_chain(uint32_t depth) {  // texture i = Checker(i + 1, i + 1) ... Solid at the end; the sphere's material shows texture 0
  RF f = sphere_world();
  f.textures.clear();
  for (uint32_t k = 0; k < depth; k++) {
    rl_texture t{};
    t.kind = RL_TEX_CHECKER, t.even = t.odd = k + 1, t.inv_scale = 1.0;
    f.textures.push_back(t);
  }
  rl_texture s{};
  s.kind = RL_TEX_SOLID;
  f.textures.push_back(s);
  return f;
}
static CF transformed_chain(uint32_t depth) {
  CF f = shape_world();
  rl_oref inner{RL_O_SPHERE, 0};
  for (uint32_t k = 0; k < depth; k++) {
    rl_rtc_transformed t{};
    identity4(t.inverse), identity4(t.inverse_transpose);
    t.child = inner;
    f.transformeds.push_back(t);
    inner = rl_oref{RL_O_TRANSFORMED, k};
  }
  f.objects = {inner};
  return f;
}
static CF csg_chain(uint32_t depth) {
  CF f = shape_world();
  rl_oref inner{RL_O_SPHERE, 0};
  for (uint32_t k = 0; k < depth; k++) {
    rl_rtc_csg c{};
    c.operation = RL_CSG_UNION, c.left = inner, c.right = rl_oref{RL_O_SPHERE, 0};
    f.csgs.push_back(c);
    inner = rl_oref{RL_O_CSG, k};
  }
  f.objects = {inner};
  return f;
}

static void part_B(const Bases &B) {
  expect_ops("B.instances.8", run_case("B.instances.8", instance_chain(8)), 8 * 2 + 2);
  run_case("B.instances.9", instance_chain(9));
  run_case("B.checker.32", checker_chain(32));
  run_case("B.checker.33", checker_chain(33));
  expect_ops("B.transformed.8", run_case("B.transformed.8", transformed_chain(8)), 8 * 2 + 2);
  run_case("B.transformed.9", transformed_chain(9));
  expect_ops("B.csg.4", run_case("B.csg.4", csg_chain(4)), 4 * 4 + 2);
  run_case("B.csg.5", csg_chain(5));
  for (uint32_t n : {0xFFFFu, 0x10000u}) {
    CF f = triangle_world();
    f.lights.assign(n, f.lights[0]);
    run_case(n == 0xFFFFu ? "B.lights.65535" : "B.lights.65536", f);
  }
  for (uint32_t depth : {7u, 8u}) {
    CF full = B.mirror, reduced = triangle_world();
    full.max_reflection_depth = reduced.max_reflection_depth = depth;
    run_case("B.reflection_depth." + std::to_string(depth) + ".full_kernel", full);
    if (depth == 8) run_case("B.reflection_depth.8.reduced_kernel", reduced);
  }
  {
    RF f = B.checkered;
    rl_rtiow_scene_desc d = f.desc();
    d.n_spheres = rl::SPH_INDEX + 1;  // refused before a record is read; SPH_INDEX itself: see the head of this file
    report("B.spheres.above_index_field", run(d));
  }
  for (int k = 0; k < 3; k++) {  // a range that ends at the item count, one past it, and one whose end wraps 32 bits
    const char *names[3] = {"at_end", "past_end", "wraps"};
    RF f = image_world();  // two items
    CF g = mixed_world();  // three items
    f.lists[0] = k == 0 ? rl_list{1, 1} : (k == 1 ? rl_list{1, 2} : rl_list{0xFFFFFFFFu, 2});
    g.groups[0] = k == 0 ? rl_rtc_group{1, 2} : (k == 1 ? rl_rtc_group{1, 3} : rl_rtc_group{0xFFFFFFFFu, 2});
    run_case(std::string("B.list_range.") + names[k], f);
    run_case(std::string("B.group_range.") + names[k], g);
  }
}

// ============================================================================================ C: depth, on a 1 MiB stack
static void on_small_stack(const std::function<void()> &body) {
  pthread_attr_t attr;
  pthread_attr_init(&attr);
  pthread_attr_setstacksize(&attr, 1u << 20);
  pthread_t th;
  auto tramp = [](void *p) -> void * {
    (*static_cast<const std::function<void()> *>(p))();
    return nullptr;
  };
  if (pthread_create(&th, &attr, tramp, const_cast<std::function<void()> *>(&body)) != 0) {
    fail("C", "pthread_create");
    return;
  }
  pthread_join(th, nullptr);
  pthread_attr_destroy(&attr);
}
// n lists, each holding the next; the last holds the sphere: the sphere's reference sits at depth n
static RF list_chain(uint32_t n) {
  RF f = sphere_world();
  f.lists.clear(), f.list_items.clear();
  for (uint32_t k = 0; k < n; k++) {
    f.lists.push_back(rl_list{k, 1});
    f.list_items.push_back(k + 1 < n ? rl_href{RL_H_LIST, k + 1} : rl_href{RL_H_SPHERE, 0});
  }
  return f;
}
// n one-child BVH nodes; the last is the leaf that holds the sphere: that node's reference sits at depth n - 1
static RF bvh_chain(uint32_t n) {
  RF f = sphere_world();
  f.lists.clear(), f.list_items.clear();
  for (uint32_t k = 0; k < n; k++) {
    rl_bvh_node nd{};
    for (int a = 0; a < 3; a++) nd.bbox[2 * a] = -2.0, nd.bbox[2 * a + 1] = 2.0;
    nd.n_children = 1, nd.child[0] = k + 1 < n ? rl_href{RL_H_BVH, k + 1} : rl_href{RL_H_SPHERE, 0};
    f.bvh_nodes.push_back(nd);
  }
  f.root = rl_href{RL_H_BVH, 0};
  return f;
}
static CF group_chain(uint32_t n) {  // as list_chain
  CF f = shape_world();
  for (uint32_t k = 0; k < n; k++) {
    f.groups.push_back(rl_rtc_group{k, 1});
    f.group_items.push_back(k + 1 < n ? rl_oref{RL_O_GROUP, k + 1} : rl_oref{RL_O_SPHERE, 0});
  }
  f.objects = {rl_oref{RL_O_GROUP, 0}};
  return f;
}
static CF bounded_chain(uint32_t n) {  // the shape's reference sits at depth n
  CF f = shape_world();
  for (uint32_t k = 0; k < n; k++) {
    rl_rtc_bounded b{};
    for (int a = 0; a < 3; a++) b.minimum[a] = -1.0, b.maximum[a] = 1.0;
    b.child = k + 1 < n ? rl_oref{RL_O_BOUNDED, k + 1} : rl_oref{RL_O_SPHERE, 0};
    f.boundeds.push_back(b);
  }
  f.objects = {rl_oref{RL_O_BOUNDED, 0}};
  return f;
}

static void part_C(const std::string &only) {
  const uint32_t N = RL_SCENE_MAX_NEST;
  if (only != "checkers")
    on_small_stack([&] {
      expect_ops("C.lists.at_max_nest", run_case("C.lists.at_max_nest", list_chain(N)), 2);
      run_case("C.lists.one_deeper", list_chain(N + 1));
    });
  if (only != "lists") on_small_stack([&] { run_case("C.checkers.2000000", checker_chain(2000000)); });
  if (!only.empty()) return;
  on_small_stack([&] {
    expect_ops("C.bvh.at_max_nest", run_case("C.bvh.at_max_nest", bvh_chain(N + 1)), N + 2);
    run_case("C.bvh.one_deeper", bvh_chain(N + 2));
    expect_ops("C.groups.at_max_nest", run_case("C.groups.at_max_nest", group_chain(N)), 2);
    run_case("C.groups.one_deeper", group_chain(N + 1));
    expect_ops("C.boundeds.at_max_nest", run_case("C.boundeds.at_max_nest", bounded_chain(N)), N + 2);
    run_case("C.boundeds.one_deeper", bounded_chain(N + 1));
  });
}

// ============================================================================================ D: sharing
// level i names level i + 1 twice; the last level holds `leaf` things
static RF doubling_lists(uint32_t levels, bool empty_leaf) {
  RF f = sphere_world();
  f.lists.clear(), f.list_items.clear();
  for (uint32_t k = 0; k < levels; k++) {
    f.lists.push_back(rl_list{2 * k, 2});
    f.list_items.push_back(rl_href{RL_H_LIST, k + 1}), f.list_items.push_back(rl_href{RL_H_LIST, k + 1});
  }
  f.lists.push_back(rl_list{2 * levels, empty_leaf ? 0u : 1u});
  f.list_items.push_back(rl_href{RL_H_SPHERE, 0});
  return f;
}
static CF doubling_groups(uint32_t levels, bool empty_leaf) {
  CF f = shape_world();
  for (uint32_t k = 0; k < levels; k++) {
    f.groups.push_back(rl_rtc_group{2 * k, 2});
    f.group_items.push_back(rl_oref{RL_O_GROUP, k + 1}), f.group_items.push_back(rl_oref{RL_O_GROUP, k + 1});
  }
  f.groups.push_back(rl_rtc_group{2 * levels, empty_leaf ? 0u : 1u});
  f.group_items.push_back(rl_oref{RL_O_SPHERE, 0});
  f.objects = {rl_oref{RL_O_GROUP, 0}};
  return f;
}
// Work that emits nothing must not be repeated with every expansion of its parent.  Both graphs double 20 times (2^20 expansions of
// the last level) and compile to 2^20 ops + the end op; the compiler that walked them naively would take 2^38 / 5 * 10^10 steps.
//   empties:  the last level holds the sphere and 2^18 references to an empty list
//   wrappers: the last level reaches the sphere through a chain of 50000 lists of one item each
static RF doubling_lists_with_empties(uint32_t levels, uint32_t empties) {
  RF f = doubling_lists(levels, false);
  f.lists.push_back(rl_list{0, 0});
  const uint32_t empty = (uint32_t)f.lists.size() - 1;
  for (uint32_t k = 0; k < empties; k++) f.list_items.push_back(rl_href{RL_H_LIST, empty});
  f.lists[levels].count = 1 + empties;
  return f;
}
static CF doubling_groups_with_empties(uint32_t levels, uint32_t empties) {
  CF f = doubling_groups(levels, false);
  f.groups.push_back(rl_rtc_group{0, 0});
  const uint32_t empty = (uint32_t)f.groups.size() - 1;
  for (uint32_t k = 0; k < empties; k++) f.group_items.push_back(rl_oref{RL_O_GROUP, empty});
  f.groups[levels].count = 1 + empties;
  return f;
}
static RF doubling_lists_over_wrappers(uint32_t levels, uint32_t chain) {
  RF f = doubling_lists(levels, false);
  for (uint32_t k = 0; k < chain; k++) {  // wrapper k holds wrapper k + 1, the last one the sphere
    const uint32_t item = (uint32_t)f.list_items.size(), next = (uint32_t)f.lists.size() + 1;
    f.list_items.push_back(k + 1 < chain ? rl_href{RL_H_LIST, next} : rl_href{RL_H_SPHERE, 0});
    f.lists.push_back(rl_list{item, 1});
  }
  f.list_items[2 * levels] = rl_href{RL_H_LIST, levels + 1};  // the last level's one item: the first wrapper
  return f;
}
static CF doubling_groups_over_wrappers(uint32_t levels, uint32_t chain) {
  CF f = doubling_groups(levels, false);
  for (uint32_t k = 0; k < chain; k++) {
    const uint32_t item = (uint32_t)f.group_items.size(), next = (uint32_t)f.groups.size() + 1;
    f.group_items.push_back(k + 1 < chain ? rl_oref{RL_O_GROUP, next} : rl_oref{RL_O_SPHERE, 0});
    f.groups.push_back(rl_rtc_group{item, 1});
  }
  f.group_items[2 * levels] = rl_oref{RL_O_GROUP, levels + 1};
  return f;
}
// a list that expands to exactly `ops` sphere ops: the levels of a 30-level doubling graph picked by the bits of `ops`
static RF exact_ops(uint32_t ops) {
  RF f = doubling_lists(30, false);  // list k expands to 2^(30 - k) ops
  const uint32_t first = (uint32_t)f.list_items.size();
  for (uint32_t k = 0; k <= 30; k++)
    if (ops >> (30 - k) & 1u) f.list_items.push_back(rl_href{RL_H_LIST, k});
  f.lists.push_back(rl_list{first, (uint32_t)f.list_items.size() - first});
  f.root = rl_href{RL_H_LIST, (uint32_t)f.lists.size() - 1};
  return f;
}
static void part_D() {
  run_case("D.rtiow.ops_at_limit", exact_ops(RL_SCENE_MAX_OPS - 1));  // + the end op = RL_SCENE_MAX_OPS: one too many
  run_case("D.rtiow.60_levels.sphere", doubling_lists(60, false));
  run_case("D.rtc.60_levels.sphere", doubling_groups(60, false));
  // a graph that expands to nothing is a valid (empty) world, as an empty list is: accepted, the program is its end op alone
  expect_ops("D.rtiow.60_levels.empty", run_case("D.rtiow.60_levels.empty", doubling_lists(60, true)), 1);
  expect_ops("D.rtc.60_levels.empty", run_case("D.rtc.60_levels.empty", doubling_groups(60, true)), 1);
  expect_ops("D.rtiow.20_levels.sphere", run_case("D.rtiow.20_levels.sphere", doubling_lists(20, false)), (1u << 20) + 1);
  expect_ops("D.rtc.20_levels.sphere", run_case("D.rtc.20_levels.sphere", doubling_groups(20, false)), (1u << 20) + 1);
  expect_ops("D.rtiow.20_levels.sphere_and_empties", run_case("D.rtiow.20_levels.sphere_and_empties", doubling_lists_with_empties(20, 1u << 18)), (1u << 20) + 1);
  expect_ops("D.rtc.20_levels.sphere_and_empties", run_case("D.rtc.20_levels.sphere_and_empties", doubling_groups_with_empties(20, 1u << 18)), (1u << 20) + 1);
  expect_ops("D.rtiow.20_levels.wrappers", run_case("D.rtiow.20_levels.wrappers", doubling_lists_over_wrappers(20, 50000)), (1u << 20) + 1);
  expect_ops("D.rtc.20_levels.wrappers", run_case("D.rtc.20_levels.wrappers", doubling_groups_over_wrappers(20, 50000)), (1u << 20) + 1);
}
static void part_D_nomem() {
  struct rlimit lim {1ull << 30, 1ull << 30};
  if (setrlimit(RLIMIT_AS, &lim) != 0) fail("D.nomem", "setrlimit");
  run_case("D.nomem.rtiow.27_levels", doubling_lists(27, false));  // 2^27 ops = 8 GiB: under the op limit, far over the memory
  run_case("D.nomem.rtc.27_levels", doubling_groups(27, false));
  run_case("D.nomem.rtiow.ops_below_limit", exact_ops(RL_SCENE_MAX_OPS - 2));  // the largest program the op limit admits (128 GiB)
}

// ============================================================================================ E: exhaustive single-field mutation
enum Class { INDEX_TOO_LARGE, INDEX_OTHER, KIND_UNKNOWN, KIND_OTHER, COUNT_ZERO, COUNT_TOO_LARGE, COUNT_GROWN, NULL_ARRAY, N_CLASSES };
static const char *CLASS_NAMES[N_CLASSES] = {"index_too_large", "index_other_valid", "kind_unknown", "kind_other_valid", "count_zero", "count_too_large", "count_grown", "null_array"};
struct Tally {
  unsigned long applied[N_CLASSES] = {}, refused[N_CLASSES] = {};
  std::map<std::pair<int, std::string>, std::pair<unsigned long, unsigned long>> per_table;  // (class, table) -> applied, refused
};
struct Field {  // one uint32 of the records
  uint32_t *p;
  bool is_kind;
  std::string table;     // index: the table it indexes; kind: the table that holds it
  uint32_t lo, n;        // index: valid values are [0, n); kind: valid values are [lo, n)
};
static void note(Tally &t, const std::string &scene, Class c, const std::string &table, const Outcome &o, const std::string &what) {
  if (!well_formed(o)) {
    std::printf("case E.%s.%s | %d | %d | %s | %s\n", scene.c_str(), what.c_str(), o.rc, o.out_null ? 1 : 0, o.err.c_str(), o.facts.c_str());
    fail("E." + scene + "." + what, "outcome is neither a clean refusal nor a checked program");
  }
  t.applied[c]++, t.per_table[{c, table}].first++;
  if (o.rc != RL_OK) t.refused[c]++, t.per_table[{c, table}].second++;
}
static const char *rtiow_table(uint32_t kind) {
  static const char *names[] = {"?", "spheres", "planars", "translates", "transforms", "bvh_nodes", "lists", "media"};
  return kind <= RL_H_MEDIUM ? names[kind] : "?";
}
static uint32_t rtiow_size(const RF &f, uint32_t kind) {
  const size_t sizes[] = {0, f.spheres.size(), f.planars.size(), f.translates.size(), f.transforms.size(), f.bvh_nodes.size(), f.lists.size(), f.media.size()};
  return kind <= RL_H_MEDIUM ? (uint32_t)sizes[kind] : 0u;
}
static std::vector<Field> fields(RF &f) {
  std::vector<Field> r;
  for (rl_href *h : hrefs(f)) {
    r.push_back(Field{&h->kind, true, "hrefs", RL_H_SPHERE, RL_H_MEDIUM + 1});
    r.push_back(Field{&h->index, false, rtiow_table(h->kind), 0, rtiow_size(f, h->kind)});
  }
  const uint32_t nm = (uint32_t)f.materials.size(), nt = (uint32_t)f.textures.size();
  for (auto &x : f.spheres) r.push_back(Field{&x.material, false, "materials", 0, nm});
  for (auto &x : f.planars) r.push_back(Field{&x.material, false, "materials", 0, nm}), r.push_back(Field{&x.kind, true, "planars", 0, RL_PLANAR_TRIANGLE + 1});
  for (auto &x : f.media) r.push_back(Field{&x.material, false, "materials", 0, nm});
  for (auto &x : f.materials) {
    r.push_back(Field{&x.kind, true, "materials", 0, RL_MAT_ISOTROPIC + 1});
    if (x.kind == RL_MAT_LAMBERTIAN || x.kind == RL_MAT_DIFFUSE_LIGHT || x.kind == RL_MAT_ISOTROPIC) r.push_back(Field{&x.texture, false, "textures", 0, nt});
  }
  for (auto &x : f.textures) {
    r.push_back(Field{&x.kind, true, "textures", 0, RL_TEX_NOISE + 1});
    if (x.kind == RL_TEX_CHECKER) r.push_back(Field{&x.even, false, "textures", 0, nt}), r.push_back(Field{&x.odd, false, "textures", 0, nt});
    if (x.kind == RL_TEX_IMAGE) r.push_back(Field{&x.image, false, "images", 0, (uint32_t)f.images.size()});
    if (x.kind == RL_TEX_NOISE) r.push_back(Field{&x.image, false, "perlins", 0, (uint32_t)f.perlins.size()});
  }
  for (auto &x : f.lists) r.push_back(Field{&x.first, false, "list_items", 0, (uint32_t)f.list_items.size() + 1});  // first == n is valid for an empty list
  return r;
}
static const char *rtc_table(uint32_t kind) {
  static const char *names[] = {"?", "triangles", "groups", "boundeds", "transformeds", "shapes", "shapes", "shapes", "shapes", "shapes", "csgs"};
  return kind <= RL_O_CSG ? names[kind] : "?";
}
static uint32_t rtc_size(const CF &f, uint32_t kind) {
  const size_t s = f.shapes.size(), sizes[] = {0, f.triangles.size(), f.groups.size(), f.boundeds.size(), f.transformeds.size(), s, s, s, s, s, f.csgs.size()};
  return kind <= RL_O_CSG ? (uint32_t)sizes[kind] : 0u;
}
static std::vector<Field> fields(CF &f) {
  std::vector<Field> r;
  for (rl_oref *o : orefs(f)) {
    r.push_back(Field{&o->kind, true, "orefs", RL_O_TRIANGLE, RL_O_CSG + 1});
    r.push_back(Field{&o->index, false, rtc_table(o->kind), 0, rtc_size(f, o->kind)});
  }
  const uint32_t nm = (uint32_t)f.materials.size();
  for (auto &x : f.triangles) r.push_back(Field{&x.material, false, "materials", 0, nm});
  for (auto &x : f.shapes) r.push_back(Field{&x.material, false, "materials", 0, nm}), r.push_back(Field{&x.kind, true, "shapes", RL_O_SPHERE, RL_O_CONE + 1});
  for (auto &x : f.materials) r.push_back(Field{&x.pattern, false, "patterns", 0, (uint32_t)f.patterns.size() + 1});  // 1-based, 0 = none
  for (auto &x : f.patterns) r.push_back(Field{&x.kind, true, "patterns", RL_PAT_STRIPE, RL_PAT_CHECKER3D + 1});
  for (auto &x : f.csgs) r.push_back(Field{&x.operation, true, "csgs", 0, RL_CSG_DIFFERENCE + 1});
  for (auto &x : f.groups) r.push_back(Field{&x.first, false, "group_items", 0, (uint32_t)f.group_items.size() + 1});
  return r;
}
// the counts a compiler can judge (see the head of this file)
static std::vector<std::pair<uint32_t *, std::string>> inner_counts(RF &f) {
  std::vector<std::pair<uint32_t *, std::string>> r;
  for (auto &x : f.lists) r.push_back({&x.count, "lists"});
  for (auto &x : f.bvh_nodes) r.push_back({&x.n_children, "bvh_nodes"});
  return r;
}
static std::vector<std::pair<uint32_t *, std::string>> inner_counts(CF &f) {
  std::vector<std::pair<uint32_t *, std::string>> r;
  for (auto &x : f.groups) r.push_back({&x.count, "groups"});
  return r;
}
// the arrays of a description: mutate(desc, which, how) with how 0: count = 0, 1: pointer = null; grow(records, which): one more zeroed record
struct ArrayRef {
  std::string table;
  const void **ptr;
  uint32_t *count;
};
#define ARR(d, ptr_field, count_field) ArrayRef{#ptr_field, (const void **)&(d).ptr_field, &(d).count_field}
static std::vector<ArrayRef> arrays(rl_rtiow_scene_desc &d) {
  return {ARR(d, spheres, n_spheres), ARR(d, planars, n_planars), ARR(d, translates, n_translates), ARR(d, transforms, n_transforms),
          ARR(d, bvh_nodes, n_bvh_nodes), ARR(d, lists, n_lists), ARR(d, list_items, n_list_items), ARR(d, materials, n_materials),
          ARR(d, textures, n_textures), ARR(d, images, n_images), ARR(d, perlins, n_perlins), ARR(d, media, n_media)};
}
static std::vector<ArrayRef> arrays(rl_rtc_scene_desc &d) {
  return {ARR(d, triangles, n_triangles), ARR(d, groups, n_groups), ARR(d, group_items, n_group_items), ARR(d, boundeds, n_boundeds),
          ARR(d, transformeds, n_transformeds), ARR(d, materials, n_materials), ARR(d, objects, n_objects), ARR(d, lights, n_lights),
          ARR(d, shapes, n_shapes), ARR(d, csgs, n_csgs), ARR(d, patterns, n_patterns)};
}
static void grow(RF &f, size_t which) {
  switch (which) {
    case 0: f.spheres.emplace_back(); break;
    case 1: f.planars.emplace_back(); break;
    case 2: f.translates.emplace_back(); break;
    case 3: f.transforms.emplace_back(); break;
    case 4: f.bvh_nodes.emplace_back(); break;
    case 5: f.lists.emplace_back(); break;
    case 6: f.list_items.emplace_back(); break;
    case 7: f.materials.emplace_back(); break;
    case 8: f.textures.emplace_back(); break;
    case 9: f.images.emplace_back(); break;
    case 10: f.perlins.emplace_back(); break;
    default: f.media.emplace_back(); break;
  }
}
static void grow(CF &f, size_t which) {
  switch (which) {
    case 0: f.triangles.emplace_back(); break;
    case 1: f.groups.emplace_back(); break;
    case 2: f.group_items.emplace_back(); break;
    case 3: f.boundeds.emplace_back(); break;
    case 4: f.transformeds.emplace_back(); break;
    case 5: f.materials.emplace_back(); break;
    case 6: f.objects.emplace_back(); break;
    case 7: f.lights.emplace_back(); break;
    case 8: f.shapes.emplace_back(); break;
    case 9: f.csgs.emplace_back(); break;
    default: f.patterns.emplace_back(); break;
  }
}

template <class F>
static void mutate_scene(const std::string &scene, const F &base, bool is_rtiow) {
  Tally t;
  const auto t0 = std::chrono::steady_clock::now();
  F probe = base;
  const size_t n_fields = fields(probe).size();
  for (size_t fi = 0; fi < n_fields; fi++) {
    const Field f0 = fields(probe)[fi];
    const uint32_t cur = *f0.p;
    std::vector<std::pair<uint32_t, Class>> values;
    if (f0.is_kind) {
      values.push_back({0u, f0.lo > 0 ? KIND_UNKNOWN : KIND_OTHER});
      values.push_back({f0.n, KIND_UNKNOWN});
      for (uint32_t v = std::max(f0.lo, 1u); v < f0.n; v++) values.push_back({v, KIND_OTHER});
    } else {
      values.push_back({f0.n, INDEX_TOO_LARGE}), values.push_back({f0.n + 1, INDEX_TOO_LARGE}), values.push_back({0xFFFFFFFFu, INDEX_TOO_LARGE});
      for (uint32_t v = 0; v < f0.n; v++) values.push_back({v, INDEX_OTHER});
    }
    for (auto &vc : values) {
      if (vc.first == cur) continue;  // not a mutation
      F m = base;
      *fields(m)[fi].p = vc.first;
      note(t, scene, vc.second, f0.table, run(m.desc()), "field" + std::to_string(fi) + "=" + std::to_string(vc.first));
    }
  }
  const size_t n_counts = inner_counts(probe).size();
  for (size_t ci = 0; ci < n_counts; ci++) {
    const uint32_t cur = *inner_counts(probe)[ci].first;
    const std::string table = inner_counts(probe)[ci].second;
    for (uint32_t v : {0u, cur + 1u, 0xFFFFFFFFu}) {
      F m = base;
      *inner_counts(m)[ci].first = v;
      note(t, scene, v == 0 ? COUNT_ZERO : COUNT_TOO_LARGE, table, run(m.desc()), "count" + std::to_string(ci) + "=" + std::to_string(v));
    }
  }
  {
    auto d0 = probe.desc();
    const size_t n_arrays = arrays(d0).size();
    for (size_t ai = 0; ai < n_arrays; ai++) {
      const std::string table = arrays(d0)[ai].table;
      const bool filled = *arrays(d0)[ai].count != 0;
      if (filled) {
        auto d = probe.desc();
        *arrays(d)[ai].count = 0;
        note(t, scene, COUNT_ZERO, table, run(d), "n_" + table + "=0");
        d = probe.desc();
        *arrays(d)[ai].ptr = nullptr;
        note(t, scene, NULL_ARRAY, table, run(d), table + "=null");
      }
      F m = base;
      grow(m, ai);
      note(t, scene, COUNT_GROWN, table, run(m.desc()), "n_" + table + "+1");
      if (is_rtiow && ai == 0) {
        auto d = probe.desc();
        *arrays(d)[ai].count = 0xFFFFFFFFu;
        note(t, scene, COUNT_TOO_LARGE, table, run(d), "n_spheres=0xFFFFFFFF");
      }
    }
  }
  const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  unsigned long all = 0;
  for (int c = 0; c < N_CLASSES; c++) all += t.applied[c];
  std::printf("E %s: %lu mutations", scene.c_str(), all);
  for (int c = 0; c < N_CLASSES; c++) std::printf(", %s %lu (%lu refused)", CLASS_NAMES[c], t.applied[c], t.refused[c]);
  std::printf("\nEtime %s: %.0f ms\n", scene.c_str(), ms);
  // neither branch vacuous
  for (auto &kv : t.per_table) {
    const int c = kv.first.first;
    if ((c == INDEX_TOO_LARGE || c == KIND_UNKNOWN || c == COUNT_TOO_LARGE || c == NULL_ARRAY) && kv.second.second == 0)
      fail("E." + scene, std::string(CLASS_NAMES[c]) + " on " + kv.first.second + ": " + std::to_string(kv.second.first) + " mutations, none refused");
    if ((c == INDEX_TOO_LARGE || c == KIND_UNKNOWN || c == NULL_ARRAY) && kv.second.second != kv.second.first)
      fail("E." + scene, std::string(CLASS_NAMES[c]) + " on " + kv.first.second + ": " + std::to_string(kv.second.first - kv.second.second) + " mutations accepted");
  }
  if (t.applied[INDEX_OTHER] == t.refused[INDEX_OTHER]) fail("E." + scene, "no other valid index was accepted");
}

static void part_E(const Bases &B) {
  mutate_scene("cornell_smoke", B.smoke, true), mutate_scene("checkered_spheres", B.checkered, true), mutate_scene("perlin_spheres", B.perlin, true);
  mutate_scene("image", B.image, true), mutate_scene("rtc_csg", B.csg, false), mutate_scene("rtc_mirror", B.mirror, false), mutate_scene("rtc_mixed", B.mixed, false);
  mutate_scene("rtc_mesh", B.mesh, false);
}

int main(int argc, char **argv) {
  const std::string mode = argc > 1 ? argv[1] : "all";
  const auto t0 = std::chrono::steady_clock::now();
  if (mode == "nomem") {
    part_D_nomem();
  } else if (mode == "lists" || mode == "checkers") {  // one case the recursive compiler died of per run (`nomem` is the third)
    part_C(mode);
  } else {
    Bases B;
    part_A(B), part_B(B), part_C(""), part_D(), part_E(B);
  }
  std::printf("wall %.1f s\n", std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
  return failures ? 1 : 0;
}
