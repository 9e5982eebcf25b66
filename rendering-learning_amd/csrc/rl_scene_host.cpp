// The host scene compiler (rl_scene_host.h): from a scene description to everything the kernels walk — the linked and guarded
// successor words of the wave kernel, the flattened sphere materials, the fast trees' leaf boxes and balls, the RTC triangle guards —
// and the self-check of those structures.  Index arithmetic on caller-supplied graphs throughout; no device, no HIP runtime.
#include "rl_scene_host.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <new>
#include <stdexcept>

namespace rl {

// Sphere::bounding_box (sphere.rs:77-88): per axis the union over time of centre -/+ |radius|
static void swept_bounds(const rl_sphere &sp, double lo[3], double hi[3]) {
  const double r = std::fabs(sp.radius);
  for (int ax = 0; ax < 3; ax++) {
    double c0 = sp.center0[ax], c1 = sp.moving ? sp.center1[ax] : sp.center0[ax];
    lo[ax] = std::fmin(c0, c1) - r, hi[ax] = std::fmax(c0, c1) + r;
  }
}

// Linked form of a sphere-only program for the wave kernel: every op keeps its box and a, b, but {code, skip}
// become {w_hit, w_miss} = (state the lane enters there) << 29 | (op index): BOX hit -> op i+1, BOX_SPH hit ->
// the same op in LEAF, miss / leaf done -> op `skip`; a target that is OP_END means "SHADE", a bare OP_SPHERE
// "LEAF".  Boxes that are not BOX_FINITE are stored as NaN so the filtered test can never call them certain.
//
// guards != nullptr: every sphere additionally gets a GUARD op at index n_ops + sphere — the sphere's own bounding box
// (sphere.rs:77-88), tested by the same filter in a TRAV step but only ever used to REJECT (not one of the reference's
// tests, not counted) — and a guard leads to a LEAF visit of that ONE sphere:
//     leaf box hit -> guard(a) -> [LEAF a] -> guard(b) -> [LEAF b] -> the leaf's skip target.
// A ray that certainly misses a sphere's box certainly misses the sphere, so the expensive binary64 Sphere::hit is skipped
// for it (65 % of the leaf visits of BASELINE configs[1] end without a new closest hit).  Needs every sphere to be
// referenced exactly once (*guards_ok = false otherwise).
static uint32_t link_ops(const std::vector<DevOp> &ops, std::vector<DevOp> &out, const rl_rtiow_scene_desc *guards = nullptr, bool *guards_ok = nullptr,
                         const GuardFrame *frame = nullptr) {
  const uint32_t n0 = (uint32_t)ops.size();
  if (guards) {
    std::vector<uint8_t> seen(guards->n_spheres, 0);
    bool ok = true;
    for (uint32_t i = 0; i < n0 && ok; i++) {
      uint32_t kind = ops[i].code & 0xFFu;
      if (kind != OP_BOX_SPH && kind != OP_SPHERE) continue;
      for (uint32_t payload : {ops[i].a, ops[i].b}) {
        if (payload == NONE) continue;
        uint32_t sidx = payload & SPH_INDEX;
        if (seen[sidx]) ok = false;
        seen[sidx] = 1;
      }
    }
    if (guards_ok) *guards_ok = ok;
    if (!ok) guards = nullptr;
  }
  auto guard_of = [&](uint32_t payload) { return n0 + (payload & SPH_INDEX); };
  auto entry = [&](uint32_t t) -> uint32_t {
    uint32_t kind = ops[t].code & 0xFFu;
    if (guards && kind == OP_SPHERE) return (ST_TRAV << 29) | guard_of(ops[t].a);
    uint32_t st = kind == OP_END ? ST_SHADE : (kind == OP_SPHERE ? ST_LEAF : ST_TRAV);
    return (st << 29) | t;
  };
  out = ops;
  const double qnan = std::numeric_limits<double>::quiet_NaN();
  for (size_t i = 0; i < ops.size(); i++) {
    uint32_t kind = ops[i].code & 0xFFu;
    if (kind == OP_END) continue;
    DevOp &L = out[i];
    L.skip = entry(ops[i].skip);
    if (kind == OP_BOX) L.code = entry((uint32_t)i + 1u);
    else if (kind == OP_BOX_SPH) L.code = guards ? ((ST_TRAV << 29) | guard_of(ops[i].a)) : ((ST_LEAF << 29) | (uint32_t)i);
    else L.code = L.skip;  // OP_SPHERE: never stepped in TRAV
    if ((kind == OP_BOX || kind == OP_BOX_SPH) && !(ops[i].code & BOX_FINITE))
      for (double &b : L.box) b = qnan;
  }
  if (guards) {
    DevOp none{};
    for (double &b : none.box) b = qnan;
    none.code = none.skip = ST_SHADE << 29;
    none.a = none.b = NONE;
    out.resize((size_t)n0 + guards->n_spheres, none);  // spheres outside the tree keep a harmless record
    for (uint32_t i = 0; i < n0; i++) {
      uint32_t kind = ops[i].code & 0xFFu;
      if (kind != OP_BOX_SPH && kind != OP_SPHERE) continue;
      const uint32_t after = entry(ops[i].skip);
      for (int k = 0; k < 2; k++) {
        uint32_t payload = k == 0 ? ops[i].a : ops[i].b;
        if (payload == NONE) continue;
        const rl_sphere &sp = guards->spheres[payload & SPH_INDEX];
        DevOp G{};
        double r = std::fabs(sp.radius), lo[3], hi[3];
        swept_bounds(sp, lo, hi);
        for (int ax = 0; ax < 3; ax++) {
          // this box only ever rejects: keep it outside the sphere by more than Sphere::hit's rounding can bridge (rl_fast_bvh.cpp guard_pad)
          double pad = std::fmax(1e-9 * (std::fabs(lo[ax]) + std::fabs(hi[ax]) + r), frame ? guard_pad(*frame, r) : 0.0);  // r = 0: inf -> NaN box
          G.box[2 * ax] = lo[ax] - pad, G.box[2 * ax + 1] = hi[ax] + pad;
        }
        for (int ax = 0; ax < 6; ax++)
          if (!(std::fabs(G.box[ax]) <= 1e30)) {  // NaN / inf / huge: never certain, i.e. always test the sphere
            for (double &b : G.box) b = qnan;
            break;
          }
        const uint32_t self = guard_of(payload);
        G.code = (ST_LEAF << 29) | self;  // box "hit" (or not certain): test the sphere
        const bool more = k == 0 && ops[i].b != NONE;
        G.skip = more ? ((ST_TRAV << 29) | guard_of(ops[i].b)) : after;  // then the leaf's other sphere, then on
        G.a = payload, G.b = NONE;
        out[self] = G;
      }
    }
  }
  return ops.empty() ? (uint32_t)(ST_SHADE << 29) : entry(0);
}

// One DevMaterial per sphere for the wave kernel's SHADE: the sphere's material with (a) a Solid texture's colour copied
// into albedo (flag MAT_TEX_SOLID) and (b) for a Dielectric albedo = {1/ior, r0(ri = 1/ior), r0(ri = ior)} with
// r0 = ((1 - ri) / (1 + ri))^2 — the very expressions material.rs:140-166 evaluates per scatter (IEEE, no contraction).
// (c) A Checker whose two children are Solid is as constant per scene as a Solid: its even colour goes into albedo (flag
// MAT_TEX_CHECKER) and its odd colour and inv_scale into the sphere's record of `checker`, all copied as they are, so that SHADE
// fetches them by sphere index beside the material instead of walking texture -> child -> colour.  Any other texture tree (a nested
// checker, say) keeps the generic walk.  `checker` has a record for every sphere, zeros where the flag is not set: SHADE loads it
// before it knows the flag.
static void flatten_sphere_materials(const RtiowProgram &rt, std::vector<DevMaterial> &out, std::vector<DevChecker> &checker) {
  out.resize(rt.spheres.size());
  checker.assign(rt.spheres.size(), DevChecker{{0.0, 0.0, 0.0}, 0.0});
  for (size_t i = 0; i < rt.spheres.size(); i++) {
    DevMaterial m = rt.materials[rt.sphere_material[i]];
    const bool textured = m.kind == RL_MAT_LAMBERTIAN || m.kind == RL_MAT_DIFFUSE_LIGHT;
    if (textured && rt.textures[m.texture].kind == RL_TEX_SOLID) {
      const DevTexture &t = rt.textures[m.texture];
      m.albedo[0] = t.color[0], m.albedo[1] = t.color[1], m.albedo[2] = t.color[2];
      m.kind |= MAT_TEX_SOLID;
    } else if (textured && rt.textures[m.texture].kind == RL_TEX_CHECKER && rt.textures[rt.textures[m.texture].even].kind == RL_TEX_SOLID &&
               rt.textures[rt.textures[m.texture].odd].kind == RL_TEX_SOLID) {
      const DevTexture &t = rt.textures[m.texture], &ev = rt.textures[t.even], &od = rt.textures[t.odd];
      m.albedo[0] = ev.color[0], m.albedo[1] = ev.color[1], m.albedo[2] = ev.color[2];
      checker[i] = DevChecker{{od.color[0], od.color[1], od.color[2]}, t.inv_scale};
      m.kind |= MAT_TEX_CHECKER;
    } else if (m.kind == RL_MAT_DIELECTRIC) {
      auto r0 = [](double ri) {
        double q = (1.0 - ri) / (1.0 + ri);
        return q * q;
      };
      double inv = 1.0 / m.ior;
      m.albedo[0] = inv, m.albedo[1] = r0(inv), m.albedo[2] = r0(m.ior);
    }
    out[i] = m;
  }
}

static int build_host_rtiow_may_throw(const rl_rtiow_scene_desc *desc, std::shared_ptr<const HostRtiow> &out, std::string &err) {
  auto H = std::make_shared<HostRtiow>();
  if (compile_rtiow(*desc, H->rt, err) != RL_OK) return RL_E_INVALID;
  const RtiowProgram &rt = H->rt;
  if (!(rt.has_planars || rt.has_instances || rt.has_images || rt.has_noise || rt.has_media) && rt.ops.size() < (1u << 29)) {
    H->entry0 = link_ops(rt.ops, H->lops);
    flatten_sphere_materials(rt, H->sphere_flat, H->sphere_checker);
    // compact guarded form (32-byte ops: binary32 box + the two successor words) for the 4-waves-per-SIMD layout
    std::vector<DevOp> gops;
    bool gok = false;
    GuardFrame frame = guard_frame(*desc);
    uint32_t gentry = link_ops(rt.ops, gops, desc, &gok, &frame);
    if (gok && gops.size() < (1u << 24)) {
      H->cops.resize(gops.size());
      for (size_t i = 0; i < gops.size(); i++) {
        for (int k = 0; k < 6; k++) H->cops[i].box[k] = (float)gops[i].box[k];
        H->cops[i].w_hit = gops[i].code, H->cops[i].w_miss = gops[i].skip;
      }
      // [one bit per sphere: Center::Moving][one bit per sphere: Metal / Dielectric material (the fast kernel's ST_SHADE2)]
      const size_t bw = (rt.spheres.size() + 31) / 32 + 1;
      H->movbits.assign(2 * bw, 0u);
      for (size_t i = 0; i < rt.spheres.size(); i++) {
        if (desc->spheres[i].moving) H->movbits[i >> 5] |= 1u << (i & 31);
        uint32_t kind = rt.materials[rt.sphere_material[i]].kind;
        if (kind == RL_MAT_METAL || kind == RL_MAT_DIELECTRIC) H->movbits[bw + (i >> 5)] |= 1u << (i & 31);
      }
      H->centry0 = gentry;
      std::memcpy(H->guard_center, frame.center, sizeof frame.center);
      H->guard_reach = frame.reach;
    }
    // the fast traversal structure of the timed (counter-free) kernel: ordered binary tree, reject-only boxes (rl_fast_bvh.cpp)
    if (!H->cops.empty() && !build_fast_bvh(*desc, rt, frame, H->fast_nodes, H->fast_root)) H->fast_nodes.clear(), H->fast_root = FAST_NONE;
    if (H->fast_root != FAST_NONE) {  // the spheres' own (padded) leaf boxes, by sphere index: what the cooperative kernel scans
      const uint32_t n_inner = (uint32_t)H->fast_nodes.size(), ns = (uint32_t)rt.spheres.size();
      H->fast_nodes_ch.reserve(n_inner);
      for (const FastNode &nd : H->fast_nodes) H->fast_nodes_ch.push_back(fast_node_ch(nd));
      H->fast_leaf_boxes.assign((size_t)ns * 8, 0.0f);
      for (uint32_t s = 0; s < ns; s++)  // a sphere the tree does not hold (n == 1: no node at all) is always a candidate
        for (int k = 0; k < 3; k++) H->fast_leaf_boxes[(size_t)s * 8 + 2 * k] = -3.0e38f, H->fast_leaf_boxes[(size_t)s * 8 + 2 * k + 1] = 3.0e38f;
      for (const FastNode &nd : H->fast_nodes)
        for (int k = 0; k < 2; k++) {
          const uint32_t e = k == 0 ? (nd.child & 0xFFFFu) : (nd.child >> 16);
          if (e >= n_inner && e - n_inner < ns) std::memcpy(&H->fast_leaf_boxes[(size_t)(e - n_inner) * 8], nd.box[k], 6 * sizeof(float));
        }
      H->fast_motion_finite = fast_leaf_balls(*desc, frame, H->fast_leaf_balls, H->fast_leaf_motion);
    }
    // ray queries walk the four-wide world-space tree on every kind of scene (rl_ray_query.h rtiow_hit_rays_fast_kernel)
    if (rt.ops.size() < (1u << 31) && !build_fast_general(*desc, rt, H->qfg)) H->qfg = FastGeneral{};
  } else if (rt.ops.size() < (1u << 31)) {
    // general scenes (planars, instances, image / noise textures): world-space tree over the primitive occurrences
    if (!build_fast_general(*desc, rt, H->fg)) H->fg = FastGeneral{};
  }
  out = H;
  return RL_OK;
}

// ------------------------------------------------------------------ RTC
// Reject-only acceleration for the triangle Groups of the RTC path.  The reference's Group (group.rs) intersects every child
// for every ray; for each ROP_TRIS range of >= 8 triangles a binary tree over the triangles IN INDEX ORDER is built here (node =
// index range, box = padded union of the triangles' bounding boxes, stored as floats; leaves = single triangles; nodes in
// depth-first order so that a left-to-right walk meets the triangles in the reference's order) and the op's `skip` field gets
// root + 1.  The kernel skips a triangle only when its box is CERTAINLY missed (guard_reject32), so every intersection the
// reference would keep is still found, in the same order.
static void build_rtc_guards(RtcProgram &rc, std::vector<RtcGuard> &guards) {
  struct Builder {
    const std::vector<DevTri> &tris;
    std::vector<RtcGuard> &out;
    void box_of(uint32_t l, uint32_t r, float *b) const {
      double mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
      for (uint32_t i = l; i < r; i++) {
        const DevTri &t = tris[i];
        for (int ax = 0; ax < 3; ax++) {
          const double v[3] = {t.p1[ax], t.p1[ax] + t.e1[ax], t.p1[ax] + t.e2[ax]};
          for (double x : v) mn[ax] = std::fmin(mn[ax], x), mx[ax] = std::fmax(mx[ax], x);
        }
      }
      bool bad = false;
      for (int ax = 0; ax < 3; ax++) {
        double pad = 1e-6 * (std::fabs(mn[ax]) + std::fabs(mx[ax]) + (mx[ax] - mn[ax])) + 1e-30;  // the box only ever rejects: keep it outside the triangles
        b[2 * ax] = (float)(mn[ax] - pad), b[2 * ax + 1] = (float)(mx[ax] + pad);
        bad |= !(std::fabs(mn[ax]) <= 1e30 && std::fabs(mx[ax]) <= 1e30);
      }
      if (bad)
        for (int k = 0; k < 6; k++) b[k] = NAN;  // never certainly missed
    }
    void build(uint32_t l, uint32_t r) {
      const uint32_t idx = (uint32_t)out.size();
      out.push_back(RtcGuard{});
      RtcGuard nd{};
      box_of(l, r, nd.box);
      if (r - l == 1) nd.tri = l, nd.skip = idx + 1;
      else {
        const uint32_t m = l + (r - l) / 2;
        build(l, m);
        build(m, r);
        nd.tri = NONE, nd.skip = (uint32_t)out.size();
      }
      out[idx] = nd;
    }
  };
  Builder b{rc.tris, guards};
  for (DevOp &op : rc.ops)
    if (op.code == ROP_TRIS && op.b >= 8) {
      op.skip = (uint32_t)guards.size() + 1u;
      b.build(op.a, op.a + op.b);
    }
}

static int build_host_rtc_may_throw(const rl_rtc_scene_desc &desc, std::shared_ptr<const HostRtc> &out, std::string &err) {
  auto H = std::make_shared<HostRtc>();
  if (compile_rtc(desc, H->rc, err) != RL_OK) return RL_E_INVALID;
  if (H->rc.lights.size() > 0xFFFFu) {
    err = "too many lights";
    return RL_E_UNSUPPORTED;
  }
  // rtc_full_kernel walks the reflection / refraction tree with a fixed stack of pending rays (RTC_MAX_PENDING): a material that is
  // both reflective and transparent keeps up to max_reflection_depth + 1 of them alive (world.rs:128-159 recurses without a cap)
  if (H->rc.needs_full && H->rc.max_reflection_depth + 1u > RTC_MAX_PENDING) {
    err = "max_reflection_depth above " + std::to_string(RTC_MAX_PENDING - 1) + " is not supported by the device kernel";
    return RL_E_UNSUPPORTED;
  }
  build_rtc_guards(H->rc, H->guards);  // both kernels walk them (the full kernel with the unbounded line test)
  out = H;
  return RL_OK;
}

// The entry points are called from behind a C ABI: nothing may be thrown through them.  Every container above is a std::vector sized by
// the caller's description, so running out of memory is an outcome like any other refusal.
template <class Build>
static int no_throw(Build build, std::string &err) {
  try {
    return build();
  } catch (const std::bad_alloc &) {
    err = "out of memory while compiling the scene";
    return RL_E_NOMEM;
  } catch (const std::exception &e) {
    err = std::string("scene compiler: ") + e.what();
    return RL_E_INVALID;
  } catch (...) {
    err = "scene compiler: unknown exception";
    return RL_E_INVALID;
  }
}

int build_host_rtiow(const rl_rtiow_scene_desc *desc, std::shared_ptr<const HostRtiow> &out, std::string &err) {
  return no_throw([&] { return build_host_rtiow_may_throw(desc, out, err); }, err);
}

int build_host_rtc(const rl_rtc_scene_desc &desc, std::shared_ptr<const HostRtc> &out, std::string &err) {
  return no_throw([&] { return build_host_rtc_may_throw(desc, out, err); }, err);
}

// ------------------------------------------------------------------ the structure report
namespace {
struct Frame {  // one entry of a tree with the box its parent holds for it
  uint32_t e;
  float box[6];
  bool has_box;
  unsigned depth;
};
bool inside(const float *outer, const double *lo, const double *hi) {
  for (int ax = 0; ax < 3; ax++)
    if (!((double)outer[2 * ax] <= lo[ax] && hi[ax] <= (double)outer[2 * ax + 1])) return false;
  return true;
}

// out16[1 .. 8], [14], [15]: the four-wide world-space tree, every stage of it
void report_general_tree(const rl_rtiow_scene_desc *desc, const FastGeneral &fg, unsigned long long *out16) {
  out16[1] = fg.items.size(), out16[2] = fg.nodes.size(), out16[3] = fg.qnodes.size();
  std::vector<uint32_t> seen(fg.items.size(), 0u);
  std::vector<Frame> st;
  for (uint32_t sr : fg.stage_roots)  // every stage: plane leaves, segment trees, media (their entries carry FASTG_MEDIUM and are no items)
    if (sr != NONE) st.push_back(Frame{sr, {0, 0, 0, 0, 0, 0}, false, 1u});
  while (!st.empty()) {
    Frame f = st.back();
    st.pop_back();
    out16[8] = std::max<unsigned long long>(out16[8], f.depth);
    if ((f.e & FASTG_LEAF) && (f.e & FASTG_MEDIUM)) continue;
    if (f.e & FASTG_LEAF) {
      const uint32_t item = f.e & ~FASTG_LEAF;
      out16[4]++;
      if (item >= seen.size()) {
        out16[7]++;
        continue;
      }
      seen[item]++;
      const FastItem &it = fg.items[item];
      if (f.has_box && it.chain == NONE) {  // world-space item: its geometry must lie inside the leaf's box
        double lo[3], hi[3];
        if (it.kind == 0) {
          swept_bounds(desc->spheres[it.payload & SPH_INDEX], lo, hi);
        } else if (desc->planars[it.payload].kind == RL_PLANAR_PLANE) {
          out16[7]++;  // an unbounded Plane must not sit below a box
          continue;
        } else {
          const rl_planar &pl = desc->planars[it.payload];
          for (int ax = 0; ax < 3; ax++) {
            double v[4] = {pl.q[ax], pl.q[ax] + pl.u[ax], pl.q[ax] + pl.v[ax], pl.kind == RL_PLANAR_QUAD ? pl.q[ax] + pl.u[ax] + pl.v[ax] : pl.q[ax]};
            lo[ax] = std::fmin(std::fmin(v[0], v[1]), std::fmin(v[2], v[3])), hi[ax] = std::fmax(std::fmax(v[0], v[1]), std::fmax(v[2], v[3]));
          }
        }
        if (!inside(f.box, lo, hi)) out16[7]++;
      }
      continue;
    }
    if (f.e >= fg.qnodes.size()) {
      out16[7]++;
      continue;
    }
    const FastNodeQ &q = fg.qnodes[f.e];
    double ulo[3] = {INFINITY, INFINITY, INFINITY}, uhi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int k = 0; k < 4; k++) {
      if (q.child[k] == NONE) continue;
      Frame c{q.child[k], {q.lo[0][k], q.hi[0][k], q.lo[1][k], q.hi[1][k], q.lo[2][k], q.hi[2][k]}, true, f.depth + 1u};
      for (int ax = 0; ax < 3; ax++) ulo[ax] = std::fmin(ulo[ax], (double)c.box[2 * ax]), uhi[ax] = std::fmax(uhi[ax], (double)c.box[2 * ax + 1]);
      st.push_back(c);
    }
    if (f.has_box && !inside(f.box, ulo, uhi)) out16[7]++;  // a node's box (held by its parent) contains its children's boxes
  }
  for (uint32_t c : seen) out16[5] += c > 1u ? 1u : 0u, out16[6] += c == 0u ? 1u : 0u;
  // media: [14] = how many, [15] = one byte per medium (the first eight): FastMedium::shape, + 0x10 when the medium has a box node
  out16[14] = fg.media.size();
  for (size_t k = 0; k < fg.media.size() && k < 8; k++)
    out16[15] |= (unsigned long long)(fg.media[k].shape | (fg.media_stage[k] != NONE && !(fg.stage_roots[fg.media_stage[k]] & FASTG_LEAF) ? 0x10u : 0u)) << (8 * k);
}

// out16[9 .. 13]: the ordered binary tree over the spheres
void report_sphere_tree(const rl_rtiow_scene_desc *desc, const HostRtiow &H, unsigned long long *out16) {
  const std::vector<FastNode> &nodes = H.fast_nodes;
  const uint32_t n_inner = (uint32_t)nodes.size(), n_sph = desc->n_spheres;
  out16[9] = n_inner;
  std::vector<uint32_t> seen(n_sph, 0u);
  std::vector<Frame> st;
  st.push_back(Frame{H.fast_root, {0, 0, 0, 0, 0, 0}, false, 1u});
  while (!st.empty()) {
    Frame f = st.back();
    st.pop_back();
    out16[13] = std::max<unsigned long long>(out16[13], f.depth);
    if (f.e >= n_inner) {
      const uint32_t si = f.e - n_inner;
      out16[10]++;
      if (si >= n_sph) {
        out16[12]++;
        continue;
      }
      seen[si]++;
      if (f.has_box) {
        double lo[3], hi[3];
        swept_bounds(desc->spheres[si], lo, hi);
        if (!inside(f.box, lo, hi)) out16[12]++;
      }
      continue;
    }
    const FastNode &nd = nodes[f.e];
    for (int k = 0; k < 2; k++) {
      Frame c{k == 0 ? (nd.child & 0xFFFFu) : (nd.child >> 16), {nd.box[k][0], nd.box[k][1], nd.box[k][2], nd.box[k][3], nd.box[k][4], nd.box[k][5]}, true, f.depth + 1u};
      const double lo[3] = {c.box[0], c.box[2], c.box[4]}, hi[3] = {c.box[1], c.box[3], c.box[5]};
      if (f.has_box && !inside(f.box, lo, hi)) out16[12]++;
      st.push_back(c);
    }
  }
  for (uint32_t c : seen) out16[11] += c != 1u ? 1u : 0u;
}
}  // namespace

void host_structures_report(const rl_rtiow_scene_desc *desc, const HostRtiow &H, unsigned long long *out16) {
  for (int i = 0; i < 16; i++) out16[i] = 0;
  if (H.fast_root != FAST_NONE) out16[0] |= 1ull;
  if (H.fg.ok) out16[0] |= 2ull;
  if (H.fg.ok) report_general_tree(desc, H.fg, out16);
  if (H.fast_root != FAST_NONE) report_sphere_tree(desc, H, out16);
}

}  // namespace rl
