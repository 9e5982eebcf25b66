// Scene "compiler": validates the caller's object graph and lowers it to the threaded program of
// rl_program.h.  Host code only (no HIP calls).
//
// Both graphs are lowered in two passes, neither of which recurses (a caller's graph may be a chain as deep as MAX_NEST, and sharing is
// legal, so the expansion may be exponentially larger than the description):
//   survey: one visit per node of the description (white / open / done colouring on an explicit stack) that checks every reference,
//           finds cycles and gathers per node what the refusals and the lowering need: the number of ops its expansion emits (64-bit,
//           saturating), the depth of the graph below it and the nesting depths of the constructs the kernels keep fixed stacks for;
//   lower:  the depth-first expansion itself, on an explicit stack, begun only when the survey has shown that it fits the op limit.
//           A list or group steps from one child whose expansion holds an op to the next such child (a link per place of the item
//           array, made once by the survey), so children that expand to nothing (lists of empty lists) cost nothing however often
//           their parent is expanded, and a list or group with ONE such child is replaced by what it stands for (a chain of them by its
//           end).  Every frame `lower` pushes then belongs to a node that emits an op of its own or has two children that do: the
//           work is bounded by the description's size plus the ops emitted.
#include "rl_program.h"

#include <cmath>
#include <cstring>

namespace rl {

namespace {

const uint32_t MAX_NEST = RL_SCENE_MAX_NEST;  // deepest reference below the root (root = 0) of a graph that compiles
const uint64_t MAX_OPS = RL_SCENE_MAX_OPS;    // a program (its END op included) must be shorter than this
const uint64_t OPS_SAT = 1ull << 62;          // where the survey's op counts saturate

enum : uint8_t { WHITE = 0, OPEN = 1, DONE = 2 };

inline uint64_t sat_add(uint64_t a, uint64_t b) { return a + b > OPS_SAT ? OPS_SAT : a + b; }  // a, b <= OPS_SAT

struct RtiowCompiler {
  const rl_rtiow_scene_desc &d;
  RtiowProgram &p;
  std::string &err;

  struct Facts {      // of one node's expansion
    uint64_t ops;     // ops it emits
    uint32_t height;  // deepest reference below it
    uint8_t state;
    uint8_t inst;     // Translate / Transform nesting inside it
    uint8_t medium;   // holds a ConstantMedium
  };
  std::vector<Facts> f_translate, f_transform, f_bvh, f_list, f_medium;
  std::vector<uint32_t> push_stack;
  std::vector<uint32_t> next_live;  // [n_list_items + 1]: the first place at or after j whose item's expansion holds an op (survey)
  std::vector<rl_href> list_is;     // [n_lists]: what a list with ONE child that emits ops stands for (kind RL_H_NONE: itself)

  RtiowCompiler(const rl_rtiow_scene_desc &d_, RtiowProgram &p_, std::string &err_)
      : d(d_), p(p_), err(err_), f_translate(d_.n_translates, Facts{}), f_transform(d_.n_transforms, Facts{}), f_bvh(d_.n_bvh_nodes, Facts{}),
        f_list(d_.n_lists, Facts{}), f_medium(d_.n_media, Facts{}), list_is(d_.n_lists, rl_href{RL_H_NONE, 0}) {}

  bool fail(const std::string &m) {
    err = m;
    return false;
  }
  bool check(rl_href h) {
    switch (h.kind) {
      case RL_H_SPHERE: return h.index < d.n_spheres || fail("sphere index out of range");
      case RL_H_PLANAR: return h.index < d.n_planars || fail("planar index out of range");
      case RL_H_TRANSLATE: return h.index < d.n_translates || fail("translate index out of range");
      case RL_H_TRANSFORM: return h.index < d.n_transforms || fail("transform index out of range");
      case RL_H_BVH: return h.index < d.n_bvh_nodes || fail("bvh node index out of range");
      case RL_H_LIST: return h.index < d.n_lists || fail("list index out of range");
      case RL_H_MEDIUM: return h.index < d.n_media || fail("medium index out of range");
      default: return fail("unknown hittable kind");
    }
  }
  uint32_t sphere_payload(uint32_t idx) { return idx | (d.spheres[idx].moving ? SPH_MOVING : 0u) | (p.sphere_uv[idx] ? SPH_UV : 0u); }

  // ---- the graph as both passes see it (references already checked)
  Facts *facts(rl_href h) {  // null: a primitive
    switch (h.kind) {
      case RL_H_TRANSLATE: return &f_translate[h.index];
      case RL_H_TRANSFORM: return &f_transform[h.index];
      case RL_H_BVH: return &f_bvh[h.index];
      case RL_H_LIST: return &f_list[h.index];
      case RL_H_MEDIUM: return &f_medium[h.index];
      default: return nullptr;
    }
  }
  Facts facts_or_leaf(rl_href h) {
    Facts *f = facts(h);
    return f ? *f : Facts{1, 0, DONE, 0, 0};
  }
  // a BVH node whose children are all spheres (1) or all planars (2) is one leaf op holding them; anything else (0) a box op over its children
  static int bvh_leaf(const rl_bvh_node &n) {
    bool all_sph = true, all_pl = true;
    for (uint32_t i = 0; i < n.n_children; i++) {
      all_sph &= n.child[i].kind == RL_H_SPHERE;
      all_pl &= n.child[i].kind == RL_H_PLANAR;
    }
    return all_sph ? 1 : (all_pl ? 2 : 0);
  }
  uint32_t n_children(rl_href h) const {
    switch (h.kind) {
      case RL_H_LIST: return d.lists[h.index].count;
      case RL_H_BVH: return bvh_leaf(d.bvh_nodes[h.index]) ? 0u : d.bvh_nodes[h.index].n_children;
      case RL_H_MEDIUM:
      case RL_H_TRANSLATE:
      case RL_H_TRANSFORM: return 1;
      default: return 0;
    }
  }
  rl_href child(rl_href h, uint32_t i) const {
    switch (h.kind) {
      case RL_H_LIST: return d.list_items[d.lists[h.index].first + i];
      case RL_H_BVH: return d.bvh_nodes[h.index].child[i];
      case RL_H_MEDIUM: return d.media[h.index].boundary;
      case RL_H_TRANSLATE: return d.translates[h.index].child;
      default: return d.transforms[h.index].child;
    }
  }

  struct Frame {
    rl_href h;
    uint32_t next;  // child to visit next
    uint32_t pc;    // lower: the op this node opened with
  };

  // ---- survey
  bool survey_open(rl_href h, std::vector<Frame> &st) {  // st.size() = depth of h below the root
    if (!check(h)) return false;
    Facts *f = facts(h);
    if (!f || f->state == DONE) return true;
    if (f->state == OPEN) {
      switch (h.kind) {
        case RL_H_LIST: return fail("cycle through a list");
        case RL_H_BVH: return fail("cycle through a bvh node");
        case RL_H_MEDIUM: return fail("a ConstantMedium boundary must not contain another medium");
        default: return fail("cycle through an instance");
      }
    }
    if (st.size() > MAX_NEST) return fail("scene graph too deep");
    if (h.kind == RL_H_LIST) {
      const rl_list &l = d.lists[h.index];
      if ((uint64_t)l.first + l.count > d.n_list_items) return fail("list range out of bounds");
    } else if (h.kind == RL_H_BVH) {
      const rl_bvh_node &n = d.bvh_nodes[h.index];
      if (n.n_children < 1 || n.n_children > 2) return fail("bvh node must have 1 or 2 children");
      for (uint32_t i = 0; i < n.n_children; i++)
        if (!check(n.child[i])) return false;
      if (bvh_leaf(n)) {
        *f = Facts{1, 0, DONE, 0, 0};
        return true;
      }
    } else if (h.kind == RL_H_MEDIUM) {
      if (d.media[h.index].material >= d.n_materials) return fail("medium material out of range");
    }
    f->state = OPEN;
    st.push_back(Frame{h, 0, 0});
    return true;
  }
  bool survey_close(rl_href h, size_t depth) {
    Facts &f = *facts(h);
    const uint32_t n = n_children(h);
    Facts sum{0, 0, DONE, 0, 0};
    uint32_t live = 0;  // children whose expansion holds an op, and the last of them
    rl_href last{RL_H_NONE, 0};
    for (uint32_t i = 0; i < n; i++) {
      Facts c = facts_or_leaf(child(h, i));
      sum.ops = sat_add(sum.ops, c.ops);
      if (c.height + 1u > sum.height) sum.height = c.height + 1u;
      if (c.inst > sum.inst) sum.inst = c.inst;
      sum.medium |= c.medium;
      if (c.ops) live++, last = child(h, i);
    }
    switch (h.kind) {
      case RL_H_LIST:  // a list with one such child expands to what that child expands to: `lower` goes there directly
        if (live == 1) list_is[h.index] = last.kind == RL_H_LIST && list_is[last.index].kind != RL_H_NONE ? list_is[last.index] : last;
        break;
      case RL_H_BVH: sum.ops = sat_add(sum.ops, 1); break;
      case RL_H_MEDIUM:  // constant_medium.rs: the boundary is evaluated by itself (twice per ray), not folded into the world
        if (sum.medium) return fail("a ConstantMedium boundary must not contain another medium");
        sum.ops = sat_add(sum.ops, 2), sum.medium = 1;
        break;
      default:
        sum.ops = sat_add(sum.ops, 2), sum.inst++;
        if (sum.inst > 8) return fail("instances nested deeper than 8");
    }
    if (depth + sum.height > MAX_NEST) return fail("scene graph too deep");
    f = sum;
    return true;
  }
  bool survey(rl_href root) {
    std::vector<Frame> st;
    if (!survey_open(root, st)) return false;
    while (!st.empty()) {
      const Frame fr = st.back();
      if (fr.next < n_children(fr.h)) {
        st.back().next++;
        if (!survey_open(child(fr.h, fr.next), st)) return false;
        continue;
      }
      st.pop_back();
      if (!survey_close(fr.h, st.size())) return false;
    }
    if (facts_or_leaf(root).ops + 1 >= MAX_OPS) return fail("program too large");
    // whether an item's expansion holds an op is a fact of its place in list_items: one backwards pass links every place to the next
    // such place, so that a list expanded many times never walks its empty children again
    next_live.assign((size_t)d.n_list_items + 1, d.n_list_items);
    for (uint32_t j = d.n_list_items; j-- > 0;) next_live[j] = item_ops(d.list_items[j]) ? j : next_live[j + 1];
    return true;
  }
  uint64_t item_ops(rl_href h) const {  // of any list item, reached by the survey or not (then 0: `lower` never meets it)
    switch (h.kind) {
      case RL_H_SPHERE: return h.index < d.n_spheres;
      case RL_H_PLANAR: return h.index < d.n_planars;
      case RL_H_TRANSLATE: return h.index < d.n_translates && f_translate[h.index].state == DONE ? f_translate[h.index].ops : 0;
      case RL_H_TRANSFORM: return h.index < d.n_transforms && f_transform[h.index].state == DONE ? f_transform[h.index].ops : 0;
      case RL_H_BVH: return h.index < d.n_bvh_nodes && f_bvh[h.index].state == DONE ? f_bvh[h.index].ops : 0;
      case RL_H_LIST: return h.index < d.n_lists && f_list[h.index].state == DONE ? f_list[h.index].ops : 0;
      case RL_H_MEDIUM: return h.index < d.n_media && f_medium[h.index].state == DONE ? f_medium[h.index].ops : 0;
      default: return 0;
    }
  }
  // the first child at or after `next` whose expansion holds an op (n_children(h): none)
  uint32_t live_child(rl_href h, uint32_t next) const {
    if (h.kind != RL_H_LIST) return next;
    const rl_list &l = d.lists[h.index];
    const uint64_t j = next_live[(size_t)l.first + next];
    return j - l.first < l.count ? (uint32_t)(j - l.first) : l.count;
  }

  // ---- lower (of a surveyed graph: nothing can fail any more)
  void lower_open(rl_href h, std::vector<Frame> &st) {
    switch (h.kind) {
      case RL_H_SPHERE: {
        DevOp op{};
        op.code = OP_SPHERE, op.a = sphere_payload(h.index), op.b = NONE;
        op.skip = (uint32_t)p.ops.size() + 1;
        p.ops.push_back(op);
        return;
      }
      case RL_H_PLANAR: {
        DevOp op{};
        op.code = OP_PLANAR, op.a = h.index, op.b = NONE;
        op.skip = (uint32_t)p.ops.size() + 1;
        p.ops.push_back(op);
        p.has_planars = true;
        return;
      }
      case RL_H_LIST:
        if (!f_list[h.index].ops) return;
        if (list_is[h.index].kind != RL_H_NONE) return lower_open(list_is[h.index], st);  // never a list that forwards again
        st.push_back(Frame{h, 0, 0});  // two children or more that emit ops: the frame is paid for by them
        return;
      case RL_H_BVH: {
        const rl_bvh_node &n = d.bvh_nodes[h.index];
        uint32_t idx = (uint32_t)p.ops.size();
        DevOp op{};
        std::memcpy(op.box, n.bbox, sizeof op.box);
        uint32_t finite = BOX_FINITE;  // every bound finite and small enough for the filtered (reciprocal) AABB test
        for (int k = 0; k < 6; k++)
          if (!(std::fabs(n.bbox[k]) <= 1e100)) finite = 0;
        const int leaf = bvh_leaf(n);
        if (leaf == 1) {
          op.code = OP_BOX_SPH | finite;
          op.a = sphere_payload(n.child[0].index);
          op.b = n.n_children == 2 ? sphere_payload(n.child[1].index) : NONE;
          op.skip = idx + 1;
          p.ops.push_back(op);
          return;
        }
        if (leaf == 2) {
          op.code = OP_BOX_PLANAR | finite;
          op.a = n.child[0].index;
          op.b = n.n_children == 2 ? n.child[1].index : NONE;
          op.skip = idx + 1;
          p.ops.push_back(op);
          p.has_planars = true;
          return;
        }
        op.code = OP_BOX | finite, op.a = op.b = NONE;
        p.ops.push_back(op);
        st.push_back(Frame{h, 0, idx});
        return;
      }
      case RL_H_MEDIUM: {
        uint32_t begin = (uint32_t)p.ops.size();
        DevOp op{};
        op.code = OP_MEDIUM_BEGIN, op.a = h.index, op.b = NONE;
        p.ops.push_back(op);
        st.push_back(Frame{h, 0, begin});
        return;
      }
      default: {  // RL_H_TRANSLATE, RL_H_TRANSFORM
        bool tr = h.kind == RL_H_TRANSLATE;
        uint32_t push_pc = (uint32_t)p.ops.size();
        DevOp op{};
        op.code = tr ? OP_PUSH_TRANSLATE : OP_PUSH_TRANSFORM;
        op.a = h.index;
        op.b = push_stack.empty() ? NONE : push_stack.back();  // parent PUSH: the chain back to the world ray
        op.skip = push_pc + 1;
        p.ops.push_back(op);
        p.has_instances = true;
        push_stack.push_back(push_pc);
        if (push_stack.size() > p.max_instance_depth) p.max_instance_depth = (uint32_t)push_stack.size();
        st.push_back(Frame{h, 0, push_pc});
        return;
      }
    }
  }
  void lower_close(const Frame &fr) {
    switch (fr.h.kind) {
      case RL_H_LIST: return;
      case RL_H_BVH: p.ops[fr.pc].skip = (uint32_t)p.ops.size(); return;
      case RL_H_MEDIUM: {
        DevOp e{};
        e.code = OP_MEDIUM_END, e.a = fr.h.index, e.b = fr.pc;
        e.skip = (uint32_t)p.ops.size() + 1;
        p.ops.push_back(e);
        p.ops[fr.pc].skip = (uint32_t)p.ops.size();
        p.has_media = true;
        return;
      }
      default: {
        push_stack.pop_back();
        DevOp po{};
        po.code = fr.h.kind == RL_H_TRANSLATE ? OP_POP_TRANSLATE : OP_POP_TRANSFORM;
        po.a = fr.h.index, po.b = fr.pc;  // matching PUSH
        po.skip = (uint32_t)p.ops.size() + 1;
        p.ops.push_back(po);
        return;
      }
    }
  }
  void lower(rl_href root) {
    p.ops.reserve((size_t)facts_or_leaf(root).ops + 1);  // known exactly: a graph the memory cannot hold fails here, before any work
    std::vector<Frame> st;
    lower_open(root, st);
    while (!st.empty()) {
      const Frame fr = st.back();
      const uint32_t next = live_child(fr.h, fr.next);
      if (next < n_children(fr.h)) {
        st.back().next = next + 1;
        lower_open(child(fr.h, next), st);
        continue;
      }
      st.pop_back();
      lower_close(fr);
    }
  }
};

// Checker nesting must be acyclic and at most 32 deep (the device follows it with a bounded loop).  One visit per texture; the walk
// holds the checkers of one path and gives up as soon as there are 33 of them, so neither a long chain nor a cycle costs more than that.
bool checker_nesting_ok(const rl_rtiow_scene_desc &d) {
  const int MAX_TEX_NEST = 32;
  std::vector<int> nest(d.n_textures, -1);  // -1 unknown, -2 on the path, >= 0 nesting depth
  struct Frame {
    uint32_t t;
    int next, deepest;  // child to visit next (0 even, 1 odd); the children's deepest nesting so far
  };
  std::vector<Frame> st;
  for (uint32_t i = 0; i < d.n_textures; i++) {
    if (nest[i] >= 0) continue;
    if (d.textures[i].kind != RL_TEX_CHECKER) {
      nest[i] = 0;
      continue;
    }
    nest[i] = -2;
    st.assign(1, Frame{i, 0, 0});
    while (!st.empty()) {
      Frame &fr = st.back();
      if (fr.next < 2) {
        const uint32_t c = fr.next++ == 0 ? d.textures[fr.t].even : d.textures[fr.t].odd;
        if (nest[c] == -2) return false;  // cycle
        if (nest[c] < 0 && d.textures[c].kind != RL_TEX_CHECKER) nest[c] = 0;
        if (nest[c] >= 0) {
          if (nest[c] > fr.deepest) fr.deepest = nest[c];
          continue;
        }
        if ((int)st.size() >= MAX_TEX_NEST) return false;  // a 33rd checker on one path
        nest[c] = -2;
        st.push_back(Frame{c, 0, 0});
        continue;
      }
      const int r = 1 + fr.deepest;
      if (r > MAX_TEX_NEST) return false;
      nest[fr.t] = r;
      st.pop_back();
      if (!st.empty() && r > st.back().deepest) st.back().deepest = r;
    }
  }
  return true;
}

}  // namespace

int compile_rtiow(const rl_rtiow_scene_desc &d, RtiowProgram &p, std::string &err) {
  auto need = [&](const void *ptr, uint32_t n, const char *what) {
    if (n && !ptr) {
      err = std::string("null array: ") + what;
      return false;
    }
    return true;
  };
  if (!need(d.spheres, d.n_spheres, "spheres") || !need(d.planars, d.n_planars, "planars") || !need(d.translates, d.n_translates, "translates") ||
      !need(d.transforms, d.n_transforms, "transforms") || !need(d.bvh_nodes, d.n_bvh_nodes, "bvh_nodes") || !need(d.lists, d.n_lists, "lists") ||
      !need(d.list_items, d.n_list_items, "list_items") || !need(d.materials, d.n_materials, "materials") ||
      !need(d.textures, d.n_textures, "textures") || !need(d.images, d.n_images, "images") || !need(d.perlins, d.n_perlins, "perlins") ||
      !need(d.media, d.n_media, "media"))
    return RL_E_INVALID;
  for (uint32_t i = 0; i < d.n_media; i++) p.media.push_back(d.media[i]);
  if (d.n_spheres > SPH_INDEX) {
    err = "too many spheres";
    return RL_E_INVALID;
  }
  for (uint32_t i = 0; i < d.n_perlins; i++) {  // perlin.rs:17-36: three permutations of 0..255
    const rl_perlin &pn = d.perlins[i];
    for (const uint32_t *perm : {pn.perm_x, pn.perm_y, pn.perm_z})
      for (int k = 0; k < 256; k++)
        if (perm[k] > 255u) {
          err = "perlin permutation entry out of range";
          return RL_E_INVALID;
        }
    p.perlins.push_back(pn);
  }

  // textures / images / materials
  for (uint32_t i = 0; i < d.n_images; i++) {
    const rl_image &im = d.images[i];
    if (!im.rgb || im.width == 0 || im.height == 0) {
      err = "Image has no data";  // texture.rs:64-67 assert
      return RL_E_INVALID;
    }
    DevImage di{im.width, im.height, (uint64_t)p.image_pool.size()};
    p.image_pool.insert(p.image_pool.end(), im.rgb, im.rgb + (size_t)im.width * im.height * 3);
    p.images.push_back(di);
    p.has_images = true;
  }
  for (uint32_t i = 0; i < d.n_textures; i++) {
    const rl_texture &t = d.textures[i];
    DevTexture dt{t.kind, t.even, t.odd, t.image, {t.color[0], t.color[1], t.color[2]}, t.inv_scale};
    if (t.kind == RL_TEX_CHECKER) {
      if (t.even >= d.n_textures || t.odd >= d.n_textures) {
        err = "checker texture child out of range";
        return RL_E_INVALID;
      }
    } else if (t.kind == RL_TEX_IMAGE) {
      if (t.image >= d.n_images) {
        err = "image index out of range";
        return RL_E_INVALID;
      }
    } else if (t.kind == RL_TEX_NOISE) {
      if (t.image >= d.n_perlins) {
        err = "perlin index out of range";
        return RL_E_INVALID;
      }
      p.has_noise = true;
    } else if (t.kind != RL_TEX_SOLID) {
      err = "unknown texture kind";
      return RL_E_INVALID;
    }
    p.textures.push_back(dt);
  }
  if (!checker_nesting_ok(d)) {
    err = "checker textures nest cyclically or deeper than 32";
    return RL_E_INVALID;
  }
  for (uint32_t i = 0; i < d.n_materials; i++) {
    const rl_material &m = d.materials[i];
    if (m.kind > RL_MAT_ISOTROPIC) {
      err = "unknown material kind";
      return RL_E_INVALID;
    }
    if ((m.kind == RL_MAT_LAMBERTIAN || m.kind == RL_MAT_DIFFUSE_LIGHT || m.kind == RL_MAT_ISOTROPIC) && m.texture >= d.n_textures) {
      err = "material texture out of range";
      return RL_E_INVALID;
    }
    p.materials.push_back(DevMaterial{m.kind, m.texture, {m.albedo[0], m.albedo[1], m.albedo[2]}, m.fuzz, m.ior});
  }
  // which materials sample an Image (their spheres must carry UVs)
  std::vector<uint8_t> mat_uv(d.n_materials, 0);
  for (uint32_t i = 0; i < d.n_materials; i++) {
    const rl_material &m = d.materials[i];
    if (m.kind != RL_MAT_LAMBERTIAN && m.kind != RL_MAT_DIFFUSE_LIGHT) continue;  // (an Isotropic's hit record carries uv (0, 0))
    std::vector<uint32_t> st{m.texture};
    std::vector<uint8_t> seen(d.n_textures, 0);
    while (!st.empty()) {
      uint32_t t = st.back();
      st.pop_back();
      if (seen[t]) continue;
      seen[t] = 1;
      if (d.textures[t].kind == RL_TEX_IMAGE) mat_uv[i] = 1;
      if (d.textures[t].kind == RL_TEX_CHECKER) st.push_back(d.textures[t].even), st.push_back(d.textures[t].odd);
    }
  }
  for (uint32_t i = 0; i < d.n_spheres; i++) {
    const rl_sphere &s = d.spheres[i];
    if (s.material >= d.n_materials) {
      err = "sphere material out of range";
      return RL_E_INVALID;
    }
    p.sphere_uv.push_back(mat_uv[s.material]);
    if (mat_uv[s.material]) p.has_sphere_uv = true;
    DevSphere ds{};
    for (int k = 0; k < 3; k++) {
      ds.c0[k] = s.center0[k];
      ds.dc[k] = s.moving ? s.center1[k] - s.center0[k] : 0.0;
    }
    ds.r2 = s.radius * s.radius;
    ds.inv_r = 1.0 / s.radius;
    p.spheres.push_back(ds);
    p.sphere_material.push_back(s.material);
  }
  for (uint32_t i = 0; i < d.n_planars; i++) {
    const rl_planar &s = d.planars[i];
    if (s.material >= d.n_materials) {
      err = "planar material out of range";
      return RL_E_INVALID;
    }
    if (s.kind > RL_PLANAR_TRIANGLE) {
      err = "unknown planar kind";
      return RL_E_INVALID;
    }
    DevPlanar dp{};
    std::memcpy(dp.q, s.q, 24), std::memcpy(dp.u, s.u, 24), std::memcpy(dp.v, s.v, 24), std::memcpy(dp.w, s.w, 24);
    std::memcpy(dp.normal, s.normal, 24);
    dp.d = s.d;
    dp.kind = s.kind, dp.material = s.material, dp.has_normals = s.has_normals, dp.has_uvs = s.has_uvs;
    std::memcpy(dp.normals, s.normals, sizeof dp.normals);
    std::memcpy(dp.uvs, s.uvs, sizeof dp.uvs);
    p.planars.push_back(dp);
  }
  p.translates.assign(d.translates, d.translates + d.n_translates);
  p.transforms.assign(d.transforms, d.transforms + d.n_transforms);

  RtiowCompiler c(d, p, err);
  if (!c.survey(d.root)) return RL_E_INVALID;
  c.lower(d.root);
  DevOp end{};
  end.code = OP_END, end.skip = (uint32_t)p.ops.size();
  end.a = end.b = NONE;
  p.ops.push_back(end);
  return RL_OK;
}

// ---------------------------------------------------------------- RTC
namespace {
struct RtcCompiler {
  const rl_rtc_scene_desc &d;
  RtcProgram &p;
  std::string &err;

  struct Facts {      // of one node's expansion
    uint64_t ops;     // ops it emits at most (adjacent triangles share one ROP_TRIS, counted here as one each)
    uint32_t height;  // deepest reference below it
    uint8_t state;
    uint8_t xform;    // Transformed nesting inside it
    uint8_t csg;      // CSG nesting inside it
  };
  std::vector<Facts> f_group, f_bounded, f_xform, f_csg;
  std::vector<uint32_t> enter_stack;
  std::vector<uint32_t> next_live;  // [n_group_items + 1]: the first place at or after j whose item's expansion holds an op (survey)
  std::vector<rl_oref> group_is;    // [n_groups]: what a group with ONE child that emits ops stands for (kind RL_O_NONE: itself)
  uint32_t csg_depth = 0;

  RtcCompiler(const rl_rtc_scene_desc &d_, RtcProgram &p_, std::string &err_)
      : d(d_), p(p_), err(err_), f_group(d_.n_groups, Facts{}), f_bounded(d_.n_boundeds, Facts{}), f_xform(d_.n_transformeds, Facts{}),
        f_csg(d_.n_csgs, Facts{}), group_is(d_.n_groups, rl_oref{RL_O_NONE, 0}) {}

  bool fail(const std::string &m) {
    err = m;
    return false;
  }
  bool check(rl_oref o) {
    switch (o.kind) {
      case RL_O_TRIANGLE: return o.index < d.n_triangles || fail("triangle index out of range");
      case RL_O_GROUP: return o.index < d.n_groups || fail("group index out of range");
      case RL_O_BOUNDED: return o.index < d.n_boundeds || fail("bounded index out of range");
      case RL_O_TRANSFORMED: return o.index < d.n_transformeds || fail("transformed index out of range");
      case RL_O_SPHERE:
      case RL_O_PLANE:
      case RL_O_CUBE:
      case RL_O_CYLINDER:
      case RL_O_CONE:
        if (o.index >= d.n_shapes) return fail("shape index out of range");
        return d.shapes[o.index].kind == o.kind || fail("shape kind does not match its reference");
      case RL_O_CSG: return o.index < d.n_csgs || fail("csg index out of range");
      default: return fail("unknown object kind");
    }
  }
  void emit_tri(uint32_t idx) {
    if (!p.ops.empty() && p.ops.back().code == ROP_TRIS && p.ops.back().a + p.ops.back().b == idx) {
      p.ops.back().b++;
      return;
    }
    DevOp op{};
    op.code = ROP_TRIS, op.a = idx, op.b = 1, op.skip = 0;
    p.ops.push_back(op);
  }

  Facts *facts(rl_oref o) {  // null: a triangle or a shape
    switch (o.kind) {
      case RL_O_GROUP: return &f_group[o.index];
      case RL_O_BOUNDED: return &f_bounded[o.index];
      case RL_O_TRANSFORMED: return &f_xform[o.index];
      case RL_O_CSG: return &f_csg[o.index];
      default: return nullptr;
    }
  }
  Facts facts_or_leaf(rl_oref o) {
    Facts *f = facts(o);
    return f ? *f : Facts{1, 0, DONE, 0, 0};
  }
  uint32_t n_children(rl_oref o) const {
    switch (o.kind) {
      case RL_O_GROUP: return d.groups[o.index].count;
      case RL_O_BOUNDED:
      case RL_O_TRANSFORMED: return 1;
      case RL_O_CSG: return 2;
      default: return 0;
    }
  }
  rl_oref child(rl_oref o, uint32_t i) const {
    switch (o.kind) {
      case RL_O_GROUP: return d.group_items[d.groups[o.index].first + i];
      case RL_O_BOUNDED: return d.boundeds[o.index].child;
      case RL_O_TRANSFORMED: return d.transformeds[o.index].child;
      default: return i == 0 ? d.csgs[o.index].left : d.csgs[o.index].right;
    }
  }

  struct Frame {
    rl_oref o;
    uint32_t next;  // child to visit next
    uint32_t pc;    // lower: the op this node opened with
  };

  // ---- survey
  bool survey_open(rl_oref o, std::vector<Frame> &st) {  // st.size() = depth of o below its world object
    if (!check(o)) return false;
    Facts *f = facts(o);
    if (!f || f->state == DONE) return true;
    if (f->state == OPEN) {
      switch (o.kind) {
        case RL_O_GROUP: return fail("cycle through a group");
        case RL_O_BOUNDED: return fail("cycle through a bounded");
        case RL_O_TRANSFORMED: return fail("cycle through a transformed");
        default: return fail("cycle through a csg");
      }
    }
    if (st.size() > MAX_NEST) return fail("scene graph too deep");
    if (o.kind == RL_O_GROUP) {
      const rl_rtc_group &g = d.groups[o.index];
      if ((uint64_t)g.first + g.count > d.n_group_items) return fail("group range out of bounds");
    } else if (o.kind == RL_O_CSG) {
      if (d.csgs[o.index].operation > RL_CSG_DIFFERENCE) return fail("unknown csg operation");
    }
    f->state = OPEN;
    st.push_back(Frame{o, 0, 0});
    return true;
  }
  bool survey_close(rl_oref o, size_t depth) {
    const uint32_t n = n_children(o);
    Facts sum{0, 0, DONE, 0, 0};
    uint32_t live = 0;  // children whose expansion holds an op, and the last of them
    rl_oref last{RL_O_NONE, 0};
    for (uint32_t i = 0; i < n; i++) {
      Facts c = facts_or_leaf(child(o, i));
      sum.ops = sat_add(sum.ops, c.ops);
      if (c.height + 1u > sum.height) sum.height = c.height + 1u;
      if (c.xform > sum.xform) sum.xform = c.xform;
      if (c.csg > sum.csg) sum.csg = c.csg;
      if (c.ops) live++, last = child(o, i);
    }
    switch (o.kind) {
      case RL_O_GROUP:  // a group with one such child expands to what that child expands to: `lower` goes there directly
        if (live == 1) group_is[o.index] = last.kind == RL_O_GROUP && group_is[last.index].kind != RL_O_NONE ? group_is[last.index] : last;
        break;
      case RL_O_BOUNDED: sum.ops = sat_add(sum.ops, 1); break;
      case RL_O_TRANSFORMED:
        sum.ops = sat_add(sum.ops, 2), sum.xform++;
        if (sum.xform > 8) return fail("Transformed nesting deeper than 8");
        break;
      default:
        sum.ops = sat_add(sum.ops, 3), sum.csg++;
        if (sum.csg > 4) return fail("CSG nesting deeper than 4");
    }
    if (depth + sum.height > MAX_NEST) return fail("scene graph too deep");
    *facts(o) = sum;
    return true;
  }
  bool survey() {
    std::vector<Frame> st;
    uint64_t total = 1;  // ROP_END
    for (uint32_t k = 0; k < d.n_objects; k++) {
      if (!survey_open(d.objects[k], st)) return false;
      while (!st.empty()) {
        const Frame fr = st.back();
        if (fr.next < n_children(fr.o)) {
          st.back().next++;
          if (!survey_open(child(fr.o, fr.next), st)) return false;
          continue;
        }
        st.pop_back();
        if (!survey_close(fr.o, st.size())) return false;
      }
      total = sat_add(total, facts_or_leaf(d.objects[k]).ops);
    }
    if (total >= MAX_OPS) return fail("program too large");
    p.ops.reserve((size_t)total);  // an upper bound: a graph the memory cannot hold fails here, before any work
    // as RtiowCompiler::survey: every place of group_items linked to the next one whose item's expansion holds an op
    next_live.assign((size_t)d.n_group_items + 1, d.n_group_items);
    for (uint32_t j = d.n_group_items; j-- > 0;) next_live[j] = item_ops(d.group_items[j]) ? j : next_live[j + 1];
    return true;
  }
  uint64_t item_ops(rl_oref o) const {  // of any group item, reached by the survey or not (then 0: `lower` never meets it)
    switch (o.kind) {
      case RL_O_TRIANGLE: return o.index < d.n_triangles;
      case RL_O_GROUP: return o.index < d.n_groups && f_group[o.index].state == DONE ? f_group[o.index].ops : 0;
      case RL_O_BOUNDED: return o.index < d.n_boundeds && f_bounded[o.index].state == DONE ? f_bounded[o.index].ops : 0;
      case RL_O_TRANSFORMED: return o.index < d.n_transformeds && f_xform[o.index].state == DONE ? f_xform[o.index].ops : 0;
      case RL_O_SPHERE:
      case RL_O_PLANE:
      case RL_O_CUBE:
      case RL_O_CYLINDER:
      case RL_O_CONE: return o.index < d.n_shapes;
      case RL_O_CSG: return o.index < d.n_csgs && f_csg[o.index].state == DONE ? f_csg[o.index].ops : 0;
      default: return 0;
    }
  }
  uint32_t live_child(rl_oref o, uint32_t next) const {  // the first child at or after `next` whose expansion holds an op
    if (o.kind != RL_O_GROUP) return next;
    const rl_rtc_group &g = d.groups[o.index];
    const uint64_t j = next_live[(size_t)g.first + next];
    return j - g.first < g.count ? (uint32_t)(j - g.first) : g.count;
  }

  // ---- lower (of a surveyed graph: nothing can fail any more)
  void lower_open(rl_oref o, std::vector<Frame> &st) {
    switch (o.kind) {
      case RL_O_TRIANGLE: emit_tri(o.index); return;
      case RL_O_SPHERE:
      case RL_O_PLANE:
      case RL_O_CUBE:
      case RL_O_CYLINDER:
      case RL_O_CONE: {
        DevOp op{};
        op.code = ROP_SHAPE, op.a = o.index;
        p.ops.push_back(op);
        p.needs_full = true;
        return;
      }
      case RL_O_CSG: {
        csg_depth++;
        if (csg_depth > p.max_csg_depth) p.max_csg_depth = csg_depth;
        DevOp op{};
        op.code = ROP_CSG_BEGIN, op.a = o.index;
        p.ops.push_back(op);
        st.push_back(Frame{o, 0, 0});
        return;
      }
      case RL_O_GROUP:
        if (!f_group[o.index].ops) return;
        if (group_is[o.index].kind != RL_O_NONE) return lower_open(group_is[o.index], st);  // never a group that forwards again
        st.push_back(Frame{o, 0, 0});  // two children or more that emit ops: the frame is paid for by them
        return;
      case RL_O_BOUNDED: {
        const rl_rtc_bounded &b = d.boundeds[o.index];
        uint32_t idx = (uint32_t)p.ops.size();
        DevOp op{};
        op.code = ROP_BOUNDS;
        op.box[0] = b.minimum[0], op.box[1] = b.maximum[0], op.box[2] = b.minimum[1], op.box[3] = b.maximum[1], op.box[4] = b.minimum[2],
        op.box[5] = b.maximum[2];
        p.ops.push_back(op);
        st.push_back(Frame{o, 0, idx});
        return;
      }
      default: {  // RL_O_TRANSFORMED
        uint32_t enter_pc = (uint32_t)p.ops.size();
        uint32_t parent = enter_stack.empty() ? NONE : enter_stack.back();
        DevOp op{};
        op.code = ROP_ENTER, op.a = o.index, op.b = parent;  // .b: pc of the enclosing ENTER (chain to the world ray)
        p.ops.push_back(op);
        enter_stack.push_back(enter_pc);
        if (enter_stack.size() > p.max_xform_depth) p.max_xform_depth = (uint32_t)enter_stack.size();
        st.push_back(Frame{o, 0, enter_pc});
        return;
      }
    }
  }
  void lower_between(const Frame &fr) {  // before child fr.next is opened
    if (fr.o.kind == RL_O_CSG && fr.next == 1) {
      DevOp mid{};
      mid.code = ROP_CSG_MID, mid.a = fr.o.index;
      p.ops.push_back(mid);
    }
  }
  void lower_close(const Frame &fr) {
    switch (fr.o.kind) {
      case RL_O_GROUP: return;
      case RL_O_BOUNDED: p.ops[fr.pc].skip = (uint32_t)p.ops.size(); return;
      case RL_O_CSG: {
        DevOp end{};
        end.code = ROP_CSG_END, end.a = fr.o.index;
        p.ops.push_back(end);
        csg_depth--;
        p.needs_full = true;
        return;
      }
      default: {
        enter_stack.pop_back();
        DevOp ex{};
        ex.code = ROP_EXIT, ex.a = fr.o.index, ex.skip = fr.pc, ex.b = enter_stack.empty() ? NONE : enter_stack.back();
        p.ops.push_back(ex);
        return;
      }
    }
  }
  void lower() {
    std::vector<Frame> st;
    for (uint32_t k = 0; k < d.n_objects; k++) {
      lower_open(d.objects[k], st);
      while (!st.empty()) {
        const Frame fr = st.back();
        const uint32_t next = live_child(fr.o, fr.next);
        if (next < n_children(fr.o)) {
          lower_between(fr);
          st.back().next = next + 1;
          lower_open(child(fr.o, next), st);
          continue;
        }
        st.pop_back();
        lower_close(fr);
      }
    }
  }
};
}  // namespace

int compile_rtc(const rl_rtc_scene_desc &d, RtcProgram &p, std::string &err) {
  auto need = [&](const void *ptr, uint32_t n, const char *what) {
    if (n && !ptr) {
      err = std::string("null array: ") + what;
      return false;
    }
    return true;
  };
  if (!need(d.triangles, d.n_triangles, "triangles") || !need(d.groups, d.n_groups, "groups") || !need(d.group_items, d.n_group_items, "group_items") ||
      !need(d.boundeds, d.n_boundeds, "boundeds") || !need(d.transformeds, d.n_transformeds, "transformeds") ||
      !need(d.materials, d.n_materials, "materials") || !need(d.objects, d.n_objects, "objects") || !need(d.lights, d.n_lights, "lights"))
    return RL_E_INVALID;
  for (uint32_t i = 0; i < d.n_triangles; i++) {
    const rl_rtc_triangle &t = d.triangles[i];
    if (t.material >= d.n_materials) {
      err = "triangle material out of range";
      return RL_E_INVALID;
    }
    DevTri dt{};
    std::memcpy(dt.p1, t.p1, 24), std::memcpy(dt.e1, t.e1, 24), std::memcpy(dt.e2, t.e2, 24);
    std::memcpy(dt.n1, t.n1, 24), std::memcpy(dt.n2, t.n2, 24), std::memcpy(dt.n3, t.n3, 24);
    dt.smooth = t.smooth, dt.material = t.material;
    p.tris.push_back(dt);
  }
  p.xforms.assign(d.transformeds, d.transformeds + d.n_transformeds);
  p.materials.assign(d.materials, d.materials + d.n_materials);
  p.lights.assign(d.lights, d.lights + d.n_lights);
  if (!need(d.shapes, d.n_shapes, "shapes") || !need(d.csgs, d.n_csgs, "csgs") || !need(d.patterns, d.n_patterns, "patterns")) return RL_E_INVALID;
  p.shapes.assign(d.shapes, d.shapes + d.n_shapes);
  p.csgs.assign(d.csgs, d.csgs + d.n_csgs);
  p.patterns.assign(d.patterns, d.patterns + d.n_patterns);
  for (const auto &sh : p.shapes)
    if (sh.material >= d.n_materials) {
      err = "shape material out of range";
      return RL_E_INVALID;
    }
  for (const auto &pt : p.patterns)
    if (pt.kind < RL_PAT_STRIPE || pt.kind > RL_PAT_CHECKER3D) {
      err = "unknown pattern kind";
      return RL_E_INVALID;
    }
  for (const auto &m : p.materials) {
    if (m.reflectivity != 0.0 || m.transparency != 0.0) p.needs_secondary = true;
    if (m.pattern > d.n_patterns) {
      err = "material pattern out of range";
      return RL_E_INVALID;
    }
    if (m.pattern != 0) p.needs_full = true;
  }
  if (p.needs_secondary) p.needs_full = true;
  p.max_reflection_depth = d.max_reflection_depth;
  std::memcpy(p.void_color, d.void_color, 24);
  RtcCompiler c(d, p, err);
  if (!c.survey()) return RL_E_INVALID;
  c.lower();
  DevOp end{};
  end.code = ROP_END;
  p.ops.push_back(end);
  return RL_OK;
}

}  // namespace rl
