// Internal (not part of the ABI): the host scene compiler — what a caller's scene description becomes before any device sees it.
// Plain C++ like rl_program.cpp and rl_fast_bvh.cpp, which it builds on: no HIP header, no device buffer, so that this half of the
// library also links into a stand-alone program and runs under the host sanitizers (tests/host/scene_host_check.cpp).
// rl_render.hip's rl_*_scene_create and rl_debug_host_structures are argument checks around the calls below.
#pragma once
#include <memory>
#include <string>
#include <vector>

#include "rl_program.h"

namespace rl {

// What the host side of a scene compiles to; immutable, shared by the per-device replicas of one scene.
struct HostRtiow {
  RtiowProgram rt;
  std::vector<DevOp> lops;  // linked ops (sphere-only scenes)
  std::vector<DevMaterial> sphere_flat;
  std::vector<DevChecker> sphere_checker;  // beside sphere_flat, one per sphere: a two-colour checker's odd colour and inv_scale
  std::vector<CompactOp> cops;  // guarded compact ops
  std::vector<uint32_t> movbits;
  uint32_t entry0 = 0, centry0 = 0;
  std::vector<FastNode> fast_nodes;  // fast traversal structure (rl_fast_bvh.cpp); fast_root == FAST_NONE: the scene does not qualify
  uint32_t fast_root = FAST_NONE;
  std::vector<FastNodeCH> fast_nodes_ch;  // fast_nodes as centre / half-extent boxes: what the wave kernels stage into LDS (fast_node_ch)
  std::vector<float> fast_leaf_boxes;  // [n_spheres][8]: each sphere's padded leaf box of the fast tree (rl_rtiow_coop.h)
  std::vector<double> fast_leaf_balls;  // [n_spheres][4]: centre and radius of a ball around each padded sphere (rl_fast_bvh.cpp fast_leaf_balls)
  std::vector<double> fast_leaf_motion;  // [n_spheres][4]: dc and |dc| / 2 of each sphere; fast_motion_finite: every value of both arrays is finite
  bool fast_motion_finite = false;
  FastGeneral fg;  // fast traversal structure of a general scene (fg.ok == false: the scene does not qualify)
  FastGeneral qfg;  // sphere-only scenes: the same structure for ray queries (rl_ray_query.h; the renders walk fast_nodes from LDS instead)
  const FastGeneral &query_tree() const { return fg.ok ? fg : qfg; }
  // the guard boxes' padding is rigorous for ray origins within guard_reach of guard_center (rl_scene_host.cpp link_ops)
  double guard_center[3] = {0, 0, 0}, guard_reach = 0;
};
struct HostRtc {
  RtcProgram rc;
  std::vector<RtcGuard> guards;
  // What rtc_kernel / rtc_pixels_kernel stage in LDS: ops, triangles, guards, in that order.  rtc_render_launch sizes the launch's dynamic LDS
  // with it and takes the global-memory instantiations above RTC_LDS_SCENE_MAX; rl_debug_rtc_program reports it.
  size_t scene_bytes() const { return rc.ops.size() * sizeof(DevOp) + rc.tris.size() * sizeof(DevTri) + guards.size() * sizeof(RtcGuard); }
};
static const size_t RTC_LDS_SCENE_MAX = 65536;

// Both return RL_OK, or the code the entry point hands on (RL_E_INVALID / RL_E_UNSUPPORTED / RL_E_NOMEM) with `err` filled; `out` is set on
// RL_OK only.  Neither throws (they are called from behind the C ABI), and neither recurses over the caller's graph: the limits a
// description must keep are listed in include/rl_render.h beside rl_rtiow_scene_create.
// RTIOW: validate + lower the graph, link the ops, flatten the materials, build the fast structures.
int build_host_rtiow(const rl_rtiow_scene_desc *desc, std::shared_ptr<const HostRtiow> &out, std::string &err);
// RTC: lower the graph, refuse what the device kernels have no room for (lights, pending rays), build the triangle guards.
int build_host_rtc(const rl_rtc_scene_desc &desc, std::shared_ptr<const HostRtc> &out, std::string &err);

// Self-check of the traversal structures `H` (= build_host_rtiow(desc)) holds, into out16[16]: [0] bit 0: sphere fast tree built, bit 1:
// general fast structure built; general structure: [1] items, [2] binary nodes, [3] four-wide nodes, [4] leaf entries reached from the
// root, [5] items reached more than once, [6] items never reached, [7] boxes that fail to contain what lies below them (child boxes of
// inner children; the vertices / swept spheres of world-space items), [8] depth of the four-wide tree; sphere tree: [9] inner nodes,
// [10] leaves reached, [11] spheres reached more than once or never, [12] boxes that fail to contain the swept sphere below, [13] depth;
// media: [14] how many, [15] one byte per medium (the first eight): FastMedium::shape, + 0x10 when the medium has a box node.
void host_structures_report(const rl_rtiow_scene_desc *desc, const HostRtiow &H, unsigned long long *out16);

}  // namespace rl
