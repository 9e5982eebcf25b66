// The launch half the RTIOW launchers share (rtiow_render_launch, rtiow_render_indep_launch, rtiow_render_pixels_launch in rl_render.hip;
// rtiow_ray_color_impl in rl_query_api.h).  Not a translation unit of its own: rl_render.hip includes it once, behind
// stage_params, and it uses that file's statics (g_sw, g_cus, g_lds_max, ensure_lds_attr, set_err, stage_params, FAST_STATS_KERNEL).
// Unlike rl_host_api.h it names kernels.  Each of three things exists once here:
//   kernel tables    — runtime flags -> template instantiation, one function per kernel family
//   LDS layouts      — fastg_prepare (fast general kernel), wave_general_lds (reference-order kernel)
//   persistent grid  — persistent_blocks and the two launch_persistent forms (parameter block by value / by pointer); coop_launch
//   launch log       — what those three funnels launched, by the kernel pointer's own name (rl_debug_rtiow_launch_log; tests assert routes from it)
// Routing (which family a call takes) and flow (passes, the cost-sorted two-phase render) stay with the launchers.
// A new flavour is one row in a table: taking a kernel's address is what instantiates it, so a table reaches exactly the kernels it names.
#pragma once

namespace {

// the body modes the wave-scheduled kernels are instantiated in (the INDEP / RAYS / PIXELS / MOMENTS constants of the *_kernel wrappers)
enum class Mode { FRAME, INDEP, RAYS, PIXELS, MOMENTS, PIXELS_MOMENTS };
using ValueKernel = void (*)(RtiowParams);
using PointerKernel = void (*)(const RtiowParams *);
using CoopKernel = void (*)(RtiowParams, CoopParams);

// ---- kernel tables

// Reference-order wave-scheduled general kernel (rl_rtiow_wave_general.h), 512 lanes per CU (2 waves per SIMD): the kernel needs ~200 VGPRs
// (~260 with the sin / Perlin / acos / atan2 code of scenes that have Noise textures or Image textures on spheres: TRANS).  At 768 lanes
// (168 VGPRs) the spills land in the TRAV loop and cost 2.3x (measured, cfg 4: 1101 vs 465 Mrays/s).
template <bool TRANS, bool STATS, bool MEDIA>
ValueKernel wave_general_row(Mode mode) {
  switch (mode) {
    case Mode::FRAME: return rtiow_wave_general_kernel<512, TRANS, STATS, MEDIA>;
    case Mode::INDEP: return rtiow_wave_general_indep_kernel<512, TRANS, STATS, MEDIA>;
    case Mode::RAYS: return rtiow_wave_general_rays_kernel<512, TRANS, STATS, MEDIA>;
    case Mode::PIXELS: return rtiow_wave_general_pixels_kernel<512, TRANS, STATS, MEDIA>;
    case Mode::MOMENTS: return rtiow_wave_general_moments_kernel<512, TRANS, STATS, MEDIA>;
    case Mode::PIXELS_MOMENTS: return rtiow_wave_general_pixels_moments_kernel<512, TRANS, STATS, MEDIA>;
  }
  return nullptr;
}
ValueKernel wave_general_kernel(Mode mode, bool trans, bool stats, bool media) {
  if (media) {
    if (trans) return stats ? wave_general_row<true, true, true>(mode) : wave_general_row<true, false, true>(mode);
    return stats ? wave_general_row<false, true, true>(mode) : wave_general_row<false, false, true>(mode);
  }
  if (trans) return stats ? wave_general_row<true, true, false>(mode) : wave_general_row<true, false, false>(mode);
  return stats ? wave_general_row<false, true, false>(mode) : wave_general_row<false, false, false>(mode);
}

// Fast general kernel (rl_rtiow_fastgen.h): <lanes per CU, stack entries per lane, TRANS, MEDIA>; fastg_prepare lays the LDS out to match.
template <int NT, int SD, bool TRANS, bool MEDIA>
PointerKernel fast_general_row(Mode mode) {
  switch (mode) {
    case Mode::FRAME: return rtiow_fast_general_kernel<NT, SD, TRANS, MEDIA>;
    case Mode::INDEP: return rtiow_fast_general_indep_kernel<NT, SD, TRANS, MEDIA>;
    case Mode::RAYS: return rtiow_fast_general_rays_kernel<NT, SD, TRANS, MEDIA>;
    case Mode::PIXELS: return rtiow_fast_general_pixels_kernel<NT, SD, TRANS, MEDIA>;
    case Mode::MOMENTS: return rtiow_fast_general_moments_kernel<NT, SD, TRANS, MEDIA>;
    case Mode::PIXELS_MOMENTS: return rtiow_fast_general_pixels_moments_kernel<NT, SD, TRANS, MEDIA>;
  }
  return nullptr;
}
// one_wave (fastg_one_wave): the one-wave-per-SIMD form exists for frame, indep and pixels only — null for the other modes, whose
// callers pass false (launch_persistent refuses a null kernel)
PointerKernel fast_general_kernel(Mode mode, bool trans, bool media, bool one_wave) {
  if (one_wave) {
    if (mode == Mode::FRAME) return rtiow_fast_general_kernel<256, 40, true, true>;
    if (mode == Mode::INDEP) return rtiow_fast_general_indep_kernel<256, 40, true, true>;
    if (mode == Mode::PIXELS) return rtiow_fast_general_pixels_kernel<256, 40, true, true>;
    return nullptr;
  }
  // several stages (media, unbounded Planes): the boundary walks and the Isotropic phase function need the 256-register budget
  if (media) return trans ? fast_general_row<512, 40, true, true>(mode) : fast_general_row<512, 40, false, true>(mode);
  // 512 lanes per CU (the transcendental texture code needs 256 VGPRs), 40-entry stacks
  if (trans) return fast_general_row<512, 40, true, false>(mode);
  // 768 lanes per CU (3 waves per SIMD hide more of the node-fetch latency), 20-entry stacks: 208 B of LDS per lane, and the
  // 4 KB that leaves of 160 KB hold the top 32 nodes of the tree (cfg 4 +1.1 %, cfg 5 +0.4 %; 128 nodes with 16-entry stacks: the same)
  return fast_general_row<768, 20, false, false>(mode);
}

// Cooperative one-wave-per-pixel kernel (rl_rtiow_coop.h), COOP_NW waves per workgroup: boxes in registers (two waves per SIMD) / from L2
// (the register budget of four waves per SIMD)
constexpr int COOP_NW = 4;
template <bool BOXES_IN_REGS, int REGS_FOR>
CoopKernel coop_row(bool pixels, bool moments) {
  if (pixels) return moments ? rtiow_coop_pixels_moments_kernel<COOP_NW, BOXES_IN_REGS, REGS_FOR> : rtiow_coop_pixels_kernel<COOP_NW, BOXES_IN_REGS, REGS_FOR>;
  return moments ? rtiow_coop_moments_kernel<COOP_NW, BOXES_IN_REGS, REGS_FOR> : rtiow_coop_kernel<COOP_NW, BOXES_IN_REGS, REGS_FOR>;
}
CoopKernel coop_kernel(bool pixels, bool moments, bool regs_mode) {
  return regs_mode ? coop_row<true, COOP_NW * 64>(pixels, moments) : coop_row<false, 1024>(pixels, moments);
}

// Wave-scheduled sphere kernel (rl_rtiow_wave.h), 1024 lanes per CU, by what lies in LDS next to the rings: 0 nothing (scene through L2),
// 2 linked ops, 3 guarded compact ops, 4 fast traversal nodes.  mode: FRAME, MOMENTS (never counting: route_moments_variant) or INDEP
// (layout 4, counter-free only).  Layout 4 counts only under rl_debug_fast_stats, and that instantiation exists in the verify build only
// (FAST_STATS_KERNEL: scheduler occupancy of the fast kernel, tools/sched.py; its box / sphere counts are its own); the stealing
// instantiation (resume launch of a small shard) exists for layout 4 only.
template <int LDS_SCENE>
ValueKernel wave_row(bool stats, bool moments) {
  if (moments) return rtiow_wave_moments_kernel<1024, LDS_SCENE>;
  return stats ? rtiow_wave_kernel<1024, LDS_SCENE, true> : rtiow_wave_kernel<1024, LDS_SCENE, false>;
}
ValueKernel wave_kernel(Mode mode, int lds_scene, bool stats, bool steal) {
  const bool moments = mode == Mode::MOMENTS;
  switch (lds_scene) {
    case 0: return wave_row<0>(stats, moments);
    case 2: return wave_row<2>(stats, moments);
    case 3: return wave_row<3>(stats, moments);
    case 4:
      if (mode == Mode::INDEP) return rtiow_wave_indep_kernel<1024, 4, false>;
      if (moments) return rtiow_wave_moments_kernel<1024, 4>;
      if (steal) return rtiow_wave_kernel<1024, 4, false, true>;
      return stats && FAST_STATS_KERNEL ? rtiow_wave_kernel<1024, 4, FAST_STATS_KERNEL> : rtiow_wave_kernel<1024, 4, false>;
  }
  return nullptr;
}

// ---- LDS layouts

// The flavour of the fast general kernel with both the media code and the Perlin / acos / atan2 code spills 126 VGPRs at 256 registers.  For small
// frames (at most three work items per lane of the 512-lane form: the frame's time is per-ray latency, and scratch round trips are part of
// it) it runs as ONE wave per SIMD with the 512-register budget instead (what would spill lives in AGPRs): final_scene.rs at 400x400 442 ->
// 522 Mrays/s, at 560x560 664 -> 782, at 640x640 786 -> 811; from 720x720 on the two-wave form wins (975 against 818; 1100 against 810
// at 1000x1000: the one-wave form's throughput ends at ~810 Mrays/s).  Measured and not taken: the same for the other flavours (quads.rs
// -17 %, flat_world.rs -24 %, cornell_smoke.rs at 600x600 -30 %: they spill little, and lose the second wave's latency hiding).
// RL_FASTG_NT256=1 / 0 forces it on / off (A/B).  work_items: the frame's pixels / the list's elements.
bool fastg_one_wave(bool trans, bool media, uint64_t work_items) {
  return trans && media && (g_sw.fastg_nt256 >= 0 ? g_sw.fastg_nt256 != 0 : work_items <= (uint64_t)g_cus * 1536u);
}

// LDS of a fast general launch, for the flavour fast_general_kernel(mode, trans, media, one_wave) returns: rings + the traversal stacks, and
// the tree's top in what is left (breadth first: FastGeneral::top_nodes).  tree: H.fg for the renders, the queries' own for the path query;
// media: that tree's stage_roots.size() > 1.  EFFECT on P: fg_top = the nodes staged, and (unless RL_TUNE set them) the kernel's tune defaults.
struct FastgLayout {
  int nt;
  size_t lds;
};
FastgLayout fastg_prepare(const FastGeneral &tree, bool trans, bool media, bool one_wave, RtiowParams &P) {
  // four steps per scheduling round (a step is an Infinity Cache / L2 round trip here, not an LDS one: lanes that fall out of TRAV
  // should not wait 24 of them): cfg 5 +6.6 %, cfg 4 +0.7 % against the sphere kernel's 24
  if (!g_sw.tune_set) P.tune[0] = 4, P.tune[2] = 4, P.tune[3] = FASTG_STEP_BUDGET;
  const int nt = one_wave ? 256 : (media || trans) ? 512 : 768, sd = (one_wave || media || trans) ? 40 : 20;
  const size_t base = (size_t)nt * (16 * sizeof(unsigned long long) + (size_t)sd * sizeof(uint32_t));
  const size_t room = g_lds_max > base ? (g_lds_max - base) / sizeof(FastNodeQ) : 0;
  P.fg_top = g_sw.fastg_top ? (uint32_t)std::min<size_t>(tree.top_nodes, std::min<size_t>(room, g_sw.fastg_top_max)) : 0u;
  size_t lds = base + (size_t)P.fg_top * sizeof(FastNodeQ);
  if (one_wave && lds < 90000) lds = 90000;  // one workgroup per CU
  return {nt, lds};
}

// LDS of a reference-order general launch (512 lanes): the rings, + the parked HitRecord of a medium scope: 96 B of LDS per lane
size_t wave_general_lds(bool media) { return (size_t)512 * (16 + (media ? MEDIA_SAVE_WORDS : 0)) * sizeof(unsigned long long); }

// ---- launch log
// Every launch of the three funnels below leaves one record in a process-wide ring of the last RTIOW_LAUNCH_LOG records (host only: one
// guarded copy per launch).  The kernel's name is asked of the runtime for the FUNCTION POINTER the launch was handed
// (hipKernelNameRefByPtr, demangled; once per distinct pointer), never derived from the flags that chose it: a table row that returns
// another instantiation than the one a test expects shows here even where both render the same bits.  api.RTIOW_LAUNCH mirrors the layout.
struct RtiowLaunchRecord {
  char kernel[192];       // e.g. "void rl::rtiow_wave_kernel<1024, 4, false, true>(rl::RtiowParams)"; "?" where the runtime knows no name
  uint64_t seq;           // 1 for the process's first launch
  uint64_t work_items;    // persistent funnels: the slots / list elements the grid was sized for; cooperative: n_pixels
  uint64_t lds_bytes;     // dynamic LDS
  uint32_t funnel;        // 0 parameter block by value, 1 by pointer, 2 coop_launch
  uint32_t wg_size, blocks;
  uint32_t sample_begin, sample_end, resume, has_tile_order, has_steal_state, fg_top, tune[4];  // of the RtiowParams launched
  uint32_t n_pixels;      // coop_launch: CoopParams::n_pixels; 0 otherwise
};
static_assert(sizeof(RtiowLaunchRecord) == 272, "api.RTIOW_LAUNCH states this layout");
constexpr unsigned RTIOW_LAUNCH_LOG = 64;
std::mutex g_launch_log_mu;
RtiowLaunchRecord g_launch_log[RTIOW_LAUNCH_LOG];
uint64_t g_launch_total = 0;
std::map<const void *, std::string> g_kernel_names;

void log_launch(const void *kern, hipStream_t stream, uint32_t funnel, uint32_t nt, uint32_t blocks, size_t lds, uint64_t work_items, const RtiowParams &P, uint32_t n_pixels) {
  std::lock_guard<std::mutex> lk(g_launch_log_mu);
  auto it = g_kernel_names.find(kern);
  if (it == g_kernel_names.end()) {
    const char *raw = hipKernelNameRefByPtr(kern, stream);
    std::string name = raw && *raw ? raw : "?";
    if (name.size() > 3 && name.compare(name.size() - 3, 3, ".kd") == 0) name.resize(name.size() - 3);  // (the descriptor's symbol)
    if (name.compare(0, 2, "_Z") == 0) {
      int status = 0;
      if (char *d = abi::__cxa_demangle(name.c_str(), nullptr, nullptr, &status)) {
        if (status == 0) name = d;
        std::free(d);
      }
    }
    it = g_kernel_names.emplace(kern, std::move(name)).first;
  }
  RtiowLaunchRecord &r = g_launch_log[g_launch_total % RTIOW_LAUNCH_LOG];
  r = RtiowLaunchRecord{};
  std::strncpy(r.kernel, it->second.c_str(), sizeof r.kernel - 1);
  r.seq = ++g_launch_total, r.work_items = work_items, r.lds_bytes = lds, r.funnel = funnel, r.wg_size = nt, r.blocks = blocks;
  r.sample_begin = P.sample_begin, r.sample_end = P.sample_end, r.resume = P.resume, r.has_tile_order = P.tile_order != nullptr, r.has_steal_state = P.steal_state != nullptr;
  r.fg_top = P.fg_top, r.tune[0] = P.tune[0], r.tune[1] = P.tune[1], r.tune[2] = P.tune[2], r.tune[3] = P.tune[3];
  r.n_pixels = n_pixels;
}

// ---- persistent grid

// persistent lanes: as many workgroups as stay resident (LDS, 2048 lanes per CU), at most one lane per work item
uint32_t persistent_blocks(uint64_t work_items, int nt, size_t lds) {
  uint32_t per_cu = (uint32_t)(g_lds_max / (lds ? lds : 1));
  if (per_cu < 1) per_cu = 1;
  if (per_cu * (uint32_t)nt > 2048) per_cu = 2048 / (uint32_t)nt;
  uint32_t blocks = (uint32_t)((work_items + nt - 1) / nt);
  if (blocks > (uint32_t)g_cus * per_cu) blocks = (uint32_t)g_cus * per_cu;
  if (g_sw.blocks_cap >= 1 && g_sw.blocks_cap < blocks) blocks = g_sw.blocks_cap;  // A/B only
  return blocks;
}
int launch_prepare(const void *kern, size_t lds) {
  if (!kern) return set_err(RL_E_UNSUPPORTED, "this kernel flavour does not exist");
  if (ensure_lds_attr(kern, lds) != 0) return set_err(RL_E_DEVICE, "hipFuncSetAttribute(MaxDynamicSharedMemorySize) failed");
  return RL_OK;
}
// parameter block by value (`scene` only makes the two forms' arguments the same)
int launch_persistent(ValueKernel kern, int nt, size_t lds, uint64_t work_items, const RtiowParams &P, const rl_scene *, hipStream_t stream) {
  int rc = launch_prepare((const void *)kern, lds);
  if (rc != RL_OK) return rc;
  const uint32_t blocks = persistent_blocks(work_items, nt, lds);
  hipLaunchKernelGGL(kern, dim3(blocks), dim3(nt), lds, stream, P);
  HIP_TRY(hipGetLastError());
  log_launch((const void *)kern, stream, 0, (uint32_t)nt, blocks, lds, work_items, P, 0);
  return RL_OK;
}
// by pointer: every launch its own stream-ordered device copy (stage_params: two slots)
int launch_persistent(PointerKernel kern, int nt, size_t lds, uint64_t work_items, const RtiowParams &P, const rl_scene *scene, hipStream_t stream) {
  int rc = launch_prepare((const void *)kern, lds);
  if (rc != RL_OK) return rc;
  const RtiowParams *slot = nullptr;
  if ((rc = stage_params(scene, P, stream, slot)) != RL_OK) return rc;
  const uint32_t blocks = persistent_blocks(work_items, nt, lds);
  hipLaunchKernelGGL(kern, dim3(blocks), dim3(nt), lds, stream, slot);
  HIP_TRY(hipGetLastError());
  log_launch((const void *)kern, stream, 1, (uint32_t)nt, blocks, lds, work_items, P, 0);
  return RL_OK;
}

// Cooperative kernel over n pixels (C.pixels: their list, or null for the list renders' own P.pix_xs / pix_ys; the caller has zeroed
// C.counter): one wave per pixel, at most 4 waves per SIMD at 128 VGPRs.  The lowest latency (boxes in registers: 3.3 us per ray, two waves
// per SIMD) while every pixel gets a wave at once; the register budget of four waves per SIMD (boxes from L2: 4.0 us per ray, +25 %
// throughput) for larger frames.  RL_COOP_MODE forces one (A/B).
int coop_launch(const RtiowParams &P, CoopParams C, uint64_t n, bool moments, bool pixels, hipStream_t stream) {
  C.n_pixels = (uint32_t)n, C.max_cand = 128;
  const size_t lds = (size_t)8 * COOP_NW * 64 * sizeof(unsigned long long) + (size_t)COOP_NW * C.max_cand * sizeof(uint32_t);
  uint32_t blocks = (uint32_t)((n + COOP_NW - 1) / COOP_NW);
  const uint32_t cap = (uint32_t)g_cus * (16 / COOP_NW);
  if (blocks > cap) blocks = cap;
  if (blocks == 0) return RL_OK;  // an empty frame shard (a list is never empty)
  const int mode = g_sw.coop_mode >= 0 ? g_sw.coop_mode : (n <= (uint64_t)g_cus * 8u ? 2 : 0);
  const CoopKernel kern = coop_kernel(pixels, moments, mode == 2);
  if (ensure_lds_attr((const void *)kern, lds) != 0) return set_err(RL_E_DEVICE, "hipFuncSetAttribute failed");
  hipLaunchKernelGGL(kern, dim3(blocks), dim3(COOP_NW * 64), lds, stream, P, C);
  HIP_TRY(hipGetLastError());
  log_launch((const void *)kern, stream, 2, COOP_NW * 64, blocks, lds, n, P, C.n_pixels);
  return RL_OK;
}

}  // namespace
