// rl_render.hip — the C ABI of include/rl_render.h over the gfx950 kernels (single-device entry points; rl_multi.hip drives
// several GPUs from one process on top of the launch halves defined here).  The one translation unit that instantiates the kernels.
// What a scene description compiles to on the host (linked ops, guards, fast trees, the structure report) is plain C++ of its own:
// rl_scene_host.cpp; rl_*_scene_create here are argument checks, that call, and the uploads.
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -fPIC -shared (see csrc/Makefile).
// No CPU fallback: every compute entry point fails with RL_E_NO_DEVICE unless rl_init succeeded on a GPU.
#include <hip/hip_runtime.h>

#include <cxxabi.h>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <atomic>
#include <cstring>
#include <limits>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "rl_scene.h"
#include "rl_rtc_kernel.h"
#include "rl_rtc_full_kernel.h"
#include "rl_rtiow_kernel.h"
#include "rl_rtiow_general.h"
#include "rl_rtiow_wave.h"
#include "rl_rtiow_wave_general.h"
#include "rl_rtiow_fastgen.h"
#include "rl_rtiow_coop.h"
#include "rl_pixel_entry.h"
#include "rl_ray_query.h"
#include "rl_material_query.h"
#include "rl_rtc_shade_query.h"
#include "rl_rtiow_features.h"
#include "rl_occlusion_query.h"

using namespace rl;

namespace {

thread_local std::string g_err;
std::mutex g_mu;
bool g_ready = false;
std::vector<DevCtx> g_ctx;  // [0] is the device rl_init chose; rl_init_multi appends the others
int g_cus = 0;
size_t g_lds_max = 65536;
// Every RL_* environment switch (A/B and debugging only: DESIGN.md section 3.6) is read ONCE, by rl_init; the render path reads this struct.
struct Switches {
  int rtiow_variant = 0;         // RL_RTIOW_KERNEL (0 = automatic)
  bool lpt = true;               // RL_LPT=0: single launch instead of the cost-sorted two-phase render
  bool coop_small = true;        // RL_COOP=0: small frames through the wave-scheduled kernel instead of the cooperative one
  unsigned long long coop_pixels_max = 0;  // RL_COOP_PIXELS_MAX=<n>: the longest pixel LIST the cooperative kernel takes (0 = default: 160 elements per CU, the frame path's bound)
  double steal_max_fill = 3.0;   // RL_STEAL=<pixels per lane> (0 = off): work stealing on small shards
  bool fast_traversal = true;    // RL_FAST=0: counter-free renders use the reference-order kernels too
  unsigned fastg_top_max = 512;  // RL_FASTG_TOP=<n > 1>: at most n nodes
  int rtc_blocks_per_cu = 0;     // RL_RTC_BLOCKS=<n>: workgroups per CU the RTC kernels are launched with (0 = as many as are resident at once: occupancy API)
  int fastg_nt256 = -1;          // RL_FASTG_NT256=0|1: never / always the one-wave-per-SIMD form of the fast general kernel (default: by frame size)
  bool fastg_top = true;         // RL_FASTG_TOP=0: the fast general kernel reads every node through L1 (A/B of the LDS tree top)
  bool tune_set = false;         // RL_TUNE="steps,floor16[,batch,fill]"
  unsigned tune[4] = {24, 6, 24, 40};
  unsigned blocks_cap = 0;       // RL_BLOCKS
  int coop_mode = -1;            // RL_COOP_MODE=2|0: boxes in registers / from L2 (any other value: as 0)
  bool rtc_force_full = false;   // RL_RTC_FORCE_FULL
  unsigned indep_k = 1;          // RL_INDEP_K=<k>: samples of one pixel per claim in the sample-parallel mode
  size_t indep_cap = (size_t)1 << 30;  // RL_INDEP_CAP_MB=<MiB>: cap of that mode's pass buffer (a smaller one forces more passes: tests)
  int pixel_entry = rl::PIXEL_ENTRY_DEFAULT;  // RL_PIXEL_ENTRY=0|1|2|3: the fast kernel's camera rays start at the root / at their pixel's entry cut of up to n entries (rl_pixel_entry.h)
  bool pixel_entry_sphere = true;  // RL_PIXEL_ENTRY_SPHERE=0: that cut keeps every leaf whose BOX the pixel's beam touches; default: only those whose sphere it may touch
  int pixel_entry_time = rl::PIXEL_ENTRY_TIME_DEFAULT;  // RL_PIXEL_ENTRY_TIME=1|2|4|8: time slices of that table, a word per pixel and slice (1: the one word for all times)
  bool pixel_entry_reuse = true;   // RL_PIXEL_ENTRY_REUSE=0: every call builds the table; default: a call that repeats the last build's camera, rows and switches reads it as it is
  bool coop_quad = true;         // RL_COOP_QUAD=0: the wave kernels' block passes lane-per-block only and FILL per lane (default: thin passes four lanes to a block, FILL wave-wide)
} g_sw;
std::atomic<unsigned long long> g_last_slow_traces{0};  // rl_debug_slow_traces.  Atomic: rl_render_status of two scenes runs under two locks.
// rl_debug_last_rtc_launch: the most recent rtc_render_launch of this process (kernel 0: none yet)
std::atomic<uint64_t> g_last_rtc_kernel{0}, g_last_rtc_list{0}, g_last_rtc_lds{0}, g_last_rtc_blocks{0};
// The instrumented fast sphere kernel rtiow_wave_kernel<1024, 4, true> (rl_debug_fast_stats, tools/sched.py) is compiled into the verify
// build only (make verify); in the product library rl_debug_fast_stats does nothing.
#ifdef RL_FASTG_VERIFY
constexpr bool FAST_STATS_KERNEL = true;
#else
constexpr bool FAST_STATS_KERNEL = false;
#endif
bool g_fast_debug_stats = false;  // verify build, tools only: counting renders run the fast kernel too (counters are then NOT the reference's)

void read_switches() {
  Switches w;
  if (const char *v = std::getenv("RL_RTIOW_KERNEL")) {
    std::string sv(v);
    w.rtiow_variant = sv == "v1" ? 1 : sv == "general" ? 2 : sv == "wavefront" ? 3 : sv == "wavegeneral" ? 4 : sv == "pool" ? 5 : sv == "pool256" ? 6 : sv == "wave2" ? 7 : sv == "wave256" ? 256 : sv == "wave512" ? 512 : sv == "wave768" ? 768 : sv == "wave1024" ? 1024 : sv == "wave1024ops" ? 1025 : sv == "wave1024guard" ? 1027 : sv == "wave1024fast" ? 1029 : sv == "coop" ? 1033 : 0;
  }
  if (const char *v = std::getenv("RL_LPT")) w.lpt = std::string(v) != "0";
  if (const char *v = std::getenv("RL_COOP")) w.coop_small = std::string(v) != "0";
  if (const char *v = std::getenv("RL_COOP_PIXELS_MAX")) w.coop_pixels_max = std::strtoull(v, nullptr, 10);
  if (const char *v = std::getenv("RL_STEAL")) w.steal_max_fill = std::atof(v);
  if (const char *v = std::getenv("RL_FAST")) w.fast_traversal = std::string(v) != "0";
  if (const char *t = std::getenv("RL_TUNE")) {
    unsigned a = 16, b = 12, c = 24, d = 40;
    int nf = std::sscanf(t, "%u,%u,%u,%u", &a, &b, &c, &d);
    if (nf >= 2) w.tune[0] = a, w.tune[1] = b, w.tune_set = true;
    if (nf >= 3) w.tune[2] = c;
    if (nf >= 4) w.tune[3] = d;
  }
  if (const char *v = std::getenv("RL_BLOCKS")) w.blocks_cap = (unsigned)std::atoi(v);
  if (const char *v = std::getenv("RL_COOP_MODE")) w.coop_mode = std::atoi(v);
  if (const char *v = std::getenv("RL_RTC_BLOCKS")) w.rtc_blocks_per_cu = std::max(0, std::atoi(v));
  if (const char *v = std::getenv("RL_FASTG_NT256")) w.fastg_nt256 = std::atoi(v) != 0;
  if (const char *v = std::getenv("RL_FASTG_TOP")) w.fastg_top = std::atoi(v) != 0, w.fastg_top_max = (unsigned)std::atoi(v) > 1u ? (unsigned)std::atoi(v) : 512u;
  w.rtc_force_full = std::getenv("RL_RTC_FORCE_FULL") != nullptr;
  if (const char *v = std::getenv("RL_INDEP_K")) w.indep_k = (unsigned)std::max(1, std::atoi(v));
  if (const char *v = std::getenv("RL_PIXEL_ENTRY")) w.pixel_entry = std::min(3, std::max(0, std::atoi(v)));
  if (const char *v = std::getenv("RL_PIXEL_ENTRY_SPHERE")) w.pixel_entry_sphere = std::string(v) != "0";
  if (const char *v = std::getenv("RL_PIXEL_ENTRY_TIME")) w.pixel_entry_time = rl::pixel_entry_slices(std::atoi(v));
  if (const char *v = std::getenv("RL_PIXEL_ENTRY_REUSE")) w.pixel_entry_reuse = std::string(v) != "0";
  if (const char *v = std::getenv("RL_COOP_QUAD")) w.coop_quad = std::string(v) != "0";
  if (const char *v = std::getenv("RL_INDEP_CAP_MB")) w.indep_cap = (size_t)std::max(1, std::atoi(v)) << 20;
  g_sw = w;
}

// hipFuncAttributeMaxDynamicSharedMemorySize is sticky per (kernel, device): set it when a launch needs more than any before it did
std::map<std::pair<const void *, int>, size_t> g_lds_attr;
int ensure_lds_attr(const void *kern, size_t lds) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) dev = 0;
  std::lock_guard<std::mutex> lk(g_mu);
  size_t &have = g_lds_attr[{kern, dev}];
  if (lds <= have) return 0;
  if (hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) return -1;
  have = lds;
  return 0;
}

int set_err(int code, const std::string &m) {
  g_err = m;
  return code;
}
#define HIP_TRY(expr)                                                                              \
  do {                                                                                             \
    hipError_t e_ = (expr);                                                                        \
    if (e_ != hipSuccess) return set_err(RL_E_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_)); \
  } while (0)

__global__ void iota_u32(uint32_t *out, uint32_t n) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = i;
}

// Output stages
// one channel's byte; also what denoise_finish_kernel (rl_denoise_render.h) writes, with inv_samples = 1
__device__ inline unsigned char rtiow_rgb8_of(double sum, double inv_samples) {
  double v = sum * inv_samples;                                                    // camera.rs:293
  double s = v <= 0.0031308 ? 12.92 * v : (1.0 + 0.055) * pow(v, 1.0 / 2.4) - 0.055;  // color.rs:130-136
  double f = floor(s * 255.999);                                                   // color.rs:47-50 (as i16 saturates; NaN -> 0)
  int q = isnan(f) ? 0 : (f >= 32767.0 ? 32767 : (f <= -32768.0 ? -32768 : (int)f));
  return (unsigned char)(q < 0 ? 0 : (q > 255 ? 255 : q));
}
__global__ void encode_rtiow_rgb8(const double *sum, unsigned long long n_vals, double inv_samples, unsigned char *out) {
  unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_vals) return;
  out[i] = rtiow_rgb8_of(sum[i], inv_samples);
}
__global__ void encode_rtc_rgb8(const double *rgb, unsigned long long n_vals, unsigned char *out) {
  unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_vals) return;
  double v = round(rgb[i] * 255.0);  // canvas.rs:53-56: f64::round = half away from zero; as i32 saturates
  int q = isnan(v) ? 0 : (v >= 2147483647.0 ? 2147483647 : (v <= -2147483648.0 ? (int)-2147483648LL : (int)v));
  out[i] = (unsigned char)(q < 0 ? 0 : (q > 255 ? 255 : q));
}

// Test hook (rl_debug_set_status_gap): one lane holds its stream for `ticks` of the 100 MHz wall clock.  Each s_sleep(127) lasts
// 127 x 64 shader clocks (>= 3 us at any clock up to 2.7 GHz), so `max_sleeps` = the wait in us ends the loop even if the clock stalls.
__global__ void status_gap_wait(unsigned long long ticks, unsigned max_sleeps) {
  const unsigned long long t0 = wall_clock64();
  for (unsigned n = 0; n < max_sleeps && wall_clock64() - t0 < ticks; n++) __builtin_amdgcn_s_sleep(127);
}
unsigned g_status_gap_dev_us = 0, g_status_gap_host_us = 0;  // rl_debug_set_status_gap (0 / 0: off)

int init_context(DevCtx &c, int device) {
  c.device = device;
  HIP_TRY(hipSetDevice(device));
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, device));
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return set_err(RL_E_NO_DEVICE, std::string("device is ") + prop.gcnArchName + ", this library carries gfx950 code only");
  g_cus = prop.multiProcessorCount;
  g_lds_max = prop.sharedMemPerBlock > 65536 ? prop.sharedMemPerBlock : 65536;
  if (prop.maxSharedMemoryPerMultiProcessor > g_lds_max) g_lds_max = prop.maxSharedMemoryPerMultiProcessor;
  if (g_lds_max > 163840) g_lds_max = 163840;
  if (!c.stream) HIP_TRY(hipStreamCreateWithFlags(&c.stream, hipStreamNonBlocking));
  if (!c.ev) HIP_TRY(hipEventCreateWithFlags(&c.ev, hipEventDisableTiming));
  return RL_OK;
}

}  // namespace

namespace rl {
int set_err_public(int code, const std::string &m) { return set_err(code, m); }  // for rl_bvh_build.hip / rl_multi.hip
bool lib_ready() { return g_ready; }
int n_contexts() { return (int)g_ctx.size(); }
DevCtx &context(int i) { return g_ctx[(size_t)i]; }
int use_context(int i) {
  HIP_TRY(hipSetDevice(g_ctx[(size_t)i].device));
  return RL_OK;
}
// rl_multi.hip: (re)build the context list — devices[g] for context g; context 0 keeps its stream when the device is unchanged
int set_contexts(const std::vector<int> &devices) {
  std::lock_guard<std::mutex> lk(g_mu);
  for (size_t i = devices.size(); i < g_ctx.size(); i++) {
    if (g_ctx[i].stream && hipSetDevice(g_ctx[i].device) == hipSuccess) hipStreamDestroy(g_ctx[i].stream), hipEventDestroy(g_ctx[i].ev);
  }
  g_ctx.resize(devices.size());
  for (size_t i = 0; i < devices.size(); i++) {
    if (g_ctx[i].stream && g_ctx[i].device != devices[i]) {
      hipSetDevice(g_ctx[i].device);
      hipStreamDestroy(g_ctx[i].stream), hipEventDestroy(g_ctx[i].ev);
      g_ctx[i] = DevCtx{};
    }
    int rc = init_context(g_ctx[i], devices[i]);
    if (rc != RL_OK) return rc;
  }
  if (!g_ctx.empty()) hipSetDevice(g_ctx[0].device);
  return RL_OK;
}
int sort_tiles_by_cost_desc(const uint32_t *d_cost, uint32_t *d_keys_tmp, uint32_t *d_order_in, uint32_t *d_order_out, uint32_t n, DevBuf<unsigned char> &temp,
                            hipStream_t stream);  // rl_bvh_build.hip (hipCUB)
void add_stats(rl_stats *acc, const rl_stats &s) {
  acc->rays += s.rays, acc->node_tests += s.node_tests, acc->sphere_tests += s.sphere_tests, acc->planar_tests += s.planar_tests;
  acc->instance_enters += s.instance_enters, acc->rng_words += s.rng_words, acc->flagged += s.flagged;
  acc->kernel_ms = std::max(acc->kernel_ms, s.kernel_ms);
}
}  // namespace rl

static void destroy_one(rl_scene *s) {
  if ((size_t)s->ctx < g_ctx.size()) hipSetDevice(g_ctx[(size_t)s->ctx].device);
  delete s;
}

// One replica per device context (rl_init: one; rl_init_multi: one per GPU — the scene is replicated): upload(g) makes
// context g's with that context's device current.  All of them or none; the current device is context 0's again afterwards.
template <class Upload>
static rl_scene *create_replicas(Upload upload) {
  std::vector<rl_scene *> reps;
  for (int g = 0; g < (int)g_ctx.size(); g++) {
    rl_scene *r = rl::use_context(g) == RL_OK ? upload(g) : nullptr;
    if (!r) {
      for (rl_scene *q : reps) destroy_one(q);
      hipSetDevice(g_ctx[0].device);
      return nullptr;
    }
    reps.push_back(r);
  }
  hipSetDevice(g_ctx[0].device);
  if (reps.size() > 1) reps[0]->replicas = reps;
  return reps[0];
}

extern "C" {

int rl_abi_version(void) { return RL_ABI_VERSION; }
const char *rl_last_error(void) { return g_err.c_str(); }

int rl_init(int device) {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0) return set_err(RL_E_NO_DEVICE, "no HIP device visible (this library has no CPU fallback)");
  if (device >= n) return set_err(RL_E_INVALID, "device index out of range");
  if (device < 0) HIP_TRY(hipGetDevice(&device));
  rl::drop_multi_state();
  int rc = rl::set_contexts({device});
  if (rc != RL_OK) return rc;
  read_switches();
  g_ready = true;
  return RL_OK;
}

void rl_shutdown(void) {
  rl::drop_multi_state();
  std::lock_guard<std::mutex> lk(g_mu);
  for (DevCtx &c : g_ctx)
    if (c.stream && hipSetDevice(c.device) == hipSuccess) hipStreamDestroy(c.stream), hipEventDestroy(c.ev);
  g_ctx.clear();
  g_ready = false;
}

int rl_device_info(char *name, int cap) {
  if (!g_ready) return set_err(RL_E_NO_DEVICE, "rl_init has not succeeded");
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, g_ctx[0].device));
  if (name && cap > 0) {
    std::strncpy(name, prop.gcnArchName, (size_t)cap - 1);
    name[cap - 1] = 0;
  }
  return prop.multiProcessorCount;
}

void rl_scene_destroy(rl_scene *s) {
  if (!s) return;
  for (size_t g = 1; g < s->replicas.size(); g++) destroy_one(s->replicas[g]);
  destroy_one(s);
  if (!g_ctx.empty()) hipSetDevice(g_ctx[0].device);
}

static int scene_common(rl_scene *s) {
  HIP_TRY(s->d_scratch.reserve(512));
  HIP_TRY(hipMemset(s->d_scratch, 0, 512));
  HIP_TRY(s->ev0.create());
  HIP_TRY(s->ev1.create());
  for (Event &e : s->ev_status) HIP_TRY(e.create(hipEventDisableTiming));
  HIP_TRY(s->ev_last.create(hipEventDisableTiming));
  HIP_TRY(s->h_status.reserve((size_t)rl_scene::N_STATUS * 8, hipHostMallocDefault));
  std::memset(s->h_status, 0, (size_t)rl_scene::N_STATUS * 64);
  return RL_OK;
}

// Device half of rl_rtiow_scene_create (the host half: rl_scene_host.cpp build_host_rtiow): one replica on device context `ctx`
// (the current device must already be that context's)
static rl_scene *upload_rtiow(const std::shared_ptr<const HostRtiow> &H, int ctx) {
  rl_scene *s = new rl_scene();
  s->kind = 1, s->ctx = ctx, s->device = g_ctx[(size_t)ctx].device, s->hrt = H;
  const RtiowProgram &rt = H->rt;
  const FastGeneral &QF = H->query_tree();  // general scenes: the renders' tree; sphere-only scenes: the queries' own
  int rc = RL_OK;
  if ((rc = s->d_ops.upload(rt.ops)) || (rc = s->d_spheres.upload(rt.spheres)) || (rc = s->d_sphere_material.upload(rt.sphere_material)) ||
      (rc = s->d_planars.upload(rt.planars)) || (rc = s->d_translates.upload(rt.translates)) || (rc = s->d_transforms.upload(rt.transforms)) ||
      (rc = s->d_materials.upload(rt.materials)) || (rc = s->d_textures.upload(rt.textures)) || (rc = s->d_images.upload(rt.images)) ||
      (rc = s->d_image_pool.upload(rt.image_pool)) || (rc = s->d_perlins.upload(rt.perlins)) || (rc = s->d_media.upload(rt.media)) ||
      (rc = scene_common(s)) ||
      (!H->lops.empty() && ((rc = s->d_lops.upload(H->lops)) || (rc = s->d_sphere_flat.upload(H->sphere_flat)) || (rc = s->d_sphere_checker.upload(H->sphere_checker)))) ||
      (!H->cops.empty() && ((rc = s->d_cops.upload(H->cops)) || (rc = s->d_movbits.upload(H->movbits)))) ||
      (H->fast_root != FAST_NONE && ((rc = s->d_fast_nodes.upload(H->fast_nodes)) || (rc = s->d_fast_nodes_ch.upload(H->fast_nodes_ch)) || (rc = s->d_fast_leaf_boxes.upload(H->fast_leaf_boxes)) ||
                                      (rc = s->d_fast_leaf_balls.upload(H->fast_leaf_balls)) || (rc = s->d_fast_leaf_motion.upload(H->fast_leaf_motion)))) ||
      (QF.ok && ((rc = s->d_fg_nodes.upload(QF.qnodes)) || (rc = s->d_fg_seg_roots.upload(QF.stage_roots)) ||
                 (rc = s->d_fg_media.upload(QF.media)) || (rc = s->d_fg_items.upload(QF.items)) || (rc = s->d_fg_spheres.upload(QF.item_spheres)) || (rc = s->d_fg_material.upload(QF.item_material))))) {
    destroy_one(s);
    return nullptr;
  }
  return s;
}

rl_scene *rl_rtiow_scene_create(const rl_rtiow_scene_desc *desc) {
  if (!g_ready) {
    set_err(RL_E_NO_DEVICE, "rl_init has not succeeded (no GPU, or not called)");
    return nullptr;
  }
  if (!desc) {
    set_err(RL_E_INVALID, "null scene descriptor");
    return nullptr;
  }
  std::shared_ptr<const HostRtiow> H;
  std::string err;
  if (int rc = build_host_rtiow(desc, H, err)) {
    set_err(rc, err);
    return nullptr;
  }
  return create_replicas([&](int g) { return upload_rtiow(H, g); });
}

// ChaCha8Rng::seed_from_u64 (rand_core 0.6.4): PCG32 expands the u64 into the 256-bit key
static void chacha_key_from_seed(uint64_t state, uint32_t key[8]) {
  const uint64_t MUL = 6364136223846793005ull, INC = 11634580027462260723ull;
  for (int k = 0; k < 8; k++) {
    state = state * MUL + INC;
    uint32_t xorshifted = (uint32_t)(((state >> 18) ^ state) >> 27);
    uint32_t rot = (uint32_t)(state >> 59);
    key[k] = (xorshifted >> rot) | (xorshifted << ((32 - rot) & 31));
  }
}

static void read_stats(const unsigned long long *h, float ms, rl_stats *st) {
  st->rays = h[0], st->node_tests = h[1], st->sphere_tests = h[2], st->planar_tests = h[3];
  st->instance_enters = h[4], st->rng_words = h[5], st->flagged = h[6];
  st->kernel_ms = ms;
}

}  // extern "C"

namespace rl {
// counting renders: ev0 / ev1 bracket the kernels on `stream`; the stats words are read back synchronously
int collect_stats(const rl_scene *scene, hipStream_t stream, rl_stats *st) {
  unsigned long long h[8];
  HIP_TRY(hipMemcpyAsync(h, scene->d_scratch + 64, sizeof h, hipMemcpyDeviceToHost, stream));
  {
    int rc = mark_render_end(scene, stream);
    if (rc != RL_OK) return rc;
  }
  HIP_TRY(hipStreamSynchronize(stream));
  float ms = 0.f;
  HIP_TRY(hipEventElapsedTime(&ms, scene->ev0, scene->ev1));
  read_stats(h, ms, st);
  if (st->flagged) return set_err(RL_E_DEGENERATE, "a reference panic site was reached (see stats.flagged)");
  return RL_OK;
}
}  // namespace rl

namespace rl {
// one finished slot of the status ring -> the scene's folded figures (rays: of the most recently enqueued render)
static void fold_status(rl_scene *ms, int slot) {
  const unsigned long long *h = ms->h_status + (size_t)slot * 8;
  ms->folded_flagged += h[6], ms->folded_slow += h[7];
  if (ms->status_seq[slot] > ms->folded_seq) ms->folded_seq = ms->status_seq[slot], ms->folded_rays = h[0];
  ms->status_pending[slot] = false;
}
// asynchronous renders: leave the stats words in pinned host memory behind an event (rl_render_status reads them).  Caller holds scene->mu.
// The render ends HERE, not at its last kernel: ev_last follows the copy, so that the next render of the scene on another stream (which
// waits only for ev_last) cannot zero or add to d_scratch before this render's counters have been read.
int post_status(const rl_scene *scene, hipStream_t stream) {
  rl_scene *ms = const_cast<rl_scene *>(scene);
  const int slot = ms->status_next;
  if (ms->status_pending[slot]) {  // the ring has come round: N_STATUS renders are in flight, wait for the oldest
    HIP_TRY(hipEventSynchronize(ms->ev_status[slot]));
    fold_status(ms, slot);
  }
  if (g_status_gap_dev_us) {  // test hook: widen the window between the render's last kernel and this copy
    hipLaunchKernelGGL(status_gap_wait, dim3(1), dim3(1), 0, stream, (unsigned long long)g_status_gap_dev_us * 100ull, g_status_gap_dev_us);
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipMemcpyAsync(ms->h_status + (size_t)slot * 8, scene->d_scratch + 64, 64, hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipEventRecord(ms->ev_status[slot], stream));
  ms->status_pending[slot] = true, ms->status_seq[slot] = ++ms->next_seq;
  ms->status_next = (slot + 1) % rl_scene::N_STATUS;
  return mark_render_end(scene, stream);
}
int order_after_previous(const rl_scene *scene, hipStream_t stream) {
  if (scene->has_last && scene->last_stream != stream) HIP_TRY(hipStreamWaitEvent(stream, scene->ev_last, 0));
  return RL_OK;
}
unsigned status_gap_host_us() { return g_status_gap_host_us; }
int mark_render_end(const rl_scene *scene, hipStream_t stream) {  // collect_stats / post_status, behind the render's stats copy
  rl_scene *ms = const_cast<rl_scene *>(scene);
  HIP_TRY(hipEventRecord(ms->ev_last, stream));
  ms->last_stream = stream, ms->has_last = true;
  return RL_OK;
}
}  // namespace rl
using rl::post_status;

#include "rl_host_api.h"  // scene_context, render_check, render_run, HostStaging

// The parameter block of one render (what every RTIOW kernel receives): scene pointers, derived camera, ChaCha key, shard geometry.
static int fill_rtiow_params(const rl_scene *scene, const rl_rtiow_camera *cam, uint64_t first_sample, uint32_t row_first, uint32_t row_step, uint32_t nrows, void *d_out,
                             bool want_stats, RtiowParams &P, uint64_t &slots) {
  const RtiowProgram &rt = scene->rt();
  const HostRtiow &H = *scene->hrt;
  const uint32_t W = cam->image_width;
  P = RtiowParams{};
  P.ops = scene->d_ops, P.spheres = scene->d_spheres, P.sphere_material = scene->d_sphere_material;
  P.planars = scene->d_planars, P.translates = scene->d_translates, P.transforms = scene->d_transforms;
  P.materials = scene->d_materials, P.textures = scene->d_textures, P.images = scene->d_images, P.image_pool = scene->d_image_pool, P.perlins = scene->d_perlins, P.media = scene->d_media;
  P.n_ops = (uint32_t)rt.ops.size(), P.n_spheres = (uint32_t)rt.spheres.size();
  P.lops = scene->d_lops, P.entry0 = H.entry0, P.sphere_flat = scene->d_sphere_flat, P.sphere_checker = scene->d_sphere_checker;
  P.cops = scene->d_cops, P.n_cops = (uint32_t)H.cops.size(), P.centry0 = H.centry0, P.movbits = scene->d_movbits;
  P.fast_nodes = scene->d_fast_nodes, P.fast_nodes_ch = scene->d_fast_nodes_ch, P.n_fast_inner = (uint32_t)H.fast_nodes.size(), P.fast_root = H.fast_root;
  P.fg_nodes = scene->d_fg_nodes, P.fg_items = scene->d_fg_items, P.fg_spheres = scene->d_fg_spheres, P.fg_material = scene->d_fg_material, P.fg_root = H.fg.qroot, P.fg_rsafe2 = H.fg.r_safe * H.fg.r_safe * 0.9999f;  // binary32 evaluation on the device: keep a margin
  P.fg_seg_roots = scene->d_fg_seg_roots, P.fg_media = scene->d_fg_media, P.fg_n_seg = (uint32_t)H.fg.stage_roots.size();
  P.fg_top = 0;  // (set by the launch that stages it: fastg_prepare)
  P.fg_center[0] = H.fg.center[0], P.fg_center[1] = H.fg.center[1], P.fg_center[2] = H.fg.center[2];
  P.fg_radius = H.fg.radius, P.fg_pad_k = H.fg.pad_k;
  P.cam = *cam;
  chacha_key_from_seed(cam->seed, P.key);
  P.first_sample = first_sample;
  P.row_first = row_first, P.row_step = row_step, P.nrows = nrows;
  P.tiles_x = (W + 7) / 8;
  slots = (uint64_t)P.tiles_x * ((nrows + 7) / 8) * 64ull;
  if (slots >= 0xFFFF0000ull) return set_err(RL_E_INVALID, "image too large");
  P.n_slots = (uint32_t)slots;
  P.work_counter = (uint32_t *)scene->d_scratch.get();
  P.stats = (unsigned long long *)(scene->d_scratch + 64);
  P.out = (double *)d_out;
  P.k8u = 8.8817841970012523e-16;
  P.tune[0] = g_sw.tune[0], P.tune[1] = g_sw.tune[1], P.tune[2] = g_sw.tune[2], P.tune[3] = g_sw.tune[3];
  P.pix_rays = want_stats ? scene->d_pix_rays : nullptr;
  P.coop_quad = g_sw.coop_quad ? 1u : 0u;
  return RL_OK;
}

// Which kernel renders this frame (RL_RTIOW_KERNEL / rl_debug_set_rtiow_variant force one where the scene qualifies), and the LDS bytes of its scene part.
struct RtiowChoice {
  int variant = 0;
  bool general = false;
  size_t compact_bytes = 0, fast_bytes = 0;
  bool fits_fast = false;
};
static int choose_rtiow_variant(const rl_scene *scene, const rl_rtiow_camera *cam, const RtiowParams &P, uint32_t nrows, bool want_stats, RtiowChoice &out) {
  const RtiowProgram &rt = scene->rt();
  const HostRtiow &H = *scene->hrt;
  const uint32_t W = cam->image_width, n_cops = P.n_cops;
  // ---- kernel variant.  The PRODUCT library carries, for sphere-only worlds, the four layouts the automatic choice below can reach
  // (1029 fast traversal / 1027 guarded compact ops / 1025 linked ops in LDS / 1024 scene through L2), the cooperative kernel (1033) and
  // the nested-loop all-primitives kernel (2: the A/B reference the tests compare against); for general worlds 1031 (fast traversal) and
  // 4 (reference order).  The variants that were measured and lost (v1, wavefront, pool, pool256, wave2, wave256 / 512 / 768, the
  // wavefront form of the general fast traversal) were retired; their numbers still get an explicit answer.
  int variant = g_sw.rtiow_variant;
  const bool general = rt.has_planars || rt.has_instances || rt.has_images || rt.has_noise || rt.has_media;
  // a ConstantMedium (RL_H_MEDIUM) draws from the pixel's RNG where the reference's fold reaches it: the reference-order kernels evaluate
  // it as a scope of the threaded program (wave-scheduled) or by recursion (RL_RTIOW_KERNEL=general); the fast traversal walks one tree per
  // program segment between two media (rl_rtiow_fastgen.h MEDIA) — counter-free renders only, as for every fast traversal
  if (rt.has_media && variant != 2 && variant != 0 && variant != 1031) variant = 4;
  for (int retired : {1, 3, 5, 6, 7, 256, 512, 768, 1035})
    if (variant == retired) return set_err(RL_E_UNSUPPORTED, "this kernel variant was retired: it was measured and lost (DESIGN.md §3.5), and its code is no longer in the library");
  // 1031 = the FAST traversal for general scenes (rl_rtiow_fastgen.h): counter-free renders only, like 1029
  const bool fits_fastg = general && H.fg.ok && (!want_stats) && g_sw.fast_traversal;
  if (variant == 2) variant = 2;               // the nested-loop all-primitives kernel (A/B reference)
  else if ((variant == 0 || variant == 1031) && fits_fastg) variant = 1031;
  else if (general || variant == 4 || variant == 1031) variant = 4;  // wave-scheduled all-primitives kernel (scene read from HBM/L2)
  const size_t compact_bytes = ((size_t)n_cops * sizeof(CompactOp) + (((size_t)P.n_spheres + 31) / 32 + 1) * sizeof(uint32_t) + 15) & ~(size_t)15;
  bool fits_compact = n_cops != 0 && (size_t)16 * 1024 * sizeof(unsigned long long) + compact_bytes <= g_lds_max;
  if (fits_compact) {
    // the guard boxes' padding covers the rounding of Sphere::hit only for ray origins within guard_reach of the scene
    // (rl_scene_host.cpp link_ops); every later origin is a hit point inside the scene, so only the camera has to be checked
    double far = 0.0;
    for (int k = 0; k < 3; k++) {
      double c = cam->lookfrom[k] - H.guard_center[k];
      far += c * c;
    }
    double disk = 0.0;
    for (int k = 0; k < 3; k++) disk += std::fabs(cam->defocus_disk_u[k]) + std::fabs(cam->defocus_disk_v[k]);
    if (!(std::sqrt(far) + disk <= H.guard_reach)) fits_compact = false;  // also for NaN
  }
  // 1029 = the FAST traversal (ordered binary tree, reject-only boxes, exact re-trace of ambiguous rays): counter-free renders only —
  // its box / sphere test counts are not the reference's, so a render that asks for rl_stats runs the counting kernel (1027)
  const size_t fast_bytes = ((size_t)P.n_fast_inner * sizeof(FastNodeCH) + 2 * (((size_t)P.n_spheres + 31) / 32 + 1) * sizeof(uint32_t) + 15) & ~(size_t)15;
  const bool fits_fast = fits_compact && H.fast_root != FAST_NONE && (!want_stats || g_fast_debug_stats) && (size_t)16 * 1024 * sizeof(unsigned long long) + fast_bytes <= g_lds_max &&
                         g_sw.fast_traversal;
  const bool fits_ops = (size_t)16 * 1024 * sizeof(unsigned long long) + (size_t)P.n_ops * sizeof(DevOp) <= g_lds_max;
  if (variant == 1029 && (general || !fits_fast)) variant = 0;
  if (variant == 1033 && (general || !fits_fast || want_stats)) variant = 0;  // cooperative kernel: the fast structure's scenes, counter-free renders
  if (variant == 1027 && (general || !fits_compact)) variant = 0;
  if (variant == 1025 && (general || !fits_ops)) variant = 0;
  if (variant == 0 && !general) {
    // automatic: 4 waves per SIMD (1024 lanes per CU, 128 KB of ChaCha rings) with, in LDS next to the rings, the fast tree / the
    // guarded compact ops / the linked ops — whichever fits first — and otherwise the whole scene read through L2
    variant = fits_fast ? 1029 : fits_compact ? 1027 : fits_ops ? 1025 : 1024;
    // Small frames (at most 10 pixels per wave the GPU can hold) are pure latency: every pixel's sample chain runs alone, and the
    // cooperative one-wave-per-pixel kernel advances a chain in 3.9 us per ray instead of ~22 (rl_rtiow_coop.h).  Measured at 1024 spp:
    // 2.2 k pixels 184 -> 30 ms, 9 k 248 -> 68, 20 k 267 -> 109, 37 k 264 -> 167, 90 k 291 -> 380 (tools/coop_check.py); from ~40 k
    // pixels on the wave-scheduled kernel with work stealing is as fast or faster (37 k: 173 ms, 90 k: 170 ms; tools/steal_ab.py).
    if (variant == 1029 && !want_stats && g_sw.coop_small && (uint64_t)nrows * W <= (uint64_t)g_cus * 16u * 10u) variant = 1033;
  }
  // 1029 keeps a path's remaining depth in 22 bits (rl_rtiow_wave.h, the self-test skip): deeper paths take the next layout that fits
  if (variant == 1029 && cam->max_depth > FAST_DEPTH_MASK) variant = fits_compact ? 1027 : fits_ops ? 1025 : 1024;
  out.variant = variant, out.general = general, out.compact_bytes = compact_bytes, out.fast_bytes = fast_bytes, out.fits_fast = fits_fast;
  return RL_OK;
}

// Where a MOMENTS frame (rl_rtiow_render_moments*) goes.  The flavour exists in the counter-free wave kernel (1029 / 1027 /
// 1025 / 1024), the cooperative kernel (1033), the fast general kernel (1031) and the reference-order wave general kernel (4, counting or
// not).  Every pixel is the same bits through every kernel, so a call whose scene, counters or forced variant would land anywhere else —
// the nested-loop kernel (2), a counting layout of the wave kernel — takes variant 4; the cost-sorted resume launch of a small shard runs
// without work stealing; the fast general kernel runs in its two-waves-per-SIMD form whatever the frame's size.
static void route_moments_variant(RtiowChoice &choice, bool want_stats) {
  const int v = choice.variant;
  if (v == 2 || (want_stats && v != 4)) choice.variant = 4;
}

// Where an ADAPTIVE frame (rl_rtiow_render_adaptive*) goes: where the moments frame goes (the stopping rule is a runtime
// mode of the MOMENTS wave, fast general and reference-order kernels), except that the cooperative one-wave-per-pixel kernel has no such
// mode: its small frames, and a forced 1033, take the fast layout of the wave kernel (every scene of 1033 has it; paths deeper than its
// depth field take the reference-order kernel).  Never work stealing: no moments call steals.
static void route_adaptive_variant(RtiowChoice &choice, const rl_rtiow_camera *cam) {
  if (choice.variant == 1033) choice.variant = cam->max_depth > FAST_DEPTH_MASK ? 4 : 1029;
}

// Variant 1029 only: the per-pixel entry table of this render's camera and rows (rl_pixel_entry.h), built on `stream` ahead of the render
// kernels into the scene's own buffers (grown on demand, like d_pos): the one-word table, and with T = g_sw.pixel_entry_time > 1 slices the
// [pixel][T] table beside it, out of the same walk.  One slice for the whole call where the slices' rounding argument has nothing to stand
// on (a motion value that is not finite), without the sphere test (the slices are a sphere test), and where the sliced table would pass 256 MB.
// The tables depend on the scene and on the key below only — progressive passes, adaptive loops and denoise_render repeat all of it call
// after call — so a call that repeats the key of the last build launches nothing (RL_PIXEL_ENTRY_REUSE=0: every call builds).
std::atomic<unsigned long long> g_pixel_entry_builds{0};  // rl_debug_pixel_entry_builds: table kernels launched by this process
static int build_pixel_entry(const rl_scene *scene, RtiowParams &P, uint32_t nrows, hipStream_t stream) {
  P.pixel_entry = nullptr, P.pixel_entry_t = nullptr, P.pixel_entry_log2t = 0;
  const size_t npix = (size_t)nrows * P.cam.image_width;
  if (g_sw.pixel_entry <= 0 || npix == 0) return RL_OK;
  rl_scene *ms = const_cast<rl_scene *>(scene);  // work buffers only
  uint32_t T = (uint32_t)g_sw.pixel_entry_time;
  if (!g_sw.pixel_entry_sphere || !scene->hrt->fast_motion_finite || npix * T * sizeof(uint32_t) > ((size_t)256 << 20)) T = 1;
  rl_scene::PixelEntryKey key;
  std::memset(&key, 0, sizeof key);  // (padding too: the keys are compared as bytes)
  const rl_rtiow_camera &c = P.cam;
  key.image_width = c.image_width, key.image_height = c.image_height, key.defocus_angle = c.defocus_angle;
  std::memcpy(key.lookfrom, c.lookfrom, sizeof key.lookfrom), std::memcpy(key.pixel_00, c.pixel_00, sizeof key.pixel_00);
  std::memcpy(key.pixel_du, c.pixel_du, sizeof key.pixel_du), std::memcpy(key.pixel_dv, c.pixel_dv, sizeof key.pixel_dv);
  std::memcpy(key.defocus_disk_u, c.defocus_disk_u, sizeof key.defocus_disk_u), std::memcpy(key.defocus_disk_v, c.defocus_disk_v, sizeof key.defocus_disk_v);
  key.row_first = P.row_first, key.row_step = P.row_step, key.nrows = nrows;
  key.max_entries = (uint32_t)g_sw.pixel_entry, key.sphere = g_sw.pixel_entry_sphere ? 1u : 0u, key.slices = T;
  // (a buffer that has to grow is a new allocation: whatever was built is gone with the old one)
  if (ms->d_pixel_entry.size() < npix || (T > 1 && ms->d_pixel_entry_t.size() < npix * T)) ms->entry_key_valid = false;
  HIP_TRY(ms->d_pixel_entry.reserve(npix));
  if (T > 1) HIP_TRY(ms->d_pixel_entry_t.reserve(npix * T));
  HIP_TRY(ms->ev_entry.create(hipEventDisableTiming));
  if (g_sw.pixel_entry_reuse && ms->entry_key_valid && std::memcmp(&key, &ms->entry_key, sizeof key) == 0) {
    if (ms->entry_stream != stream) HIP_TRY(hipStreamWaitEvent(stream, ms->ev_entry, 0));  // built on another stream: behind that build
  } else {
    ms->entry_key_valid = false;
    const dim3 grid((unsigned)((npix + 255) / 256)), block(256);
    const float *boxes = scene->d_fast_leaf_boxes;
    const double *balls = g_sw.pixel_entry_sphere ? (const double *)scene->d_fast_leaf_balls : (const double *)nullptr, *motion = scene->d_fast_leaf_motion;
    const uint32_t me = (uint32_t)g_sw.pixel_entry;
    uint32_t *one = ms->d_pixel_entry, *sliced = T > 1 ? (uint32_t *)ms->d_pixel_entry_t : nullptr;
    if (T == 8) hipLaunchKernelGGL(rtiow_pixel_entry_kernel<9>, grid, block, 0, stream, P, boxes, balls, motion, me, one, sliced);
    else if (T == 4) hipLaunchKernelGGL(rtiow_pixel_entry_kernel<5>, grid, block, 0, stream, P, boxes, balls, motion, me, one, sliced);
    else if (T == 2) hipLaunchKernelGGL(rtiow_pixel_entry_kernel<3>, grid, block, 0, stream, P, boxes, balls, motion, me, one, sliced);
    else hipLaunchKernelGGL(rtiow_pixel_entry_kernel<1>, grid, block, 0, stream, P, boxes, balls, motion, me, one, sliced);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(ms->ev_entry, stream));
    g_pixel_entry_builds++;
    ms->entry_key = key, ms->entry_key_valid = true, ms->entry_stream = stream;
  }
  P.pixel_entry = ms->d_pixel_entry;
  if (T > 1) P.pixel_entry_t = ms->d_pixel_entry_t, P.pixel_entry_log2t = T == 8 ? 3u : T == 4 ? 2u : 1u;
  return RL_OK;
}

// The kernels that take the parameter block by pointer read a device copy of it.  Two slots, used in turn: the cost-sorted render launches
// twice with different parameters (and the sample-parallel mode and the ray queries once per pass), all enqueued before the first one runs.
static int stage_params(const rl_scene *scene, const RtiowParams &P, hipStream_t stream, const RtiowParams *&slot) {
  rl_scene *ms = const_cast<rl_scene *>(scene);  // work buffers only
  HIP_TRY(ms->d_params.reserve(2 * sizeof(RtiowParams)));
  RtiowParams *dst = (RtiowParams *)ms->d_params.get() + (ms->params_slot++ & 1);
  HIP_TRY(hipMemcpyAsync(dst, &P, sizeof(RtiowParams), hipMemcpyHostToDevice, stream));
  slot = dst;
  return RL_OK;
}

#include "rl_rtiow_launch.h"  // kernel tables, fastg_prepare, wave_general_lds, persistent_blocks, launch_persistent, coop_launch

namespace rl {
int rtiow_render_launch(const rl_scene *scene, const rl_rtiow_camera *cam, uint64_t first_sample, uint32_t row_first, uint32_t row_step, void *d_out,
                        hipStream_t stream, bool want_stats, void *d_out_sq, const rl_rtiow_adaptive *rule, void *d_out_count) {
  const RtiowProgram &rt = scene->rt();
  const HostRtiow &H = *scene->hrt;
  uint32_t H_ = cam->image_height, W = cam->image_width;
  uint32_t nrows = row_first < H_ ? (H_ - row_first + row_step - 1) / row_step : 0;
  RtiowParams P;
  uint64_t slots = 0;
  {
    int rcp = fill_rtiow_params(scene, cam, first_sample, row_first, row_step, nrows, d_out, want_stats, P, slots);
    if (rcp != RL_OK) return rcp;
  }
  const bool moments = d_out_sq != nullptr;  // the MOMENTS instantiations: second moments beside the sums, same layout
  P.out_sq = (double *)d_out_sq;
  const bool adaptive = moments && rule && d_out_count;  // the MOMENTS frame kernels' runtime mode: pixels stop by the rule, counts beside the moments
  if (adaptive) P.out_count = (uint32_t *)d_out_count, P.adapt = *rule, P.adapt_total = cam->samples_per_pixel;

  {
    int rco = order_after_previous(scene, stream);
    if (rco != RL_OK) return rco;
  }
  HIP_TRY(hipMemsetAsync(scene->d_scratch, 0, 512, stream));  // [0] work counter, [64..] stats, [256] cooperative kernel's / stealing counter
  if (scene->progress_on) {  // the work counter in host-visible memory (rl_rtiow_render_progress)
    const_cast<rl_scene *>(scene)->progress_total = slots;
    P.work_counter = scene->d_progress;
    HIP_TRY(hipMemsetAsync(scene->d_progress, 0, 8, stream));
  }
  RtiowChoice choice;
  {
    int rcv = choose_rtiow_variant(scene, cam, P, nrows, want_stats, choice);
    if (rcv != RL_OK) return rcv;
  }
  if (moments) route_moments_variant(choice, want_stats);
  if (adaptive) route_adaptive_variant(choice, cam);
  const int variant = choice.variant;
  const size_t compact_bytes = choice.compact_bytes, fast_bytes = choice.fast_bytes;
  if (variant == 1029) {
    int rce = build_pixel_entry(scene, P, nrows, stream);
    if (rce != RL_OK) return rce;
    if (want_stats) {  // the instrumented kernel (verify build, tools/sched.py) repeats the table's tests on the visits it counts as wasted
      CensusTables ct{nullptr, nullptr, nullptr, *cam};
      if (P.pixel_entry) ct = CensusTables{scene->d_fast_leaf_boxes, scene->d_fast_leaf_balls, scene->d_fast_leaf_motion, *cam};
      HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(rl::g_census), &ct, sizeof ct));  // (a tool's path: the blocking copy)
    }
  }
  bool steal = false;  // set for the resume launch of a small shard (variant 1029)
  const Mode mode = moments ? Mode::MOMENTS : Mode::FRAME;
  const bool trans = rt.has_noise || rt.has_sphere_uv;
  auto launch_variant = [&]() -> int {
    if (variant == 2) {
      constexpr int NT = 256;
      // register budget of two waves per SIMD (256 registers instead of 256 + 151): cornell_smoke 309 -> 493 Mrays/s, final_scene 170 -> 219
      // (three waves: 390 / 182).
      const ValueKernel kern = want_stats ? rtiow_general_kernel<NT, true, 512> : rtiow_general_kernel<NT, false, 512>;
      return launch_persistent(kern, NT, (size_t)8 * NT * sizeof(unsigned long long), slots, P, scene, stream);
    }
    if (variant == 1031) {  // rings + the traversal stacks in LDS; a moments frame in the two-waves-per-SIMD form whatever its size
      const bool media = H.fg.stage_roots.size() > 1;
      const bool one_wave = !moments && fastg_one_wave(trans, media, (uint64_t)nrows * W);
      const FastgLayout lay = fastg_prepare(H.fg, trans, media, one_wave, P);
      return launch_persistent(fast_general_kernel(mode, trans, media, one_wave), lay.nt, lay.lds, slots, P, scene, stream);
    }
    if (variant == 4) return launch_persistent(wave_general_kernel(mode, trans, want_stats, rt.has_media), 512, wave_general_lds(rt.has_media), slots, P, scene, stream);
    if (variant == 1033) {  // A/B: EVERY pixel through the cooperative one-wave-per-pixel kernel (rl_rtiow_coop.h)
      rl_scene *ms = const_cast<rl_scene *>(scene);
      const size_t npix = (size_t)nrows * W;
      HIP_TRY(ms->d_coop_pixels.reserve(npix));
      hipLaunchKernelGGL(iota_u32, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, stream, ms->d_coop_pixels, (uint32_t)npix);
      CoopParams C{};
      C.pixels = ms->d_coop_pixels, C.leaf_boxes = scene->d_fast_leaf_boxes, C.counter = (uint32_t *)(scene->d_scratch + 256);
      HIP_TRY(hipMemsetAsync(C.counter, 0, 4, stream));
      return coop_launch(P, C, (uint32_t)npix, moments, false, stream);
    }
    // the wave kernel, 4 waves per SIMD: the rings and, in LDS next to them, the fast traversal nodes (1029; never a counting render) / the
    // compact guarded ops (1027) / the linked ops (1025) / nothing: everything through L2 (1024: sphere-only worlds too large for LDS)
    const int lds_scene = variant == 1029 ? 4 : variant == 1027 ? 3 : variant == 1025 ? 2 : 0;
    const size_t scene_bytes = lds_scene == 4 ? fast_bytes : lds_scene == 3 ? compact_bytes : lds_scene == 2 ? (size_t)P.n_ops * sizeof(DevOp) : 0;
    // leave a TRAV round when fewer than a quarter of the lanes it started with are still walking (the counting kernels: 3/8): with
    // pair nodes and inline misses the walks are short and uneven — +2.1 % (6596 -> 6734 Mrays/s; 24,2: 6740; 24,1: 6586; tools: RL_TUNE)
    if (lds_scene == 4 && !g_sw.tune_set) P.tune[1] = 4, P.tune[2] = 4;
    return launch_persistent(wave_kernel(mode, lds_scene, want_stats, steal), 1024, (size_t)16 * 1024 * sizeof(unsigned long long) + scene_bytes, slots, P, scene, stream);
  };
  P.sample_begin = 0, P.sample_end = cam->samples_per_pixel, P.resume = 0;
  P.pos_state = nullptr, P.tile_order = nullptr, P.tile_cost = nullptr;
  // Cost-sorted two-phase render (wave kernels, spp >= 64): a short first launch renders samples [0, 8) of every
  // pixel and records each 8x8 tile's ray count; the tiles are then sorted by cost and the remaining samples are
  // rendered expensive-tiles-first (LPT), so the tail of the launch holds cheap pixels only.  Pixels are resumed
  // with their exact sums and ChaCha word positions: results are bit-identical to a single launch.
  const bool lpt_enabled = g_sw.lpt;
  const uint32_t lpt_first = 8;  // (round 3: 2 / 4 / 16 probe samples measure 6727 / 6752 / 6710 Mrays/s against 6711 — flat)
  bool lpt = lpt_enabled && (variant >= 256 || variant == 4) && cam->samples_per_pixel >= 64;
  if (want_stats) HIP_TRY(hipEventRecord(scene->ev0, stream));
  int rc = RL_OK;
  if (!lpt) rc = launch_variant();
  else {
    rl_scene *ms = const_cast<rl_scene *>(scene);  // scratch buffers only; the scene program itself is immutable
    size_t npix = (size_t)nrows * W, ntiles = (size_t)(slots >> 6);
    HIP_TRY(ms->d_pos.reserve(npix));
    HIP_TRY(ms->d_tile_cost.reserve(ntiles));
    HIP_TRY(ms->d_tile_order.reserve(ntiles));
    HIP_TRY(ms->d_tile_keys.reserve(ntiles));
    HIP_TRY(ms->d_tile_iota.reserve(ntiles));
    HIP_TRY(hipMemsetAsync(ms->d_tile_cost, 0, ntiles * sizeof(uint32_t), stream));
    P.sample_end = lpt_first, P.pos_state = ms->d_pos, P.tile_cost = ms->d_tile_cost;
    rc = launch_variant();
    if (rc != RL_OK) return rc;
    // tiles by cost, most expensive first, on the device (stable radix sort): the whole render stays asynchronous on `stream`
    rc = rl::sort_tiles_by_cost_desc(ms->d_tile_cost, ms->d_tile_keys, ms->d_tile_iota, ms->d_tile_order, (uint32_t)ntiles, ms->d_sort_temp, stream);
    if (rc != RL_OK) return rc;
    HIP_TRY(hipMemsetAsync(scene->d_scratch, 0, 4, stream));  // work counter only; stats keep accumulating
    if (scene->progress_on) P.work_counter = scene->d_progress + 1;  // the resume launch counts in the second host-visible word
    P.sample_begin = lpt_first, P.sample_end = cam->samples_per_pixel, P.resume = 1;
    P.tile_order = ms->d_tile_order, P.tile_cost = nullptr;
    if (variant == 1029 && !want_stats && !moments && g_sw.steal_max_fill > 0.0 && (double)npix <= g_sw.steal_max_fill * (double)g_cus * 1024.0) {
      // small shard: waves that run out of pixels take over pixels other lanes are still rendering (rl_rtiow_coop.h rtiow_steal_loop)
      HIP_TRY(ms->d_steal_state.reserve(npix));
      HIP_TRY(ms->d_steal_n.reserve(npix));
      HIP_TRY(hipMemsetAsync(ms->d_steal_state, 0, npix * sizeof(uint32_t), stream));
      HIP_TRY(hipMemsetAsync(ms->d_steal_n, 0xFF, npix * sizeof(uint32_t), stream));  // 0xFFFFFFFF: never released (rl_debug_steal_read)
      HIP_TRY(hipMemsetAsync(scene->d_scratch + 256, 0, 4, stream));
      P.steal_state = ms->d_steal_state, P.steal_n = ms->d_steal_n, P.steal_counter = (uint32_t *)(scene->d_scratch + 256);
      P.coop_leaf_boxes = scene->d_fast_leaf_boxes;
      steal = true;
    }
    rc = launch_variant();
  }
  if (want_stats) HIP_TRY(hipEventRecord(scene->ev1, stream));
  return rc;  // the caller ends the render with collect_stats / post_status, which record ev_last behind the stats copy
}

// The sample-parallel mode (include/rl_render.h rl_rtiow_render_independent*).  A work item is (sample group of indep_k samples, pixel),
// every sample from ChaCha word 0 on its own stream; the samples of a PASS write their colours to the scene's pass buffer and
// rtiow_indep_fold adds them to d_out in ascending sample order.  Passes are sized so the buffer stays under g_sw.indep_cap and the
// pass's slots fit the u32 work counter; they are enqueued back to back on `stream`.  The stats words are zeroed once per render.
int rtiow_render_indep_launch(const rl_scene *scene, const rl_rtiow_camera *cam, uint64_t first_sample, uint32_t row_first, uint32_t row_step,
                              bool accumulate, void *d_out, hipStream_t stream, bool want_stats) {
  const RtiowProgram &rt = scene->rt();
  const HostRtiow &H = *scene->hrt;
  const uint32_t H_ = cam->image_height, W = cam->image_width;
  const uint32_t nrows = row_first < H_ ? (H_ - row_first + row_step - 1) / row_step : 0;
  RtiowParams P;
  uint64_t tile_slots = 0;
  {
    int rcp = fill_rtiow_params(scene, cam, first_sample, row_first, row_step, nrows, d_out, want_stats, P, tile_slots);
    if (rcp != RL_OK) return rcp;
  }
  P.pix_rays = nullptr, P.pos_state = nullptr, P.tile_order = nullptr, P.tile_cost = nullptr, P.resume = 0;
  RtiowChoice choice;
  {
    int rcv = choose_rtiow_variant(scene, cam, P, nrows, want_stats, choice);
    if (rcv != RL_OK) return rcv;
  }
  // the fast traversals where the automatic choice takes them (the cooperative kernel's small frames included: here they have
  // pixels x samples of parallelism), and the reference-order wave-scheduled general kernel for everything else (counting renders too)
  int variant = choice.variant;
  if (variant == 1033) variant = 1029;
  if ((variant == 1029 && want_stats) || (variant != 1029 && variant != 1031)) variant = 4;
  const uint32_t S = cam->samples_per_pixel;
  const uint64_t n_vals = (uint64_t)nrows * W * 3u;
  const size_t sample_bytes = (size_t)n_vals * sizeof(double);
  const uint32_t K = g_sw.indep_k ? g_sw.indep_k : 1u;
  // samples per pass: the buffer cap, and the slots (groups x tile slots) below the u32 work counter's end
  uint64_t per_pass = std::max<uint64_t>(1, g_sw.indep_cap / sample_bytes);
  const uint64_t max_groups = std::max<uint64_t>(1, (0xFFFF0000ull - 1) / tile_slots);
  per_pass = std::min<uint64_t>(per_pass, max_groups * K);
  per_pass = std::min<uint64_t>(per_pass, std::max<uint32_t>(S, 1u));
  rl_scene *ms = const_cast<rl_scene *>(scene);  // work buffers only; the scene program is immutable
  {
    int rco = order_after_previous(scene, stream);
    if (rco != RL_OK) return rco;
  }
  if (S > 0) HIP_TRY(ms->d_indep.reserve((size_t)per_pass * (size_t)n_vals));
  P.indep_buf = ms->d_indep, P.indep_k = K, P.indep_tile_slots = (uint32_t)tile_slots;
  if (variant == 1029) {  // the sample-parallel fast kernel shares the body: its camera rays start at their pixel's entry too
    int rce = build_pixel_entry(scene, P, nrows, stream);
    if (rce != RL_OK) return rce;
  }
  HIP_TRY(hipMemsetAsync(scene->d_scratch, 0, 512, stream));  // work counter and stats: once per render
  const bool trans = rt.has_noise || rt.has_sphere_uv;
  ValueKernel kern = nullptr;       // variants 1029 and 4: parameter block by value
  PointerKernel kern_ptr = nullptr;  // variant 1031: by pointer, each pass its own stream-ordered copy
  int nt = 512;
  size_t lds = 0;
  if (variant == 1029) {
    kern = wave_kernel(Mode::INDEP, 4, false, false), nt = 1024, lds = (size_t)16 * 1024 * sizeof(unsigned long long) + choice.fast_bytes;
    if (!g_sw.tune_set) P.tune[1] = 4, P.tune[2] = 4;
  } else if (variant == 1031) {
    const bool media = H.fg.stage_roots.size() > 1, one_wave = fastg_one_wave(trans, media, (uint64_t)nrows * W);
    const FastgLayout lay = fastg_prepare(H.fg, trans, media, one_wave, P);
    kern_ptr = fast_general_kernel(Mode::INDEP, trans, media, one_wave), nt = lay.nt, lds = lay.lds;
  } else {
    kern = wave_general_kernel(Mode::INDEP, trans, want_stats, rt.has_media), lds = wave_general_lds(rt.has_media);
  }
  auto launch_pass = [&]() -> int {
    return kern_ptr ? launch_persistent(kern_ptr, nt, lds, P.n_slots, P, scene, stream) : launch_persistent(kern, nt, lds, P.n_slots, P, scene, stream);
  };
  if (want_stats) HIP_TRY(hipEventRecord(scene->ev0, stream));
  int rc = RL_OK;
  if (S == 0 && !accumulate && n_vals) HIP_TRY(hipMemsetAsync(d_out, 0, sample_bytes, stream));  // no samples: the empty sum
  for (uint64_t b = 0; b < S && rc == RL_OK; b += per_pass) {
    const uint32_t e = (uint32_t)std::min<uint64_t>(S, b + per_pass), np = e - (uint32_t)b;
    P.sample_begin = (uint32_t)b, P.sample_end = e;
    P.n_slots = (uint32_t)((uint64_t)((np + K - 1) / K) * tile_slots);
    if (b != 0) HIP_TRY(hipMemsetAsync(scene->d_scratch, 0, 4, stream));  // work counter only; stats keep accumulating
    rc = launch_pass();
    if (rc != RL_OK) break;
    const uint32_t fb = 256;
    hipLaunchKernelGGL(rtiow_indep_fold, dim3((unsigned)((n_vals + fb - 1) / fb)), dim3(fb), 0, stream, (double *)d_out, (const double *)ms->d_indep, (unsigned long long)n_vals, np,
                       (uint32_t)(b != 0 || accumulate));
    HIP_TRY(hipGetLastError());
  }
  if (want_stats) HIP_TRY(hipEventRecord(scene->ev1, stream));
  return rc;  // the caller ends the render with collect_stats / post_status, which record ev_last behind the stats copy
}
}  // namespace rl

// Which kernel renders a pixel LIST (rl_rtiow_render_pixels*; with second moments, rl_rtiow_render_pixels_moments*, §3.14: all
// three list kernels have the MOMENTS flavour, so a moments list goes where the plain list goes — except that the fast general kernel runs in
// its two-waves-per-SIMD form whatever the list's length).  The list kernels are the cooperative one-wave-per-pixel
// kernel (sphere-only scenes that have the fast structure, counter-free), the fast general kernel (general scenes with a fast tree,
// counter-free) and the reference-order wave-scheduled general kernel (every counting call, and every scene the other two do not take).
// rl_debug_set_fast_traversal(0) / rl_debug_set_coop(0) send the counter-free calls to the reference-order kernel (tests, A/B).
enum PixelsKernel { PIXELS_REFERENCE = 0, PIXELS_FAST_GENERAL = 1, PIXELS_COOP = 2 };
static int choose_rtiow_pixels_kernel(const rl_scene *scene, const rl_rtiow_camera *cam, const RtiowParams &P, uint64_t n, bool want_stats, PixelsKernel &out) {
  RtiowChoice choice;
  int rc = choose_rtiow_variant(scene, cam, P, cam->image_height, want_stats, choice);  // for what fits: the frame's own rules
  if (rc != RL_OK) return rc;
  const HostRtiow &H = *scene->hrt;
  out = PIXELS_REFERENCE;
  if (want_stats) return RL_OK;
  if (choice.general) {
    if (H.fg.ok && g_sw.fast_traversal) out = PIXELS_FAST_GENERAL;
  } else if (choice.fits_fast && cam->max_depth <= FAST_DEPTH_MASK && g_sw.coop_small) {
    // one wave per pixel is a latency kernel: beyond the frame path's bound (160 pixels per CU, choose_rtiow_variant) its throughput is a
    // fraction of a lane-per-pixel kernel's (measured: DESIGN.md §3.13), and the reference-order kernel takes the list
    const uint64_t limit = g_sw.coop_pixels_max ? g_sw.coop_pixels_max : (uint64_t)g_cus * 160u;
    if (n <= limit) out = PIXELS_COOP;
  }
  return RL_OK;
}

namespace rl {
// The launch half of rl_rtiow_render_pixels*: n list elements (d_xs[i], d_ys[i]) of the whole frame -> d_out[i], all on `stream`.
// want_stats: a counting call (reference-order kernel); timed: the caller reads the stats words synchronously (ev0 / ev1 bracket the kernel)
int rtiow_render_pixels_launch(const rl_scene *scene, const rl_rtiow_camera *cam, uint64_t first_sample, const uint32_t *d_xs, const uint32_t *d_ys, uint64_t n,
                               void *d_out, hipStream_t stream, bool want_stats, bool timed, void *d_out_sq) {
  const RtiowProgram &rt = scene->rt();
  const HostRtiow &H = *scene->hrt;
  if (n >= PIXEL_LIST_MAX_N) return set_err(RL_E_INVALID, "image too large");  // the u32 work counter (the entry points have checked already)
  RtiowParams P;
  uint64_t tile_slots = 0;
  {
    int rcp = fill_rtiow_params(scene, cam, first_sample, 0, 1, cam->image_height, d_out, want_stats, P, tile_slots);
    if (rcp != RL_OK) return rcp;
  }
  P.n_slots = (uint32_t)n, P.pix_xs = d_xs, P.pix_ys = d_ys;
  const bool moments = d_out_sq != nullptr;  // the MOMENTS instantiations: second moments beside the sums, compact as they are
  P.out_sq = (double *)d_out_sq;
  P.pix_rays = nullptr, P.pos_state = nullptr, P.tile_order = nullptr, P.tile_cost = nullptr, P.resume = 0;
  P.sample_begin = 0, P.sample_end = cam->samples_per_pixel;
  PixelsKernel which;
  {
    int rcv = choose_rtiow_pixels_kernel(scene, cam, P, n, want_stats, which);
    if (rcv != RL_OK) return rcv;
  }
  {
    int rco = order_after_previous(scene, stream);
    if (rco != RL_OK) return rco;
  }
  HIP_TRY(hipMemsetAsync(scene->d_scratch, 0, 512, stream));  // [0] work counter, [64..] stats, [256] the cooperative kernel's counter
  uint32_t *coop_counter = (uint32_t *)(scene->d_scratch + 256);
  if (scene->progress_on) {  // rl_rtiow_render_progress: the list's elements claimed so far, of n (one launch: phase 0)
    const_cast<rl_scene *>(scene)->progress_total = n;
    P.work_counter = scene->d_progress, coop_counter = scene->d_progress;
    HIP_TRY(hipMemsetAsync(scene->d_progress, 0, 8, stream));
  }
  const Mode mode = moments ? Mode::PIXELS_MOMENTS : Mode::PIXELS;
  const bool trans = rt.has_noise || rt.has_sphere_uv;
  if (timed) HIP_TRY(hipEventRecord(scene->ev0, stream));
  int rc = RL_OK;
  if (which == PIXELS_COOP) {  // one wave per element
    CoopParams C{};
    C.pixels = nullptr, C.leaf_boxes = scene->d_fast_leaf_boxes, C.counter = coop_counter;
    rc = coop_launch(P, C, n, moments, true, stream);
  } else if (which == PIXELS_FAST_GENERAL) {  // a moments list in the two-waves-per-SIMD form whatever its length
    const bool media = H.fg.stage_roots.size() > 1;
    const bool one_wave = !moments && fastg_one_wave(trans, media, n);
    const FastgLayout lay = fastg_prepare(H.fg, trans, media, one_wave, P);
    rc = launch_persistent(fast_general_kernel(mode, trans, media, one_wave), lay.nt, lay.lds, n, P, scene, stream);
  } else {  // reference order
    rc = launch_persistent(wave_general_kernel(mode, trans, want_stats, rt.has_media), 512, wave_general_lds(rt.has_media), n, P, scene, stream);
  }
  if (timed) HIP_TRY(hipEventRecord(scene->ev1, stream));
  return rc;  // the caller ends the render with collect_stats / post_status, which record ev_last behind the stats copy
}
}  // namespace rl

extern "C" {

int rl_rtiow_render_device(const rl_scene *scene, const rl_rtiow_camera *cam, uint64_t first_sample, uint32_t row_first, uint32_t row_step,
                           void *d_out, void *hip_stream, rl_stats *st) {
  bool done;
  int rc = render_check(scene, 1, frame_of(cam), d_out && row_step != 0, row_first, "empty image", st, done);
  if (done) return rc;
  hipStream_t stream = (hipStream_t)hip_stream;
  return render_run(scene, stream, st, [&] { return rl::rtiow_render_launch(scene, cam, first_sample, row_first, row_step, d_out, stream, st != nullptr); });
}

int rl_rtiow_render_independent_device(const rl_scene *scene, const rl_rtiow_camera *cam, uint64_t first_sample, uint32_t row_first, uint32_t row_step,
                                       uint32_t accumulate, void *d_out, void *hip_stream, rl_stats *st) {
  bool done;
  int rc = render_check(scene, 1, frame_of(cam), d_out && row_step != 0, row_first, "empty image", st, done);
  if (done) return rc;
  hipStream_t stream = (hipStream_t)hip_stream;
  return render_run(scene, stream, st,
                    [&] { return rl::rtiow_render_indep_launch(scene, cam, first_sample, row_first, row_step, accumulate != 0, d_out, stream, st != nullptr); });
}

// Pixel-list renders (include/rl_render.h "Pixel-list renders").  counting: the caller gave opt_stats (reference-order
// kernel, all seven counters); sync_st: filled synchronously (the host form always; rays and flagged only when !counting); null: asynchronous.
// d_out_sq: the moments forms' second buffer; null: a plain list render.
static int rtiow_render_pixels_impl(const rl_scene *scene, const rl_rtiow_camera *cam, uint64_t first_sample, const void *d_xs, const void *d_ys, uint64_t n,
                                    void *d_out, hipStream_t stream, bool counting, rl_stats *sync_st, void *d_out_sq = nullptr) {
  return render_run(scene, stream, sync_st, [&] {
    return rl::rtiow_render_pixels_launch(scene, cam, first_sample, (const uint32_t *)d_xs, (const uint32_t *)d_ys, n, d_out, stream, counting, sync_st != nullptr,
                                          d_out_sq);
  });
}

int rl_rtiow_render_pixels_device(const rl_scene *scene, const rl_rtiow_camera *cam, uint64_t first_sample, const void *d_xs, const void *d_ys, uint64_t n,
                                  void *d_out, void *hip_stream, rl_stats *st) {
  bool done;
  int rc = render_check(scene, 1, frame_of(cam), n == 0 || (d_xs && d_ys && d_out), 0, "empty image", st, done);
  if (done) return rc;
  rc = list_length_check(n, st, done);
  if (done) return rc;
  return rtiow_render_pixels_impl(scene, cam, first_sample, d_xs, d_ys, n, d_out, (hipStream_t)hip_stream, st != nullptr, st);
}

// Renders with second moments (include/rl_render.h "Second moments"): the plain calls' checks, run and status, with the
// second buffer handed to the launch, which then takes the MOMENTS instantiations.
int rl_rtiow_render_moments_device(const rl_scene *scene, const rl_rtiow_camera *cam, uint64_t first_sample, uint32_t row_first, uint32_t row_step,
                                   void *d_out, void *d_out_sq, void *hip_stream, rl_stats *st) {
  bool done;
  int rc = render_check(scene, 1, frame_of(cam), d_out && d_out_sq && row_step != 0, row_first, "empty image", st, done);
  if (done) return rc;
  hipStream_t stream = (hipStream_t)hip_stream;
  return render_run(scene, stream, st, [&] { return rl::rtiow_render_launch(scene, cam, first_sample, row_first, row_step, d_out, stream, st != nullptr, d_out_sq); });
}

// Adaptive renders (include/rl_render.h "Adaptive renders"): the moments call with a stopping rule and a third buffer, the
// per-pixel sample counts.  What the rule itself can be wrong by is refused first, device or not.
static bool adaptive_rule_ok(const rl_rtiow_adaptive *rule) {
  return rule && rule->min_samples >= 2 && rule->check_every >= 1 && rule->abs_variance >= 0.0 && rule->rel_variance >= 0.0;  // (a NaN bound compares false)
}
int rl_rtiow_render_adaptive_device(const rl_scene *scene, const rl_rtiow_camera *cam, uint64_t first_sample, uint32_t row_first, uint32_t row_step,
                                    const rl_rtiow_adaptive *rule, void *d_out, void *d_out_sq, void *d_out_count, void *hip_stream, rl_stats *st) {
  if (!adaptive_rule_ok(rule) || !d_out || !d_out_sq || !d_out_count) return set_err(RL_E_INVALID, "bad argument");
  bool done;
  int rc = render_check(scene, 1, frame_of(cam), row_step != 0, row_first, "empty image", st, done);
  if (done) return rc;
  hipStream_t stream = (hipStream_t)hip_stream;
  return render_run(scene, stream, st, [&] {
    return rl::rtiow_render_launch(scene, cam, first_sample, row_first, row_step, d_out, stream, st != nullptr, d_out_sq, rule, d_out_count);
  });
}

int rl_rtiow_render_pixels_moments_device(const rl_scene *scene, const rl_rtiow_camera *cam, uint64_t first_sample, const void *d_xs, const void *d_ys, uint64_t n,
                                          void *d_out, void *d_out_sq, void *hip_stream, rl_stats *st) {
  bool done;
  int rc = render_check(scene, 1, frame_of(cam), d_out_sq && (n == 0 || (d_xs && d_ys && d_out)), 0, "empty image", st, done);
  if (done) return rc;
  rc = list_length_check(n, st, done);
  if (done) return rc;
  return rtiow_render_pixels_impl(scene, cam, first_sample, d_xs, d_ys, n, d_out, (hipStream_t)hip_stream, st != nullptr, st, d_out_sq);
}

// Completion + status of the last ASYNCHRONOUS render of this scene (rl_*_render_device / rl_*_render_multi_device with
// opt_stats == NULL): waits for it, fills rays and flagged (the other counters need a counting render) and returns
// RL_E_DEGENERATE when a reference panic site was reached.  RL_OK with zero counters when nothing is pending.
int rl_render_status(const rl_scene *scene, rl_stats *st) {
  if (!g_ready) return set_err(RL_E_NO_DEVICE, "rl_init has not succeeded");
  if (!scene) return set_err(RL_E_INVALID, "bad argument");
  rl_stats acc;
  std::memset(&acc, 0, sizeof acc);
  g_last_slow_traces = 0;
  size_t n = scene->replicas.empty() ? 1 : scene->replicas.size();
  for (size_t g = 0; g < n; g++) {
    rl_scene *r = const_cast<rl_scene *>(scene->replicas.empty() ? scene : scene->replicas[g]);
    std::lock_guard<std::mutex> lk(r->mu);
    bool any = false;
    for (int k = 0; k < rl_scene::N_STATUS; k++) any |= r->status_pending[k];
    if (any) {
      DevCtx *c;
      int rc = scene_context(r, c);
      if (rc != RL_OK) return rc;
      for (int k = 0; k < rl_scene::N_STATUS; k++)
        if (r->status_pending[k]) {
          HIP_TRY(hipEventSynchronize(r->ev_status[k]));
          rl::fold_status(r, k);
        }
    }
    // rays: of the most recently enqueued render of this replica (summed over the replicas of a multi-GPU scene); flagged: every render since the last call
    acc.rays += r->folded_rays, acc.flagged += r->folded_flagged;
    g_last_slow_traces += r->folded_slow;
    r->folded_rays = r->folded_flagged = r->folded_slow = 0, r->folded_seq = r->next_seq;
  }
  if (n > 1) rl::use_context(0);
  if (st) *st = acc;
  if (acc.flagged) return set_err(RL_E_DEGENERATE, "a reference panic site was reached (see stats.flagged)");
  return RL_OK;
}

int rl_rtiow_render_progress(const rl_scene *scene, uint64_t *pixels_claimed, uint64_t *pixels_total, uint32_t *phase) {
  if (!g_ready) return set_err(RL_E_NO_DEVICE, "rl_init has not succeeded");
  if (!scene || scene->kind != 1) return set_err(RL_E_INVALID, "bad argument");
  if (!scene->replicas.empty()) return set_err(RL_E_UNSUPPORTED, "rl_rtiow_render_progress does not follow multi-GPU renders (scene created under rl_init_multi)");
  rl_scene *ms = const_cast<rl_scene *>(scene);
  unsigned long long total = 0, c0 = 0, c1 = 0;
  {
    std::lock_guard<std::mutex> lk(ms->mu);
    if (!ms->progress_on) {  // first call: renders enqueued from now on count in host-visible memory
      DevCtx *c;
      int rc = scene_context(ms, c);
      if (rc != RL_OK) return rc;
      HIP_TRY(ms->h_progress.reserve(16, hipHostMallocMapped | hipHostMallocCoherent));
      std::memset(ms->h_progress, 0, 64);
      HIP_TRY(hipHostGetDevicePointer((void **)&ms->d_progress, ms->h_progress, 0));
      ms->progress_on = true;
    }
    total = ms->progress_total;
    c0 = __atomic_load_n(&ms->h_progress[0], __ATOMIC_RELAXED), c1 = __atomic_load_n(&ms->h_progress[1], __ATOMIC_RELAXED);
  }
  // lanes that find the queue empty still bump the counter: clamp; the resume launch has started once its counter moves
  const unsigned ph = c1 != 0 ? 1u : 0u;
  unsigned long long claimed = ph ? c1 : c0;
  if (claimed > total) claimed = total;
  if (pixels_claimed) *pixels_claimed = claimed;
  if (pixels_total) *pixels_total = total;
  if (phase) *phase = ph;
  return RL_OK;
}

// Not part of the ABI (tests / tools only).  Host-only self-check of the traversal structures a scene compiles to (no device needed:
// tests/test_host_structures.py runs it in the CPU tier): the 16 words of host_structures_report (rl_scene_host.h).  Returns RL_OK or
// the compile error.
int rl_debug_host_structures(const rl_rtiow_scene_desc *desc, unsigned long long *out16) {
  if (!desc || !out16) return set_err(RL_E_INVALID, "bad argument");
  std::shared_ptr<const HostRtiow> H;
  std::string err;
  int rc = build_host_rtiow(desc, H, err);
  if (rc != RL_OK) return set_err(rc, err);
  host_structures_report(desc, *H, out16);
  return RL_OK;
}
// Not part of the ABI (tests only).  Host-only: the RTC program a scene description compiles to, as the kernels read it — the DevOp, DevTri and
// RtcGuard records (build_host_rtc), the first cap[0], cap[1], cap[2] of them copied where the pointer is not null — and counts[4] = n_ops,
// n_tris, n_guards, HostRtc::scene_bytes (what rtc_render_launch compares with the LDS limit).  Returns RL_OK or the compile error.
int rl_debug_rtc_program(const rl_rtc_scene_desc *desc, void *ops, void *tris, void *guards, const uint64_t cap[3], uint64_t counts[4]) {
  if (!desc || !counts || ((ops || tris || guards) && !cap)) return set_err(RL_E_INVALID, "bad argument");
  std::shared_ptr<const HostRtc> H;
  std::string err;
  int rc = build_host_rtc(*desc, H, err);
  if (rc != RL_OK) return set_err(rc, err);
  counts[0] = H->rc.ops.size(), counts[1] = H->rc.tris.size(), counts[2] = H->guards.size(), counts[3] = H->scene_bytes();
  if (ops) std::memcpy(ops, H->rc.ops.data(), (size_t)std::min<uint64_t>(cap[0], counts[0]) * sizeof(DevOp));
  if (tris) std::memcpy(tris, H->rc.tris.data(), (size_t)std::min<uint64_t>(cap[1], counts[1]) * sizeof(DevTri));
  if (guards) std::memcpy(guards, H->guards.data(), (size_t)std::min<uint64_t>(cap[2], counts[2]) * sizeof(RtcGuard));
  return RL_OK;
}
// Tests: out[4] = which kernel the most recent rtc_render_launch of this process took (0 none yet, 1 rtc_kernel / rtc_pixels_kernel, 2 the
// full kernel), 1 for the list flavour, the launch's dynamic LDS bytes (0: the scene is read from global memory), its workgroups.
void rl_debug_last_rtc_launch(uint64_t out[4]) {
  if (out) out[0] = g_last_rtc_kernel.load(), out[1] = g_last_rtc_list.load(), out[2] = g_last_rtc_lds.load(), out[3] = g_last_rtc_blocks.load();
}
// Tests: the RTIOW launch log (rl_rtiow_launch.h).  The number of launches the three funnels have made in this process ...
unsigned long long rl_debug_rtiow_launch_total(void) {
  std::lock_guard<std::mutex> lk(g_launch_log_mu);
  return g_launch_total;
}
// ... and the newest min(cap, 64, total) of their records (RtiowLaunchRecord, 272 bytes each), oldest of them first.  Returns their number.
int rl_debug_rtiow_launch_log(void *out, uint32_t cap) {
  if (!out) return 0;
  std::lock_guard<std::mutex> lk(g_launch_log_mu);
  const uint64_t n = std::min<uint64_t>(std::min<uint64_t>(cap, RTIOW_LAUNCH_LOG), g_launch_total);
  for (uint64_t i = 0; i < n; i++) ((RtiowLaunchRecord *)out)[i] = g_launch_log[(g_launch_total - n + i) % RTIOW_LAUNCH_LOG];
  return (int)n;
}
// Tests: the hand-over record of the scene's most recent stealing launch (rtiow_render_launch: the resume launch of a small shard), after
// everything enqueued has finished: steal_state (3 = the pixel finished) and steal_n (the sample at which a lane last offered the pixel to
// a wave that asked for it; 0xFFFFFFFF: never) of its first n_pixels pixels.
int rl_debug_steal_read(const rl_scene *scene, uint32_t *state_out, uint32_t *n_out, uint64_t n_pixels) {
  if (!scene || !state_out || !n_out || !scene->d_steal_state || !scene->d_steal_n || n_pixels > scene->d_steal_state.size() || n_pixels > scene->d_steal_n.size())
    return RL_E_INVALID;
  DevCtx *c;
  int rc0 = scene_context(scene, c);
  if (rc0 != RL_OK) return rc0;
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(state_out, scene->d_steal_state, n_pixels * sizeof(uint32_t), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(n_out, scene->d_steal_n, n_pixels * sizeof(uint32_t), hipMemcpyDeviceToHost));
  return RL_OK;
}
// force an RTIOW kernel variant (0 auto, 1 nested-loop, 2 general, 512/768/1024 wave)
void rl_debug_set_rtiow_variant(int v) { g_sw.rtiow_variant = v; }
void rl_debug_set_lpt(int on) { g_sw.lpt = on != 0; }
void rl_debug_set_coop(int on) { g_sw.coop_small = on != 0; }
void rl_debug_set_coop_pixels_max(unsigned long long n) { g_sw.coop_pixels_max = n; }  // longest pixel list through the cooperative kernel (0: default; tests, A/B)
void rl_debug_set_steal(double max_fill) { g_sw.steal_max_fill = max_fill; }
void rl_debug_set_fast_traversal(int on) { g_sw.fast_traversal = on != 0; }
void rl_debug_set_rtc_blocks(int per_cu) { g_sw.rtc_blocks_per_cu = per_cu < 0 ? 0 : per_cu; }  // 0: as many as are resident (default); n: n per CU (tests)
void rl_debug_set_indep_cap(unsigned long long bytes) { g_sw.indep_cap = bytes ? (size_t)bytes : (size_t)1 << 30; }  // sample-parallel pass buffer cap (0: default 1 GiB)
void rl_debug_set_indep_k(unsigned k) { g_sw.indep_k = k ? k : 1u; }  // samples of one pixel per claim in the sample-parallel mode
void rl_debug_set_pixel_entry(int max_entries) { g_sw.pixel_entry = std::min(3, std::max(0, max_entries)); }  // 0: camera rays start at the root (A/B, tests)
void rl_debug_set_pixel_entry_sphere(int on) { g_sw.pixel_entry_sphere = on != 0; }  // 0: the box-only cut (A/B, tests)
void rl_debug_set_pixel_entry_time(int slices) { g_sw.pixel_entry_time = rl::pixel_entry_slices(slices); }  // 1, 2, 4 or 8 (anything else: the default); 1: one word per pixel
void rl_debug_set_pixel_entry_reuse(int on) { g_sw.pixel_entry_reuse = on != 0; }  // 0: every call builds its table
// Tests: how many table kernels this process has launched (the launch log lists the render kernels only); a call that reuses the table adds none
unsigned long long rl_debug_pixel_entry_builds(void) { return g_pixel_entry_builds.load(); }
// Tests: the sliced table of the scene's most recent fast-traversal render, n_pixels * slices words as [pixel][slice]; returns RL_E_INVALID when that render had one slice
int rl_debug_pixel_entry_time_read(const rl_scene *scene, uint32_t *out, uint64_t n_pixels, uint32_t slices) {
  if (!scene || !out || !scene->d_pixel_entry_t || !scene->entry_key_valid || scene->entry_key.slices != slices || slices < 2 ||
      n_pixels * slices > scene->d_pixel_entry_t.size())
    return RL_E_INVALID;
  DevCtx *c;
  int rc0 = scene_context(scene, c);
  if (rc0 != RL_OK) return rc0;
  HIP_TRY(hipMemcpy(out, scene->d_pixel_entry_t, n_pixels * slices * sizeof(uint32_t), hipMemcpyDeviceToHost));
  return RL_OK;
}
// Tools (tools/sched.py): the census of the instrumented fast kernel's last launch, 6 x u64: camera LEAF visits that ended at disc < 0 on a moving
// sphere; those of them / of the ones on stationary spheres whose leaf the all-times table holds for the pixel; of the moving ones the table
// holds, those the ball of the sample's time slice leaves out, for 2, 4 and 8 slices
int rl_debug_pixel_entry_census(const rl_scene *scene, unsigned long long *out6) {
  if (!scene || !out6) return RL_E_INVALID;
  HIP_TRY(hipMemcpy(out6, scene->d_scratch + 128 + 31 * 8, 6 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  return RL_OK;
}
// Tests: the entry table of the scene's most recent fast-traversal render (n_pixels words, rows x W of the shard rendered), after that render has finished
int rl_debug_pixel_entry_read(const rl_scene *scene, uint32_t *out, uint64_t n_pixels) {
  if (!scene || !out || !scene->d_pixel_entry || n_pixels > scene->d_pixel_entry.size()) return RL_E_INVALID;
  DevCtx *c;
  int rc0 = scene_context(scene, c);
  if (rc0 != RL_OK) return rc0;
  HIP_TRY(hipMemcpy(out, scene->d_pixel_entry, n_pixels * sizeof(uint32_t), hipMemcpyDeviceToHost));
  return RL_OK;
}
// Tests: the fast tree's shape — children[2 i], children[2 i + 1] = the entry ids of inner node i's children, for the first `cap` nodes; *root = the
// entry a root walk starts at.  Returns the number of inner nodes, -1 when the scene has no fast structure.
int rl_debug_fast_tree(const rl_scene *scene, uint32_t *children, uint32_t cap, uint32_t *root) {
  if (!scene || scene->kind != 1 || !scene->hrt || scene->hrt->fast_root == FAST_NONE) return -1;
  const HostRtiow &H = *scene->hrt;
  if (root) *root = H.fast_root;
  for (uint32_t i = 0; children && i < cap && i < H.fast_nodes.size(); i++) children[2 * i] = H.fast_nodes[i].child & 0xFFFFu, children[2 * i + 1] = H.fast_nodes[i].child >> 16;
  return (int)H.fast_nodes.size();
}
void rl_debug_set_fastg_one_wave(int mode) { g_sw.fastg_nt256 = mode; }  // -1: by frame size (default), 0 / 1: never / always the one-wave-per-SIMD form (tests)
// Tests only: widen the windows in which concurrent renders of one scene could lose a panic-site count.  device_us: a one-lane wait
// kernel on the render's stream just before its status copy; host_us: a host sleep between a multi-GPU frame and its status post.
// Each is capped at 20 ms; 0 / 0 (the default) adds nothing to the render path.
int rl_debug_set_status_gap(unsigned device_us, unsigned host_us) {
  if (!g_ready) return set_err(RL_E_NO_DEVICE, "rl_init has not succeeded");
  g_status_gap_dev_us = std::min(device_us, 20000u), g_status_gap_host_us = std::min(host_us, 20000u);
  return RL_OK;
}
void rl_debug_fast_stats(int on) { g_fast_debug_stats = FAST_STATS_KERNEL && on != 0; }
#ifdef RL_FASTG_VERIFY
int rl_debug_fastg_verify(unsigned int *count, double *log768) {
  HIP_TRY(hipMemcpyFromSymbol(count, HIP_SYMBOL(rl::g_vcount), 4));
  HIP_TRY(hipMemcpyFromSymbol(log768, HIP_SYMBOL(rl::g_vlog), 64 * 12 * 8));
  return RL_OK;
}
int rl_debug_fastg_counts(unsigned long long *out4) {
  HIP_TRY(hipMemcpyFromSymbol(out4, HIP_SYMBOL(rl::g_vstats), 32));
  return RL_OK;
}
#endif
// rays of the render rl_render_status last waited for that the fast traversal re-traced in the reference's order
unsigned long long rl_debug_slow_traces(void) { return g_last_slow_traces; }

// Not part of the ABI (tests): the device allocations the library owns right now, out[0] their number, out[1] their bytes (rl_devbuf.h)
void rl_debug_live_buffers(unsigned long long out[2]) { out[0] = rl::g_live_buffers.load(), out[1] = rl::g_live_bytes.load(); }

// Not part of the ABI (tools only): scheduler occupancy counters of the last STATS launch, 32 x u64 ([3s .. 3s+2] per state; [24]: the
// fast kernel's skipped self tests, rl_rtiow_wave.h fast_self_miss; [25 .. 28]: the camera rays' TRAV lane-steps, LEAF visits, number, and
// LEAF visits that ended at disc < 0; [29]: the scheduling decisions that chose TRAV — [3] counts its steps; [31]: those of [28] on a moving
// sphere, the first word of rl_debug_pixel_entry_census).
int rl_debug_sched(const rl_scene *scene, unsigned long long *out32) {
  if (!scene || !out32) return RL_E_INVALID;
  HIP_TRY(hipMemcpy(out32, scene->d_scratch + 128, 32 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  return RL_OK;
}

// Not part of the ABI (tools only): per-pixel ray counts of the NEXT counting renders of this scene, n_pixels u32 (rows x W of
// the shard rendered); rl_debug_pixel_rays_read copies them back.  Pass 0 to switch the recording off.
int rl_debug_pixel_rays(const rl_scene *scene, uint64_t n_pixels) {
  if (!scene) return RL_E_INVALID;
  rl_scene *ms = const_cast<rl_scene *>(scene);
  ms->d_pix_rays.release();
  if (n_pixels) {
    HIP_TRY(ms->d_pix_rays.reserve(n_pixels));
    HIP_TRY(hipMemset(ms->d_pix_rays, 0, n_pixels * sizeof(uint32_t)));
  }
  return RL_OK;
}
int rl_debug_pixel_rays_read(const rl_scene *scene, uint32_t *out, uint64_t n_pixels) {
  if (!scene || !scene->d_pix_rays || !out) return RL_E_INVALID;
  HIP_TRY(hipMemcpy(out, scene->d_pix_rays, n_pixels * sizeof(uint32_t), hipMemcpyDeviceToHost));
  return RL_OK;
}

int rl_rtiow_render_rows(const rl_scene *scene, const rl_rtiow_camera *cam, uint64_t first_sample, uint32_t row_first, uint32_t row_step,
                         double *out, rl_stats *st) {
  bool done;
  int rc = render_check(scene, 1, frame_of(cam), out && row_step != 0, row_first, nullptr, st, done);
  if (done) return rc;
  HostStaging q(scene);
  void *d_out = q.out(out, frame_of(cam).rows_bytes(row_first, row_step));
  if (q.rc != RL_OK) return q.rc;
  rl_stats local;
  return q.finish(rl_rtiow_render_device(scene, cam, first_sample, row_first, row_step, d_out, q.stream, &local), st, local);
}

int rl_rtiow_render_independent_rows(const rl_scene *scene, const rl_rtiow_camera *cam, uint64_t first_sample, uint32_t row_first, uint32_t row_step,
                                     uint32_t accumulate, double *out, rl_stats *st) {
  bool done;
  int rc = render_check(scene, 1, frame_of(cam), out && row_step != 0, row_first, nullptr, st, done);
  if (done) return rc;
  HostStaging q(scene);
  const size_t bytes = frame_of(cam).rows_bytes(row_first, row_step);
  void *d_out = accumulate ? q.inout(out, bytes) : q.out(out, bytes);  // accumulate: the caller's sums are the fold's start
  if (q.rc != RL_OK) return q.rc;
  rl_stats local;
  return q.finish(rl_rtiow_render_independent_device(scene, cam, first_sample, row_first, row_step, accumulate, d_out, q.stream, &local), st, local);
}

int rl_rtiow_render_pixels(const rl_scene *scene, const rl_rtiow_camera *cam, uint64_t first_sample, const uint32_t *xs, const uint32_t *ys, uint64_t n,
                           double *out, rl_stats *st) {
  bool done;
  int rc = render_check(scene, 1, frame_of(cam), n == 0 || (xs && ys && out), 0, "empty image", st, done);
  if (done) return rc;
  rc = list_length_check(n, st, done);
  if (done) return rc;
  if ((rc = pixel_list_check(frame_of(cam), xs, ys, n)) != RL_OK) return rc;
  HostStaging q(scene);
  const unsigned char *d_xy = (const unsigned char *)q.in({{xs, (size_t)n * sizeof(uint32_t)}, {ys, (size_t)n * sizeof(uint32_t)}});
  void *d_out = q.out(out, (size_t)n * 3 * sizeof(double));
  if (q.rc != RL_OK) return q.rc;
  rl_stats local;
  return q.finish(rtiow_render_pixels_impl(scene, cam, first_sample, d_xy, d_xy + (size_t)n * sizeof(uint32_t), n, d_out, q.stream, st != nullptr, &local), st, local);
}

int rl_rtiow_render_moments_rows(const rl_scene *scene, const rl_rtiow_camera *cam, uint64_t first_sample, uint32_t row_first, uint32_t row_step, double *out,
                                 double *out_sq, rl_stats *st) {
  bool done;
  int rc = render_check(scene, 1, frame_of(cam), out && out_sq && row_step != 0, row_first, nullptr, st, done);
  if (done) return rc;
  HostStaging q(scene);
  const size_t bytes = frame_of(cam).rows_bytes(row_first, row_step);
  void *d_out = q.out(out, bytes), *d_out_sq = q.out(out_sq, bytes);
  if (q.rc != RL_OK) return q.rc;
  rl_stats local;
  return q.finish(rl_rtiow_render_moments_device(scene, cam, first_sample, row_first, row_step, d_out, d_out_sq, q.stream, &local), st, local);
}

int rl_rtiow_render_adaptive_rows(const rl_scene *scene, const rl_rtiow_camera *cam, uint64_t first_sample, uint32_t row_first, uint32_t row_step,
                                  const rl_rtiow_adaptive *rule, double *out, double *out_sq, uint32_t *out_count, rl_stats *st) {
  if (!adaptive_rule_ok(rule) || !out || !out_sq || !out_count) return set_err(RL_E_INVALID, "bad argument");
  bool done;
  int rc = render_check(scene, 1, frame_of(cam), row_step != 0, row_first, nullptr, st, done);
  if (done) return rc;
  HostStaging q(scene);
  const size_t bytes = frame_of(cam).rows_bytes(row_first, row_step);
  void *d_out = q.out(out, bytes), *d_out_sq = q.out(out_sq, bytes), *d_out_count = q.out(out_count, bytes / (3 * sizeof(double)) * sizeof(uint32_t));
  if (q.rc != RL_OK) return q.rc;
  rl_stats local;
  return q.finish(rl_rtiow_render_adaptive_device(scene, cam, first_sample, row_first, row_step, rule, d_out, d_out_sq, d_out_count, q.stream, &local), st, local);
}

int rl_rtiow_render_pixels_moments(const rl_scene *scene, const rl_rtiow_camera *cam, uint64_t first_sample, const uint32_t *xs, const uint32_t *ys, uint64_t n,
                                   double *out, double *out_sq, rl_stats *st) {
  bool done;
  int rc = render_check(scene, 1, frame_of(cam), out_sq && (n == 0 || (xs && ys && out)), 0, "empty image", st, done);
  if (done) return rc;
  rc = list_length_check(n, st, done);
  if (done) return rc;
  if ((rc = pixel_list_check(frame_of(cam), xs, ys, n)) != RL_OK) return rc;
  HostStaging q(scene);
  const unsigned char *d_xy = (const unsigned char *)q.in({{xs, (size_t)n * sizeof(uint32_t)}, {ys, (size_t)n * sizeof(uint32_t)}});
  void *d_out = q.out(out, (size_t)n * 3 * sizeof(double)), *d_out_sq = q.out(out_sq, (size_t)n * 3 * sizeof(double));
  if (q.rc != RL_OK) return q.rc;
  rl_stats local;
  return q.finish(rtiow_render_pixels_impl(scene, cam, first_sample, d_xy, d_xy + (size_t)n * sizeof(uint32_t), n, d_out, q.stream, st != nullptr, &local, d_out_sq), st,
                  local);
}

int rl_rtiow_encode_rgb8_device(const void *d_rgb_sum, uint64_t n_pixels, uint32_t samples, void *d_rgb8, void *hip_stream) {
  if (!g_ready) return set_err(RL_E_NO_DEVICE, "rl_init has not succeeded");
  if (!d_rgb_sum || !d_rgb8 || samples == 0) return set_err(RL_E_INVALID, "bad argument");
  unsigned long long n = n_pixels * 3ull;
  if (n == 0) return RL_OK;
  hipLaunchKernelGGL(encode_rtiow_rgb8, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)hip_stream, (const double *)d_rgb_sum, n,
                     1.0 / (double)samples, (unsigned char *)d_rgb8);
  HIP_TRY(hipGetLastError());
  return RL_OK;
}

int rl_rtiow_render_rgb8(const rl_scene *scene, const rl_rtiow_camera *cam, uint64_t first_sample, uint8_t *out, rl_stats *st) {
  bool done;
  int rc = render_check(scene, 1, frame_of(cam), out != nullptr, 0, "empty image / zero samples", st, done);
  if (done) return rc;
  if (cam->samples_per_pixel == 0) return set_err(RL_E_INVALID, "empty image / zero samples");
  const size_t npix = (size_t)cam->image_width * cam->image_height;
  return render_rgb8(
      scene, npix, out, st, [&](void *d_sum, hipStream_t stream, rl_stats *local) { return rl_rtiow_render_device(scene, cam, first_sample, 0, 1, d_sum, stream, local); },
      [&](void *d_sum, void *d_u8, hipStream_t stream) { return rl_rtiow_encode_rgb8_device(d_sum, npix, cam->samples_per_pixel, d_u8, stream); });
}

int rl_rtiow_render(const rl_scene *scene, const rl_rtiow_camera *cam, uint64_t first_sample, double *out, rl_stats *st) {
  return rl_rtiow_render_rows(scene, cam, first_sample, 0, 1, out, st);
}

// ------------------------------------------------------------------ RTC
static rl_scene *upload_rtc(const std::shared_ptr<const HostRtc> &H, int ctx) {
  rl_scene *s = new rl_scene();
  s->kind = 2, s->ctx = ctx, s->device = g_ctx[(size_t)ctx].device, s->hrc = H;
  const RtcProgram &rc_ = H->rc;
  int rc = RL_OK;
  if ((!H->guards.empty() && (rc = s->d_guards.upload(H->guards))) || (rc = s->d_ops.upload(rc_.ops)) || (rc = s->d_tris.upload(rc_.tris)) ||
      (rc = s->d_xforms.upload(rc_.xforms)) || (rc = s->d_rmaterials.upload(rc_.materials)) || (rc = s->d_lights.upload(rc_.lights)) ||
      (rc = s->d_shapes.upload(rc_.shapes)) || (rc = s->d_csgs.upload(rc_.csgs)) || (rc = s->d_patterns.upload(rc_.patterns)) || (rc = scene_common(s))) {
    destroy_one(s);
    return nullptr;
  }
  return s;
}

rl_scene *rl_rtc_scene_create(const rl_rtc_scene_desc *desc) {
  if (!g_ready) {
    set_err(RL_E_NO_DEVICE, "rl_init has not succeeded (no GPU, or not called)");
    return nullptr;
  }
  if (!desc) {
    set_err(RL_E_INVALID, "null scene descriptor");
    return nullptr;
  }
  std::shared_ptr<const HostRtc> H;
  std::string err;
  if (int rc = build_host_rtc(*desc, H, err)) {
    set_err(rc, err);
    return nullptr;
  }
  return create_replicas([&](int g) { return upload_rtc(H, g); });
}

}  // extern "C"

namespace rl {
// d_xs != null: the list flavour (rtc_render_pixels_launch) — n elements (d_xs[i], d_ys[i]) of the whole frame instead of the shard's pixels
int rtc_render_launch(const rl_scene *scene, const rl_rtc_camera *cam, uint32_t aa, uint32_t row_first, uint32_t row_step, void *d_out, hipStream_t stream,
                      bool want_stats, const uint32_t *d_xs, const uint32_t *d_ys, uint64_t n_list) {
  const RtcProgram &rc_ = scene->rc();
  const bool list = d_xs != nullptr;
  if (list && n_list >= PIXEL_LIST_MAX_N) return set_err(RL_E_INVALID, "image too large");  // the RTIOW list renders' bound (the entry points have checked already)
  uint32_t H = cam->vsize, W = cam->hsize;
  uint32_t nrows = row_first < H ? (H - row_first + row_step - 1) / row_step : 0;
  const uint32_t n_guards = (uint32_t)scene->hrc->guards.size();
  RtcParams P{};
  P.ops = scene->d_ops, P.tris = scene->d_tris, P.xforms = scene->d_xforms, P.materials = scene->d_rmaterials, P.lights = scene->d_lights;
  P.n_ops = (uint32_t)rc_.ops.size(), P.n_tris = (uint32_t)rc_.tris.size();
  P.guards = n_guards ? scene->d_guards : nullptr, P.n_guards = n_guards;
  P.n_xforms = (uint32_t)rc_.xforms.size(), P.n_lights = (uint32_t)rc_.lights.size();
  P.cam = *cam;
  P.aa = aa;
  P.row_first = row_first, P.row_step = row_step, P.nrows = nrows;
  std::memcpy(P.void_color, rc_.void_color, 24);
  P.out = (double *)d_out;
  P.stats = (unsigned long long *)(scene->d_scratch + 64);
  {
    int rco = order_after_previous(scene, stream);
    if (rco != RL_OK) return rco;
  }
  HIP_TRY(hipMemsetAsync(scene->d_scratch, 0, 512, stream));
  constexpr int NT = 256;
  size_t scene_bytes = scene->hrc->scene_bytes();
  bool lds_scene = scene_bytes <= RTC_LDS_SCENE_MAX;
  size_t lds = lds_scene ? scene_bytes : 0;
  uint64_t total = list ? n_list : (uint64_t)W * nrows;
  uint64_t want = (total + NT - 1) / NT;
  // The grid is exactly what is RESIDENT at once (occupancy API: 2 workgroups per CU for rtc_kernel's 241 VGPRs, 3 for rtc_full_kernel's budget):
  // every workgroup stages the scene in LDS once and strides over the pixels.  Measured against the 8 per CU of rounds 1 - 2 (workgroups
  // queueing behind the resident ones, each staging the scene again, the last round of them half empty): teapot AA 1 0.548 -> 0.317 ms per
  // frame, AA 8 19.5 -> 17.0 ms; mirror scene 13.5 -> 10.8 ms, CSG scene 2.11 -> 1.76 ms.  RL_RTC_BLOCKS=<n> forces n per CU (A/B).
  auto grid_for = [&](const void *kern, size_t dyn_lds) -> uint32_t {
    uint64_t per_cu = (uint64_t)g_sw.rtc_blocks_per_cu;
    if (per_cu == 0) {
      static std::mutex mu;
      static std::map<std::pair<const void *, size_t>, int> cache;
      std::lock_guard<std::mutex> lk(mu);
      auto key = std::make_pair(kern, dyn_lds ^ ((size_t)scene->device << 48));
      auto it = cache.find(key);
      if (it == cache.end()) {
        int nb = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kern, NT, dyn_lds) != hipSuccess || nb < 1) nb = 2;
        it = cache.emplace(key, nb).first;
      }
      per_cu = (uint64_t)it->second;
    }
    return (uint32_t)(want < (uint64_t)g_cus * per_cu ? want : (uint64_t)g_cus * per_cu);
  };
  uint32_t blocks = 0;
  if (want_stats) HIP_TRY(hipEventRecord(scene->ev0, stream));
  const bool full = rc_.needs_full || g_sw.rtc_force_full;
  if (full) {  // (RL_RTC_FORCE_FULL: A/B, triangle-only worlds through the full kernel)  // shapes / CSG / patterns / reflection / refraction: the full World::color_at kernel
    RtcFullParams F{};
    F.R = P;
    F.shapes = scene->d_shapes, F.csgs = scene->d_csgs, F.patterns = scene->d_patterns;
    F.n_tris = P.n_tris, F.max_reflection_depth = rc_.max_reflection_depth;
    // register budget of three waves per SIMD (168 VGPRs; ~165 of the kernel's binary64 temporaries then live in scratch, at points that
    // run once per ray): measured 13.3 / 14.0 / 19.2 ms for 3 / 2 / 1 waves on the mirror scene at 1080p, 2.7 / 2.9 / 4.2 ms on the teapot
    // forced through this kernel.
    if (list) {
      blocks = grid_for((const void *)rtc_full_pixels_kernel<NT, 768>, 0);
      hipLaunchKernelGGL((rtc_full_pixels_kernel<NT, 768>), dim3(blocks), dim3(NT), 0, stream, F, d_xs, d_ys, n_list);
    } else {
      blocks = grid_for((const void *)rtc_full_kernel<NT, 768>, 0);
      hipLaunchKernelGGL((rtc_full_kernel<NT, 768>), dim3(blocks), dim3(NT), 0, stream, F);
    }
  // (241 VGPRs -> two waves per SIMD.  Measured in round 3 with the register budgets of three / four waves (68 / 128 spilled VGPRs): AA 8 19.5 -> 21.1 /
  // 22.5 ms, AA 1 0.547 -> 0.518 / 0.517 ms: the binary64 Moeller-Trumbore + Phong temporaries in scratch cost more than the extra waves hide.)
  } else if (list && lds_scene) {
    blocks = grid_for((const void *)rtc_pixels_kernel<NT, true>, lds);
    hipLaunchKernelGGL((rtc_pixels_kernel<NT, true>), dim3(blocks), dim3(NT), lds, stream, P, d_xs, d_ys, n_list);
  } else if (list) {
    blocks = grid_for((const void *)rtc_pixels_kernel<NT, false>, 0);
    hipLaunchKernelGGL((rtc_pixels_kernel<NT, false>), dim3(blocks), dim3(NT), 0, stream, P, d_xs, d_ys, n_list);
  } else if (lds_scene) {
    blocks = grid_for((const void *)rtc_kernel<NT, true>, lds);
    hipLaunchKernelGGL((rtc_kernel<NT, true>), dim3(blocks), dim3(NT), lds, stream, P);
  } else {
    blocks = grid_for((const void *)rtc_kernel<NT, false>, 0);
    hipLaunchKernelGGL((rtc_kernel<NT, false>), dim3(blocks), dim3(NT), 0, stream, P);
  }
  g_last_rtc_kernel = full ? 2u : 1u, g_last_rtc_list = list ? 1u : 0u, g_last_rtc_lds = full ? 0u : lds, g_last_rtc_blocks = blocks;
  HIP_TRY(hipGetLastError());
  if (want_stats) HIP_TRY(hipEventRecord(scene->ev1, stream));
  return RL_OK;  // the caller ends the render with collect_stats / post_status, which record ev_last behind the stats copy
}
// The launch half of rl_rtc_render_pixels*: rtc_render_launch's parameters, kernel choice and grid with the list flavours of the two kernels
int rtc_render_pixels_launch(const rl_scene *scene, const rl_rtc_camera *cam, uint32_t aa, const uint32_t *d_xs, const uint32_t *d_ys, uint64_t n, void *d_out,
                             hipStream_t stream, bool want_stats) {
  return rtc_render_launch(scene, cam, aa, 0, 1, d_out, stream, want_stats, d_xs, d_ys, n);
}
}  // namespace rl

extern "C" {

int rl_rtc_render_device(const rl_scene *scene, const rl_rtc_camera *cam, uint32_t aa, uint32_t row_first, uint32_t row_step, void *d_out,
                         void *hip_stream, rl_stats *st) {
  bool done;
  int rc = render_check(scene, 2, frame_of(cam), d_out && row_step != 0 && aa != 0, row_first, "empty image", st, done);
  if (done) return rc;
  hipStream_t stream = (hipStream_t)hip_stream;
  return render_run(scene, stream, st, [&] { return rl::rtc_render_launch(scene, cam, aa, row_first, row_step, d_out, stream, st != nullptr); });
}

// (the host forms leave aa == 0 to the _device form they call: a render of no rows is RL_OK whatever aa is, as it always was)
int rl_rtc_render_rows(const rl_scene *scene, const rl_rtc_camera *cam, uint32_t aa, uint32_t row_first, uint32_t row_step, double *out,
                       rl_stats *st) {
  bool done;
  int rc = render_check(scene, 2, frame_of(cam), out && row_step != 0, row_first, nullptr, st, done);
  if (done) return rc;
  HostStaging q(scene);
  void *d_out = q.out(out, frame_of(cam).rows_bytes(row_first, row_step));
  if (q.rc != RL_OK) return q.rc;
  rl_stats local;
  return q.finish(rl_rtc_render_device(scene, cam, aa, row_first, row_step, d_out, q.stream, &local), st, local);
}

int rl_rtc_render_pixels_device(const rl_scene *scene, const rl_rtc_camera *cam, uint32_t aa, const void *d_xs, const void *d_ys, uint64_t n, void *d_out,
                                void *hip_stream, rl_stats *st) {
  bool done;
  int rc = render_check(scene, 2, frame_of(cam), aa != 0 && (n == 0 || (d_xs && d_ys && d_out)), 0, "empty image", st, done);
  if (done) return rc;
  rc = list_length_check(n, st, done);
  if (done) return rc;
  hipStream_t stream = (hipStream_t)hip_stream;
  return render_run(scene, stream, st, [&] {
    return rl::rtc_render_pixels_launch(scene, cam, aa, (const uint32_t *)d_xs, (const uint32_t *)d_ys, n, d_out, stream, st != nullptr);
  });
}

int rl_rtc_render_pixels(const rl_scene *scene, const rl_rtc_camera *cam, uint32_t aa, const uint32_t *xs, const uint32_t *ys, uint64_t n, double *out,
                         rl_stats *st) {
  bool done;
  int rc = render_check(scene, 2, frame_of(cam), aa != 0 && (n == 0 || (xs && ys && out)), 0, "empty image", st, done);
  if (done) return rc;
  rc = list_length_check(n, st, done);
  if (done) return rc;
  if ((rc = pixel_list_check(frame_of(cam), xs, ys, n)) != RL_OK) return rc;
  HostStaging q(scene);
  const unsigned char *d_xy = (const unsigned char *)q.in({{xs, (size_t)n * sizeof(uint32_t)}, {ys, (size_t)n * sizeof(uint32_t)}});
  void *d_out = q.out(out, (size_t)n * 3 * sizeof(double));
  if (q.rc != RL_OK) return q.rc;
  rl_stats local;
  return q.finish(rl_rtc_render_pixels_device(scene, cam, aa, d_xy, d_xy + (size_t)n * sizeof(uint32_t), n, d_out, q.stream, &local), st, local);
}

int rl_rtc_encode_rgb8_device(const void *d_rgb, uint64_t n_pixels, void *d_rgb8, void *hip_stream) {
  if (!g_ready) return set_err(RL_E_NO_DEVICE, "rl_init has not succeeded");
  if (!d_rgb || !d_rgb8) return set_err(RL_E_INVALID, "bad argument");
  unsigned long long n = n_pixels * 3ull;
  if (n == 0) return RL_OK;
  hipLaunchKernelGGL(encode_rtc_rgb8, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)hip_stream, (const double *)d_rgb, n, (unsigned char *)d_rgb8);
  HIP_TRY(hipGetLastError());
  return RL_OK;
}

int rl_rtc_render_rgb8(const rl_scene *scene, const rl_rtc_camera *cam, uint32_t aa, uint8_t *out, rl_stats *st) {
  bool done;
  int rc = render_check(scene, 2, frame_of(cam), out != nullptr, 0, "empty image", st, done);
  if (done) return rc;
  const size_t npix = (size_t)cam->hsize * cam->vsize;
  return render_rgb8(
      scene, npix, out, st, [&](void *d_rgb, hipStream_t stream, rl_stats *local) { return rl_rtc_render_device(scene, cam, aa, 0, 1, d_rgb, stream, local); },
      [&](void *d_rgb, void *d_u8, hipStream_t stream) { return rl_rtc_encode_rgb8_device(d_rgb, npix, d_u8, stream); });
}

int rl_rtc_render(const rl_scene *scene, const rl_rtc_camera *cam, uint32_t aa, double *out, rl_stats *st) {
  return rl_rtc_render_rows(scene, cam, aa, 0, 1, out, st);
}

}  // extern "C"

// the batched queries' host layer (22 entry points); last, so that its kernels keep their order of first use
#include "rl_query_api.h"
#include "rl_pixel_render_api.h"  // the entry forms and the launch of rl_features_api.h, rl_ao_api.h, rl_direct_api.h, rl_nee_api.h
#include "rl_features_api.h"
#include "rl_denoise.h"
#include "rl_denoise_render.h"
#include "rl_occlusion_api.h"  // behind everything: its kernels are instantiated last, every earlier kernel keeps its place
#include "rl_rtiow_ao.h"       // (and the ambient-occlusion renders behind those, for the same reason)
#include "rl_ao_api.h"
#include "rl_rtiow_direct.h"   // (and the direct-lighting renders behind those; rl_rtiow_direct.h calls rl_rtiow_ao.h's any-hit walk)
#include "rl_direct_api.h"
#include "rl_rtiow_nee.h"      // (and the NEE path renders behind those; rl_rtiow_nee.h calls both walks, the texture and the scatter)
#include "rl_nee_api.h"
