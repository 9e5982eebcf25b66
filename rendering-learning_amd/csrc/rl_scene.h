// Internal (not part of the ABI): the library's per-device context and the rl_scene object, shared by rl_render.hip (the
// single-device entry points) and rl_multi.hip (one process driving several GPUs).  Device buffers, pinned memory and events are held
// by the owning types of rl_devbuf.h (DevBuf<T>, PinnedBuf<T>, Event): rl_scene has no hand-written teardown.
#pragma once
#include <hip/hip_runtime.h>

#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "rl_devbuf.h"
#include "rl_program.h"
#include "rl_scene_host.h"  // HostRtiow, HostRtc: what the host side of a scene compiles to

namespace rl {

// One per GPU the library drives.  rl_init(device) creates exactly one; rl_init_multi(n) one per device 0 .. n-1.
struct DevCtx {
  int device = -1;        // HIP device ordinal
  hipStream_t stream = nullptr;  // library-owned stream (host-buffer entry points, multi-GPU renders)
  hipEvent_t ev = nullptr;       // "this device's shard has arrived" (peer-copy gather)
};

}  // namespace rl

struct rl_scene {
  int kind = 0;  // 1 = RTIOW, 2 = RTC
  int ctx = 0;   // index of the device context this replica lives on
  int device = -1;  // ... and that context's HIP device ordinal at creation (a later rl_init may point context 0 elsewhere)
  std::shared_ptr<const rl::HostRtiow> hrt;
  std::shared_ptr<const rl::HostRtc> hrc;
  const rl::RtiowProgram &rt() const { return hrt->rt; }
  const rl::RtcProgram &rc() const { return hrc->rc; }
  std::vector<rl_scene *> replicas;  // multi-GPU: replicas[g] lives on device context g; replicas[0] == this (empty: single device)
  // Every d_* / h_* / ev* member owns what it names (rl_devbuf.h): deleting the scene releases all of it, and a buffer that is grown
  // on demand is one reserve() at its use site.
  // RTIOW
  rl::DevBuf<rl::DevOp> d_ops, d_lops;
  rl::DevBuf<rl::DevMaterial> d_sphere_flat;
  rl::DevBuf<rl::DevChecker> d_sphere_checker;
  rl::DevBuf<rl::CompactOp> d_cops;
  rl::DevBuf<uint32_t> d_movbits;
  rl::DevBuf<rl::FastNode> d_fast_nodes;
  rl::DevBuf<rl::FastNodeCH> d_fast_nodes_ch;
  rl::DevBuf<float> d_fast_leaf_boxes;
  rl::DevBuf<double> d_fast_leaf_balls, d_fast_leaf_motion;
  rl::DevBuf<uint32_t> d_coop_pixels;  // cooperative kernel: pixel list (scratch, grown on demand)
  rl::DevBuf<uint32_t> d_steal_state, d_steal_n;  // work stealing on small shards (RtiowParams::steal_state)
  rl::DevBuf<rl::FastNodeQ> d_fg_nodes;
  rl::DevBuf<uint32_t> d_fg_seg_roots;
  rl::DevBuf<rl::FastMedium> d_fg_media;
  rl::DevBuf<rl::FastItem> d_fg_items;
  rl::DevBuf<rl::DevSphere> d_fg_spheres;
  rl::DevBuf<uint32_t> d_fg_material;
  rl::DevBuf<rl::DevSphere> d_spheres;
  rl::DevBuf<uint32_t> d_sphere_material;
  rl::DevBuf<rl::DevPlanar> d_planars;
  rl::DevBuf<rl_translate> d_translates;
  rl::DevBuf<rl_transform> d_transforms;
  rl::DevBuf<rl::DevMaterial> d_materials;
  rl::DevBuf<rl::DevTexture> d_textures;
  rl::DevBuf<rl::DevImage> d_images;
  rl::DevBuf<float> d_image_pool;
  rl::DevBuf<rl_perlin> d_perlins;
  rl::DevBuf<rl_medium> d_media;
  // RTC
  rl::DevBuf<rl::DevTri> d_tris;
  rl::DevBuf<rl_rtc_transformed> d_xforms;
  rl::DevBuf<rl_rtc_material> d_rmaterials;
  rl::DevBuf<rl_rtc_light> d_lights;
  rl::DevBuf<rl_rtc_shape> d_shapes;
  rl::DevBuf<rl_rtc_csg> d_csgs;
  rl::DevBuf<rl_rtc_pattern> d_patterns;
  rl::DevBuf<rl::RtcGuard> d_guards;
  rl::Event ev0, ev1;  // bracket the kernels of a counting render
  // Renders of one scene may be issued from several host threads and on several streams at once (the reference's Camera::render takes
  // &self, camera.rs:122).  The scene owns ONE set of work buffers, so: `mu` serialises the host side (enqueueing a render and handing
  // its status over, in one hold: a multi-GPU frame posts every replica's status before it lets go), and a render enqueued on another
  // stream than its predecessor first waits, on the device, for the predecessor's END (`ev_last`: recorded behind its stats copy by
  // post_status / collect_stats, so the next render's memset of d_scratch cannot overtake that copy) — concurrent callers are safe, their
  // frames are rendered one after the other (each one fills the GPU anyway).
  mutable std::mutex mu;
  hipStream_t last_stream = nullptr;
  rl::Event ev_last;
  bool has_last = false;
  // status of the asynchronous renders (opt_stats == NULL) not yet collected by rl_render_status: a ring of N_STATUS slots of 8 stats
  // words in pinned host memory, each behind the event that follows its copy; a slot that comes round again while still pending is
  // waited for and folded into `folded_*`, so no panic-site count is ever lost
  static constexpr int N_STATUS = 8;
  rl::PinnedBuf<unsigned long long> h_status;  // [N_STATUS][8]
  rl::Event ev_status[N_STATUS];
  bool status_pending[N_STATUS] = {};
  unsigned long long status_seq[N_STATUS] = {};
  int status_next = 0;
  unsigned long long next_seq = 0, folded_seq = 0, folded_rays = 0, folded_flagged = 0, folded_slow = 0;
  // cost-sorted (LPT) two-phase render: per-pixel ChaCha word positions, per-tile cost and order, the radix sort's scratch
  rl::DevBuf<uint32_t> d_pos, d_tile_cost, d_tile_order, d_tile_keys, d_tile_iota;
  rl::DevBuf<unsigned char> d_sort_temp;
  rl::DevBuf<uint32_t> d_pixel_entry;  // fast traversal: the current render's per-pixel entry words (rl_pixel_entry.h), grown on demand
  rl::DevBuf<uint32_t> d_pixel_entry_t;  // ... and its words by time slice, [pixel][T], grown on demand
  // What the two tables were last built from (rl_render.hip build_pixel_entry): a call that repeats all of it reads them as they are.  The event
  // follows the build, so that a call on another stream waits for it; entry_key_valid is false until a build and after a buffer was regrown.
  struct PixelEntryKey {
    uint32_t image_width, image_height;
    double lookfrom[3], pixel_00[3], pixel_du[3], pixel_dv[3], defocus_disk_u[3], defocus_disk_v[3], defocus_angle;
    uint32_t row_first, row_step, nrows, max_entries, sphere, slices;
  } entry_key;
  bool entry_key_valid = false;
  rl::Event ev_entry;
  hipStream_t entry_stream = nullptr;
  // multi-GPU: this replica's row shard / on replica 0 the gather buffer [G][max_rows][W][3]
  rl::DevBuf<double> d_shard;
  rl::Event ev_gather_read;  // replica 0: recorded behind the de-interleave kernel that reads the gather slots
  bool ev_gather_read_valid = false;
  // rl_rtiow_render_progress (opt-in: its first call switches it on for the renders that follow): the kernels' work counters then live
  // in two words of pinned HOST memory the device reaches over PCIe — [0] the first (or only) launch of a render, [1] the cost-sorted
  // resume launch — so that the host reads them with plain loads while the kernels run; `progress_total` = slots of the render enqueued last
  bool progress_on = false;
  unsigned long long progress_total = 0;
  rl::PinnedBuf<uint32_t> h_progress;  // host address
  uint32_t *d_progress = nullptr;      // the same words as the device sees them (not an allocation of its own)
  rl::DevBuf<unsigned char> d_params;  // device copies (two slots) of the parameter block for the kernels that take it by pointer
  unsigned params_slot = 0;
  rl::DevBuf<uint32_t> d_pix_rays;  // debug (tools/): per-pixel ray counts of the last counting render
  rl::DevBuf<double> d_indep;       // sample-parallel mode: the pass buffer [samples of a pass][shard pixels][3] (rl_rtiow_render_independent*)
  // per-scene scratch, 512 bytes: [0] work counter (u32), [64..] 8 x u64 stats, [128..384) the 32 scheduler debug words of rl_debug_sched
  // (word 31, byte 376: the first census word), [384..424) the other five census words of rl_debug_pixel_entry_census; [256] is also the
  // cooperative / stealing counter, which no counting launch uses.  Declared LAST, so released FIRST:
  // every scene has it, and its hipFree waits for the device's work in flight before the events and the pinned memory above go.
  rl::DevBuf<unsigned char> d_scratch;
};

namespace rl {

int set_err_public(int code, const std::string &m);
bool lib_ready();
int n_contexts();
DevCtx &context(int i);
int use_context(int i);  // hipSetDevice(context(i).device)
void drop_multi_state();  // rl_multi.hip: RCCL communicators + the emulation flag, dropped whenever the context list is rebuilt

// Launch-only halves of the render entry points (rl_render.hip): enqueue everything on `stream`, never synchronise.  The caller finishes
// the render, holding scene->mu since the launch, with collect_stats (want_stats; synchronises the stream) or post_status.
// d_out_sq (rl_rtiow_render_moments*, rl_rtiow_render_pixels_moments*): the second moments' buffer, laid out as d_out; null: a plain render
// rule, d_out_count (rl_rtiow_render_adaptive*, with d_out_sq): the stopping rule and the per-pixel sample counts; null: every pixel takes all its samples
int rtiow_render_launch(const rl_scene *scene, const rl_rtiow_camera *cam, uint64_t first_sample, uint32_t row_first, uint32_t row_step, void *d_out,
                        hipStream_t stream, bool want_stats, void *d_out_sq = nullptr, const rl_rtiow_adaptive *rule = nullptr, void *d_out_count = nullptr);
int rtc_render_launch(const rl_scene *scene, const rl_rtc_camera *cam, uint32_t aa, uint32_t row_first, uint32_t row_step, void *d_out, hipStream_t stream,
                      bool want_stats, const uint32_t *d_xs = nullptr, const uint32_t *d_ys = nullptr, uint64_t n_list = 0);
// pixel-list renders (rl_*_render_pixels*): n elements (d_xs[i], d_ys[i]) of the whole frame -> d_out[i]
int rtiow_render_pixels_launch(const rl_scene *scene, const rl_rtiow_camera *cam, uint64_t first_sample, const uint32_t *d_xs, const uint32_t *d_ys, uint64_t n,
                               void *d_out, hipStream_t stream, bool want_stats, bool timed, void *d_out_sq = nullptr);
int rtc_render_pixels_launch(const rl_scene *scene, const rl_rtc_camera *cam, uint32_t aa, const uint32_t *d_xs, const uint32_t *d_ys, uint64_t n, void *d_out,
                             hipStream_t stream, bool want_stats);
int collect_stats(const rl_scene *scene, hipStream_t stream, rl_stats *st);  // RL_OK / RL_E_DEGENERATE / RL_E_DEVICE
int post_status(const rl_scene *scene, hipStream_t stream);                  // asynchronous renders: next slot of the status ring
int order_after_previous(const rl_scene *scene, hipStream_t stream);         // start of a render: device-side wait for the scene's previous render
int mark_render_end(const rl_scene *scene, hipStream_t stream);              // end of a render: behind its stats copy (collect_stats / post_status)
void add_stats(rl_stats *acc, const rl_stats &s);                             // sums counters, max of kernel_ms
unsigned status_gap_host_us();                                                // rl_debug_set_status_gap's host sleep (tests; 0: none)

}  // namespace rl
