// What the host side of every render and query entry point is made of (include/rl_render.h).  Not a translation unit of
// its own: rl_render.hip and rl_multi.hip include it once each, behind their HIP_TRY, which it uses.  No kernel is named here.
//   scene_context — the device context a scene lives on, made current; a scene whose context is gone is refused
//   render_check  — library ready, scene family, null arguments, the empty image, row_first past the last row
//   list_length_check / pixel_list_check — what the pixel-list renders add to it: the empty list, the list's bound, an element outside the image
//   render_run    — the scene's lock around a render's launches and its status (the queries' counterpart: rl_query_api.h query_run)
//   HostStaging   — the host-buffer forms' device copies of the caller's arrays, and the copy back
//   render_rgb8   — the two _rgb8 forms: staged sums, the family's render and encode, the bytes copied back
// A host-buffer form is a check, a staging line, the call of its _device form and finish.
#pragma once
#include <cstring>
#include <initializer_list>
#include <mutex>
#include <utility>
#include <vector>

#include "rl_scene.h"

namespace {
// a call that ended with one of these has written every output
bool outputs_written(int rc) { return rc == RL_OK || rc == RL_E_DEGENERATE; }

// The device context `scene` was created on, made current.  A later rl_init / rl_init_multi may have dropped that context or pointed it
// at another device: the scene's buffers are then not that context's stream's to use.
int scene_context(const rl_scene *scene, rl::DevCtx *&c) {
  if (scene->ctx < 0 || scene->ctx >= rl::n_contexts() || rl::context(scene->ctx).device != scene->device)
    return rl::set_err_public(RL_E_INVALID, "scene belongs to a device context that no longer exists (created under another rl_init / rl_init_multi)");
  c = &rl::context(scene->ctx);
  return rl::use_context(scene->ctx);
}

// what the render checks and the staging need of either family's camera
struct Frame {
  bool cam = false;  // the camera pointer was not null
  uint32_t w = 0, h = 0;
  // rows row_first, row_first + row_step, ... of the frame, compact: [nrows][w][3] f64
  size_t rows_bytes(uint32_t row_first, uint32_t row_step) const {
    const uint32_t nrows = row_first < h ? (h - row_first + row_step - 1) / row_step : 0;
    return (size_t)nrows * w * 3 * sizeof(double);
  }
};
Frame frame_of(const rl_rtiow_camera *c) { return c ? Frame{true, c->image_width, c->image_height} : Frame{}; }
Frame frame_of(const rl_rtc_camera *c) { return c ? Frame{true, c->hsize, c->vsize} : Frame{}; }

// The argument rules every render shares.  kind: the scene family the call takes (1 RTIOW, 2 RTC); args_ok: what else the call cannot do
// without (buffers, row_step, aa).  empty_text: what the call refuses an image without pixels with; null: it takes one as it takes
// row_first past the last row.  done: the call ends here with the returned code — an error, or a render of no rows, which touches no
// buffer and zeroes `st` when given.
int render_check(const rl_scene *scene, int kind, const Frame &f, bool args_ok, uint32_t row_first, const char *empty_text, rl_stats *st, bool &done) {
  done = true;
  if (!rl::lib_ready()) return rl::set_err_public(RL_E_NO_DEVICE, "rl_init has not succeeded");
  if (!scene || scene->kind != kind || !f.cam || !args_ok) return rl::set_err_public(RL_E_INVALID, "bad argument");
  const bool empty = f.w == 0 || f.h == 0;
  if (empty && empty_text) return rl::set_err_public(RL_E_INVALID, empty_text);
  if (empty || row_first >= f.h) {
    if (st) std::memset(st, 0, sizeof *st);
    return RL_OK;
  }
  done = false;
  return RL_OK;
}

// The pixel-list renders (rl_*_render_pixels*): an empty list is RL_OK, touches no buffer and zeroes `st` when given, as the empty batch of
// a query; a list the 32-bit work counter cannot number is refused; done: the call ends here with the returned code.  Both before
// anything is read, staged or launched.  The host forms then refuse a list with an element outside the image (pixel_list_check).
constexpr uint64_t PIXEL_LIST_MAX_N = 0xFFFF0000ull;  // n < this
int list_length_check(uint64_t n, rl_stats *st, bool &done) {
  done = true;
  if (n == 0) {
    if (st) std::memset(st, 0, sizeof *st);
    return RL_OK;
  }
  if (n >= PIXEL_LIST_MAX_N) return rl::set_err_public(RL_E_INVALID, "image too large");
  done = false;
  return RL_OK;
}
int pixel_list_check(const Frame &f, const uint32_t *xs, const uint32_t *ys, uint64_t n) {
  for (uint64_t i = 0; i < n; i++)
    if (xs[i] >= f.w || ys[i] >= f.h) return rl::set_err_public(RL_E_INVALID, "pixel outside the image");
  return RL_OK;
}

// One render of `scene` on `stream`: what `launch` enqueues (-> RL_*), then the status.  st: filled synchronously; null: asynchronous,
// status ring.  The scene's lock is held throughout (concurrent renders of one scene: see rl_scene::mu).
template <class Launch>
int render_run(const rl_scene *scene, hipStream_t stream, rl_stats *st, Launch launch) {
  std::lock_guard<std::mutex> lk(scene->mu);
  int rc = launch();
  if (rc != RL_OK) return rc;
  return st ? rl::collect_stats(scene, stream, st) : rl::post_status(scene, stream);
}

// The host-buffer forms: the caller's arrays staged in device memory of the scene's context, the call run on that context's library
// stream (synchronously: every form passes a local rl_stats or waits itself), the outputs copied back.  in / out / inout / back return
// the device pointer; an absent optional output is null in and null out.  The first failure stays in `rc` and makes the later steps do
// nothing: a form looks at it once, before it launches.
class HostStaging {
 public:
  int rc;
  hipStream_t stream = nullptr;
  // scene == null: the library's context 0 (a call without a scene; the multi-GPU forms, whose frames end on GPU 0 and which test the
  // scene's replicas themselves)
  explicit HostStaging(const rl_scene *scene) {
    rl::DevCtx *c = nullptr;
    if (scene) rc = scene_context(scene, c);
    else if ((rc = rl::use_context(0)) == RL_OK) c = &rl::context(0);
    if (rc == RL_OK) stream = c->stream;
    bufs_.reserve(5), back_.reserve(4);  // what the largest form stages: one host allocation each, whatever the call
  }
  // host arrays uploaded back to back into one allocation
  void *in(std::initializer_list<std::pair<const void *, size_t>> parts) {
    size_t total = 0, at = 0;
    for (const auto &p : parts) total += p.second;
    unsigned char *d = (unsigned char *)scratch(total);
    for (const auto &p : parts) {
      if (rc == RL_OK) rc = upload(d + at, p.first, p.second);
      at += p.second;
    }
    return d;
  }
  void *in(const void *host, size_t bytes) { return in({{host, bytes}}); }
  void *out(void *host, size_t bytes) { return host ? back(host, scratch(bytes), bytes) : nullptr; }
  void *inout(void *host, size_t bytes) { return host ? back(host, in(host, bytes), bytes) : nullptr; }
  // `dev` (staged by in) is also an output, copied to another host array than it came from
  void *back(void *host, void *dev, size_t bytes) {
    if (!host) return nullptr;
    back_.push_back({host, dev, bytes});
    return dev;
  }
  // device memory that is neither uploaded nor copied back
  void *scratch(size_t bytes) {
    if (rc != RL_OK) return nullptr;
    bufs_.emplace_back();
    rc = [&]() -> int {
      HIP_TRY(bufs_.back().reserve(bytes ? bytes : 1));
      return RL_OK;
    }();
    return bufs_.back().get();
  }
  // after the call returned qrc: the copies back, and *st = local when the caller gave opt_stats, where every output is written
  // (RL_OK, RL_E_DEGENERATE).  -> qrc, or what a copy failed with.
  int finish(int qrc, rl_stats *st, const rl_stats &local) {
    if (!outputs_written(qrc)) return qrc;
    int rcb = copy_back();
    if (rcb != RL_OK) return rcb;
    if (st) *st = local;
    return qrc;
  }
  // the forms without statistics: the copies back on RL_OK only
  int finish(int qrc) { return qrc == RL_OK ? copy_back() : qrc; }

 private:
  struct Back {
    void *host, *dev;
    size_t bytes;
  };
  std::vector<rl::DevBuf<unsigned char>> bufs_;
  std::vector<Back> back_;
  int copy_back() {
    for (const Back &b : back_)
      if (b.bytes) HIP_TRY(hipMemcpy(b.host, b.dev, b.bytes, hipMemcpyDeviceToHost));
    return RL_OK;
  }
  static int upload(void *dev, const void *host, size_t bytes) {
    if (bytes) HIP_TRY(hipMemcpy(dev, host, bytes, hipMemcpyHostToDevice));
    return RL_OK;
  }
};

// The _rgb8 forms: the whole frame rendered into staged sums (render(d_sum, stream, &stats) -> RL_*), encoded on the same stream
// (encode(d_sum, d_u8, stream)), and the bytes copied back on it: the library's stream does not wait for the null stream's copies.
template <class Render, class Encode>
int render_rgb8(const rl_scene *scene, size_t npix, uint8_t *out, rl_stats *st, Render render, Encode encode) {
  HostStaging q(scene);
  void *d_sum = q.scratch(npix * 3 * sizeof(double)), *d_u8 = q.scratch(npix * 3);
  if (q.rc != RL_OK) return q.rc;
  rl_stats local;
  int rc = render(d_sum, q.stream, &local);
  if (outputs_written(rc)) {
    int rce = encode(d_sum, d_u8, q.stream);
    if (rce != RL_OK) return rce;
    HIP_TRY(hipMemcpyAsync(out, d_u8, npix * 3, hipMemcpyDeviceToHost, q.stream));
    HIP_TRY(hipStreamSynchronize(q.stream));
  }
  return q.finish(rc, st, local);
}
}  // namespace
