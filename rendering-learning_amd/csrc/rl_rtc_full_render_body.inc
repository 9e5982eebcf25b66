  // The body of rtc_full_kernel / rtc_full_pixels_kernel (rl_rtc_full_kernel.h): included inside both, with LIST, xs, ys, n_list (and the kernel's
  // template parameters) in scope.  Textual, not a function: the frame kernel keeps the register allocation it had before the list flavour existed.
  const RtcParams &P = F.R;
  const int tid = threadIdx.x;
  const DevOp *ops = P.ops;
  const DevTri *tris = P.tris;
  const rl_rtc_camera &cam = P.cam;
  const uint32_t W = cam.hsize;
  RtcFullCounters cnt{0, 0, 0, 0, 0, 0};
  const uint64_t total = LIST ? n_list : (uint64_t)W * P.nrows;
  Ent list[RL_RTC_K];
  Pending stack[RTC_MAX_PENDING];
  for (uint64_t idx = (uint64_t)blockIdx.x * NT + tid; idx < total; idx += (uint64_t)gridDim.x * NT) {
    uint32_t px, py;
    if constexpr (LIST) {
      px = xs[idx], py = ys[idx];
      if (px >= W || py >= cam.vsize) {
        double *outp = P.out + idx * 3;
        outp[0] = 0.0, outp[1] = 0.0, outp[2] = 0.0;
        continue;
      }
    } else {
      uint32_t r = (uint32_t)(idx / W);
      px = (uint32_t)(idx % W);
      py = P.row_first + r * P.row_step;
    }
    D3 acc = d3(0.0, 0.0, 0.0);
    bool have = false;
    for (uint32_t nx = 0; nx < P.aa; nx++)
      for (uint32_t ny = 0; ny < P.aa; ny++) {
        double sample_offset = 1.0 / (double)P.aa;
        double xoffset = ((double)px + sample_offset * ((double)nx + 0.5)) * cam.pixel_size;
        double yoffset = ((double)py + sample_offset * ((double)ny + 0.5)) * cam.pixel_size;
        D3 pixel = mul_point(cam.inverse, d3(cam.half_width - xoffset, cam.half_height - yoffset, -1.0));
        D3 origin = mul_point(cam.inverse, d3(0.0, 0.0, 0.0));
        D3 dir;
        if (!norm(pixel - origin, dir)) {
          cnt.flagged++;
          dir = d3(0.0, 0.0, 0.0);
        }
#include "rl_rtc_color_at_body.inc"  // D3 c = color_at(origin, dir)
        acc = have ? acc + c : c;
        have = true;
      }
    D3 res = acc * (1.0 / (double)((uint64_t)P.aa * P.aa));
    double *outp = P.out + idx * 3;
    outp[0] = res.x, outp[1] = res.y, outp[2] = res.z;
  }
  rtc_query_flush(cnt, P.stats, tid);
