// denoise_render on the device (include/rl_render.h "Denoising", rl_denoise_prepare_device .. rl_rtiow_render_denoised_rgb8; DESIGN.md
// §3.18): the two elementwise kernels around the a-trous passes of rl_denoise.h, and their host side.  Not a translation unit of its own:
// rl_render.hip includes it once, behind rl_denoise.h, and it uses that file's statics and the staging of rl_host_api.h.
//
// prepare turns what the moments / adaptive renders and the feature render wrote into the three images a pass reads; finish multiplies
// the filtered images back by the albedo and can encode the picture.  Binary64, every operation rounded on its own (no FMA), sums left to
// right; uint32 inputs convert exactly.  Per pixel p and channel c (tests/denoise_render_model.py is this statement in numpy):
//     n        = (double)counts[p]  with a counts image, else (double)samples
//     mean[c]  = sums[c] / n        with counts;  sums[c] * (1.0 / samples)  without (the reciprocal is one rounded division)
//     raw[c]   = (((sq[c] - (sums[c] * sums[c]) / n) / (n - 1.0)) / n)
//     var[c]   = raw[c] < 0 ? 0.0 : raw[c]                       -- not fmax: a NaN stays NaN
//     alb[c]   = albedo_sum[c] * (1.0 / feature_samples)
//     a[c]     = alb[c] > 0 ? alb[c] : 1.0                       -- a NaN albedo divides by 1
//     color[c] = mean[c] / a[c] ;  variance[c] = var[c] / (a[c] * a[c])
//     guides, in this order, each group present iff its RL_GUIDE_* bit of `want` is set:
//       albedo (3):   alb[c]
//       normal (3):   l = sqrt((ns0*ns0 + ns1*ns1) + ns2*ns2) ;  l != 0 ? ns[c] / l : 0.0      (sqrt: the correctly rounded one)
//       depth (1):    depth_sum / (double)max(hit_count, 1)
//       coverage (1): (double)hit_count / (double)feature_samples
//     finish:  out_color[c] = color_f[c] * a[c] ;  out_variance[c] = variance_f[c] * (a[c] * a[c])      -- a recomputed from albedo_sum
//              out_rgb8[c]  = the byte rl_rtiow_encode_rgb8_device gives out_color[c] with samples = 1
// No input is scanned: a pixel whose count is 0 or 1 gets the non-finite values the arithmetic gives (x / 0, 0 / 0), and the passes spread
// them to the pixels whose 25-tap footprints touch it and no further (rl_denoise.h).
#pragma once

namespace {
constexpr uint32_t DENOISE_NT = 256;
constexpr uint32_t DENOISE_ROW = 9;  // doubles between two pixels' guide rows in LDS: the first odd number that holds 8 channels
constexpr uint32_t DENOISE_MAX_BLOCKS_PER_CU = 2048 / DENOISE_NT;
constexpr uint32_t GUIDE_ALL = RL_GUIDE_ALBEDO | RL_GUIDE_NORMAL | RL_GUIDE_DEPTH | RL_GUIDE_COVERAGE;

uint32_t guide_channels(uint32_t want) {
  return 3 * !!(want & RL_GUIDE_ALBEDO) + 3 * !!(want & RL_GUIDE_NORMAL) + !!(want & RL_GUIDE_DEPTH) + !!(want & RL_GUIDE_COVERAGE);
}

struct DenoisePrepare {
  uint64_t npix;
  const double *sums, *sq;
  const uint32_t *counts;  // null: every pixel took n_all samples
  const double *albedo_sum, *normal_sum, *depth_sum;
  const uint32_t *hit_count;
  double n_all, inv_samples, inv_feature_samples, feature_samples;  // (double)samples, 1.0 / samples, 1.0 / feature_samples, (double)feature_samples
  uint32_t want, G;
  double *color, *variance, *guides;
};

struct DenoiseFinish {
  uint64_t npix;
  const double *color, *variance, *albedo_sum;  // variance: read iff out_variance
  double inv_feature_samples;
  double *out_color, *out_variance;  // each optional
  unsigned char *out_rgb8;           // optional
};

// a[c] of the definition: what the colour is divided by before the passes and multiplied by after them
__device__ inline double denoise_albedo_divisor(double alb) { return alb > 0.0 ? alb : 1.0; }

// One workgroup takes 256 adjacent pixels, grid-stride over such blocks.  Colour and variance need nothing of a pixel but its count, so
// the block's 768 values of each [H][W][3] image are walked flat, lane t at value j * 256 + t: every access of a wave is 512 contiguous
// bytes.  (One pixel per lane, 24 bytes apart, and a 64-byte guide row per lane, reached 0.47 of a copy's bandwidth)
// The guide rows are put together in LDS (the normal needs its pixel's three sums in one lane) and written out flat as well.
__global__ void __launch_bounds__(DENOISE_NT) denoise_prepare_kernel(const DenoisePrepare P) {
  __shared__ double rows[DENOISE_NT * DENOISE_ROW];  // the block's guide rows, DENOISE_ROW doubles apart: an odd stride, no bank conflict
  __shared__ double normal_sums[DENOISE_NT * 3];
  const uint32_t t = threadIdx.x;
  const uint64_t blocks = (P.npix + DENOISE_NT - 1) / DENOISE_NT;
  for (uint64_t b = blockIdx.x; b < blocks; b += gridDim.x) {
    const uint64_t p0 = b * DENOISE_NT;
    const uint32_t np = (uint32_t)(P.npix - p0 < DENOISE_NT ? P.npix - p0 : DENOISE_NT);  // the last block may be short
    uint32_t at = 0;  // the channel the next group of guides starts at
    for (uint32_t j = 0; j < 3; j++) {
      const uint32_t v = j * DENOISE_NT + t, pl = v / 3, c = v - pl * 3;
      if (v < np * 3) {
        const uint64_t e = p0 * 3 + v;
        const double n = P.counts ? (double)P.counts[p0 + pl] : P.n_all;
        const double s = P.sums[e];
        const double mean = P.counts ? s / n : s * P.inv_samples;
        const double raw = (((P.sq[e] - (s * s) / n) / (n - 1.0)) / n);
        const double var = raw < 0.0 ? 0.0 : raw;
        const double alb = P.albedo_sum[e] * P.inv_feature_samples;
        const double a = denoise_albedo_divisor(alb);
        P.color[e] = mean / a;
        P.variance[e] = var / (a * a);
        if (P.want & RL_GUIDE_ALBEDO) rows[pl * DENOISE_ROW + c] = alb;
        if (P.want & RL_GUIDE_NORMAL) normal_sums[v] = P.normal_sum[e];
      }
    }
    if (P.want & RL_GUIDE_ALBEDO) at += 3;
    if (P.want & RL_GUIDE_NORMAL) {
      __syncthreads();
      if (t < np) {
        const double ns[3] = {normal_sums[t * 3], normal_sums[t * 3 + 1], normal_sums[t * 3 + 2]};
        const double l = sqrt((ns[0] * ns[0] + ns[1] * ns[1]) + ns[2] * ns[2]);
        for (int c = 0; c < 3; c++) rows[t * DENOISE_ROW + at + c] = l != 0.0 ? ns[c] / l : 0.0;
      }
      at += 3;
    }
    if ((P.want & (RL_GUIDE_DEPTH | RL_GUIDE_COVERAGE)) && t < np) {
      const uint32_t k = P.hit_count[p0 + t];
      if (P.want & RL_GUIDE_DEPTH) rows[t * DENOISE_ROW + at++] = P.depth_sum[p0 + t] / (double)(k > 1 ? k : 1);
      if (P.want & RL_GUIDE_COVERAGE) rows[t * DENOISE_ROW + at] = (double)k / P.feature_samples;
    }
    __syncthreads();
    for (uint32_t v = t; v < np * P.G; v += DENOISE_NT) {
      const uint32_t pl = v / P.G;
      P.guides[p0 * P.G + v] = rows[pl * DENOISE_ROW + (v - pl * P.G)];
    }
    __syncthreads();  // the next block's rows overwrite what this one's lanes read
  }
}

// Elementwise in the single values: nothing here needs to know which pixel a value belongs to, so lane i takes value i of npix * 3 and
// every access of a wave is contiguous.  Every lane reads its value before it writes it, so an output may be the input of the same name.
__global__ void __launch_bounds__(DENOISE_NT) denoise_finish_kernel(const DenoiseFinish F) {
  for (uint64_t e = (uint64_t)blockIdx.x * DENOISE_NT + threadIdx.x; e < F.npix * 3; e += (uint64_t)gridDim.x * DENOISE_NT) {
    const double a = denoise_albedo_divisor(F.albedo_sum[e] * F.inv_feature_samples);
    const double col = F.color[e] * a;
    if (F.out_variance) F.out_variance[e] = F.variance[e] * (a * a);
    if (F.out_color) F.out_color[e] = col;
    if (F.out_rgb8) F.out_rgb8[e] = rtiow_rgb8_of(col, 1.0);
  }
}

// min(ceil(n / 256), cap) workgroups for n pixels (prepare) or values (finish): rl_debug_set_denoise_blocks caps these two as it caps a
// pass (rl_debug_last_denoise_launch reports passes only)
uint32_t denoise_elementwise_blocks(uint64_t npix) {
  const uint32_t max_blocks = g_denoise_max_blocks.load();
  const uint64_t cap = max_blocks ? max_blocks : (uint64_t)std::max(1, g_cus) * DENOISE_MAX_BLOCKS_PER_CU;
  return (uint32_t)std::min<uint64_t>((npix + DENOISE_NT - 1) / DENOISE_NT, cap);
}

bool denoise_npix_ok(uint32_t width, uint32_t height) { return (uint64_t)width * height < PIXEL_LIST_MAX_N; }

// What every entry point asks of an rl_denoise_inputs, before the device is looked at: RL_OK or RL_E_INVALID.
int denoise_inputs_check(const rl_denoise_inputs *in) {
  if (!in || !in->sums || !in->sq || !in->albedo_sum) return set_err(RL_E_INVALID, "bad argument");
  if ((in->want & ~GUIDE_ALL) || in->reserved != 0) return set_err(RL_E_INVALID, "want holds a bit beyond the four guides, or reserved not 0");
  if (((in->want & RL_GUIDE_NORMAL) && !in->normal_sum) || ((in->want & RL_GUIDE_DEPTH) && !in->depth_sum) ||
      ((in->want & (RL_GUIDE_DEPTH | RL_GUIDE_COVERAGE)) && !in->hit_count))
    return set_err(RL_E_INVALID, "a guide is asked for whose sums are missing");
  if (in->feature_samples == 0) return set_err(RL_E_INVALID, "feature_samples must be >= 1");
  if (!in->counts && in->samples < 2) return set_err(RL_E_INVALID, "a variance estimate needs samples >= 2");
  return RL_OK;
}

// ... and of what rl_denoise_render_device and rl_denoise_render take beside it (the images of the passes are carved from the work buffer,
// so of atrous_check only the parameter rules and the image's bound are left to ask)
int denoise_render_check(uint32_t width, uint32_t height, const rl_denoise_inputs *in, uint32_t iterations, const rl_atrous_params *p, const void *out_color,
                         const void *out_variance, const void *out_rgb8) {
  int rc = denoise_inputs_check(in);
  if (rc != RL_OK) return rc;
  if (!p) return set_err(RL_E_INVALID, "bad argument");
  if ((rc = atrous_params_check(p)) != RL_OK) return rc;
  if (p->n_guides != guide_channels(in->want)) return set_err(RL_E_INVALID, "n_guides is not the number of guide channels want asks for");
  if (iterations > ATROUS_MAX_ITERATIONS) return set_err(RL_E_INVALID, "iterations beyond 12");
  if (!out_color && !out_variance && !out_rgb8) return set_err(RL_E_INVALID, "no output asked for");
  if (out_color && out_color == out_variance) return set_err(RL_E_INVALID, "the two outputs are one buffer");
  if (!denoise_npix_ok(width, height)) return set_err(RL_E_INVALID, "image too large");
  return RL_OK;
}
}  // namespace

extern "C" {

int rl_denoise_prepare_device(uint32_t width, uint32_t height, const rl_denoise_inputs *in, void *d_color, void *d_variance, void *d_guides, void *hip_stream) {
  int rc = denoise_inputs_check(in);
  if (rc != RL_OK) return rc;
  const uint32_t G = guide_channels(in->want);
  if (!d_color || !d_variance || (G != 0 && !d_guides) || d_color == d_variance) return set_err(RL_E_INVALID, "bad argument");
  if (!denoise_npix_ok(width, height)) return set_err(RL_E_INVALID, "image too large");
  if (!g_ready) return set_err(RL_E_NO_DEVICE, "rl_init has not succeeded");
  if (width == 0 || height == 0) return RL_OK;
  DenoisePrepare P{};
  P.npix = (uint64_t)width * height;
  P.sums = (const double *)in->sums, P.sq = (const double *)in->sq, P.counts = (const uint32_t *)in->counts;
  P.albedo_sum = (const double *)in->albedo_sum, P.normal_sum = (const double *)in->normal_sum, P.depth_sum = (const double *)in->depth_sum;
  P.hit_count = (const uint32_t *)in->hit_count;
  if (!in->counts) P.n_all = (double)in->samples, P.inv_samples = 1.0 / (double)in->samples;
  P.feature_samples = (double)in->feature_samples, P.inv_feature_samples = 1.0 / (double)in->feature_samples;
  P.want = in->want, P.G = G;
  P.color = (double *)d_color, P.variance = (double *)d_variance, P.guides = (double *)d_guides;
  hipLaunchKernelGGL(denoise_prepare_kernel, dim3(denoise_elementwise_blocks(P.npix)), dim3(DENOISE_NT), 0, (hipStream_t)hip_stream, P);
  HIP_TRY(hipGetLastError());
  return RL_OK;
}

int rl_denoise_finish_device(uint32_t width, uint32_t height, const void *d_color, const void *d_variance, const void *d_albedo_sum, uint32_t feature_samples,
                             void *d_out_color, void *d_out_variance, void *d_out_rgb8, void *hip_stream) {
  if (!d_color || !d_albedo_sum || (d_out_variance && !d_variance) || feature_samples == 0) return set_err(RL_E_INVALID, "bad argument");
  if (!d_out_color && !d_out_variance && !d_out_rgb8) return set_err(RL_E_INVALID, "no output asked for");
  if (d_out_color && d_out_color == d_out_variance) return set_err(RL_E_INVALID, "the two outputs are one buffer");
  if (!denoise_npix_ok(width, height)) return set_err(RL_E_INVALID, "image too large");
  if (!g_ready) return set_err(RL_E_NO_DEVICE, "rl_init has not succeeded");
  if (width == 0 || height == 0) return RL_OK;
  DenoiseFinish F{};
  F.npix = (uint64_t)width * height;
  F.color = (const double *)d_color, F.variance = (const double *)d_variance, F.albedo_sum = (const double *)d_albedo_sum;
  F.inv_feature_samples = 1.0 / (double)feature_samples;
  F.out_color = (double *)d_out_color, F.out_variance = (double *)d_out_variance, F.out_rgb8 = (unsigned char *)d_out_rgb8;
  hipLaunchKernelGGL(denoise_finish_kernel, dim3(denoise_elementwise_blocks(F.npix * 3)), dim3(DENOISE_NT), 0, (hipStream_t)hip_stream, F);
  HIP_TRY(hipGetLastError());
  return RL_OK;
}

uint64_t rl_denoise_render_work_bytes(uint32_t width, uint32_t height, uint32_t n_guides) {
  return (uint64_t)width * height * sizeof(double) * (12 + (uint64_t)n_guides);
}

int rl_denoise_render_device(uint32_t width, uint32_t height, const rl_denoise_inputs *in, uint32_t iterations, const rl_atrous_params *p, void *d_work,
                             uint64_t work_bytes, void *d_out_color, void *d_out_variance, void *d_out_rgb8, void *hip_stream) {
  int rc = denoise_render_check(width, height, in, iterations, p, d_out_color, d_out_variance, d_out_rgb8);
  if (rc != RL_OK) return rc;
  const uint64_t need = rl_denoise_render_work_bytes(width, height, p->n_guides);
  if (work_bytes < need || (need != 0 && !d_work)) return set_err(RL_E_INVALID, "the work buffer is smaller than rl_denoise_render_work_bytes");
  if (!g_ready) return set_err(RL_E_NO_DEVICE, "rl_init has not succeeded");
  if (width == 0 || height == 0) return RL_OK;
  // the work buffer: two colour / variance pairs for the passes' ping-pong, then the guide image
  const size_t image = (size_t)width * height * 3 * sizeof(double);
  unsigned char *w = (unsigned char *)d_work;
  struct Pair {
    void *color, *variance;
  } pairs[2] = {{w, w + image}, {w + 2 * image, w + 3 * image}}, src = pairs[0];
  void *d_guides = p->n_guides ? w + 4 * image : nullptr;
  if ((rc = rl_denoise_prepare_device(width, height, in, src.color, src.variance, d_guides, hip_stream)) != RL_OK) return rc;
  for (uint32_t it = 0; it < iterations; it++) {  // step = 1, 2, .., 2^(iterations - 1)
    Pair dst = pairs[(it + 1) & 1];
    if (it + 1 == iterations && !d_out_variance) dst.variance = nullptr;  // the last pass: nothing reads its variance
    if ((rc = rl_denoise_atrous_pass_device(width, height, 1u << it, p, src.color, src.variance, d_guides, dst.color, dst.variance, hip_stream)) != RL_OK) return rc;
    src = dst;
  }
  return rl_denoise_finish_device(width, height, src.color, src.variance, in->albedo_sum, in->feature_samples, d_out_color, d_out_variance, d_out_rgb8, hip_stream);
}

int rl_denoise_render(uint32_t width, uint32_t height, const rl_denoise_inputs *in, uint32_t iterations, const rl_atrous_params *p, double *out_color,
                      double *out_variance, uint8_t *out_rgb8) {
  int rc = denoise_render_check(width, height, in, iterations, p, out_color, out_variance, out_rgb8);
  if (rc != RL_OK) return rc;
  if (!g_ready) return set_err(RL_E_NO_DEVICE, "rl_init has not succeeded");
  const size_t npix = (size_t)width * height, rgb = npix * 3 * sizeof(double), one = npix * sizeof(double), word = npix * sizeof(uint32_t);
  if (npix == 0) return RL_OK;
  const bool normal = in->want & RL_GUIDE_NORMAL, depth = in->want & RL_GUIDE_DEPTH, hits = in->want & (RL_GUIDE_DEPTH | RL_GUIDE_COVERAGE);
  HostStaging q(nullptr);
  // one allocation, the f64 images first: every one of them starts at a multiple of 8 bytes
  unsigned char *d = (unsigned char *)q.in({{in->sums, rgb}, {in->sq, rgb}, {in->albedo_sum, rgb}, {in->normal_sum, normal ? rgb : 0}, {in->depth_sum, depth ? one : 0},
                                            {in->counts, in->counts ? word : 0}, {in->hit_count, hits ? word : 0}});
  rl_denoise_inputs dev = *in;
  size_t at = 0;
  auto take = [&](bool present, size_t bytes) -> const void * {
    const void *ptr = present ? d + at : nullptr;
    at += present ? bytes : 0;
    return ptr;
  };
  dev.sums = take(true, rgb), dev.sq = take(true, rgb), dev.albedo_sum = take(true, rgb), dev.normal_sum = take(normal, rgb), dev.depth_sum = take(depth, one);
  dev.counts = take(in->counts != nullptr, word), dev.hit_count = take(hits, word);
  const uint64_t work_bytes = rl_denoise_render_work_bytes(width, height, p->n_guides);
  void *d_work = q.scratch(work_bytes);
  void *d_out_color = q.out(out_color, rgb), *d_out_variance = q.out(out_variance, rgb), *d_out_rgb8 = q.out(out_rgb8, npix * 3);
  if (q.rc != RL_OK) return q.rc;
  rc = rl_denoise_render_device(width, height, &dev, iterations, p, d_work, work_bytes, d_out_color, d_out_variance, d_out_rgb8, q.stream);
  if (rc != RL_OK) return rc;
  HIP_TRY(hipStreamSynchronize(q.stream));  // the copies back run on the null stream, which the library's stream does not wait for
  return q.finish(RL_OK);
}

// The sibling of rl_rtiow_render_rgb8: the public device forms composed on the library's stream.  Every rule of the scene, the camera and
// the rows is the composed calls' own.
int rl_rtiow_render_denoised_rgb8(const rl_scene *scene, const rl_rtiow_camera *cam, const rl_rtiow_adaptive *opt_rule, uint32_t feature_samples, uint32_t want,
                                  uint32_t iterations, const rl_atrous_params *p, uint8_t *out_rgb8) {
  if (!scene || !cam || !out_rgb8) return set_err(RL_E_INVALID, "bad argument");
  const uint32_t W = cam->image_width, H = cam->image_height;
  if (!denoise_npix_ok(W, H)) return set_err(RL_E_INVALID, "image too large");
  const size_t npix = (size_t)W * H, rgb = npix * 3 * sizeof(double);
  rl_denoise_inputs in{};
  in.samples = cam->samples_per_pixel, in.feature_samples = feature_samples, in.want = want;
  // placeholders that the argument check can look at before the device is: they are replaced below
  in.sums = in.sq = in.albedo_sum = in.normal_sum = in.depth_sum = in.hit_count = cam;
  if (opt_rule) in.counts = cam;
  int rc = denoise_render_check(W, H, &in, iterations, p, nullptr, nullptr, out_rgb8);
  if (rc != RL_OK) return rc;
  if (!g_ready) return set_err(RL_E_NO_DEVICE, "rl_init has not succeeded");
  const bool normal = want & RL_GUIDE_NORMAL, depth = want & RL_GUIDE_DEPTH, hits = want & (RL_GUIDE_DEPTH | RL_GUIDE_COVERAGE);
  HostStaging q(scene);
  in.sums = q.scratch(rgb), in.sq = q.scratch(rgb), in.albedo_sum = q.scratch(rgb);
  in.counts = opt_rule ? q.scratch(npix * sizeof(uint32_t)) : nullptr;
  in.normal_sum = normal ? q.scratch(rgb) : nullptr, in.depth_sum = depth ? q.scratch(npix * sizeof(double)) : nullptr;
  in.hit_count = hits ? q.scratch(npix * sizeof(uint32_t)) : nullptr;
  const uint64_t work_bytes = rl_denoise_render_work_bytes(W, H, p->n_guides);
  void *d_work = q.scratch(work_bytes), *d_u8 = q.scratch(npix * 3);
  if (q.rc != RL_OK) return q.rc;
  rc = opt_rule ? rl_rtiow_render_adaptive_device(scene, cam, 0, 0, 1, opt_rule, (void *)in.sums, (void *)in.sq, (void *)in.counts, q.stream, nullptr)
                : rl_rtiow_render_moments_device(scene, cam, 0, 0, 1, (void *)in.sums, (void *)in.sq, q.stream, nullptr);
  if (rc != RL_OK) return rc;
  rl_rtiow_camera fcam = *cam;
  fcam.samples_per_pixel = feature_samples;
  const rl_rtiow_features f{(double *)in.albedo_sum, (double *)in.normal_sum, (double *)in.depth_sum, (uint32_t *)in.hit_count};
  if ((rc = rl_rtiow_render_features_device(scene, &fcam, 0, 0, 1, &f, q.stream, nullptr)) != RL_OK) return rc;
  if (npix == 0) return RL_OK;
  if ((rc = rl_denoise_render_device(W, H, &in, iterations, p, d_work, work_bytes, nullptr, nullptr, d_u8, q.stream)) != RL_OK) return rc;
  HIP_TRY(hipMemcpyAsync(out_rgb8, d_u8, npix * 3, hipMemcpyDeviceToHost, q.stream));
  HIP_TRY(hipStreamSynchronize(q.stream));
  return rl_render_status(scene, nullptr);  // the two renders were asynchronous: RL_E_DEGENERATE where one reached a panic site, the picture written
}

}  // extern "C"
