// The edge-avoiding a-trous denoiser (include/rl_render.h "Denoising", rl_denoise_atrous*): one kernel and its host side.
// Not a translation unit of its own: rl_render.hip includes it once, behind rl_features_api.h, and it uses that file's statics (g_ready,
// g_cus, g_lds_max, set_err, HIP_TRY) and the staging of rl_host_api.h.  It needs no scene.
//
// One pass.  Images are row-major f64: color [H][W][3], variance [H][W][3] (the variance of each pixel mean, >= 0), guides [H][W][G],
// 0 <= G <= 8.  Parameters: color_sigma2 >= 0, variance_floor >= DBL_MIN, guide_inv_sigma[G] >= 0 (0 switches a guide off), step >= 1.
// Let h = [1/16, 1/4, 3/8, 1/4, 1/16].  For pixel p = (x, y), visit the 25 taps q = (x + i*step, y + j*step) with j = -2..2 outer and
// i = -2..2 inner.  Skip taps outside the image.  Every operation is rounded separately (binary64, no FMA) and sums run left to right:
//     vsum(r) = (var_r[0] + var_r[1]) + var_r[2]
//     d       = color_p - color_q ;  d2 = (d0*d0 + d1*d1) + d2*d2
//     D       = color_sigma2 * (vsum(p) + vsum(q)) + variance_floor
//     xg      = 0 ; for k in 0..G-1: e = (guide_p[k] - guide_q[k]) * guide_inv_sigma[k] ; xg = xg + e*e
//     w       = ((h[j+2]*h[i+2]) * D) / ((D + d2) * (1.0 + xg))
//     sw      = sw + w ;  ac[c] = ac[c] + w * color_q[c] ;  av[c] = av[c] + (w*w) * var_q[c]
//     out_color[c] = ac[c] / sw ;  out_variance[c] = av[c] / (sw*sw)
// sw, ac and av start at +0.0.  The weights are Cauchy-type, 1 / (1 + x), in place of exp(-x): + - * / only, so tests/atrous_model.py
// reproduces every output bit.  variance_floor is a normal number, so wherever D is finite the centre tap has w = (9/64 * D) / (D * 1) > 0
// and sw > 0 (a subnormal floor is refused: 9/64 * 5e-324 rounds to 0, and a flat image without variance would be 0 / 0 everywhere).  With
// finite inputs and color_sigma2 * (vsum(p) + vsum(q)) + variance_floor finite for every pair, every output is finite: an overflowing d2 or
// xg only takes that tap's w to 0.  Where D overflows, w is inf / inf and every output of the pixel is NaN.  A non-finite input gives
// non-finite outputs in the pixels whose footprint touches it, and in no other; no input is scanned.
//
// Two routes, one arithmetic (atrous_pixel), the same bytes.  "images": a workgroup takes 32 x 8 adjacent pixels and every tap is read from
// the images.  "lds": a workgroup takes 32 x 8 pixels of one LATTICE of the pass, the pixels (phx + u*step, phy + v*step): their taps lie
// on the same lattice, so the tile and a halo of two lattice points per side, 36 x 12 points of 6 + G doubles (at most 48,384 bytes, whatever
// the step), are staged in LDS, channel planes apart, and every tap is read from there.  Which one serves a pass: atrous_route_lds.
#pragma once

namespace {
constexpr uint32_t ATROUS_TILE_W = 32, ATROUS_TILE_H = 8;  // one pixel per lane; a half-wave is one row of 32: 256 contiguous bytes of an LDS plane
constexpr uint32_t ATROUS_NT = ATROUS_TILE_W * ATROUS_TILE_H;
constexpr uint32_t ATROUS_LDS_W = ATROUS_TILE_W + 4, ATROUS_LDS_H = ATROUS_TILE_H + 4, ATROUS_LDS_PLANE = ATROUS_LDS_W * ATROUS_LDS_H;
constexpr uint32_t ATROUS_MAX_BLOCKS_PER_CU = 2048 / ATROUS_NT;
constexpr uint32_t ATROUS_MAX_GUIDES = 8, ATROUS_MAX_STEP = 1u << 20, ATROUS_MAX_ITERATIONS = 12;

struct AtrousPass {
  uint32_t W, H, step, G;
  // the tiling: phases_x * phases_y lattices (one, of step 1, on the images route) of tiles_x * tiles_y tiles each
  uint32_t phases_x, phases_y, tiles_x, tiles_y;
  uint64_t tiles;
  double color_sigma2, variance_floor;
  double guide_inv_sigma[ATROUS_MAX_GUIDES];
  const double *color, *variance, *guides;
  double *out_color, *out_variance;  // out_variance: optional
};

// lds: lattices of `step` (only the phases that hold a pixel: an image narrower than the step has fewer); images: the one lattice of step 1
void atrous_tiling(AtrousPass &A, bool lds) {
  const uint32_t s = lds ? A.step : 1;
  A.phases_x = std::min(s, A.W), A.phases_y = std::min(s, A.H);
  const uint64_t nu = ((uint64_t)A.W + s - 1) / s, nv = ((uint64_t)A.H + s - 1) / s;  // lattice points of phase 0, the largest
  A.tiles_x = (uint32_t)((nu + ATROUS_TILE_W - 1) / ATROUS_TILE_W), A.tiles_y = (uint32_t)((nv + ATROUS_TILE_H - 1) / ATROUS_TILE_H);
  A.tiles = (uint64_t)A.phases_x * A.phases_y * A.tiles_x * A.tiles_y;
}

// The images as a pixel's taps read them, tap (i, j) = pixel (x + i*step, y + j*step): from global memory ...
struct AtrousImageTaps {
  const AtrousPass &A;
  int64_t centre;  // y * W + x
  __device__ size_t at(int i, int j) const { return (size_t)(centre + ((int64_t)j * A.W + i) * (int64_t)A.step); }
  __device__ double color(int i, int j, int c) const { return A.color[at(i, j) * 3 + c]; }
  __device__ double variance(int i, int j, int c) const { return A.variance[at(i, j) * 3 + c]; }
  __device__ double guide(int i, int j, uint32_t k) const { return A.guides[at(i, j) * A.G + k]; }
};
// ... or from the staged lattice points: plane c of 6 + G (colour, variance, guides) at lds + c * ATROUS_LDS_PLANE
struct AtrousLdsTaps {
  const double *lds;
  uint32_t centre;  // (ly + 2) * ATROUS_LDS_W + lx + 2
  __device__ uint32_t at(int i, int j) const { return (uint32_t)((int)centre + j * (int)ATROUS_LDS_W + i); }
  __device__ double color(int i, int j, int c) const { return lds[(uint32_t)c * ATROUS_LDS_PLANE + at(i, j)]; }
  __device__ double variance(int i, int j, int c) const { return lds[(uint32_t)(3 + c) * ATROUS_LDS_PLANE + at(i, j)]; }
  __device__ double guide(int i, int j, uint32_t k) const { return lds[(6 + k) * ATROUS_LDS_PLANE + at(i, j)]; }
};

// The definition above for pixel (x, y) of the image, statement for statement.
template <class Taps>
__device__ void atrous_pixel(const AtrousPass &A, const Taps &T, uint32_t x, uint32_t y) {
  const double h[5] = {1.0 / 16.0, 1.0 / 4.0, 3.0 / 8.0, 1.0 / 4.0, 1.0 / 16.0};
  double cp[3], gp[ATROUS_MAX_GUIDES];
  for (int c = 0; c < 3; c++) cp[c] = T.color(0, 0, c);
  const double vsum_p = (T.variance(0, 0, 0) + T.variance(0, 0, 1)) + T.variance(0, 0, 2);
#pragma unroll
  for (uint32_t k = 0; k < ATROUS_MAX_GUIDES; k++) gp[k] = k < A.G ? T.guide(0, 0, k) : 0.0;
  double sw = 0.0, ac[3] = {0.0, 0.0, 0.0}, av[3] = {0.0, 0.0, 0.0};
  for (int j = -2; j <= 2; j++) {
    const int64_t qy = (int64_t)y + (int64_t)j * (int64_t)A.step;
    if (qy < 0 || qy >= (int64_t)A.H) continue;
    for (int i = -2; i <= 2; i++) {
      const int64_t qx = (int64_t)x + (int64_t)i * (int64_t)A.step;
      if (qx < 0 || qx >= (int64_t)A.W) continue;
      double cq[3], vq[3];
      for (int c = 0; c < 3; c++) cq[c] = T.color(i, j, c), vq[c] = T.variance(i, j, c);
      const double d0 = cp[0] - cq[0], d1 = cp[1] - cq[1], d2c = cp[2] - cq[2];
      const double d2 = (d0 * d0 + d1 * d1) + d2c * d2c;
      const double vsum_q = (vq[0] + vq[1]) + vq[2];
      const double D = A.color_sigma2 * (vsum_p + vsum_q) + A.variance_floor;
      double xg = 0.0;
#pragma unroll
      for (uint32_t k = 0; k < ATROUS_MAX_GUIDES; k++)
        if (k < A.G) {
          const double e = (gp[k] - T.guide(i, j, k)) * A.guide_inv_sigma[k];
          xg = xg + e * e;
        }
      const double w = ((h[j + 2] * h[i + 2]) * D) / ((D + d2) * (1.0 + xg));
      const double ww = w * w;
      sw = sw + w;
      for (int c = 0; c < 3; c++) ac[c] = ac[c] + w * cq[c], av[c] = av[c] + ww * vq[c];
    }
  }
  const size_t o = ((size_t)y * A.W + x) * 3;
  for (int c = 0; c < 3; c++) A.out_color[o + c] = ac[c] / sw;
  if (A.out_variance) {
    const double sw2 = sw * sw;
    for (int c = 0; c < 3; c++) A.out_variance[o + c] = av[c] / sw2;
  }
}

// 256 lanes = one 32 x 8 tile of one lattice (atrous_tiling), grid-stride over the tiles.  LDS: the tile's lattice points and their halo are
// staged first, as far as they lie inside the image (the taps outside are skipped, so what is not staged is not read).
template <bool LDS>
__global__ void RL_KERNEL_ALIGN __launch_bounds__(ATROUS_NT) atrous_pass_kernel(const AtrousPass A) {
  extern __shared__ double atrous_lds[];
  const uint32_t lx = threadIdx.x % ATROUS_TILE_W, ly = threadIdx.x / ATROUS_TILE_W;
  const uint32_t s = LDS ? A.step : 1;
  for (uint64_t t = blockIdx.x; t < A.tiles; t += gridDim.x) {
    const uint32_t tx = (uint32_t)(t % A.tiles_x), ty = (uint32_t)(t / A.tiles_x % A.tiles_y);
    const uint64_t phase = t / A.tiles_x / A.tiles_y;
    const uint32_t phx = (uint32_t)(phase % A.phases_x), phy = (uint32_t)(phase / A.phases_x);
    // lattice point (u, v) is pixel (phx + u*s, phy + v*s); this lattice has nu x nv points inside the image
    const uint64_t x = phx + (uint64_t)(tx * ATROUS_TILE_W + lx) * s, y = phy + (uint64_t)(ty * ATROUS_TILE_H + ly) * s;
    const bool live = x < A.W && y < A.H;
    if constexpr (LDS) {
      const int64_t nu = ((int64_t)A.W - phx + s - 1) / s, nv = ((int64_t)A.H - phy + s - 1) / s;
      const int64_t u0 = (int64_t)tx * ATROUS_TILE_W - 2, v0 = (int64_t)ty * ATROUS_TILE_H - 2;
      const int64_t us = u0 < 0 ? 0 : u0, vs = v0 < 0 ? 0 : v0;
      const int64_t ue = u0 + ATROUS_LDS_W < nu ? u0 + ATROUS_LDS_W : nu, ve = v0 + ATROUS_LDS_H < nv ? v0 + ATROUS_LDS_H : nv;
      const uint32_t nx = ue > us ? (uint32_t)(ue - us) : 0, ny = ve > vs ? (uint32_t)(ve - vs) : 0;
      const uint32_t base = (uint32_t)(vs - v0) * ATROUS_LDS_W + (uint32_t)(us - u0);
      for (uint32_t e = threadIdx.x; e < ny * nx * 3; e += ATROUS_NT) {
        const uint32_t r = e / (nx * 3), in_row = e % (nx * 3), pu = in_row / 3, c = in_row % 3;
        const size_t g = ((size_t)(phy + (uint64_t)(vs + r) * s) * A.W + (size_t)(phx + (uint64_t)(us + pu) * s)) * 3 + c;
        const uint32_t l = base + r * ATROUS_LDS_W + pu;
        atrous_lds[c * ATROUS_LDS_PLANE + l] = A.color[g];
        atrous_lds[(3 + c) * ATROUS_LDS_PLANE + l] = A.variance[g];
      }
      for (uint32_t e = threadIdx.x; e < ny * nx * A.G; e += ATROUS_NT) {
        const uint32_t r = e / (nx * A.G), in_row = e % (nx * A.G), pu = in_row / A.G, k = in_row % A.G;
        const size_t g = ((size_t)(phy + (uint64_t)(vs + r) * s) * A.W + (size_t)(phx + (uint64_t)(us + pu) * s)) * A.G + k;
        atrous_lds[(6 + k) * ATROUS_LDS_PLANE + base + r * ATROUS_LDS_W + pu] = A.guides[g];
      }
      __syncthreads();
      if (live) atrous_pixel(A, AtrousLdsTaps{atrous_lds, (ly + 2) * ATROUS_LDS_W + lx + 2}, (uint32_t)x, (uint32_t)y);
      __syncthreads();  // the next tile's staging overwrites what this one's taps read
    } else {
      if (live) atrous_pixel(A, AtrousImageTaps{A, (int64_t)(y * A.W + x)}, (uint32_t)x, (uint32_t)y);
    }
  }
}

// rl_debug_set_denoise_route: -1 the default (atrous_route_lds), 0 always the images, 1 always LDS (tests, tools/denoise_ab.py)
int g_denoise_route = -1;
std::atomic<int> g_last_denoise_route{-1};  // rl_debug_last_denoise_route: 0 images / 1 LDS of the most recent pass; -1 none yet

// Does the LDS route serve this pass?  By default always: at 1920 x 1080 with eight guides it took 0.30 - 0.35 ms at step 1 .. 16 where the
// images route took 1.14 - 1.18 ms (profiles/denoise.json).
bool atrous_route_lds() { return g_denoise_route != 0; }

// rl_debug_set_denoise_blocks: 0 the default (the CU-derived cap of the route), else the most workgroups a pass launches, so that tests
// put several tiles, or all of them, through one workgroup's grid-stride loop
std::atomic<uint32_t> g_denoise_max_blocks{0};
std::atomic<uint64_t> g_last_denoise_tiles{0}, g_last_denoise_blocks{0};  // rl_debug_last_denoise_launch: of the most recent pass; 0, 0 none yet

bool atrous_number_ok(double v) { return std::isfinite(v) && v >= 0.0; }

// What the struct itself must satisfy (also asked by rl_denoise_render*, rl_denoise_render.h): RL_OK or RL_E_INVALID.
int atrous_params_check(const rl_atrous_params *p) {
  if (p->n_guides > ATROUS_MAX_GUIDES || p->reserved != 0) return set_err(RL_E_INVALID, "n_guides beyond 8, or reserved not 0");
  // a subnormal floor can leave the centre tap's 9/64 * D at 0 (5e-324 on a flat image without variance: sw = 0, every output 0 / 0)
  if (!atrous_number_ok(p->color_sigma2) || !atrous_number_ok(p->variance_floor) || !(p->variance_floor >= std::numeric_limits<double>::min()))
    return set_err(RL_E_INVALID, "color_sigma2 must be finite and >= 0, variance_floor finite and a normal number (>= DBL_MIN)");
  for (uint32_t k = 0; k < p->n_guides; k++)
    if (!atrous_number_ok(p->guide_inv_sigma[k])) return set_err(RL_E_INVALID, "guide_inv_sigma must be finite and >= 0");
  return RL_OK;
}

// The argument rules of both entry points, looked at before the device: RL_OK or RL_E_INVALID.
int atrous_check(uint32_t width, uint32_t height, const rl_atrous_params *p, const void *color, const void *variance, const void *guides, const void *out_color,
                 const void *out_variance) {
  if (!p || !color || !variance || !out_color) return set_err(RL_E_INVALID, "bad argument");
  if (int rc = atrous_params_check(p); rc != RL_OK) return rc;
  if (p->n_guides != 0 && !guides) return set_err(RL_E_INVALID, "bad argument");
  const void *ins[3] = {color, variance, p->n_guides ? guides : nullptr}, *outs[2] = {out_color, out_variance};
  for (const void *o : outs)
    for (const void *i : ins)
      if (o && o == i) return set_err(RL_E_INVALID, "an output is an input: a pass is not in place");
  if (out_color == out_variance) return set_err(RL_E_INVALID, "the two outputs are one buffer");
  if ((uint64_t)width * height >= PIXEL_LIST_MAX_N) return set_err(RL_E_INVALID, "image too large");
  return RL_OK;
}
}  // namespace

extern "C" {

void rl_debug_set_denoise_route(int route) { g_denoise_route = route < 0 ? -1 : (route != 0); }
int rl_debug_last_denoise_route(void) { return g_last_denoise_route.load(); }
void rl_debug_set_denoise_blocks(uint32_t max_blocks) { g_denoise_max_blocks = max_blocks; }
void rl_debug_last_denoise_launch(uint64_t out[2]) {
  if (out) out[0] = g_last_denoise_tiles.load(), out[1] = g_last_denoise_blocks.load();
}

int rl_denoise_atrous_pass_device(uint32_t width, uint32_t height, uint32_t step, const rl_atrous_params *p, const void *d_color, const void *d_variance,
                                  const void *d_guides, void *d_out_color, void *d_out_variance, void *hip_stream) {
  int rc = atrous_check(width, height, p, d_color, d_variance, d_guides, d_out_color, d_out_variance);
  if (rc != RL_OK) return rc;
  if (step == 0 || step > ATROUS_MAX_STEP) return set_err(RL_E_INVALID, "step must be 1 .. 1 << 20");
  if (!g_ready) return set_err(RL_E_NO_DEVICE, "rl_init has not succeeded");
  if (width == 0 || height == 0) return RL_OK;
  AtrousPass A{};
  A.W = width, A.H = height, A.step = step, A.G = p->n_guides;
  A.color_sigma2 = p->color_sigma2, A.variance_floor = p->variance_floor;
  for (uint32_t k = 0; k < A.G; k++) A.guide_inv_sigma[k] = p->guide_inv_sigma[k];
  A.color = (const double *)d_color, A.variance = (const double *)d_variance, A.guides = A.G ? (const double *)d_guides : nullptr;
  A.out_color = (double *)d_out_color, A.out_variance = (double *)d_out_variance;
  const bool lds_route = atrous_route_lds();
  atrous_tiling(A, lds_route);
  const size_t lds = lds_route ? (size_t)ATROUS_LDS_PLANE * (6 + A.G) * sizeof(double) : 0;  // at most 48,384 bytes: no attribute to raise
  void (*kern)(const AtrousPass) = lds_route ? atrous_pass_kernel<true> : atrous_pass_kernel<false>;
  const uint64_t per_cu = lds_route ? std::min<size_t>(g_lds_max / lds, ATROUS_MAX_BLOCKS_PER_CU) : ATROUS_MAX_BLOCKS_PER_CU;
  const uint32_t max_blocks = g_denoise_max_blocks.load();
  const uint64_t cap = max_blocks ? max_blocks : (uint64_t)std::max(1, g_cus) * per_cu;
  const uint64_t blocks = std::min(A.tiles, cap);
  hipLaunchKernelGGL(kern, dim3((uint32_t)blocks), dim3(ATROUS_NT), lds, (hipStream_t)hip_stream, A);
  HIP_TRY(hipGetLastError());
  g_last_denoise_route = lds_route ? 1 : 0;
  g_last_denoise_tiles = A.tiles, g_last_denoise_blocks = blocks;
  return RL_OK;
}

int rl_denoise_atrous(uint32_t width, uint32_t height, uint32_t iterations, const rl_atrous_params *p, const double *color, const double *variance,
                      const double *guides, double *out_color, double *out_variance) {
  int rc = atrous_check(width, height, p, color, variance, guides, out_color, out_variance);
  if (rc != RL_OK) return rc;
  if (iterations > ATROUS_MAX_ITERATIONS) return set_err(RL_E_INVALID, "iterations beyond 12");
  if (!g_ready) return set_err(RL_E_NO_DEVICE, "rl_init has not succeeded");
  const size_t npix = (size_t)width * height, bytes = npix * 3 * sizeof(double);
  if (npix == 0) return RL_OK;
  if (iterations == 0) {
    std::memcpy(out_color, color, bytes);
    if (out_variance) std::memcpy(out_variance, variance, bytes);
    return RL_OK;
  }
  HostStaging q(nullptr);
  struct Pair {
    void *color, *variance;
  } src{q.in(color, bytes), q.in(variance, bytes)}, work[2] = {{nullptr, nullptr}, {nullptr, nullptr}};
  void *d_guides = p->n_guides ? q.in(guides, npix * p->n_guides * sizeof(double)) : nullptr;
  for (uint32_t i = 0; i < std::min(iterations, 2u); i++) work[i] = {q.scratch(bytes), q.scratch(bytes)};
  if (q.rc != RL_OK) return q.rc;
  Pair dst = src;
  for (uint32_t it = 0; it < iterations; it++) {  // step = 1, 2, .., 2^(iterations - 1), ping-pong between the two staged pairs
    dst = work[it & 1];
    if (it + 1 == iterations && !out_variance) dst.variance = nullptr;  // the last pass: nothing reads its variance
    rc = rl_denoise_atrous_pass_device(width, height, 1u << it, p, src.color, src.variance, d_guides, dst.color, dst.variance, q.stream);
    if (rc != RL_OK) return rc;
    src = dst;
  }
  HIP_TRY(hipStreamSynchronize(q.stream));  // the copies back run on the null stream, which the library's stream does not wait for
  q.back(out_color, dst.color, bytes), q.back(out_variance, dst.variance, bytes);
  return q.finish(RL_OK);
}

}  // extern "C"
