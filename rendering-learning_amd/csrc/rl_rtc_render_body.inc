  // The body of rtc_kernel / rtc_pixels_kernel (rl_rtc_kernel.h): included inside both, with LIST, xs, ys, n_list (and the kernel's template
  // parameters) in scope.  Textual, not a function: the frame kernel compiles to the code it compiled to before the list flavour existed.
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x;
  const DevOp *ops = P.ops;
  const DevTri *tris = P.tris;
  const RtcGuard *guards = P.guards;
  if (LDS_SCENE) {
    DevOp *s_ops = (DevOp *)smem;
    DevTri *s_tris = (DevTri *)(s_ops + P.n_ops);
    const uint4 *g = (const uint4 *)P.ops;
    uint4 *l = (uint4 *)s_ops;
    for (uint32_t i = tid; i < P.n_ops * 4u; i += NT) l[i] = g[i];
    g = (const uint4 *)P.tris;
    l = (uint4 *)s_tris;
    for (uint32_t i = tid; i < P.n_tris * 10u; i += NT) l[i] = g[i];
    if (guards) {
      RtcGuard *s_guards = (RtcGuard *)(s_tris + P.n_tris);
      g = (const uint4 *)P.guards;
      l = (uint4 *)s_guards;
      for (uint32_t i = tid; i < P.n_guards * 2u; i += NT) l[i] = g[i];
      guards = s_guards;
    }
    __syncthreads();
    ops = s_ops;
    tris = s_tris;
  }
  const rl_rtc_camera &cam = P.cam;
  const uint32_t W = cam.hsize;
  RtcCounters cnt{0, 0, 0, 0, 0};
  const double INF = __longlong_as_double(0x7FF0000000000000ll);
  const uint64_t total = LIST ? n_list : (uint64_t)W * P.nrows;
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
      for (uint32_t ny = 0; ny < P.aa; ny++) {  // camera.rs:71-88
        double sample_offset = 1.0 / (double)P.aa;
        double xoffset = ((double)px + sample_offset * ((double)nx + 0.5)) * cam.pixel_size;
        double yoffset = ((double)py + sample_offset * ((double)ny + 0.5)) * cam.pixel_size;
        double world_x = cam.half_width - xoffset;
        double world_y = cam.half_height - yoffset;
        D3 pixel = mul_point(cam.inverse, d3(world_x, world_y, -1.0));
        D3 origin = mul_point(cam.inverse, d3(0.0, 0.0, 0.0));
        D3 dir;
        if (!norm(pixel - origin, dir)) {
          cnt.flagged++;
          dir = d3(0.0, 0.0, 0.0);
        }
        // World::color_at -> color_at_internal (world.rs:89-102)
        cnt.rays++;
        RtcHit best{INF, NONE, 0u, d3(0.0, 0.0, 0.0)};
        rtc_traverse<false>(P, ops, tris, guards, origin, dir, 0.0, best, cnt);
        D3 c = ld3(P.void_color);
        if (best.tri != NONE && P.n_lights > 0) {
          // prepare_computations (intersect.rs:48-71)
          const DevTri &tr = tris[best.tri];
          const rl_rtc_material &m = P.materials[tr.material];
          D3 point = origin + dir * best.t;
          D3 eye_v;
          if (!norm(-dir, eye_v)) {
            cnt.flagged++;
            eye_v = -dir;
          }
          D3 normal_v = best.normal;
          if (dot(normal_v, eye_v) < 0.0) normal_v = -normal_v;
          D3 over_point = point + normal_v * 1e-5;
          D3 object_color = ld3(m.color);
          D3 lsum = d3(0.0, 0.0, 0.0);
          for (uint32_t li = 0; li < P.n_lights; li++) {  // shade_hit (world.rs:57-87)
            const rl_rtc_light &light = P.lights[li];
            D3 lpos = ld3(light.position), intensity = ld3(light.intensity);
            // shadow_attenuation (world.rs:104-126)
            D3 v = lpos - over_point;
            double distance = mag(v);
            D3 sdir;
            double shadow_att = 1.0;
            if (norm(v, sdir)) {
              cnt.rays++;
              RtcHit dummy{INF, NONE, 0u, d3(0.0, 0.0, 0.0)};
              shadow_att = rtc_traverse<true>(P, ops, tris, guards, over_point, sdir, distance, dummy, cnt);
            }
            D3 surface = rtc_lighting(m, point, object_color, lpos, intensity, eye_v, normal_v, shadow_att);
            // reflectivity == transparency == 0 on this path: surface + (black + black)
            D3 col = surface + (d3(0.0, 0.0, 0.0) + d3(0.0, 0.0, 0.0));
            lsum = (li == 0) ? col : lsum + col;
          }
          c = lsum;
        }
        acc = have ? acc + c : c;
        have = true;
      }
    D3 res = acc * (1.0 / (double)((uint64_t)P.aa * P.aa));
    double *outp = P.out + idx * 3;
    outp[0] = res.x, outp[1] = res.y, outp[2] = res.z;
  }
  unsigned long long v;
  v = wave_sum(cnt.rays);
  if ((tid & 63) == 0) atomicAdd(&P.stats[0], v);
  v = wave_sum(cnt.nodes);
  if ((tid & 63) == 0) atomicAdd(&P.stats[1], v);
  v = wave_sum(cnt.tris);
  if ((tid & 63) == 0) atomicAdd(&P.stats[3], v);
  v = wave_sum(cnt.enters);
  if ((tid & 63) == 0) atomicAdd(&P.stats[4], v);
  v = wave_sum(cnt.flagged);
  if ((tid & 63) == 0 && v) atomicAdd(&P.stats[6], v);
