  // The body of rtiow_wave_kernel / rtiow_wave_indep_kernel / rtiow_wave_moments_kernel (rl_rtiow_wave.h): included inside all three, with
  // INDEP and MOMENTS (and the kernel's template parameters) in scope.
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x;
  // LDS layout: [linked ops][spheres][ChaCha rings 16 x NT u64]; with the scene in HBM the rings start at 0
  const size_t bits_words = ((size_t)P.n_spheres + 31) / 32 + 1;
  const size_t scene_lds = LDS_SCENE == 4   ? (((size_t)P.n_fast_inner * sizeof(FastNodeCH) + 2 * bits_words * sizeof(uint32_t) + 15) & ~(size_t)15)
                           : LDS_SCENE == 3 ? (((size_t)P.n_cops * sizeof(CompactOp) + bits_words * sizeof(uint32_t) + 15) & ~(size_t)15)
                           : LDS_SCENE      ? ((size_t)P.n_ops * sizeof(DevOp) + (LDS_SCENE == 1 ? (size_t)P.n_spheres * sizeof(DevSphere) : 0))
                                            : 0;
  unsigned long long *s_rng = (unsigned long long *)(smem + scene_lds);  // [16][NT]
  const unsigned char *opbase = (const unsigned char *)P.lops;  // pc is an index (HBM) or a byte offset (LDS) into this
  const DevSphere *spheres = P.spheres;
  const uint32_t *s_bits = nullptr;  // LDS_SCENE == 3: one bit per sphere (Center::Moving)
  const uint32_t lds_base = (uint32_t)(uintptr_t)smem;  // the dynamic LDS segment's own address (low half of the flat address)
  if (LDS_SCENE == 4) {
    const uint4 *g = (const uint4 *)P.fast_nodes_ch;
    uint4 *l = (uint4 *)smem;
    for (uint32_t i = tid; i < P.n_fast_inner * 4u; i += NT) l[i] = g[i];
    uint32_t *bl = (uint32_t *)(smem + (size_t)P.n_fast_inner * sizeof(FastNodeCH));
    for (uint32_t i = tid; i < 2u * (uint32_t)bits_words; i += NT) bl[i] = P.movbits[i];  // [moving bits][specular-material bits]
    __syncthreads();
    opbase = smem;
    s_bits = bl;
  } else if (LDS_SCENE == 3) {
    const uint4 *g = (const uint4 *)P.cops;
    uint4 *l = (uint4 *)smem;
    for (uint32_t i = tid; i < P.n_cops * 2u; i += NT) {
      uint4 v = g[i];
      if (i & 1u) {  // {box[4], box[5], w_hit, w_miss}: successor indices -> absolute LDS addresses (no add per step)
        v.z = (v.z & 0xE0000000u) | (((v.z & 0x1FFFFFFFu) << 5) + lds_base);
        v.w = (v.w & 0xE0000000u) | (((v.w & 0x1FFFFFFFu) << 5) + lds_base);
      }
      l[i] = v;
    }
    uint32_t *bl = (uint32_t *)(smem + (size_t)P.n_cops * sizeof(CompactOp));
    for (uint32_t i = tid; i < (uint32_t)bits_words; i += NT) bl[i] = P.movbits[i];
    __syncthreads();
    opbase = smem;
    s_bits = bl;
  } else if (LDS_SCENE) {
    DevOp *s_ops = (DevOp *)smem;
    DevSphere *s_sph = (DevSphere *)(s_ops + P.n_ops);
    const uint4 *g = (const uint4 *)P.lops;
    uint4 *l = (uint4 *)s_ops;
    for (uint32_t i = tid; i < P.n_ops * 4u; i += NT) {
      uint4 v = g[i];
      if ((i & 3u) == 3u) {  // {w_hit, w_miss, a, b}: successor indices -> LDS byte offsets
        v.x = (v.x & 0xE0000000u) | ((v.x & 0x1FFFFFFFu) << 6);
        v.y = (v.y & 0xE0000000u) | ((v.y & 0x1FFFFFFFu) << 6);
        l[i] = v;
      }
    }
    // the box, re-stored as six floats in the first 24 bytes of the op (the binary64 box stays in HBM for the exact path)
    for (uint32_t i = tid; i < P.n_ops; i += NT) {
      const double *bx = P.lops[i].box;
      float *f = (float *)(s_ops + i);
#pragma unroll
      for (int k = 0; k < 6; k++) f[k] = (float)bx[k];
    }
    if (LDS_SCENE == 1) {
      g = (const uint4 *)P.spheres;
      l = (uint4 *)s_sph;
      for (uint32_t i = tid; i < P.n_spheres * 4u; i += NT) l[i] = g[i];
      spheres = s_sph;
    }
    __syncthreads();
    opbase = smem;
  }
  const uint32_t entry0 = LDS_SCENE == 4   ? 0u  // fast traversal: rays start through fast_start()
                          : LDS_SCENE == 3 ? ((P.centry0 & 0xE0000000u) | (((P.centry0 & 0x1FFFFFFFu) << 5) + lds_base))
                          : LDS_SCENE  ? ((P.entry0 & 0xE0000000u) | ((P.entry0 & 0x1FFFFFFFu) << 6))
                                       : P.entry0;
  const rl_rtiow_camera &cam = P.cam;
  const uint32_t W = cam.image_width;
  const uint32_t s_begin = P.sample_begin, spp = P.sample_end;  // this launch renders samples [s_begin, spp) of every pixel
  const uint64_t WH = (uint64_t)cam.image_width * (uint64_t)cam.image_height;
  const double INF = __longlong_as_double(0x7FF0000000000000ll);

  // ---- per-lane persistent state
  // (the stealing instantiation keeps the unrolled block function on its hot paths: measured, 1/8 and 1/4 shard 170 / 263 ms against 163 / 283 rolled)
  // (the moments kernel with the scene in global memory keeps lane-per-block passes and the per-lane FILL: with the four-lanes-per-block
  // pass in it, it spills a VGPR, 8 bytes of scratch, where it spilled none)
  constexpr bool COOP_QUAD = !(MOMENTS && LDS_SCENE == 0);
  Ring<NT, !STEAL, false, COOP_QUAD> rng{P.key, s_rng, tid, 0ull, 0u, 0u, 0u};
  uint32_t state = ST_GEN;
  uint32_t px = 0, pr = 0, n = spp;  // n == spp: no pixel owned yet
  uint32_t n_end = spp;              // INDEP: end of the lane's sample group
  uint32_t ptile = 0, pix_rays = 0;
  bool have_pixel = false;
  D3 sum = d3(0.0, 0.0, 0.0);
  D3 sq = d3(0.0, 0.0, 0.0);  // MOMENTS: per channel the sum of the squared sample colours (each product rounded, then added), beside sum
  D3 o = d3(0.0, 0.0, 0.0), d = d3(0.0, 0.0, 1.0), thr = d3(1.0, 1.0, 1.0);
  RayAux ra = ray_aux(o, d);
  RayAux32 ra32 = ray_aux32(ra);
  double time = 0.0, closest = INF;
  uint32_t pc = 0, hit_prim = NONE, depth = 0;
  // fast traversal: depth carries, in its top ten bits, the entry id of the sphere the ray has just left when fast_self_miss proved that the
  // ray's own LEAF visit would accept nothing (FAST_NONE otherwise, and for camera rays); the remaining depth sits in the low 22 bits
  // (the host runs variant 1029 for max_depth < 2^22 only).  The budget is 128 VGPRs (one more costs a wave per SIMD); the headline kernel uses 119.
  constexpr uint32_t DEPTH_MASK = LDS_SCENE == 4 ? FAST_DEPTH_MASK : ~0u;
  uint32_t c_rays = 0, c_flag = 0, c_slow = 0;  // c_slow: rays the fast traversal handed to the reference-order fold
  unsigned long long c_nodes = 0, c_sph = 0, c_words = 0, c_self = 0;  // c_self (STATS): self tests skipped
  // STATS census (tools/sched.py): the camera rays' share — a camera ray is the one whose remaining depth is still cam.max_depth
  // c_cam_miss: those of their LEAF visits that return at the discriminant test (disc < 0) — a sphere whose box the ray passed but not the sphere
  unsigned long long c_cam_trav = 0, c_cam_leaf = 0, c_cam_rays = 0, c_cam_miss = 0;
  // ... split: on a moving sphere; on a moving / a stationary sphere that the all-times entry table holds for the pixel (the others lie below an
  // entry without being in its leaf set); and of the moving ones in the table, those the ball of the sample's time slice excludes, T = 2, 4, 8
  unsigned long long c_cam_miss_mov = 0, c_cam_miss_mov_tab = 0, c_cam_miss_sta_tab = 0, c_cam_miss_cut[3] = {0, 0, 0};

  // fast traversal (LDS_SCENE = 4): 16 ten-bit entry ids in five registers, newest in the low bits of stk0; all ones = empty
  uint32_t stk0 = ~0u, stk1 = ~0u, stk2 = ~0u, stk3 = ~0u, stk4 = ~0u;
  bool amb = false;  // this ray must be re-traced in the reference's order
  auto fast_push = [&](uint32_t e) {
    stk4 = __builtin_amdgcn_alignbit(stk4, stk3, 22), stk3 = __builtin_amdgcn_alignbit(stk3, stk2, 22);
    stk2 = __builtin_amdgcn_alignbit(stk2, stk1, 22), stk1 = __builtin_amdgcn_alignbit(stk1, stk0, 22);
    stk0 = (stk0 << 10) | e;
  };
  auto fast_pop = [&]() -> uint32_t {
    uint32_t e = stk0 & 1023u;
    stk0 = __builtin_amdgcn_alignbit(stk1, stk0, 10), stk1 = __builtin_amdgcn_alignbit(stk2, stk1, 10);
    stk2 = __builtin_amdgcn_alignbit(stk3, stk2, 10), stk3 = __builtin_amdgcn_alignbit(stk4, stk3, 10);
    stk4 = (stk4 >> 10) | (FAST_NONE << 22);
    return e;
  };
  // measured and lost (kept switchable): a separate block for Metal / Dielectric hits shortens SHADE (35.7 % -> 23.3 + 5.2 % of the
  // wave time) but a sixth state thins every other block (TRAV population 21.2 -> 18.5, LEAF 30.8 -> 27.0): 6.14 -> 5.52 Grays/s
  constexpr bool SPLIT_SHADE = false;
  // SPLIT_LEAF (fast traversal): LEAF only evaluates the discriminant — a sphere whose box the ray passed but which it misses (about half of
  // the visits) sends the lane straight back to TRAV — and the roots, the tie band and the order checks of an actual hit run in LEAF2.
  // Measured (round 3, -DRL_SPLIT_LEAF=true): 6709 -> 5907 Mrays/s, 1/8 shard 173 -> 205 ms — like SPLIT_SHADE, one more scheduling class
  // costs more in population per block than the shorter blocks give back (tools/sched.py: LEAF is 32 % of the time at 35 lanes per block)
  constexpr bool SPLIT_LEAF = RL_SPLIT_LEAF;
  // shade() writes the next ray over the old one before it knows whether the path goes on (see there).  The fast kernels only: the
  // reference-order layouts gain nothing (the counting instantiation's SHADE pick path reads 509 -> 824 instructions, 94 -> 102 spilled SGPRs)
  constexpr bool SHADE_RAY_IN_PLACE = LDS_SCENE == 4;
  constexpr int SHADE_TRIES = RL_SHADE_TRIES;  // rl_rtiow_wave.h
  auto shade_state = [&]() -> uint32_t {  // where a finished traversal is shaded
    if (!SPLIT_SHADE || LDS_SCENE != 4 || hit_prim == NONE) return ST_SHADE;
    const uint32_t si = hit_prim & SPH_INDEX;
    return ((s_bits[bits_words + (si >> 5)] >> (si & 31u)) & 1u) ? ST_SHADE2 : ST_SHADE;
  };
  auto fast_go = [&](uint32_t e) {  // continue with entry e: an inner node (TRAV), a sphere (LEAF), or nothing left
    const bool end = e == FAST_NONE;
#ifdef RL_FASTG_VERIFY
    if (LDS_SCENE == 4 && end && !amb) {  // a walk that trusts its own answer: the reference's fold must give the same one
      fast_verify_ray(P.ops, spheres, o, d, time, closest, hit_prim, 2.0);
      atomicAdd(&g_vstats[3], 1ull);
    }
#endif
    // State and pc are selects, not branches: no divergent region is left in a TRAV step after the push and the pop.  A walk that ends
    // with a hit leaves pc = FAST_NONE behind, which nothing reads: SHADE and FILL do not look at pc, and GEN only for FAST_MISSED.
    // A miss needs no SHADE visit (+10 %), and no work here either: the lane goes to GEN in every case, where a sample ends anyway, and
    // GEN adds the background and counts the sample when it finds the marker.  Resolved here, the three products of thr * background are
    // hoisted into every TRAV pick's preamble and the adds sit in a nest of exec-mask regions inside the step (DESIGN.md section 3.1)
    const bool leaf = e >= P.n_fast_inner, miss = hit_prim == NONE, settled = end && !amb;
    const uint32_t st_hit = SPLIT_SHADE && settled && !miss ? shade_state() : ST_SHADE;
    pc = settled ? (miss ? FAST_MISSED : e) : end ? FAST_SLOW : leaf ? e : lds_base + (e << 6);
    state = settled ? (miss ? ST_GEN : st_hit) : leaf ? ST_LEAF : ST_TRAV;
  };
  // w (fast traversal): where the walk starts — up to three entry ids, the first one in the low ten bits, FAST_NONE in the unused slots,
  // the top two bits set.  fast_root_word for a scattered ray; a camera ray takes its pixel's word of P.pixel_entry (rl_pixel_entry.h)
  const uint32_t fast_root_word = P.fast_root | ~1023u;
  auto start_ray = [&](uint32_t w) {  // o, d set: per-ray constants of the box filter, then the first traversal state
    closest = INF, hit_prim = NONE;
    if (LDS_SCENE == 4) ra32 = ray_aux32_direct(o, d);
    else {
      ra = ray_aux(o, d);
      if (!ra.fast_ok) ra.slack = INF;
      ra32 = ray_aux32(ra);
    }
    if (LDS_SCENE == 4) {
      stk0 = (w >> 10) | (FAST_NONE << 22), stk1 = stk2 = stk3 = stk4 = ~0u;
      amb = !(ra32.slack < __int_as_float(0x7F800000));  // outside the binary32 filter's range: the reference's order from the start
      fast_go(amb ? FAST_NONE : w & 1023u);
    } else {
      pc = entry0 & 0x1FFFFFFFu;
      state = entry0 >> 29;
    }
  };

  // SHADE: miss -> background; hit -> rebuild the HitRecord, scatter, next ray.  MODE 0 = every material (reference-order kernels),
  // 1 = everything but Metal / Dielectric, 2 = Metal / Dielectric only (ST_SHADE2): the fast kernel's two halves
  // (the generic statement of Material::scatter is rl_rtiow_scatter.h; this one stays its own: flattened sphere records, hoisted us / vn, the SHADE2 split)
  auto shade = [&](auto mode) {
    constexpr int MODE = decltype(mode)::value;
        bool path_done = false;
        D3 nd = d;
        D3 p = o;
        if (MODE != 2 && hit_prim == NONE) {  // miss -> background (camera.rs:257)
          if constexpr (MOMENTS) {
            const D3 c = thr * ld3(cam.background);
            sum = sum + c;
            sq = sq + c * c;
          } else sum = sum + thr * ld3(cam.background);
          path_done = true;
        } else {
          uint32_t si = hit_prim & SPH_INDEX;
          const DevSphere &s = spheres[si];
          D3 c0 = ld3(s.c0);
          D3 center = (hit_prim & SPH_MOVING) ? c0 + ld3(s.dc) * time : c0;
          p = o + d * closest;
          D3 outward = (p - center) * s.inv_r;
          bool front = dot(d, outward) <= 0.0;
          D3 normal = front ? outward : -outward;
          // one flattened record per sphere (rl_scene_host.cpp flatten_sphere_materials): the material with a Solid texture's
          // colour inlined, and for a Dielectric the constants 1/ior and Schlick's r0 of both orientations — one load
          // instead of the sphere -> material -> texture chain, same values bit for bit
          const DevMaterial &m = P.sphere_flat[si];
          // ... and, for a Checker of two Solid colours, the odd colour and inv_scale from the sphere's own record beside it (the even
          // colour is in albedo): addressed by sphere index alone; apply_texture below is what makes it one round of loads with the material's
          const DevChecker &ck = P.sphere_checker[si];
          const uint32_t kind = m.kind & 0xFFu;
          const bool solid = (m.kind & MAT_TEX_SOLID) != 0u, checker = (m.kind & MAT_TEX_CHECKER) != 0u;
          // shared sub-expressions, evaluated once per block instead of once per material branch (same values, same
          // RNG order: the unit-sphere draw is the first draw of both Lambertian and Metal scatter)
          const bool is_lamb = MODE != 2 && kind == RL_MAT_LAMBERTIAN, is_metal = MODE != 1 && kind == RL_MAT_METAL, is_diel = MODE != 1 && kind == RL_MAT_DIELECTRIC;
          const bool is_light = MODE != 2 && kind == RL_MAT_DIFFUSE_LIGHT;
          // Texture::value at p, once for both materials that have a texture.  Solid: albedo.  Two-colour checker: texture_value's own
          // parity expression on the inlined inv_scale, then one of the two inlined colours, as they are.  Anything else (a nested
          // checker): the generic walk, a region no wave enters unless it has such a lane.
          // The records' fields are made values before the flag is looked at: the compiler issues a load where its value is used, i.e.
          // inside the region of the branch that needs it — albedo behind kind, inv_scale behind the checker flag, the odd colour behind
          // the parity: four rounds in series.  The empty asm makes each a value that exists here, so the loads stand beside kind's
          // and the one wait that kind needs anyway covers them.
          // The colour is used up at once — thr for Lambertian, sum for DiffuseLight: both apply it whatever the draw gives — so that
          // neither it nor the checker record is held through the rejection loop and normalize(): held to the material branches the
          // headline kernel takes 124 VGPRs, with the records' values held through the loop 128, instead of 118 (tools/wave_codegen.py).
          // (TEX_EARLY = false, the layouts that read the scene from global memory, LDS_SCENE = 0, for scenes too large for LDS: the
          // statements stay in the material branches, a Solid's colour inlined and every other texture walked, MAT_TEX_CHECKER ignored.
          // With this block those instantiations, which spill as they are, spill more: rtiow_wave_kernel<1024, 0, true> 18 VGPRs
          // instead of 6, tools/kernel_regs.py)
          constexpr bool TEX_EARLY = LDS_SCENE != 0;
          auto tex_late = [&] { return solid ? ld3(m.albedo) : texture_value(P, m.texture, 0.0, 0.0, p); };
          auto apply_texture = [&] {
            if (!TEX_EARLY) return;
            D3 texc = ld3(m.albedo), tex_odd = ld3(ck.odd);
            double inv_scale = ck.inv_scale;
            asm volatile("" : "+v"(texc.x), "+v"(texc.y), "+v"(texc.z), "+v"(tex_odd.x), "+v"(tex_odd.y), "+v"(tex_odd.z), "+v"(inv_scale));
            if (is_lamb | is_light) {
              if (checker) {
                const uint32_t odd = f64_as_i64_low_bit(floor(p.x * inv_scale)) ^ f64_as_i64_low_bit(floor(p.y * inv_scale)) ^
                                     f64_as_i64_low_bit(floor(p.z * inv_scale));
                if (odd) texc = tex_odd;
              } else if (!solid) texc = texture_value(P, m.texture, 0.0, 0.0, p);
              if (is_lamb) thr = thr * texc;
              else {
                if constexpr (MOMENTS) {
                  const D3 c = thr * texc;
                  sum = sum + c;
                  sq = sq + c * c;
                } else sum = sum + thr * texc;
              }
            }
          };
          // The unit-sphere draw, the first draw of both Lambertian and Metal scatter.  SHADE_TRIES > 0 (A/B): a lane that has not
          // accepted after that many tries leaves shade() here with nothing but rng.pos advanced — it stays in ST_SHADE and draws on
          // at its next SHADE pick (the rejected words are consumed, the loop is memoryless), passing rng.low() and FILL on the way.
          // Everything above it writes locals only, so the colour is then fetched and applied behind the draw: a second round of loads.
          if (SHADE_TRIES == 0) apply_texture();
          D3 us = d3(0.0, 0.0, 0.0);
          if (is_lamb | is_metal) {
            if constexpr (SHADE_TRIES > 0) {
              if (!rng.template unit_sphere_tries<SHADE_TRIES>(us)) return;
            } else us = rng.unit_sphere_tail();
          }
          if (SHADE_TRIES > 0) apply_texture();
          D3 reflected = d - normal * (2.0 * dot(d, normal));  // material.rs reflect(): used by Metal
          D3 vin = is_metal ? reflected : d;
          D3 vn = vin;
          double m2 = len2(vin);
          if (is_metal | is_diel) vn = div_s(vin, sqrt(m2));  // normalize(): vec3.rs:56
          if (is_lamb) {
            D3 dir = normal + us;
            bool near_zero = approx_eq_eps(dir.x, 0.0, 1e-8) && approx_eq_eps(dir.y, 0.0, 1e-8) && approx_eq_eps(dir.z, 0.0, 1e-8);
            nd = near_zero ? normal : dir;
            if (!TEX_EARLY) thr = thr * tex_late();  // (else thr has its texture colour already)
          } else if (is_metal) {
            nd = vn + us * m.fuzz;
            if (!(dot(nd, normal) > 0.0)) path_done = true;  // absorbed
            else thr = thr * ld3(m.albedo);
          } else if (is_diel) {
            double ri = front ? m.albedo[0] : m.ior;  // albedo[0] = 1.0 / ior
            D3 ud = vn;
            if (approx_eq_eps(m2, 0.0, 1e-16)) {
              c_flag++;
              ud = d;
            }
            double cos_theta = fmin(dot(-ud, normal), 1.0);
            double sin_theta = sqrt(1.0 - cos_theta * cos_theta);
            bool reflect = ri * sin_theta > 1.0;
            if (!reflect) {
              double r0 = front ? m.albedo[1] : m.albedo[2];  // ((1 - ri) / (1 + ri))^2 for ri = 1/ior and ri = ior
              double xx = 1.0 - cos_theta;
              double x2 = xx * xx;
              double refl = r0 + (1.0 - r0) * (xx * (x2 * x2));
              reflect = refl > rng.gen_f64();
            }
            if (reflect) nd = ud - normal * (2.0 * dot(ud, normal));
            else {
              D3 perp = (ud + normal * cos_theta) * ri;
              D3 par = normal * (-sqrt(fabs(1.0 - len2(perp))));
              nd = perp + par;
            }
          } else if (is_light) {
            if (!TEX_EARLY) {  // (else its emission is in sum already)
              if constexpr (MOMENTS) {
                const D3 c = thr * tex_late();
                sum = sum + c;
                sq = sq + c * c;
              } else sum = sum + thr * tex_late();
            }
            path_done = true;
          } else {
            path_done = true;  // Flat
          }
          // fast traversal: may the next ray skip its test of this sphere?  (decided for every hit: a path that ends here starts its
          // next sample in GEN, which clears the entry.)  The sphere is read again and its centre and oc = p - center re-derived — the
          // same expressions, the same values — instead of being held through the material code above (held, oc and r2 take the headline
          // kernel from 119 to 123 VGPRs and make SHADE's pick path longer, 779 -> 784 instructions with 18 more v_mov: tools/wave_codegen.py)
          if (LDS_SCENE == 4) {
            const DevSphere *sp = spheres + si;
            asm volatile("" : "+v"(sp));  // a fresh load, not the registers of the first one
            D3 c1 = ld3(sp->c0);
            if (hit_prim & SPH_MOVING) c1 = c1 + ld3(sp->dc) * time;
            depth = (depth & DEPTH_MASK) | ((fast_self_miss(*sp, p - c1, nd) ? P.n_fast_inner + si : FAST_NONE) << 22);
          }
        }
        if (!path_done) {
          depth--;
          if ((depth & DEPTH_MASK) == 0) path_done = true;  // ray_color(.., 0) = black
        }
        // The next ray is written over the old one whether the path goes on or not, so that the old one dies at its last use above and
        // the two are not both held through the material code.  A lane whose path ends here enters GEN, which sets o, d, thr, time and
        // depth before its start_ray; while it waits there inactive (a slot outside the image, no work left) it reads none of them; the
        // hand-over to a stealing wave stores sum, pos and n only.  For a miss shaded here p == o and nd == d.
        if (SHADE_RAY_IN_PLACE) o = p, d = nd;
        if (path_done) {
          n++;
          state = ST_GEN;
        } else {
          c_rays++;
          pix_rays++;
          if (!SHADE_RAY_IN_PLACE) o = p, d = nd;
          start_ray(fast_root_word);
        }
  };

  unsigned long long sc_exec[7] = {0, 0, 0, 0, 0, 0, 0}, sc_pop[7] = {0, 0, 0, 0, 0, 0, 0}, sc_cyc[7] = {0, 0, 0, 0, 0, 0, 0};
  unsigned long long sc_trav_picks = 0;  // STATS: scheduling decisions that chose TRAV (sc_exec[ST_TRAV] counts its steps)
  unsigned long long sc_pass[4] = {0, 0, 0, 0};  // STATS: block passes of Ring::coop_blocks: GEN's full / quad, FILL's full / quad
  for (;;) {
    RL_CG_MARK("HEAD");
    // a finished traversal goes to SHADE; lanes reading from their newest ChaCha block top the ring up first
    if ((state == ST_SHADE || (SPLIT_SHADE && LDS_SCENE == 4 && state == ST_SHADE2)) && rng.low()) state = ST_FILL;
    // ---- wave scheduler: run the state with the most lanes in it (ties -> TRAV, SHADE, FILL, GEN)
    int n_trav = __popcll(__ballot(state == ST_TRAV));
    int n_shade = __popcll(__ballot(state == ST_SHADE));
    int n_fill = __popcll(__ballot(state == ST_FILL));
    int n_gen = __popcll(__ballot(state == ST_GEN));
    int n_leaf = __popcll(__ballot(state == ST_LEAF));
    int n_shade2 = SPLIT_SHADE && LDS_SCENE == 4 ? __popcll(__ballot(state == ST_SHADE2)) : 0;
    int n_leaf2 = SPLIT_LEAF && LDS_SCENE == 4 ? __popcll(__ballot(state == ST_LEAF2)) : 0;
    if ((n_trav | n_shade | n_fill | n_gen | n_leaf | n_shade2 | n_leaf2) == 0) break;
    uint32_t pick = ST_TRAV;
    // (A/B, RL_TUNE third field w: TRAV competes with n_trav * w / 4 — a TRAV step costs a tenth of a LEAF or SHADE block, so running it for
    // fewer lanes feeds bigger LEAF / SHADE blocks; w = 4 is the plain most-lanes rule)
    int best = LDS_SCENE == 4 ? (n_trav * (int)P.tune[2]) >> 2 : n_trav;
    if (n_leaf > best) pick = ST_LEAF, best = n_leaf;
    if (n_shade > best) pick = ST_SHADE, best = n_shade;
    if (n_fill > best) pick = ST_FILL, best = n_fill;
    if (n_gen > best) pick = ST_GEN, best = n_gen;
    if (SPLIT_SHADE && LDS_SCENE == 4 && n_shade2 > best) pick = ST_SHADE2, best = n_shade2;
    if (SPLIT_LEAF && LDS_SCENE == 4 && n_leaf2 > best) pick = ST_LEAF2, best = n_leaf2;

    // The blocks are separate `if`s, each on its own opaque copy of the wave-uniform pick, and not an else-if chain.  A chain (or the
    // switch it becomes) is ONE region with several uniform branches around divergent code, and the compiler linearises such a region:
    // flow blocks with a "not run yet" flag after every block, and in each of them a merge of every variable the block may write with
    // an undefined value.  The register allocator answers those merges with a second copy of the lane state: 117 v_mov on a TRAV
    // pick's way round the loop, for o, d, thr, time and the ray constants that TRAV never writes, and about as many around the other
    // blocks.  A lone `if` with one uniform branch is left as the scalar branch it is, its join merges old and new value only, and the
    // lane state stays in place: 13 v_mov on that path (tools/wave_codegen.py, DESIGN.md section 3.1).  The tests that follow a block
    // that ran cost two scalar instructions each.  (The opaque copy is not what keeps the chain away — without it the separate `if`s
    // compile to the same paths — but with it the headline kernel spills 71 SGPRs instead of 75: the measured form.)
    auto picked = [&](uint32_t s) {
      uint32_t p = pick;
      asm volatile("" : "+s"(p));
      return p == s;
    };
    unsigned long long t_begin = 0;
    if (STATS) {  // debug (tools/sched.py): block executions, lanes served and shader cycles per state, per wave
      t_begin = __builtin_readcyclecounter();
      if (pick != ST_TRAV) {
#pragma unroll
        for (int k = 0; k < 7; k++)
          if (pick == (uint32_t)k) sc_exec[k]++, sc_pop[k] += (unsigned)best;
      }
    }
    if (picked(ST_TRAV)) {
      RL_CG_MARK("TRAV_B");
      if (STATS) sc_trav_picks++;
      // several steps per scheduling decision while the population stays near its starting size
      int floor_n = ((LDS_SCENE == 4 ? n_trav : best) * (int)P.tune[1]) >> 4;
      auto trav_step = [&]() {
        if (STATS) {
          int np = __popcll(__ballot(state == ST_TRAV));
          sc_exec[ST_TRAV]++, sc_pop[ST_TRAV] += (unsigned)np;
        }
        RL_CG_MARK("STEP_B");
        if (state == ST_TRAV) {
          // one LDS round trip: the whole 64-B linked op {box, w_hit, w_miss}; every op stepped here is a box op,
          // the successor words already carry the state the lane enters there (rl_scene_host.cpp link_ops)
          uint32_t w_hit, w_miss;
          bool certain, hitb;
          if (LDS_SCENE == 4) {  // one node = both children: reject-only binary32 tests, nearer child first, the other one pushed
            LdsFloat4 *nd = (LdsFloat4 *)(size_t)pc;
            const Float4 q0 = nd[0], q1 = nd[1], q2 = nd[2];
            const uint32_t w = *(LdsU32 *)(size_t)(pc + 48u);
            const float c32 = (float)closest;
            // a child box as centre c and half-extent h (FastNodeCH): per axis the ray enters the slab at t_c - h |1/d| and leaves it at
            // t_c + h |1/d|, whatever the sign of d, so no min / max orders a slab's two planes (error bound and the host's pad: ray_aux32_direct)
            auto missed = [&](float cx, float cy, float cz, float hx, float hy, float hz, float &tmin) {
              const float tcx = fmaf(cx, ra32.invx, -ra32.oix), tcy = fmaf(cy, ra32.invy, -ra32.oiy), tcz = fmaf(cz, ra32.invz, -ra32.oiz);
              const float ax = fabsf(ra32.invx), ay = fabsf(ra32.invy), az = fabsf(ra32.invz);
              tmin = fmaxf(fmaxf(fmaxf(fmaf(-hx, ax, tcx), fmaf(-hy, ay, tcy)), fmaf(-hz, az, tcz)), 1e-10f);
              float tmax = fminf(fminf(fminf(fmaf(hx, ax, tcx), fmaf(hy, ay, tcy)), fmaf(hz, az, tcz)), c32);
              float diff = tmax - tmin;
              float thresh = fast_miss_thresh(ra32, tmin, tmax);
              return diff < -thresh;  // certainly tmin > tmax; false for NaN arithmetic: visit
            };
            if (STATS) c_nodes += 2;  // debug instantiation only (rl_debug_fast_stats): the fast structure's own tests, not the reference's
            if (STATS && (depth & DEPTH_MASK) == cam.max_depth) c_cam_trav++;
            float tA, tB;
            const uint32_t eA = w & 0xFFFFu, eB = w >> 16, self = depth >> 22;  // self: the sphere the ray left, proven missed (fast_self_miss)
            const bool boxA = !missed(q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, tA);  // {c.xyz, h.xyz} of child A, then of child B
            const bool boxB = !missed(q1.z, q1.w, q2.x, q2.y, q2.z, q2.w, tB);
            const bool hitA = boxA && eA != self, hitB = boxB && eB != self;
            if (STATS) c_self += (boxA && !hitA) + (boxB && !hitB);
            const bool a_first = hitA && (!hitB || tA <= tB);
            uint32_t first = a_first ? eA : eB;
            if (hitA && hitB) fast_push(a_first ? eB : eA);
            if (!(hitA || hitB)) first = fast_pop();
            fast_go(first);
          } else if (LDS_SCENE == 3) {  // 32-byte op: binary32 box + the two successor words
            const LdsCompactOp &op = *(const LdsCompactOp *)(size_t)pc;
            float bx[6] = {op.box[0], op.box[1], op.box[2], op.box[3], op.box[4], op.box[5]};
            w_hit = op.w_hit, w_miss = op.w_miss;
            hitb = aabb_fast32(bx, ra32, (float)closest, certain);
            const uint32_t op_index = (pc - lds_base) >> 5;
            const bool guard = op_index >= P.n_ops;  // a sphere's own box: only ever REJECTS; not one of the reference's tests
            if (!certain) hitb = guard ? true : aabb_hit(P.ops[op_index].box, o, d, 1e-10, closest);  // rare: exact divisions
            if (STATS) c_nodes += guard ? 0u : 1u, c_sph += guard ? 1u : 0u;  // the guarded Sphere::hit counts, skipped or not
          } else {
            const DevOp &op = *(const DevOp *)(LDS_SCENE ? opbase + pc : opbase + (size_t)pc * sizeof(DevOp));
            w_hit = op.code, w_miss = op.skip;
            if (LDS_SCENE) {
              const float *fb = (const float *)&op;
              float bx[6] = {fb[0], fb[1], fb[2], fb[3], fb[4], fb[5]};
              hitb = aabb_fast32(bx, ra32, (float)closest, certain);  // non-finite boxes are NaN here, !fast_ok rays have slack = inf: never certain
            } else {
              double bx[6] = {op.box[0], op.box[1], op.box[2], op.box[3], op.box[4], op.box[5]};
              hitb = aabb_fast(bx, ra, closest, certain, P.k8u);
            }
            if (!certain) hitb = aabb_hit(P.ops[LDS_SCENE ? (pc >> 6) : pc].box, o, d, 1e-10, closest);  // rare: exact divisions
            if (STATS) c_nodes++;
          }
          if (LDS_SCENE != 4) {
            uint32_t w = hitb ? w_hit : w_miss;
            pc = w & 0x1FFFFFFFu;
            state = w >> 29;
          }
        }
        RL_CG_MARK("STEP_E");
      };
      for (int it = 0; it < (int)P.tune[0]; it += 2) {  // two steps per population check
        trav_step();
        trav_step();
        if (__popcll(__ballot(state == ST_TRAV)) < floor_n) break;
      }
      RL_CG_MARK("TRAV_E");
    }
    if (picked(ST_LEAF)) {
      RL_CG_MARK("LEAF_B");
      if (LDS_SCENE == 4) {
        if (state == ST_LEAF) {
          if (__builtin_expect(pc == FAST_SLOW, 0)) {  // rare: the answer may depend on the visiting order -> the reference's own fold
            c_flag += fast_slow_trace(P.ops, spheres, o, d, time, closest, hit_prim);
            c_slow++;
            state = shade_state();
          } else {
            const uint32_t sidx = pc - P.n_fast_inner;
            const uint32_t payload = sidx | (((s_bits[sidx >> 5] >> (sidx & 31u)) & 1u) ? SPH_MOVING : 0u);
            if (STATS) c_sph++;
            if (STATS && (depth & DEPTH_MASK) == cam.max_depth) {
              c_cam_leaf++;
              if (fast_sphere_misses(spheres[sidx], payload, o, d, time)) {
                c_cam_miss++;
                const bool moving = (payload & SPH_MOVING) != 0u;
                if (moving) c_cam_miss_mov++;
                // what the entry table says of this leaf for this pixel, and whether the ball of the sample's time slice would have left it out
                if (g_census.boxes) {
                  const uint32_t ct = census_leaf(px, P.row_first + pr * P.row_step, sidx, time, moving);
                  if (ct & 1u) {
                    if (moving) c_cam_miss_mov_tab++;
                    else c_cam_miss_sta_tab++;
                  }
                  c_cam_miss_cut[0] += (ct >> 1) & 1u, c_cam_miss_cut[1] += (ct >> 2) & 1u, c_cam_miss_cut[2] += (ct >> 3) & 1u;
                }
              }
            }
            if (SPLIT_LEAF) {
              if (fast_sphere_misses(spheres[sidx], payload, o, d, time)) fast_go(fast_pop());
              else state = ST_LEAF2;
            } else {
              fast_sphere_hit(spheres[sidx], payload, o, d, time, ra32.oimax(), closest, hit_prim, amb);
              fast_go(fast_pop());
            }
          }
        }
      } else if (state == ST_LEAF) {  // Sphere::hit for the 1-2 spheres of a BVH leaf / one list item, in stored order
        uint32_t a, b, w;
        if (LDS_SCENE == 3) {  // a guard op: the ONE sphere it stands for (index = op index - n_ops), counted at the guard step
          const LdsCompactOp &op = *(const LdsCompactOp *)(size_t)pc;
          const uint32_t sidx = ((pc - lds_base) >> 5) - P.n_ops;
          a = sidx | (((s_bits[sidx >> 5] >> (sidx & 31u)) & 1u) ? SPH_MOVING : 0u), b = NONE, w = op.w_miss;
        } else {
          const DevOp &op = *(const DevOp *)(LDS_SCENE ? opbase + pc : opbase + (size_t)pc * sizeof(DevOp));
          a = op.a, b = op.b, w = op.skip;
          if (STATS) c_sph++;
        }
        Hit h{closest, hit_prim};
        if (sphere_hit(spheres[a & SPH_INDEX], a, o, d, time, 1e-10, h)) c_flag++;
        if (LDS_SCENE != 3 && b != NONE) {
          if (STATS) c_sph++;
          if (sphere_hit(spheres[b & SPH_INDEX], b, o, d, time, 1e-10, h)) c_flag++;
        }
        closest = h.t, hit_prim = h.prim;
        pc = w & 0x1FFFFFFFu;
        state = w >> 29;
      }
      RL_CG_MARK("LEAF_E");
    }
    if (SPLIT_LEAF && LDS_SCENE == 4 && picked(ST_LEAF2)) {
      if (state == ST_LEAF2) {
        const uint32_t sidx = pc - P.n_fast_inner;
        const uint32_t payload = sidx | (((s_bits[sidx >> 5] >> (sidx & 31u)) & 1u) ? SPH_MOVING : 0u);
        fast_sphere_hit(spheres[sidx], payload, o, d, time, ra32.oimax(), closest, hit_prim, amb);
        fast_go(fast_pop());
      }
    }
    if (picked(ST_SHADE)) {  // (placed here, not last: behind GEN the allocator spills two VGPRs in SHADE's inline ring refill)
      RL_CG_MARK("SHADE_B");
      if (state == ST_SHADE) {
        if (SPLIT_SHADE && LDS_SCENE == 4) shade(std::integral_constant<int, 1>{});
        else shade(std::integral_constant<int, 0>{});
      }
      RL_CG_MARK("SHADE_E");
    }
    if (picked(ST_FILL)) {
      RL_CG_MARK("FILL_B");
      if (COOP_QUAD && RL_COOP_GEN && P.coop_quad) {  // the FILL lanes' blocks as one job list, like GEN's stream resets: one block each, top_up's
        uint32_t nb = 0u, first = 0u;
        if (state == ST_FILL) nb = 1u, first = rng.blk_lo + rng.nres;
        const uint32_t np = rng.template coop_blocks<true, false>(nb, first, true);
        if (STATS) sc_pass[2] += np & 0xFFFFu, sc_pass[3] += np >> 16;
        if (state == ST_FILL) {
          rng.top_up_done();
          state = shade_state();
        }
      } else if (state == ST_FILL) {
        rng.top_up();
        state = shade_state();
      }
      RL_CG_MARK("FILL_E");
    }
    if (picked(ST_GEN)) {
      RL_CG_MARK("GEN_B");
      bool active = false;
      if (state == ST_GEN) {
        active = true;
        // fast traversal: a walk that ended without a hit left its marker (fast_go).  The sample is closed here, before anything below looks
        // at sum, sq or n: background (camera.rs:257), sample done.  thr is the missed ray's: nothing writes it between the walk and this visit.
        if (LDS_SCENE == 4 && pc == FAST_MISSED) {
          if constexpr (MOMENTS) {
            const D3 c = thr * ld3(cam.background);
            sum = sum + c;
            sq = sq + c * c;
          } else sum = sum + thr * ld3(cam.background);
          n++;
          pc = 0;
        }
        if (STEAL && P.steal_state && have_pixel && n < spp) {  // a sample boundary: has a wave without work asked for this pixel?
          const size_t pix = (size_t)pr * W + px;
          if (__atomic_load_n(&P.steal_state[pix], __ATOMIC_RELAXED) == 1u) {
            double *outp = P.out + pix * 3;
            outp[0] = sum.x, outp[1] = sum.y, outp[2] = sum.z;
            P.pos_state[pix] = rng.pos;
            P.steal_n[pix] = n;
            __threadfence();  // the state above is visible before the release
            if (atomicCAS(&P.steal_state[pix], 1u, 2u) == 1u) {
              have_pixel = false;
              n = spp;  // -> claim (the queue is empty by now: the lane is done)
            }  // else: the request was withdrawn in the meantime — the pixel stays here
          }
        }
        if (INDEP && have_pixel) {  // sample n - 1 is done: its colour to the pass buffer; the next one starts from word 0 and (0,0,0)
          rtiow_indep_store(P, n - 1u - s_begin, pr, px, sum);
          if (STATS) c_words += rng.pos;
          if (n >= n_end) have_pixel = false;
          else rng.pos = 0, rng.nres = 0, sum = d3(0.0, 0.0, 0.0);
        }
        // adaptive renders (P.out_count, MOMENTS only): the pixel is also finished at the first checkpoint where its variance estimate is below the caller's bound
        bool stop = false;
        if constexpr (MOMENTS) stop = P.out_count && have_pixel && rtiow_adaptive_stop(P.adapt, P.adapt_total, n, sum, sq);
        if (stop || n >= (INDEP ? n_end : spp)) {  // pixel finished (or none yet): write it out, claim the next slot
          if (have_pixel) {
            size_t pix = (size_t)pr * W + px;
            double *outp = P.out + pix * 3;
            outp[0] = sum.x, outp[1] = sum.y, outp[2] = sum.z;
            if constexpr (MOMENTS) {
              double *outq = P.out_sq + pix * 3;
              outq[0] = sq.x, outq[1] = sq.y, outq[2] = sq.z;
              // its sample count: n where it stopped; the call's total otherwise — also from the first of two launches, whose resume launch tells by that which pixels to continue
              if (P.out_count) P.out_count[pix] = stop ? n : P.adapt_total;
              if (stop) n = spp;  // (a lane whose next slot lies outside the image claims again at its next visit)
            }
            if (STEAL && P.steal_state) atomicExch(&P.steal_state[pix], 3u);  // finished: a request that arrives now finds nothing to take
            if (P.pos_state) P.pos_state[pix] = rng.pos;               // resumable: the next launch continues this pixel
            if (P.tile_cost) atomicAdd(&P.tile_cost[ptile], pix_rays);  // cost estimate for the LPT order of the next launch
            if (STATS && !P.tile_cost) c_words += rng.pos;
            if (STATS && P.pix_rays) P.pix_rays[pix] += pix_rays;
            have_pixel = false;
          }
          uint32_t slot = wave_claim(P.work_counter);
          if (slot >= P.n_slots) {
            state = ST_DONE;
            active = false;
          } else {
            uint32_t grp = 0;
            if (INDEP) grp = slot / P.indep_tile_slots, slot -= grp * P.indep_tile_slots;  // sample-major: a wave claim is one tile at one group
            uint32_t tile = slot >> 6, in = slot & 63u;
            if (P.tile_order) tile = P.tile_order[tile];  // expensive tiles first
            ptile = tile;
            // (the empty asm: the division's reciprocal is formed here, once per pixel, instead of being hoisted out of the loop into a
            // VGPR held through every block — with RL_COOP_GEN that register would spill)
            uint32_t tiles_x = P.tiles_x;
            asm volatile("" : "+s"(tiles_x));
            px = (tile % tiles_x) * 8u + (in & 7u);
            pr = (tile / tiles_x) * 8u + (in >> 3);
            if (px >= W || pr >= P.nrows) active = false;  // slot outside the image: stay in GEN, claim again next time
            else {
              have_pixel = true;
              n = s_begin;
              if (INDEP) n += grp * P.indep_k, n_end = min(n + P.indep_k, spp);
              pix_rays = 0;
              if (P.resume) {  // continue where the previous launch stopped: same sums, same ChaCha word position
                size_t pix = (size_t)pr * W + px;
                const double *inp = P.out + pix * 3;
                sum = d3(inp[0], inp[1], inp[2]);
                if constexpr (MOMENTS) {
                  const double *inq = P.out_sq + pix * 3;
                  sq = d3(inq[0], inq[1], inq[2]);
                  if (P.out_count && P.out_count[pix] != P.adapt_total) have_pixel = false, n = spp;  // stopped in the first launch: not resumed
                }
                rng.pos = P.pos_state[pix];
              } else {
                rng.pos = 0;
                sum = d3(0.0, 0.0, 0.0);
                if (MOMENTS) sq = d3(0.0, 0.0, 0.0);
              }
              rng.nres = 0;
              if (n >= (INDEP ? n_end : spp)) active = false;
            }
          }
        }
        if (active) {
          uint32_t y = P.row_first + pr * P.row_step;
          uint64_t sample_index = (uint64_t)n + P.first_sample;
          const uint64_t stream = sample_index * WH + (uint64_t)px * (uint64_t)W + (uint64_t)y;  // camera.rs:167-170
          if (RL_COOP_GEN) rng.stream = stream, rng.blk_lo = rng.pos >> 4;  // blocks blk_lo, blk_lo + 1: generated below, wave-wide
          else rng.reset_stream(stream);
        }
      }
      bool fill = false;
      if (RL_COOP_GEN) {
        uint32_t nb = active ? 2u : 0u, first = rng.blk_lo;
        if (RL_COOP_GEN == 2) {  // FILL lanes ride along when the pass has room for them: one block each, top_up's
          const uint32_t g2 = 2u * (uint32_t)__popcll(__ballot(active)), nf = (uint32_t)__popcll(__ballot(state == ST_FILL));
          fill = state == ST_FILL && (g2 + nf + 63u) / 64u <= (g2 > 64u ? 2u : 1u);
          if (fill) nb = 1u, first = rng.blk_lo + rng.nres;
        }
        const uint32_t np = rng.template coop_blocks<RL_COOP_GEN == 2>(nb, first, P.coop_quad != 0u);
        if (STATS) sc_pass[0] += np & 0xFFFFu, sc_pass[1] += np >> 16;
        if (active) rng.nres = 2;
        if (fill) {
          rng.top_up_done();
          state = shade_state();
        }
      }
      if (active) {
        uint32_t y = P.row_first + pr * P.row_step;
        // get_ray camera.rs:203-216
        D3 p00 = ld3(cam.pixel_00), du = ld3(cam.pixel_du), dv = ld3(cam.pixel_dv);
        D3 pixel_center = (p00 + du * (double)px) + dv * (double)y;
        double sx = -0.5 + rng.gen_f64();
        double sy = -0.5 + rng.gen_f64();
        D3 pixel_sample = pixel_center + (du * sx + dv * sy);
        if (cam.defocus_angle <= 0.0) o = ld3(cam.lookfrom);
        else {
          double a, b;
          rng.unit_disc(a, b);
          o = (ld3(cam.lookfrom) + ld3(cam.defocus_disk_u) * a) + ld3(cam.defocus_disk_v) * b;
        }
        d = pixel_sample - o;
        // (gen_f64, spelled out: the draw's high word also names the time slice of the pixel's entry word below)
        const uint64_t time_bits = rng.next_u64();
        const uint32_t time_hi = (uint32_t)(time_bits >> 32);
        time = (double)(time_bits >> 11) * 0x1.0p-53;
        thr = d3(1.0, 1.0, 1.0);
        depth = LDS_SCENE == 4 ? cam.max_depth | (FAST_NONE << 22) : cam.max_depth;  // a camera ray has no sphere of its own
        if (cam.max_depth == 0) {  // ray_color(depth 0) = black: the sample contributes (0,0,0)
          sum = sum + d3(0.0, 0.0, 0.0);
          n++;
        } else {
          c_rays++;
          pix_rays++;
          if (STATS) c_cam_rays++;
          // the pixel's entry word: read and used up here, and not loaded ahead of the block pass above: held across it, the word makes GEN's pick
          // path longer (382 -> 408 instructions) and the stealing instantiation spill 109 SGPRs instead of 97
          // With time slices (P.pixel_entry_t; null: the one word of P.pixel_entry) the word is the one of the slice `time` falls into, k =
          // floor(time T), taken from the draw's high word: the index instructions are all it adds, and one load serves both tables (table and
          // shift are scalar selects).  Measured: with k = (uint32_t)(time * T) the headline kernel takes 120 VGPRs instead of 118.  A frame has
          // fewer than 2^32 pixels and the sliced table at most 2^26 words (rl_render.hip build_pixel_entry): the index is formed in 32 bits.
          uint32_t word = fast_root_word;
          if (LDS_SCENE == 4 && P.pixel_entry) {
            const uint32_t *tab = P.pixel_entry_t ? P.pixel_entry_t : P.pixel_entry;
            const uint32_t lg = P.pixel_entry_t ? P.pixel_entry_log2t : 0u;
            word = tab[((pr * W + px) << lg) + time_slice_bits(time_hi, lg)];
          }
          start_ray(word);
        }
      }
      RL_CG_MARK("GEN_E");
    }
    if (SPLIT_SHADE && picked(ST_SHADE2)) {
      if (state == ST_SHADE2) shade(std::integral_constant<int, 2>{});
    }
    if (STATS) {
      unsigned long long dt = __builtin_readcyclecounter() - t_begin;
#pragma unroll
      for (int k = 0; k < 7; k++)
        if (pick == (uint32_t)k) sc_cyc[k] += dt;
    }
  }
  if (STATS && (tid & 63) == 0) {
    unsigned long long *sched = P.stats + 8;  // [3*s] executions, [3*s+1] lanes served, [3*s+2] cycles
#pragma unroll
    for (int s = 0; s < 7; s++) {
      atomicAdd(&sched[3 * s], sc_exec[s]);
      atomicAdd(&sched[3 * s + 1], sc_pop[s]);
      atomicAdd(&sched[3 * s + 2], sc_cyc[s]);
    }
    atomicAdd(&sched[29], sc_trav_picks);  // rl_debug_sched out[29]
    atomicAdd(&sched[21], sc_pass[0]), atomicAdd(&sched[22], sc_pass[1]);  // out[21], out[22]: GEN's full and quad passes
    atomicAdd(&sched[23], sc_pass[2]), atomicAdd(&sched[30], sc_pass[3]);  // out[23], out[30]: FILL's
  }

  if (STEAL && LDS_SCENE == 4 && P.steal_state) {
    // every lane of this wave is out of work: take over pixels that other lanes are still rendering (most expensive tiles first) and
    // run them one at a time with all 64 lanes (its own counters go to P.stats from there)
    rtiow_steal_loop<NT>(P, rng.s_rng);
  }
  unsigned long long v;
  v = wave_sum((unsigned long long)c_rays);
  if ((tid & 63) == 0 && v) atomicAdd(&P.stats[0], v);
  v = wave_sum((unsigned long long)c_flag);
  if ((tid & 63) == 0 && v) atomicAdd(&P.stats[6], v);
  if (LDS_SCENE == 4) {
    v = wave_sum((unsigned long long)c_slow);
    if ((tid & 63) == 0 && v) atomicAdd(&P.stats[7], v);
  }
  if (STATS) {
    v = wave_sum(c_nodes);
    if ((tid & 63) == 0) atomicAdd(&P.stats[1], v);
    v = wave_sum(c_sph);
    if ((tid & 63) == 0) atomicAdd(&P.stats[2], v);
    v = wave_sum(c_words);
    if ((tid & 63) == 0) atomicAdd(&P.stats[5], v);
    if (LDS_SCENE == 4) {
      v = wave_sum(c_self);
      if ((tid & 63) == 0) atomicAdd(&P.stats[8 + 24], v);  // after the scheduler's 21 words (rl_debug_sched out[24])
      v = wave_sum(c_cam_trav);  // the census: camera rays' TRAV lane-steps, LEAF visits, and their number (out[25 .. 27])
      if ((tid & 63) == 0) atomicAdd(&P.stats[8 + 25], v);
      v = wave_sum(c_cam_leaf);
      if ((tid & 63) == 0) atomicAdd(&P.stats[8 + 26], v);
      v = wave_sum(c_cam_rays);
      if ((tid & 63) == 0) atomicAdd(&P.stats[8 + 27], v);
      v = wave_sum(c_cam_miss);  // out[28]
      if ((tid & 63) == 0) atomicAdd(&P.stats[8 + 28], v);
      v = wave_sum(c_cam_miss_mov);  // out[31]; rl_debug_pixel_entry_census: [0] this one, [1] .. [5] the ones below
      if ((tid & 63) == 0) atomicAdd(&P.stats[8 + 31], v);
      v = wave_sum(c_cam_miss_mov_tab);
      if ((tid & 63) == 0) atomicAdd(&P.stats[8 + 32], v);
      v = wave_sum(c_cam_miss_sta_tab);
      if ((tid & 63) == 0) atomicAdd(&P.stats[8 + 33], v);
#pragma unroll
      for (int k = 0; k < 3; k++) {
        v = wave_sum(c_cam_miss_cut[k]);
        if ((tid & 63) == 0) atomicAdd(&P.stats[8 + 34 + k], v);
      }
    }
  }
