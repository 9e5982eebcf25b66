// Material::scatter + Material::emitted on a hit (material.rs:11-20, 59-214): the one statement that the general kernel
// (rl_rtiow_general.h), the wave-scheduled general body (rl_rtiow_wave_general_body.inc) and the scatter query (rl_material_query.h)
// shade with.  Their frames and records are equal bit for bit because they inline this text.
// Three kernels keep a statement of their own, the same bits from other text (tests/test_gpu_scatter_forms.py holds them all against
// each other): rl_rtiow_wave_body.inc's `shade`, the specialised form for sphere scenes (a flattened per-sphere record,
// sub-expressions hoisted across branches, the SHADE2 split); the cooperative kernel (rl_rtiow_coop.h) and the SHADE block of
// rl_rtiow_fastgen_body.inc, which both came out about 1.2 % slower with this function inlined (profiles/scatter_refactor.txt; the
// fast general kernel keeps its own POP text for the same reason).
//
// A caller evaluates the texture first (material_texture), scatters (material_scatter) and does what is its own with the result: a
// render multiplies its throughput, adds the emitted colour and ends or continues the path, the query packs a record.
#pragma once
#include "rl_rtiow_kernel.h"

namespace rl {

enum : uint32_t {
  SCATTER_NONE = 0,      // no scattered ray, nothing emitted (Flat, an unknown kind)
  SCATTER_RAY = 1,       // Some((scattered, attenuation)): dir, att
  SCATTER_ABSORBED = 2,  // a Metal reflection below the surface: None — after its unit_sphere has been drawn
  SCATTER_EMITTED = 3,   // DiffuseLight: emitted() = the texture colour, no scattered ray
};

struct Scatter {
  uint32_t what;  // SCATTER_*
  bool flagged;   // the Dielectric's incoming direction could not be normalized (material.rs:150-151 would panic): one panic site
  D3 att;         // SCATTER_RAY: the attenuation, else zeros
  D3 dir;         // SCATTER_RAY: the scattered ray's direction (its origin is the hit point); SCATTER_ABSORBED: the rejected direction; else zeros
  D3 emitted;     // SCATTER_EMITTED: the emitted colour, else zeros
};

// The colour the material's texture gives at the hit: Lambertian and Isotropic attenuation, DiffuseLight emission; (0,0,0) for the kinds
// that have no texture.  `value(texture id)` is the caller's texture_value<MODE> with the hit's (u, v, p) — it is not called for the
// other kinds.  It draws no random numbers, and its transcendental code (acos / atan2 for sphere UVs, sin and Perlin for Noise) is
// register-hungry: it runs BEFORE material_scatter, while no scatter temporary is live.
// MEDIA: the scene may hold Isotropic materials.
template <bool MEDIA, class Value>
__device__ __forceinline__ D3 material_texture(const DevMaterial &m, Value value) {
  if (m.kind == RL_MAT_LAMBERTIAN || m.kind == RL_MAT_DIFFUSE_LIGHT || (MEDIA && m.kind == RL_MAT_ISOTROPIC)) return value(m.texture);
  return d3(0.0, 0.0, 0.0);
}

// wd: the incoming ray's direction; normal, front: the hit record's.  `tex()` gives the texture colour at the hit — material_texture's
// value, evaluated beforehand (`[&] { return texc; }`) — and is read where the reference calls texture.value, at most once.  `rng`
// supplies unit_sphere() and gen_f64() from the path's stream (Ring as it is; RngDraws for the general kernel; LazyDraws for the scatter
// query): each material draws what the reference draws, in its order — at most one of the two, once.
template <bool MEDIA, class Tex, class Draws>
__device__ __forceinline__ Scatter material_scatter(const DevMaterial &m, D3 wd, D3 normal, bool front, Tex tex, Draws &rng) {
  const uint32_t kind = m.kind;
  Scatter s{SCATTER_NONE, false, d3(0.0, 0.0, 0.0), d3(0.0, 0.0, 0.0), d3(0.0, 0.0, 0.0)};
  if (MEDIA && kind == RL_MAT_ISOTROPIC) {  // material.rs:201-214: Vec3::random_unit_vector, attenuation = texture.value(uv, p)
    s.dir = rng.unit_sphere();
    s.att = tex(), s.what = SCATTER_RAY;
  } else if (kind == RL_MAT_LAMBERTIAN) {
    D3 dir = normal + rng.unit_sphere();
    bool near_zero = approx_eq_eps(dir.x, 0.0, 1e-8) && approx_eq_eps(dir.y, 0.0, 1e-8) && approx_eq_eps(dir.z, 0.0, 1e-8);
    s.dir = near_zero ? normal : dir;
    s.att = tex(), s.what = SCATTER_RAY;
  } else if (kind == RL_MAT_METAL) {
    D3 reflected = wd - normal * (2.0 * dot(wd, normal));
    s.dir = normalize(reflected) + rng.unit_sphere() * m.fuzz;
    if (dot(s.dir, normal) > 0.0) s.att = ld3(m.albedo), s.what = SCATTER_RAY;
    else s.what = SCATTER_ABSORBED;
  } else if (kind == RL_MAT_DIELECTRIC) {
    double ri = front ? 1.0 / m.ior : m.ior;
    double m2 = len2(wd);
    D3 ud;
    if (approx_eq_eps(m2, 0.0, 1e-16)) {
      s.flagged = true;
      ud = wd;
    } else
      ud = normalize(wd);
    double cos_theta = fmin(dot(-ud, normal), 1.0);
    double sin_theta = sqrt(1.0 - cos_theta * cos_theta);
    bool reflect = ri * sin_theta > 1.0;
    if (!reflect) {
      double q = (1.0 - ri) / (1.0 + ri);
      double r0 = q * q;
      double xx = 1.0 - cos_theta;
      double x2 = xx * xx;
      double refl = r0 + (1.0 - r0) * (xx * (x2 * x2));
      reflect = refl > rng.gen_f64();
    }
    if (reflect) s.dir = ud - normal * (2.0 * dot(ud, normal));
    else {
      D3 perp = (ud + normal * cos_theta) * ri;
      D3 par = normal * (-sqrt(fabs(1.0 - len2(perp))));
      s.dir = perp + par;
    }
    s.att = d3(1.0, 1.0, 1.0), s.what = SCATTER_RAY;
  } else if (kind == RL_MAT_DIFFUSE_LIGHT) {
    s.emitted = tex(), s.what = SCATTER_EMITTED;
  }
  return s;
}

}  // namespace rl
