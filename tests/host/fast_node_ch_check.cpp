// Stand-alone check of the centre / half-extent form of the fast sphere tree's nodes (csrc/rl_fast_bvh.cpp fast_node_ch) and of the TRAV
// step's box test on it (csrc/rl_rtiow_wave_body.inc; derivation at ray_aux32_direct, csrc/rl_rtiow_wave.h): no HIP, no Python.
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -I rendering-learning_amd \
//       tests/host/fast_node_ch_check.cpp rendering-learning_amd/csrc/{rl_program,rl_fast_bvh,rl_scene_host}.cpp -o fast_node_ch_check
// 1. Enclosure.  For the trees of a set of worlds every derived box [c - h, c + h] holds its [lo, hi] box with delta = fast_ch_delta to
//    spare on both sides, and h is the smallest binary32 that does — decided in exact arithmetic (a 2560-bit fixed-point sum).  Worlds
//    that must get no tree get no derived nodes either.  One line per world:  world NAME inner N bad B loose L
// 2. The step's test.  A binary32 model with the kernel's operation order (fmaf; inv32 = 1 / d32 moved by -1, 0 or +1 ulp to stand for
//    v_rcp_f32) against a slab test of the ORIGINAL [lo, hi] box for the binary64 ray in long double.  The model must never reject a
//    (ray, box, closest) the ray touches inside [1e-10, closest]; "touches" is decided with 1e-15 relative of slop towards touching, ten
//    thousand times the long double roundings and a ten-millionth of the model's own margin.  The triples are built, not drawn: rays
//    aimed at face, edge and corner points moved by 0, +-1, +-16 ulps, thin direction components, origins at the frame's bound,
//    |c| / h up to 1e6, closest at the entry distance +- a few ulps.  Rejections of CLEAR misses are counted for this model and for the
//    lo / hi model of the parent commit's step on the same triples.  One line:
//        model triples N in_range R touching T wrong W clear C rejected_ch A rejected_lohi B near E near_ch F near_lohi G
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "csrc/rl_scene_host.h"
#include "host/scenes.hpp"

extern "C" int rl_bvh_build(const double *, const rl_href *, uint32_t, uint32_t, rl_bvh_node *, uint32_t, uint32_t *) { return RL_E_NO_DEVICE; }
extern "C" const char *rl_last_error(void) { return "no device: stand-alone host check"; }

static int failures = 0;
static void fail(const std::string &name, const std::string &what) {
  std::printf("FAIL %s: %s\n", name.c_str(), what.c_str());
  failures++;
}

// ---- exact sums of binary64 numbers: two's-complement fixed point, bit 0 = 2^-1200
struct Exact {
  static const int LIMBS = 40;
  uint64_t w[LIMBS];
  Exact() { std::memset(w, 0, sizeof w); }
  void add(double x) {
    if (x == 0.0) return;
    int e;
    const double m = std::frexp(std::fabs(x), &e);        // |x| = m 2^e, m in [0.5, 1)
    const uint64_t mant = (uint64_t)std::ldexp(m, 53);    // exact: 53 bits
    const int sh = e - 53 + 1200, limb = sh / 64, off = sh % 64;
    uint64_t part[2] = {mant << off, off ? mant >> (64 - off) : 0};
    unsigned carry = 0;
    for (int i = limb; i < LIMBS; i++) {
      const uint64_t p = i - limb < 2 ? part[i - limb] : 0, old = w[i];
      if (x > 0.0) {
        w[i] = old + p + carry;
        carry = (w[i] < old || (carry && w[i] == old)) ? 1 : 0;
      } else {
        w[i] = old - p - carry;
        carry = (old < p || (carry && old == p)) ? 1 : 0;
      }
    }
  }
  int sign() const {
    if (w[LIMBS - 1] >> 63) return -1;
    for (int i = 0; i < LIMBS; i++)
      if (w[i]) return 1;
    return 0;
  }
};
static int sum_sign(std::initializer_list<double> xs) {
  Exact s;
  for (double x : xs) s.add(x);
  return s.sign();
}
// c - h <= lo - delta and c + h >= hi + delta
static bool encloses(float c, float h, float lo, float hi, double delta) { return sum_sign({c, -(double)h, -(double)lo, delta}) <= 0 && sum_sign({hi, delta, -(double)c, -(double)h}) <= 0; }

// ---- worlds
struct Rng {
  uint64_t s;
  uint64_t next() {  // splitmix64
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull, z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
  }
  double uni() { return (double)(next() >> 11) * 0x1.0p-53; }
  double range(double a, double b) { return a + (b - a) * uni(); }
  double logrange(double a, double b) { return a * std::exp(std::log(b / a) * uni()); }
  int pick(int n) { return (int)(next() % (uint64_t)n); }
};
static rtiow::HittablePtr ball(rtiow::Center c, double r) { return std::make_shared<rtiow::Sphere>(c, r, rtiow::Lambertian(rtiow::SolidColor(rtiow::Color(0.5, 0.5, 0.5)))); }
static scenes::RtiowScene list_world(std::vector<rtiow::HittablePtr> v) { return scenes::RtiowScene{std::make_shared<rtiow::HittableList>(std::move(v)), {}}; }
// n spheres of radius [0.1, 0.5] s in a slab of 22 s x 1 s x 22 s around `at`, every third one moving, over a ground sphere of radius 1000 s when asked
static scenes::RtiowScene random_world(uint64_t seed, int n, double s, double at, bool ground, double rmin = 0.1, double rmax = 0.5) {
  Rng g{seed};
  std::vector<rtiow::HittablePtr> v;
  if (ground) v.push_back(ball(rtiow::Center::Stationary(rtiow::Point3(at, at - 1000.0 * s, at)), 1000.0 * s)), n--;
  for (int i = 0; i < n; i++) {
    const double r = g.range(rmin, rmax) * s;
    const rtiow::Point3 p(at + g.range(-11, 11) * s, at + r + g.range(0, 1) * s, at + g.range(-11, 11) * s);
    if (i % 3 == 2) v.push_back(ball(rtiow::Center::Moving(p, rtiow::Point3(p.x(), p.y() + g.range(0, 0.5) * s, p.z())), r));
    else v.push_back(ball(rtiow::Center::Stationary(p), r));
  }
  return list_world(std::move(v));
}

struct FrameBox {
  rl::FastNode nd;
  double M;  // the bound on origin coordinates that goes with it (GuardFrame::M)
};
static std::vector<FrameBox> g_boxes;  // nodes of the worlds' trees, for the model's triples

static void check_world(const char *name, const scenes::RtiowScene &s, bool want_tree) {
  rtiow::Flattened f;
  f.root = s.world->flatten(f);
  rl_rtiow_scene_desc d = f.desc();
  std::shared_ptr<const rl::HostRtiow> H;
  std::string err;
  const int rc = rl::build_host_rtiow(&d, H, err);
  if (rc != RL_OK || !H) return fail(name, "build_host_rtiow = " + std::to_string(rc) + " (" + err + ")");
  const bool tree = H->fast_root != rl::FAST_NONE;
  if (tree != want_tree) fail(name, want_tree ? "no fast tree" : "a fast tree was built");
  if (H->fast_nodes_ch.size() != H->fast_nodes.size()) fail(name, "derived nodes: " + std::to_string(H->fast_nodes_ch.size()) + " for " + std::to_string(H->fast_nodes.size()));
  size_t bad = 0, loose = 0;
  for (size_t i = 0; i < H->fast_nodes.size() && i < H->fast_nodes_ch.size(); i++) {
    const rl::FastNode &nd = H->fast_nodes[i];
    const rl::FastNodeCH &q = H->fast_nodes_ch[i];
    if (q.child != nd.child) bad++;
    for (int side = 0; side < 2; side++)
      for (int ax = 0; ax < 3; ax++) {
        const float lo = nd.box[side][2 * ax], hi = nd.box[side][2 * ax + 1], c = q.ch[side][ax], h = q.ch[side][3 + ax];
        const double delta = rl::fast_ch_delta(c, lo, hi);
        if (!(std::isfinite(c) && std::isfinite(h) && h >= 0.0f && delta >= 4.76837158203125e-07 * std::fabs((double)c)) || !encloses(c, h, lo, hi, delta)) bad++;
        else if (h > 0.0f && encloses(c, std::nextafterf(h, 0.0f), lo, hi, delta)) loose++;
        if (!(std::fabs((double)c - 0.5 * ((double)lo + (double)hi)) <= 6e-8 * std::fabs((double)c) + 1e-45)) bad++;  // c = RN32(midpoint)
      }
    if (i < 400) g_boxes.push_back(FrameBox{nd, rl::guard_frame(d).M});
  }
  std::printf("world %s inner %zu bad %zu loose %zu\n", name, H->fast_nodes.size(), bad, loose);
  if (bad || loose) fail(name, "derived boxes: " + std::to_string(bad) + " do not enclose, " + std::to_string(loose) + " are larger than needed");
}

// ---- the step's test in binary32
struct Ray32 {
  float inv[3], oi[3], slack;
};
// ray_aux32_direct with the reciprocal moved by k ulps; false: the ray is outside the filter's range (slack = +inf: nothing is rejected)
static bool ray32(const double o[3], const double d[3], const int k[3], Ray32 &r) {
  float m = 0, imin = INFINITY, imax = 0, omax = 0;
  for (int a = 0; a < 3; a++) {
    float inv = 1.0f / (float)d[a];
    if (k[a]) inv = std::nextafterf(inv, k[a] > 0 ? INFINITY : -INFINITY);
    r.inv[a] = inv, r.oi[a] = (float)o[a] * inv;
    m = std::fmax(m, std::fabs(r.oi[a])), imin = std::fmin(imin, std::fabs(inv)), imax = std::fmax(imax, std::fabs(inv)), omax = std::fmax(omax, std::fabs((float)o[a]));
  }
  const bool ok = imin >= 1e-30f && imax <= 1e30f && m <= 1e30f && omax <= 1e30f;
  r.slack = ok ? m * 1.430511474609375e-06f : INFINITY;
  return ok;
}
static bool decide(float tmin, float tmax, const Ray32 &r) {
  const float diff = tmax - tmin, thresh = std::fmaf(tmin + std::fabs(tmax), 7.152557373046875e-07f, r.slack);
  return diff < -thresh;
}
static bool missed_ch(const float ch[6], const Ray32 &r, float c32) {
  float tn[3], tf[3];
  for (int a = 0; a < 3; a++) {
    const float tc = std::fmaf(ch[a], r.inv[a], -r.oi[a]), ai = std::fabs(r.inv[a]);
    tn[a] = std::fmaf(-ch[3 + a], ai, tc), tf[a] = std::fmaf(ch[3 + a], ai, tc);
  }
  return decide(std::fmax(std::fmax(std::fmax(tn[0], tn[1]), tn[2]), 1e-10f), std::fmin(std::fmin(std::fmin(tf[0], tf[1]), tf[2]), c32), r);
}
static bool missed_lohi(const float b[6], const Ray32 &r, float c32) {  // the step before the centre / half-extent form
  float tn[3], tf[3];
  for (int a = 0; a < 3; a++) {
    const float t0 = std::fmaf(b[2 * a], r.inv[a], -r.oi[a]), t1 = std::fmaf(b[2 * a + 1], r.inv[a], -r.oi[a]);
    tn[a] = std::fmin(t0, t1), tf[a] = std::fmax(t0, t1);
  }
  return decide(std::fmax(std::fmax(std::fmax(tn[0], tn[1]), tn[2]), 1e-10f), std::fmin(std::fmin(std::fmin(tf[0], tf[1]), tf[2]), c32), r);
}
// the ray's parameter interval inside [lo, hi], in long double
static void slab(const float b[6], const double o[3], const double d[3], long double &t_in, long double &t_out, long double &scale) {
  t_in = -INFINITY, t_out = INFINITY, scale = 0;
  for (int a = 0; a < 3; a++) {
    const long double t0 = ((long double)b[2 * a] - o[a]) / d[a], t1 = ((long double)b[2 * a + 1] - o[a]) / d[a];
    t_in = std::fmax(t_in, std::fmin(t0, t1)), t_out = std::fmin(t_out, std::fmax(t0, t1));
    scale = std::fmax(scale, std::fabs((long double)o[a] / d[a]));
  }
}

struct Tally {
  unsigned long long triples = 0, in_range = 0, touching = 0, wrong = 0, clear = 0, rej_ch = 0, rej_lohi = 0, near = 0, near_ch = 0, near_lohi = 0;
};
static void one_triple(const rl::FastNode &nd, const rl::FastNodeCH &q, int side, const double o[3], const double d[3], double closest, Rng &g, Tally &T) {
  const int k[3] = {g.pick(3) - 1, g.pick(3) - 1, g.pick(3) - 1};
  Ray32 r;
  T.triples++;
  if (!ray32(o, d, k, r)) return;
  T.in_range++;
  long double t_in, t_out, scale;
  slab(nd.box[side], o, d, t_in, t_out, scale);
  const long double lo = std::fmax(t_in, (long double)1e-10), hi = std::fmin(t_out, (long double)closest), size = std::fabs(lo) + std::fabs(hi) + scale;
  const bool touches = lo <= hi + 1e-15L * size, clear = lo > hi + 1e-3L * size;
  const bool rc = missed_ch(q.ch[side], r, (float)closest), rl_ = missed_lohi(nd.box[side], r, (float)closest);
  T.touching += touches, T.clear += clear;
  if (touches && rc) {
    if (T.wrong++ < 5)
      std::printf("WRONG box [%a %a][%a %a][%a %a] o %a %a %a d %a %a %a closest %a k %d %d %d\n", nd.box[side][0], nd.box[side][1], nd.box[side][2], nd.box[side][3], nd.box[side][4],
                  nd.box[side][5], o[0], o[1], o[2], d[0], d[1], d[2], closest, k[0], k[1], k[2]);
  }
  if (clear) T.rej_ch += rc, T.rej_lohi += rl_;
  if (!touches && !clear) T.near++, T.near_ch += rc, T.near_lohi += rl_;  // near misses: how tight the two forms are (reported only)
}

static float ulps(float x, int n) {
  for (; n > 0; n--) x = std::nextafterf(x, INFINITY);
  for (; n < 0; n++) x = std::nextafterf(x, -INFINITY);
  return x;
}

static void model(Tally &T) {
  Rng g{2024};
  static const int DISP[5] = {0, 1, -1, 16, -16};
  std::vector<FrameBox> boxes = g_boxes;  // the worlds' own nodes, then made-up ones at four scales with |c| / h up to 1e6
  static const double SCALES[4] = {1e-3, 1.0, 1e3, 1e4};
  for (int i = 0; i < 3200; i++) {
    rl::FastNode nd{};
    const double S = SCALES[i & 3];
    for (int side = 0; side < 2; side++)
      for (int a = 0; a < 3; a++) {
        const double c = (i % 5 == 4 ? (g.pick(2) ? S : -S) : g.range(-S, S)), h = (i % 5 >= 3 ? g.logrange(1e-6, 1e-5) * std::fabs(c) : g.logrange(1e-6, 1.0) * S);
        nd.box[side][2 * a] = (float)(c - h), nd.box[side][2 * a + 1] = std::nextafterf((float)(c + h), INFINITY);
      }
    boxes.push_back(FrameBox{nd, 8.0 * S});
  }
  for (size_t bi = 0; bi < boxes.size(); bi++) {
    const rl::FastNode &nd = boxes[bi].nd;
    const rl::FastNodeCH q = rl::fast_node_ch(nd);
    double cmax = 0, ext = 0;
    for (int j = 0; j < 6; j++) cmax = std::fmax(cmax, std::fabs((double)nd.box[0][j])), ext = std::fmax(ext, (double)nd.box[0][j | 1] - (double)nd.box[0][j & ~1]);
    const double M = boxes[bi].M;
    for (int rep = 0; rep < 40; rep++) {
      const int side = rep & 1;
      const float *b = nd.box[side];
      // a target point: per axis the low plane, the high plane (moved by some ulps) or somewhere between / beside them
      double p[3], o[3], d[3];
      const int kind = rep % 10;  // 0-2 corner, 3-4 edge, 5-6 face, 7 inside, 8-9 beside (a clear miss most of the time)
      const int n_on = kind <= 2 ? 3 : kind <= 4 ? 2 : kind <= 6 ? 1 : 0, first = g.pick(3);
      for (int j = 0; j < 3; j++) {
        const int a = (first + j) % 3;
        const float lo = b[2 * a], hi = b[2 * a + 1];
        if (j < n_on) p[a] = ulps(g.pick(2) ? lo : hi, DISP[g.pick(5)]);
        else if (kind <= 7) p[a] = g.range(lo, hi);
        else p[a] = (g.pick(2) ? (double)hi + g.logrange(1e-4, 10.0) * ((double)hi - lo + 1e-6 * std::fabs((double)hi)) : g.range(lo, hi));
      }
      // an origin: near the box, far away, or on the frame's bound; and the direction towards p, scaled at random
      const int where = g.pick(4);
      for (int a = 0; a < 3; a++) {
        if (where == 0) o[a] = p[a] + g.range(-3, 3) * (ext + 1e-3 * cmax);
        else if (where == 1) o[a] = g.range(-M, M);
        else if (where == 2) o[a] = g.pick(2) ? M : -M;
        else o[a] = p[a] + 1.0;  // (replaced below)
      }
      const double len = g.logrange(1e-3, 1e3);
      bool zero = false;
      for (int a = 0; a < 3; a++) d[a] = (p[a] - o[a]) * len, zero = zero || d[a] == 0.0;
      if (where == 3) {  // one or two components down to 1e-6 of the largest, set directly; the origin follows from the target
        const double big = g.logrange(1e-3, 1e3) * (g.pick(2) ? 1 : -1);
        for (int a = 0; a < 3; a++) d[a] = a == first ? big : big * g.logrange(1e-6, 1e-3) * (g.pick(2) ? 1 : -1);
        if (g.pick(2)) d[(first + 1) % 3] = big * g.range(0.1, 1.0);
        const double t = g.logrange(1e-3, 1.0) * M / std::fabs(big);
        for (int a = 0; a < 3; a++) o[a] = p[a] - t * d[a];
      }
      if (zero) continue;
      long double t_in, t_out, scale;
      slab(b, o, d, t_in, t_out, scale);
      const double entry = (double)std::fmax(t_in, (long double)1e-10);
      // closest: nothing found yet, far behind the box, and the entry distance moved by a few binary64 and binary32 ulps
      one_triple(nd, q, side, o, d, INFINITY, g, T);
      one_triple(nd, q, side, o, d, std::fabs(entry) * 4.0 + 1.0, g, T);
      for (int e = -2; e <= 2; e++) one_triple(nd, q, side, o, d, entry * (1.0 + e * 0x1.0p-52), g, T);
      for (int e : {-16, -3, -1, 1, 3, 16}) one_triple(nd, q, side, o, d, entry * (1.0 + e * 0x1.0p-23), g, T);
      one_triple(nd, q, side, o, d, entry * g.logrange(0.5, 2.0), g, T);
    }
  }
}

int main() {
  check_world("bouncing_spheres", scenes::bouncing_spheres(1), true);
  check_world("one_sphere", list_world({ball(rtiow::Center::Stationary(rtiow::Point3(0, 0, -1)), 0.5)}), true);
  check_world("two_spheres", list_world({ball(rtiow::Center::Stationary(rtiow::Point3(0, 0, -1)), 0.5), ball(rtiow::Center::Stationary(rtiow::Point3(0, -100.5, -1)), 100)}), true);
  check_world("moving_511", random_world(7, 511, 1.0, 0.0, false), true);
  check_world("scaled_1e-3", random_world(11, 200, 1e-3, 0.0, false), true);
  check_world("scaled_1e3", random_world(13, 200, 1e3, 0.0, false), true);
  check_world("small_at_1e4", random_world(17, 120, 0.02, 1e4, false, 0.5, 0.5), true);  // radius 0.01 around (1e4, 1e4, 1e4)
  check_world("nan_centre", list_world({ball(rtiow::Center::Stationary(rtiow::Point3(NAN, 0, -1)), 0.5), ball(rtiow::Center::Stationary(rtiow::Point3(0, 0, 1)), 0.5)}), false);
  check_world("huge_centre", list_world({ball(rtiow::Center::Stationary(rtiow::Point3(1e200, 0, -1)), 0.5), ball(rtiow::Center::Stationary(rtiow::Point3(0, 0, 1)), 0.5)}), false);
  {  // fast_node_ch on boxes build_fast_bvh never makes: no finite box -> NaN (the step's comparison is false, the child is visited)
    rl::FastNode nd{};
    nd.box[0][0] = -INFINITY, nd.box[0][1] = 1.0f, nd.box[0][2] = NAN, nd.box[0][3] = 1.0f, nd.box[0][4] = -3e38f, nd.box[0][5] = 3e38f;
    const rl::FastNodeCH q = rl::fast_node_ch(nd);
    if (!(std::isnan(q.ch[0][0]) && std::isnan(q.ch[0][3]) && std::isnan(q.ch[0][1]) && std::isnan(q.ch[0][4]))) fail("non_finite", "a box without finite planes did not become NaN");
    if (!(q.ch[0][5] >= 3e38f)) fail("non_finite", "a box as wide as binary32 lost its extent");
  }
  Tally T;
  model(T);
  std::printf("model triples %llu in_range %llu touching %llu wrong %llu clear %llu rejected_ch %llu rejected_lohi %llu near %llu near_ch %llu near_lohi %llu\n", T.triples, T.in_range, T.touching, T.wrong,
              T.clear, T.rej_ch, T.rej_lohi, T.near, T.near_ch, T.near_lohi);
  if (T.wrong) fail("model", std::to_string(T.wrong) + " touched boxes were rejected");
  return failures ? 1 : 0;
}
