/*
 * rl_render.h — the C-ABI drop-in boundary for the per-pixel / per-ray hot path of
 * marcantony/rendering-learning, rebuilt as hand-written HIP for MI355X (gfx950).
 *
 * The reference has NO existing FFI; this header *creates* the seam.  Each entry point
 * names the reference interface it replaces (paths relative to /root/reference):
 *
 *   rl_rtiow_render*      <- ray-tracing-one-weekend/src/camera.rs:122  Camera::render
 *                            camera.rs:136  Camera::render_from_checkpoint (first_sample)
 *                            camera.rs:145-199  Camera::_render  (the per-pixel loop)
 *   rl_rtc_render*        <- ray-tracer-challenge/src/scene/camera.rs:93  Camera::render
 *                            scene/mod.rs:24  Scene::render
 *   rl_rtiow_scene_create <- what `world: H where H: Hittable` carries into render()
 *                            (hittable/mod.rs:40-43 trait, bvh.rs:11-20, sphere.rs:16-21 ...)
 *   rl_rtc_scene_create   <- scene/world.rs:26-31  World{objects,lights,max_reflection_depth,void_color}
 *
 * Conventions: plain pointers and sizes only; 0 on success, negative RL_E_* otherwise; the
 * library never unwinds or aborts across the boundary (every reference panic site becomes an
 * error code or a flagged-pixel count); scene_create deep-copies, so the caller may free its
 * arrays as soon as it returns; the caller owns all host pointers.
 * Concurrency: as Camera::render takes `&self` and a `Sync` world (camera.rs:122), every render entry point may be
 * called on ONE rl_scene from several host threads and on several HIP streams at once.  The scene's program is
 * immutable; it owns one set of work buffers (counters, the cost-sorted tile order), so the library serialises the
 * host side per scene and makes a render wait on the device for the scene's previous one when their streams differ:
 * concurrent callers get the frames a lone caller gets, rendered one after the other (each fills the GPU).  Use
 * several scene handles for renders that should share the GPU.  rl_init / rl_init_multi / rl_shutdown / scene
 * creation and destruction are NOT to be raced against renders.
 * Everything is IEEE binary64 unless stated.  There is NO CPU fallback: without a GPU / without
 * the HIP code object every compute entry point fails with RL_E_NO_DEVICE.
 */
#ifndef RL_RENDER_H
#define RL_RENDER_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RL_ABI_VERSION 6

/* ------------------------------------------------------------------ errors */
#define RL_OK 0
#define RL_E_INVALID (-1)     /* bad argument / malformed scene graph (out-of-range index, cycle) */
#define RL_E_NO_DEVICE (-2)   /* no HIP device / library not initialised */
#define RL_E_DEVICE (-3)      /* HIP runtime error (text in rl_last_error) */
#define RL_E_UNSUPPORTED (-4) /* scene uses a feature this build has no kernel for */
#define RL_E_DEGENERATE (-5)  /* a reference panic site was reached; output is written, stats.flagged > 0 */
#define RL_E_NOMEM (-6)       /* the host ran out of memory, e.g. while compiling a scene description; nothing was created */

/* ------------------------------------------------------------------ lifetime */
/* device < 0: keep the process's current HIP device.  One GPU (use this form for one process per GPU, e.g. under
 * torch.distributed / MPI, with rl_*_render_device + the caller's own gather). */
int rl_init(int device);
/* One process, n_devices GPUs (0 = every visible one): the reference calls ONE Camera::render(&world) from one thread
 * (ray-tracing-one-weekend/src/camera.rs:122, examples/common/mod.rs:16; ray-tracer-challenge/src/scene/camera.rs:93), so a drop-in
 * host reaches all GPUs of the node through rl_*_render_multi.  The library owns one stream per device and the RCCL communicators
 * (ncclCommInitAll, one rank per GPU; librccl is dlopen'ed here, a single-GPU host never loads it).  Scenes created AFTERWARDS are
 * replicated on every device. */
int rl_init_multi(int n_devices);
int rl_device_count(void); /* device contexts the library drives: 1 after rl_init, n after rl_init_multi, 0 before either */
void rl_shutdown(void);
const char *rl_last_error(void); /* thread-local, owned by the library */
int rl_abi_version(void);
/* Fills name (NUL-terminated, <= cap) with the device's gcnArchName; returns CU count or <0. */
int rl_device_info(char *name, int cap);

typedef struct rl_scene rl_scene;
void rl_scene_destroy(rl_scene *);

/* per-render counters; every field is a sum over the pixels rendered by the call.  They count the calls the REFERENCE's
 * algorithm makes on the same input (the oracle's counters are equal, which is how the tests prove that every branch went the
 * same way): where the device proves with a conservative bounding-box test that a Sphere::hit / Triangle::intersect cannot
 * produce an intersection the reference would keep and skips the arithmetic, the call is still counted. */
typedef struct rl_stats {
  uint64_t rays;            /* RTIOW: ray_color calls with depth>0 (camera.rs:232). RTC: color_at + shadow rays */
  uint64_t node_tests;      /* AABB::hit calls (aabb.rs:123) / Bounded::test (bounded.rs:100) */
  uint64_t sphere_tests;    /* Sphere::hit calls (sphere.rs:34) */
  uint64_t planar_tests;    /* Plane::hit_ab (plane.rs:51) / RTC Triangle::intersect (triangle.rs:63) */
  uint64_t instance_enters; /* Transform::hit + Translate::hit / RTC Transformed::intersect */
  uint64_t rng_words;       /* ChaCha8 u32 words consumed (RTIOW only) */
  uint64_t flagged;         /* reference panic sites reached (see RL_E_DEGENERATE) */
  double kernel_ms;         /* device time of the render kernel(s), HIP events on the launch stream */
} rl_stats;

/* =====================================================================
 *  RTIOW  (ray-tracing-one-weekend)
 * ===================================================================== */

/* reference to any Hittable: (kind, index into that kind's array) */
typedef struct rl_href {
  uint32_t kind;
  uint32_t index;
} rl_href;
enum {
  RL_H_NONE = 0,
  RL_H_SPHERE = 1,    /* hittable/sphere.rs:16 Sphere<M> */
  RL_H_PLANAR = 2,    /* hittable/flat/{plane,quad,triangle}.rs */
  RL_H_TRANSLATE = 3, /* hittable/translate.rs:6 */
  RL_H_TRANSFORM = 4, /* hittable/transform.rs:13 */
  RL_H_BVH = 5,       /* bvh.rs:11 Bvh<H> node */
  RL_H_LIST = 6,      /* hittable/mod.rs:88 impl Hittable for [H] */
  RL_H_MEDIUM = 7     /* hittable/constant_medium.rs:9 ConstantMedium (deterministic variant, see rl_medium) */
};

typedef struct rl_sphere { /* sphere.rs:11-21 */
  double center0[3];       /* Center::Stationary(p) or Moving(p1, _) */
  double center1[3];       /* Moving(_, p2); ignored unless moving */
  double radius;
  uint32_t moving;
  uint32_t material;
} rl_sphere;

enum { RL_PLANAR_PLANE = 0, RL_PLANAR_QUAD = 1, RL_PLANAR_TRIANGLE = 2 };
typedef struct rl_planar { /* flat/plane.rs:12-20 + quad.rs:13 + triangle.rs:13-18 */
  double q[3], u[3], v[3];
  double w[3];      /* n/(n.n), n = u x v            (plane.rs:30) */
  double normal[3]; /* unit(n)                       (plane.rs:26) */
  double d;         /* normal . q                    (plane.rs:28) */
  uint32_t kind;    /* RL_PLANAR_* */
  uint32_t material;
  uint32_t has_normals; /* triangle.rs:16 Option<[Vec3;3]> */
  uint32_t has_uvs;     /* triangle.rs:17 Option<[(f64,f64);3]> */
  double normals[9];    /* v1,v2,v3 */
  double uvs[6];        /* (u,v) x3 */
} rl_planar;

typedef struct rl_translate { /* translate.rs:6-9 */
  double offset[3];
  rl_href child;
} rl_translate;

typedef struct rl_transform { /* transform.rs:13-19; row-major 3x3 */
  double m[9], inv[9], inv_t[9];
  rl_href child;
} rl_transform;

typedef struct rl_bvh_node { /* bvh.rs:11-20 */
  double bbox[6];            /* x.min,x.max,y.min,y.max,z.min,z.max (aabb.rs:7-11), already padded */
  uint32_t n_children;       /* 1 or 2, in the reference's stored order */
  uint32_t reserved;
  rl_href child[2];
} rl_bvh_node;

/* hittable/constant_medium.rs:9-80 with ONE deliberate difference: the reference draws the free path from the process-global
 * `rand::random::<f64>()` (constant_medium.rs:55; its own comment: "This breaks deterministic/repeatable renders"), which no seeded
 * reference run can reproduce.  Here the draw comes from the pixel's ChaCha8 stream — the `rng` Camera::_render hands to scatter —
 * at the moment ConstantMedium::hit reaches it, in the reference's evaluation order: hit_distance = neg_inv_density * ln(gen::<f64>()).
 * Everything else is the reference's: boundary.hit(r, universe), boundary.hit(r, [t1 + 1e-4, inf]), clamping to ray_t, the arbitrary
 * normal (1, 0, 0) / uv (0, 0) / Face::Front.  The boundary may be any hittable except another medium. */
typedef struct rl_medium {
  rl_href boundary;
  double neg_inv_density; /* -1.0 / density (constant_medium.rs:19) */
  uint32_t material;      /* phase function: meant to be RL_MAT_ISOTROPIC */
  uint32_t reserved;
} rl_medium;

typedef struct rl_list { /* a slice of hittables; items live in list_items[first .. first+count) */
  uint32_t first, count;
} rl_list;

enum {
  RL_MAT_FLAT = 0,       /* material.rs:52 */
  RL_MAT_LAMBERTIAN = 1, /* material.rs:69 */
  RL_MAT_METAL = 2,      /* material.rs:99 */
  RL_MAT_DIELECTRIC = 3, /* material.rs:134 */
  RL_MAT_DIFFUSE_LIGHT = 4, /* material.rs:178 */
  RL_MAT_ISOTROPIC = 5      /* material.rs:197: scatters into Vec3::random_unit_vector, attenuation = texture (uses `texture`) */
};
typedef struct rl_material {
  uint32_t kind;
  uint32_t texture;  /* Lambertian / DiffuseLight */
  double albedo[3];  /* Metal */
  double fuzz;       /* Metal */
  double ior;        /* Dielectric.refraction_index */
} rl_material;

enum { RL_TEX_SOLID = 0, RL_TEX_CHECKER = 1, RL_TEX_IMAGE = 2, RL_TEX_NOISE = 3 };
typedef struct rl_texture { /* texture.rs:15,25,58,84 */
  uint32_t kind;
  uint32_t even, odd; /* Checker: texture ids */
  uint32_t image;     /* Image: image id;  Noise: perlin id */
  double color[3];    /* SolidColor.albedo */
  double inv_scale;   /* Checker.inv_scale;  Noise.scale */
} rl_texture;

/* perlin.rs:9-14: the tables Perlin::new drew from the caller's Rng (the device only evaluates noise()/turb()) */
typedef struct rl_perlin {
  double randvec[256][3];
  uint32_t perm_x[256], perm_y[256], perm_z[256]; /* each a permutation of 0..255 */
} rl_perlin;

typedef struct rl_image { /* texture.rs:58 Image{Rgb32FImage}: linear RGB f32, row-major, top row first */
  uint32_t width, height;
  const float *rgb;
} rl_image;

typedef struct rl_rtiow_scene_desc {
  const rl_sphere *spheres;       uint32_t n_spheres;
  const rl_planar *planars;       uint32_t n_planars;
  const rl_translate *translates; uint32_t n_translates;
  const rl_transform *transforms; uint32_t n_transforms;
  const rl_bvh_node *bvh_nodes;   uint32_t n_bvh_nodes;
  const rl_list *lists;           uint32_t n_lists;
  const rl_href *list_items;      uint32_t n_list_items;
  const rl_material *materials;   uint32_t n_materials;
  const rl_texture *textures;     uint32_t n_textures;
  const rl_image *images;         uint32_t n_images;
  rl_href root;
  const rl_perlin *perlins;       uint32_t n_perlins; /* ABI v3 */
  const rl_medium *media;         uint32_t n_media;   /* ABI v5 */
} rl_rtiow_scene_desc;

/* The DERIVED camera: outputs of Camera::new (camera.rs:72-118). The host keeps Camera::new
 * (tan() stays on the host); the device receives the vectors. */
typedef struct rl_rtiow_camera {
  uint32_t image_width, image_height;
  uint32_t samples_per_pixel, max_depth;
  double lookfrom[3];
  double pixel_00[3], pixel_du[3], pixel_dv[3];
  double defocus_disk_u[3], defocus_disk_v[3];
  double defocus_angle;
  double background[3];
  uint64_t seed;
} rl_rtiow_camera;

/* What a description must keep.  Both *_scene_create validate the whole description on the host before any device sees it (every
 * kernel trusts the compiled program); one that breaks a rule below gives NULL, with the code in the second column behind
 * rl_last_error()'s text.  Sharing is legal (one record referenced from many places: every reference is lowered again), cycles
 * are not.  The cost of a refusal is bounded by the size of the description, never by the size of its expansion, and the
 * compilers use a constant amount of stack whatever the depth of the graph.
 *   every array with a non-zero count is non-NULL; every index lies inside its table; every kind is a known one
 *                                                                         RL_E_INVALID
 *   no hittable / object contains itself                                  RL_E_INVALID  "cycle through ..."
 *   deepest reference below the root (RTC: below a world object), the
 *   root being 0, at most RL_SCENE_MAX_NEST                               RL_E_INVALID  "scene graph too deep"
 *   ops of the expanded program, its end op included, fewer than
 *   RL_SCENE_MAX_OPS (a sphere, planar, triangle, shape, BVH node or
 *   Bounded is one op, a Translate / Transform / Transformed /
 *   ConstantMedium two, a CSG three; lists and groups none.  RTC counts
 *   every triangle reference as one op although the program merges
 *   consecutive triangles into one: there the limit bounds the count
 *   from above, not the program's final size)                             RL_E_INVALID  "program too large"
 *   RTIOW: Translate / Transform nested at most 8 deep                    RL_E_INVALID
 *          Checker textures acyclic, nested at most 32 deep               RL_E_INVALID
 *          no ConstantMedium inside a ConstantMedium's boundary           RL_E_INVALID
 *          n_spheres <= 0x3FFFFFFF; a BVH node has 1 or 2 children        RL_E_INVALID
 *   RTC:   Transformed nested at most 8 deep, CSG at most 4 deep          RL_E_INVALID
 *          at most 0xFFFF lights                                          RL_E_UNSUPPORTED
 *          max_reflection_depth <= 7 in a world with shapes, CSG,
 *          patterns, or reflective / transparent materials                RL_E_UNSUPPORTED
 *   the host has the memory for the compiled program                      RL_E_NOMEM
 * Not checked: that an array is as long as its count says, cameras, non-finite or degenerate geometry. */
#define RL_SCENE_MAX_NEST 100000u
#define RL_SCENE_MAX_OPS 0x7FFFFFFFu

rl_scene *rl_rtiow_scene_create(const rl_rtiow_scene_desc *desc);

/* Bvh::new (bvh.rs:22-60) on the device, for worlds too big to build comfortably on the host (1 M spheres: seconds).
 * Input: n hittables as their bounding boxes (6 doubles each: x.min, x.max, y.min, y.max, z.min, z.max = what
 * Hittable::bounding_box() returns, already padded by AABB::new) and their hrefs.  Output: the nodes in the order the
 * reference's recursion creates them (node, left subtree, right subtree; node 0 is the root): box = merge of the boxes
 * below (aabb.rs:135), split on the longest axis (bvh.rs:63-77) after a STABLE sort by `box.axis.min` under
 * f64::total_cmp (bvh.rs:49 uses sort_unstable_by: the order of equal keys is implementation-defined there), left half =
 * the first len / 2, leaves of 1-2 hittables.  Inner nodes reference their children as RL_H_BVH node_base + index, so the
 * records can be appended to a scene's bvh_nodes at position node_base.  *out_n_nodes receives the node count (also
 * when cap is too small: RL_E_INVALID).  Host pointers. */
int rl_bvh_build(const double *prim_boxes, const rl_href *prims, uint32_t n, uint32_t node_base, rl_bvh_node *out_nodes,
                 uint32_t cap, uint32_t *out_n_nodes);

/* Replaces Camera::render / render_from_checkpoint's _render(first_sample, world).
 * out_rgb_sum: caller-owned host buffer, W*H*3 doubles, row-major, holds SUMS over samples
 * exactly like Canvas.data (camera.rs:269). */
int rl_rtiow_render(const rl_scene *, const rl_rtiow_camera *, uint64_t first_sample,
                    double *out_rgb_sum, rl_stats *opt_stats);

/* Row-sharded form (multi-GPU: rank g renders rows g, g+G, ...). Output holds only those rows,
 * compact: nrows = ceil((H - row_first) / row_step), each W*3 doubles. Host output buffer. */
int rl_rtiow_render_rows(const rl_scene *, const rl_rtiow_camera *, uint64_t first_sample,
                         uint32_t row_first, uint32_t row_step, double *out_rgb_sum,
                         rl_stats *opt_stats);

/* Same, but the output stays in HBM: d_out_rgb_sum is a DEVICE pointer (e.g. a torch tensor's
 * data_ptr), hip_stream is a hipStream_t (NULL = default stream). Asynchronous unless opt_stats
 * is non-NULL (stats need a sync). This is what bench.py times. */
int rl_rtiow_render_device(const rl_scene *, const rl_rtiow_camera *, uint64_t first_sample,
                           uint32_t row_first, uint32_t row_step, void *d_out_rgb_sum,
                           void *hip_stream, rl_stats *opt_stats);

/* Sample-parallel rendering with independent sample streams.  Every sample is rendered as the reference renders the FIRST sample of
 * a render: c_s(x, y) = Camera::_render(s, world) with samples_per_pixel = 1 — a fresh ChaCha8Rng at word position 0 on stream
 * s*W*H + x*W + y, get_ray, ray_color (ray-tracing-one-weekend/src/camera.rs:145-174).  With F = first_sample and S =
 * cam->samples_per_pixel the output is, per component, in f64 and left to right without contraction:
 *     out(x, y) = ((((A + c_F) + c_{F+1}) + ...) + c_{F+S-1}),   A = 0.0 (accumulate = 0) or the sums already in out (accumulate = 1)
 * — bit for bit the canvas of S repetitions of `canvas = cam1.render_from_checkpoint(world, &canvas)` from a canvas that holds A with
 * samples = F (cam1: the same camera with samples_per_pixel = 1; camera.rs:136-143, Canvas::merge camera.rs:273-291).  The samples do
 * not chain, so the frame does not depend on how the work is split: a + b samples in two calls with accumulate = 1, any row shard and
 * any number of passes give the same bits as one call.  It is a different image from rl_rtiow_render* of S samples (same distribution,
 * other random numbers).  Output: compact shard rows as rl_rtiow_render_rows; when accumulate = 1 the buffer is read first.
 * The _rows form takes a host buffer; the _device form a device buffer and a hipStream_t, asynchronous unless opt_stats is non-NULL
 * (then all seven counters, as the sums of the S single-sample counting renders).  rl_render_status reports rays and flagged for the
 * asynchronous form; a reached panic site returns RL_E_DEGENERATE.  rl_rtiow_render_progress reports nothing for these renders. */
int rl_rtiow_render_independent_rows(const rl_scene *, const rl_rtiow_camera *, uint64_t first_sample, uint32_t row_first,
                                     uint32_t row_step, uint32_t accumulate, double *out_rgb_sum, rl_stats *opt_stats);
int rl_rtiow_render_independent_device(const rl_scene *, const rl_rtiow_camera *, uint64_t first_sample, uint32_t row_first,
                                       uint32_t row_step, uint32_t accumulate, void *d_out_rgb_sum, void *hip_stream,
                                       rl_stats *opt_stats);

/* Completion + status of the ASYNCHRONOUS renders of this scene since the last call (rl_*_render_device / rl_*_render_multi_device
 * with opt_stats == NULL): waits for all of them, fills opt_stats->rays with the ray count of the most recently enqueued one and
 * ->flagged with the panic sites reached by any of them (the other counters need a counting render) and returns RL_E_DEGENERATE
 * if a reference panic site (camera.rs:86, material.rs:151, vec3.rs:220, ...) was reached, else RL_OK.  Renders of one scene issued
 * concurrently (several threads, streams or multi-GPU frames) each count exactly once. */
int rl_render_status(const rl_scene *, rl_stats *opt_stats);

/* Progress of the RTIOW render that is executing on this scene — the reference logs "Scanline-equivalents remaining" once per `image_width`
 * finished pixels (camera.rs:176-184); a host that wants that line polls this from another thread.  pixels_claimed: pixel slots the
 * kernel's lanes have taken so far in the launch that is running; pixels_total: slots of that launch (the shard's pixels rounded up to
 * 8 x 8 tiles); phase: a render of >= 64 samples per pixel is two launches (0: samples [0, 8) of every pixel, 1: the rest).  Never waits:
 * the FIRST call switches progress counting on for the renders enqueued after it (their work counters then live in pinned host memory the
 * kernels reach over PCIe, one atomic per wave per 64 pixels) and reports zeros; later calls are two host loads.  Frames of at most ~41 k
 * pixels (cooperative kernel) and counting renders report through the same words.  All three outputs are optional (NULL).  A scene
 * created under rl_init_multi (one replica per device) is not followed: RL_E_UNSUPPORTED. */
int rl_rtiow_render_progress(const rl_scene *, uint64_t *pixels_claimed, uint64_t *pixels_total, uint32_t *phase);

/* Camera::render on every GPU of rl_init_multi: image row r is rendered by GPU r mod G with the single-GPU
 * kernels (no collective during the render), then ONE exchange — ncclSend / ncclRecv of ceil(H/G)*W*3 f64 per peer to GPU 0 in one
 * RCCL group, each peer over its own xGMI link — and a de-interleave kernel on GPU 0.  The frame is bit-identical for every G.
 * out_rgb_sum: host buffer, W*H*3 doubles (Canvas.data order, sums).  With G = 1 this is rl_rtiow_render. */
int rl_rtiow_render_multi(const rl_scene *, const rl_rtiow_camera *, uint64_t first_sample, double *out_rgb_sum, rl_stats *opt_stats);
/* Same with the frame left in GPU 0's HBM (d_out_rgb_sum: device pointer on device 0).  Asynchronous on the library's streams
 * unless opt_stats is non-NULL; rl_render_status(scene) waits for the frame. */
int rl_rtiow_render_multi_device(const rl_scene *, const rl_rtiow_camera *, uint64_t first_sample, void *d_out_rgb_sum, rl_stats *opt_stats);

/* Output stage on the device (color.rs:22-57, output.rs:5-14): mean = sum * (1/samples), linear_to_srgb,
 * floor(v * 255.999) clamped to 0..255.  d_rgb_sum / d_rgb8 are DEVICE pointers (n_pixels*3 f64 / u8). */
int rl_rtiow_encode_rgb8_device(const void *d_rgb_sum, uint64_t n_pixels, uint32_t samples, void *d_rgb8, void *hip_stream);
/* Render + encode on the device, copy back only the W*H*3 bytes a P3 PPM prints (24x less PCIe traffic). */
int rl_rtiow_render_rgb8(const rl_scene *, const rl_rtiow_camera *, uint64_t first_sample, uint8_t *out_rgb8, rl_stats *opt_stats);

/* =====================================================================
 *  RTC  (ray-tracer-challenge)
 * ===================================================================== */

typedef struct rl_oref { /* reference to any Object (scene/object/mod.rs:10) */
  uint32_t kind;
  uint32_t index;
} rl_oref;
enum {
  RL_O_NONE = 0,
  RL_O_TRIANGLE = 1,    /* object/triangle.rs:22 */
  RL_O_GROUP = 2,       /* object/group.rs:14 */
  RL_O_BOUNDED = 3,     /* object/bounded.rs:86 */
  RL_O_TRANSFORMED = 4, /* object/transformed.rs:12 */
  RL_O_SPHERE = 5,      /* object/sphere.rs:10   (index into shapes[]) */
  RL_O_PLANE = 6,       /* object/plane.rs:11 */
  RL_O_CUBE = 7,        /* object/cube.rs:10 */
  RL_O_CYLINDER = 8,    /* object/cylinder.rs:13 */
  RL_O_CONE = 9,        /* object/cone.rs:13 */
  RL_O_CSG = 10         /* object/csg.rs:32      (index into csgs[]) */
};

typedef struct rl_rtc_triangle { /* triangle.rs:22-27 */
  double p1[3];
  double e1[3], e2[3];
  uint32_t smooth;  /* TriangleNormal::Smooth vs Flat */
  uint32_t material;
  double n1[3], n2[3], n3[3]; /* smooth: vertex normals; flat: n1 = the flat normal */
} rl_rtc_triangle;

typedef struct rl_rtc_group { /* children live in group_items[first .. first+count) */
  uint32_t first, count;
} rl_rtc_group;

typedef struct rl_rtc_bounded { /* bounded.rs:11-14,86-89 */
  double minimum[3], maximum[3];
  rl_oref child;
} rl_rtc_bounded;

typedef struct rl_rtc_transformed { /* transformed.rs:12-16; row-major 4x4 */
  double inverse[16];
  double inverse_transpose[16];
  rl_oref child;
} rl_rtc_transformed;

typedef struct rl_rtc_material { /* scene/material.rs:22-31 */
  double color[3];   /* Surface::Color(c) when pattern == 0 */
  double ambient, diffuse, specular, shininess;
  double reflectivity, transparency, refractive_index;
  uint32_t pattern;  /* 0: Surface::Color; k > 0: Surface::Pattern(patterns[k-1]) */
  uint32_t reserved;
} rl_rtc_material;

/* analytic shapes in their own object space: unit sphere, xz plane, [-1,1]^3 cube, y-axis cylinder / double cone */
typedef struct rl_rtc_shape { /* object/{sphere,plane,cube,cylinder,cone}.rs */
  uint32_t kind;      /* RL_O_SPHERE .. RL_O_CONE */
  uint32_t material;
  uint32_t has_minimum, has_maximum; /* cylinder / cone: Option<f64> */
  uint32_t closed, reserved;
  double minimum, maximum;
} rl_rtc_shape;

enum { RL_CSG_UNION = 0, RL_CSG_INTERSECTION = 1, RL_CSG_DIFFERENCE = 2 };
typedef struct rl_rtc_csg { /* object/csg.rs:9-36 */
  uint32_t operation;
  uint32_t reserved;
  rl_oref left, right;
} rl_rtc_csg;

enum { RL_PAT_STRIPE = 1, RL_PAT_RING = 2, RL_PAT_GRADIENT = 3, RL_PAT_CHECKER3D = 4 };
typedef struct rl_rtc_pattern { /* scene/pattern/{stripe,ring,gradient,checker3d}.rs: two colours + the pattern's own transform.inverse() (row-major) */
  uint32_t kind;
  uint32_t reserved;
  double a[3], b[3];
  double inverse[16];
} rl_rtc_pattern;

typedef struct rl_rtc_light { /* scene/light.rs:4-7 */
  double position[3];
  double intensity[3];
} rl_rtc_light;

typedef struct rl_rtc_scene_desc { /* scene/world.rs:26-31 */
  const rl_rtc_triangle *triangles;       uint32_t n_triangles;
  const rl_rtc_group *groups;             uint32_t n_groups;
  const rl_oref *group_items;             uint32_t n_group_items;
  const rl_rtc_bounded *boundeds;         uint32_t n_boundeds;
  const rl_rtc_transformed *transformeds; uint32_t n_transformeds;
  const rl_rtc_material *materials;       uint32_t n_materials;
  const rl_oref *objects;                 uint32_t n_objects; /* World.objects, in order */
  const rl_rtc_light *lights;             uint32_t n_lights;
  uint32_t max_reflection_depth;
  uint32_t reserved;
  double void_color[3];
  const rl_rtc_shape *shapes;             uint32_t n_shapes;
  const rl_rtc_csg *csgs;                 uint32_t n_csgs;
  const rl_rtc_pattern *patterns;         uint32_t n_patterns;
} rl_rtc_scene_desc;

typedef struct rl_rtc_camera { /* scene/camera.rs:11-19: the derived fields + transform.inverse() */
  uint32_t hsize, vsize;
  double inverse[16]; /* row-major */
  double pixel_size, half_width, half_height;
} rl_rtc_camera;

/* The limits a description must keep and the codes of a refusal: see rl_rtiow_scene_create. */
rl_scene *rl_rtc_scene_create(const rl_rtc_scene_desc *desc);

/* Replaces Camera::render(&world, &RenderOpts{anti_aliasing_samples}) (scene/camera.rs:93).
 * out_rgb: W*H*3 doubles, row-major (Canvas.data order, draw/canvas.rs:44), pixel MEANS. */
int rl_rtc_render(const rl_scene *, const rl_rtc_camera *, uint32_t aa_samples, double *out_rgb,
                  rl_stats *opt_stats);
int rl_rtc_render_rows(const rl_scene *, const rl_rtc_camera *, uint32_t aa_samples,
                       uint32_t row_first, uint32_t row_step, double *out_rgb, rl_stats *opt_stats);
int rl_rtc_render_device(const rl_scene *, const rl_rtc_camera *, uint32_t aa_samples,
                         uint32_t row_first, uint32_t row_step, void *d_out_rgb, void *hip_stream,
                         rl_stats *opt_stats);

/* Camera::render(&world, opts) over every GPU of rl_init_multi: rows interleaved, one RCCL exchange to GPU 0 (see rl_rtiow_render_multi). */
int rl_rtc_render_multi(const rl_scene *, const rl_rtc_camera *, uint32_t aa_samples, double *out_rgb, rl_stats *opt_stats);
int rl_rtc_render_multi_device(const rl_scene *, const rl_rtc_camera *, uint32_t aa_samples, void *d_out_rgb, rl_stats *opt_stats);

/* Output stage on the device (draw/canvas.rs:53-56): round(c * 255) (half away from zero) clamped to 0..255. */
int rl_rtc_encode_rgb8_device(const void *d_rgb, uint64_t n_pixels, void *d_rgb8, void *hip_stream);
int rl_rtc_render_rgb8(const rl_scene *, const rl_rtc_camera *, uint32_t aa_samples, uint8_t *out_rgb8, rl_stats *opt_stats);

/* =====================================================================
 *  Pixel-list renders: the pixels of the caller's choosing, not a frame or a set of rows
 * =====================================================================
 *   rl_rtiow_render_pixels*  <- ray-tracing-one-weekend/src/camera.rs:145-199  Camera::_render's per-pixel loop, for the listed pixels only
 *   rl_rtc_render_pixels*    <- ray-tracer-challenge/src/scene/camera.rs:93-124 Camera::render's per-pixel body (rays_for_pixel, color_at, the AA mean)
 * (xs[i], ys[i]), i < n, are pixels of the camera's WHOLE frame (x < W, y < H).  The list may be unsorted and may hold duplicates: every
 * element is rendered on its own, duplicates get identical bits.  Output is compact: element i is written at out[3*i ..], never at
 * (y*W + x)*3.
 * Values.  out[i] is bit for bit what rl_rtiow_render_rows(.., first_sample, 0, 1, ..) / rl_rtc_render(.., aa_samples, ..) writes for
 * that pixel, whatever else is in the list: for RTIOW the sum over cam->samples_per_pixel CHAINED samples accumulated from 0.0, sample s
 * on stream (first_sample + s)*W*H + x*W + y with the ChaCha word position carried from sample to sample (camera.rs:161-174); for RTC the
 * mean over the aa_samples x aa_samples grid.  Scenes with ConstantMedium objects are accepted, as in the renders.
 * Stats.  With opt_stats all seven counters are the reference's for exactly the listed pixels (a duplicate counts twice), from the
 * reference-order kernels; without it the call is counter-free, may take the fast traversals and gives the same bits.
 * Forms.  The plain forms take host buffers; the _device forms take device buffers (d_xs, d_ys: n uint32 each; d_out: n*3 f64) and a
 * hipStream_t and are asynchronous unless opt_stats is non-NULL; rl_render_status covers them, each call counting once.
 * Errors.  A pixel outside the image: RL_E_INVALID from the plain forms, before anything is launched and with `out` untouched; in the
 * _device forms (which cannot look at the list) such an element is written as zeros and traces nothing.  n = 0: RL_OK, no buffer is
 * touched (opt_stats, when given, is zeroed).  NULL buffers with n > 0, aa_samples = 0, an empty image, a scene of the other family:
 * RL_E_INVALID; n >= 0xFFFF0000 (the 32-bit work counter): RL_E_INVALID "image too large".  A reached panic site sets flagged and
 * returns RL_E_DEGENERATE with every output written.  Concurrency: as the renders (serialised per scene).  Under rl_init_multi the call
 * runs on device 0's replica (a list is not split across GPUs).
 * Progress.  rl_rtiow_render_progress follows an RTIOW pixel-list render: pixels_claimed of pixels_total = n list elements, phase 0. */
int rl_rtiow_render_pixels(const rl_scene *, const rl_rtiow_camera *, uint64_t first_sample, const uint32_t *xs, const uint32_t *ys,
                           uint64_t n, double *out_rgb_sum /* [n][3] */, rl_stats *opt_stats);
int rl_rtiow_render_pixels_device(const rl_scene *, const rl_rtiow_camera *, uint64_t first_sample, const void *d_xs, const void *d_ys,
                                  uint64_t n, void *d_out_rgb_sum, void *hip_stream, rl_stats *opt_stats);
int rl_rtc_render_pixels(const rl_scene *, const rl_rtc_camera *, uint32_t aa_samples, const uint32_t *xs, const uint32_t *ys,
                         uint64_t n, double *out_rgb /* [n][3] */, rl_stats *opt_stats);
int rl_rtc_render_pixels_device(const rl_scene *, const rl_rtc_camera *, uint32_t aa_samples, const void *d_xs, const void *d_ys,
                                uint64_t n, void *d_out_rgb, void *hip_stream, rl_stats *opt_stats);

/* =====================================================================
 *  Second moments: sum of the squared sample colours beside the sum, for adaptive sampling
 * =====================================================================
 * The chained RTIOW renders once more, with a second output.  out_rgb_sum is exactly what the matching plain call writes
 * (rl_rtiow_render_rows / _device, rl_rtiow_render_pixels / _device: same bits, same layout).  out_rgb_sq has the same layout and holds,
 * per pixel and channel, with c_n the colour sample n adds to the sum (0 for a path that contributes nothing):
 *     sq = 0.0;  for n ascending:  sq = sq + (c_n * c_n)
 * in f64, the product rounded before the add (no FMA).  With both, (sq - sum^2 / S) / (S - 1) / S estimates the variance of the pixel's mean.
 * Second moments of calls that continue each other (first_sample) add, as the sums do.  The _rows form always counts, as
 * rl_rtiow_render_rows does; the list form counts when opt_stats is given, as rl_rtiow_render_pixels does.
 * Status codes, opt_stats (a counting call takes the reference-order kernel: all seven counters, as the plain call's), rl_render_status,
 * rl_rtiow_render_progress and concurrency are those of the plain calls; a NULL out_rgb_sq is RL_E_INVALID; in the _device list form an
 * element outside the image writes zeros to BOTH buffers.  There is no CPU fallback: without a device RL_E_NO_DEVICE, outputs untouched.
 * Not offered: the independent-sample renders, the multi-GPU renders, rgb8 output, and the RTC family (its AA grid is deterministic). */
int rl_rtiow_render_moments_rows(const rl_scene *, const rl_rtiow_camera *, uint64_t first_sample, uint32_t row_first, uint32_t row_step,
                                 double *out_rgb_sum, double *out_rgb_sq, rl_stats *opt_stats);
int rl_rtiow_render_moments_device(const rl_scene *, const rl_rtiow_camera *, uint64_t first_sample, uint32_t row_first, uint32_t row_step,
                                   void *d_out_rgb_sum, void *d_out_rgb_sq, void *hip_stream, rl_stats *opt_stats);
int rl_rtiow_render_pixels_moments(const rl_scene *, const rl_rtiow_camera *, uint64_t first_sample, const uint32_t *xs, const uint32_t *ys,
                                   uint64_t n, double *out_rgb_sum /* [n][3] */, double *out_rgb_sq /* [n][3] */, rl_stats *opt_stats);
int rl_rtiow_render_pixels_moments_device(const rl_scene *, const rl_rtiow_camera *, uint64_t first_sample, const void *d_xs, const void *d_ys,
                                          uint64_t n, void *d_out_rgb_sum, void *d_out_rgb_sq, void *hip_stream, rl_stats *opt_stats);

/* =====================================================================
 *  Adaptive renders: every pixel stops, inside the launch, once its variance estimate is below the caller's bound
 * =====================================================================
 * rl_rtiow_render_moments_rows / _device once more, with a stopping rule.  A pixel is rendered exactly as the chained render renders it
 * (streams, the word position carried from sample to sample, sum and sq as "Second moments" defines them; first_sample only shifts the
 * streams).  Let n be the number of samples OF THIS CALL accumulated so far.  At a checkpoint n = min_samples + k * check_every (k >= 0)
 * with n < cam->samples_per_pixel the pixel's three channels c are tested, in binary64, every operation rounded on its own (no FMA), in
 * exactly this order:
 *     nd  = (double)n
 *     s2  = sum_c * sum_c
 *     lhs = (nd * sq_c) - s2
 *     rhs = (nd - 1.0) * ((abs_variance * (nd * nd)) + (rel_variance * s2))
 *     ok_c = lhs <= rhs
 * and the pixel stops at the first checkpoint where ok_r && ok_g && ok_b; otherwise it runs to samples_per_pixel.  A NaN in any term
 * makes ok_c false: the pixel runs on.  Algebraically the rule is  variance of the mean <= abs_variance + rel_variance * mean^2,
 * multiplied through by n^2 (n - 1): no division, so that a host can reproduce every count to the bit.
 * Outputs per pixel, laid out as the plain call's pixels: out_rgb_sum and out_rgb_sq (3 f64 each), out_count (one uint32: the samples
 * taken).  For every pixel sum and sq are bit for bit what rl_rtiow_render_moments_rows writes for it when the camera's
 * samples_per_pixel equals the pixel's count: a prefix of a chain is the chain of a shorter render.  min_samples >= samples_per_pixel
 * never reaches a checkpoint: the moments call's bytes, and count == samples_per_pixel everywhere.
 * RL_E_INVALID, outputs untouched: a NULL rule, a NULL output, min_samples < 2, check_every == 0, a negative or NaN bound.  Everything
 * else follows the moments calls: _rows always counts, _device is asynchronous unless opt_stats is given; a counting call takes the
 * reference-order kernel and its seven counters are the reference's for exactly the samples rendered (each pixel's count);
 * rl_render_status, rl_rtiow_render_progress and per-scene serialisation as for the plain renders; no CPU fallback (RL_E_NO_DEVICE,
 * outputs untouched).
 * Not offered: pixel-list forms, the independent-sample renders, the multi-GPU renders, rgb8 output, the RTC family; the cooperative
 * one-wave-per-pixel kernel has no adaptive mode (its small frames run in the wave-scheduled kernel: same bits). */
typedef struct rl_rtiow_adaptive {
  uint32_t min_samples;  /* >= 2: the first checkpoint                                   */
  uint32_t check_every;  /* >= 1: checkpoints at n = min_samples + k * check_every, k >= 0 */
  double abs_variance;   /* >= 0                                                          */
  double rel_variance;   /* >= 0                                                          */
} rl_rtiow_adaptive;
int rl_rtiow_render_adaptive_rows(const rl_scene *, const rl_rtiow_camera *, uint64_t first_sample, uint32_t row_first, uint32_t row_step,
                                  const rl_rtiow_adaptive *rule, double *out_rgb_sum, double *out_rgb_sq, uint32_t *out_count, rl_stats *opt_stats);
int rl_rtiow_render_adaptive_device(const rl_scene *, const rl_rtiow_camera *, uint64_t first_sample, uint32_t row_first, uint32_t row_step,
                                    const rl_rtiow_adaptive *rule, void *d_out_rgb_sum, void *d_out_rgb_sq, void *d_out_count, void *hip_stream,
                                    rl_stats *opt_stats);

/* =====================================================================
 *  Feature renders: first-hit albedo, normal and depth sums, the guide buffers of a denoiser
 * =====================================================================
 * One launch traces cam->samples_per_pixel jittered camera rays per pixel to their FIRST hit and keeps four sums.  Let the pixel be
 * (x, y) of the camera's whole frame, F = first_sample, S = cam->samples_per_pixel, W x H the frame.  For s = F, F+1, .., F+S-1, in
 * this order:
 *     rng  = ChaCha8Rng::seed_from_u64(cam->seed), set_stream(s*W*H + x*W + y), word position 0
 *     ray  = Camera::get_ray(&mut rng, x, y)                 -- what rl_rtiow_camera_rays returns for that cursor
 *     hit  = world.hit(&ray, &Interval{1e-10, +inf}), media drawing from rng
 *                                                            -- what rl_rtiow_hit_rays_seeded returns for (ray, cursor behind get_ray)
 *     if hit.hit:  m = materials[hit.material]
 *                  a = Lambertian, Isotropic, DiffuseLight: textures[m.texture].value(hit.u, hit.v, &hit.p)
 *                      Metal: m.albedo        Dielectric: (1, 1, 1)        Flat / any other kind: (0, 0, 0)
 *                  nrm = hit.normal;  d = hit.t;  k = 1
 *     else:        a = cam->background;  nrm = (0, 0, 0);  d = 0.0;  k = 0
 *     albedo_sum = albedo_sum + a;  normal_sum = normal_sum + nrm;  depth_sum = depth_sum + d;  hit_count += k
 * All four sums start at +0.0 / 0; binary64, every add rounded on its own (no FMA).  So the host composition of rl_rtiow_camera_rays,
 * rl_rtiow_hit_rays_seeded and rl_rtiow_texture_values with a left-to-right fold reproduces every output bit for bit.
 * What follows from the definition:
 *  - Same camera rays as the beauty image: these are the camera rays of rl_rtiow_render_independent* sample for sample, and of the first
 *    sample of every chained render.
 *  - Every first vertex is covered by `a`, the factor the first vertex puts on the path: attenuation where it scatters (a Metal's albedo
 *    whether or not the fuzzed reflection is absorbed), emission where it emits, background where it misses.  beauty / albedo is defined
 *    wherever the beauty is nonzero.
 *  - Normal and depth are the reference's record fields: a ConstantMedium gives normal (1, 0, 0); t is the ray parameter and `dir` is
 *    not normalised.
 *  - A pixel's values depend on nothing but the pixel, F, S, the camera and the scene: row shards and pixel lists give the frame's bits.
 *  - cam->max_depth is not read.
 *  - Sums of calls that continue each other (first_sample) add; the added result is not promised to be bit-equal to one longer call.
 * Layout is that of the plain calls: compact shard rows for _rows and _device ([nrows][W]), out[i] for the lists.  Each pointer of
 * rl_rtiow_features is optional; an output that is not asked for is not written, and the others have the same bits.  The plain forms
 * take host pointers in the struct, the _device forms device pointers and a hipStream_t; those are asynchronous unless opt_stats is given.
 * Errors.  A NULL struct or one whose four pointers are all NULL: RL_E_INVALID, before anything else is looked at (so also without a
 * device), outputs untouched; then, without a device, RL_E_NO_DEVICE (no CPU fallback), outputs untouched; then the plain calls' own
 * rules (a NULL scene or camera, row_step 0, an RTC scene, an empty image: RL_E_INVALID).  Pixel lists follow rl_rtiow_render_pixels*:
 * unsorted, duplicates allowed, n = 0 is RL_OK, the host form refuses a pixel outside the image, the _device form writes zeros to every
 * given output for such an element and traces nothing; n >= 0xFFFF0000: RL_E_INVALID; under rl_init_multi device 0's replica.  A reached
 * panic site sets flagged and returns RL_E_DEGENERATE with every output written.
 * Stats.  With opt_stats all seven counters are the reference's for exactly these S * pixels rays, the nested boundary traces of media
 * included (reference-order trace); rng_words = the words get_ray and the media consumed.  Without it the call is counter-free, may take
 * the fast walk and gives the same bits.  _rows always counts, as rl_rtiow_render_rows does.  rl_render_status covers the asynchronous
 * forms, each call counting once, rays = S * pixels.  Per-scene serialisation as for every render; rl_rtiow_render_progress reports
 * nothing for these calls, as for the independent renders.
 * Not offered: multi-GPU forms, rgb8 output, the RTC family (rl_rtc_prepare_rays on pixel-centre rays already returns point, normal, t
 * and object colour in one call), and features of a chained render's later samples (their camera rays depend on the path before them). */
typedef struct rl_rtiow_features { /* each pointer optional; all NULL: RL_E_INVALID */
  double *albedo_sum;  /* [n][3] */
  double *normal_sum;  /* [n][3] */
  double *depth_sum;   /* [n]    */
  uint32_t *hit_count; /* [n]    */
} rl_rtiow_features;
int rl_rtiow_render_features_rows(const rl_scene *, const rl_rtiow_camera *, uint64_t first_sample, uint32_t row_first, uint32_t row_step,
                                  const rl_rtiow_features *out, rl_stats *opt_stats);
int rl_rtiow_render_features_device(const rl_scene *, const rl_rtiow_camera *, uint64_t first_sample, uint32_t row_first, uint32_t row_step,
                                    const rl_rtiow_features *d_out, void *hip_stream, rl_stats *opt_stats);
int rl_rtiow_render_pixels_features(const rl_scene *, const rl_rtiow_camera *, uint64_t first_sample, const uint32_t *xs, const uint32_t *ys,
                                    uint64_t n, const rl_rtiow_features *out, rl_stats *opt_stats);
int rl_rtiow_render_pixels_features_device(const rl_scene *, const rl_rtiow_camera *, uint64_t first_sample, const void *d_xs, const void *d_ys,
                                           uint64_t n, const rl_rtiow_features *d_out, void *hip_stream, rl_stats *opt_stats);

/* =====================================================================
 *  Ambient-occlusion renders: seeded any-hit rays at first hits
 * =====================================================================
 * One launch traces cam->samples_per_pixel jittered camera rays per pixel to their first hit and sends ao_rays cosine-weighted any-hit
 * rays from each hit.  Let the pixel be (x, y) of the camera's whole W x H frame, F = first_sample, S = cam->samples_per_pixel,
 * K = ao_rays, R = radius.  For s = F, F+1, .., F+S-1, in this order:
 *     rng = ChaCha8Rng::seed_from_u64(cam->seed), set_stream(s*W*H + x*W + y), word position 0
 *     ray = Camera::get_ray(&mut rng, x, y)                  -- camera.rs:203-216, what rl_rtiow_camera_rays returns for that cursor
 *     hit = world.hit(&ray, &Interval{1e-10, +inf})          -- what rl_rtiow_hit_rays returns
 *     if hit:  hit_count += 1
 *              repeat K times:
 *                d = hit.normal + Vec3::random_unit_vector(&mut rng);  if d.near_zero() { d = hit.normal }
 *                                                            -- Lambertian::scatter's direction (material.rs:80-86), whatever the
 *                                                               hit's material
 *                a = d.normalize()                           -- vec3.rs:56: d * (1.0 / d.length()), length_squared as vec3.rs:36-38, no FMA
 *                occluded = world.hit(&Ray{hit.p, a, ray.time}, &Interval{1e-10, R}).is_some()
 *                                                            -- what rl_rtiow_occluded_rays returns
 *                open_count += !occluded
 * The two outputs are uint32_t open_count[n] and uint32_t hit_count[n]; each is optional, an output that is not asked for is not
 * written and the other has the same bits.  Both counts start at 0.  The visibility of a pixel is open_count / (K * hit_count): the
 * cosine weighting of `normal + unit vector` makes that the ambient-occlusion integral.  The ambient ray inherits the camera ray's
 * time, so moving spheres occlude where they are for that sample.  R is a Euclidean distance, because `a` is normalised.
 * What follows from the definition:
 *  - A pixel's values depend on nothing but the pixel, F, S, K, R, the camera and the scene: row shards and pixel lists give the frame's
 *    bits.
 *  - The outputs are integers, so calls that continue each other add EXACTLY: (F = 0, S = 2) + (F = 2, S = 1) equals (F = 0, S = 3).  (The
 *    floating-point sums of the feature renders do not promise this.)
 *  - The camera rays are those of rl_rtiow_render_independent* and rl_rtiow_render_features*, sample for sample.
 *  - cam->max_depth is not read.
 * Layout is that of the feature renders: compact shard rows for _rows and _device ([nrows][W]), out[i] for the lists.  The plain forms
 * take host pointers, the _device forms device pointers and a hipStream_t; those are asynchronous unless opt_stats is given.
 * Errors.  ao_rays == 0, S * ao_rays >= 2^32, a radius that is NaN or <= 0 (+inf is legal), or both outputs NULL: RL_E_INVALID, before a
 * device is looked at, outputs untouched; then, without a device, RL_E_NO_DEVICE (no CPU fallback), outputs untouched; then the plain
 * renders' rules (a NULL scene or camera, row_step 0, an RTC scene, an empty image: RL_E_INVALID).  A scene with ConstantMedium objects:
 * RL_E_UNSUPPORTED, for rl_rtiow_occluded_rays' reason (there is no seeded any-hit).  Pixel lists follow
 * rl_rtiow_render_pixels_features* exactly: unsorted, duplicates allowed, n = 0 is RL_OK, the host form refuses a pixel outside the
 * image, the _device form writes zeros to every given output for such an element and traces nothing; n >= 0xFFFF0000: RL_E_INVALID;
 * under rl_init_multi device 0's replica.  A reached panic site sets flagged and returns RL_E_DEGENERATE with every output written; in
 * the counter-free form this holds with rl_rtiow_occluded_rays' caveat for ambient rays the any-hit walk decides by itself.
 * Stats.  With opt_stats the call is counting and every ray runs the reference-order fold: rays = S * pixels + K * (sum of hit_count);
 * the traversal counters are the sums of what rl_rtiow_hit_rays and rl_rtiow_occluded_rays report for those rays; rng_words = the words
 * get_ray and the K unit-vector draws consumed.  Without it the call is counter-free, may take the fast walks and gives the same bytes.
 * _rows counts or not exactly as rl_rtiow_render_features_rows does (always).  rl_render_status and per-scene serialisation: as the
 * feature renders.
 * Not offered: media scenes, a bent-normal output (a floating-point sum would need an order), a radius per sample, multi-GPU forms,
 * rgb8 output, the RTC family. */
int rl_rtiow_render_ao_rows(const rl_scene *, const rl_rtiow_camera *, uint64_t first_sample, uint32_t row_first, uint32_t row_step, uint32_t ao_rays,
                            double radius, uint32_t *out_open_count, uint32_t *out_hit_count, rl_stats *opt_stats);
int rl_rtiow_render_ao_device(const rl_scene *, const rl_rtiow_camera *, uint64_t first_sample, uint32_t row_first, uint32_t row_step, uint32_t ao_rays,
                              double radius, void *d_out_open_count, void *d_out_hit_count, void *hip_stream, rl_stats *opt_stats);
int rl_rtiow_render_pixels_ao(const rl_scene *, const rl_rtiow_camera *, uint64_t first_sample, const uint32_t *xs, const uint32_t *ys, uint64_t n,
                              uint32_t ao_rays, double radius, uint32_t *out_open_count, uint32_t *out_hit_count, rl_stats *opt_stats);
int rl_rtiow_render_pixels_ao_device(const rl_scene *, const rl_rtiow_camera *, uint64_t first_sample, const void *d_xs, const void *d_ys, uint64_t n,
                                     uint32_t ao_rays, double radius, void *d_out_open_count, void *d_out_hit_count, void *hip_stream,
                                     rl_stats *opt_stats);

/* =====================================================================
 *  Direct-lighting renders: seeded shadow segments to quad lights
 * =====================================================================
 * One launch traces cam->samples_per_pixel jittered camera rays per pixel to their first hit and, from each hit, tests the segments to
 * light_samples points drawn on each of n_lights quad lights with the any-hit query.  A light is 12 doubles, Q[3], u[3], v[3], E[3]: the
 * parallelogram Q + a*u + b*v, a, b in [0,1) (Quad::new(Q, u, v, ..), quad.rs) and its emitted radiance (what DiffuseLight{SolidColor}
 * returns from `emitted`, two-sided as there).  `lights` is [n_lights][12].  For every light nl = u.cross(v) with vec3.rs:48-54's
 * component order, every product rounded, no FMA.  Let the pixel be (x, y) of the camera's whole W x H frame, F = first_sample,
 * S = cam->samples_per_pixel, L = n_lights, K = light_samples, T = seg_tmax.  For s = F, F+1, .., F+S-1, in this order:
 *     rng = ChaCha8Rng::seed_from_u64(cam->seed), set_stream(s*W*H + x*W + y), word position 0     -- as the AO and feature renders
 *     ray = Camera::get_ray(&mut rng, x, y)
 *     hit = world.hit(&ray, &Interval{1e-10, +inf})
 *     if hit:  hit_count += 1
 *       for l in 0..L:  for k in 0..K:
 *          a = rng.gen::<f64>();  b = rng.gen::<f64>()       -- always drawn: 4 words per light sample
 *          yl = (Q + u*a) + v*b
 *          d  = yl - hit.p
 *          d2 = d.x*d.x + d.y*d.y + d.z*d.z                   -- vec3.rs length_squared order
 *          cs = hit.normal.dot(d)                             -- the record's normal (it faces the camera ray), whatever the material
 *          cl = |nl.dot(d)|
 *          if !(cs > 0) or !(cl > 0) or !(d2 > 0):  continue  -- faces away, edge-on or degenerate: nothing traced
 *          g  = (cs * cl) / (d2 * d2)                         -- = cos(theta) cos(theta_l) area / |d|^2: no sqrt and no normalisation
 *          occluded = world.hit(&Ray{hit.p, d, ray.time}, &Interval{1e-10, T}).is_some()      -- what rl_rtiow_occluded_rays returns
 *          for c in r, g, b:  e = E[c] * g;  unshadowed[c] = unshadowed[c] + e;  if !occluded: direct[c] = direct[c] + e
 * Every operation is one rounded binary64 + - x or /.  The outputs are double direct[n][3], double unshadowed[n][3] and
 * uint32_t hit_count[n]; each is optional (not all three), an output that is not asked for is not written and the others have the same
 * bits.  All start at 0.
 *  - direct / (K * hit_count) is the unoccluded irradiance estimate at the first hits.  It is DEMODULATED: no albedo and no 1/pi are
 *    applied; rl_rtiow_render_features' albedo supplies those.  (That also keeps texture evaluation out of the kernel.)
 *  - direct / unshadowed is the shadow ratio of a compositing pass.
 *  - T is in (1e-10, 1].  A light that is also geometry of the scene (cornell_box's) sits at t = 1 of its segments, so such callers pass
 *    T a little under 1.
 * What follows from the definition:
 *  - A pixel's values depend on nothing but the pixel and the call's scalars, lights, camera and scene: row shards and pixel lists give
 *    the frame's bits.
 *  - hit_count of calls that continue each other adds EXACTLY.  The floating-point sums of a continued call are those of THAT call, a
 *    fresh fold from 0, as for the feature renders.
 *  - The camera rays are those of rl_rtiow_render_independent*, rl_rtiow_render_features* and rl_rtiow_render_ao*, sample for sample.
 *  - cam->max_depth is not read.
 *  - The shadow segment inherits the camera ray's time, so moving spheres shadow where they are for that sample.
 * Layout, _device asynchrony, _rows always counting, the pixel-list rules (unsorted, duplicates allowed, n = 0 is RL_OK, the host form
 * refuses a pixel outside the image, the _device form writes zeros to every given output for such an element and traces nothing),
 * rl_init_multi (device 0's replica), rl_render_status and the degenerate flag follow rl_rtiow_render_ao* exactly; direct and
 * unshadowed are laid out [n][3] where the AO counts are [n].  The lights travel by value in the launch: n_lights <=
 * RL_DIRECT_MAX_LIGHTS, and the asynchronous forms keep no pointer of the caller's.
 * Errors.  n_lights == 0 or > RL_DIRECT_MAX_LIGHTS, lights == NULL, light_samples == 0, S * L * K >= 2^32, a light component that is not
 * finite, u x v == 0 (all three components), seg_tmax NaN, <= 1e-10 or > 1, or all three outputs NULL: RL_E_INVALID, before a device is
 * looked at, outputs untouched; then, without a device, RL_E_NO_DEVICE (no CPU fallback), outputs untouched; then the plain renders'
 * rules.  A scene with ConstantMedium objects: RL_E_UNSUPPORTED, for rl_rtiow_occluded_rays' reason (there is no seeded any-hit).
 * Stats.  With opt_stats the call is counting and every ray runs the reference-order fold: rays = S * pixels + (segments traced) — a
 * skipped light sample traces nothing and counts nothing; the traversal counters are the sums of what rl_rtiow_hit_rays and
 * rl_rtiow_occluded_rays report for those rays; rng_words = get_ray's words + 4 * L * K * (sum of hit_count).  Without it the call is
 * counter-free, may take the fast walks and gives the same bytes.
 * Not offered: sphere and textured lights, media scenes, a light picked at random instead of looped, multi-GPU forms, rgb8 output, the
 * RTC family. */
#define RL_DIRECT_MAX_LIGHTS 16u /* 16 x 12 doubles = 1536 bytes of launch arguments */
int rl_rtiow_render_direct_rows(const rl_scene *, const rl_rtiow_camera *, uint64_t first_sample, uint32_t row_first, uint32_t row_step,
                                uint32_t n_lights, const double *lights, uint32_t light_samples, double seg_tmax, double *out_direct,
                                double *out_unshadowed, uint32_t *out_hit_count, rl_stats *opt_stats);
int rl_rtiow_render_direct_device(const rl_scene *, const rl_rtiow_camera *, uint64_t first_sample, uint32_t row_first, uint32_t row_step,
                                  uint32_t n_lights, const double *lights, uint32_t light_samples, double seg_tmax, void *d_out_direct,
                                  void *d_out_unshadowed, void *d_out_hit_count, void *hip_stream, rl_stats *opt_stats);
int rl_rtiow_render_pixels_direct(const rl_scene *, const rl_rtiow_camera *, uint64_t first_sample, const uint32_t *xs, const uint32_t *ys,
                                  uint64_t n, uint32_t n_lights, const double *lights, uint32_t light_samples, double seg_tmax,
                                  double *out_direct, double *out_unshadowed, uint32_t *out_hit_count, rl_stats *opt_stats);
int rl_rtiow_render_pixels_direct_device(const rl_scene *, const rl_rtiow_camera *, uint64_t first_sample, const void *d_xs, const void *d_ys,
                                         uint64_t n, uint32_t n_lights, const double *lights, uint32_t light_samples, double seg_tmax,
                                         void *d_out_direct, void *d_out_unshadowed, void *d_out_hit_count, void *hip_stream,
                                         rl_stats *opt_stats);

/* =====================================================================
 *  NEE path renders: ray_color with shadow segments to quad lights
 * =====================================================================
 * One launch traces cam->samples_per_pixel paths per pixel, Camera::ray_color (camera.rs:232-260) with next-event estimation: every
 * Lambertian vertex but the last connects to light_samples points drawn on each of n_lights quad lights with the direct-lighting renders'
 * draws, geometry term and any-hit segment test, and in exchange the emission its scattered ray finds is not counted.  A light is the
 * direct-lighting renders' 12 doubles Q, u, v, E; `lights` is [n_lights][12], nl = u.cross(v) as there.  Let the pixel be (x, y) of the
 * camera's whole W x H frame, F = first_sample, S = cam->samples_per_pixel, L = n_lights, K = light_samples, T = seg_tmax,
 * kf = 1.0 / (M_PI * (double)K) (one rounded product, one rounded quotient; computed once on the host).  For s = F, F+1, .., F+S-1, in
 * this order:
 *     rng = ChaCha8Rng::seed_from_u64(cam->seed), set_stream(s*W*H + x*W + y), word position 0     -- as the AO and direct renders
 *     ray = Camera::get_ray(&mut rng, x, y);  time = ray.time
 *     c = (0,0,0);  thr = (1,1,1);  count_emission = true
 *     for i in 1 ..= cam->max_depth:
 *       1. hit = world.hit(&ray, &Interval{1e-10, +inf});   if none:  c = c + thr * cam->background;  break
 *       2. em = hit.mat.emitted(hit.u, hit.v, &hit.p);      if count_emission:  c = c + thr * em
 *       3. if hit.mat is RL_MAT_LAMBERTIAN and i < cam->max_depth:
 *            tex = the material's texture value at the hit     -- the attenuation `scatter` will return
 *            dsum = (0,0,0)
 *            for l in 0..L:  for k in 0..K:
 *               a = rng.gen::<f64>();  b = rng.gen::<f64>()       -- always drawn: 4 words per light sample
 *               yl = (Q + u*a) + v*b;  d = yl - hit.p
 *               d2 = d.x*d.x + d.y*d.y + d.z*d.z;  cs = hit.normal.dot(d);  cl = |nl.dot(d)|
 *               if !(cs > 0) or !(cl > 0) or !(d2 > 0):  continue  -- faces away, edge-on or degenerate: nothing traced
 *               g = (cs * cl) / (d2 * d2)
 *               if world.hit(&Ray{hit.p, d, time}, &Interval{1e-10, T}).is_none():
 *                  for ch in r, g, b:  dsum[ch] = dsum[ch] + E[ch] * g
 *            for ch in r, g, b:  c[ch] = c[ch] + ((thr[ch] * tex[ch]) * dsum[ch]) * kf
 *       4. match hit.mat.scatter(&mut rng, &ray, &hit):        -- drawing AFTER the light points
 *            None:  break
 *            Some((scattered, attenuation)):  thr = thr * attenuation;  ray = scattered;  count_emission = (step 3 was not taken)
 *     for ch in r, g, b:  sums[ch] = sums[ch] + c[ch];  sq[ch] = sq[ch] + c[ch] * c[ch]
 * Every operation is one rounded binary64 + - x or /.  The outputs are double sums[n][3] and double sq[n][3], what
 * rl_rtiow_render_moments_rows gives for the plain path; each is optional (not both), an output that is not asked for is not written
 * and the other has the same bits.  Both start at 0.
 * What follows from the definition:
 *  - Step 3's `i < max_depth` makes the estimator's expectation equal to ray_color's at the same max_depth: a connection made at vertex
 *    i stands for the emission plain path tracing would find at vertex i+1.  This holds PROVIDED `lights` LISTS EVERY DiffuseLight
 *    SURFACE OF THE SCENE (as quads with a SolidColor emission).  An emitter that is not listed is seen only directly and through Metal,
 *    Dielectric, Isotropic and Flat chains; a light that is listed but is not geometry of the scene lights Lambertian surfaces and is
 *    never seen.  The background is always counted on a miss.
 *  - Isotropic vertices do no light sampling (a phase function needs 1/|d|^3, hence a sqrt).  The Dielectric's panic site (a zero
 *    direction, material.rs:150-151) is flagged and behaves as in rl_rtiow_scatter_rays.
 *  - A pixel's values depend on nothing but the pixel and the call's scalars, lights, camera and scene: row shards and pixel lists give
 *    the frame's bits.  sums and sq of calls that continue each other are added by the caller, as for rl_rtiow_render_moments_rows.
 *  - The camera rays are those of rl_rtiow_render_independent* and of the feature, AO and direct-lighting renders, sample for sample.
 *  - Segments and scattered rays inherit the camera ray's time.
 * Layout, _device asynchrony, _rows always counting, the pixel-list rules, rl_init_multi, rl_render_status and the degenerate flag
 * follow rl_rtiow_render_direct* exactly.
 * Errors.  The direct-lighting renders' rules on n_lights, lights, light_samples, S * L * K and seg_tmax, cam->max_depth == 0, or both
 * outputs NULL: RL_E_INVALID, before a device is looked at, outputs untouched; then, without a device, RL_E_NO_DEVICE (no CPU
 * fallback); then the plain renders' rules.  A scene with ConstantMedium objects: RL_E_UNSUPPORTED (there is no seeded any-hit).
 * Stats.  With opt_stats the call is counting and every ray runs the reference-order fold: rays = path rays + segments traced; the
 * traversal counters are the sums of what rl_rtiow_hit_rays and rl_rtiow_occluded_rays report for those rays; rng_words = the words
 * drawn (get_ray's, 4 per light sample, the scatters').  Without it the call is counter-free, may take the fast walks and gives the
 * same bytes.
 * Not offered: sphere and textured lights, media scenes, Russian roulette, adaptive stopping, multi-GPU forms, rgb8 output, the RTC
 * family.  Multiple importance sampling with the scattered ray is the next section's rl_rtiow_render_nee_mis*. */
int rl_rtiow_render_nee_rows(const rl_scene *, const rl_rtiow_camera *, uint64_t first_sample, uint32_t row_first, uint32_t row_step,
                             uint32_t n_lights, const double *lights, uint32_t light_samples, double seg_tmax, double *out_sums, double *out_sq,
                             rl_stats *opt_stats);
int rl_rtiow_render_nee_device(const rl_scene *, const rl_rtiow_camera *, uint64_t first_sample, uint32_t row_first, uint32_t row_step,
                               uint32_t n_lights, const double *lights, uint32_t light_samples, double seg_tmax, void *d_out_sums, void *d_out_sq,
                               void *hip_stream, rl_stats *opt_stats);
int rl_rtiow_render_pixels_nee(const rl_scene *, const rl_rtiow_camera *, uint64_t first_sample, const uint32_t *xs, const uint32_t *ys,
                               uint64_t n, uint32_t n_lights, const double *lights, uint32_t light_samples, double seg_tmax, double *out_sums,
                               double *out_sq, rl_stats *opt_stats);
int rl_rtiow_render_pixels_nee_device(const rl_scene *, const rl_rtiow_camera *, uint64_t first_sample, const void *d_xs, const void *d_ys,
                                      uint64_t n, uint32_t n_lights, const double *lights, uint32_t light_samples, double seg_tmax,
                                      void *d_out_sums, void *d_out_sq, void *hip_stream, rl_stats *opt_stats);

/* =====================================================================
 *  NEE path renders with multiple importance sampling: weighted light and scattered-ray samples
 * =====================================================================
 * The NEE path renders above with one more argument, `heuristic`: RL_MIS_BALANCE or RL_MIS_POWER (exponent 2).  A vertex that samples
 * the lights now has TWO strategies for the listed lights' contribution: the light points, and its own scattered ray where that ray
 * crosses a light's parallelogram.  Each is weighted by its density's share of the pair.  For a Lambertian vertex that share needs no
 * sqrt: with p_bsdf = cos(theta) / pi, p_light = |d|^2 / (A cos(theta_l)) and kf = 1 / (pi K), the ratio p_bsdf / (K p_light) is
 * exactly q = g * kf, g the geometry term the light points already form.  The draws, the path, the `i < max_depth` rule,
 * count_emission and the outputs are the NEE path renders'; what is NEW is marked.  With the names of that definition:
 *       3. if hit.mat is RL_MAT_LAMBERTIAN and i < cam->max_depth:
 *            ... a, b, yl, d, d2, cs, cl, the skip and g = (cs * cl) / (d2 * d2) as there, then
 *               NEW  if !(g < +inf):  continue                                    -- not traced
 *               NEW  q = g * kf
 *               NEW  RL_MIS_BALANCE:  wl = g / (1.0 + q)         RL_MIS_POWER:  wl = g / (1.0 + q*q)
 *               if world.hit(&Ray{hit.p, d, time}, &Interval{1e-10, T}).is_none():
 *                  for ch in r, g, b:  dsum[ch] = dsum[ch] + E[ch] * wl             -- wl in g's place
 *            for ch in r, g, b:  c[ch] = c[ch] + ((thr[ch] * tex[ch]) * dsum[ch]) * kf
 *       4. match hit.mat.scatter(&mut rng, &ray, &hit):
 *            None:  break
 *            Some((scattered, attenuation)):  thr = thr * attenuation
 *               NEW  if step 3 was taken:                                           -- draws nothing
 *                      x = hit.p;  n = hit.normal;  w = scattered.direction         -- as rl_rtiow_scatter_rays returns it, not normalised
 *                      bsum = (0,0,0)
 *                      for l in 0..L:
 *                         den = nl.dot(w);                          if !(|den| > 0):  continue
 *                         r = Q - x;  t = nl.dot(r) / den;          if !(t > 0) or !(t < +inf):  continue
 *                         d = w * t;  y = x + d;  h = y - Q
 *                         nn = nl.dot(nl);  al = nl.dot(h.cross(v)) / nn;  be = nl.dot(u.cross(h)) / nn
 *                         if !(0 <= al <= 1) or !(0 <= be <= 1):  continue                     -- beside the parallelogram
 *                         d2 = d.dot(d);  cs = n.dot(d);  cl = |nl.dot(d)|
 *                         if !(cs > 0) or !(cl > 0) or !(d2 > 0):  continue
 *                         g = (cs * cl) / (d2 * d2);                if !(g < +inf):  continue
 *                         q = g * kf
 *                         RL_MIS_BALANCE:  wb = q / (1.0 + q)       RL_MIS_POWER:  wb = (q*q) / (1.0 + q*q)
 *                         if world.hit(&Ray{x, d, time}, &Interval{1e-10, T}).is_none():
 *                            for ch in r, g, b:  bsum[ch] = bsum[ch] + E[ch] * wb
 *                      for ch in r, g, b:  c[ch] = c[ch] + thr[ch] * bsum[ch]
 *               ray = scattered;  count_emission = (step 3 was not taken)
 * a.dot(b) is (a.x*b.x + a.y*b.y) + a.z*b.z and cross is vec3.rs:48-54's, every product rounded; every line is one rounded binary64
 * + - x or /.  The segment of a scattered ray is tested exactly as a light point's is (the same any-hit query, the same T) and is counted
 * in `rays`.
 * What follows from the definition:
 *  - Both strategies estimate the listed lights' contribution THROUGH THE SEGMENT TEST, and wl * kf / (g * kf) + wb = 1, so the
 *    expectation is the NEE path renders' for ANY `lights`, whether or not they are geometry of the scene; with every emitter listed it
 *    is ray_color's.  The emission a scattered ray finds after step 3 stays uncounted, as there.
 *  - wl * kf <= 1 and wb <= 1: one weighted light sample adds at most thr * tex * E and the scattered-ray term at most thr * E per light,
 *    however close the light point is.  What uniform area sampling lets grow without bound (g, where a light is near a surface) is
 *    capped.  It does NOT lower the variance everywhere: away from a light at small K the rare scattered ray that reaches it adds a
 *    little noise of its own (DESIGN.md §3.23 has the measurements).
 *  - rng_words equals the NEE path renders' for the same arguments (the new strategy draws nothing); rays = theirs + the scattered-ray
 *    segments traced.  The path itself (every closest hit, every scatter) is theirs.
 *  - The two heuristics give different bytes; neither gives the NEE path renders' bytes unless no light point counts and no scattered
 *    ray crosses a light.
 * Everything else (outputs, layout, _device asynchrony, _rows always counting, the pixel-list rules, stats, rl_render_status) follows
 * rl_rtiow_render_nee* exactly.
 * Errors.  The NEE path renders' rules, or heuristic > RL_MIS_POWER: RL_E_INVALID, before a device is looked at, outputs untouched; then
 * as there.
 * Not offered: textured lights, media scenes, Isotropic vertices (no light sampling, as there), Russian roulette, adaptive
 * stopping, multi-GPU forms, rgb8 output, the RTC family.  (Sphere lights: the next block.) */
#define RL_MIS_BALANCE 0u
#define RL_MIS_POWER 1u
int rl_rtiow_render_nee_mis_rows(const rl_scene *, const rl_rtiow_camera *, uint64_t first_sample, uint32_t row_first, uint32_t row_step,
                                 uint32_t n_lights, const double *lights, uint32_t light_samples, double seg_tmax, uint32_t heuristic,
                                 double *out_sums, double *out_sq, rl_stats *opt_stats);
int rl_rtiow_render_nee_mis_device(const rl_scene *, const rl_rtiow_camera *, uint64_t first_sample, uint32_t row_first, uint32_t row_step,
                                   uint32_t n_lights, const double *lights, uint32_t light_samples, double seg_tmax, uint32_t heuristic,
                                   void *d_out_sums, void *d_out_sq, void *hip_stream, rl_stats *opt_stats);
int rl_rtiow_render_pixels_nee_mis(const rl_scene *, const rl_rtiow_camera *, uint64_t first_sample, const uint32_t *xs, const uint32_t *ys,
                                   uint64_t n, uint32_t n_lights, const double *lights, uint32_t light_samples, double seg_tmax,
                                   uint32_t heuristic, double *out_sums, double *out_sq, rl_stats *opt_stats);
int rl_rtiow_render_pixels_nee_mis_device(const rl_scene *, const rl_rtiow_camera *, uint64_t first_sample, const void *d_xs,
                                          const void *d_ys, uint64_t n, uint32_t n_lights, const double *lights, uint32_t light_samples,
                                          double seg_tmax, uint32_t heuristic, void *d_out_sums, void *d_out_sq, void *hip_stream,
                                          rl_stats *opt_stats);

/* =====================================================================
 *  NEE path renders with sphere lights: a second light shape for the renders with multiple importance sampling
 * =====================================================================
 * The renders with multiple importance sampling above with a second light array behind `lights`:
 *    n_sphere_lights, sphere_lights [Ls][7] = C[3], r, E[3]
 * A sphere light is stationary, has its centre at C and radius r > 0, and emits E OUTWARD ONLY.  It is sampled uniformly by area with
 * rand_distr's UnitSphere (Marsaglia's draw, the one Lambertian::scatter takes from the same stream: two Uniform(-1, 1) per try, tries
 * until x1^2 + x2^2 < 1, one sqrt).  On the host, once per light: A = (4.0 * M_PI) * (r * r).  With cl carrying A the way a quad's
 * |nl . d| carries |u x v|, q = g * kf is again exactly p_bsdf / (K p_light): no sqrt in the weights.
 * Everything is the MIS definition's except what is named here.  With its names (x = hit.p, n = hit.normal, w = scattered.direction):
 *   Step 3, the light strategy.  Behind the L quads (unchanged), for each sphere light j in 0..Ls, K times:
 *        wu = UnitSphere.sample(rng)                            -- rng.unit_sphere(): 4 words per try, drawn whether or not the point counts
 *        yl = C + wu * r;  d = yl - x;  d2 = d.dot(d);  cs = n.dot(d);  co = -(wu.dot(d));  cl = co * A
 *        if !(cs > 0) or !(co > 0) or !(d2 > 0):  continue       -- not traced
 *        g = (cs * cl) / (d2 * d2);                  if !(g < +inf):  continue
 *        q, wl, the segment test and dsum as there.
 *   Step 4, the scattered-ray strategy.  Behind the quads' candidates, one candidate per sphere light, no draw:
 *        oc = x - C;  a = w.dot(w);  hb = oc.dot(w);  cc = oc.dot(oc) - r * r;  disc = hb * hb - a * cc      -- Sphere::hit's order
 *        if !(disc > 0):  continue
 *        sd = sqrt(disc);  t = (-hb - sd) / a                    -- the near root only
 *        if !(t > 0) or !(t < +inf):  continue
 *        d = w * t;  y = x + d;  wn = (y - C) / r;  co = -(wn.dot(d));  cl = co * A             -- three divisions by r
 *        d2, cs, the same skip, g, q and wb; the same segment test, counted in `rays`; a free segment adds E * wb to bsum.
 * Every line is one rounded binary64 + - x /, or sqrt where named; the negations are exact.
 * What follows from the definition:
 *  - Both strategies estimate the OUTWARD emission of the listed sphere through the segment test, and wl / g + wb = 1 at a crossing: the
 *    expectation is ray_color's at the same max_depth where `lights` and `sphere_lights` together list every DiffuseLight surface (the
 *    reference's simple_light with its quad and its sphere listed), for sphere lights that are geometry of the scene or not.
 *  - Points on the far side of a sphere have co <= 0: they cost their draws but no trace (about half of them, seen from far away).
 *  - A vertex INSIDE a listed sphere gets nothing from it by either strategy (every point faces away; the near root is behind the
 *    vertex).  The reference's DiffuseLight emits from both sides of its surface, so for that one configuration the expectation differs.
 *  - wl * kf <= 1 and wb <= 1: the MIS renders' cap holds with L + Ls in L's place, no sample exceeds
 *    max(background) + Emax * (1 + (max_depth - 1) * (L + Ls) * (K + 1)) for textures and albedos <= 1.
 *  - rng_words has no closed form any more: the tries of a sphere point vary.  rays = path rays + every segment traced.
 * Arguments.  n_lights may be 0; 1 <= n_lights + n_sphere_lights <= RL_DIRECT_MAX_LIGHTS (the two kinds share the slots).
 * With n_sphere_lights == 0 a call IS the MIS call of the same form: the same kernels, bytes and counters.
 * Errors.  RL_E_INVALID before a device is looked at, outputs untouched: a total of 0 or above RL_DIRECT_MAX_LIGHTS, a null array with a
 * nonzero count, a component that is not finite, !(r > 0), A not finite, S * (L + Ls) * K >= 2^32, and the MIS renders' rules; then as
 * there (RL_E_NO_DEVICE, the renders' rules, RL_E_UNSUPPORTED on media scenes).
 * Not offered: sphere lights for the direct-lighting and the plain NEE renders (uniform area sampling without weights has their tail),
 * visible-cap or cone sampling, moving centres, textured lights, two-sided spheres, media scenes, and what the MIS renders do not offer. */
int rl_rtiow_render_nee_mis_spheres_rows(const rl_scene *, const rl_rtiow_camera *, uint64_t first_sample, uint32_t row_first,
                                         uint32_t row_step, uint32_t n_lights, const double *lights, uint32_t n_sphere_lights,
                                         const double *sphere_lights, uint32_t light_samples, double seg_tmax, uint32_t heuristic,
                                         double *out_sums, double *out_sq, rl_stats *opt_stats);
int rl_rtiow_render_nee_mis_spheres_device(const rl_scene *, const rl_rtiow_camera *, uint64_t first_sample, uint32_t row_first,
                                           uint32_t row_step, uint32_t n_lights, const double *lights, uint32_t n_sphere_lights,
                                           const double *sphere_lights, uint32_t light_samples, double seg_tmax, uint32_t heuristic,
                                           void *d_out_sums, void *d_out_sq, void *hip_stream, rl_stats *opt_stats);
int rl_rtiow_render_pixels_nee_mis_spheres(const rl_scene *, const rl_rtiow_camera *, uint64_t first_sample, const uint32_t *xs,
                                           const uint32_t *ys, uint64_t n, uint32_t n_lights, const double *lights, uint32_t n_sphere_lights,
                                           const double *sphere_lights, uint32_t light_samples, double seg_tmax, uint32_t heuristic,
                                           double *out_sums, double *out_sq, rl_stats *opt_stats);
int rl_rtiow_render_pixels_nee_mis_spheres_device(const rl_scene *, const rl_rtiow_camera *, uint64_t first_sample, const void *d_xs,
                                                  const void *d_ys, uint64_t n, uint32_t n_lights, const double *lights,
                                                  uint32_t n_sphere_lights, const double *sphere_lights, uint32_t light_samples,
                                                  double seg_tmax, uint32_t heuristic, void *d_out_sums, void *d_out_sq, void *hip_stream,
                                                  rl_stats *opt_stats);

/* =====================================================================
 *  Denoising: an edge-avoiding a-trous filter for noisy and adaptive renders
 * =====================================================================
 * What consumes the mean and variance of the moments and adaptive renders and the guide buffers of the feature renders.  It needs no scene.
 * One pass.  All images are row-major f64: color [H][W][3], variance [H][W][3] (the variance of each pixel mean, >= 0), guides [H][W][G]
 * with 0 <= G <= 8 (G = n_guides).  Parameters: color_sigma2 >= 0, variance_floor >= DBL_MIN, guide_inv_sigma[G] >= 0 where 0 switches a guide
 * off, step >= 1.  Let h = [1/16, 1/4, 3/8, 1/4, 1/16].  For pixel p = (x, y), visit the 25 taps q = (x + i*step, y + j*step) with
 * j = -2..2 outer and i = -2..2 inner.  Skip taps outside the image.  Every operation is rounded separately and sums run left to right:
 *     vsum(r) = (var_r[0] + var_r[1]) + var_r[2]
 *     d       = color_p - color_q ;  d2 = (d0*d0 + d1*d1) + d2*d2
 *     D       = color_sigma2 * (vsum(p) + vsum(q)) + variance_floor
 *     xg      = 0 ; for k in 0..G-1: e = (guide_p[k] - guide_q[k]) * guide_inv_sigma[k] ; xg = xg + e*e
 *     w       = ((h[j+2]*h[i+2]) * D) / ((D + d2) * (1.0 + xg))
 *     sw      = sw + w ;  ac[c] = ac[c] + w * color_q[c] ;  av[c] = av[c] + (w*w) * var_q[c]
 *     out_color[c] = ac[c] / sw ;  out_variance[c] = av[c] / (sw*sw)
 * sw, ac and av start at +0.0.  Binary64 throughout, + - * / only, no FMA, no libm call: the weights are Cauchy-type, 1 / (1 + x), in
 * place of the usual exp(-x), so a host that follows the statement gets every output bit (tests/atrous_model.py does).  One division per tap.
 * What follows from the definition:
 *  - variance_floor is finite and a normal number (>= DBL_MIN), so D >= DBL_MIN wherever it is finite; there the centre tap has
 *    w = (9/64 * D) / (D * 1) > 0, so sw > 0 wherever D is finite, a 1 x 1 image included.  (A subnormal floor is refused because it
 *    breaks this: with 5e-324 on a flat image without variance, 9/64 * D rounds to 0, sw = 0 and every output is 0 / 0.)
 *  - With finite inputs and color_sigma2 * (vsum(p) + vsum(q)) + variance_floor finite for every pair of a pixel and a tap, every output
 *    is finite: an overflowing d2 or xg only takes that tap's w to 0.  (Two provisos at the very edge of the range: a guide difference that
 *    itself overflows under guide_inv_sigma[k] = 0 is inf * 0, and colours within a few ulps of DBL_MAX can round ac up to inf.)
 *  - Where D overflows to +inf (finite variances whose scaled sum exceeds DBL_MAX), that tap's w is inf / inf = NaN, and sw and every
 *    output of that pixel are NaN.  No input is scanned for this either.
 *  - Non-finite inputs give non-finite outputs in the pixels whose footprint (the 25 taps) they touch, and in no other pixel.  No input is
 *    scanned.
 *  - A guide with guide_inv_sigma[k] = 0 leaves every bit as the call without that channel has it (finite guides: e = +-0, xg + 0 = xg).
 *  - A pass is not in place: every pixel reads its neighbours' inputs.
 * rl_denoise_atrous_pass_device enqueues ONE pass on the caller's stream and returns: asynchronous, device pointers, owns no device memory.
 * rl_denoise_atrous takes host arrays, stages them and runs `iterations` passes with step = 1, 2, .., 2^(iterations-1), each reading the
 * colour and variance the one before wrote (the guides stay), ping-ponging between two staged pairs, and copies the last pass's outputs
 * back; iterations = 0 copies the inputs through.  d_out_variance / out_variance may be NULL (the colour bytes are the same); d_guides /
 * guides may be NULL when n_guides = 0 and is not read then.  guide_inv_sigma[k] for k >= n_guides is not read.
 * Errors.  RL_E_INVALID, before the device is looked at (so also without one), nothing written: NULL params, colour, variance or colour
 * output; NULL guides with n_guides > 0; n_guides > 8; reserved != 0; variance_floor not finite and a normal number (below DBL_MIN: 0, subnormal); a non-finite or negative color_sigma2,
 * variance_floor or guide_inv_sigma[k < n_guides]; step = 0 or step > 1 << 20; iterations > 12; an output pointer equal to an input
 * pointer or to the other output; width * height >= 0xFFFF0000.  Then, without a device, RL_E_NO_DEVICE (no CPU fallback).  Then a
 * zero-area image: RL_OK, nothing read or written.  The device form runs on the current device; the host form on the library's device 0.
 * Not offered: f32 images, temporal accumulation, a variance pre-filter, multi-GPU forms. */
typedef struct rl_atrous_params {
  double color_sigma2;       /* >= 0: how many variances of colour difference halve a tap's weight */
  double variance_floor;     /* finite and a normal number, >= DBL_MIN: keeps D positive where both variances are 0 */
  uint32_t n_guides;         /* G, 0 .. 8 */
  uint32_t reserved;         /* 0 */
  double guide_inv_sigma[8]; /* 1 / sigma of guide channel k; 0: that guide is off */
} rl_atrous_params;          /* 88 bytes */
int rl_denoise_atrous_pass_device(uint32_t width, uint32_t height, uint32_t step, const rl_atrous_params *, const void *d_color,
                                  const void *d_variance, const void *d_guides, void *d_out_color, void *d_out_variance, void *hip_stream);
int rl_denoise_atrous(uint32_t width, uint32_t height, uint32_t iterations, const rl_atrous_params *, const double *color,
                      const double *variance, const double *guides, double *out_color, double *out_variance);

/* From the renders' buffers to a denoised picture without leaving the device: prepare, the passes, finish.
 * prepare turns sums, second moments and counts (moments / adaptive renders) and the feature sums into the colour, variance and guide
 * images a pass reads; finish multiplies the filtered images back by the albedo and can encode the picture.  Binary64, every operation
 * rounded on its own (no FMA), sums left to right, uint32 inputs converted exactly; sqrt is the correctly rounded one.  Per pixel p and
 * channel c (tests/denoise_render_model.py is this statement in numpy; api.denoise_render computes the same bytes on the host):
 *     n        = (double)counts[p]  if a counts image is given, else (double)samples
 *     mean[c]  = sums[c] / n  with counts;  sums[c] * (1.0 / samples)  without (the reciprocal is one rounded division)
 *     raw[c]   = (((sq[c] - (sums[c] * sums[c]) / n) / (n - 1.0)) / n)
 *     var[c]   = raw[c] < 0 ? 0.0 : raw[c]                     -- a NaN stays NaN
 *     alb[c]   = albedo_sum[c] * (1.0 / feature_samples)
 *     a[c]     = alb[c] > 0 ? alb[c] : 1.0                     -- zero, negative and NaN albedo: the colour is left as it is
 *     color[c] = mean[c] / a[c] ;  variance[c] = var[c] / (a[c] * a[c])
 *     guides [H][W][G], in this fixed order, each group present iff its RL_GUIDE_* bit of `want` is set:
 *       albedo (3):   alb[c]
 *       normal (3):   l = sqrt((ns0*ns0 + ns1*ns1) + ns2*ns2) ;  l != 0 ? ns[c] / l : 0.0
 *       depth (1):    depth_sum / (double)max(hit_count, 1)
 *       coverage (1): (double)hit_count / (double)feature_samples
 *   finish:  out_color[c] = color_f[c] * a[c] ;  out_variance[c] = variance_f[c] * (a[c] * a[c])   -- a recomputed from albedo_sum, not stored
 *            out_rgb8[c]  = the byte of rl_rtiow_encode_rgb8_device(out_color, n, samples = 1)
 * No input is scanned.  A pixel whose count is 0 or 1 gets the non-finite values the arithmetic gives (x / 0, 0 / 0); the passes spread
 * them to the pixels whose 25-tap footprints touch it and no further (above).
 * rl_denoise_prepare_device and rl_denoise_finish_device enqueue one elementwise kernel each on the caller's stream and return.  finish's
 * outputs may be its inputs (d_out_color = d_color, d_out_variance = d_variance); d_variance is read iff d_out_variance is given; each of
 * its three outputs is optional, one at least must be given.  d_guides may be NULL when want = 0.
 * rl_denoise_render_device enqueues prepare, `iterations` passes at step 1, 2, 4, .. (rl_denoise_atrous_pass_device) and finish on the
 * caller's stream and returns without waiting.  It owns no memory: two colour / variance pairs and the guide image are carved from d_work,
 * rl_denoise_render_work_bytes(width, height, G) bytes, whose contents before and after the call mean nothing.  iterations = 0 runs prepare
 * and finish only.  d_out_variance and d_out_rgb8 are optional, d_out_color too when one of the others is given; the last pass writes no
 * variance when nobody wants one, and the colour bytes are the same.  rl_denoise_render takes host arrays in the struct and the outputs,
 * stages them on the library's device 0 and waits.
 * Errors.  RL_E_INVALID, before the device is looked at (so also without one), nothing written: a NULL struct; NULL sums, sq or
 * albedo_sum; a pointer that a `want` bit needs is missing; `want` with bits beyond the four; reserved != 0; feature_samples = 0;
 * counts = NULL with samples < 2; params->n_guides != G; whatever the params of a pass are refused for (above); iterations > 12;
 * work_bytes too small (or a NULL d_work); no output at all; the two f64 outputs one buffer; width * height >= 0xFFFF0000.  Then,
 * without a device, RL_E_NO_DEVICE (no CPU fallback).  Then a zero-area image: RL_OK, nothing read or written.
 * rl_rtiow_render_denoised_rgb8 is the sibling of rl_rtiow_render_rgb8, one call from scene to picture: rl_rtiow_render_adaptive_device
 * with opt_rule (rl_rtiow_render_moments_device when it is NULL), rl_rtiow_render_features_device with a copy of the camera whose
 * samples_per_pixel is feature_samples, and rl_denoise_render_device, all on the library's stream (first_sample 0, the whole frame), then
 * W*H*3 bytes copied back.  What rl_denoise_render_device refuses is refused before anything is rendered; after that the first non-OK
 * code of a composed call is returned, and every rule of the scene, the camera and concurrency is the composed calls' own.  The two
 * renders are asynchronous, so the call ends with rl_render_status(scene): RL_E_DEGENERATE, with the picture written, when a panic site
 * was reached.  It takes no stats.
 * Not offered: row shards, pixel lists and multi-GPU forms of the one-call render; f32 images. */
#define RL_GUIDE_ALBEDO 1u   /* 3 channels */
#define RL_GUIDE_NORMAL 2u   /* 3 channels */
#define RL_GUIDE_DEPTH 4u    /* 1 channel  */
#define RL_GUIDE_COVERAGE 8u /* 1 channel  */
typedef struct rl_denoise_inputs { /* pointers: device in the _device forms, host in rl_denoise_render */
  const void *sums;                /* [H][W][3] f64 */
  const void *sq;                  /* [H][W][3] f64 */
  const void *counts;              /* [H][W] u32 (adaptive) or NULL: every pixel took `samples` */
  const void *albedo_sum;          /* [H][W][3] f64, required: the colour is divided by its mean */
  const void *normal_sum;          /* [H][W][3] f64, needed iff want has RL_GUIDE_NORMAL */
  const void *depth_sum;           /* [H][W] f64, needed iff want has RL_GUIDE_DEPTH */
  const void *hit_count;           /* [H][W] u32, needed iff want has RL_GUIDE_DEPTH or RL_GUIDE_COVERAGE */
  uint32_t samples;                /* read iff counts == NULL; then >= 2 */
  uint32_t feature_samples;        /* >= 1: samples_per_pixel of the feature render */
  uint32_t want;                   /* RL_GUIDE_* bits; G = 3*albedo + 3*normal + depth + coverage */
  uint32_t reserved;               /* 0 */
} rl_denoise_inputs;               /* 72 bytes */
int rl_denoise_prepare_device(uint32_t width, uint32_t height, const rl_denoise_inputs *, void *d_color, void *d_variance, void *d_guides,
                              void *hip_stream);
int rl_denoise_finish_device(uint32_t width, uint32_t height, const void *d_color, const void *d_variance, const void *d_albedo_sum,
                             uint32_t feature_samples, void *d_out_color, void *d_out_variance, void *d_out_rgb8, void *hip_stream);
uint64_t rl_denoise_render_work_bytes(uint32_t width, uint32_t height, uint32_t n_guides); /* width * height * 8 * (12 + n_guides) */
int rl_denoise_render_device(uint32_t width, uint32_t height, const rl_denoise_inputs *, uint32_t iterations, const rl_atrous_params *,
                             void *d_work, uint64_t work_bytes, void *d_out_color, void *d_out_variance, void *d_out_rgb8, void *hip_stream);
int rl_denoise_render(uint32_t width, uint32_t height, const rl_denoise_inputs *, uint32_t iterations, const rl_atrous_params *,
                      double *out_color, double *out_variance, uint8_t *out_rgb8);
int rl_rtiow_render_denoised_rgb8(const rl_scene *, const rl_rtiow_camera *, const rl_rtiow_adaptive *opt_rule, uint32_t feature_samples,
                                  uint32_t want, uint32_t iterations, const rl_atrous_params *, uint8_t *out_rgb8);

/* =====================================================================
 *  Batched ray queries: the reference's per-ray primitives on the device
 * =====================================================================
 *   rl_rtiow_hit_rays*      <- ray-tracing-one-weekend/src/hittable/mod.rs:42  Hittable::hit(&Ray, &Interval) -> Option<(&Material, HitRecord)>
 *                              on the scene root (the slice fold hittable/mod.rs:88-111, Bvh::hit bvh.rs:79-95, ...)
 *   rl_rtc_intersect_rays*  <- ray-tracer-challenge/src/scene/world.rs:46  World::intersect, scene/intersect.rs:159-168  hit
 *   rl_rtc_color_at_rays*   <- ray-tracer-challenge/src/scene/world.rs:100 World::color_at(&Ray)
 * Rays are plain records, used as given: `dir` is NOT normalised (the reference does not normalise either).  The plain forms take
 * host buffers; the _device forms take device buffers and a hipStream_t and are asynchronous unless opt_stats is non-NULL.
 * opt_stats counts as a render does: rays = the queried rays (color_at: + the reflection / refraction / shadow rays, as rl_rtc_render);
 * a reached panic site sets flagged and returns RL_E_DEGENERATE with every output written; rl_render_status covers the asynchronous
 * forms, each query counting once.  n = 0: RL_OK, no buffer is touched (opt_stats, when given, is zeroed).  NULL buffers with n > 0, a
 * NaN interval bound, a scene of the other family: RL_E_INVALID.  Concurrency: as the renders (serialised per scene).  Under
 * rl_init_multi the query runs on device 0's replica (a batch is not split across GPUs).
 * Results, and all counters, are those of the reference's algorithm on the same ray.  rl_rtiow_hit_rays* without opt_stats and with
 * tmin == 1e-10 (camera.rs:242-245) may be served by a fast tree walk that re-traces every order-sensitive ray: the records are bit for bit
 * those of the reference-order kernel.  A zero `dir` reaches no panic site (Sphere::hit: a = 0, NaN roots, no hit; RTC: no intersection). */
typedef struct rl_ray { /* ray.rs:5-9 Ray{origin, direction, time} / RTC ray.rs Ray{origin, direction} */
  double origin[3], dir[3];
  double time; /* RTIOW only (moving spheres, sphere.rs:36); ignored by the RTC queries */
} rl_ray;      /* 56 bytes */
typedef struct rl_rtiow_hit { /* hittable/mod.rs:24-30 HitRecord + the &Material of the returned tuple */
  double t, p[3], normal[3], u, v;
  uint32_t hit;        /* 0: None (then t = +inf and every other field is 0) */
  uint32_t front_face; /* Face::Front = 1 */
  uint32_t material;   /* index into the scene's materials */
  uint32_t _pad;
} rl_rtiow_hit; /* 88 bytes */
typedef struct rl_rtc_isect { /* scene/intersect.rs:11-16 Intersection{t, object, normal} */
  double t, normal[3];
  uint32_t object; /* object identity: triangles first (index into triangles[]), then shapes (n_triangles + index into shapes[]) */
  uint32_t _pad;
} rl_rtc_isect; /* 40 bytes */

/* out_hits[i] = world.hit(&rays[i], &Interval{min: tmin, max: tmax}); the interval is closed at both ends (interval.rs).
 * Scenes with ConstantMedium objects: RL_E_UNSUPPORTED — a medium's hit draws its free path from the pixel's RNG stream
 * (constant_medium.rs:55, see rl_medium), and a bare ray has none.  rl_rtiow_hit_rays_seeded below is the seeded form of this call:
 * there every ray carries an RNG cursor, and media scenes are accepted (as in rl_rtiow_ray_color_rays, which traces whole paths). */
int rl_rtiow_hit_rays(const rl_scene *, const rl_ray *rays, uint64_t n, double tmin, double tmax, rl_rtiow_hit *out_hits, rl_stats *opt_stats);
int rl_rtiow_hit_rays_device(const rl_scene *, const void *d_rays, uint64_t n, double tmin, double tmax, void *d_out_hits, void *hip_stream,
                             rl_stats *opt_stats);
/* out_counts[i] = the length of World::intersect(&rays[i])'s sorted list; out_isects[i*k .. i*k + min(count, k)) = its first entries in
 * the reference's order (stable by t; the entries beyond are left untouched); k = 0 with out_isects = NULL asks for the counts only.
 * out_hit_index (optional): the index hit() picks in that list (lowest t >= 0, later wins ties), reported also when it lies beyond k,
 * or UINT32_MAX.  A ray with more than 48 intersections is flagged (as in the renders) and reports 48. */
int rl_rtc_intersect_rays(const rl_scene *, const rl_ray *rays, uint64_t n, uint32_t k, rl_rtc_isect *out_isects, uint32_t *out_counts,
                          uint32_t *out_hit_index, rl_stats *opt_stats);
int rl_rtc_intersect_rays_device(const rl_scene *, const void *d_rays, uint64_t n, uint32_t k, void *d_out_isects, void *d_out_counts,
                                 void *d_out_hit_index, void *hip_stream, rl_stats *opt_stats);
/* out_rgb[3*i ..] = World::color_at(&rays[i]) with the scene's max_reflection_depth. */
int rl_rtc_color_at_rays(const rl_scene *, const rl_ray *rays, uint64_t n, double *out_rgb, rl_stats *opt_stats);
int rl_rtc_color_at_rays_device(const rl_scene *, const void *d_rays, uint64_t n, void *d_out_rgb, void *hip_stream, rl_stats *opt_stats);

/* =====================================================================
 *  Seeded path queries: Camera::get_ray and Camera::ray_color for ray buffers
 * =====================================================================
 *   rl_rtiow_camera_rays*     <- ray-tracing-one-weekend/src/camera.rs:203-216  Camera::get_ray(&mut rng, x, y)
 *   rl_rtiow_ray_color_rays*  <- ray-tracing-one-weekend/src/camera.rs:232-260  Camera::ray_color(&mut rng, &ray, world, depth)
 * Both take, per ray, an RNG cursor and return the advanced one.  A cursor is ChaCha8Rng::seed_from_u64(seed) after
 * set_stream(stream), at word position word_pos (get_word_pos; a draw is two words).  The reference's _render derives its stream per
 * pixel and sample as sample_index * W * H + x * W + y and keeps the word position from sample to sample (camera.rs:161-170); the
 * library does not compute streams for the caller.  With both calls a host rebuilds that loop itself and gets the library's own frames
 * bit for bit: cursors (s*W*H + x*W + y, 0) for every sample give rl_rtiow_render_independent*, carrying each pixel's word_pos from one
 * sample's output cursor into the next sample's input gives rl_rtiow_render*.  The kernels keep the position in 32 bits: an input
 * word_pos >= 2^31 is RL_E_INVALID (host forms; the device forms document it as undefined).
 * Status, concurrency, rl_init_multi, n = 0, NULL buffers and the wrong scene family: as stated for the batched ray queries above. */
typedef struct rl_rng_cursor {
  uint64_t stream;   /* ChaCha8Rng::set_stream */
  uint64_t word_pos; /* ChaCha8Rng::get_word_pos, < 2^31 */
} rl_rng_cursor;     /* 16 bytes */

/* out_rays[i] = cam.get_ray(&mut rng_i, px[i], py[i]), rng_i = cursors[i] of seed cam->seed; out_cursors[i] = rng_i afterwards
 * (out_cursors may alias cursors).  The draws are, in order: the pixel square's two, UnitDisc only when defocus_angle > 0, then time.
 * px[i] >= image_width or py[i] >= image_height: RL_E_INVALID (host form; device form: undefined).  Needs an initialised device
 * context but no scene; the host form runs on the current context's library stream and is synchronous, the device form is asynchronous
 * on hip_stream (HIP errors are reported by the stream's next synchronising call). */
int rl_rtiow_camera_rays(const rl_rtiow_camera *, uint64_t n, const uint32_t *px, const uint32_t *py, const rl_rng_cursor *cursors,
                         rl_ray *out_rays, rl_rng_cursor *out_cursors);
int rl_rtiow_camera_rays_device(const rl_rtiow_camera *, uint64_t n, const void *d_px, const void *d_py, const void *d_cursors,
                                void *d_out_rays, void *d_out_cursors, void *hip_stream);

/* out_rgb[3*i ..] = ray_color(&mut rng_i, &rays[i], world, max_depth) with rng_i = cursors[i] of `seed`, under the renders' arithmetic
 * contract: it is the value a render adds to a pixel for that sample, defined as the sample-parallel mode defines a sample's colour
 * (the accumulator starts at 0.0).  opt_out_cursors[i] = the cursor behind the path (may alias cursors); opt_out_ray_counts[i] = the
 * rays traced for path i, their sum is stats.rays.  max_depth == 0: black, no ray, the cursor unchanged.  Rays are used as given, from
 * any origin, without normalisation; a NaN or zero ray gives a defined result and is flagged only where the reference would panic.
 * Scenes with ConstantMedium objects are accepted: the free path is drawn from the ray's own cursor where the reference's fold
 * evaluates the medium, as in the renders.  Without opt_stats the call is counter-free and may be served by the fast tree walk (same
 * bits; order-sensitive rays are re-traced in the reference's order); with opt_stats all counters are the reference's, rng_words = the
 * words the paths consumed.  A batch beyond the 32-bit work counter runs as several passes back to back on the stream. */
int rl_rtiow_ray_color_rays(const rl_scene *, const rl_ray *rays, const rl_rng_cursor *cursors, uint64_t n, uint64_t seed,
                            uint32_t max_depth, const double background[3], double *out_rgb, rl_rng_cursor *opt_out_cursors,
                            uint32_t *opt_out_ray_counts, rl_stats *opt_stats);
int rl_rtiow_ray_color_rays_device(const rl_scene *, const void *d_rays, const void *d_cursors, uint64_t n, uint64_t seed,
                                   uint32_t max_depth, const double background[3], void *d_out_rgb, void *d_opt_out_cursors,
                                   void *d_opt_out_ray_counts, void *hip_stream, rl_stats *opt_stats);

/* =====================================================================
 *  Material queries: Material::scatter, Material::emitted and Texture::value for buffers
 * =====================================================================
 *   rl_rtiow_scatter_rays*    <- ray-tracing-one-weekend/src/material.rs:11-20  Material::scatter(&mut rng, &ray, &hit_record) -> Option<(Color, Ray)>
 *                                and Material::emitted(u, v, &p)
 *   rl_rtiow_texture_values*  <- ray-tracing-one-weekend/src/texture.rs  Texture::value(u, v, &p)
 * What ray_color (camera.rs:232-260) does with a hit, as a primitive of its own: with rl_rtiow_hit_rays a host writes its own
 * light-transport loop (its own depth rule, Russian roulette, probe rays, per-bounce buffers) and still shades as the library does.  The
 * arithmetic is that of the render kernels, so the loop
 *     sum = 0, thr = 1; up to max_depth times: hit = hit_rays(ray, tmin = 1e-10); a miss: sum += thr * background, stop;
 *     s = scatter_rays(ray, hit, cursor); sum = sum + thr * s.emitted; s.scatter == 0: stop; thr = thr * s.attenuation; ray = s.scattered
 * gives rl_rtiow_ray_color_rays' colours, cursors and ray counts bit for bit.  A scene with ConstantMedium objects, which
 * rl_rtiow_hit_rays refuses: use rl_rtiow_hit_rays_seeded there (hit, cursor = hit_rays_seeded(ray, cursor, tmin = 1e-10), the cursor then
 * passed on to scatter_rays); it serves every RTIOW scene.  Cursors, seed and the word_pos rules are those of the seeded path queries above
 * (odd positions are legal; word_pos >= 2^31 is RL_E_INVALID in the host form).  Status, concurrency, rl_init_multi, n = 0, NULL buffers and the wrong scene family:
 * as stated for the batched ray queries. */
typedef struct rl_rtiow_scatter { /* material.rs:11-20: scatter's Option<(Color, Ray)> + emitted's Color */
  double attenuation[3];          /* zeros unless scatter == 1 */
  double emitted[3];              /* mat.emitted(hit.u, hit.v, &hit.p) */
  rl_ray scattered;               /* origin = hit.p, time = rays[i].time; zeros unless scatter == 1 */
  uint32_t scatter;               /* 1: Some, 0: None (Flat, DiffuseLight, an absorbed Metal reflection, hit == 0) */
  uint32_t _pad;
} rl_rtiow_scatter;               /* 112 bytes */

/* out[i]: mat = materials[hits[i].material], rng_i = cursors[i] of `seed`; emitted = mat.emitted(hits[i].u, hits[i].v, &hits[i].p) and
 * mat.scatter(&mut rng_i, &rays[i], &hits[i]); opt_out_cursors[i] = rng_i afterwards (may alias cursors).  Inputs are used as given: of
 * rays[i] only dir and time are read; hits[i].normal is neither normalised nor checked; p, u, v, front_face and material are read, t is
 * not.  hits[i].hit == 0: the record is all zeros and the cursor unchanged.  All six material kinds are served in every RTIOW scene,
 * RL_MAT_ISOTROPIC included (it needs only a hit record, so a caller may make one for a medium of its own).  The draws: UnitSphere's
 * rejection loop for Lambertian, Metal (also when the reflection is then absorbed) and Isotropic; one f64 for Dielectric's Schlick test,
 * drawn only when refraction is possible; none for Flat and DiffuseLight.
 * hits[i].material outside the scene's table: RL_E_INVALID before anything is launched (host form); the device form treats the
 * element as hit == 0 and never reads outside the table.
 * The one panic site is Dielectric with a zero-length incident direction (material.rs:150-151): counted in flagged, RL_E_DEGENERATE is
 * returned, every output is written and the element's values are those a render produces there.
 * opt_stats: rays = elements with hit != 0, rng_words = words consumed, flagged as above; the traversal counters are 0. */
int rl_rtiow_scatter_rays(const rl_scene *, const rl_ray *rays, const rl_rtiow_hit *hits, const rl_rng_cursor *cursors, uint64_t n,
                          uint64_t seed, rl_rtiow_scatter *out, rl_rng_cursor *opt_out_cursors, rl_stats *opt_stats);
int rl_rtiow_scatter_rays_device(const rl_scene *, const void *d_rays, const void *d_hits, const void *d_cursors, uint64_t n,
                                 uint64_t seed, void *d_out, void *d_opt_out_cursors, void *hip_stream, rl_stats *opt_stats);

/* out_rgb[3*i ..] = textures[textures[i]].value(uv[2*i], uv[2*i + 1], &p[3*i ..]) over the whole texture tree: Solid, Checker, Image,
 * Noise.  A texture id outside the scene's table: RL_E_INVALID (host form); zeros (device form).  No RNG, no stats; the device form is
 * asynchronous on hip_stream, and rl_render_status counts it as a query of 0 rays. */
int rl_rtiow_texture_values(const rl_scene *, const uint32_t *textures, const double *uv, const double *p, uint64_t n, double *out_rgb);
int rl_rtiow_texture_values_device(const rl_scene *, const void *d_textures, const void *d_uv, const void *d_p, uint64_t n, void *d_out_rgb,
                                   void *hip_stream);

/* =====================================================================
 *  Seeded hit queries: Hittable::hit for rays that carry an RNG cursor
 * =====================================================================
 *   rl_rtiow_hit_rays_seeded*  <- ray-tracing-one-weekend/src/hittable/mod.rs:42  Hittable::hit(&Ray, &Interval) on the scene root, with
 *                                 ray-tracing-one-weekend/src/hittable/constant_medium.rs:27-80  ConstantMedium::hit (the deterministic
 *                                 variant of rl_medium: the free path is drawn from the pixel's ChaCha8 stream)
 * rl_rtiow_hit_rays for every RTIOW scene, ConstantMedium objects included: the one primitive of the host loop above that needs
 * randomness only in some scenes.  out_hits[i] = world.hit(&rays[i], &Interval{min: tmin, max: tmax}) with rng_i = cursors[i] of `seed`.
 * Every ConstantMedium::hit the reference's fold reaches with rec1.t < rec2.t after clamping (constant_medium.rs:42-47) takes one
 * gen::<f64>() (two words) from rng_i, in the fold's evaluation order: an object listed before the medium does not keep the medium from
 * drawing, a closer hit found BEFORE the medium that cuts its chord to nothing does.  opt_out_cursors[i] = rng_i afterwards (may alias
 * cursors).  A ray whose fold reaches no such medium leaves its cursor unchanged.
 * A medium's hit record is the reference's own: t, p = r.at(t), material = the medium's phase-function material, and the reference's
 * arbitrary fields as they are: normal (1, 0, 0), u = v = 0, front_face = 1.  The interval is the caller's and closed at both ends, as
 * rl_rtiow_hit_rays treats it; inside a medium it clamps the chord (rec1.t.max(tmin), rec2.t.min(tmax)).  Rays are used as given: `dir`
 * is not normalised, and its length scales the medium's free path (ray_length, constant_medium.rs:49).
 * Scenes without media are accepted: the records are bit for bit those of rl_rtiow_hit_rays (the same kernels and the same fast /
 * reference-order selection), the cursors come back unchanged (opt_out_cursors, when given and not the input, receives a copy) and
 * rng_words is 0.  Scenes with media: with opt_stats every counter is the reference's (the nested boundary traces included, as in the
 * renders) and rng_words = the words consumed; without it the call is counter-free and records, cursors and flagged are the same bits.
 * Cursor rules as the seeded path queries state them: odd positions are legal; word_pos >= 2^31 is RL_E_INVALID in the host form and
 * undefined in the device form.  NaN interval bounds, NULL buffers with n > 0, n = 0, a scene of the other family, status, concurrency
 * and rl_init_multi: as stated for the batched ray queries. */
int rl_rtiow_hit_rays_seeded(const rl_scene *, const rl_ray *rays, const rl_rng_cursor *cursors, uint64_t n, uint64_t seed, double tmin,
                             double tmax, rl_rtiow_hit *out_hits, rl_rng_cursor *opt_out_cursors, rl_stats *opt_stats);
int rl_rtiow_hit_rays_seeded_device(const rl_scene *, const void *d_rays, const void *d_cursors, uint64_t n, uint64_t seed, double tmin,
                                    double tmax, void *d_out_hits, void *d_opt_out_cursors, void *hip_stream, rl_stats *opt_stats);

/* =====================================================================
 *  RTC shading queries: prepare_computations, shade_hit, shadow_attenuation and lighting for buffers
 * =====================================================================
 *   rl_rtc_prepare_rays*        <- ray-tracer-challenge/src/scene/intersect.rs:159-168 hit + :38-115 Intersection::prepare_computations
 *   rl_rtc_shade_hits*          <- ray-tracer-challenge/src/scene/world.rs:57-87 World::shade_hit up to its recursion, with
 *                                  intersect.rs:139-156 Precomputation::schlick and the rays of world.rs:128-159
 *   rl_rtc_shadow_attenuation*  <- ray-tracer-challenge/src/scene/world.rs:104-126 World::shadow_attenuation(&point, light)
 *   rl_rtc_lighting*            <- ray-tracer-challenge/src/scene/material.rs:54-90 material::lighting
 * What World::color_at (world.rs:89-102) does with a hit, as primitives of their own: with them a host writes its own integrator (its own
 * depth rule, area lights sampled with many shadow queries, visibility from arbitrary points, per-bounce buffers) and still shades as the
 * library does.  The arithmetic is that of the render kernels, so the loop
 *     c = 0; stack = [(ray, w = 1, remaining = max_reflection_depth, mult = 1)]
 *     while stack: pop (ray, w, remaining, mult)
 *       k = prepare_rays(ray);  k.hit == 0 or n_lights == 0:  c = c + void_color * w; continue
 *       s = shade_hits(k);      c = c + s.surface * w
 *       m = materials[k.material]; wl = w * (double)n_lights; both = m.reflectivity > 0 && m.transparency > 0
 *       remaining > 0 && s.refract: push (s.refracted, wl * m.transparency * (both ? 1 - s.schlick : 1), remaining - 1, mult * n_lights)
 *       remaining > 0 && s.reflect: push (s.reflected, wl * m.reflectivity * (both ? s.schlick : 1), remaining - 1, mult * n_lights)
 * gives rl_rtc_color_at_rays' colours bit for bit (the refraction is pushed first, so the reflection is popped first; multiplications
 * associate left to right), and the sum over all nodes of mult * (prepare's stats.rays + shade's stats.rays) is a counting
 * rl_rtc_color_at_rays' stats.rays (the reference evaluates reflected_color / refracted_color once per light, world.rs:73-74).
 * Status, concurrency, rl_init_multi, n = 0, NULL buffers and the wrong scene family (here: an RTIOW scene): as stated for the batched
 * ray queries. */
typedef struct rl_rtc_comps {      /* scene/intersect.rs:123-137 Precomputation */
  double t, point[3], eye_v[3], normal_v[3], over_point[3], under_point[3], reflect_v[3];
  double n1, n2;                   /* refraction_exiting, refraction_entering */
  double object_color[3];          /* Surface::color_at at the hit: the pattern evaluated as the render does (rtc_hit_color) */
  uint32_t hit;                    /* 0: intersect::hit gave None; every other field is 0 */
  uint32_t inside;
  uint32_t object;                 /* identity as in rl_rtc_isect.object */
  uint32_t material;               /* index into the scene's materials */
} rl_rtc_comps;                    /* 208 bytes */

typedef struct rl_rtc_shade {      /* what World::shade_hit (world.rs:57-87) computes before it recurses */
  double surface[3];               /* lighting(.., shadow_attenuation) summed over the lights in order; the first light's value starts the sum */
  double schlick;                  /* Precomputation::schlick (intersect.rs:139-156), always computed */
  rl_ray reflected;                /* origin over_point, dir reflect_v, time 0; zeros unless reflect == 1 */
  rl_ray refracted;                /* origin under_point, dir by world.rs:143-154; zeros unless refract == 1 */
  uint32_t reflect;                /* material.reflectivity != 0 */
  uint32_t refract;                /* material.transparency != 0 and no total internal reflection */
} rl_rtc_shade;                    /* 152 bytes */

/* out_comps[i] = hit(&World::intersect(&rays[i])).map(|h| h.prepare_computations(&rays[i], &xs)) (intersect.rs:159-168, :48-115).
 * n1 and n2 are computed for every material, as the reference does (the containers walk of intersect.rs:72-99); the renders compute them
 * only where a transparent material reads them.  inside = normal . eye_v < 0, and normal_v is then the negated normal.
 * Panic sites (intersect.rs:57, :70): a failed eye_v or reflect_v normalisation is counted in flagged and the element carries the value
 * the renders go on with (-dir, dir); a ray with more than 48 intersections is flagged, as in the renders.  RL_E_DEGENERATE is then
 * returned with every output written.  A zero dir gives hit == 0 and reaches no panic site.
 * opt_stats: rays = n, the traversal counters as rl_rtc_intersect_rays reports them. */
int rl_rtc_prepare_rays(const rl_scene *, const rl_ray *rays, uint64_t n, rl_rtc_comps *out_comps, rl_stats *opt_stats);
int rl_rtc_prepare_rays_device(const rl_scene *, const void *d_rays, uint64_t n, void *d_out_comps, void *hip_stream, rl_stats *opt_stats);

/* out[i]: what world.shade_hit(&comps[i], remaining) (world.rs:57-87) computes itself: per light, in order, shadow_attenuation from
 * over_point (world.rs:61) and lighting (:63-71), summed as the reference's reduce sums them; schlick; and the rays reflected_color /
 * refracted_color would trace (world.rs:132, :143-154).  comps are used as given and need not come from rl_rtc_prepare_rays: t, inside,
 * object and under_point / reflect_v of an element without a secondary ray are not read.  comps[i].hit == 0: an all-zero record, no ray.
 * A scene without lights: surface = 0 and reflect = refract = 0 (the reference's reduce over no lights is None).
 * opt_out_shadow ([n][n_lights], may be NULL): the attenuation used for each light (zeros where hit == 0).
 * comps[i].material outside the scene's table: RL_E_INVALID before anything is launched (host form); the device form treats the element
 * as hit == 0 and never reads outside the table.
 * opt_stats: rays = the shadow rays traced (none for a light at over_point itself, world.rs:107-125), the traversal counters theirs. */
int rl_rtc_shade_hits(const rl_scene *, const rl_rtc_comps *comps, uint64_t n, rl_rtc_shade *out, double *opt_out_shadow, rl_stats *opt_stats);
int rl_rtc_shade_hits_device(const rl_scene *, const void *d_comps, uint64_t n, void *d_out, void *d_opt_out_shadow, void *hip_stream,
                             rl_stats *opt_stats);

/* out_att[i] = world.shadow_attenuation(&points[3*i ..], light at light_positions[3*i ..]) (world.rs:104-126): the product of the
 * transparencies of the distinct objects between the point and the position, which need not be one of the scene's lights.  Coincident
 * point and position: 1.0, no ray (world.rs:107, :125).  opt_stats: rays = the shadow rays traced. */
int rl_rtc_shadow_attenuation(const rl_scene *, const double *points, const double *light_positions, uint64_t n, double *out_att,
                              rl_stats *opt_stats);
int rl_rtc_shadow_attenuation_device(const rl_scene *, const void *d_points, const void *d_light_positions, uint64_t n, void *d_out_att,
                                     void *hip_stream, rl_stats *opt_stats);

/* out_rgb[3*i ..] = lighting(materials[comps[i].material], &comps[i].point, &comps[i].object_color, &PointLight{light_positions[3*i ..],
 * light_intensities[3*i ..]}, &comps[i].eye_v, &comps[i].normal_v, shadow_att[i]) (material.rs:54-90).  hit == 0: zeros.  A material
 * outside the scene's table: RL_E_INVALID (host form); zeros (device form).  No traversal, no stats; the device form is asynchronous on
 * hip_stream, and rl_render_status counts it as a query of 0 rays. */
int rl_rtc_lighting(const rl_scene *, const rl_rtc_comps *comps, const double *light_positions, const double *light_intensities,
                    const double *shadow_att, uint64_t n, double *out_rgb);
int rl_rtc_lighting_device(const rl_scene *, const void *d_comps, const void *d_light_positions, const void *d_light_intensities,
                           const void *d_shadow_att, uint64_t n, void *d_out_rgb, void *hip_stream);

/* =====================================================================
 *  RTIOW occlusion queries: any-hit visibility for ray buffers
 * =====================================================================
 *   rl_rtiow_occluded_rays*  <- ray-tracing-one-weekend/src/hittable/mod.rs:42  Hittable::hit(&Ray, &Interval).is_some() on the scene root
 * "Is anything in the way": shadow rays towards a light the host samples itself, ambient occlusion, visibility between probes, picking.
 * out_occluded[i] = 1 where world.hit(&rays[i], &Interval{min: tmin, max: tmax}) is Some, else 0: the value of `hit` in the record
 * rl_rtiow_hit_rays writes for the same ray and interval, at one byte per ray.  The interval is closed at both ends, as rl_rtiow_hit_rays
 * treats it.  Rays are used as given, so an unnormalised dir = target - origin with tmax = 1 is the segment test between the two points
 * (tmin = 1e-10 keeps the origin's own surface out, as camera.rs:242-245 does).
 * With opt_stats the call is counting: it runs the reference-order fold, and every counter, flagged included, is bit for bit that of
 * rl_rtiow_hit_rays on the same batch.  Without opt_stats it is counter-free and, with tmin == 1e-10, may be served by an any-hit tree
 * walk that stops at the first primitive that is certainly hit and evaluates no normal of its own: flagged and RL_E_DEGENERATE then
 * come only from the rays that walk handed to the reference's fold (roots next to tmax, grazing / edge hits, far spheres, rays outside
 * the filter's range), so a panic site on a ray the walk decided by itself goes unreported; the bytes are the same either way.
 * Rules: those of rl_rtiow_hit_rays — n = 0 touches no buffer and zeroes opt_stats; NULL buffers with n > 0, n > 2^40, a NaN bound or an
 * RTC scene: RL_E_INVALID; a scene with ConstantMedium objects: RL_E_UNSUPPORTED (there is no seeded form of this call).  The _device
 * form is asynchronous unless opt_stats is given; status, concurrency and rl_init_multi: as stated for the batched ray queries. */
int rl_rtiow_occluded_rays(const rl_scene *, const rl_ray *rays, uint64_t n, double tmin, double tmax, uint8_t *out_occluded, rl_stats *opt_stats);
int rl_rtiow_occluded_rays_device(const rl_scene *, const void *d_rays, uint64_t n, double tmin, double tmax, void *d_out_occluded,
                                  void *hip_stream, rl_stats *opt_stats);

#ifdef __cplusplus
}
#endif
#endif /* RL_RENDER_H */
