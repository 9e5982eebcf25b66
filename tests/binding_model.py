"""What the C side says about the Python binding, read from the C text itself: a small prototype parser over include/rl_render.h
(declarations), csrc/ (the rl_debug_* definitions, which no header declares) and host/*.cpp (the rlh_* definitions), and the classes
both sides are compared in (tests/test_binding_signatures.py).  Below it, a recorder that stands in for the render library, one for
the host library's probes, and a driver that calls every wrapper of api.py, ao.py, direct.py, nee.py, occlusion.py and entry_table.py
on tiny inputs (tests/test_binding_calls.py, tools/record_binding_calls.py): what each wrapper hands to C, pinned without a GPU.

Classes.  A parameter or return is one of
  None                      void (returns only)
  ("ptr", pointee)          any `*` or `[]`; pointee = the struct's name where it is an rl_* / rlh_* struct, the scalar class where it is
                            a scalar, "void" otherwise
  ("int", bytes, signed)    so that `unsigned long long` and uint64_t compare equal
  ("float", bytes)
A parameter that fits none of them raises: the tests fail, they do not skip."""
import ctypes as C
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "rendering-learning_amd")
HEADER = os.path.join(ROOT, "include", "rl_render.h")

_SCALARS = {"char": ("int", 1, True), "int": ("int", 4, True), "signed": ("int", 4, True), "signed int": ("int", 4, True),
            "unsigned": ("int", 4, False), "unsigned int": ("int", 4, False), "long long": ("int", 8, True),
            "unsigned long long": ("int", 8, False), "int32_t": ("int", 4, True), "uint32_t": ("int", 4, False),
            "int64_t": ("int", 8, True), "uint64_t": ("int", 8, False), "uint8_t": ("int", 1, False), "size_t": ("int", 8, False),
            "float": ("float", 4), "double": ("float", 8)}
_TYPE_WORDS = {w for k in _SCALARS for w in k.split()} | {"void"}
_QUALIFIERS = {"const", "volatile", "struct", "extern", "static", "inline"}
_NOT_A_TYPE = {"return", "else", "new", "delete", "case", "goto", "typedef", "throw", "sizeof"}


def strip_comments(src):
    """C text without its comments (string literals are kept as they are, and a // or /* inside one is not a comment)."""
    pat = re.compile(r'"(?:\\.|[^"\\])*"|\'(?:\\.|[^\'\\])*\'|/\*.*?\*/|//[^\n]*', re.S)
    return pat.sub(lambda m: m.group(0) if m.group(0)[0] in "\"'" else " ", src)


def classify(decl, what):
    """The class of one parameter or return type as written (`const rl_scene *`, `unsigned long long out[2]`, `uint32_t n`, `void`)."""
    words = [w for w in re.findall(r"\w+", decl) if w not in _QUALIFIERS]
    if "*" in decl or "[" in decl:
        structs = [w for w in words if re.fullmatch(r"rlh?_\w+", w)]
        if structs:
            return ("ptr", structs[0])
        run = []
        for w in words:
            if w not in _TYPE_WORDS:
                break
            run.append(w)
        return ("ptr", _SCALARS.get(" ".join(run), "void") if run != ["void"] else "void")
    run = []
    for w in words:
        if w not in _TYPE_WORDS:
            break
        run.append(w)
    if run == ["void"] and len(words) == 1:
        return None
    key = " ".join(run)
    if key not in _SCALARS or len(words) - len(run) > 1:  # at most one word may follow the type: the parameter's name
        raise ValueError(f"{what}: cannot classify {decl.strip()!r}")
    return _SCALARS[key]


# a prototype starts a line or follows a `;`, `{` or `}`: return type words and stars, the name, the parameters, then `;` or `{`
_PROTO = re.compile(r"(?:^|[;{}])[ \t]*((?:\w+[\s*]+)+)(rlh?_\w+)\s*\(([^(){};]*)\)\s*([;{])", re.M)


def prototypes(src, end, name_re):
    """{name: (return class, [parameter classes])} of every `ret name(params)` followed by `end` (";" a declaration, "{" a definition)
    whose name matches name_re, in comment-stripped C text."""
    out = {}
    for ret, name, params, tail in _PROTO.findall(strip_comments(src)):
        if tail != end or not re.fullmatch(name_re, name) or ret.split()[0] in _NOT_A_TYPE:
            continue
        params = [p for p in (q.strip() for q in params.split(",")) if p]
        if params == ["void"]:
            params = []
        sig = (classify(ret, f"{name} (return)"), [classify(p, f"{name} (parameter {i})") for i, p in enumerate(params)])
        if name in out and out[name] != sig:
            raise ValueError(f"{name} is stated twice, differently")
        out[name] = sig
    return out


def _read(paths):
    return "\n".join(open(p, errors="replace").read() for p in sorted(paths))


def header_prototypes():
    """The public entry points include/rl_render.h declares."""
    return prototypes(_read([HEADER]), ";", r"rl_\w+")


def debug_prototypes():
    """The rl_debug_* entry points, from their definitions under csrc/ (they are declared in no header)."""
    paths = [p for p in glob.glob(os.path.join(PKG, "csrc", "*")) if p.endswith((".hip", ".h", ".cpp", ".inc"))]
    return prototypes(_read(paths), "{", r"rl_debug_\w+")


def host_prototypes():
    """The rlh_* entry points, from their definitions in host/*.cpp."""
    return prototypes(_read(glob.glob(os.path.join(PKG, "host", "*.cpp"))), "{", r"rlh_\w+")


def ctypes_class(t, struct_names):
    """The class of a ctypes restype / argtypes entry; struct_names: {ctypes Structure: the C struct's name}."""
    if t is None:
        return None
    code = getattr(t, "_type_", None)
    if isinstance(code, str):
        if code == "P":
            return ("ptr", "void")
        if code == "z":
            return ("ptr", _SCALARS["char"])
        if code in "fd":
            return ("float", C.sizeof(t))
        if code in "bBhHiIlLqQ":
            return ("int", C.sizeof(t), code.islower())
        raise ValueError(f"cannot classify ctypes type {t!r}")
    if code is not None and issubclass(t, C._Pointer):
        if issubclass(code, C.Structure):
            return ("ptr", struct_names[code])
        return ("ptr", ctypes_class(code, struct_names))
    raise ValueError(f"cannot classify ctypes type {t!r}")


def same_class(c_side, py_side):
    """Whether a ctypes class states the C class.  Scalars and void must be equal.  A pointer must be a pointer; an untyped one
    (c_void_p, c_char_p) may stand for any pointee, a typed one must name the C side's pointee."""
    if c_side is None or py_side is None or c_side[0] != "ptr" or py_side[0] != "ptr":
        return c_side == py_side
    return py_side[1] in ("void", _SCALARS["char"]) or py_side[1] == c_side[1]


# ----------------------------------------------------------------------------- what each wrapper hands to C
RL_E_DEGENERATE = -5
FAKE_SCENE = 0x5CE0E0  # the handle the recorder's *_scene_create return: never dereferenced, the driver clears it before it returns


def _field(v, t):
    if isinstance(v, C.Array):
        return list(v)
    if getattr(t, "_type_", None) == "P":
        return "ptr" if v else "null"
    return v


def _normalise(arg, cls, where):
    """One argument as the record keeps it, by the C side's class of its position."""
    if cls[0] == "ptr":
        if arg is None:
            return "null"
        if isinstance(arg, int):
            return "ptr" if arg else "null"
        if isinstance(arg, C.c_void_p):
            return "ptr" if arg.value else "null"
        obj = getattr(arg, "_obj", None)  # byref(obj)
        if isinstance(obj, C.Structure):
            return {k: _field(getattr(obj, k), t) for k, t in obj._fields_}
        return "ptr"
    if isinstance(arg, C._SimpleCData):
        arg = arg.value
    if isinstance(arg, bool) or not isinstance(arg, (int, float)):
        raise TypeError(f"{where}: {arg!r} handed to a scalar position")
    if cls[0] == "int" and not isinstance(arg, int):
        raise TypeError(f"{where}: {arg!r} handed to an integer position")
    return float(arg) if cls[0] == "float" else arg


class _Entry:
    """One symbol of the recorder: callable, and (as a ctypes function object) open to attribute assignments."""

    def __init__(self, rec, name):
        self._rec, self._name = rec, name

    def __call__(self, *args):
        rec, name = self._rec, self._name
        ret, params = rec.protos[name]
        if len(args) != len(params):
            raise TypeError(f"{name} takes {len(params)} arguments, {len(args)} given")
        rec.calls.append([name, [_normalise(a, c, f"{name} (parameter {i})") for i, (a, c) in enumerate(zip(args, params))]])
        if name.endswith("_scene_create"):
            return FAKE_SCENE
        if name == "rl_last_error":
            return b""
        if name == "rl_device_count":
            return 1
        if ret == ("int", 8, False):
            return 7
        if ret is None:
            return None
        return rec.rc if "opt_stats" in rec.stats_params.get(name, ()) or name in rec.status_calls else 0


class Recorder:
    """Stands in for api.render_lib(): every symbol the C text states (header and rl_debug_* definitions) is a callable that notes
    (symbol, normalised arguments) and returns RL_OK — or `rc` from the calls that render or query —, a fake handle from the two
    *_scene_create, b"" from rl_last_error and a small integer from the uint64 getters.  A symbol the C text lacks is an AttributeError,
    as on a CDLL."""
    status_calls = ("rl_render_status", "rl_rtiow_render_rgb8", "rl_rtc_render_rgb8", "rl_rtiow_render_denoised_rgb8")

    def __init__(self):
        self.protos = dict(header_prototypes(), **debug_prototypes())
        # the entry points whose last parameter is `rl_stats *opt_stats`: the ones a reached panic site can make return RL_E_DEGENERATE
        self.stats_params = {n: ("opt_stats",) for n, (_, ps) in header_prototypes().items() if ps and ps[-1] == ("ptr", "rl_stats")}
        self.calls, self.rc, self._entries = [], 0, {}

    def __getattr__(self, name):
        if name.startswith("_") or name not in self.protos:
            raise AttributeError(name)
        return self._entries.setdefault(name, _Entry(self, name))


class HostProbes:
    """Stands in for api.host_lib(), for the rlh_*_probe symbols only: they note (symbol, normalised arguments) in the Recorder's list
    and return 0.  Every other name is the real host library's, which still serves Camera, World and the rest."""
    rc, stats_params, status_calls = 0, {}, ()

    def __init__(self, real, rec):
        self._real, self._rec = real, rec
        self.protos = {n: p for n, p in host_prototypes().items() if n.endswith("_probe")}

    calls = property(lambda self: self._rec.calls)

    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError(name)
        return _Entry(self, name) if name in self.protos else getattr(self._real, name)


FAMILY_MODULES = ("ao", "direct", "nee", "occlusion", "entry_table")  # the package's modules beside api whose public functions are wrappers
PURE_PACKERS = {"pack_lights", "pack_sphere_lights"}  # ... except these: they reach no library


def drive(api, patch):
    """Calls every public wrapper of api.py and of the FAMILY_MODULES that reaches the render library (or, the cpp_mirror_probe*, an
    rlh_*_probe of the host library), against a Recorder, on tiny inputs: a 4 x 2 camera, three rays / pixels / records, a 4 x 2 image
    with two guide channels, one quad light and one sphere light.  patch(object, name, value) is monkeypatch.setattr or a stand-in
    that restores.  Each entry holds the wrapper's inspect.signature as text, and each wrapper runs up to four times:
      plain        as listed                                   -> the calls it made
      stats        with stats={} where it takes stats          -> the calls, and the dict's keys
      degenerate   the library answering RL_E_DEGENERATE       -> whether it raised; the dict's keys and rc
      allowed      likewise with allow_degenerate=True where the wrapper has it
    Returns [{"wrapper": label, variant: result, ...}] in a fixed order."""
    import importlib
    import inspect
    import numpy as np
    rec = Recorder()
    probes = HostProbes(api.host_lib(), rec)
    patch(api, "render_lib", lambda: rec)
    patch(api, "host_lib", lambda: probes)
    patch(api, "_inited", False)
    ao, direct, nee, occlusion, entry_table = (importlib.import_module(f"{api.__package__}.{m}") for m in FAMILY_MODULES)
    worlds, out = [], []

    def run(label, fn, *args, **kw):
        names = inspect.signature(fn).parameters
        entry = {"wrapper": label, "signature": str(inspect.signature(fn))}

        def once(variant, rc, **extra):
            api._inited = False
            rec.calls, rec.rc = [], rc
            stats = extra.get("stats")
            try:
                with np.errstate(all="ignore"):
                    fn(*args, **dict(kw, **extra))
                outcome = "ok"
            except api.RLError as e:
                outcome = f"RLError({e.code})"
            res = {"calls": rec.calls} if rc == 0 else {"outcome": outcome}
            if rc == 0 and outcome != "ok":
                raise AssertionError(f"{label} [{variant}]: {outcome} from a library that answers RL_OK")
            if stats is not None:
                res["keys"] = sorted(stats)
                if rc != 0:
                    res["rc"] = stats.get("rc")
            entry[variant] = res

        with_stats = {"stats": {}} if "stats" in names else {}
        once("plain", 0)
        if with_stats:
            once("stats", 0, stats={})
        once("degenerate", RL_E_DEGENERATE, **({"stats": {}} if with_stats else {}))
        if "allow_degenerate" in names:
            once("allowed", RL_E_DEGENERATE, allow_degenerate=True, **({"stats": {}} if with_stats else {}))
        out.append(entry)

    try:
        sph = np.zeros(1, dtype=api.SPHERE)
        sph["center0"], sph["center1"], sph["radius"] = (0, 0, -2), (0, 0, -2), 0.5
        mat = np.zeros(1, dtype=api.MATERIAL)
        mat["kind"], mat["albedo"], mat["ior"] = api.MAT_LAMBERTIAN, (0.5, 0.5, 0.5), 1.0
        tex = np.zeros(1, dtype=api.TEXTURE)

        def new_world():
            w = api.World.from_spheres(sph, mat, tex, True)
            worlds.append(w)
            return w

        world = new_world()
        cam = api.Camera(api.CameraParams(aspect_ratio=2.0, image_width=4, samples_per_pixel=2, max_depth=3, seed=9))
        rtc = api.RtcWorld.test_mirror_scene(4, 2)
        worlds.append(rtc)
        o3, d3, t3 = np.zeros((3, 3)), np.tile((0.0, 0.0, -1.0), (3, 1)), np.array([0.0, 0.25, 0.5])
        rays, cur = api.pack_rays(o3, d3, t3), api.pack_cursors(np.arange(3), 2)
        hits, comps = np.zeros(3, dtype=api.RTIOW_HIT), np.zeros(3, dtype=api.RTC_COMPS)
        xs, ys = [0, 3, 1], [0, 1, 1]
        D = 0x1000  # "device pointers": D * k, never dereferenced
        bg = (0.25, 0.5, 1.0)

        # ---- module level
        run("init", api.init, 0)
        run("init_multi", api.init_multi, 2)
        run("init_multi[emulate]", api.init_multi, emulate=2)
        run("World.device", lambda: new_world().device())
        run("RtcWorld.device", lambda: (worlds.append(api.RtcWorld.test_csg_scene(4, 2)), worlds[-1].device()))
        world.device(), rtc.device()
        run("render_status", api.render_status, world)
        run("render_progress", api.render_progress, world)
        for name, arg in (("set_fast_traversal", True), ("set_coop", 0), ("set_lpt", 1), ("set_coop_pixels_max", 12), ("set_steal", 1.5),
                          ("set_indep_cap", 1 << 20), ("set_indep_k", 2), ("set_fastg_one_wave", -1), ("set_pixel_entry", 2),
                          ("set_pixel_entry_sphere", True), ("set_query_pass_cap", 5), ("set_denoise_route", -1), ("set_denoise_blocks", 3),
                          ("set_rtiow_variant", 1031)):
            run(name, getattr(api, name), arg)
        run("set_status_gap", api.set_status_gap, 10, 20)
        for name in ("live_buffers", "last_query", "last_denoise_route", "last_denoise_launch", "material_query_max_lanes", "features_max_lanes"):
            run(name, getattr(api, name))
        run("pixel_entry_table", api.pixel_entry_table, world, 8)
        run("fast_tree", api.fast_tree, world)

        # ---- World
        run("World.hit_rays", world.hit_rays, o3, d3, t3)
        run("World.hit_rays_device", world.hit_rays_device, D, 2 * D, 3, stream=3 * D)
        run("World.hit_rays_seeded", world.hit_rays_seeded, rays, cur, 9)
        run("World.hit_rays_seeded_device", world.hit_rays_seeded_device, D, 2 * D, 3, 9, 3 * D)
        run("World.hit_rays_seeded_device[out_cursors]", world.hit_rays_seeded_device, D, 2 * D, 3, 9, 3 * D, 4 * D, stream=5 * D)
        run("World.ray_color_rays", world.ray_color_rays, o3, d3, t3, cur, 9, 3, bg)
        run("World.ray_color_rays[rays]", world.ray_color_rays, None, None, None, cur, 9, 3, bg, rays=rays)
        run("World.ray_color_rays_device", world.ray_color_rays_device, D, 2 * D, 3, 9, 3, bg, 3 * D)
        run("World.ray_color_rays_device[outputs]", world.ray_color_rays_device, D, 2 * D, 3, 9, 3, bg, 3 * D, 4 * D, 5 * D, 6 * D)
        run("World.scatter_rays", world.scatter_rays, rays, hits, cur, 9)
        run("World.scatter_rays_device", world.scatter_rays_device, D, 2 * D, 3 * D, 3, 9, 4 * D)
        run("World.scatter_rays_device[out_cursors]", world.scatter_rays_device, D, 2 * D, 3 * D, 3, 9, 4 * D, 5 * D, 6 * D)
        run("World.texture_values", world.texture_values, [0, 0, 0], np.zeros((3, 2)), np.zeros((3, 3)))
        run("World.texture_values_device", world.texture_values_device, D, 2 * D, 3 * D, 3, 4 * D, 5 * D)

        # ---- Camera
        ckpt = api.Canvas(2, 4, 2, np.ones((2, 4, 3)))
        run("Camera.render", cam.render, world)
        run("Camera.render_rgb8", cam.render_rgb8, world)
        run("Camera.render_denoised_rgb8", cam.render_denoised_rgb8, world, 2)
        run("Camera.render_denoised_rgb8[rule]", cam.render_denoised_rgb8, world, 2, rule=(2, 1, 1e-4, 0.0), iterations=2, want=("albedo", "depth"))
        run("Camera.render_from_checkpoint", cam.render_from_checkpoint, world, ckpt)
        run("Camera.render_rows", cam.render_rows, world, 1, 2, first_sample=4)
        run("Camera.render_independent", cam.render_independent, world)
        run("Camera.render_independent[checkpoint]", cam.render_independent, world, ckpt)
        run("Camera.render_independent_rows", cam.render_independent_rows, world, 1, 2, first_sample=4)
        run("Camera.render_independent_device", cam.render_independent_device, world, D, stream=2 * D, row_first=1, row_step=2, accumulate=True)
        run("Camera.get_rays", cam.get_rays, xs, ys, cur)
        run("Camera.get_rays_device", cam.get_rays_device, D, 2 * D, 3 * D, 4 * D, 5 * D, 3, stream=6 * D)
        run("Camera.render_multi", cam.render_multi, world, first_sample=2)
        run("Camera.render_multi_device", cam.render_multi_device, world, D)
        run("Camera.render_device", cam.render_device, world, D, stream=2 * D, row_first=1, row_step=2)
        run("Camera.render_pixels", cam.render_pixels, world, xs, ys)
        run("Camera.render_pixels_device", cam.render_pixels_device, world, D, 2 * D, 3, 3 * D, stream=4 * D)
        run("Camera.render_moments", cam.render_moments, world, row_first=1, row_step=2)
        run("Camera.render_moments_device", cam.render_moments_device, world, D, 2 * D, stream=3 * D)
        run("Camera.render_pixels_moments", cam.render_pixels_moments, world, xs, ys, first_sample=1)
        run("Camera.render_pixels_moments_device", cam.render_pixels_moments_device, world, D, 2 * D, 3, 3 * D, 4 * D)
        run("Camera.render_adaptive", cam.render_adaptive, world, 2, 1, abs_variance=1e-3, rel_variance=1e-2)
        run("Camera.render_adaptive_device", cam.render_adaptive_device, world, 2, 1, D, 2 * D, 3 * D, rel_variance=1e-2, stream=4 * D)
        run("Camera.render_features", cam.render_features, world)
        run("Camera.render_features[want]", cam.render_features, world, row_first=1, row_step=2, want=("normal_sum", "hit_count"))
        run("Camera.render_features_device", cam.render_features_device, world, stream=D, d_albedo_sum=2 * D, d_depth_sum=3 * D)
        run("Camera.render_pixels_features", cam.render_pixels_features, world, xs, ys)
        run("Camera.render_pixels_features[want]", cam.render_pixels_features, world, xs, ys, want=("albedo_sum",))
        run("Camera.render_pixels_features_device", cam.render_pixels_features_device, world, D, 2 * D, 3, d_normal_sum=3 * D, d_hit_count=4 * D)

        # ---- denoising: a 4 x 2 image, two guide channels
        img, var, guides = np.full((2, 4, 3), 0.5), np.full((2, 4, 3), 0.01), np.zeros((2, 4, 2))
        mom = api.Moments(4, np.full((2, 4, 3), 2.0), np.full((2, 4, 3), 1.5))
        ada = api.Adaptive(np.full((2, 4, 3), 2.0), np.full((2, 4, 3), 1.5), np.full((2, 4), 4, dtype=np.uint32))
        feat = api.Features(2, np.ones((2, 4, 3)), np.ones((2, 4, 3)), np.ones((2, 4)), np.full((2, 4), 2, dtype=np.uint32))
        p2 = api.atrous_params(2, guide_sigma=(0.5, None))
        dev_in = api.denoise_inputs({"sums": D, "sq": 2 * D, "albedo_sum": 3 * D, "hit_count": 4 * D}, want=("albedo", "coverage"), samples=4, feature_samples=2)
        run("denoise_atrous", api.denoise_atrous, img, var, guides, iterations=2)
        run("denoise_atrous[no guides, no variance]", api.denoise_atrous, img, var, out_variance=False)
        run("denoise_atrous_pass_device", api.denoise_atrous_pass_device, 4, 2, 1, p2, D, 2 * D, 3 * D, 4 * D)
        run("denoise_atrous_pass_device[variance]", api.denoise_atrous_pass_device, 4, 2, 2, api.atrous_params(0), D, 2 * D, 0, 4 * D, 5 * D, 6 * D)
        run("denoise_render", api.denoise_render, mom, feat, iterations=1)
        run("denoise_prepare_device", api.denoise_prepare_device, 4, 2, dev_in, D, 2 * D, 3 * D, 4 * D)
        run("denoise_finish_device", api.denoise_finish_device, 4, 2, D, 2 * D, 3 * D, 2, d_out_rgb8=4 * D)
        run("denoise_render_work_bytes", api.denoise_render_work_bytes, 4, 2, 2)
        run("denoise_render_device", api.denoise_render_device, 4, 2, dev_in, 2, api.atrous_params(4), D, 4096, d_out_color=2 * D, stream=3 * D)
        run("denoise_render_gpu", api.denoise_render_gpu, mom, feat, iterations=1)
        run("denoise_render_gpu[adaptive, rgb8]", api.denoise_render_gpu, ada, feat, want=("albedo", "normal"), rgb8=True)

        # ---- RtcWorld
        cam2 = api.rtc_camera(4, 2, 1.0, (0, 0, -5), (0, 0, 0), (0, 1, 0))
        run("RtcWorld.render", rtc.render, 2, row_first=1, row_step=2)
        run("RtcWorld.render[camera]", rtc.render, camera=cam2)
        run("RtcWorld.render_rgb8", rtc.render_rgb8, 2)
        run("RtcWorld.render_multi", rtc.render_multi, 2)
        run("RtcWorld.render_device", rtc.render_device, D, 2, stream=2 * D)
        run("RtcWorld.render_pixels", rtc.render_pixels, xs, ys, 2)
        run("RtcWorld.render_pixels_device", rtc.render_pixels_device, D, 2 * D, 3, 3 * D, stream=4 * D)
        run("RtcWorld.intersect_rays", rtc.intersect_rays, o3, d3, k=2)
        run("RtcWorld.intersect_rays[k=0]", rtc.intersect_rays, o3, d3, k=0)
        run("RtcWorld.intersect_rays_device", rtc.intersect_rays_device, D, 3, 2, 2 * D, 3 * D)
        run("RtcWorld.intersect_rays_device[hit_index]", rtc.intersect_rays_device, D, 3, 0, 0, 3 * D, 4 * D, 5 * D)
        run("RtcWorld.color_at_rays", rtc.color_at_rays, o3, d3)
        run("RtcWorld.color_at_rays_device", rtc.color_at_rays_device, D, 2 * D, 3, stream=3 * D)
        run("RtcWorld.prepare_rays", rtc.prepare_rays, o3, d3)
        run("RtcWorld.prepare_rays_device", rtc.prepare_rays_device, D, 3, 2 * D)
        run("RtcWorld.shade_hits", rtc.shade_hits, comps)
        run("RtcWorld.shade_hits_device", rtc.shade_hits_device, D, 3, 2 * D)
        run("RtcWorld.shade_hits_device[shadow]", rtc.shade_hits_device, D, 3, 2 * D, 3 * D, 4 * D)
        run("RtcWorld.shadow_attenuation", rtc.shadow_attenuation, o3, (0.0, 10.0, 0.0))
        run("RtcWorld.shadow_attenuation_device", rtc.shadow_attenuation_device, D, 2 * D, 3, 3 * D)
        run("RtcWorld.lighting", rtc.lighting, comps, (0.0, 10.0, 0.0), (1.0, 1.0, 1.0), 1.0)
        run("RtcWorld.lighting_device", rtc.lighting_device, D, 2 * D, 3 * D, 4 * D, 3, 5 * D, 6 * D)
        # ---- RTC read-outs (appended: the rows above keep their places in the fixture)
        run("last_rtc_launch", api.last_rtc_launch)
        run("rtc_program", api.rtc_program, rtc)
        # ---- RTIOW launch log and hand-over record (appended likewise; the recorder's total is 7: seven launches asked for)
        run("rtiow_launch_total", api.rtiow_launch_total)
        run("rtiow_launches", api.rtiow_launches, 0)
        run("steal_record", api.steal_record, world, 8)

        # ---- the modules beside api (appended likewise): occlusion queries, the entry table's switches, the pixel-render families
        run("occlusion.occluded_rays", occlusion.occluded_rays, world, o3, d3, t3)
        run("occlusion.occluded_rays_device", occlusion.occluded_rays_device, world, D, 2 * D, 3, 0.5, 2.0, stream=3 * D)
        run("entry_table.set_slices", entry_table.set_slices, 2)
        run("entry_table.set_reuse", entry_table.set_reuse, False)
        run("entry_table.builds", entry_table.builds)
        run("entry_table.sliced_table", entry_table.sliced_table, world, 8, 2)
        run("entry_table.census", entry_table.census, world)

        quad, ball = [((0, 4, 0), (2, 0, 0), (0, 0, 2), (5, 4, 3))], [((0, 5, 0), 1.0, 2.0)]
        shard = {"row_first": 1, "row_step": 2}

        def family(mod, stem, outputs, *particular, subset={}, routes={}):
            """The four wrappers of one family, each plain and with a strict subset of its outputs (the row forms on a shard; `subset`:
            more keyword arguments of those rows), then once per route (routes: {tag: keyword arguments})."""
            name = mod.__name__.rsplit(".", 1)[1]
            rows, dev = getattr(mod, f"render_{stem}"), getattr(mod, f"render_{stem}_device")
            pix, pixdev = getattr(mod, f"render_pixels_{stem}"), getattr(mod, f"render_pixels_{stem}_device")
            d_all = {f"d_{k}": (i + 4) * D for i, k in enumerate(outputs)}
            d_some = {f"d_{outputs[-1]}": 7 * D}
            run(f"{name}.{rows.__name__}", rows, cam, world, *particular)
            run(f"{name}.{rows.__name__}[want]", rows, cam, world, *particular, first_sample=4, want=outputs[:1], **shard, **subset)
            run(f"{name}.{dev.__name__}", dev, cam, world, *particular, stream=3 * D, **d_all)
            run(f"{name}.{dev.__name__}[subset]", dev, cam, world, *particular, first_sample=4, **shard, **d_some, **subset)
            run(f"{name}.{pix.__name__}", pix, cam, world, xs, ys, *particular)
            run(f"{name}.{pix.__name__}[want]", pix, cam, world, xs, ys, *particular, first_sample=1, want=outputs[1:], **subset)
            run(f"{name}.{pixdev.__name__}", pixdev, cam, world, D, 2 * D, 3, *particular, stream=3 * D, **d_all)
            run(f"{name}.{pixdev.__name__}[subset]", pixdev, cam, world, D, 2 * D, 3, *particular, first_sample=1, **d_some, **subset)
            for tag, kw in routes.items():
                run(f"{name}.{rows.__name__}[{tag}]", rows, cam, world, **kw)
                run(f"{name}.{dev.__name__}[{tag}]", dev, cam, world, **d_some, **kw)
                run(f"{name}.{pix.__name__}[{tag}]", pix, cam, world, xs, ys, **kw)
                run(f"{name}.{pixdev.__name__}[{tag}]", pixdev, cam, world, D, 2 * D, 3, **d_all, **kw)

        family(ao, "ao", ("open", "hits"), 4, 1.5)
        family(direct, "direct", ("direct", "unshadowed", "hits"), quad, 2, subset={"seg_tmax": 0.5})
        family(nee, "nee", ("sums", "sq"), quad, 2, subset={"seg_tmax": 0.5})
        family(nee, "nee_mis", ("sums", "sq"), quad, 2, subset={"seg_tmax": 0.5, "heuristic": "power"},
               routes={"spheres": {"lights": quad, "light_samples": 2, "sphere_lights": ball},
                       "spheres, no lights": {"lights": [], "light_samples": 3, "heuristic": "power", "sphere_lights": ball}})

        # ---- the C++ mirror's probes: the host library's rlh_*_probe, noted by HostProbes
        run("direct.cpp_mirror_probe", direct.cpp_mirror_probe, 4, 2, 1, quad, 2)
        run("nee.cpp_mirror_probe", nee.cpp_mirror_probe, 4, 2, 1, quad, 3, seg_tmax=0.5)
        run("nee.cpp_mirror_probe_mis", nee.cpp_mirror_probe_mis, 4, 2, 1, quad, 2, heuristic="power")
        run("nee.cpp_mirror_probe_spheres", nee.cpp_mirror_probe_spheres, 4, 2, 1, quad, ball, 2)
        run("nee.cpp_mirror_probe_spheres[power, no lights]", nee.cpp_mirror_probe_spheres, 4, 2, 0, [], ball, 3, seg_tmax=0.5, heuristic="power")
    finally:
        for w in worlds:  # the handles are the recorder's: nothing of the real library may ever see them
            w._device = None
    return out


def names_render_lib(api):
    """The public callables of Camera, World, RtcWorld and api itself whose source names render_lib()."""
    import inspect
    names = []
    for owner, label in ((api.Camera, "Camera."), (api.World, "World."), (api.RtcWorld, "RtcWorld."), (api, "")):
        for k, f in vars(owner).items():
            f = getattr(f, "__func__", f)
            if k.startswith("_") or k in ("render_lib", "host_lib") or not inspect.isfunction(f) or f.__module__ != api.__name__:
                continue
            if "render_lib()" in inspect.getsource(f):
                names.append(label + k)
    return names


def covered_wrappers(api, at_least=()):
    """What drive() has to call.  Of api: `at_least` and whatever else names_render_lib finds (a wrapper that reaches the library through
    a shared form does not name it, so the rule alone would let it go).  Of the FAMILY_MODULES, by exclusion: every public function
    defined there but the PURE_PACKERS, labelled "module.name"."""
    import importlib
    import inspect
    names = list(at_least) + [n for n in names_render_lib(api) if n not in at_least]
    for m in FAMILY_MODULES:
        mod = importlib.import_module(f"{api.__package__}.{m}")
        names += [f"{m}.{k}" for k, f in vars(mod).items()
                  if not k.startswith("_") and inspect.isfunction(f) and f.__module__ == mod.__name__ and k not in PURE_PACKERS]
    return names
