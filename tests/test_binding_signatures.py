"""CPU tier: the two signature tables of api.py (RENDER_SIGNATURES, HOST_SIGNATURES) against the C text they restate — the
declarations of include/rl_render.h, the rl_debug_* definitions under csrc/ and the rlh_* definitions in host/*.cpp — read by the
prototype parser of tests/binding_model.py.  A table entry with a wrong width, a wrong signedness, a scalar where C takes a pointer, a
missing or default restype on a function that returns a pointer, or an entry point without a table line fails here."""
import ctypes
import os
import re

import pytest

import binding_model as bm


@pytest.fixture(scope="module")
def api(rl):
    return rl.api


def struct_names(api):
    return {api.RtiowCamera: "rl_rtiow_camera", api.RtcCamera: "rl_rtc_camera", api.Stats: "rl_stats", api.RtiowAdaptive: "rl_rtiow_adaptive",
            api.RtiowFeatures: "rl_rtiow_features", api.AtrousParams: "rl_atrous_params", api.DenoiseInputs: "rl_denoise_inputs",
            api._HCameraParams: "rlh_camera_params"}


def mismatches(api, table, c_side):
    """Every way in which table entries differ from the C prototypes of the same names."""
    names, bad = struct_names(api), []
    for name, (c_ret, c_params) in c_side.items():
        restype, argtypes = table[name]
        if not bm.same_class(c_ret, bm.ctypes_class(restype, names)):
            bad.append(f"{name}: returns {c_ret}, restype {restype}")
        if len(argtypes) != len(c_params):
            bad.append(f"{name}: {len(c_params)} parameters, {len(argtypes)} argtypes")
            continue
        for i, (c, t) in enumerate(zip(c_params, argtypes)):
            if not bm.same_class(c, bm.ctypes_class(t, names)):
                bad.append(f"{name}: parameter {i} is {c}, argtypes[{i}] {t}")
    return bad


def test_the_parser_classifies_every_prototype():
    # counts as the sources stand; a new entry point moves them together with the tables
    header, debug, host = bm.header_prototypes(), bm.debug_prototypes(), bm.host_prototypes()
    assert len(header) >= 75 and len(debug) >= 35 and len(host) >= 61
    assert all(n.startswith("rl_") and not n.startswith("rl_debug_") for n in header)
    with pytest.raises(ValueError):
        bm.prototypes("int rl_x(struct_of_no_known_kind v);", ";", r"rl_\w+")
    # unsigned long long and uint64_t are one class; a pointer carries its rl_* pointee
    p = bm.prototypes("unsigned long long rl_a(uint64_t n, const rl_stats *s, double v[3]); /* int rl_b(void); */", ";", r"rl_\w+")
    assert p == {"rl_a": (("int", 8, False), [("int", 8, False), ("ptr", "rl_stats"), ("ptr", ("float", 8))])}


def test_render_table_public_part_is_the_header(api):
    header = bm.header_prototypes()
    public = {n: s for n, s in api.RENDER_SIGNATURES.items() if not n.startswith("rl_debug_")}
    assert sorted(public) == sorted(header)
    assert api.RENDER_SYMBOLS == list(public)
    assert mismatches(api, public, header) == []


def test_typed_pointers_name_the_c_struct(api):
    """Where the C side takes one of the structs the binding mirrors, the table says so (a c_void_p there would accept anything)."""
    names = struct_names(api)
    mirrored = set(names.values())
    c_side = dict(bm.header_prototypes(), **bm.host_prototypes())
    for table in (api.RENDER_SIGNATURES, api.HOST_SIGNATURES):
        for name, (_, argtypes) in table.items():
            if name.startswith("rl_debug_"):
                continue
            for i, (c, t) in enumerate(zip(c_side[name][1], argtypes)):
                if c[0] == "ptr" and c[1] in mirrored:
                    assert bm.ctypes_class(t, names) == c, (name, i, c, t)


def test_render_table_debug_part_is_the_definitions(api):
    debug = bm.debug_prototypes()
    table = {n: s for n, s in api.RENDER_SIGNATURES.items() if n.startswith("rl_debug_")}
    assert sorted(table) == sorted(debug)
    assert mismatches(api, table, debug) == []


def test_host_table_is_the_definitions_and_covers_api(api):
    host = bm.host_prototypes()
    table = api.HOST_SIGNATURES
    assert set(table) <= set(host), sorted(set(table) - set(host))
    assert mismatches(api, table, {n: host[n] for n in table}) == []
    src = open(os.path.join(bm.PKG, "api.py")).read()
    used = set(re.findall(r"\brlh_\w+", src))
    assert used - set(table) == set(), sorted(used - set(table))
    for name, (restype, _) in table.items():  # a pointer cut to 32 bits is the failure this table exists to prevent
        if host[name][0] is not None and host[name][0][0] == "ptr":
            assert restype in (ctypes.c_void_p, ctypes.c_char_p), name


def test_no_signature_is_assigned_outside_the_loader(api):
    src = open(os.path.join(bm.PKG, "api.py")).read()
    lines = [ln.strip() for ln in src.splitlines() if re.search(r"\.(argtypes|restype)\b.*=[^=]", ln) and not ln.lstrip().startswith(("#", '"'))]
    assert lines == ["fn.restype, fn.argtypes = restype, argtypes"], lines


def test_loaded_libraries_carry_the_tables(api):
    verify_only = {"rl_debug_fastg_verify", "rl_debug_fastg_counts"}  # csrc/rl_render.hip defines them under RL_FASTG_VERIFY (make verify)
    for lib, table in ((api.render_lib(), api.RENDER_SIGNATURES), (api.host_lib(), api.HOST_SIGNATURES)):
        for name, (restype, argtypes) in table.items():
            if not hasattr(lib, name):  # the loader skips what a build lacks; of this tree's builds only the two above may be absent
                assert name in verify_only, name
                continue
            fn = getattr(lib, name)
            assert fn.restype is restype, name
            assert list(fn.argtypes) == list(argtypes), name
