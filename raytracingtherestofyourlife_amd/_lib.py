"""ctypes binding of librtp.so: the one table of its C signatures (SIGNATURES,
a group of rows per header: include/rtp.h, rtp_mesh.h, rtp_adaptive.h, and the
internal hooks), the one place that applies it (bind, which load() calls; a
tool binds its A/B library with it too), the structs and the pointer helpers.
A new entry point is a row in its header's group, in the header's order.

There is no CPU fallback: if the HIP library is missing or fails to load,
every entry point raises.  The product path is the HIP path.
"""
from __future__ import annotations

import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RTP_LIB_PATH") or os.path.join(_HERE, "librtp.so")  # override: experiments only

RTP_OK = 0
RTP_ERR_INVALID_ARGUMENT = -1
RTP_ERR_NO_SCENE = -2
RTP_ERR_DEVICE = -3
RTP_ERR_OUT_OF_MEMORY = -4

f32p = ctypes.POINTER(ctypes.c_float)
i32p = ctypes.POINTER(ctypes.c_int32)
u32p = ctypes.POINTER(ctypes.c_uint32)
i64p = ctypes.POINTER(ctypes.c_int64)
vp = ctypes.c_void_p  # rtp_context*, void*, and every device buffer: callers hold addresses


class RtpCamera(ctypes.Structure):
    _fields_ = [("position", ctypes.c_float * 3), ("look_at", ctypes.c_float * 3),
                ("view_up", ctypes.c_float * 3), ("fov_y_deg", ctypes.c_float)]


class RtpView(ctypes.Structure):
    _fields_ = [("camera", RtpCamera), ("seed_base", ctypes.c_uint32)]


class RtpSceneDesc(ctypes.Structure):
    _fields_ = [
        ("points", f32p), ("n_points", ctypes.c_int32),
        ("quad_points", i32p), ("quad_mat", i32p), ("quad_tex", i32p), ("n_quads", ctypes.c_int32),
        ("sphere_point", i32p), ("sphere_radius", f32p), ("sphere_mat", i32p), ("sphere_tex", i32p),
        ("n_spheres", ctypes.c_int32),
        ("mat_type", i32p), ("n_mat", ctypes.c_int32),
        ("tex_type", i32p), ("n_tex_type", ctypes.c_int32),
        ("tex_rgb", f32p), ("n_tex", ctypes.c_int32),
        ("light_quad_points", ctypes.c_int32 * 4), ("light_sphere_point", ctypes.c_int32),
        ("ior", ctypes.c_float),
    ]


class RtpStats(ctypes.Structure):
    _fields_ = [("samples", ctypes.c_uint64), ("live_bounces", ctypes.c_uint64),
                ("nan_pixels", ctypes.c_uint64), ("kernel_ms", ctypes.c_double)]


class RtpPixelAux(ctypes.Structure):
    _fields_ = [("final_seed", u32p), ("live_bounces", u32p)]


class RtpRenderState(ctypes.Structure):
    """rtp_render_state: the arrays a render is continued from (device or host
    pointers matching the call)."""
    _fields_ = [("rgba", f32p), ("seed", u32p), ("live_bounces", u32p), ("m2", f32p)]


class RtpDirectDesc(ctypes.Structure):
    _fields_ = [("clip_near", ctypes.c_float), ("clip_far", ctypes.c_float), ("background", ctypes.c_float * 4),
                ("composite_background", ctypes.c_int32), ("quad_scalar", f32p), ("color_map", f32p),
                ("color_map_size", ctypes.c_int32)]


class RtpDenoiseParams(ctypes.Structure):
    _fields_ = [("levels", ctypes.c_int32), ("sigma_l", ctypes.c_float), ("sigma_z", ctypes.c_float),
                ("sigma_a", ctypes.c_float), ("normal_log2", ctypes.c_int32)]


class RtpRefineParams(ctypes.Structure):
    """rtp_refine_params (include/rtp_adaptive.h)."""
    _fields_ = [("threshold", ctypes.c_float), ("spp", ctypes.c_int32), ("max_spp", ctypes.c_int32)]


RTP_AOV_COLOR, RTP_AOV_NORMALS, RTP_AOV_ALBEDO = 1, 2, 4
RTP_FF_TABLES_AUTO, RTP_FF_TABLES_OFF, RTP_FF_TABLES_ON = 0, 1, 2


class RtpFfInfo(ctypes.Structure):
    _fields_ = [("policy", ctypes.c_int32), ("built", ctypes.c_int32), ("chain_tables", ctypes.c_int32),
                ("direct_first", ctypes.c_int32), ("direct_count", ctypes.c_int32), ("bytes", ctypes.c_uint64),
                ("alloc_ms", ctypes.c_double), ("build_ms", ctypes.c_double), ("samples_seen", ctypes.c_uint64),
                ("auto_samples", ctypes.c_uint64), ("auto_samples_direct", ctypes.c_uint64)]


# rtp::DbgCounter (csrc/rtp_layout.hpp) in its order, then the extra slot
# rtp_debug_counters fills on request: the longest wave lifetime.
DEBUG_COUNTERS = ("bounce_steps", "bounce_lanes", "ff_phases", "ff_lanes", "ff_iters", "cycles_bounce",
                  "cycles_ff", "cycles_total", "cycles_intersect", "cycles_bounce_call", "cycles_end",
                  "cycles_refill", "real_start", "real_end", "hw_id", "tail_steps", "tail_lanes",
                  "tail_cycles", "fallback_steps", "fallback_lanes", "refill_visits", "refill_lanes",
                  "hit_visits", "hit_lanes", "gen_visits", "gen_lanes", "cycles_gen", "cycles_pdf", "end_visits",
                  "end_lanes", "ffrad_visits", "ffrad_lanes", "ffrad_rows", "dead_lanes", "diel_visits", "diel_lanes",
                  "cycles_diel", "light_visits", "light_lanes", "box_free_steps", "box_lanes",
                  "max_wave_cycles")
N_DBG_COUNTERS = len(DEBUG_COUNTERS) - 1  # rtp::kDbgCounters: the width of a per-wave record


# The internal hooks that Python code of this repository calls (the package's
# mesh helpers, the tests, the tools): exported beside the public entry points
# and declared, for the C++ units, in these two headers of csrc/.
HOOKS = "hooks"
HOOK_HEADERS = ("rtp_launch_decl.hpp", "rtp_mesh.hpp")


def _signatures() -> dict:
    """Every function Python calls in librtp.so, grouped by the header that
    declares it and in that header's order: group -> name -> (restype, argtypes)."""
    i32, u32, i64, st = ctypes.c_int32, ctypes.c_uint32, ctypes.c_int64, ctypes.c_int32  # st: rtp_status
    P = ctypes.POINTER
    u64p, d64p = P(ctypes.c_uint64), P(ctypes.c_double)
    cam, stats, aux, state = P(RtpCamera), P(RtpStats), P(RtpPixelAux), P(RtpRenderState)
    desc, prm = P(RtpSceneDesc), P(RtpRefineParams)
    cint, cintp = ctypes.c_int, P(ctypes.c_int)  # the launcher header's plain C types
    return {"include/rtp.h": {
        "rtp_last_error": (ctypes.c_char_p, []),
        "rtp_abi_version": (i32, []),
        "rtp_create": (st, [i32, P(vp)]),
        "rtp_destroy": (None, [vp]),
        "rtp_set_scene": (st, [vp, desc]),
        "rtp_render": (st, [vp, cam, i32, i32, i32, i32, u32, f32p, stats]),
        "rtp_render_tiles_device": (st, [vp, cam, i32, i32, i32, i32, u32, i32, i32, vp, vp, stats]),
        "rtp_render_device": (st, [vp, cam, i32, i32, i32, i32, u32, i64, i64, vp, vp, aux, vp, stats]),
        "rtp_render_planned_device": (st, [vp, cam, i32, i32, i32, i32, u32, i64, i64, vp, vp, i32, vp, aux, vp,
                                           stats]),
        "rtp_render_pixels": (st, [vp, cam, i32, i32, i32, i32, u32, i64p, i64, f32p, aux, stats]),
        "rtp_render_views_device": (st, [vp, P(RtpView), i32, i32, i32, i32, i32, vp, aux, vp, stats]),
        "rtp_render_views": (st, [vp, P(RtpView), i32, i32, i32, i32, i32, f32p, stats]),
        "rtp_render_resume_device": (st, [vp, cam, i32, i32, i32, i32, i64, i64, vp, state, vp, stats]),
        "rtp_render_resume": (st, [vp, cam, i32, i32, i32, i32, i64p, i64, state, stats]),
        "rtp_render_guides_device": (st, [vp, cam, i32, i32, vp, vp, vp, vp, stats]),
        "rtp_render_guides": (st, [vp, cam, i32, i32, f32p, f32p, i32p, stats]),
        "rtp_resolve_device": (st, [vp, vp, vp, vp, i32, i64, vp, vp, stats]),
        "rtp_resolve": (st, [vp, f32p, f32p, i32p, i32, i64, f32p, stats]),
        "rtp_denoise_device": (st, [vp, vp, vp, vp, i32, i32, P(RtpDenoiseParams), vp, vp, vp, stats]),
        "rtp_denoise": (st, [vp, f32p, f32p, f32p, i32, i32, P(RtpDenoiseParams), f32p, stats]),
        "rtp_normalize": (st, [f32p, i64, i32]),
        "rtp_write_pnm": (st, [ctypes.c_char_p, f32p, i32, i32]),
        "rtp_cornell_box": (st, [i32, desc]),
        "rtp_render_direct": (st, [vp, cam, i32, i32, P(RtpDirectDesc), f32p, f32p, f32p, f32p, stats]),
        "rtp_render_direct_device": (st, [vp, cam, i32, i32, P(RtpDirectDesc), vp, vp, vp, vp, vp, stats]),
        "rtp_sample_color_table": (st, [d64p, i32, d64p, i32, d64p, i32, f32p]),
        "rtp_quad_scalars": (st, [f32p, i32, i32p, i32, f32p]),
        "rtp_cornell_point_field": (st, [i32, P(f32p), P(i32), P(i32p), P(i32)]),
        "rtp_write_pnm_depth": (st, [ctypes.c_char_p, f32p, i32, i32]),
        "rtp_eval_powf": (st, [vp, f32p, ctypes.c_float, f32p, i64]),
        "rtp_set_ff_tables": (st, [vp, i32]),
        "rtp_get_ff_tables": (st, [vp, P(RtpFfInfo)]),
        "rtp_eval_primitive": (st, [vp, i32, vp, vp, i64]),
        "rtp_debug_counters": (i32, [vp, u64p, i32]),
        "rtp_debug_closest_hit": (st, [vp, vp, i64, vp]),
        "rtp_debug_bounce": (st, [vp, vp, vp, i64, vp]),
        "rtp_debug_raygen": (st, [vp, cam, i32, i32, i64p, P(u32), i64, P(u32)]),
        "rtp_sphere_walk": (i32, [vp]),
        "rtp_sphere_walk_oct_mask": (i32, [vp]),
        "rtp_verify_fast_math": (st, [vp, i32, u32, u32, u64p, P(u32)]),
    }, "include/rtp_mesh.h": {
        "rtp_set_scene_mesh": (st, [vp, desc]),
        "rtp_mesh_guarantee": (st, [vp, f32p, f32p]),
        "rtp_mesh_counts": (st, [vp, i32p, i32p, i32p]),
        "rtp_set_scene_mesh_device": (st, [vp, desc, vp]),
    }, "include/rtp_adaptive.h": {
        "rtp_noise_device": (st, [vp, vp, vp, vp, i64, vp, vp, stats]),
        "rtp_noise": (st, [vp, f32p, f32p, i32p, i64, f32p, stats]),
        "rtp_select_active_device": (st, [vp, vp, vp, vp, i64, prm, vp, vp, vp, stats]),
        "rtp_refine_device": (st, [vp, cam, i32, i32, i32, state, vp, prm, i64p, vp, stats]),
        "rtp_refine": (st, [vp, cam, i32, i32, i32, state, i32p, prm, i64p, stats]),
        "rtp_render_adaptive_device": (st, [vp, cam, i32, i32, i32, state, vp, prm, i32, i64p, P(i32), vp, stats]),
        "rtp_refine_last_timing": (st, [vp, d64p]),
        "rtp_normalize_counts": (st, [f32p, i32p, i64]),
    }, HOOKS: {
        # csrc/rtp_launch_decl.hpp
        "rtp_instance_name": (ctypes.c_char_p, [cint] * 8),
        "rtp_plan_history_lanes": (i64, [i64, cint, cint, cint, cintp, cintp]),
        "rtp_plan_steal": (cint, [i64, cint]),
        # csrc/rtp_mesh.hpp
        "rtp_mesh_build_host": (st, [desc, i32, i32, i32p, vp, i32p, f32p, f32p, f32p]),
        "rtp_mesh_leaf_size": (i32, []),
        "rtp_mesh_compact_host": (None, [vp, i64, u32p]),
        "rtp_mesh_scan_host": (st, [desc, f32p, i64, u32p]),
        "rtp_debug_mesh_readback": (st, [vp, i32, i32, i32p, vp, i32p, f32p, f32p]),
        "rtp_debug_mesh_records": (st, [vp, i64, vp]),
    }}


SIGNATURES = _signatures()
EXPORTED_SYMBOLS = list(SIGNATURES["include/rtp.h"])


def bind(L: ctypes.CDLL) -> list:
    """Apply every row of SIGNATURES to L: the names L does not export."""
    missing = []
    for group in SIGNATURES.values():
        for name, (restype, argtypes) in group.items():
            try:
                fn = getattr(L, name)
            except AttributeError:
                missing.append(name)
                continue
            fn.restype, fn.argtypes = restype, argtypes
    return missing


class RtpError(RuntimeError):
    def __init__(self, status: int, msg: str):
        super().__init__(f"rtp error {status}: {msg}")
        self.status = status


class ErrorBadValue(ValueError):
    """vtkm::cont::ErrorBadValue."""


_lib = None


def load(build_if_missing: bool = True) -> ctypes.CDLL:
    """Load librtp.so (building it with hipcc first if it is absent)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        if not build_if_missing:
            raise RuntimeError(f"{LIB_PATH} is missing; run raytracingtherestofyourlife_amd/build.py")
        from . import build as _build
        _build.build()
    # One HIP runtime per process: torch bundles a libamdhip64 with the same
    # soname (libamdhip64.so.7) as /opt/rocm's.  Loading torch's first makes
    # librtp.so bind to it (soname match), so torch streams/allocations and
    # our launches share one runtime.  Without torch, /opt/rocm's is used.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = ctypes.CDLL(LIB_PATH)
    # An experiment library named by RTP_LIB_PATH may be built from a revision
    # before any of the symbols (tools/build_variant.sh RTP_SRC_REV, the A/B
    # baselines of the tools/*_bench.py): it loads without them, and calling
    # one raises AttributeError.  The in-tree library must export them all.
    missing = bind(L)
    if missing and not os.environ.get("RTP_LIB_PATH"):
        raise RuntimeError(f"{LIB_PATH} does not export {', '.join(missing)}; rebuild it "
                           "(raytracingtherestofyourlife_amd/build.py)")
    _lib = L
    return L


def check(status: int) -> None:
    if status != RTP_OK:
        raise RtpError(status, load().rtp_last_error().decode(errors="replace"))


# ------------------------------------------------------------ pointers --
# What ctypes converts by itself once argtypes are declared needs no helper:
# an int (0 = NULL) or None for a c_void_p argument, an instance for a
# POINTER(T) argument.  The two conversions it leaves to the caller:
_POINTEE = {"float32": ctypes.c_float, "float64": ctypes.c_double, "int32": ctypes.c_int32,
            "uint32": ctypes.c_uint32, "int64": ctypes.c_int64, "uint64": ctypes.c_uint64}


def ptr(a):
    """A numpy array's memory as the pointer type of its dtype (None: NULL).
    The array is the caller's to keep contiguous and alive across the call."""
    return None if a is None else a.ctypes.data_as(ctypes.POINTER(_POINTEE[a.dtype.name]))


def _field(x, ptype):
    """A typed pointer for a struct field from what a caller holds: a host
    array (its dtype must be the field's) or a device address (0 or None: NULL)."""
    if hasattr(x, "ctypes"):
        return ptr(x)
    return ctypes.cast(x, ptype) if x else None


def pixel_aux(seed, live) -> RtpPixelAux:
    """rtp_pixel_aux of two optional buffers: host uint32 arrays or device addresses."""
    return RtpPixelAux(_field(seed, u32p), _field(live, u32p))


def render_state(rgba, seed, live=None, m2=None) -> RtpRenderState:
    """rtp_render_state likewise (rgba, m2: float32; seed, live: uint32)."""
    return RtpRenderState(_field(rgba, f32p), _field(seed, u32p), _field(live, u32p), _field(m2, f32p))
