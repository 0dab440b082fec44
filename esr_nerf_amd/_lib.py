"""ctypes binding of libesr_hip.so (include/esr_hip.h).

The library is the product: if it is missing or fails to load, everything that
needs it raises -- there is no CPU or PyTorch fallback on the product path.
"""
from __future__ import annotations

import ctypes as C
import os
import re

import torch

from .build import HEADER, LIB as LIB_PATH
# developer experiments only (python -m esr_nerf_amd.build --variant builds alternative libraries; tools/ab_env.sh times them
# side by side on one box)
LIB_PATH = os.environ.get("ESR_LIB_PATH", LIB_PATH)
_lib = None


class EsrScene(C.Structure):
    _fields_ = [
        ("xyz_min", C.c_float * 3), ("xyz_max", C.c_float * 3),
        ("mask_min", C.c_float * 3), ("mask_max", C.c_float * 3),
        ("gx", C.c_int32), ("gy", C.c_int32), ("gz", C.c_int32),
        ("mx", C.c_int32), ("my", C.c_int32), ("mz", C.c_int32),
        ("near_", C.c_float), ("stepdist", C.c_float), ("voxel_size", C.c_float),
        ("act_shift", C.c_float), ("mask_thres", C.c_float), ("fast_thres", C.c_float),
        ("s_val", C.c_float), ("max_steps", C.c_int32), ("grad_feat", C.c_float * 4),
    ]


class EsrPlan(C.Structure):
    _fields_ = [(n, C.c_int32) for n in
                ("n_on", "n_off", "tiles_on", "tiles_all", "m0", "m1", "m2", "overflow")]


class EsrMarch(C.Structure):               # esr_march_t
    _fields_ = [("scene", C.POINTER(EsrScene))] + \
               [(n, C.c_void_p) for n in ("rays_o", "rays_d", "viewdirs", "mask_density", "sdf", "gg")] + \
               [("n_rays", C.c_int32), ("flags", C.c_int32)] + \
               [(n, C.c_void_p) for n in ("cnt3", "alphainv_last", "cum_weights", "ray_stats", "plan", "off3", "rec_ray",
                                          "rec_step", "rec_w", "rec_sdf", "dweight", "dlast", "grad_sdf", "grad_gg",
                                          "dsdf_rec")] + \
               [("accumulate", C.c_int32), ("cache", C.c_void_p)]


class EsrFeatArgs(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("rays_o", "rays_d", "viewdirs", "rec_ray", "rec_step", "rec_sdf",
                                          "pts", "pt_viewdirs", "pt_sdf")] + \
               [("n_pts", C.c_int32), ("sdf", C.c_void_p), ("color_on", C.c_void_p * 3),
                ("color_off", C.c_void_p * 3), ("tiles_on", C.c_int32), ("tiles_all", C.c_int32)]


class EsrFeatBwdSrc(C.Structure):
    _fields_ = [("dX", C.c_void_p), ("grad_color_on", C.c_void_p), ("grad_color_off", C.c_void_p),
                ("t0", C.c_int32), ("t1", C.c_int32)]


class EsrLtsArgs(C.Structure):
    _fields_ = [("n_pts", C.c_int32), ("n_rays", C.c_int32), ("n_sg", C.c_int32), ("pdra_mode", C.c_int32)] + \
               [(n, C.c_void_p) for n in ("base", "rough", "metal", "normal", "view", "dirs", "off_m", "emo_m",
                                          "last2", "mus", "lambdas", "lobes", "emission", "umask")]


class EsrLtsGather(C.Structure):          # esr_lts_gather_t
    _fields_ = [(n, C.c_void_p) for n in ("jp", "ray64", "pts_all", "eg", "rec_sdf", "viewdirs", "brdf_a", "emit_a",
                                          "umask_rays")] + [("n_pts", C.c_int32)] + \
               [(n, C.c_void_p) for n in ("pts2", "vd2", "sdf2", "normal", "base", "rough", "metal", "emis", "umask", "pt1")]


class EsrActJob(C.Structure):             # esr_act_job_t
    _fields_ = [("z", C.c_void_p), ("g_tile", C.c_void_p), ("out", C.c_void_p), ("tiles", C.c_int32), ("rows", C.c_int32),
                ("n_ch", C.c_int32), ("act", C.c_int32), ("bwd", C.c_int32), ("src", C.c_void_p), ("src_c", C.c_int32),
                ("n_src", C.c_int32), ("inv", C.c_void_p), ("pt1", C.c_void_p), ("ex", C.c_void_p * 3),
                ("ex_c", C.c_int32 * 3), ("ex_col0", C.c_int32 * 3)]


class EsrGatherJob(C.Structure):          # esr_gather_job_t
    _fields_ = [("src", C.c_void_p), ("tile_rows", C.c_int32), ("row_stride", C.c_int32), ("col0", C.c_int32),
                ("n_ch", C.c_int32), ("perm", C.c_void_p), ("n", C.c_int32), ("out", C.c_void_p)]


class EsrPairJob(C.Structure):            # esr_pair_job_t
    _fields_ = [("a", C.c_void_p), ("b", C.c_void_p), ("rows", C.c_int64), ("cols", C.c_int32), ("row_mask", C.c_void_p),
                ("mask_value", C.c_int32), ("count_dev", C.c_void_p), ("kind", C.c_int32), ("w_value", C.c_float),
                ("w_a", C.c_float), ("w_b", C.c_float), ("ga", C.c_void_p), ("gb", C.c_void_p)]


class EsrLtsGrads(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("d_off_m", "d_emo_m", "d_last2", "d_base", "d_rough", "d_metal",
                                          "d_emission", "d_mus", "d_lambdas", "d_lobes")]


class EsrCdIndex(C.Structure):           # esr_cd_index_t
    _fields_ = [("origin", C.c_double * 3), ("h", C.c_double), ("dims", C.c_int32 * 3), ("coarse", C.c_int32),
                ("cap", C.c_int64), ("keys", C.c_void_p), ("cells", C.c_void_p), ("start", C.c_void_p), ("pts", C.c_void_p),
                ("ids", C.c_void_p), ("ccap", C.c_int64), ("ckeys", C.c_void_p)]


class EsrDvgo(C.Structure):             # esr_dvgo_t
    _fields_ = [("density", C.c_void_p), ("off_color", C.c_void_p), ("emo_color", C.c_void_p), ("dims", C.c_int32 * 3),
                ("xyz_min", C.c_float * 3), ("xyz_max", C.c_float * 3)] + \
               [(n, C.c_float) for n in ("near_", "far_", "step_scale", "interval", "act_shift")] + [("n_samples", C.c_int32)]


class EsrDvgoRays(C.Structure):         # esr_dvgo_rays_t
    _fields_ = [(n, C.c_void_p) for n in ("rays_o", "rays_d", "nrm", "jitter", "em_modes")] + \
               [("em_all", C.c_int32), ("n_rays", C.c_int64)]


class EsrDvgoOut(C.Structure):          # esr_dvgo_out_t
    _fields_ = [(n, C.c_void_p) for n in ("alpha", "alphainv_cum", "weights", "raw_rgb", "rgb", "depth", "disp", "white_bg",
                                          "off_rgb", "on_rgb", "emo_rgb")]


class EsrDvgoBwd(C.Structure):          # esr_dvgo_bwd_t
    _fields_ = [(n, C.c_void_p) for n in ("alpha", "alphainv_cum", "raw_rgb", "g_alphainv_cum", "g_weights", "g_raw_rgb",
                                          "g_rgb", "grad_density", "grad_off", "grad_emo")]


class EsrViewPost(C.Structure):         # esr_view_post_t
    _fields_ = [("v", C.c_void_p), ("wbg", C.c_void_p), ("wbg_scale", C.c_float), ("lin", C.c_int32), ("n", C.c_int64),
                ("channels", C.c_int32)] + \
               [(n, C.c_void_p) for n in ("out", "gamma", "out_u8", "gamma_u8", "target_out", "target_gamma", "partials",
                                          "sqerr")]


class EsrCamera(C.Structure):           # esr_camera_t
    _fields_ = [(n, C.c_float) for n in ("fx", "fy", "cx", "cy")] + [(n, C.c_int32) for n in ("width", "height", "n_views")]


class EsrRegroupStats(C.Structure):     # esr_regroup_stats_t
    _fields_ = [(n, C.c_int64) for n in ("n_set", "n_clear", "n_nan")] + \
               [(n, C.c_float) for n in ("min_all", "max_all", "min_set", "max_set", "min_clear", "max_clear")]


class EsrSurfaceLight(C.Structure):     # esr_surface_light_t
    _fields_ = [("nodes", C.c_void_p), ("n_faces", C.c_int64), ("vertices", C.c_void_p), ("n_vertices", C.c_int64),
                ("triangles", C.c_void_p), ("n_sources", C.c_int64), ("slots", C.c_int32), ("mode", C.c_int32)] + \
               [(n, C.c_void_p) for n in ("l_point", "l_normal", "l_weight", "l_radiance", "l_face")] + \
               [("n_points", C.c_int64)] + \
               [(n, C.c_void_p) for n in ("p_point", "p_normal", "p_base", "p_rough", "p_metal", "p_wo")] + \
               [("eps", C.c_double), ("out", C.c_void_p), ("seen", C.c_void_p)]


class EsrMlpWeights(C.Structure):
    _fields_ = [("w", C.c_void_p * 4), ("b", C.c_void_p * 4)]


class EsrWgradJob(C.Structure):
    """esr_wgrad_job_t"""
    _fields_ = [("kind", C.c_int32), ("color_row0", C.c_int32), ("t0", C.c_int32), ("t1", C.c_int32),
                ("X", C.c_void_p), ("H", C.c_void_p), ("dZ", C.c_void_p), ("dz", C.c_void_p),
                ("gw", C.c_void_p), ("gb", C.c_void_p), ("X16", C.c_void_p), ("amax", C.c_void_p)]


# The C ABI is declared once, in include/esr_hip.h: its integer #defines are this module's constants (ESR_ABI_VERSION ->
# ABI_VERSION, ESR_PARTITION_BLOCK -> PARTITION_BLOCK, ...), and SIGNATURES -- entry -> (restype, argtypes), in header order --
# is parsed from its prototypes, so ctypes converts and checks every argument of every call: a bare Python int reaches an
# int64_t parameter whole, a bare float a float or double one.  EXPORTS lists the entries.  A new entry point is declared in
# the header and defined in its .hip file; only a new struct needs a class above.
_SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "float": C.c_float, "double": C.c_double}
_RESTYPES = {"int": C.c_int, "int64_t": C.c_int64, "const char *": C.c_char_p}
# the pointers that stay typed (every other one is a c_void_p: call sites pass byref()s, pointer arrays and plain addresses)
_TYPED_POINTERS = {
    **{(f"esr_march_{w}", "a"): C.POINTER(EsrMarch) for w in ("count", "fill", "bwd")},
    ("esr_nonempty_mask", "mask_box_host"): C.POINTER(C.c_float), ("esr_density_bounds", "box_host"): C.POINTER(C.c_float),
}


def _parse_header(path):
    """(integer #defines without their ESR_ prefix, SIGNATURES) of the header; a prototype it cannot type is an error."""
    with open(path) as f:
        text = re.sub(r"/\*.*?\*/|//[^\n]*", "", f.read(), flags=re.S)
    defines = {n: int(v) for n, v in re.findall(r"^[ \t]*#[ \t]*define[ \t]+ESR_(\w+)[ \t]+\(?(-?\d+)\)?[ \t]*$", text, re.M)}
    signatures, pointers = {}, set()
    for res, name, params in re.findall(r"^[ \t]*(int|int64_t|const char \*)\s*(esr_\w+)\s*\(([^)]*)\)\s*;", text, re.M):
        args = []
        for param in (" ".join(p.split()) for p in params.split(",") if p.strip() != "void"):
            m = re.fullmatch(r"(.*?)(\w+)", param)
            ctype, pname = m.group(1).strip(), m.group(2)
            if ctype.endswith("*"):
                args.append(_TYPED_POINTERS.get((name, pname), C.c_void_p))
                pointers.add((name, pname))
            elif ctype in _SCALARS:
                args.append(_SCALARS[ctype])
            else:
                raise RuntimeError(f"{path}: {name}: parameter `{param}` has a type the ctypes binding does not know")
        signatures[name] = (_RESTYPES[res], args)
    if set(_TYPED_POINTERS) - pointers:
        raise RuntimeError(f"{path}: not pointer parameters of the header: {sorted(set(_TYPED_POINTERS) - pointers)}")
    unparsed = set(re.findall(r"\b(esr_\w+)\s*\(", text)) - set(signatures)
    if unparsed:
        raise RuntimeError(f"{path}: prototypes the ctypes binding cannot read: {sorted(unparsed)}")
    return defines, signatures


_defines, SIGNATURES = _parse_header(HEADER)
globals().update(_defines)
EXPORTS = list(SIGNATURES)


def lib() -> C.CDLL:
    """Load the HIP library; raises (never falls back) when it is unavailable."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: build it with `python -m esr_nerf_amd.build` "
                "(there is no CPU fallback for the HIP path)")
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            if hasattr(L, name):               # (a variant library may lack an entry)
                getattr(L, name).restype, getattr(L, name).argtypes = res, args
        if L.esr_abi_version() != ABI_VERSION:
            raise RuntimeError("libesr_hip.so ABI version mismatch: rebuild")
        _lib = L
    return _lib


def check(code: int, what: str):
    if code != 0:
        raise RuntimeError(f"{what} failed with code {code}" +
                           (" (hipError)" if code > 0 else
                            " (a capacity limit of the kernels is exceeded, include/esr_hip.h: ESR_ECAP)" if code == -2 else
                            " (bad argument)"))


def ptr(t):
    """Device pointer of a contiguous CUDA(HIP) tensor (or NULL for None)."""
    if t is None:
        return C.c_void_p(0)
    if not t.is_cuda:
        raise RuntimeError("esr_hip ops need device tensors (got a CPU tensor)")
    if not t.is_contiguous():
        raise RuntimeError("esr_hip ops need contiguous tensors")
    return C.c_void_p(t.data_ptr())


_dev_index = {}


def stream_ptr(device=None):
    """The current HIP stream of ``device`` as a void pointer.  (``torch.cuda.current_stream(device).cuda_stream`` builds a
    Stream object per call, ~5 us; a light-transport step asks ~100 times -- the raw getter is what torch's own
    compiled code uses.)"""
    idx = _dev_index.get(device)
    if idx is None:
        idx = torch.cuda.current_device() if device is None else torch.device(device).index
        if idx is None:
            idx = torch.cuda.current_device()            # ("cuda" without an index: not cached)
        elif device is not None:
            _dev_index[device] = idx
    return C.c_void_p(torch._C._cuda_getCurrentRawStream(idx))


def ptr_array(tensors, n=None):
    n = n or len(tensors)
    arr = (C.c_void_p * n)()
    for i, t in enumerate(tensors):
        arr[i] = 0 if t is None else t.data_ptr()
    return arr
