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


# The C ABI is declared once, in include/esr_hip.h: its integer #defines are this module's constants (ESR_ABI_VERSION ->
# ABI_VERSION, ESR_PARTITION_BLOCK -> PARTITION_BLOCK, ...), every `typedef struct ... esr_x_y_t` is this module's
# ctypes.Structure EsrXY with the header's fields in the header's order, and SIGNATURES -- entry -> (restype, argtypes), in
# header order -- is parsed from its prototypes, so ctypes converts and checks every argument of every call: a bare Python int
# reaches an int64_t parameter whole, a bare float a float or double one.  EXPORTS lists the entries.  A new struct, like a new
# entry point, is declared in the header only (and the entry defined in its .hip file); nothing here changes for either.
_SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "float": C.c_float, "double": C.c_double}
_RESTYPES = {"int": C.c_int, "int64_t": C.c_int64, "const char *": C.c_char_p}
# (entry or struct, parameter or field) -> C type of the pointee, for the pointers that stay typed: [host] structs and boxes,
# which ctypes should type-check.  Every other pointer is a c_void_p (a device address: call sites pass plain addresses,
# pointer arrays and byref()s).
_TYPED_POINTERS = {
    **{(f"esr_march_{w}", "a"): "esr_march_t" for w in ("count", "fill", "bwd")}, ("esr_march_t", "scene"): "esr_scene_t",
    ("esr_nonempty_mask", "mask_box_host"): "float", ("esr_density_bounds", "box_host"): "float",
}
# (an __attribute__((aligned(16))) on the tag -- esr_bvh_node -- is skipped: it changes neither the size nor an offset of that
# struct, and its instances live in device memory only, so ctypes never has to place one)
_STRUCT = re.compile(r"typedef\s+struct\s*(?:__attribute__\s*\(\(aligned\(\d+\)\)\)\s*)?(?:\w+\s*)?"
                     r"\{([^{}]*)\}\s*(esr_\w+)_t\s*;")


def _parse_header(path):
    """(integer #defines without their ESR_ prefix, class name -> Structure, SIGNATURES) of the header; a field, a struct or a
    prototype it cannot type is an error."""
    with open(path) as f:
        text = re.sub(r"/\*.*?\*/|//[^\n]*", "", f.read(), flags=re.S)
    defines = {n: int(v) for n, v in re.findall(r"^[ \t]*#[ \t]*define[ \t]+ESR_(\w+)[ \t]+\(?(-?\d+)\)?[ \t]*$", text, re.M)}
    structs, signatures, pointers = {}, {}, set()

    def pointer(owner, name):
        pointers.add((owner, name))
        if (owner, name) not in _TYPED_POINTERS:
            return C.c_void_p
        pointee = _TYPED_POINTERS[owner, name]
        return C.POINTER(_SCALARS[pointee] if pointee in _SCALARS else structs[pointee])

    for body, tag in _STRUCT.findall(text):
        fields = []
        for decl in (" ".join(d.split()) for d in body.split(";") if d.strip()):
            base, _, declarators = decl.removeprefix("const ").partition(" ")
            for d in declarators.split(", "):
                m = re.fullmatch(r"((?:\*(?:const )?)*)(\w+)((?:\[\w+\])*)", d)
                if not m:
                    raise RuntimeError(f"{path}: {tag}_t: the ctypes binding cannot read the declaration `{decl}`")
                star, name, dims = m.groups()
                if not star and base not in _SCALARS:
                    raise RuntimeError(f"{path}: {tag}_t: field `{name}` has a type the ctypes binding does not know: `{decl}`")
                ctype = pointer(tag + "_t", name) if star else _SCALARS[base]
                for n in reversed(re.findall(r"\w+", dims)):      # T x[N][M] is (T * M) * N
                    if not n.isdigit() and (n[:4] != "ESR_" or n[4:] not in defines):
                        raise RuntimeError(f"{path}: {tag}_t: field `{name}`: `{n}` is neither a number nor an integer macro of the header")
                    ctype = ctype * (int(n) if n.isdigit() else defines[n[4:]])
                fields.append((name, ctype))
        structs[tag + "_t"] = type("".join(w.capitalize() for w in tag.split("_")), (C.Structure,), {"_fields_": fields})
    unparsed = re.findall(r"\bstruct\b[^;{]*", _STRUCT.sub("", text))
    if unparsed:
        raise RuntimeError(f"{path}: structs the ctypes binding cannot read: {sorted(' '.join(u.split()) for u in unparsed)}")
    for res, name, params in re.findall(r"^[ \t]*(int|int64_t|const char \*)\s*(esr_\w+)\s*\(([^)]*)\)\s*;", text, re.M):
        args = []
        for param in (" ".join(p.split()) for p in params.split(",") if p.strip() != "void"):
            m = re.fullmatch(r"(.*?)(\w+)", param)
            ctype, pname = m.group(1).strip(), m.group(2)
            if ctype.endswith("*"):
                args.append(pointer(name, pname))
            elif ctype in _SCALARS:
                args.append(_SCALARS[ctype])
            else:
                raise RuntimeError(f"{path}: {name}: parameter `{param}` has a type the ctypes binding does not know")
        signatures[name] = (_RESTYPES[res], args)
    if set(_TYPED_POINTERS) - pointers:
        raise RuntimeError(f"{path}: not pointers of the header: {sorted(set(_TYPED_POINTERS) - pointers)}")
    unparsed = set(re.findall(r"\b(esr_\w+)\s*\(", text)) - set(signatures)
    if unparsed:
        raise RuntimeError(f"{path}: prototypes the ctypes binding cannot read: {sorted(unparsed)}")
    return defines, {c.__name__: c for c in structs.values()}, signatures


_defines, _structs, SIGNATURES = _parse_header(HEADER)
globals().update(_defines)
globals().update(_structs)
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
                            " (a capacity limit of the kernels is exceeded, include/esr_hip.h: ESR_ECAP)" if code == ECAP else
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
