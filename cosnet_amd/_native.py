"""ctypes binding of libcosnet_hip.so (the C ABI declared in include/cosnet_hip.h).

The library is the only compute path: if it is missing or cannot be loaded on a GPU box,
every op raises instead of falling back to anything else.  torch must be imported before
the library is loaded so that both share torch's HIP runtime (same soname).
"""
import ctypes
import os
import re

import torch  # noqa: F401  (loads the HIP runtime the library binds to)

_HERE = os.path.dirname(os.path.abspath(__file__))
# COSNET_HIP_LIB: development override (tools/ A/B builds); the package loads the in-tree build
LIB_PATH = os.environ.get("COSNET_HIP_LIB") or os.path.join(_HERE, "_lib", "libcosnet_hip.so")

DT_F32 = 0
DT_BF16 = 1

HEADER = os.path.join(_HERE, "..", "include", "cosnet_hip.h")
# inference extensions: launches that replace a pair of reference calls (conv2d + eval BatchNorm2d);
# a table of their own, so the core header's entry points stay the set its tests pin
HEADER_INFER = os.path.join(_HERE, "..", "include", "cosnet_hip_infer.h")
# the same pairs on static-scale fp8 operands: again a table of its own, for the same reason
HEADER_INFER_FP8 = os.path.join(_HERE, "..", "include", "cosnet_hip_infer_fp8.h")
# the bank head's split reduce conv (the per-frame partial and the conv that adds it): likewise
HEADER_INFER_HEAD = os.path.join(_HERE, "..", "include", "cosnet_hip_infer_head.h")


class NativeError(RuntimeError):
    pass


# The closed set of C types the ABI may use: by value these, any pointer as a void*, and a
# const char* result.  A new type has to be admitted here on purpose: signatures() raises on
# anything else instead of guessing int.
_CTYPES = {"int": ctypes.c_int, "long long": ctypes.c_longlong, "float": ctypes.c_float,
           "double": ctypes.c_double, "size_t": ctypes.c_size_t, "hipStream_t": ctypes.c_void_p}
_RESTYPES = {"int": ctypes.c_int, "size_t": ctypes.c_size_t, "const char*": ctypes.c_char_p}


def signatures(header_text):
    """{name: (restype, [argtypes], [parameter names])} of every cn_* prototype in the text of
    include/cosnet_hip.h: the header is the binding, nothing is transcribed by hand."""
    text = re.sub(r"/\*.*?\*/", " ", header_text, flags=re.S)      # comments, also inside parameter lists
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)
    sigs = {}
    for ret, name, params in re.findall(r"^(\w[\w \t*]*?)\s*\b(cn_\w+)\(([^)]*)\);", text, re.M):
        if ret not in _RESTYPES:
            raise NativeError("%s: result type %r is not one the binding admits" % (name, ret))
        types, names = [], []
        for prm in ([] if params.strip() == "void" else params.split(",")):
            ctype, pname = re.fullmatch(r"(.*?)\s*(\w+)", " ".join(prm.split())).groups()
            value = ctype[6:] if ctype.startswith("const ") else ctype
            if "*" not in ctype and value not in _CTYPES:
                raise NativeError("%s: parameter %r has type %r, not one the binding admits" % (name, pname, ctype))
            types.append(ctypes.c_void_p if "*" in ctype else _CTYPES[value])
            names.append(pname)
        sigs[name] = (_RESTYPES[ret], types, names)
    return sigs


_sigs = None
_ext_sigs = None
_fp8_ext_sigs = None
_head_ext_sigs = None


def _signatures():
    global _sigs
    if _sigs is None:
        with open(HEADER) as fh:
            _sigs = signatures(fh.read())
    return _sigs


def _extension_signatures():
    global _ext_sigs
    if _ext_sigs is None:
        with open(HEADER_INFER) as fh:
            _ext_sigs = signatures(fh.read())
    return _ext_sigs


def _fp8_extension_signatures():
    global _fp8_ext_sigs
    if _fp8_ext_sigs is None:
        with open(HEADER_INFER_FP8) as fh:
            _fp8_ext_sigs = signatures(fh.read())
    return _fp8_ext_sigs


def _head_extension_signatures():
    global _head_ext_sigs
    if _head_ext_sigs is None:
        with open(HEADER_INFER_HEAD) as fh:
            _head_ext_sigs = signatures(fh.read())
    return _head_ext_sigs


def _signature(name):
    """The prototype of one entry point, from whichever header declares it."""
    return (_signatures().get(name) or _extension_signatures().get(name)
            or _fp8_extension_signatures().get(name) or _head_extension_signatures()[name])


_lib = None


def load():
    """Load the library (once).  Raises NativeError if it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise NativeError("libcosnet_hip.so not built (%s); run __graft_entry__.build()" % LIB_PATH)
    lib = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL)
    for name, (res, args, _) in (list(_signatures().items()) + list(_extension_signatures().items())
                                   + list(_fp8_extension_signatures().items())
                                   + list(_head_extension_signatures().items())):
        # an A/B build of an older tree (COSNET_HIP_LIB) may lack the newest entry points; the
        # in-tree product library must export every one
        if os.environ.get("COSNET_HIP_LIB") and not hasattr(lib, name):
            continue
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


HASHED_SOURCES = ["gemm.hip", "gemm_ws.hip", "conv.hip", "bn.hip", "ew.hip", "coatt.hip", "coatt_fused.hip",
                  "coatt_q48.hip", "coatt_flash.hip", "coatt_f8.hip", "fp8.hip", "frames.hip", "eval.hip",
                  "../../include/cosnet_hip_infer_fp8.h", "../../include/cosnet_hip_infer_head.h", "common.h", "gemm.h", "gemm_dev.h", "coatt_fused.h", "../../include/cosnet_hip.h",
                  "../../include/cosnet_hip_infer.h"]   # csrc/Makefile HASHED, same order


def source_hash():
    """SHA-256 (16 hex digits) of the HIP sources in this tree, as the Makefile stamps it."""
    import hashlib
    h = hashlib.sha256()
    for f in HASHED_SOURCES:
        with open(os.path.join(_HERE, "csrc", f), "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


def build_info():
    """{library hash stamped at build, this tree's source hash, match, library sha256}."""
    import hashlib
    lib_hash = load().cn_build_source_hash().decode()
    with open(LIB_PATH, "rb") as fh:
        so = hashlib.sha256(fh.read()).hexdigest()[:16]
    src = source_hash()
    return {"lib_source_hash": lib_hash, "tree_source_hash": src, "built_from_tree": lib_hash == src,
            "lib_sha256": so, "lib": os.path.relpath(LIB_PATH, os.path.dirname(_HERE))}


def exported_symbols():
    return sorted(_signatures())


def extension_symbols():
    """The entry points of include/cosnet_hip_infer.h (exported_symbols() stays the core header's)."""
    return sorted(_extension_signatures())


def fp8_extension_symbols():
    """The entry points of include/cosnet_hip_infer_fp8.h."""
    return sorted(_fp8_extension_signatures())


def head_extension_symbols():
    """The entry points of include/cosnet_hip_infer_head.h."""
    return sorted(_head_extension_signatures())


_ERR = {-1: "shape", -2: "alignment", -3: "unsupported", -4: "hip runtime"}


def call(name, *args):
    """Invoke one C-ABI entry point; non-zero status -> NativeError."""
    try:
        rc = getattr(load(), name)(*args)
    except ctypes.ArgumentError as e:   # "argument 9: TypeError: ..." -> name the C parameter
        i = int(re.match(r"argument (\d+)", str(e)).group(1))
        raise NativeError("%s: argument %d (%s): %s" % (name, i, _signature(name)[2][i - 1], e)) from e
    if rc != 0:
        raise NativeError("%s failed: %s (%d)" % (name, _ERR.get(rc, "hipError"), rc))
    return rc


def query(name, *args):
    return getattr(load(), name)(*args)


def stream():
    return torch.cuda.current_stream().cuda_stream


def ptr(t):
    return None if t is None else t.data_ptr()


def dtype_code(dt):
    if dt == torch.bfloat16:
        return DT_BF16
    if dt == torch.float32:
        return DT_F32
    raise NativeError("unsupported compute dtype %s" % dt)
