"""ctypes binding of libdepgan.so, derived from include/depgan.h (the C ABI).

The header is the one statement of the boundary: parse_header() reads every prototype, the all-reduce typedef, the
integer #defines, the enums and depgan_config from it, and load() binds the library from that.  Nothing here restates a
signature.  There is no CPU fallback: if the HIP library is missing the import fails loudly.
"""
from __future__ import annotations

import collections
import ctypes as C
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DEPGAN_LIB") or os.path.join(HERE, "libdepgan.so")   # DEPGAN_LIB: A/B another build
HEADER_PATH = os.path.join(HERE, "..", "include", "depgan.h")                    # build.source_hash() reads it too


class DepganError(RuntimeError):
    pass


# The header's closed type vocabulary.  Every pointer or array parameter is a c_void_p (the header cannot tell a device
# float* from a host one), except char* / const char*; any other scalar type is an error, never a guess.
_SCALARS = {"int": C.c_int, "long": C.c_long, "float": C.c_float, "double": C.c_double, "unsigned": C.c_uint}
_RETURNS = dict(_SCALARS, size_t=C.c_size_t, void=None)

Header = collections.namedtuple("Header", "prototypes allreduce_fn constants config_fields")


def _ctype(decl, scalars, where, named=True):
    """ctypes type of one C declaration: a parameter (`named`: its last word is the name) or a return type."""
    decl = " ".join(decl.split())
    if "[" in decl:
        return C.c_void_p
    if "*" in decl:
        return C.c_char_p if decl.rpartition("*")[0].split() in (["char"], ["const", "char"]) else C.c_void_p
    ctype = decl.rpartition(" ")[0] if named else decl
    if ctype not in scalars:
        raise DepganError("include/depgan.h: %s: no ctypes mapping for `%s`" % (where, decl))
    return scalars[ctype]


def _signature(ret, params, scalars, where):
    params = [] if params.strip() in ("", "void") else params.split(",")
    return _ctype(ret, _RETURNS, where, named=False), [_ctype(p, scalars, where) for p in params]


def read_header(path=HEADER_PATH):
    try:
        with open(path) as f:
            return f.read()
    except OSError as e:
        raise DepganError("cannot read the C ABI header %s: %s" % (os.path.abspath(path), e))


def parse_header(text):
    """Everything the binding needs from the text of include/depgan.h, as a Header:
    prototypes {name: (restype, argtypes)} in header order, the CFUNCTYPE of depgan_allreduce_fn (None if absent),
    constants {name: int} of the integer #defines and the enums, and the (name, ctype) fields of depgan_config."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    defines = re.findall(r"^[ \t]*#[ \t]*define[ \t]+(DEPGAN_\w+)[ \t]+(-?\d+)[ \t]*$", text, re.M)
    constants = {k: int(v) for k, v in defines}
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)
    for body in re.findall(r"\benum\s*\{([^}]*)\}", text):
        constants.update((k, int(v)) for k, v in re.findall(r"(\w+)\s*=\s*(-?\d+)", body))
    config = re.search(r"typedef struct depgan_config \{(.*?)\} depgan_config;", text, re.S)
    fields = []
    for decl in (config.group(1).split(";") if config else []):
        if decl.strip():
            ctype, names = decl.split(None, 1)
            fields += [(n.strip(), _ctype(ctype + " " + n, _SCALARS, "depgan_config")) for n in names.split(",")]
    scalars, allreduce = dict(_SCALARS), None
    hook = re.search(r"typedef([\w\s*]+?)\(\s*\*\s*depgan_allreduce_fn\s*\)\s*\(([^()]*)\)\s*;", text)
    if hook:
        ret, args = _signature(hook.group(1), hook.group(2), _SCALARS, "depgan_allreduce_fn")
        allreduce = scalars["depgan_allreduce_fn"] = C.CFUNCTYPE(ret, *args)
    found = re.findall(r"(?:\A|(?<=[;{}]))\s*([\w\s*]+?)\b(depgan_\w+)\s*\(([^()]*)\)\s*;", text)
    names, called = [name for _, name, _ in found], re.findall(r"\b(depgan_\w+)\s*\(", text)
    if called != names:      # every prototype is also in `called`, in the same order: the first difference is the stray
        stray = next(a for a, b in zip(called, names + [None]) if a != b)
        raise DepganError("include/depgan.h: `%s(` is not a prototype this binding can read" % stray)
    prototypes = collections.OrderedDict((name, _signature(ret, params, scalars, name)) for ret, name, params in found)
    return Header(prototypes, allreduce, constants, fields)


_HDR = parse_header(read_header())
_K = _HDR.constants

EXPORTS = list(_HDR.prototypes)          # every depgan_* entry, in header order
ABI_VERSION = 3          # the ABI engine.py's call sites were written against; load() holds header and library to it
MAX_MULTI, MAX_CRITIC_STEPS = _K["DEPGAN_MAX_MULTI"], _K["DEPGAN_MAX_CRITIC_STEPS"]
RCCL_ID_BYTES = _K["DEPGAN_RCCL_ID_BYTES"]
EVAL_NCOUNT, EVAL_LABEL_NCOUNT = _K["DEPGAN_EVAL_NCOUNT"], _K["DEPGAN_EVAL_LABEL_NCOUNT"]
MAX_HEAD_CLASSES = _K["DEPGAN_MAX_HEAD_CLASSES"]     # a softmax head has 2 .. this many classes
NET_G, NET_D_Y2, NET_D_DEM = (_K["DEPGAN_NET_" + n] for n in ("G", "D_Y2", "D_DEM"))
ARENA_PARAMS, ARENA_NONTRAINABLE, ARENA_GRADS, ARENA_ADAM_M, ARENA_ADAM_V = (
    _K["DEPGAN_ARENA_" + n] for n in ("PARAMS", "NONTRAINABLE", "GRADS", "ADAM_M", "ADAM_V"))

# int fn(void* user, float* dev_ptr, long n, void* hip_stream): the all-reduce hook of depgan_set_allreduce
ALLREDUCE_FN = _HDR.allreduce_fn


class Config(C.Structure):
    """depgan_config of include/depgan.h, field for field."""
    _fields_ = _HDR.config_fields

    def __init__(self, **kw):
        super().__init__(**kw)
        self.struct_size = C.sizeof(Config)


_lib = None


def _bind(lib, name):
    fn = getattr(lib, name)
    fn.restype, fn.argtypes = _HDR.prototypes[name]
    return fn


def load():
    """Load libdepgan.so; raises if it has not been built (python -m dep_gan_im_amd.build)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise DepganError(
            "libdepgan.so not found at %s -- the HIP library is the product; build it with "
            "`python -m dep_gan_im_amd.build` (needs hipcc). There is no CPU fallback." % LIB_PATH)
    # PyTorch-ROCm ships its own HIP runtime.  It must be in the process BEFORE libdepgan.so is loaded, so that the
    # library binds to that runtime: loaded the other way round, two runtimes coexist and hipMalloc inside the
    # library reports "no ROCm-capable device is detected".
    import torch  # noqa: F401
    lib = C.CDLL(LIB_PATH)
    abi, size = _bind(lib, "depgan_abi_version")(), _bind(lib, "depgan_config_size")()
    if {abi, _K.get("DEPGAN_ABI_VERSION")} != {ABI_VERSION} or size != C.sizeof(Config):
        raise DepganError("libdepgan.so at %s has ABI %d / depgan_config of %d bytes, this binding expects ABI %d / %d "
                          "bytes: rebuild with `python -m dep_gan_im_amd.build`"
                          % (LIB_PATH, abi, size, ABI_VERSION, C.sizeof(Config)))
    if os.path.isdir(os.path.join(HERE, "csrc")) and not os.environ.get("DEPGAN_LIB"):
        from .build import source_hash
        built, here = _bind(lib, "depgan_source_hash")().decode(), source_hash()
        if built != here:
            raise DepganError("libdepgan.so at %s was built from other sources (hash %s, the sources here hash to %s): "
                              "rebuild with `python -m dep_gan_im_amd.build`" % (LIB_PATH, built, here))
    for name in EXPORTS:
        _bind(lib, name)
    _lib = lib
    return lib


def check(rc, what=""):
    if rc != 0:
        msg = load().depgan_last_error()
        raise DepganError("%s failed (status %d): %s" % (what or "libdepgan call", rc,
                                                         msg.decode() if msg else "?"))


_hip = None


def hip():
    """libamdhip64 for raw device copies (weights in/out of the C-side arenas)."""
    global _hip
    if _hip is None:
        last = None
        for name in ("libamdhip64.so", "/opt/rocm/lib/libamdhip64.so", "libamdhip64.so.7", "libamdhip64.so.6"):
            try:
                _hip = C.CDLL(name)
                break
            except OSError as e:  # pragma: no cover
                last = e
        if _hip is None:
            raise DepganError("cannot load libamdhip64: %s" % last)
        _hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        _hip.hipDeviceSynchronize.argtypes = []
    return _hip


H2D, D2H, D2D = 1, 2, 3


def memcpy(dst, src, nbytes, kind):
    rc = hip().hipMemcpy(C.c_void_p(dst), C.c_void_p(src), C.c_size_t(nbytes), C.c_int(kind))
    if rc != 0:
        raise DepganError("hipMemcpy failed with status %d" % rc)
