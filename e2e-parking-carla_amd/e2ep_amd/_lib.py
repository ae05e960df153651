"""ctypes binding of libe2ep_hip.so (C ABI: include/e2ep.h).

The library is built in-tree by csrc/Makefile (or __graft_entry__.build()).  There is no
fallback: if it is missing or fails to load, every op raises — the product path never
silently degrades to PyTorch or CPU code.
"""
import ctypes
import os
import re

import torch  # noqa: F401  (loads torch's libamdhip64 first, so the library binds to it)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("E2EP_LIB", os.path.join(_HERE, "libe2ep_hip.so"))

HEADER_PATH = os.environ.get("E2EP_HEADER", os.path.join(_HERE, "..", "..", "include", "e2ep.h"))

_POINTER = ctypes.c_void_p  # every pointer argument, host or device, typed or void
_SCALARS = {"int": ctypes.c_int, "int32_t": ctypes.c_int, "long long": ctypes.c_longlong,
            "int64_t": ctypes.c_longlong, "float": ctypes.c_float, "double": ctypes.c_double,
            "size_t": ctypes.c_size_t}


class E2EPError(RuntimeError):
    pass


def _ctype(decl, text, ret=False):
    """ctypes type of one argument (`type name`) or, with ret, of a return type."""
    words = [w for w in text.replace("*", " * ").split() if w != "const"]
    if ret and words == ["char", "*"]:
        return ctypes.c_char_p
    if "*" in words and not ret:
        return _POINTER
    kind = " ".join(words if ret else words[:-1])  # an argument's last word is its name
    if kind not in _SCALARS:
        raise E2EPError(f"e2ep.h: cannot map `{text.strip()}` of `{decl}` to ctypes")
    return _SCALARS[kind]


def parse_header(text):
    """(signatures, constants) of the C ABI from the text of e2ep.h: name -> (restype,
    argtypes) for every `ret name(args);`, and name -> int for every `#define E2EP_* <int>`.
    A declaration whose types are not in the table above raises: nothing is guessed."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    consts = {m[1]: int(m[2]) for m in re.finditer(
        r"^[ \t]*#[ \t]*define[ \t]+(E2EP_\w+)[ \t]+\(?[ \t]*(-?\d+)[ \t]*\)?[ \t]*$", text, re.M)}
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)
    sigs = {}
    for m in re.finditer(r"([^;{}]+);", text):
        decl = " ".join(m[1].split())
        d = re.fullmatch(r"(.+?)(\w+) ?\(([^()]*)\)", decl)
        if d is None:
            raise E2EPError(f"e2ep.h: cannot parse `{decl}`")
        args = [] if d[3].strip() in ("", "void") else d[3].split(",")
        sigs[d[2]] = (_ctype(decl, d[1], ret=True), [_ctype(decl, a) for a in args])
    return sigs, consts


_HEADER = None


def _header():
    """The parsed header, read once per process on first use (load(), SIGNATURES, CONSTANTS)."""
    global _HEADER
    if _HEADER is None:
        try:
            with open(HEADER_PATH) as f:
                text = f.read()
        except OSError as e:
            raise E2EPError(f"C ABI header unavailable ({HEADER_PATH}): {e}") from None
        _HEADER = parse_header(text)
    return _HEADER


def __getattr__(name):
    if name == "SIGNATURES":  # name -> (restype, argtypes)
        return _header()[0]
    if name == "CONSTANTS":  # the header's integer E2EP_* macros
        return _header()[1]
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


def io_mask(x=False, dy=False, dx=False):
    """The `io` argument (E2EP_IO_*): which of a call's tensors are stored bf16."""
    c = _header()[1]
    return ((c["E2EP_IO_X_BF16"] if x else 0) | (c["E2EP_IO_DY_BF16"] if dy else 0)
            | (c["E2EP_IO_DX_BF16"] if dx else 0))


_LIB = None
_ERR = None


def load():
    """Load and bind the library once; raise E2EPError if it is not there."""
    global _LIB, _ERR
    if _LIB is not None:
        return _LIB
    if _ERR is not None:
        raise _ERR
    signatures = _header()[0]
    try:
        lib = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL)
        for name, (res, args) in signatures.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
    except (OSError, AttributeError) as e:
        _ERR = E2EPError(f"libe2ep_hip.so unavailable ({LIB_PATH}): {e}. Build it with "
                         f"`make -C e2e-parking-carla_amd/csrc` or __graft_entry__.build().")
        raise _ERR
    _LIB = lib
    if os.environ.get("E2EP_CONV_VARIANT"):  # A/B timing of the conv GEMM kernel choice
        lib.e2ep_conv_gemm_variant(int(os.environ["E2EP_CONV_VARIANT"]))
    if os.environ.get("E2EP_GEMM_SKINNY"):  # A/B timing of the few-row GEMM path
        lib.e2ep_gemm_skinny(int(os.environ["E2EP_GEMM_SKINNY"]))
    if os.environ.get("E2EP_CONV_SPLIT"):  # "target,thresh[,wgrad_target]" for A/B timing
        v = [int(x) for x in os.environ["E2EP_CONV_SPLIT"].split(",")] + [0]
        lib.e2ep_conv_split_params(v[0], v[1], v[2])
    if os.environ.get("E2EP_BN_SMALL_LIMITS"):  # "fwd_max_vec,bwd_max_vec" for A/B timing
        f, b = (int(x) for x in os.environ["E2EP_BN_SMALL_LIMITS"].split(","))
        lib.e2ep_bn_small_limits(f, b)
    if os.environ.get("E2EP_TUNE"):  # "key=value,..." launch-plan tunables for A/B timing
        for kv in os.environ["E2EP_TUNE"].split(","):
            k, v = kv.split("=")
            lib.e2ep_tune(int(k), int(v))
    if os.environ.get("E2EP_GEMM_SPLIT_MIN"):  # A/B timing of small-grid K splits
        lib.e2ep_gemm_split_min(int(os.environ["E2EP_GEMM_SPLIT_MIN"]))
    return lib


def call(name, *args):
    lib = load()
    rc = getattr(lib, name)(*args)
    if rc != 0:
        raise E2EPError(f"{name} failed ({rc}): {lib.e2ep_last_error().decode()}")


def call_raw(name, *args):
    """Call an entry point that returns a value rather than a status."""
    return getattr(load(), name)(*args)


def ptr(t):
    """Device pointer of a tensor (None -> NULL)."""
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def nbytes(t):
    """Size in bytes of a workspace tensor (None -> 0), passed with it as workspace_bytes."""
    return 0 if t is None else t.numel() * t.element_size()


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def dims(vals):
    """A host int32 array (kept alive by the caller for the duration of the call)."""
    return (ctypes.c_int * len(vals))(*[int(v) for v in vals])


def host3(vals):
    return (ctypes.c_float * 3)(*[float(v) for v in vals])
