"""The ctypes binding is read from include/e2ep.h: the header parser on declarations written
out here, the real header's table, and the built library exporting every declared symbol (CPU
only; no compute call is made without a GPU)."""
import ctypes
import os
import re

import pytest

from conftest import ROOT

CODES = {ctypes.c_void_p: "p", ctypes.c_int: "i", ctypes.c_longlong: "i64", ctypes.c_float: "f",
         ctypes.c_double: "d", ctypes.c_size_t: "sz", ctypes.c_char_p: "s"}


def _codes(sig):
    res, args = sig
    return CODES[res], [CODES[a] for a in args]


def _declared():
    src = open(os.path.join(ROOT, "include", "e2ep.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(e2ep_[a-z0-9_]+)\s*\(", src)))


SAMPLE = """
/* a block comment with a declaration inside: int e2ep_not_this(int a);
 * and a second line */
#ifndef E2EP_H
#define E2EP_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif
#define E2EP_EINVAL (-1) /* bad shape / argument */
#define E2EP_IO_X_BF16 1  /* the input activation x */
#define E2EP_LSS_TILE 64
int e2ep_abi_version(void);
const char *e2ep_last_error(void);
size_t e2ep_ws(int B, int XYZ);
int e2ep_wrapped(const float *prob, const int32_t *offsets,
                 int B, long long bev_bstride,
                 float p, double lr,
                 void *stream, int io /* 0, or E2EP_IO_X_BF16 */);
int e2ep_tables(const long long *table, const int *dims, const float *const *srcs, int n,
                int64_t value, uint8_t *mask, size_t workspace_bytes);
#ifdef __cplusplus
}
#endif
#endif
"""


def test_parser_on_written_out_declarations():
    from e2ep_amd import _lib
    sigs, consts = _lib.parse_header(SAMPLE)
    assert list(sigs) == ["e2ep_abi_version", "e2ep_last_error", "e2ep_ws", "e2ep_wrapped",
                          "e2ep_tables"]
    assert _codes(sigs["e2ep_abi_version"]) == ("i", [])                    # (void)
    assert _codes(sigs["e2ep_last_error"]) == ("s", [])                     # const char * return
    assert _codes(sigs["e2ep_ws"]) == ("sz", ["i", "i"])                    # size_t return
    # four lines, a comment inside the argument list, long long by int, double by float
    assert _codes(sigs["e2ep_wrapped"]) == ("i", ["p", "p", "i", "i64", "f", "d", "p", "i"])
    # const long long *table and const int *dims are pointers, not scalars
    assert _codes(sigs["e2ep_tables"]) == ("i", ["p", "p", "p", "i", "i64", "p", "sz"])
    # parenthesised negative value, trailing comment; the include guard (no value) is no constant
    assert consts == {"E2EP_EINVAL": -1, "E2EP_IO_X_BF16": 1, "E2EP_LSS_TILE": 64}


@pytest.mark.parametrize("decl, named", [
    ("int e2ep_bad(const float *x, unsigned n);", "e2ep_bad"),          # unknown scalar type
    ("int e2ep_bad(struct e2ep_dims d, void *stream);", "e2ep_bad"),    # by-value struct
    ("float *e2ep_bad(int n);", "e2ep_bad"),                            # pointer return
    ("int e2ep_bad(int);", "e2ep_bad"),                                 # unnamed argument
    ("int e2ep_bad(void (*cb)(int), int n);", "e2ep_bad"),              # function pointer
])
def test_parser_raises_on_what_it_cannot_map(decl, named):
    from e2ep_amd import _lib
    with pytest.raises(_lib.E2EPError, match=named):
        _lib.parse_header("int e2ep_fine(int a);\n" + decl)


def test_missing_header_raises(tmp_path, monkeypatch):
    from e2ep_amd import _lib
    monkeypatch.setattr(_lib, "HEADER_PATH", str(tmp_path / "absent.h"))
    monkeypatch.setattr(_lib, "_HEADER", None)
    with pytest.raises(_lib.E2EPError, match="absent.h"):
        _lib.SIGNATURES


def test_header_declares_the_boundary():
    names = _declared()
    for must in ("e2ep_geom_index", "e2ep_lss_plan", "e2ep_lss_fwd", "e2ep_lss_bwd", "e2ep_target_bev"):
        assert must in names


def test_real_header_table():
    from e2ep_amd import _lib
    sigs = _lib.SIGNATURES
    assert set(sigs) == set(_declared())  # every declaration parsed, nothing else
    assert len(sigs) >= 149
    assert len(sigs["e2ep_bn_bwd"][1]) == 25
    assert len(sigs["e2ep_se_bwd_bn"][1]) == 26
    assert _codes(sigs["e2ep_adam_step"]) == (
        "i", ["p", "i", "p", "p", "p", "p", "p", "p", "p", "p", "d", "d", "d", "d", "f", "p", "p"])
    assert _codes(sigs["e2ep_grad_gather"]) == ("i", ["p", "i", "p", "p", "p", "p"])
    bce = ["p", "p", "i", "i", "i", "i", "i", "f", "f", "p", "p", "p", "p", "p"]
    assert _codes(sigs["e2ep_depth_bce_fwd"]) == ("i", bce)
    assert _codes(sigs["e2ep_depth_bce_fwd_f64"]) == ("i", [{"f": "d"}.get(c, c) for c in bce])
    assert _codes(sigs["e2ep_last_error"]) == ("s", [])
    assert _codes(sigs["e2ep_conv_fwd_workspace"]) == ("sz", ["p"])
    # host arrays and out-parameters are plain pointers too (ctypes arrays and byref() pass)
    assert _codes(sigs["e2ep_geom_index"])[1][3:5] == ["p", "p"]
    assert _codes(sigs["e2ep_capture_unjoined"]) == ("i", ["p", "p", "p"])
    assert _lib.CONSTANTS == {"E2EP_EINVAL": -1, "E2EP_ERANGE": -2, "E2EP_IO_X_BF16": 1,
                              "E2EP_IO_DY_BF16": 2, "E2EP_IO_DX_BF16": 4, "E2EP_LSS_TILE": 64}
    assert _lib.io_mask() == 0 and _lib.io_mask(x=True, dx=True) == 5 and _lib.io_mask(dy=True) == 2


def test_library_exports_every_declared_symbol():
    from e2ep_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail("libe2ep_hip.so not built; run __graft_entry__.build()")
    lib = _lib.load()
    for name in _declared():
        assert hasattr(lib, name), name
    assert set(_declared()) <= set(_lib.SIGNATURES), "ctypes table misses a declared entry point"
    assert lib.e2ep_abi_version() == 4


def test_library_is_gfx950_code_object():
    from e2ep_amd import _lib
    blob = open(_lib.LIB_PATH, "rb").read()
    assert b"gfx950" in blob


def test_dwconv_bf16_predicate_host_only():
    """e2ep_dwconv_bf16_ok is a host-side geometry predicate (no GPU call): the MBConv
    depthwise shapes of the C3 step take bf16 storage, geometries without a strip kernel or with
    planes not a multiple of 4 do not.  dims = (N, C, H, W, K, P, Q, stride, pad_top, pad_left)."""
    from e2ep_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail("libe2ep_hip.so not built; run __graft_entry__.build()")
    lib = _lib.load()

    def ok(*d):
        return lib.e2ep_dwconv_bf16_ok((ctypes.c_int * 10)(*d))

    assert ok(32, 192, 64, 64, 3, 64, 64, 1, 1, 1) == 1     # k3 s1
    assert ok(32, 336, 32, 32, 5, 32, 32, 1, 2, 2) == 1     # k5 s1
    assert ok(32, 144, 128, 128, 3, 64, 64, 2, 0, 0) == 1   # k3 s2
    assert ok(2, 32, 30, 30, 3, 30, 30, 1, 1, 1) == 0       # W % 4 != 0
    assert ok(2, 16, 16, 16, 7, 16, 16, 1, 3, 3) == 0       # K = 7
    assert ok(2, 32, 18, 18, 5, 9, 9, 2, 2, 2) == 0         # 9 x 9 output
    assert ok(0, 32, 16, 16, 3, 16, 16, 1, 1, 1) == 0       # empty batch
