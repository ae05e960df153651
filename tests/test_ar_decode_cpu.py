"""The incremental decode path away from the GPU: its gate, its ABI table entries, and that
CPU callers of predict_tokens get what they got before (no GPU needed)."""
import ctypes
import os

import pytest
import torch

NEW = ("e2ep_dec_self_attn", "e2ep_dec_cross_attn", "e2ep_dec_row_gemv")


def _cp():
    from model.control_predict import ControlPredict
    from tool.config import default_cfg
    torch.manual_seed(0)
    return ControlPredict(default_cfg()).eval()


def test_switch_defaults_on_and_is_a_flippable_list():
    from e2ep_amd import ar_decode
    assert isinstance(ar_decode._DECODE_CACHE, list) and len(ar_decode._DECODE_CACHE) == 1
    if "E2EP_DECODE_CACHE" not in os.environ:
        assert ar_decode._DECODE_CACHE[0] is True


def test_not_eligible_for_cpu_tensors():
    from e2ep_amd import ar_decode
    cp = _cp()
    mem = torch.randn(2, 5, 258)
    toks = torch.full((2, 1), 201, dtype=torch.long)
    with torch.no_grad():
        assert ar_decode.eligible(cp, mem, toks) is False


def test_predict_tokens_on_cpu_is_the_predict_loop():
    """On CPU tensors predict_tokens is the reference-style loop over predict(), as before: the
    same tokens where predict computes some, and where predict refuses CPU tensors (the e2ep
    ops run on a HIP device only) the same error, with no e2ep_dec_* entry point reached."""
    from e2ep_amd import _lib, ar_decode
    cp = _cp()
    mem = torch.randn(2, 5, 258, generator=torch.Generator().manual_seed(1))
    toks = torch.full((2, 1), 201, dtype=torch.long)

    def loop():
        t = toks
        for _ in range(2):
            t = torch.cat([t, cp.predict(mem, t)], dim=1)
        return t
    n0 = ar_decode.LAUNCHES[0]
    with torch.no_grad():
        try:
            want, err = loop(), None
        except _lib.E2EPError as e:
            want, err = None, str(e)
        if err is None:
            assert torch.equal(cp.predict_tokens(mem, toks, 2), want)
        else:
            with pytest.raises(_lib.E2EPError) as got:
                cp.predict_tokens(mem, toks, 2)
            assert str(got.value) == err
    assert ar_decode.LAUNCHES[0] == n0


def test_new_symbols_bound_with_the_declared_arity():
    """Declared and exported; the binding's arity is the header's by construction
    (test_abi_cpu.py)."""
    from e2ep_amd import _lib
    for name in NEW:
        assert name in _lib.SIGNATURES, f"{name} not declared in include/e2ep.h"
        assert _lib.SIGNATURES[name][0] is ctypes.c_int
    if os.path.exists(_lib.LIB_PATH):
        lib = _lib.load()
        for name in NEW:
            assert hasattr(lib, name)
