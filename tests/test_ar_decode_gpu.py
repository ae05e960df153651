"""KV-cached incremental decoding of the control-token decoder (csrc/ar_decode.hip,
e2ep_amd/ar_decode.py, ControlPredict.predict_tokens).

Reference = torch's own nn.TransformerDecoder in fp64 on the CPU (the module deep-copied and
made double): the full pass over the PAD-padded sequence with the causal and the key-padding
mask, of which row t is what an incremental step at position t must give.  Bound on the logits:
rel-L2 < 1e-5, the bound tests/test_attention_gpu.py holds the fused attention to against fp64."""
import copy
import functools

import pytest
import torch
from torch import nn

from helpers import rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-5
BOS = 201


# ------------------------------------------------------------------------------------------
# modules and the fp64 reference
# ------------------------------------------------------------------------------------------
def _small_cfg(E, H):
    from tool.config import default_cfg
    return default_cfg(tf_de_dim=E, tf_de_heads=H, tf_de_tgt_dim=7, token_nums=11)


@functools.lru_cache(maxsize=None)
def _module(name):
    """(fp32 module on the GPU, its fp64 CPU copy).  default: E 258, H 6, F 2048, T 14, V 204;
    small: E 26, H 2 (dh 13), F 40, T 6, V 11; odd: E 27, H 3 (dh 9), F 41 (dword loads)."""
    from model.control_predict import ControlPredict
    from tool.config import default_cfg
    torch.manual_seed({"default": 11, "small": 12, "odd": 13}[name])
    if name == "default":
        cp = ControlPredict(default_cfg())
    else:
        E, H, Fd = (26, 2, 40) if name == "small" else (27, 3, 41)
        cp = ControlPredict(_small_cfg(E, H))
        for layer in cp.tf_decoder.layers:
            layer.linear1, layer.linear2 = nn.Linear(E, Fd), nn.Linear(Fd, E)
    with torch.no_grad():  # the biases and LayerNorm parameters away from their 0 / 1 init
        for n, p in cp.named_parameters():
            if p.dim() == 1:
                p.add_(torch.randn_like(p) * 0.1)
    cp.eval()
    cp64 = copy.deepcopy(cp).double()
    return cp.to(DEV), cp64


def _padded(cp, toks):
    T = cp.cfg.tf_de_tgt_dim - 1
    pad = torch.full((toks.shape[0], T - toks.shape[1]), cp.pad_idx, dtype=torch.long,
                     device=toks.device)
    return torch.cat([toks, pad], 1)


def _full64(cp64, memory, seq):
    """fp64 logits (B, T, V) of the full pass over seq (B, T), torch's own decoder."""
    T = seq.shape[1]
    with torch.no_grad():
        x = cp64.embedding(seq) + cp64.pos_embed
        mask = torch.full((T, T), float("-inf"), dtype=torch.float64).triu(1)
        y = cp64.tf_decoder(x.transpose(0, 1), memory.double().transpose(0, 1), tgt_mask=mask,
                            tgt_key_padding_mask=seq == cp64.pad_idx)
        return cp64.output(y.transpose(0, 1))


def _full_gpu(cp, memory, seq):
    """The existing full-pass GPU path's logits (B, T, V)."""
    from e2ep_amd import nn_ops
    with torch.no_grad():
        mask, padm = cp.create_mask(seq)
        emb = nn_ops.embed_tokens(seq, cp.embedding.weight, cp.pos_embed)
        return cp.project(cp.decoder(memory, emb, mask, padm))


def _loop64(cp64, memory, toks, steps):
    """The reference's predict loop in fp64: (tokens, smallest top-2 logit gap over the steps)."""
    gap = float("inf")
    for _ in range(steps):
        row = _full64(cp64, memory, _padded(cp64, toks))[:, toks.shape[1] - 1]
        top = row.topk(2, dim=-1).values
        gap = min(gap, float((top[:, 0] - top[:, 1]).min()))
        toks = torch.cat([toks, row.softmax(-1).argmax(-1, keepdim=True)], 1)
    return toks, gap


def _switch(on):
    from e2ep_amd import ar_decode
    old = ar_decode._DECODE_CACHE[0]
    ar_decode._DECODE_CACHE[0] = on
    return old


def _tokens(cp, memory, toks, steps, on, grad=False):
    """(predict_tokens' result, e2ep_dec_* launches it made) with the switch set to `on`."""
    from e2ep_amd import ar_decode
    old = _switch(on)
    try:
        n0 = ar_decode.LAUNCHES[0]
        with torch.set_grad_enabled(grad):
            out = cp.predict_tokens(memory, toks, steps).clone()
        return out, ar_decode.LAUNCHES[0] - n0
    finally:
        _switch(old)


# ------------------------------------------------------------------------------------------
# 1. logits against the fp64 full pass
# ------------------------------------------------------------------------------------------
def _check_steps(name, Sk, B, L):
    from e2ep_amd import ar_decode
    cp, cp64 = _module(name)
    E, V = cp.cfg.tf_de_dim, cp.cfg.token_nums
    g = torch.Generator().manual_seed(1000 * Sk + 10 * B + L)
    memory = torch.randn(B, Sk, E, generator=g)
    toks = torch.randint(0, V - 1, (B, L), generator=g)  # no PAD
    toks[:, 0] = min(BOS, V - 2)
    seq = _padded(cp64, toks)
    ref = _full64(cp64, memory, seq)
    # (the full-pass GPU path is measured beside it for the two configurations it is built for)
    old = _full_gpu(cp, memory.to(DEV), seq.to(DEV)) if name != "odd" else None
    with torch.no_grad():
        dec = ar_decode.IncrementalDecoder(cp).start(memory.to(DEV))
        seqd = seq.to(DEV)
        for t in range(L):
            got = dec.step(seqd, t)
            assert tuple(got.shape) == (B, V)
            e_new = rel_l2(got, ref[:, t])
            e_old = rel_l2(old[:, t], ref[:, t]) if old is not None else float("nan")
            print(f"{name} Sk={Sk} B={B} L={L} t={t}: rel-L2 vs fp64 incremental {e_new:.3e}, "
                  f"full pass {e_old:.3e}")
            assert e_new < TOL, (name, Sk, B, L, t, e_new)


@pytest.mark.parametrize("L", [1, 3])
@pytest.mark.parametrize("B", [1, 3, 16])
@pytest.mark.parametrize("Sk", [256, 5])
@pytest.mark.parametrize("name", ["default", "small"])
def test_step_logits_match_fp64_full_pass(name, Sk, B, L):
    _check_steps(name, Sk, B, L)


@pytest.mark.parametrize("Sk,B,L", [(5, 3, 3), (131, 5, 2)])
def test_step_logits_odd_width(Sk, B, L):
    """E = 27: no row is 8-byte aligned, so every kernel takes its dword-load path; Sk = 131
    crosses the 128-key tile of the cross attention, B = 5 the 4-row chunk of the row GEMV."""
    _check_steps("odd", Sk, B, L)


# ------------------------------------------------------------------------------------------
# 2. a PAD key inside the sequence
# ------------------------------------------------------------------------------------------
def test_pad_key_inside_the_sequence():
    from e2ep_amd import ar_decode
    cp, cp64 = _module("default")
    cp = copy.deepcopy(cp)  # its PAD embedding row is perturbed below
    pad = cp.pad_idx
    g = torch.Generator().manual_seed(2)
    memory = torch.randn(2, 256, 258, generator=g)
    toks = torch.tensor([[BOS, pad, 57, 33], [BOS, 12, 57, 33]])
    seq = _padded(cp64, toks)
    ref = _full64(cp64, memory, seq)  # masks key 1 of sample 0

    def run():
        with torch.no_grad():
            dec = ar_decode.IncrementalDecoder(cp).start(memory.to(DEV))
            return [dec.step(seq.to(DEV), t).clone() for t in range(4)]
    got = run()
    for t in (2, 3):
        err = rel_l2(got[t], ref[:, t])
        print(f"PAD at key 1, t={t}: rel-L2 vs fp64 {err:.3e}")
        assert err < TOL
    with torch.no_grad():
        cp.embedding.weight[pad] += 1.0
    again = run()
    for t in (2, 3):  # the masked key's content reaches nothing
        assert torch.equal(again[t], got[t])
    assert not torch.equal(again[1][0], got[1][0])  # (the PAD position's own row does move)


# ------------------------------------------------------------------------------------------
# 3. tokens equal to the existing path and to fp64
# ------------------------------------------------------------------------------------------
def _token_case(seed, B, L):
    from model.control_predict import ControlPredict
    from tool.config import default_cfg
    torch.manual_seed(seed)
    cp = ControlPredict(default_cfg()).eval()
    g = torch.Generator().manual_seed(100 * seed + B)
    memory = torch.randn(B, 256, 258, generator=g)
    toks = torch.full((B, L), BOS, dtype=torch.long)
    if L > 1:  # prefix tokens after BOS: from the same generator, after the memory
        toks[:, 1:] = torch.randint(0, 200, (B, L - 1), generator=g)
    return cp, memory, toks


@pytest.mark.parametrize("B,L", [(1, 1), (3, 2), (8, 1)])
@pytest.mark.parametrize("seed", [0, 3])
def test_tokens_equal_full_pass_and_fp64(seed, B, L):
    cp, memory, toks = _token_case(seed, B, L)
    want, gap = _loop64(copy.deepcopy(cp).double(), memory, toks, 4)
    print(f"seed {seed} B={B} L={L}: smallest fp64 top-2 logit gap {gap:.3e}")
    assert gap >= 1e-3, "not a valid case (checked on the CPU when the cases were chosen)"
    cp = cp.to(DEV)
    on, n_on = _tokens(cp, memory.to(DEV), toks.to(DEV), 4, True)
    off, n_off = _tokens(cp, memory.to(DEV), toks.to(DEV), 4, False)
    assert n_off == 0 and n_on == (L - 1 + 4) * 24 + 4  # 6 launches x 4 layers, 4 projections
    assert tuple(on.shape) == (B, L + 4)
    assert torch.equal(on, off)
    assert torch.equal(on.cpu(), want)


# ------------------------------------------------------------------------------------------
# 4. capture and determinism
# ------------------------------------------------------------------------------------------
def test_captured_predict_tokens_and_bitwise_repeat():
    from e2ep_amd import ar_decode, graphs
    cp, _ = _module("default")
    g = torch.Generator().manual_seed(4)
    mems = [torch.randn(1, 256, 258, generator=g).to(DEV) for _ in range(2)]
    toks = torch.full((1, 1), BOS, dtype=torch.long, device=DEV)
    eager = [_tokens(cp, m, toks, 3, True)[0] for m in mems]
    static = mems[0].clone()

    def call():
        with torch.no_grad():
            return cp.predict_tokens(static, toks, 3)
    old = _switch(True)
    try:
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            call()
        torch.cuda.current_stream().wait_stream(s)
        n0 = ar_decode.LAUNCHES[0]
        graph, out, _ = graphs.capture(call)
        assert ar_decode.LAUNCHES[0] - n0 == 3 * 25  # the captured work is the new path's
    finally:
        _switch(old)
    graph.replay()
    torch.cuda.synchronize()
    first = out.clone()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(first, eager[0]) and torch.equal(out, first)
    static.copy_(mems[1])
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager[1])
    # two eager runs: bit-equal logits
    seq = _padded(cp, torch.tensor([[BOS, 5, 77]], device=DEV))
    runs = []
    for _ in range(2):
        with torch.no_grad():
            dec = ar_decode.IncrementalDecoder(cp).start(mems[0])
            runs.append([dec.step(seq, t).clone() for t in range(3)])
    for a, b in zip(*runs):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------
# 5. the gate
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("why", ["none", "hook", "B17", "bf16", "train", "grad"])
def test_gate_takes_the_existing_path(why):
    from e2ep_amd import precision
    from model.control_predict import ControlPredict
    from tool.config import default_cfg
    torch.manual_seed(5)
    cp = ControlPredict(default_cfg(deterministic=True)).to(DEV).eval()  # no dropout: .train()
    B = 17 if why == "B17" else 2
    memory = torch.randn(B, 256, 258, generator=torch.Generator().manual_seed(5)).to(DEV)
    toks = torch.full((B, 1), BOS, dtype=torch.long, device=DEV)
    seen = []
    hook = None
    if why == "hook":
        hook = cp.tf_decoder.layers[1].multihead_attn.register_forward_hook(
            lambda mod, args, out: seen.append(1))
    if why == "train":
        cp.train()
    try:
        with precision.use("bf16" if why == "bf16" else "fp32"):
            # "grad": autograd would record the call
            on, n_on = _tokens(cp, memory, toks, 3, True, grad=why == "grad")
            n_seen = len(seen)
            off, n_off = _tokens(cp, memory, toks, 3, False)
    finally:
        if hook is not None:
            hook.remove()
    assert n_off == 0
    assert torch.equal(on, off)
    if why == "none":
        assert n_on == 3 * 25
    else:
        assert n_on == 0, why
    if why == "hook":
        assert n_seen == 3  # once per generated token: the caller's hook still fires


# ------------------------------------------------------------------------------------------
# 6. range errors
# ------------------------------------------------------------------------------------------
def test_entry_points_reject_shapes_outside_their_range():
    from e2ep_amd import _lib
    buf = torch.zeros(1 << 16, device=DEV)
    seq = torch.zeros(17, 40, dtype=torch.long, device=DEV)
    p, q, s = _lib.ptr(buf), _lib.ptr(seq), _lib.stream()
    ERANGE = -2

    def self_attn(B, T, E, H):
        return _lib.call_raw("e2ep_dec_self_attn", p, E, p, p, 1e-5, p, 4, p, p, q, 40, 3, p, p, p,
                             p, B, T, 0, E, H, s)

    def cross_attn(B, Sk, E, H):
        return _lib.call_raw("e2ep_dec_cross_attn", p, E, p, p, 1e-5, p, p, p, 2 * E, p, B, Sk, E,
                             H, s)

    def gemv(B, N, K):
        return _lib.call_raw("e2ep_dec_row_gemv", p, K, p, p, 1e-5, p, p, p, N, p, p, 1e-5, p, N, B,
                             N, K, 0, s)
    assert self_attn(2, 33, 16, 2) == ERANGE      # T = 33
    assert self_attn(2, 8, 65, 1) == ERANGE       # dh = 65
    assert self_attn(17, 8, 16, 2) == ERANGE      # B = 17
    assert cross_attn(2, 257, 16, 2) == ERANGE    # Sk = 257
    assert cross_attn(2, 8, 130, 2) == ERANGE     # dh = 65
    assert cross_attn(17, 8, 16, 2) == ERANGE
    assert gemv(17, 8, 8) == ERANGE
    assert gemv(2, 8, 4089) == ERANGE             # the staged rows would not fit the LDS
    assert b"limits" in _lib.load().e2ep_last_error()
    torch.cuda.synchronize()
    assert float(buf.abs().sum()) == 0.0  # nothing ran
