"""csrc/gemm.hip on operands that are offset and strided inside larger buffers (tests/placement.py):
every leading dimension above its minimum, every base pointer off its alignment, NaN in every
element an operand does not own and a sentinel in every element an output does not own.

Per case: the payload against an fp64 CPU product (rel-L2 < 2e-6, the bound of test_gemm_gpu.py
for fp32 and for bf16-rounded operands), bitwise equality with the same call on dense, aligned
copies under the same tile / split / fold setting (the vector width changes how values are
loaded, not the order in which they are summed; not asserted between k_gemm_skinny<2> and <1>,
whose k-to-lane mappings differ), no NaN in a payload, every output gap untouched
(placement.check_gaps) and, under guard.allocations with both fills, clean bands.

Row length 77 (K for the forward layout), G_BK = 32: three K-steps, the last with a 13-wide
tail; three forced splits give every split one step.  Placement (ld, off) -> vec_of class:

    v0d (77, 0) dense: vec 0      v2  (80, 0) vec 2            v1p (80, 2) vec 1 by pointer
    v1l (78, 0) vec 1 by ld       v0p (80, 1) vec 0 by pointer  v0l (79, 0) vec 0 by ld

Where each instantiation is reached (test ids):

    k_gemm<true,true,tile 1|2,AVEC,BVEC>      test_forward_layout_every_vec_pair[t{1,2}-A_<a>-B_<b>]
        (AVEC, BVEC) = (2,2) A_v2-B_v2; (2,1) A_v2-B_v1p, A_v2-B_v1l; (2,0) A_v2-B_v0d|v0p|v0l;
        (1,2) A_v1p|v1l-B_v2; (1,1) A_v1p|v1l-B_v1p|v1l; (1,0) A_v1p|v1l-B_v0d|v0p|v0l;
        (0,2) A_v0d|v0p|v0l-B_v2; (0,1) A_v0*-B_v1p|v1l; (0,0) A_v0*-B_v0*
        each: unsplit, 3 splits folded in the launch, 3 splits + k_gemm_reduce<1> (ldc = N + 3,
        or C off alignment) — both epilogues, ldc in {N, N + 3}
    k_gemm<..., OP = 1> (bf16)                test_forward_layout_bf16[t{1,2}-A_<a>-B_<b>]
    k_gemm<true,false|false,true|false,false> test_other_layouts[t{1,2}-<layout>-<placement>]
    tiles 3 .. 6                              test_large_tiles_mixed_placement[t{3..6}]
    full-step control, K = 96                 test_full_step_control[A_<class>-B_<class>]
    k_gemm_skinny<2>                          test_skinny[*-v2]  (and [K78-*-dense])
    k_gemm_skinny<1>                          test_skinny[*-lda|ldb|aptr|bptr]  (and [K77-*-dense])
    M = 17 leaves the skinny kernel           test_skinny[*-M17-*]
    rs column: k_gemm<false,false>; the fold;  test_rowsum[t0-nosplit], [t{1,2}-{nosplit,fold,reduce}]
        k_gemm_reduce<1> writing rowsum       test_rowsum[t{1,2}-reduce]
    k_gemm_pair<..., AV1>, unsplit            test_linear_bwd[*-plan-*]
    k_gemm_pair with both problems split      test_linear_bwd[*-split-*]
    k_gemm_reduce<4> (dense aligned C)        the dense controls of every `reduce` setting
    every other k_gemm / k_gemm_pair built    test_remaining_instantiations, test_linear_bwd_
                                              remaining_instantiations (33 x 70 x 77, unsplit)"""
import contextlib

import pytest
import torch

import guard
import placement as P
from helpers import rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 2e-6
M, N = 70, 130
KPLACE = {"v0d": (77, 0), "v2": (80, 0), "v1p": (80, 2), "v1l": (78, 0), "v0p": (80, 1),
          "v0l": (79, 0)}
VEC = {"v0d": 0, "v2": 2, "v1p": 1, "v1l": 1, "v0p": 0, "v0l": 0}
SPLITS = {"nosplit": (1, None), "fold": (3, 2), "reduce": (3, 1)}  # (forced splits, tune key 28)
FILLS = (guard.FILL_A, guard.FILL_B)


def _lib():
    from e2ep_amd import _lib
    return _lib


@contextlib.contextmanager
def _settings(tile=0, splits=0, fold=None, bf16=False, split_min=None):
    """e2ep_gemm_force / e2ep_tune key 28 / e2ep_gemm_precision / e2ep_gemm_split_min for the
    block, every one of them put back in the finally."""
    L = _lib()
    lib = L.load()
    prev_fold = prev_prec = prev_min = None
    try:
        L.call("e2ep_gemm_force", tile, splits, 0)
        if fold is not None:
            prev_fold = lib.e2ep_tune(28, fold)
        if bf16:
            prev_prec = lib.e2ep_gemm_precision(1)
        if split_min is not None:
            prev_min = lib.e2ep_gemm_split_min(split_min)
        yield
    finally:
        L.call("e2ep_gemm_force", 0, 0, 0)
        if prev_fold is not None:
            lib.e2ep_tune(28, prev_fold)
        if prev_prec is not None:
            lib.e2ep_gemm_precision(prev_prec)
        if prev_min is not None:
            lib.e2ep_gemm_split_min(prev_min)


def _vec_class(t):
    """vec_of (gemm.hip) of a k-contiguous operand."""
    if t.stride(0) % 4 == 0 and t.data_ptr() % 16 == 0:
        return 2
    return 1 if t.stride(0) % 2 == 0 and t.data_ptr() % 8 == 0 else 0


def _gemm(A, ak, B, bk, C, m, n, k, bias=None, cadd=None, relu=False):
    """e2ep_gemm through the C ABI with the operands' own strides; workspace sized for the
    current settings (poisoned under a guard context)."""
    L = _lib()
    ws = torch.empty(max(16, L.load().e2ep_gemm_workspace(m, n, k)), dtype=torch.uint8, device=DEV)
    L.call("e2ep_gemm", L.ptr(A), A.stride(0), int(ak), L.ptr(B), B.stride(0), int(bk), L.ptr(bias),
           L.ptr(cadd), cadd.stride(0) if cadd is not None else 0, L.ptr(C), C.stride(0), m, n, k,
           int(relu), L.ptr(ws), L.nbytes(ws), L.stream())
    return C


def _check(got, want64, dense, what, bitwise=True):
    """The per-output assertions: no NaN, fp64 bound, bitwise equal to the dense control, gaps."""
    assert not bool(got.isnan().any()), f"{what}: NaN in the payload"
    err = rel_l2(got, want64)
    assert err < TOL, f"{what}: rel-L2 {err:.3e} vs fp64"
    if bitwise:
        assert torch.equal(got, dense), f"{what}: differs bitwise from the dense, aligned call"
    P.check_gaps(got, what)


class _Problem:
    """Host operands of one (m, n, k, ak, bk) product with both epilogues' inputs and fp64
    references, computed once per module."""
    _cache = {}

    def __new__(cls, m, n, k, ak, bk, bf16=False):
        key = (m, n, k, ak, bk, bf16)
        if key not in cls._cache:
            self = super().__new__(cls)
            g = torch.Generator().manual_seed(1000 * m + 10 * n + k + 3 * ak + 5 * bk)
            self.A = torch.randn((m, k) if ak else (k, m), generator=g)
            self.B = torch.randn((n, k) if bk else (k, n), generator=g)
            self.bias = torch.randn(n, generator=g)
            self.cadd = torch.randn(m, n, generator=g)
            A64, B64 = ((t.bfloat16() if bf16 else t).double() for t in (self.A, self.B))
            self.plain = (A64 if ak else A64.t()) @ (B64.t() if bk else B64)
            self.full = (self.plain + self.bias.double() + self.cadd.double()).clamp_min(0)
            self.dims, self.layout = (m, n, k), (ak, bk)
            self.dense = {}
            cls._cache[key] = self
        return cls._cache[key]

    def control(self, setting, epi):
        """The same call on dense, aligned operands under the current settings, once per
        (setting, epilogue)."""
        if (setting, epi) not in self.dense:
            m, n, k = self.dims
            ak, bk = self.layout
            C = torch.full((m, n), float("nan"), device=DEV)
            extra = dict(bias=self.bias.to(DEV), cadd=self.cadd.to(DEV), relu=True) if epi else {}
            _gemm(self.A.to(DEV), ak, self.B.to(DEV), bk, C, m, n, k, **extra)
            self.dense[(setting, epi)] = C
        return self.dense[(setting, epi)]

    def run(self, setting, pa, pb, epi, ldc, what):
        """One placed call: A at pa, B at pb (ld, off), C at (ldc, 1); epi: bias 8 bytes off,
        Cadd at ldadd = n + 2, ReLU."""
        m, n, k = self.dims
        ak, bk = self.layout
        A = P.placed(self.A, *pa, device=DEV)
        B = P.placed(self.B, *pb, device=DEV)
        C = P.out((m, n), ldc, 1, device=DEV)
        extra = {}
        if epi:
            extra = dict(bias=P.placed(self.bias, None, 2, device=DEV),
                         cadd=P.placed(self.cadd, n + 2, 3, device=DEV), relu=True)
            assert extra["bias"].data_ptr() % 16 == 8 and extra["cadd"].stride(0) == n + 2
        assert C.data_ptr() % 16 == 4 and C.stride(0) == ldc
        _gemm(A, ak, B, bk, C, m, n, k, **extra)
        _check(C, self.full if epi else self.plain, self.control(setting, epi), what)
        return A, B


def _forward_matrix(prob, tile, pa, pb, splits=SPLITS, epis=(False, True), ldcs=None, bf16=False):
    m, n, k = prob.dims
    for sname, (nsplit, fold) in splits.items():
        with _settings(tile, nsplit, fold, bf16):
            setting = (tile, sname, bf16)
            for epi in epis:
                prob.control(setting, epi)  # outside the guard contexts: kept for later cases
            for fill in FILLS:
                with guard.allocations(fill) as g:
                    for epi in epis:
                        for ldc in ldcs or (n, n + 3):
                            A, B = prob.run(setting, pa, pb, epi, ldc,
                                            f"tile {tile} {sname} epi {epi} ldc {ldc} fill {fill:#x}")
                g.check()
    return A, B


PAIRS = [(a, b) for a in KPLACE for b in KPLACE]


@pytest.mark.parametrize("a,b", PAIRS, ids=[f"A_{a}-B_{b}" for a, b in PAIRS])
@pytest.mark.parametrize("tile", [1, 2], ids=["t1", "t2"])
def test_forward_layout_every_vec_pair(tile, a, b):
    prob = _Problem(M, N, 77, True, True)
    A, B = _forward_matrix(prob, tile, KPLACE[a], KPLACE[b])
    assert (_vec_class(A), _vec_class(B)) == (VEC[a], VEC[b])  # the instantiation the id names


# one placement per class pair, alternating the by-pointer and by-ld flavours
BF16_PAIRS = [("v2", "v2"), ("v2", "v1p"), ("v2", "v0l"), ("v1l", "v2"), ("v1p", "v1l"),
              ("v1l", "v0p"), ("v0p", "v2"), ("v0l", "v1p"), ("v0d", "v0l")]


@pytest.mark.parametrize("a,b", BF16_PAIRS, ids=[f"A_{a}-B_{b}" for a, b in BF16_PAIRS])
@pytest.mark.parametrize("tile", [1, 2], ids=["t1", "t2"])
def test_forward_layout_bf16(tile, a, b):
    """e2ep_gemm_precision(1): against fp64 of the bf16-rounded operands."""
    prob = _Problem(M, N, 77, True, True, bf16=True)
    A, B = _forward_matrix(prob, tile, KPLACE[a], KPLACE[b], bf16=True)
    assert (_vec_class(A), _vec_class(B)) == (VEC[a], VEC[b])
    assert rel_l2(prob.control((tile, "nosplit", True), False),
                  _Problem(M, N, 77, True, True).plain) > 1e-4  # the rounding really happens


CLASS96 = {"v2": (100, 0), "v1": (100, 2), "v0": (100, 1)}
PAIRS96 = [(a, b) for a in CLASS96 for b in CLASS96]


@pytest.mark.parametrize("a,b", PAIRS96, ids=[f"A_{a}-B_{b}" for a, b in PAIRS96])
def test_full_step_control(a, b):
    """K = 96: three full K-steps, no tail mask."""
    prob = _Problem(M, N, 96, True, True)
    for tile in (1, 2):
        _forward_matrix(prob, tile, CLASS96[a], CLASS96[b], ldcs=(N + 3,))


ROWC = 5, 3  # the one placement of a row-contiguous operand: (min + 5, 3)
OTHER = ([("TF", p) for p in ("v2", "v1p", "v0l")] + [("FT", p) for p in ("v2", "v1l", "v0p")]
         + [("FF", "rows")])


@pytest.mark.parametrize("layout,p", OTHER, ids=[f"{lay}-{p}" for lay, p in OTHER])
@pytest.mark.parametrize("tile", [1, 2], ids=["t1", "t2"])
def test_other_layouts(tile, layout, p):
    """(ak, bk) = (T, F), (F, T), (F, F): the k-contiguous operand at each vec class, the
    row-contiguous one at (min + 5, 3)."""
    ak, bk = layout[0] == "T", layout[1] == "T"
    prob = _Problem(M, N, 77, ak, bk)
    pa = KPLACE[p] if ak else (M + ROWC[0], ROWC[1])
    pb = KPLACE[p] if bk else (N + ROWC[0], ROWC[1])
    _forward_matrix(prob, tile, pa, pb)


@pytest.mark.parametrize("tile", [3, 4, 5, 6], ids=["t3", "t4", "t5", "t6"])
def test_large_tiles_mixed_placement(tile):
    prob = _Problem(M, N, 77, True, True)
    A, B = _forward_matrix(prob, tile, KPLACE["v1p"], KPLACE["v0l"])
    assert (_vec_class(A), _vec_class(B)) == (1, 0)


def _terminals():
    """(ak, bk, AVEC, BVEC, tile, bf16) of the k_gemm instantiations the tests above and
    test_gemm_gpu.py leave out (read off a kernel trace of both files): the large tiles at every
    vector-width pair but (0, 0) and (1, 0) for the forward layout, and at a vector width at all
    for the other two layouts; bf16 operands for the layouts with one k-contiguous operand."""
    big = (3, 4, 5, 6)
    out = [(True, True, a, b, t, False) for a in (0, 1, 2) for b in (0, 1, 2) for t in big
           if (a, b) not in ((0, 0), (1, 0))]
    out += [(True, False, 1, 0, t, False) for t in (3, 5, 6)]
    out += [(True, False, 2, 0, t, False) for t in big]
    out += [(True, False, 0, 0, 1, True), (True, False, 1, 0, 2, True)]
    out += [(False, True, 0, b, t, False) for b in (1, 2) for t in big]
    out += [(False, True, 0, b, t, True) for b in (0, 1, 2) for t in (1, 2)]
    return out


SMALL = 33, 70  # two 32-row tiles; a ragged last tile at every block width
VEC_PLACE = {2: "v2", 1: "v1p", 0: "v0p"}


@pytest.mark.parametrize("ak,bk,avec,bvec,tile,bf16", _terminals(),
                         ids=[f"{'FT'[a]}{'FT'[b]}-a{av}-b{bv}-t{t}-{'bf16' if h else 'fp32'}"
                              for a, b, av, bv, t, h in _terminals()])
def test_remaining_instantiations(ak, bk, avec, bvec, tile, bf16):
    """One small unsplit product per k_gemm<AK, BKC, tile, AVEC, BVEC, OP> no other test launches."""
    m, n = SMALL
    prob = _Problem(m, n, 77, ak, bk, bf16=bf16)
    pa = KPLACE[VEC_PLACE[avec]] if ak else (m + ROWC[0], ROWC[1])
    pb = KPLACE[VEC_PLACE[bvec]] if bk else (n + ROWC[0], ROWC[1])
    with _settings(tile, 1, None, bf16):
        setting = (tile, "nosplit", bf16)
        A, B = prob.run(setting, pa, pb, False, n + 3, f"tile {tile} bf16 {bf16}")
    assert (_vec_class(A) if ak else 0, _vec_class(B) if bk else 0) == (avec, bvec)


# ------------------------------------------------------------------------------------------
# k_gemm_skinny
# ------------------------------------------------------------------------------------------
SK_N = 33
# name -> (A (ld - K, off), B (ld - K, off)) for odd and for even K
SK_PLACE = {
    "dense": {77: ((0, 0), (0, 0)), 78: ((0, 0), (0, 0))},
    "v2": {77: ((1, 0), (3, 2)), 78: ((2, 2), (4, 0))},
    "lda": {77: ((2, 0), (1, 0)), 78: ((3, 0), (2, 0))},
    "ldb": {77: ((1, 0), (2, 0)), 78: ((2, 0), (3, 0))},
    "aptr": {77: ((1, 1), (1, 0)), 78: ((2, 3), (2, 0))},
    "bptr": {77: ((1, 0), (1, 1)), 78: ((2, 0), (2, 3))},
}


def _sk_v2(A, B):
    return (A.stride(0) % 2 == 0 and B.stride(0) % 2 == 0 and A.data_ptr() % 8 == 0
            and B.data_ptr() % 8 == 0)


@pytest.mark.parametrize("name", list(SK_PLACE))
@pytest.mark.parametrize("m", [1, 14, 16, 17], ids=lambda m: f"M{m}")
@pytest.mark.parametrize("k", [77, 78], ids=lambda k: f"K{k}")
def test_skinny(k, m, name):
    """M <= 16 rows take k_gemm_skinny<2> (lda, ldb even, A and B 8-byte aligned) or <1>; the
    two sum in different orders, so the dense control binds bitwise only where it runs the same
    variant.  M = 17 is on the MFMA tiles (equal to a forced tile 2, which never goes skinny)."""
    L = _lib()
    assert L.load().e2ep_gemm_skinny(-1) == 16
    prob = _Problem(m, SK_N, k, True, True)
    (dla, oa), (dlb, ob) = SK_PLACE[name][k]
    want_v2 = name == "v2" or (name == "dense" and k == 78)
    for epi in (False, True):
        extra_d = dict(bias=prob.bias.to(DEV), cadd=prob.cadd.to(DEV), relu=True) if epi else {}
        Ad, Bd = prob.A.to(DEV), prob.B.to(DEV)
        dense = _gemm(Ad, True, Bd, True, torch.full((m, SK_N), float("nan"), device=DEV), m, SK_N,
                      k, **extra_d)
        with _settings(2, 1):
            mfma = _gemm(Ad, True, Bd, True, torch.full((m, SK_N), float("nan"), device=DEV), m,
                         SK_N, k, **extra_d)
        assert rel_l2(mfma, prob.full if epi else prob.plain) < TOL
        assert torch.equal(dense, mfma) == (m == 17), "M <= 16 is skinny, M = 17 is not"
        for fill in FILLS:
            with guard.allocations(fill) as g:
                A = P.placed(prob.A, k + dla, oa, device=DEV)
                B = P.placed(prob.B, k + dlb, ob, device=DEV)
                assert _sk_v2(A, B) == want_v2
                C = P.out((m, SK_N), SK_N + 3, 1, device=DEV)
                extra = {}
                if epi:
                    extra = dict(bias=P.placed(prob.bias, None, 1, device=DEV),
                                 cadd=P.placed(prob.cadd, SK_N + 1, 3, device=DEV), relu=True)
                _gemm(A, True, B, True, C, m, SK_N, k, **extra)
                _check(C, prob.full if epi else prob.plain, dense, f"skinny {name} epi {epi}",
                       bitwise=m == 17 or want_v2 == _sk_v2(Ad, Bd))
            g.check()


# ------------------------------------------------------------------------------------------
# e2ep_gemm_rowsum
# ------------------------------------------------------------------------------------------
def _rowsum(A, B, C, rs, m, n, k):
    L = _lib()
    ws = torch.empty(max(16, L.load().e2ep_gemm_rowsum_workspace(m, n, k)), dtype=torch.uint8,
                     device=DEV)
    L.call("e2ep_gemm_rowsum", L.ptr(A), A.stride(0), L.ptr(B), B.stride(0), L.ptr(C), C.stride(0),
           L.ptr(rs), m, n, k, L.ptr(ws), L.nbytes(ws), L.stream())


RS_CASES = [(0, "nosplit")] + [(t, s) for t in (1, 2) for s in SPLITS]


@pytest.mark.parametrize("tile,sname", RS_CASES, ids=[f"t{t}-{s}" for t, s in RS_CASES])
def test_rowsum(tile, sname):
    """C = A^T B with rowsum[m] = sum_k A(k, m): lda, ldb, ldc above their minimum, rowsum at an
    odd offset.  Tile 0 is the automatic plan (which does not split this shape)."""
    nsplit, fold = SPLITS[sname]
    if tile == 0:
        nsplit = 0
    k = 77
    prob = _Problem(M, N, k, False, False)
    want_rs = prob.A.double().sum(0)
    with _settings(tile, nsplit, fold):
        Cd = torch.full((M, N), float("nan"), device=DEV)
        rsd = torch.full((M,), float("nan"), device=DEV)
        _rowsum(prob.A.to(DEV), prob.B.to(DEV), Cd, rsd, M, N, k)
        for fill in FILLS:
            with guard.allocations(fill) as g:
                A = P.placed(prob.A, M + 5, 3, device=DEV)
                B = P.placed(prob.B, N + 7, 1, device=DEV)
                C = P.out((M, N), N + 3, 1, device=DEV)
                rs = P.out((M,), None, 3, device=DEV)
                _rowsum(A, B, C, rs, M, N, k)
                _check(C, prob.plain, Cd, f"rowsum C tile {tile} {sname}")
                _check(rs, want_rs, rsd, f"rowsum tile {tile} {sname}")
            g.check()


# ------------------------------------------------------------------------------------------
# e2ep_linear_bwd (k_gemm_pair)
# ------------------------------------------------------------------------------------------
LB = 70, 77, 50  # rows M, out features N (dy's row length), in features K
DY_PLACE = ["v2", "v1p", "v1l", "v0p", "v0l"]  # (v0d is the minimal ldy)


def _linear_bwd(dy, x, w, gs, dx, dw, db, dims=LB):
    L = _lib()
    lib = L.load()
    m, n, k = dims
    wsx = torch.empty(max(16, lib.e2ep_gemm_workspace(m, k, n)), dtype=torch.uint8, device=DEV)
    wsw = torch.empty(max(16, lib.e2ep_gemm_rowsum_workspace(n, k, m)), dtype=torch.uint8, device=DEV)
    L.call("e2ep_linear_bwd", L.ptr(dy), dy.stride(0), L.ptr(x), x.stride(0), L.ptr(w), w.stride(0),
           L.ptr(gs), gs.stride(0) if gs is not None else 0, L.ptr(dx), dx.stride(0), L.ptr(dw),
           dw.stride(0), L.ptr(db), m, n, k, L.ptr(wsx), L.nbytes(wsx), L.ptr(wsw), L.nbytes(wsw),
           L.stream())
    return lib.e2ep_gemm_workspace(m, k, n), lib.e2ep_gemm_rowsum_workspace(n, k, m)


@pytest.mark.parametrize("p", DY_PLACE)
@pytest.mark.parametrize("skip", [False, True], ids=["noskip", "gskip"])
@pytest.mark.parametrize("plan", ["plan", "split"])
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_linear_bwd(prec, plan, skip, p):
    """dX = dY W (+ gskip), dW = dY^T X, db = column sums of dY in one k_gemm_pair launch: six
    pairwise different leading dimensions, db 8 bytes off; as planned (neither problem splits)
    and with e2ep_gemm_split_min(1) and the fold on (both split three ways and fold)."""
    m, n, k = LB
    g = torch.Generator().manual_seed(7)
    dy, x = torch.randn(m, n, generator=g), torch.randn(m, k, generator=g)
    w, gs = torch.randn(n, k, generator=g) / k ** 0.5, torch.randn(m, k, generator=g)
    r = (lambda t: t.bfloat16().double()) if prec == "bf16" else (lambda t: t.double())
    want_dx = r(dy) @ r(w) + (gs.double() if skip else 0)
    want_dw = r(dy).t() @ r(x)
    want_db = r(dy).sum(0)
    ldy, offy = KPLACE[p]
    lds = (ldy, k + 3, k + 5, k + 7, k + 9, k + 11)
    assert len(set(lds)) == 6 and ldy > n
    with _settings(0, 0, 2 if plan == "split" else None, prec == "bf16",
                   1 if plan == "split" else None):
        dxd, dwd, dbd = (torch.full(s, float("nan"), device=DEV) for s in ((m, k), (n, k), (n,)))
        need = _linear_bwd(dy.to(DEV), x.to(DEV), w.to(DEV), gs.to(DEV) if skip else None, dxd,
                           dwd, dbd)
        assert (need[0] > 0 and need[1] > 0) == (plan == "split")  # both problems split, or neither
        for fill in FILLS:
            with guard.allocations(fill) as gd:
                dyp = P.placed(dy, ldy, offy, device=DEV)
                assert _vec_class(dyp) == VEC[p]
                xp = P.placed(x, lds[1], 1, device=DEV)
                wp = P.placed(w, lds[2], 3, device=DEV)
                gp = P.placed(gs, lds[3], 2, device=DEV) if skip else None
                dx = P.out((m, k), lds[4], 1, device=DEV)
                dw = P.out((n, k), lds[5], 3, device=DEV)
                db = P.out((n,), None, 2, device=DEV)
                assert db.data_ptr() % 16 == 8
                _linear_bwd(dyp, xp, wp, gp, dx, dw, db)
                what = f"linear_bwd {prec} {plan} skip {skip} dy {p}"
                _check(dx, want_dx, dxd, what + " dx")
                _check(dw, want_dw, dwd, what + " dw")
                _check(db, want_db, dbd, what + " db")
            gd.check()


# (rows M, out features N, AV1, precision): 20 rows or features put that half on the 32 x 128
# tile (WM = 1: 20 mod 64 is in 1..32), 40 on the 64 x 64 tile (WM = 2); dy's row length is N.
# The k_gemm_pair<WM1, AV1, OP, WM2> that test_linear_bwd and test_gemm_gpu.py leave out (read
# off a kernel trace).
PAIR_REST = [(20, 40, 0, "fp32"), (20, 40, 0, "bf16"), (20, 40, 1, "bf16"), (20, 40, 2, "bf16"),
             (40, 20, 0, "fp32"), (40, 40, 0, "fp32"), (40, 20, 0, "bf16"), (40, 40, 0, "bf16"),
             (40, 40, 1, "bf16"), (40, 20, 2, "bf16")]
# dy's (ld - N, off) per vector width
DY_VEC = {40: {2: (0, 0), 1: (0, 2), 0: (1, 0)}, 20: {2: (0, 0), 1: (2, 0), 0: (1, 0)}}


@pytest.mark.parametrize("m,n,av1,prec", PAIR_REST,
                         ids=[f"M{m}-N{n}-av{a}-{p}" for m, n, a, p in PAIR_REST])
def test_linear_bwd_remaining_instantiations(m, n, av1, prec):
    """One small unsplit e2ep_linear_bwd per k_gemm_pair instantiation no other test launches."""
    k = 50
    g = torch.Generator().manual_seed(m + 2 * n)
    dy, x = torch.randn(m, n, generator=g), torch.randn(m, k, generator=g)
    w = torch.randn(n, k, generator=g) / k ** 0.5
    r = (lambda t: t.bfloat16().double()) if prec == "bf16" else (lambda t: t.double())
    dld, offy = DY_VEC[n][av1]
    with _settings(0, 0, None, prec == "bf16"):
        dxd, dwd, dbd = (torch.full(s, float("nan"), device=DEV) for s in ((m, k), (n, k), (n,)))
        need = _linear_bwd(dy.to(DEV), x.to(DEV), w.to(DEV), None, dxd, dwd, dbd, (m, n, k))
        assert need == (0, 0)  # neither problem splits
        dyp = P.placed(dy, n + dld, offy, device=DEV)
        assert _vec_class(dyp) == av1
        dx, dw, db = P.out((m, k), k + 3, 1, device=DEV), P.out((n, k), k + 5, 3, device=DEV), P.out((n,), None, 2, device=DEV)
        _linear_bwd(dyp, P.placed(x, k + 1, 1, device=DEV), P.placed(w, k + 7, 3, device=DEV), None,
                    dx, dw, db, (m, n, k))
    what = f"linear_bwd {prec} M {m} N {n} av1 {av1}"
    _check(dx, r(dy) @ r(w), dxd, what + " dx")
    _check(dw, r(dy).t() @ r(x), dwd, what + " dw")
    _check(db, r(dy).sum(0), dbd, what + " db")


# ------------------------------------------------------------------------------------------
# the wrappers
# ------------------------------------------------------------------------------------------
def test_wrapper_gemm_out_strided_view():
    from e2ep_amd import nn_ops
    prob = _Problem(M, N, 77, True, True)
    for fill in FILLS:
        with guard.allocations(fill) as g:
            C = P.out((M, N), N + 3, 1, device=DEV)
            got = nn_ops.gemm(P.placed(prob.A, 80, 2, device=DEV), True,
                              P.placed(prob.B, 79, 0, device=DEV), True, M, N, 77, out=C)
            assert got is C
            dense = nn_ops.gemm(prob.A.to(DEV), True, prob.B.to(DEV), True, M, N, 77)
            _check(C, prob.plain, dense, "nn_ops.gemm(out=)")
        g.check()


@pytest.mark.parametrize("xs", ["xcols", "xrows"])
@pytest.mark.parametrize("ws", ["wrows", "wcols"])
def test_wrapper_linear_sliced_operands(xs, ws):
    """nn_ops.linear forward and backward with x a column / row slice of a larger tensor, weight
    a row / column slice (inner stride 1) and bias a slice, against fp64 autograd; the big
    tensors hold NaN outside the slices."""
    from e2ep_amd import nn_ops
    g = torch.Generator().manual_seed(21)
    R, K, Nf = 35, 77, 50
    x, w, b = torch.randn(2, R, K, generator=g), torch.randn(Nf, K, generator=g) / 8, torch.randn(Nf, generator=g)
    gy = torch.randn(2, R, Nf, generator=g)
    x64, w64, b64 = (t.double().requires_grad_() for t in (x, w, b))
    torch.nn.functional.linear(x64, w64, b64).backward(gy.double())
    for fill in FILLS:
        with guard.allocations(fill) as gd:
            nan = float("nan")
            if xs == "xcols":
                xb = torch.full((2, R, K + 3), nan)
                xb[..., 2:2 + K] = x
                xd = guard.put(xb).requires_grad_()
                xv = xd[..., 2:2 + K]
            else:
                xb = torch.full((4, R, K), nan)
                xb[1:3] = x
                xd = guard.put(xb).requires_grad_()
                xv = xd[1:3]
            if ws == "wrows":
                wb = torch.full((Nf + 4, K), nan)
                wb[3:3 + Nf] = w
                wd = guard.put(wb).requires_grad_()
                wv = wd[3:3 + Nf]
            else:
                wb = torch.full((Nf, K + 3), nan)
                wb[:, 1:1 + K] = w
                wd = guard.put(wb).requires_grad_()
                wv = wd[:, 1:1 + K]
            bb = torch.full((Nf + 3,), nan)
            bb[1:1 + Nf] = b
            bd = guard.put(bb).requires_grad_()
            y = nn_ops.linear(xv, wv, bd[1:1 + Nf])
            y.backward(gy.to(DEV))
            assert rel_l2(y, torch.nn.functional.linear(x64, w64, b64)) < TOL
            gx = xd.grad[..., 2:2 + K] if xs == "xcols" else xd.grad[1:3]
            gw = wd.grad[3:3 + Nf] if ws == "wrows" else wd.grad[:, 1:1 + K]
            assert rel_l2(gx, x64.grad) < TOL
            assert rel_l2(gw, w64.grad) < TOL
            assert rel_l2(bd.grad[1:1 + Nf], b64.grad) < TOL
            # the slices' complements got no gradient
            for full, part in ((xd.grad, gx), (wd.grad, gw), (bd.grad, bd.grad[1:1 + Nf])):
                assert not bool(full.isnan().any())
                part.zero_()
                assert not bool(full.any())
        gd.check()


@pytest.mark.parametrize("E", [26, 27])
def test_wrapper_in_proj_qkv(E):
    """weight[E:], bias[E:], dw[E:], db[E:] row slices (E = 27: bias[E:] 12 bytes off 16-byte
    alignment, E = 26: 8) forward and backward against fp64."""
    from e2ep_amd import nn_ops
    g = torch.Generator().manual_seed(E)
    xq, xkv = torch.randn(2, 7, E, generator=g), torch.randn(2, 19, E, generator=g)
    w, b = torch.randn(3 * E, E, generator=g) / 5, torch.randn(3 * E, generator=g)
    gq, gkv = torch.randn(2, 7, E, generator=g), torch.randn(2, 19, 2 * E, generator=g)
    gsq, gskv = torch.randn(2, 7, E, generator=g), torch.randn(2, 19, E, generator=g)
    r = [t.double().requires_grad_() for t in (xq, xkv, w, b)]
    q64 = torch.nn.functional.linear(r[0], r[2][:E], r[3][:E])
    kv64 = torch.nn.functional.linear(r[1], r[2][E:], r[3][E:])
    ((q64 * gq.double()).sum() + (kv64 * gkv.double()).sum() + (r[0] * gsq.double()).sum()
     + (r[1] * gskv.double()).sum()).backward()
    for fill in FILLS:
        with guard.allocations(fill) as gd:
            d = [guard.put(t).requires_grad_() for t in (xq, xkv, w, b)]
            q, kv, sq, skv = nn_ops.in_proj_qkv(d[0], d[1], d[2], d[3], E)
            ((q * gq.to(DEV)).sum() + (kv * gkv.to(DEV)).sum() + (sq * gsq.to(DEV)).sum()
             + (skv * gskv.to(DEV)).sum()).backward()
            assert rel_l2(q, q64) < TOL and rel_l2(kv, kv64) < TOL
            for got, want, name in zip(d, r, ("dxq", "dxkv", "dw", "db")):
                assert not bool(got.grad.isnan().any()), name
                assert rel_l2(got.grad, want.grad) < TOL, name
        gd.check()
