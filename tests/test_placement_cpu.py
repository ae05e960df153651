"""tests/placement.py on host tensors: the view it builds, what check_gaps reports, and that the
fp64 reference the GPU placement tests compare against cannot mistake a wrong placement for a
right one."""
import pytest
import torch

import guard
import placement as P
from helpers import rel_l2

# the k-contiguous placements of tests/test_gemm_placement_gpu.py (row length 77)
KPLACE = [(77, 0), (80, 0), (80, 2), (78, 0), (80, 1), (79, 0)]


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("ld,off", KPLACE)
def test_view_shape_strides_and_alignment(ld, off):
    t = torch.randn(70, 77, generator=torch.Generator().manual_seed(ld + off))
    v = P.placed(t, ld, off)
    assert tuple(v.shape) == (70, 77) and v.stride() == (ld, 1) and v.storage_offset() == off
    assert torch.equal(v, t)
    parent = P.parent_of(v)
    assert parent.dim() == 1 and parent.numel() == off + 69 * ld + 77 + P.TAIL
    assert parent.data_ptr() % 16 == 0 and v.data_ptr() % 16 == 4 * off % 16
    # every element outside the view is the fill, bit for bit
    assert P.gap_count(v) == parent.numel() - 70 * 77
    gaps = _bits(parent)[v._placement[1]]
    assert gaps.numel() == P.gap_count(v) and bool((gaps == P.NAN).all())
    assert bool(parent[v._placement[1]].isnan().all())
    P.check_gaps(v)


def test_vector_and_batched_views():
    b = P.placed(torch.arange(5.0), None, 3)
    assert tuple(b.shape) == (5,) and b.stride() == (1,) and b.data_ptr() % 16 == 12
    assert P.parent_of(b).numel() == 3 + 5 + P.TAIL
    t = torch.randn(3, 4, 6)
    v = P.placed(t, 9, 1)  # (B, R, ld) rows read as (B, R, C)
    assert v.stride() == (36, 9, 1) and torch.equal(v, t)
    x = torch.randn(2, 5, 3, 4)
    w = P.placed(x, off=2, strides=(5 * 12 + 7, 12, 4, 1))  # channel slices of a wider tensor
    assert w.stride() == (67, 12, 4, 1) and torch.equal(w, x)
    s = P.placed(torch.arange(12).view(3, 4), 7, 1, fill=9)
    assert s.dtype == torch.int64 and s.stride() == (7, 1)
    assert bool((P.parent_of(s)[s._placement[1]] == 9).all())
    with pytest.raises(AssertionError, match="overlap"):
        P.placed(torch.zeros(3, 4), 3, 0)


def test_output_placement_and_check_gaps():
    c = P.out((7, 5), 8, 1)
    assert bool(c.isnan().all())
    assert bool((_bits(P.parent_of(c))[c._placement[1]] == P.SENTINEL).all())
    c.copy_(torch.randn(7, 5))      # payload writes are accepted
    c[3, 4] = float("nan")          # whatever their value
    P.check_gaps(c)
    parent = P.parent_of(c)
    parent[1 + 2 * 8 + 6] = 1.5     # row 2, column 6: in the gap after the 5-wide payload
    with pytest.raises(AssertionError) as e:
        P.check_gaps(c, "C")
    msg = str(e.value)
    assert "C: 1 gap element" in msg and "parent offsets 23 .. 23" in msg
    assert "row 2 column 6" in msg and "column 4" in msg
    parent.view(torch.int32)[23] = P.SENTINEL
    P.check_gaps(c)
    # a NaN of another payload is a write too (bitwise, not isnan), and so is the head / tail
    parent.view(torch.int32)[23] = P.NAN
    with pytest.raises(AssertionError, match="row 2 column 6"):
        P.check_gaps(c)
    parent.view(torch.int32)[23] = P.SENTINEL
    parent[0] = 0.0
    parent[-1] = 0.0
    with pytest.raises(AssertionError, match="2 gap element.*1 element.s. before the view"):
        P.check_gaps(c)


@pytest.mark.parametrize("fill", [guard.FILL_A, guard.FILL_B])
def test_parent_is_guarded_inside_a_context(fill):
    t = torch.randn(6, 5)
    with guard.allocations(fill, device_type="cpu") as g:
        v = P.placed(t, 8, 3, device="cpu")
        assert g.owns(v) and g.owns(P.parent_of(v))
        assert P.parent_of(v).data_ptr() % guard.ALIGN == 0 and v.data_ptr() % 16 == 12
        assert torch.equal(v, t)
        g.check()
        parent = P.parent_of(v)  # one element past the parent: the trailing band
        parent.as_strided((1,), (1,), parent.storage_offset() + parent.numel())[0] = 1.0
        with pytest.raises(guard.GuardError, match="trailing"):
            g.check()
    u = P.placed(t, 8, 3, device="cpu")  # outside a context: a plain copy
    assert not guard.owns(u) and torch.equal(u, t)


@pytest.mark.parametrize("K", [77, 96])
def test_fp64_reference_notices_a_wrong_placement(K):
    """A kernel that ignored `ld` or the base offset of one operand computes the product of the
    parent misread; with zero gaps that is rel-L2 1.37 .. 1.44 from the true one for every
    placement below, five orders over the 2e-6 the GPU tests allow.  Bound 0.1."""
    M, N = 70, 130
    g = torch.Generator().manual_seed(K)
    A, B = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g)
    ref = A.double() @ B.double().t()
    assert rel_l2(A @ B.t(), ref) < 2e-6  # (the fp32 product itself: 1.6e-7)
    for ld, off in KPLACE:
        ld += K - 77
        for which in "AB":
            v = P.placed(A if which == "A" else B, ld, off, fill=P.ZERO)
            rows = v.shape[0]
            parent = P.parent_of(v)
            wrong = []
            if ld != K:
                wrong.append(parent.as_strided((rows, K), (K, 1), off))
            if off:
                wrong.append(parent.as_strided((rows, K), (ld, 1), 0))
            for m in wrong:
                got = (m.double() @ B.double().t()) if which == "A" else (A.double() @ m.double().t())
                err = rel_l2(got, ref)
                print(f"K={K} {which} ld={ld} off={off}: misread rel-L2 {err:.3f}")
                assert err > 0.1
            got = (v.double() @ B.double().t()) if which == "A" else (A.double() @ v.double().t())
            assert rel_l2(got, ref) == 0.0
