"""CPU self-test of tests/kernel_check.py on synthetic outputs of an fp64 GEMM: the element-wise bound accepts the correctly
rounded result and the result one ulp off in every element type, and rejects the defects that a Frobenius-norm relative
error lets through at the bars of the existing kernel tests (relerr in tests/test_hip_kernels.py)."""
import torch
import pytest

import kernel_check as KC
from test_hip_kernels import relerr

TYPES = [torch.bfloat16, torch.float16, torch.float32]


def gemm64(M, N, K, dtype, seed):
    """ref = A W^T in fp64 of T-rounded operands, mag = |A| |W|^T, K: the bound's reduction length."""
    g = torch.Generator().manual_seed(seed)
    A = torch.randn(M, K, generator=g).to(dtype).double()
    W = (torch.rand(N, K, generator=g) * 0.2 - 0.1).to(dtype).double()
    return A @ W.T, A.abs() @ W.abs().T


def bound_ok(got, ref, mag, dtype, K):
    return KC.check_bound(got, ref, mag, dtype, 1, K * KC.U, "synthetic", tile=(128, 192))


def one_ulp_off(x, dtype):
    """x (already T-representable) moved one ulp away from zero, element-wise."""
    bits = x.contiguous().view(KC._INT[x.element_size()])
    return (bits + 1).view(dtype)


def other_neighbour(ref, dtype):
    """The T-neighbour of ref on the other side from round-to-nearest: a faithfully but not correctly rounded result,
    up to one ulp from ref."""
    r = ref.to(dtype)
    bits = r.view(KC._INT[r.element_size()]).clone()
    down = (r.double().abs() > ref.abs()) & (r != 0)     # sign-magnitude: bits - 1 is the smaller magnitude
    bits = torch.where(down, bits - 1, bits + 1)
    return bits.view(dtype)


@pytest.mark.parametrize("dtype", TYPES)
def test_accepts_correctly_rounded_and_one_ulp(dtype):
    ref, mag = gemm64(392, 192, 64, dtype, 1)
    got = ref.to(dtype)
    assert bound_ok(got, ref, mag, dtype, 64) <= 1.0
    off = other_neighbour(ref, dtype)
    assert (off != got).all()
    assert bound_ok(off, ref, mag, dtype, 64) <= 1.0


@pytest.mark.parametrize("dtype", TYPES)
def test_rejects_three_ulps_in_one_element(dtype):
    # K = 1: the reduction term k u mag is then below half an fp32 ulp, so the bound is at most 1.5 ulps in every type
    # (at k >= 6 the fp32 accumulation term alone admits 3 fp32 ulps)
    ref, mag = gemm64(64, 64, 1, dtype, 2)
    got = ref.to(dtype)
    bits = got.view(KC._INT[got.element_size()]).clone()
    bits[5, 7] += 3
    with pytest.raises(AssertionError, match=r"\(5, 7\)"):
        bound_ok(bits.view(dtype), ref, mag, dtype, 1)


def test_rejects_one_zeroed_row_that_relerr_passes():
    M, N, K = 50176, 192, 64
    ref, mag = gemm64(M, N, K, torch.bfloat16, 3)
    got = ref.to(torch.bfloat16)
    got[31337] = 0
    assert relerr(got, ref) < 6e-3                # test_gemm_nt_epilogues' bar
    with pytest.raises(AssertionError, match=r"tile \(244, 0\)"):
        bound_ok(got, ref, mag, torch.bfloat16, K)


def test_rejects_one_block_at_half_error_that_relerr_passes():
    M, N, K = 9800, 384, 64                        # a dq / dk / dv slice at B = 50, N = 196, H = 6
    ref, mag = gemm64(M, N, K, torch.bfloat16, 4)
    got = ref.clone()
    got[4096:4128, 128:192] *= 1.5
    got = got.to(torch.bfloat16)
    assert relerr(got, ref) < 1.5e-2              # test_attention_bf16_backward_schedules' bar
    with pytest.raises(AssertionError, match="2048 of"):
        bound_ok(got, ref, mag, torch.bfloat16, K)


def test_rejects_one_row_at_ten_percent_that_relerr_passes():
    M, N, K = 392, 192, 192
    ref, mag = gemm64(M, N, K, torch.bfloat16, 5)
    got = ref.clone()
    got[200] *= 1.1
    got = got.to(torch.bfloat16)
    assert relerr(got, ref) < 6e-3                # test_gemm_nt_epilogues' bar
    with pytest.raises(AssertionError, match=r"\(200, "):
        bound_ok(got, ref, mag, torch.bfloat16, K)


def test_rejects_two_swapped_columns():
    ref, mag = gemm64(256, 192, 64, torch.bfloat16, 6)
    got = ref.to(torch.bfloat16)
    got[:, [100, 101]] = got[:, [101, 100]]
    with pytest.raises(AssertionError, match="out of bound"):
        bound_ok(got, ref, mag, torch.bfloat16, 64)


@pytest.mark.parametrize("dtype", TYPES)
def test_guards_see_margin_gap_and_unwritten_elements(dtype):
    g = KC.guarded(33, 40, dtype, ld=48, device="cpu")
    assert g.t.shape == (33, 40) and g.t.stride() == (48, 1)
    assert torch.isnan(g.t.float()).all()         # the canary is a NaN: an unwritten element cannot pass a bound either
    with pytest.raises(AssertionError, match="1320 output elements never written"):
        g.check("fresh")
    g.t.copy_(torch.ones(33, 40))
    g.check("written")
    g.raw.view(torch.uint8)[KC.GUARD_BYTES * 2 + 33 * 48 * g.esz - 1] ^= 1   # one byte of the back margin
    with pytest.raises(AssertionError, match="back margin: 1 elements changed"):
        g.check("margin")
    g = KC.guarded(33, 40, dtype, ld=48, device="cpu")
    g.t.copy_(torch.ones(33, 40))
    g.raw.view(torch.uint8)[0] ^= 0x80             # first byte of the front margin
    with pytest.raises(AssertionError, match="front margin"):
        g.check("front")
    g = KC.guarded(33, 40, dtype, ld=48, device="cpu")
    g.t.copy_(torch.ones(33, 40))
    g.t.as_strided((1,), (1,), g.t.storage_offset() + 7 * 48 + 44)[0] = 0   # inside the ld gap of row 7
    with pytest.raises(AssertionError, match=r"ld gap: 1 elements changed, first \(row, col\) \[\(7, 44\)\]"):
        g.check("gap")
    g = KC.guarded(33, 40, dtype, ld=48, device="cpu")
    g.t.copy_(torch.ones(33, 40))
    g.raw[g.off + 12 * 48 + 3] = g.canary          # one output element left at the canary
    with pytest.raises(AssertionError, match=r"1 output elements never written, first \[\(12, 3\)\]"):
        g.check("unwritten")


def test_guarded_vector_and_nan_padding():
    v = KC.guarded(10, None, torch.float32, device="cpu")
    v.t.copy_(torch.arange(10.0))
    v.check("vec")
    x = torch.arange(12.0).view(3, 4)
    p = KC.nan_padded(x, ld=8, extra_rows=2)
    assert torch.equal(p, x) and p.stride() == (8, 1)
    full = p.as_strided((5, 8), (8, 1))
    assert torch.isnan(full[:, 4:]).all() and torch.isnan(full[3:]).all()


def test_ulp_definition():
    for dtype, p in ((torch.bfloat16, 7), (torch.float16, 10), (torch.float32, 23)):
        x = torch.tensor([1.0, 1.5, 2.0, -3.0, 0.0])
        u = KC.ulp(x, dtype)
        assert u[0] == 2.0 ** -p and u[1] == 2.0 ** -p and u[2] == 2.0 ** (1 - p) and u[3] == 2.0 ** (1 - p)
        emin = -14 if dtype == torch.float16 else -126
        assert u[4] == 2.0 ** (emin - p)
        # the grid spacing of T itself at 1.0
        one = torch.ones(1, dtype=dtype)
        assert float(one_ulp_off(one, dtype).double() - 1.0) == 2.0 ** -p
