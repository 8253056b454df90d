"""GPU parity of every C-ABI entry called with RGBNM_DT_F16 (fp16 activations and MFMA operands, fp32 accumulate) against
torch fp32 computed on the same fp16-rounded operands.  fp16 keeps 10 mantissa bits (bf16: 7), so the bars here sit well
below the bf16 bars of tests/test_hip_kernels.py.  Conversions must behave like torch's `.half()`: round to nearest even,
overflow to +-inf, subnormals kept, NaN propagated."""
import math

import numpy as np
import pytest
import torch

import rgb_no_more_amd as rg
from rgb_no_more_amd import detfill, lib as L

pytestmark = pytest.mark.gpu

DEV = "cuda"
H = torch.float16


def dev(a, dt=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV).to(dt).contiguous()


def relerr(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def gemm_nt(epi, A, W, bias=None, R=None, pos=None, period=0, c_f32=False):
    M, K = A.shape
    N = W.shape[0]
    Cc = torch.empty(M, N, device=DEV, dtype=torch.float32 if c_f32 else H)
    C2 = torch.empty(M, N, device=DEV, dtype=H) if epi == L.EPI_GELU else None
    L.check(L.lib().rgbnm_gemm_nt(L.DT_F16, epi, A.data_ptr(), K, W.data_ptr(), K, Cc.data_ptr(), N, L.ptr(bias),
                                  L.ptr(R), N, L.ptr(C2), N, L.ptr(pos), period, M, N, K, int(c_f32), L.stream()))
    torch.cuda.synchronize()
    return Cc, C2


# (392, 192): staged epilogue; (300, 200): ragged N -> direct epilogue; (256, 1000): head width, N % 8 == 0
@pytest.mark.parametrize("M,N,K", [(392, 192, 192), (300, 200, 384), (256, 1000, 192), (1568, 576, 192)])
def test_gemm_nt_all_epilogues(M, N, K):
    A = dev(detfill.normalish((M, K), 11), H)
    W = dev(detfill.uniform((N, K), 12, -0.1, 0.1), H)
    b = dev(detfill.uniform((N,), 13))
    R = dev(detfill.normalish((M, N), 14), H)
    base = A.float() @ W.float().T
    out, _ = gemm_nt(L.EPI_NONE, A, W, b)
    assert relerr(out, base + b) < 1e-3
    out32, _ = gemm_nt(L.EPI_NONE, A, W, b, c_f32=True)
    assert out32.dtype == torch.float32 and relerr(out32, base + b) < 2e-6
    out, _ = gemm_nt(L.EPI_RES, A, W, b, R=R)
    assert relerr(out, base + b + R.float()) < 1e-3
    out, dg = gemm_nt(L.EPI_GELU, A, W, b)
    u = (base + b).to(H).float().requires_grad_(True)      # pre-activation at fp16 precision
    gref = torch.nn.functional.gelu(u)
    gref.sum().backward()
    assert relerr(out, gref) < 1e-3
    assert relerr(dg, u.grad) < 1e-3
    pos = dev(detfill.uniform((196, N), 15))
    out, _ = gemm_nt(L.EPI_POS, A, W, b, pos=pos, period=196)
    rows = torch.arange(M, device=DEV) % 196
    assert relerr(out, base + b + pos[rows]) < 1e-3
    out, _ = gemm_nt(L.EPI_DGELU, A, W, None, R=R)
    assert relerr(out, base * R.float()) < 1e-3
    out, _ = gemm_nt(L.EPI_TANH, A, W, b)
    assert relerr(out, torch.tanh(base + b)) < 1e-3
    h = torch.tanh(R.float()).to(H)
    out, _ = gemm_nt(L.EPI_DTANH, A, W, None, R=h)
    assert relerr(out, base * (1 - h.float() ** 2)) < 1e-3


def test_gemm_nt_fp16_is_finer_than_bf16():
    """Same operands (exact in both formats), same fp32 accumulation: the fp16 result's rounding error is about 8x smaller."""
    M, N, K = 392, 192, 192
    A32 = torch.from_numpy(detfill.normalish((M, K), 16)).bfloat16().float().to(DEV)
    W32 = torch.from_numpy(detfill.uniform((N, K), 17, -0.1, 0.1)).bfloat16().float().to(DEV)
    ref = A32 @ W32.T
    errs = {}
    for dt, code in ((H, L.DT_F16), (torch.bfloat16, L.DT_BF16)):
        Cc = torch.empty(M, N, device=DEV, dtype=dt)
        A, W = A32.to(dt), W32.to(dt)
        L.check(L.lib().rgbnm_gemm_nt(code, L.EPI_NONE, A.data_ptr(), K, W.data_ptr(), K, Cc.data_ptr(), N, None, None, N,
                                      None, N, None, 0, M, N, K, 0, L.stream()))
        torch.cuda.synchronize()
        errs[dt] = relerr(Cc, ref)
    assert errs[H] < errs[torch.bfloat16] / 4, errs


@pytest.mark.parametrize("N", [192, 200])       # staged and direct epilogue
def test_gemm_nt_overflow_nan_and_subnormals(N):
    M, K = 256, 192
    A = torch.full((M, K), 300.0, device=DEV, dtype=H)
    A[1] = -300.0
    A[2] = 2.0 ** -12
    A[3, 5] = float("nan")
    A[4:] = 1.0
    W = torch.full((N, K), 300.0, device=DEV, dtype=H)
    W[:, 16:] = 0
    W[:, :16] = 300.0
    out, _ = gemm_nt(L.EPI_NONE, A, W)
    # row 0: 16 * 300 * 300 = 1.44e6 > 65504 -> +inf; row 1 -> -inf (not saturated to the largest finite value)
    assert torch.isinf(out[0]).all() and (out[0] > 0).all()
    assert torch.isinf(out[1]).all() and (out[1] < 0).all()
    # a NaN operand propagates to its whole row
    assert torch.isnan(out[3]).all()
    assert torch.isfinite(out[4:]).all()
    assert (out[4:].cpu() == 4800.0).all() and (out[2].cpu() == 1.171875).all()
    # a subnormal result survives
    Ws = torch.zeros(N, K, device=DEV, dtype=H)
    Ws[:, :16] = 2.0 ** -12
    As = torch.full((M, K), 2.0 ** -12, device=DEV, dtype=H)
    out, _ = gemm_nt(L.EPI_NONE, As, Ws)
    want = torch.tensor(16 * 2.0 ** -24, dtype=H)          # 2^-20: fp16 subnormal (smallest normal 2^-14)
    assert want.item() != 0.0
    assert (out.cpu() == want).all()
    # rounding to nearest even, as torch's .half(): values between two fp16 neighbours
    x = torch.from_numpy(detfill.normalish((M, K), 18)).to(DEV) * 100
    eye = torch.zeros(N, K, device=DEV, dtype=H)
    n = min(N, K)
    eye[torch.arange(n), torch.arange(n)] = 1.0
    b = torch.from_numpy(detfill.normalish((N,), 19)).float().to(DEV) * 0.37
    xh = x.half()
    out, _ = gemm_nt(L.EPI_NONE, xh, eye, bias=b)
    ref = (xh.float()[:, :n] + b[:n]).half()
    assert torch.equal(out[:, :n], ref)


@pytest.mark.parametrize("M,No,Ki,heads", [(1568, 576, 192, 3), (392, 192, 768, 0), (100, 1000, 192, 0), (260, 192, 384, 0)])
def test_gemm_tn(M, No, Ki, heads):
    dY = dev(detfill.normalish((M, No), 21), H)
    X = dev(detfill.normalish((M, Ki), 22), H)
    dW = torch.full((No, Ki), 7.0, device=DEV)
    db = torch.full((No,), 7.0, device=DEV)
    wsb = L.lib().rgbnm_gemm_tn_workspace(M, No, Ki)
    ws = torch.empty(wsb, device=DEV, dtype=torch.uint8)
    L.check(L.lib().rgbnm_gemm_tn(L.DT_F16, dY.data_ptr(), No, X.data_ptr(), Ki, dW.data_ptr(), db.data_ptr(), M, No,
                                  Ki, heads, 0, ws.data_ptr(), wsb, L.stream()))
    ref = dY.float().T @ X.float()
    rb = dY.float().sum(0)
    if heads:
        inner = heads * 64
        n = torch.arange(No, device=DEV)
        s3, rem = n // inner, n % inner
        dst = (rem // 64) * 192 + (rem % 64) * 3 + s3
        r2, b2 = torch.empty_like(ref), torch.empty_like(rb)
        r2[dst] = ref
        b2[dst] = rb
        ref, rb = r2, b2
    torch.cuda.synchronize()
    assert relerr(dW, ref) < 1e-5 and relerr(db, rb) < 1e-5     # fp16 inputs are exact in fp32; fp32 accumulate
    L.check(L.lib().rgbnm_gemm_tn(L.DT_F16, dY.data_ptr(), No, X.data_ptr(), Ki, dW.data_ptr(), db.data_ptr(), M, No,
                                  Ki, heads, 1, ws.data_ptr(), wsb, L.stream()))
    torch.cuda.synchronize()
    assert relerr(dW, 2 * ref) < 1e-5


def ref_attention(qkv, B, N, Hh, scale):
    I = Hh * 64
    q, k, v = [qkv[:, i * I:(i + 1) * I].reshape(B, N, Hh, 64).permute(0, 2, 1, 3) for i in range(3)]
    s = (q @ k.transpose(-1, -2)) * scale
    out = (torch.softmax(s, dim=-1) @ v).permute(0, 2, 1, 3).reshape(B * N, I)
    return out, torch.logsumexp(s, dim=-1)


@pytest.mark.parametrize("B,N,Hh", [(3, 196, 3), (2, 196, 6), (1, 100, 2), (2, 294, 3)])
def test_attention_fwd_bwd(B, N, Hh):
    I = Hh * 64
    scale = 1.0 / math.sqrt(Hh * 64)
    qkv = dev(detfill.normalish((B * N, 3 * I), 41) * 1.5, H)
    out = torch.empty(B * N, I, device=DEV, dtype=H)
    lse = torch.empty(B * Hh * N, device=DEV)
    L.check(L.lib().rgbnm_attention_fwd(L.DT_F16, qkv.data_ptr(), out.data_ptr(), lse.data_ptr(), B, N, Hh, scale, L.stream()))
    qr = qkv.float().clone().requires_grad_(True)
    oref, lref = ref_attention(qr, B, N, Hh, scale)
    torch.cuda.synchronize()
    assert relerr(out, oref) < 1.5e-3, relerr(out, oref)          # (bf16 bar: 6e-3)
    assert relerr(lse.view(B, Hh, N), lref) < 2e-6
    dout = dev(detfill.normalish((B * N, I), 42), H)
    oref.backward(dout.float())
    dqkv = torch.full_like(qkv, float("nan"))
    L.check(L.lib().rgbnm_attention_bwd(L.DT_F16, qkv.data_ptr(), out.data_ptr(), dout.data_ptr(), lse.data_ptr(),
                                        dqkv.data_ptr(), B, N, Hh, scale, L.stream()))
    torch.cuda.synchronize()
    assert torch.isfinite(dqkv.float()).all()
    for i, nm in enumerate("qkv"):
        e = relerr(dqkv[:, i * I:(i + 1) * I], qr.grad[:, i * I:(i + 1) * I])
        assert e < 4e-3, (nm, e)                                  # (bf16 bar: 1.5e-2)


@pytest.mark.parametrize("E", [192, 384, 768])
def test_layernorm(E):
    M = 1000
    x = dev(detfill.normalish((M, E), 31) * 2 + 0.5, H)
    g = dev(1 + detfill.uniform((E,), 32, -0.2, 0.2))
    b = dev(detfill.uniform((E,), 33, -0.2, 0.2))
    y = torch.empty_like(x)
    mean, rstd = torch.empty(M, device=DEV), torch.empty(M, device=DEV)
    L.check(L.lib().rgbnm_layernorm_fwd(L.DT_F16, x.data_ptr(), g.data_ptr(), b.data_ptr(), y.data_ptr(), mean.data_ptr(),
                                        rstd.data_ptr(), M, E, 1e-5, L.stream()))
    xr = x.float().clone().requires_grad_(True)
    gr, br = g.clone().requires_grad_(True), b.clone().requires_grad_(True)
    yr = torch.nn.functional.layer_norm(xr, (E,), gr, br, 1e-5)
    torch.cuda.synchronize()
    assert relerr(y, yr) < 5e-4                                   # (bf16 bar: 3e-3)
    assert relerr(mean, xr.mean(1)) < 1e-5
    dy = dev(detfill.normalish((M, E), 34), H)
    dres = dev(detfill.normalish((M, E), 35), H)
    yr.backward(dy.float())
    dx = torch.empty_like(x)
    dg, dbt = torch.empty(E, device=DEV), torch.empty(E, device=DEV)
    wsb = L.lib().rgbnm_layernorm_bwd_workspace(M, E)
    ws = torch.empty(wsb, device=DEV, dtype=torch.uint8)
    L.check(L.lib().rgbnm_layernorm_bwd(L.DT_F16, dy.data_ptr(), x.data_ptr(), g.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                                        dres.data_ptr(), dx.data_ptr(), dg.data_ptr(), dbt.data_ptr(), M, E, 0, ws.data_ptr(),
                                        wsb, L.stream()))
    torch.cuda.synchronize()
    assert relerr(dx, xr.grad + dres.float()) < 7e-4             # (bf16 bar: 4e-3)
    assert relerr(dg, gr.grad) < 1e-5 and relerr(dbt, br.grad) < 1e-5


@pytest.mark.parametrize("E", [192, 384, 1024])
def test_pool_fwd_bwd(E):
    B, N = 4, 196
    x = dev(detfill.normalish((B * N, E), 36) * 2 + 0.3, H)
    g = dev(1 + detfill.uniform((E,), 37, -0.2, 0.2))
    b = dev(detfill.uniform((E,), 38, -0.2, 0.2))
    pooled = torch.empty(B, E, device=DEV, dtype=H)
    mean, rstd = torch.empty(B * N, device=DEV), torch.empty(B * N, device=DEV)
    L.check(L.lib().rgbnm_head_pool_fwd(L.DT_F16, x.data_ptr(), g.data_ptr(), b.data_ptr(), pooled.data_ptr(),
                                        mean.data_ptr(), rstd.data_ptr(), B, N, E, 1e-5, L.stream()))
    xr = x.float().clone().requires_grad_(True)
    gr, br = g.clone().requires_grad_(True), b.clone().requires_grad_(True)
    pr = torch.nn.functional.layer_norm(xr, (E,), gr, br, 1e-5).view(B, N, E).mean(1)
    torch.cuda.synchronize()
    assert relerr(pooled, pr) < 1e-3
    dp = dev(detfill.normalish((B, E), 39), H)
    pr.backward(dp.float())
    dx = torch.empty_like(x)
    dg, dbt = torch.empty(E, device=DEV), torch.empty(E, device=DEV)
    wsb = max(L.lib().rgbnm_layernorm_bwd_workspace(B * N, E), B * 2 * E * 4)
    ws = torch.empty(wsb, device=DEV, dtype=torch.uint8)
    L.check(L.lib().rgbnm_head_pool_bwd(L.DT_F16, dp.data_ptr(), x.data_ptr(), g.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                                        dx.data_ptr(), dg.data_ptr(), dbt.data_ptr(), B, N, E, 0, ws.data_ptr(), wsb,
                                        L.stream()))
    torch.cuda.synchronize()
    assert relerr(dx, xr.grad) < 1e-3
    assert relerr(dg, gr.grad) < 1e-5 and relerr(dbt, br.grad) < 1e-5


def _subblock(in_code, out_dt, y, c, A, lam=None, B=2, Hb=4, Wb=6):
    feat = torch.empty(B * (Hb // 2) * (Wb // 2), 384, device=DEV, dtype=out_dt)
    L.check(L.lib().rgbnm_subblock_embed_mix(in_code, L.dt_of(out_dt), y.data_ptr(), c.data_ptr(), L.ptr(lam), A.data_ptr(),
                                             feat.data_ptr(), B, Hb, Wb, 0, L.stream()))
    torch.cuda.synchronize()
    return feat


def test_subblock_embed_fp16_output_is_the_fp32_output_rounded():
    y = dev(detfill.normalish((2, 1, 4, 6, 8, 8), 61) * 300)
    c = dev(detfill.normalish((2, 2, 2, 3, 8, 8), 62) * 300)
    A = rg.dct_ops.generate_conversion_matrix(8, 2).to(DEV).contiguous()
    f32 = _subblock(L.DT_F32, torch.float32, y, c, A)
    assert torch.equal(_subblock(L.DT_F32, H, y, c, A), f32.half())
    # with the mixup applied while loading (fp32 input: the mixed values stay fp32 in both kernels)
    lam = torch.tensor([0.7, 0.3], device=DEV)
    assert torch.equal(_subblock(L.DT_F32, H, y, c, A, lam), _subblock(L.DT_F32, torch.float32, y, c, A, lam).half())
    # bf16 and fp16 inputs: the same as the fp32 kernel on the (exactly widened) inputs, rounded
    for dt, code in ((torch.bfloat16, L.DT_BF16), (H, L.DT_F16)):
        yi, ci = y.to(dt), c.to(dt)
        want = _subblock(L.DT_F32, torch.float32, yi.float().contiguous(), ci.float().contiguous(), A).half()
        assert torch.equal(_subblock(code, H, yi, ci, A), want), dt


@pytest.mark.parametrize("hard", [False, True])
def test_softxent_fp16_gradient_is_the_fp32_gradient_rounded(hard):
    B, Cn = 37, 1000
    z = dev(detfill.normalish((B, Cn), 51) * 3)
    if hard:
        t = torch.from_numpy(detfill.integers((B,), 52, 0, Cn - 1, np.int64)).to(DEV)
    else:
        tt = detfill.uniform((B, Cn), 53, 0, 1)
        t = dev(tt / tt.sum(1, keepdims=True))
    lib, s = L.lib(), L.stream()
    rows, loss = torch.empty(B, device=DEV), torch.empty(1, device=DEV)
    soft, lab = (None, t.data_ptr()) if hard else (t.data_ptr(), None)
    d32 = torch.empty(B, Cn, device=DEV)
    d16 = torch.empty(B, Cn, device=DEV, dtype=H)
    scale = 65536.0 / B                  # a GradScaler-sized gradient: still well inside fp16's range
    L.check(lib.rgbnm_softxent(L.DT_F32, z.data_ptr(), soft, lab, rows.data_ptr(), loss.data_ptr(), d32.data_ptr(), B, Cn, scale, s))
    L.check(lib.rgbnm_softxent(L.DT_F16, z.data_ptr(), soft, lab, rows.data_ptr(), loss.data_ptr(), d16.data_ptr(), B, Cn, scale, s))
    torch.cuda.synchronize()
    assert torch.equal(d16, d32.half())
    # the two-launch form (loss, then gradient from the saved row statistics)
    stat, ticket = torch.empty(2 * B, device=DEV), torch.zeros(1, device=DEV, dtype=torch.int32)
    gout = torch.ones(1, device=DEV)
    L.check(lib.rgbnm_softxent_loss(z.data_ptr(), soft, lab, rows.data_ptr(), stat.data_ptr(), loss.data_ptr(), ticket.data_ptr(),
                                    B, Cn, s))
    L.check(lib.rgbnm_softxent_grad(L.DT_F32, z.data_ptr(), soft, lab, stat.data_ptr(), gout.data_ptr(), d32.data_ptr(), B, Cn,
                                    scale, s))
    L.check(lib.rgbnm_softxent_grad(L.DT_F16, z.data_ptr(), soft, lab, stat.data_ptr(), gout.data_ptr(), d16.data_ptr(), B, Cn,
                                    scale, s))
    torch.cuda.synchronize()
    assert torch.equal(d16, d32.half())
    if hard:        # lazy mixup target
        lam = torch.tensor([0.6, 0.4], device=DEV)
        L.check(lib.rgbnm_softxent_loss_mix(z.data_ptr(), t.data_ptr(), lam.data_ptr(), rows.data_ptr(), stat.data_ptr(),
                                            loss.data_ptr(), ticket.data_ptr(), B, Cn, s))
        L.check(lib.rgbnm_softxent_grad_mix(L.DT_F32, z.data_ptr(), t.data_ptr(), lam.data_ptr(), stat.data_ptr(), gout.data_ptr(),
                                            d32.data_ptr(), B, Cn, scale, s))
        L.check(lib.rgbnm_softxent_grad_mix(L.DT_F16, z.data_ptr(), t.data_ptr(), lam.data_ptr(), stat.data_ptr(), gout.data_ptr(),
                                            d16.data_ptr(), B, Cn, scale, s))
        torch.cuda.synchronize()
        assert torch.equal(d16, d32.half())
