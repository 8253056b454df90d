"""SwinV2's own kernels in fp16 (window attention, the any-width LayerNorm, the sub-block embedding, the merge gather, the token
mean) against the fp32 oracle.  The bars calibrate themselves, as in tests/test_fp16_model.py: every error is measured for bf16 on
the same inputs as well, and fp16 (three more mantissa bits) must come in at a quarter of it or better -- except window attention's
d(scale), a heavily cancelling sum with one entry per head, whose measured fp16 / bf16 ratio is 0.14 - 0.30 (pooled over four output
gradients; the other attention figures: 0.09 - 0.16): a third there.  Inputs are rounded to bf16 first, so both modes see the same
(exactly representable) values and only the kernels' own rounding differs."""
import numpy as np
import pytest
import torch

from rgb_no_more_amd import detfill, lib as L, swinv2 as SW
from oracle import swin_torch as S

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTS = (torch.bfloat16, torch.float16)


def _bf(a):
    """fp32 values that bf16 and fp16 both hold exactly (normal range, 8 significant bits)."""
    return torch.from_numpy(a).bfloat16().float()


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def _check(errs, what, ratio=0.25):
    e16, ebf = errs[torch.float16], errs[torch.bfloat16]
    print(f"   {what}: fp16 {e16:.3e} bf16 {ebf:.3e} (ratio {e16 / max(ebf, 1e-30):.3f})")
    assert np.isfinite(e16)
    assert e16 <= ebf * ratio, (what, e16, ebf)


# ------------------------------------------------------------------------------------------------ window attention
def _attn_oracle(qkv32, bias, scale, B, res, heads, shift, w):
    C_ = heads * 32
    q32 = qkv32.clone().requires_grad_(True)
    bias_r, scale_r = bias.clone().requires_grad_(True), scale.clone().requires_grad_(True)
    x = q32.reshape(B, res, res, 3 * C_)
    xs = torch.roll(x, (-shift, -shift), (1, 2)) if shift else x
    nw = res // 8
    xw = xs.reshape(B, nw, 8, nw, 8, 3 * C_).permute(0, 1, 3, 2, 4, 5).reshape(B * nw * nw, 64, 3, heads, 32)
    q, k, v = xw.permute(2, 0, 3, 1, 4)
    att = torch.nn.functional.normalize(q, dim=-1) @ torch.nn.functional.normalize(k, dim=-1).transpose(-2, -1)
    att = att * scale_r.view(1, heads, 1, 1) + bias_r.unsqueeze(0)
    if shift:
        m = S.shift_mask(res, 8, shift)
        att = (att.reshape(B, nw * nw, heads, 64, 64) + m[None, :, None]).reshape(-1, heads, 64, 64)
    lse = torch.logsumexp(att, -1).detach().reshape(-1)           # [(window, head, query)]: the kernel's lse layout
    o = (torch.softmax(att, -1) @ v).transpose(1, 2).reshape(B, nw, nw, 8, 8, C_).permute(0, 1, 3, 2, 4, 5)
    o = o.reshape(B, res, res, C_)
    ref = (torch.roll(o, (shift, shift), (1, 2)) if shift else o).reshape(B * res * res, C_)
    (ref * w).sum().backward()
    return ref.detach(), lse, q32.grad, bias_r.grad, scale_r.grad


@pytest.mark.parametrize("res,heads,shift", [(16, 3, 0), (16, 3, 4), (8, 6, 0), (32, 3, 4)])
def test_window_attention_fp16_vs_oracle_and_bf16(res, heads, shift):
    B, C_ = 2, heads * 32
    qkv32 = _bf(detfill.normalish((B * res * res, 3 * C_), 21))
    bias = torch.from_numpy(detfill.uniform((heads, 64, 64), 22, 0.0, 16.0)).float()
    scale = torch.from_numpy(detfill.uniform((heads,), 23, 5.0, 30.0)).float()
    # the gradients are pooled over four output-gradient draws: d(scale) has one entry per head, a heavily cancelling sum, and its
    # error on a single draw is as much luck as arithmetic
    ws = [torch.from_numpy(detfill.normalish((B * res * res, C_), 24 + k)).float() for k in range(4)]   # fp32: dO is rounded
    refs = [_attn_oracle(qkv32, bias, scale, B, res, heads, shift, w) for w in ws]
    ref, lse_ref = refs[0][0], refs[0][1]
    errs = {k: {} for k in ("out", "lse", "dqkv", "dbias", "dscale")}
    for dt in DTS:
        got = []
        for w in ws:
            qg = qkv32.to(DEV).to(dt).requires_grad_(True)
            bg, sg = bias.to(DEV).requires_grad_(True), scale.to(DEV).requires_grad_(True)
            out = SW._WinAttnFn.apply(qg, bg, sg, B, res, C_, heads, shift)
            assert out.dtype == dt
            lse = out.grad_fn.saved_tensors[4]
            (out.float() * w.to(DEV)).sum().backward()
            torch.cuda.synchronize()
            assert qg.grad.dtype == dt and torch.isfinite(qg.grad.float()).all()
            got.append((qg.grad.float(), bg.grad, sg.grad))
        errs["out"][dt] = (out.float().cpu() - ref).abs().max().item()
        errs["lse"][dt] = (lse.cpu() - lse_ref).abs().max().item()
        for i, k in enumerate(("dqkv", "dbias", "dscale")):
            errs[k][dt] = _rel(torch.cat([x[i].reshape(-1) for x in got]), torch.cat([r[2 + i].reshape(-1) for r in refs]))
    print(f"[win attn res={res} heads={heads} shift={shift}]")
    for k, e in errs.items():
        _check(e, k, 1 / 3 if k == "dscale" else 0.25)


# ------------------------------------------------------------------------------------------------ LayerNorm
@pytest.mark.parametrize("E,N", [(96, 70), (192, 70), (384, 70), (768, 70), (100, 70), (96, 4099), (768, 1031)])
def test_layernorm_fp16_with_residual_and_sample_scale(E, N):
    """y = res + s_b LN(x): the lanes-per-row kernels (stage widths) and the any-width one (E = 100), forward and backward."""
    B = 3
    M = B * N
    x32 = _bf(detfill.normalish((M, E), 11))
    r32 = _bf(detfill.normalish((M, E), 12))
    g = torch.from_numpy(1.0 + detfill.uniform((E,), 13, -0.3, 0.3)).float()
    b = torch.from_numpy(detfill.uniform((E,), 14, -0.3, 0.3)).float()
    ss = torch.tensor([0.0, 1.25, 1.25])
    w = torch.from_numpy(detfill.normalish((M, E), 15)).float()
    xr, rr = x32.clone().requires_grad_(True), r32.clone().requires_grad_(True)
    gr, br = g.clone().requires_grad_(True), b.clone().requires_grad_(True)
    ref = rr + ss.repeat_interleave(N)[:, None] * torch.nn.functional.layer_norm(xr, (E,), gr, br, 1e-5)
    (ref * w).sum().backward()
    errs = {k: {} for k in ("y", "dx", "dres", "dgamma", "dbeta")}
    for dt in DTS:
        xg = x32.to(DEV).to(dt).requires_grad_(True)
        rg_ = r32.to(DEV).to(dt).requires_grad_(True)
        gg, bb = g.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True)
        out = SW._LNFn.apply(xg, gg, bb, rg_, ss.to(DEV), N)
        assert out.dtype == dt
        (out.float() * w.to(DEV)).sum().backward()
        torch.cuda.synchronize()
        errs["y"][dt] = (out.float().cpu() - ref.detach()).abs().max().item()
        errs["dx"][dt] = _rel(xg.grad.float(), xr.grad)
        errs["dres"][dt] = _rel(rg_.grad.float(), rr.grad)
        errs["dgamma"][dt] = _rel(gg.grad, gr.grad)
        errs["dbeta"][dt] = _rel(bb.grad, br.grad)
    print(f"[layernorm E={E} rows={M}]")
    for k, e in errs.items():
        _check(e, k)


# ------------------------------------------------------------------------------------------------ embedding
def _embed(y, c, out_dt, B, H):
    Ay = torch.from_numpy(S.dct_np.conversion_matrix(4, 2)).float().to(DEV)
    Ac = torch.from_numpy(S.dct_np.conversion_matrix(2, 4)).float().to(DEV)
    out = torch.empty(B * 4 * H * H, 24, device=DEV, dtype=out_dt)
    L.check(L.lib().rgbnm_swin_embed(L.dt_of(y.dtype), L.dt_of(out_dt), y.data_ptr(), c.data_ptr(), Ay.data_ptr(), Ac.data_ptr(),
                                     out.data_ptr(), B, H, H, L.stream()), "swin_embed")
    torch.cuda.synchronize()
    return out


def test_swin_embed_fp16_output_is_the_fp32_output_rounded():
    B, H = 3, 6
    y = torch.from_numpy(detfill.normalish((B, 1, H, H, 8, 8), 5)).to(DEV)
    c = torch.from_numpy(detfill.normalish((B, 2, H // 2, H // 2, 8, 8), 6)).to(DEV)
    for in_dt in (torch.float32, torch.bfloat16, torch.float16):
        yi, ci = y.to(in_dt), c.to(in_dt)
        f32 = _embed(yi.float(), ci.float(), torch.float32, B, H)          # the input widened exactly: the fp32 path's bits
        f16 = _embed(yi, ci, torch.float16, B, H)
        assert torch.equal(f16.view(torch.int16), f32.half().view(torch.int16)), in_dt
    # fp16 input to fp32 / bf16 output: the fp32 input path on the same values
    yh, ch = y.half(), c.half()
    for out_dt in (torch.float32, torch.bfloat16):
        got = _embed(yh, ch, out_dt, B, H)
        want = _embed(yh.float(), ch.float(), out_dt, B, H)
        assert torch.equal(got.view(torch.int16) if out_dt != torch.float32 else got.view(torch.int32),
                           want.view(torch.int16) if out_dt != torch.float32 else want.view(torch.int32)), out_dt
    # Y and CbCr must share a dtype: the model refuses a mix
    with pytest.raises(TypeError):
        m = SW.SwinTransformerV2(img_size=128, embed_dim=96, depths=[2, 2, 2], num_heads=[3, 6, 12], window_size=8,
                                 device=DEV, pixel_space="dct")
        m(torch.zeros(1, 1, 16, 16, 8, 8, device=DEV, dtype=torch.float16), torch.zeros(1, 2, 8, 8, 8, 8, device=DEV))


# ------------------------------------------------------------------------------------------------ merge gather / token mean
def test_merge_gather_fp16_round_trip_is_bit_exact():
    B, res, C_ = 2, 16, 96
    bits = torch.randint(-32768, 32768, (B * res * res, C_), dtype=torch.int32, generator=torch.Generator().manual_seed(7))
    x = bits.to(torch.int16).view(torch.float16).to(DEV)          # every bit pattern: subnormals, infinities, NaN payloads
    out = torch.empty(B * (res // 2) ** 2, 4 * C_, device=DEV, dtype=torch.float16)
    L.check(L.lib().rgbnm_merge_gather(L.DT_F16, x.data_ptr(), out.data_ptr(), B, res, C_, 0, L.stream()), "merge_gather")
    back = torch.empty_like(x)
    L.check(L.lib().rgbnm_merge_gather(L.DT_F16, out.data_ptr(), back.data_ptr(), B, res, C_, 1, L.stream()), "merge_scatter")
    torch.cuda.synchronize()
    xi = x.view(torch.int16).reshape(B, res, res, C_)
    ref = torch.cat([xi[:, 0::2, 0::2], xi[:, 1::2, 0::2], xi[:, 0::2, 1::2], xi[:, 1::2, 1::2]], -1).reshape(-1, 4 * C_)
    assert torch.equal(out.view(torch.int16), ref)
    assert torch.equal(back.view(torch.int16), x.view(torch.int16))


def _ulp16(v):
    """one fp16 ulp at |v| (subnormal spacing below 2^-14)."""
    a = v.abs().float().clamp_min(2.0 ** -14)
    return torch.exp2(torch.floor(torch.log2(a)) - 10)


@pytest.mark.parametrize("N,C_", [(64, 768), (10, 16), (49, 96), (10, 12), (7, 3)])
def test_token_mean_fp16_within_one_ulp(N, C_):
    """C % 8 == 0: the 16-byte-vector kernels; otherwise the scalar ones.  fp32 sums, one rounding."""
    B = 3
    x = _bf(detfill.normalish((B * N, C_), 31)).to(DEV).half()
    out = torch.empty(B, C_, device=DEV, dtype=torch.float16)
    L.check(L.lib().rgbnm_token_mean(L.DT_F16, x.data_ptr(), out.data_ptr(), B, N, C_, 0, L.stream()), "token_mean")
    ref = x.float().reshape(B, N, C_).double().mean(1).float().half()
    dy = _bf(detfill.normalish((B, C_), 32)).to(DEV).half()
    dx = torch.empty(B * N, C_, device=DEV, dtype=torch.float16)
    L.check(L.lib().rgbnm_token_mean(L.DT_F16, dy.data_ptr(), dx.data_ptr(), B, N, C_, 1, L.stream()), "token_mean_bwd")
    torch.cuda.synchronize()
    dref = (dy.float() / N).half().repeat_interleave(N, 0)
    assert ((out.float() - ref.float()).abs() <= _ulp16(ref)).all()
    assert ((dx.float() - dref.float()).abs() <= _ulp16(dref)).all()
