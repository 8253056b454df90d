"""fp64 references and per-element bounds of ONE encoder block, stage by stage (a plain module, imported by name from
tests/test_block_edges.py and tests/test_block_edges_cpu.py; reference: TransformerEncoderBlock, models/plainvit.py:493-529).

Design: every tensor a path writes is checked against the fp64 result of that ONE stage applied to the tensors the same run
stored upstream.  Rounding therefore never accumulates across stages -- each bound stays
    |got - ref| <= ulp_T(ref) + k u mag + named terms          (kernel_check.check_bound)
-- and a wrong upstream tensor is caught at its own stage.  For the one-launch forward this is exact, not an approximation:
csrc/vit_chain.hip keeps the residual stream as packed bf16 (`Rows xr`), LN1 / LN2 read the rounded values it also stores, and
q, k, v, the attention output, the LayerNorm outputs and gelu are rounded to bf16 where they are stored (its header, "Arithmetic
vs the per-operation path").  The one-launch backward hands du, d(x_mid), d(attention output) and d(qkv) on as the bf16 values it
stores (csrc/vit_chain_bwd.hip phases M, P, A, X).  tests/test_block_edges_cpu.py composes the stages in fp64 and reproduces
oracle/vit_torch's block and its autograd gradients to 1e-12: stage-local checks + that anchor = whole-block correctness.

Layouts: wqkv / bqkv are DE-INTERLEAVED (rows q | k | v, each heads x 64), as the kernels take them; the reference layout is
the interleaved '(h d qkv)' of plainvit.py:447 -- interleaved row of de-interleaved row n = QKV_ROWS[n].  Weight gradients are
checked in the reference layout.

Bounds reuse the terms derived in tests/test_kernel_edges.py for the same operations (its docstring: inter, GELU; ATTN_C and LN_C
are that file's constants, measured there on the per-operation kernels and NOT refitted here).  What the fused forms add:
- residual epilogue: the staged per-operation epilogues round acc + bias to bf16 before the residual (`inter`); the chain adds
  x + acc + bias in fp32 (vit_chain.hip proj / fc2 epilogues) and has no such term: inter=False is the tighter bound.  The
  one-launch BACKWARD keeps the per-operation arithmetic: du = bf16(bf16(dy . W2) * gelu') (vit_chain_bwd.hip:506,
  `(bf16)((float)(bf16)a1[..] * (float)gpv[j])`, the body of mlp_bwd_kernel), so du carries `inter` on every path.
- fp16 underflow (the generic composites in fp16 only; 2^-133 in bf16): P and dS are rounded to the element type before the
  second products of the attention backward, with an ABSOLUTE error of up to 2^(emin - p) = 2^-24 where they are subnormal --
  near one-hot rows are full of such weights.  Summed like the gradient itself: + 2^-24 scale sum_j |k_jd| (dq),
  + 2^-24 scale sum_i |q_id| (dk), + 2^-24 sum_i |dO_id| (dv).
- LayerNorm backward behind a GEMM (ln_bwd_rows.h `Cs`: the GEMM result is rounded to bf16 in the LDS staging tile before
  the LayerNorm backward reads it): the backward is linear in that operand, so |delta_j| <= ulp_bf16(dxn_j) + K u mag_j (the bound
  of the GEMM element itself) is propagated through it in fp64:
      row i:  rstd (|g_i delta_i| + mean_j |g_j delta_j| + |xh_i| mean_j |g_j delta_j xh_j|),
  and the same delta enters the dgamma / dbeta sums: sum_t delta_tj |xh_tj| and sum_t delta_tj.
- logit error (logit=True, the cases built with make_params(offset=...) only): logit_err below, through the softmax and through
  P = exp(S - lse) / dS of the backward; derived in tests/regime_ref.py.  Every other case keeps the bounds it had.
- table GELU: the table holds the library's own GELU arithmetic for every bf16 input, so the GELU terms apply unchanged; the
  documented exception (bf16-denormal pre-activations) is excluded by the inputs: no |pre| below 2^-120 (asserted, no mask).
"""
import math

import numpy as np
import torch

import kernel_check as KC
from kernel_check import U, ulp, check_bound
from rgb_no_more_amd import detfill

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
E, HEADS, NTOK, INNER, HID, NPAD = 192, 3, 196, 192, 768, 224
EPS = 1e-5
SCALE = 1.0 / math.sqrt(E)            # plainvit.py:455: softmax(q k^T / sqrt(emb_size))
SQRT1_2 = 1.0 / math.sqrt(2.0)
# tests/test_kernel_edges.py (measured there, twice the worst of the per-operation kernels)
ATTN_C = {"out": 2.5, "lse": 0.13, "dq": 1.0, "dk": 2.0, "dv": 4.6}
# lse is held to ATTN_C["lse"] u lmag PLUS a = 2 fp32 ulps of the result here, where tests/test_kernel_edges.py uses a = 0 for the
# same per-operation kernels: its inputs (std 1.5 everywhere) keep lmag large, these have flat rows where lmag ~ |lse| + 1 and the
# roundings at the size of the result show -- mx * scale, the hardware log2 times ln 2, the final add: three roundings, bound 2 ulps.
# A reference-side term (the number format, not a kernel); measured on the MI355X: 1.7 fp32 ulps on such rows [a = 2]; the whole
# lse bound is met at 0.55 (one-launch) / 0.58 (per-operation), i.e. it is 1.7 times the worst measured.
# Worst |err| / bound measured there with the constants below, one-launch | per-operation: attention output 0.40 | 0.51,
# dq 0.32 | 0.33, dk 0.22 | 0.35, dv 0.35 | 0.29 (fp16 with its subnormal term included), LayerNorm y 0.50, statistics 0.03 | 0.01,
# dx 0.54 | 0.51 (with the staging-tile term), du 0.50 | 0.50 (with `inter`), per-image parts 0.25, dW 0.015, db 0.013.
LSE_ULPS = 2
LN_C = {"y": 1.2, "stat": 1.4, "dx": 1.3}
DENORMAL_FREE = 2.0 ** -120

# the cases of tests/test_block_edges.py (B "cu" / "cu+1" = the device's CU count / CU count + 1, resolved on the GPU)
CHAIN_B = (1, 2, "cu", "cu+1", 300)
CHAIN_DEPTHS = (1, 2, 12)
CHAIN_CASES = [(1, 1), (2, 1), ("cu", 1), ("cu+1", 1), (300, 1), (1, 2), (2, 2), ("cu", 2), ("cu+1", 2), (300, 2), (1, 12),
               (2, 12), (300, 12), (16, 1), (16, 2), (16, 12)]  # (B, depth); the large B x depth 12 product is one case.  (16, 12): 196 B tokens are a
#                                      multiple of 64 only for B % 16 == 0 -- the grouped weight-gradient launch with n = 12; (16, 1)
#                                      and (16, 2): its 12- and 6-way token splits at 3136 tokens, where the (M + 2) u mag bound is
#                                      sixteen times sharper than at B = 256 (four missing tokens are 1.3e-3 of the sum)
DW_N = (1, 2, 12)


def resolve_b(b, cus=256):
    """cus defaults to the MI355X's 256 CUs for the CPU file.  Its assertion that every n of DW_N reaches the grouped launch
    through "cu" holds for CU counts that are multiples of 16 (196 B % 64 == 0); the B = 16 cases reach it on any device."""
    return cus if b == "cu" else cus + 1 if b == "cu+1" else b


def qkv_rows(heads=HEADS):
    """interleaved '(h d qkv)' row of de-interleaved row n = s * inner + h * 64 + d  ->  h * 192 + d * 3 + s."""
    n = torch.arange(3 * heads * 64)
    inner = heads * 64
    s, rem = n // inner, n % inner
    return (rem // 64) * 192 + (rem % 64) * 3 + s


# ------------------------------------------------------------------------------------------------------------------ inputs
def _n(shape, seed, scale=1.0):
    return torch.from_numpy(detfill.normalish(tuple(shape), seed)) * scale


def offset_k0(scale):
    """b of the large-|lse| regime (tests/regime_ref.py): the smallest power of two with 32 b scale >= 90 (90 <= 32 b scale <= 180)."""
    b = 2.0 ** math.ceil(math.log2(90.0 / (32.0 * scale)))
    assert 90.0 <= 32.0 * b * scale <= 180.0
    return b


def make_params(depth, seed=1, e=E, heads=HEADS, offset=None):
    """Block parameters on the CPU: bf16 weights (de-interleaved qkv), fp32 biases and LayerNorm parameters.  Regimes, each block:
    head 0's q and k rows x 4 (logit spread >> ln 196: near one-hot attention rows); fc1 biases 0..7 = -24, 8..15 = +10 (the GELU
    table's negative and positive tails -- measured ends on the MI355X: -16 and 4 --; the rest sits in its window).
    offset (None, +1 or -1): row d = 0 of every head's q and k weight is zero and the biases there are 32 and +-b (offset_k0), so
    q[:, 0] = 32 and k[:, 0] = +-b in every head, exactly: every logit, and lse, carries 32 b scale = +-90 .. 180 scaled units."""
    out = []
    for i in range(depth):
        s = 1000 * seed + 40 * i
        inner, hid, sw = heads * 64, 4 * e, 0.07 * math.sqrt(E / e)          # (weights: std 0.97 / sqrt(fan-in))
        wqkv = _n((3 * inner, e), s + 5, sw)
        wqkv[0:64] *= 4.0
        wqkv[inner:inner + 64] *= 4.0
        bqkv = _n((3 * inner,), s + 6, 0.2)
        if offset is not None:
            d0 = torch.arange(heads) * 64
            wqkv[d0] = 0.0
            wqkv[inner + d0] = 0.0
            bqkv[d0] = 32.0
            bqkv[inner + d0] = offset * offset_k0(1.0 / math.sqrt(e))
        b1 = _n((hid,), s + 10, 0.2)
        b1[0:8] = -24.0
        b1[8:16] = 10.0
        out.append(dict(ln1_g=1 + _n((e,), s + 1, 0.2), ln1_b=_n((e,), s + 2, 0.2), ln2_g=1 + _n((e,), s + 3, 0.2),
                        ln2_b=_n((e,), s + 4, 0.2), wqkv=wqkv.to(BF16), bqkv=bqkv,
                        wproj=_n((e, inner), s + 7, 0.07 * math.sqrt(E / inner)).to(BF16), bproj=_n((e,), s + 8, 0.2),
                        w1=_n((hid, e), s + 9, sw).to(BF16), b1=b1, w2=_n((e, hid), s + 11, 0.04 * math.sqrt(E / e)).to(BF16),
                        b2=_n((e,), s + 12, 0.2)))
    return out


CONST_ROWS = (5, 195)       # tokens of every image whose residual row is near-constant (rstd ~ eps^-1/2)


def make_x0(B, seed=1, e=E):
    """Residual stream at the scale of deep blocks (std 3), bf16 [B * 196, 192]; tokens CONST_ROWS of every image are 2.0 with a few
    elements one bf16 ulp up: variance << eps."""
    x = _n((B * NTOK, e), 7000 + seed, 3.0)
    bump = _n((B * len(CONST_ROWS), e), 7100 + seed) > 2.5
    rows = torch.cat([torch.arange(B) * NTOK + t for t in CONST_ROWS])
    x[rows] = 2.0 + bump.float() * 2.0 ** -6
    return x.to(BF16)


def make_dy(B, seed=1, e=E):
    return _n((B * NTOK, e), 7200 + seed, 1.0).to(BF16)


def make_feat(B, seed=1):
    return _n((B * NTOK, 384), 7300 + seed, 1.0).to(BF16)


# ------------------------------------------------------------------------------------------------ fp64 stage references
def gelu64(x):
    return 0.5 * x * (1.0 + torch.special.erf(x * SQRT1_2))


def dgelu64(x):
    return 0.5 * (1.0 + torch.special.erf(x * SQRT1_2)) + x * torch.exp(-0.5 * x * x) / math.sqrt(2 * math.pi)


def ln_fwd(x, g, b, eps=EPS):
    """x [M, E] fp64 -> dict(y, ymag, mean, rstd, meanmag)."""
    mu = x.mean(1, keepdim=True)
    rs = 1.0 / torch.sqrt(((x - mu) ** 2).mean(1, keepdim=True) + eps)
    xh = (x - mu) * rs
    return dict(y=xh * g + b, ymag=g.abs() * (xh.abs() + rs * x.abs().mean(1, keepdim=True)) + b.abs(), mean=mu[:, 0],
                rstd=rs[:, 0], meanmag=x.abs().mean(1))


def linear(x, w, b=None):
    """(x w^T + b, the same on absolute values)."""
    ref, mag = x @ w.T, x.abs() @ w.abs().T
    if b is not None:
        ref, mag = ref + b, mag + b.abs()
    return ref, mag


def _heads(t, B, k=1):                              # [B * N, k * I] -> k tensors [B, H, N, 64]
    I = t.shape[1] // k
    return [t[:, i * I:(i + 1) * I].reshape(B, -1, I // 64, 64).permute(0, 2, 1, 3) for i in range(k)]


def _flat(t):                                       # [B, H, N, 64] -> [B * N, I]
    return t.permute(0, 2, 1, 3).reshape(-1, t.shape[1] * 64)


LOGIT_C = 64        # fp32 roundings a term of the 64-term score accumulation can meet (tests/regime_ref.py, C_D)


def logit_err(S, A, lse):
    """|error| of a kernel's scaled logit, per element (tests/regime_ref.py derives it): LOGIT_C u scale |q|.|k| + 4 u (|S| + |lse|);
    A = scale |q| |k|^T.  At unit-scale logits it is far below u_P; with a common offset of +-100 .. 150 it is the error."""
    return LOGIT_C * U * A + 4 * U * (S.abs() + lse.abs()[..., None])


def attn_fwd(qkv, B, scale=SCALE, logit=False):
    """qkv [B * N, 3 I] fp64 -> dict(out, outmag [B * N, I]; lse, lsemag [B, H, N]; pmax [B, H, N]).  logit: also the logit error
    through the softmax, out_logit = (P o e)|v| + (sum_j P e) P|v| and lse_logit = sum_j P e."""
    q, k, v = _heads(qkv, B, 3)
    S = (q @ k.transpose(-1, -2)) * scale
    lse = torch.logsumexp(S, -1)
    P = torch.exp(S - lse[..., None])
    A = scale * (q.abs() @ k.abs().transpose(-1, -2))
    lmag = A.amax(-1) * 64 + lse.abs() + 1
    r = dict(out=_flat(P @ v), outmag=_flat(P @ v.abs()), lse=lse, lsemag=lmag, pmax=P.amax(-1), out_logit=None, lse_logit=None)
    if logit:
        Pe = P * logit_err(S, A, lse)
        spe = Pe.sum(-1, keepdim=True)
        r["out_logit"], r["lse_logit"] = _flat(Pe @ v.abs() + spe * (P @ v.abs())), spe[..., 0]
    return r


def attn_bwd(qkv, attn, dattn, lse, B, scale=SCALE, delta=None, logit=False):
    """From the STORED qkv, attention output, its gradient and lse [B, H, N]: dict(dq, dk, dv: (ref, mag, prop) each [B * N, I]).
    delta (|error| of every dattn element, or None): the backward is linear in dattn, so prop = the same sums on |delta|.
    logit: out["logit"] = the logit error through P = exp(S - lse) and dS = P (dP - D), summed like the gradients."""
    q, k, v = _heads(qkv, B, 3)
    S = (q @ k.transpose(-1, -2)) * scale
    P = torch.exp(S - lse[..., None])
    dO, O = _heads(dattn, B)[0], _heads(attn, B)[0]
    D = (dO * O).sum(-1, keepdim=True)
    dS = P * (dO @ v.transpose(-1, -2) - D)
    mD = (dO.abs() * (P @ v.abs())).sum(-1, keepdim=True)
    mdS = P * (dO.abs() @ v.abs().transpose(-1, -2) + mD)
    Pt = P.transpose(-1, -2)
    out = dict(dq=[_flat(scale * dS @ k), _flat(scale * mdS @ k.abs()), None],
               dk=[_flat(scale * dS.transpose(-1, -2) @ q), _flat(scale * mdS.transpose(-1, -2) @ q.abs()), None],
               dv=[_flat(Pt @ dO), _flat(Pt @ dO.abs()), None])
    tok = lambda t: _flat(t.abs().sum(2, keepdim=True).expand_as(t))           # noqa: E731  (sums over the image's tokens)
    out["under"] = dict(dq=scale * tok(k), dk=scale * tok(q), dv=tok(dO))
    out["logit"] = None
    if logit:
        Pe = P * logit_err(S, scale * (q.abs() @ k.abs().transpose(-1, -2)), lse)
        EdS = Pe * (dO @ v.transpose(-1, -2) - D).abs()
        out["logit"] = dict(dq=_flat(scale * EdS @ k.abs()), dk=_flat(scale * EdS.transpose(-1, -2) @ q.abs()),
                            dv=_flat(Pe.transpose(-1, -2) @ dO.abs()))
    if delta is not None:
        dl = _heads(delta, B)[0]
        pdS = P * (dl @ v.abs().transpose(-1, -2) + (dl * O.abs()).sum(-1, keepdim=True))
        out["dq"][2], out["dk"][2] = _flat(scale * pdS @ k.abs()), _flat(scale * pdS.transpose(-1, -2) @ q.abs())
        out["dv"][2] = _flat(Pt @ dl)
    return out


def ln_bwd(dxn, x, mean, rstd, g, res, delta=None, ntok=NTOK):
    """LayerNorm backward w.r.t. x (saved mean / rstd [M]) + residual gradient.  dict(dx, dxmag, prop: the propagated |delta| or None,
    dgamma, dbeta and their mags / delta terms per image [B, E])."""
    mu, rs = mean[:, None], rstd[:, None]
    xh = (x - mu) * rs
    gv = dxn * g
    dx = rs * (gv - gv.mean(1, keepdim=True) - xh * (gv * xh).mean(1, keepdim=True)) + res
    mag = rs * (gv.abs() + gv.abs().mean(1, keepdim=True) + xh.abs() * (gv * xh).abs().mean(1, keepdim=True)) + res.abs()
    img = lambda t: t.reshape(-1, ntok, t.shape[1]).sum(1)            # noqa: E731
    out = dict(dx=dx, dxmag=mag, dgamma=img(dxn * xh), dgmag=img((dxn * xh).abs()), dbeta=img(dxn), dbmag=img(dxn.abs()),
               prop=None, dgprop=None, dbprop=None)
    if delta is not None:
        gd = g.abs() * delta
        out["prop"] = rs * (gd + gd.mean(1, keepdim=True) + xh.abs() * (gd * xh.abs()).mean(1, keepdim=True))
        out["dgprop"], out["dbprop"] = img(delta * xh.abs()), img(delta)
    return out


def tn(dy, x):
    """dW = dy^T x, db = column sums of dy, and the same on absolute values."""
    return dy.T @ x, dy.abs().T @ x.abs(), dy.sum(0), dy.abs().sum(0)


# ----------------------------------------------------------------------------------------------------------------- checks
def _tail(t, B):
    """tokens 192 .. 195 of every image (the seventh wave of the chain kernels owns only these four)."""
    return t.reshape(B, NTOK, -1)[:, 192:]


def _chk(worst, key, got, ref, mag, c_u, where, extra=None, B=None, tile=None):
    """Element type = got's own (bf16 on the fast paths; the generic composites also run in fp16 and fp32)."""
    dt = got.dtype
    r = _cb(worst, key, got, ref, mag, dt, 1, c_u, f"{where} {key}", extra=extra, tile=tile)
    if B is not None:               # stated on its own: the last four tokens of every image are written and in bound
        ex = _tail(extra, B) if torch.is_tensor(extra) else extra
        _cb(worst, key + "[192:196]", _tail(got, B), _tail(ref, B), _tail(mag, B), dt, 1, c_u, f"{where} {key} tokens 192..195",
            extra=ex)
    return r


def _cb(worst, key, *args, **kw):
    """check_bound into worst[key].  A Worst with an `errors` list collects the violations (the GPU test reports every stage of a
    case, then fails); without one the first violation raises."""
    try:
        return worst(key, check_bound(*args, **kw))
    except AssertionError as e:
        if getattr(worst, "errors", None) is None:
            raise
        worst.errors.append(str(e)[:700])
        return worst(key, math.inf)


def d64(t):
    return t.double()


def tiny(dt):
    """spacing of the subnormals of the element type: 2^(emin - p)"""
    p, emin = KC._FMT[dt]
    return 2.0 ** (emin - p)


def u_p(dt, N=NTOK):
    """unit roundoff of P before P . V (tests/test_kernel_edges.py attn_case): the 16-bit types round P, fp32 sums N terms."""
    return KC.U_OF[dt] if dt != F32 else N * U


def check_ln_fwd(worst, key, where, x, g, b, y, mean, rstd, B=None):
    r = ln_fwd(d64(x), d64(g), d64(b))
    e = x.shape[1]
    _chk(worst, key, y, r["y"], r["ymag"], LN_C["y"] * e * U, where, B=B, tile=(32, e))
    _chk(worst, key + "-stat", mean, r["mean"], r["meanmag"], LN_C["stat"] * e * U, where + " mean")
    _chk(worst, key + "-stat", rstd, r["rstd"], r["rstd"], LN_C["stat"] * e * U, where + " rstd")
    return r


def check_res(worst, key, where, a, w, b, res, got, inter, B=None, f=None):
    """got = res + a w^T + b.  inter: the staged 16-bit epilogues round a w^T + b to the element type first.
    f (fp64 [M, N], keep . scale of the dropout site, or None): got = res + f (a w^T + b), the terms of
    tests/test_dropout_kernels.py nt_drop_case -- the mask multiplies the staged value (f inter) and the product is rounded to fp32
    once more (gemm.hip epilogue, `drop_one`: v * d.scale in fp32): + 2 fp32 ulps of f pre."""
    pre, mag = linear(d64(a), d64(w), d64(b))
    extra = ulp(pre, got.dtype) if inter and got.dtype != F32 else None
    if f is not None:
        extra = 2 * ulp(f * pre, F32) + (f * extra if extra is not None else 0.0)
        pre, mag = f * pre, f * mag
    _chk(worst, key, got, pre + d64(res), mag + d64(res).abs(), a.shape[1] * U, where, extra=extra, B=B, tile=(32, got.shape[1]))


def check_gelu(worst, where, xn2, w1, b1, gl, u, B=None, f=None):
    """f (fp64 [M, 4 E], keep . scale of site 1, or None): gl = f gelu(pre), u = f gelu'(pre) with nt_drop_case's terms: every
    term of the unmasked bound times f, and 2 more fp32 ulps of the result for the product with the scale."""
    pre, mag = linear(d64(xn2), d64(w1), d64(b1))
    tiny = float(pre.abs().min())
    assert tiny >= DENORMAL_FREE, f"{where}: a pre-activation of magnitude {tiny:.3g} (the table's documented exception)"
    up = ulp(pre, gl.dtype)
    K = xn2.shape[1]
    ref, ref2 = gelu64(pre), dgelu64(pre)
    if f is not None:
        if gl.dtype == F32:
            up = 0.0                      # (nt_drop_case: the pre-activation is rounded to T in the 16-bit modes only)
        ref, ref2 = f * ref, f * ref2
        _chk(worst, "gl", gl, ref, 1.13 * f * mag, K * U, where, extra=f * (1.13 * up + 2.0 ** -22 * pre.abs()) + 4 * ulp(ref, F32),
             B=B, tile=(32, 64))
        _chk(worst, "u", u, ref2, 0.8 * f * mag, K * U, where, extra=f * (0.8 * up + 2.0 ** -21) + 4 * ulp(ref2, F32), B=B,
             tile=(32, 64))
        return pre
    _chk(worst, "gl", gl, ref, 1.13 * mag, K * U, where, extra=1.13 * up + 2.0 ** -22 * pre.abs() + 2 * ulp(ref, F32), B=B,
         tile=(32, 64))
    _chk(worst, "u", u, ref2, 0.8 * mag, K * U, where, extra=0.8 * up + 2.0 ** -21 + 2 * ulp(ref2, F32), B=B, tile=(32, 64))
    return pre


def check_attn_fwd(worst, where, qkv, attn, lse, B, scale=SCALE, logit=False):
    r = attn_fwd(d64(qkv), B, scale, logit)
    _chk(worst, "attn", attn, r["out"], r["outmag"], ATTN_C["out"] * u_p(attn.dtype), where, extra=r["out_logit"], B=B, tile=(NTOK, 64))
    # lse = mx * scale + __logf(sum) (vit_chain.hip:697; attention_v2.hip alike): LSE_ULPS above
    _cb(worst, "lse", lse.reshape(r["lse"].shape), r["lse"], r["lsemag"], F32, LSE_ULPS, ATTN_C["lse"] * U, where + " lse",
        extra=r["lse_logit"])
    return r


def check_block_fwd(worst, where, P, A, B, inter=False, nxt=None, f=None, logit=False):
    """Stages 1 - 7 (8 with nxt = (next block's parameters, its xn1 / mean1 / rstd1 dict)) of one block, each from the tensors
    the run itself stored.  P, A: dicts of tensors on one device.  Returns what the regime assertions need.
    f: None, or the dropout factors {0: [M, E], 1: [M, 4 E], 2: [M, E]} (fp64, keep . scale) of rgbnm_vit_block_fwd_drop."""
    f = f or {}
    info = {}
    r = check_ln_fwd(worst, "xn1", where, A["x_in"], P["ln1_g"], P["ln1_b"], A["xn1"], A["mean1"], A["rstd1"], B)
    info["rstd1_max"] = float(r["rstd"].max())
    ref, mag = linear(d64(A["xn1"]), d64(P["wqkv"]), d64(P["bqkv"]))
    e = A["x_in"].shape[1]
    _chk(worst, "qkv", A["qkv"], ref, mag, e * U, where, B=B, tile=(32, 64))
    r = check_attn_fwd(worst, where, A["qkv"], A["attn"], A["lse"], B, 1.0 / math.sqrt(e), logit)
    info["onehot_rows"] = int((r["pmax"] > 0.9).sum())
    info["lse_absmin"] = float(r["lse"].abs().min())
    del r, ref, mag
    check_res(worst, "x_mid", where, A["attn"], P["wproj"], P["bproj"], A["x_in"], A["x_mid"], inter, B, f.get(0))
    check_ln_fwd(worst, "xn2", where, A["x_mid"], P["ln2_g"], P["ln2_b"], A["xn2"], A["mean2"], A["rstd2"], B)
    info["pre"] = check_gelu(worst, where, A["xn2"], P["w1"], P["b1"], A["gl"], A["u"], B, f.get(1))
    check_res(worst, "x_out", where, A["gl"], P["w2"], P["b2"], A["x_mid"], A["x_out"], inter, B, f.get(2))
    if nxt is not None:
        check_ln_fwd(worst, "next-xn1", where, A["x_out"], nxt[0]["ln1_g"], nxt[0]["ln1_b"], nxt[1]["xn1"], nxt[1]["mean1"],
                     nxt[1]["rstd1"], B)
    return info


def gemm_bound(ref, mag, K, dt=BF16):
    return ulp(ref, dt) + K * U * mag


def check_lnbwd_fused(worst, key, where, a, wt, x, mean, rstd, g, res, dx, part, B):
    """dx = res + LN'(a wt) with a wt rounded to the element type on its way (ln_bwd_rows.h; the generic composites store it
    as dxn in between: the same arithmetic); part [B, 2, E] = per-image dgamma | dbeta."""
    dxn, dmag = d64(a) @ d64(wt), d64(a).abs() @ d64(wt).abs()
    K, e = a.shape[1], x.shape[1]
    delta = gemm_bound(dxn, dmag, K, dx.dtype)
    r = ln_bwd(dxn, d64(x), d64(mean), d64(rstd), d64(g), d64(res), delta)
    _chk(worst, key, dx, r["dx"], r["dxmag"], LN_C["dx"] * e * U, where, extra=r["prop"], B=B, tile=(32, e))
    if part is not None:
        cu = (NTOK + e) * U
        _cb(worst, key + "-part", part[:, 0], r["dgamma"], r["dgmag"], F32, 1, cu, f"{where} {key} part dgamma",
            extra=r["dgprop"])
        _cb(worst, key + "-part", part[:, 1], r["dbeta"], r["dbmag"], F32, 1, cu, f"{where} {key} part dbeta",
            extra=r["dbprop"])
    return r


def check_block_bwd(worst, where, P, A, G, B, logit=False):
    """Backward stages 1 - 6a of one block on the fused forms (one-launch backward / per-operation fused path): G holds dy, du,
    dx_mid, dattn (None: its scratch was reused), dqkv, dx and part2 / part1 ([B, 2, E], None: not checked here).
    The dropout backward (vit.hip block_bwd with d) adds dy_m and dxmid_m: the GEMM operands of du and dattn; the two residuals
    stay G["dy"] and G["dx_mid"]."""
    dy = d64(G["dy_m"] if G.get("dy_m") is not None else G["dy"])
    pre, mag = dy @ d64(P["w2"]), dy.abs() @ d64(P["w2"]).abs()
    uu = d64(A["u"])
    dt, e, inner = G["du"].dtype, dy.shape[1], A["attn"].shape[1]
    _chk(worst, "du", G["du"], pre * uu, mag * uu.abs(), e * U, where,
         extra=ulp(pre, dt) * uu.abs() if dt != F32 else None, B=B, tile=(32, 64))
    del pre, mag, uu
    r2 = check_lnbwd_fused(worst, "dx_mid", where, G["du"], P["w1"], A["x_mid"], A["mean2"], A["rstd2"], P["ln2_g"], G["dy"],
                           G["dx_mid"], G.get("part2"), B)
    r2 = {k: v for k, v in r2.items() if k.startswith(("dg", "db"))}
    dxm = d64(G["dxmid_m"] if G.get("dxmid_m") is not None else G["dx_mid"])
    ref, mag = dxm @ d64(P["wproj"]), dxm.abs() @ d64(P["wproj"]).abs()
    del dxm
    delta = None
    if G.get("dattn") is not None:
        _chk(worst, "dattn", G["dattn"], ref, mag, e * U, where, B=B, tile=(32, 64))
        ref = d64(G["dattn"])
    else:       # the scratch has been reused by an earlier block: d(qkv) from the fp64 d(attention output), its GEMM bound propagated
        delta = gemm_bound(ref, mag, e, dt)
    r = attn_bwd(d64(A["qkv"]), d64(A["attn"]), ref, d64(A["lse"]).reshape(B, inner // 64, NTOK), B, 1.0 / math.sqrt(e), delta, logit)
    del ref, mag, delta
    for i, nm in enumerate(("dq", "dk", "dv")):
        extra = tiny(dt) * r["under"][nm] + (r[nm][2] if r[nm][2] is not None else 0.0) + (r["logit"][nm] if logit else 0.0)
        _chk(worst, nm, G["dqkv"][:, i * inner:(i + 1) * inner], r[nm][0], r[nm][1], ATTN_C[nm] * u_p(dt), where, extra=extra,
             B=B, tile=(NTOK, 64))
    del r
    r1 = check_lnbwd_fused(worst, "dx", where, G["dqkv"], P["wqkv"], A["x_in"], A["mean1"], A["rstd1"], P["ln1_g"], G["dx_mid"],
                           G["dx"], G.get("part1"), B)
    return r2, {k: v for k, v in r1.items() if k.startswith(("dg", "db"))}


def check_dln_total(worst, where, r2, r1, W, B):
    """The per-operation paths reduce the LayerNorm parameter gradients over row panels, not images: dln*_g / dln*_b against the
    fp64 sums over all tokens, with the staging tile's delta summed like the gradient itself (r2, r1: check_block_bwd's)."""
    cu = (B * NTOK + W["dln1_g"].shape[0]) * U
    for ln, r in (("dln2", r2), ("dln1", r1)):
        _cb(worst, ln, W[ln + "_g"], r["dgamma"].sum(0), r["dgmag"].sum(0), F32, 1, cu, f"{where} {ln}_g", extra=r["dgprop"].sum(0))
        _cb(worst, ln, W[ln + "_b"], r["dbeta"].sum(0), r["dbmag"].sum(0), F32, 1, cu, f"{where} {ln}_b", extra=r["dbprop"].sum(0))


DW_NAMES = ("dln1_g", "dln1_b", "dln2_g", "dln2_b", "dwqkv", "dbqkv", "dwproj", "dbproj", "dw1", "db1", "dw2", "db2")


def check_block_dw(worst, where, A, G, W, B):
    """Backward stages 6b, 7: the twelve parameter gradients W (fp32, reference layouts) from the stored operands.  The LayerNorm
    parameter gradients are the sums over images of the STORED part2 / part1."""
    M = B * NTOK
    cu = (M + 2) * U
    dyg = G["dy_m"] if G.get("dy_m") is not None else G["dy"]                    # (the dropout backward's masked operands)
    dxmg = G["dxmid_m"] if G.get("dxmid_m") is not None else G["dx_mid"]
    for key, dyk, xk, perm in (("dw2", dyg, A["gl"], False), ("dw1", G["du"], A["xn2"], False),
                               ("dwproj", dxmg, A["attn"], False), ("dwqkv", G["dqkv"], A["xn1"], True)):
        ref, mag, rb, mb = tn(d64(dyk), d64(xk))
        if perm:
            dst = qkv_rows(ref.shape[0] // 192).to(ref.device)
            for t in (ref, mag, rb, mb):
                t[dst] = t.clone()
        _cb(worst, key, W[key], ref, mag, F32, 1, cu, f"{where} {key}", tile=(128, 192))
        _cb(worst, "db" + key[2:], W["db" + key[2:]], rb, mb, F32, 1, cu, f"{where} db{key[2:]}")
    for ln, part in (("dln2", G.get("part2")), ("dln1", G.get("part1"))):
        if part is None:
            continue                # the per-operation paths: check_dln_total
        p = d64(part)
        for j, nm in enumerate(("_g", "_b")):
            _cb(worst, ln, W[ln + nm], p[:, j].sum(0), p[:, j].abs().sum(0), F32, 1, (B + 2) * U, f"{where} {ln}{nm}")


def check_pe_dw(worst, where, dx0, feat, pe_dw, pe_db, B):
    ref, mag, rb, mb = tn(d64(dx0), d64(feat))
    cu = (B * NTOK + 2) * U
    _cb(worst, "pe_dw", pe_dw, ref, mag, F32, 1, cu, f"{where} pe_dw", tile=(128, 192))
    _cb(worst, "pe_db", pe_db, rb, mb, F32, 1, cu, f"{where} pe_db")


# ------------------------------------------------------------------ torch emulations of the paths' rounding points (fp32 / bf16)
def _f(t):
    return t.float()


def _b(t):
    return t.to(BF16)


def emu_ln(x, g, b):
    xf = _f(x)
    mu = xf.mean(1, keepdim=True)
    rs = torch.rsqrt(((xf - mu) ** 2).mean(1, keepdim=True) + EPS)
    return _b((xf - mu) * rs * g + b), mu[:, 0].clone(), rs[:, 0].clone()


def emu_attn_fwd(qkv, B, scale=SCALE):
    q, k, v = _heads(_f(qkv), B, 3)
    S = q @ k.transpose(-1, -2)
    mx = S.amax(-1, keepdim=True)
    p = torch.exp2((S - mx) * (scale * 1.4426950408889634))
    sm = p.sum(-1, keepdim=True)
    O = (_f(_b(p)) @ v) / sm                                       # P rounded to bf16 for P . V, the sum taken before
    return _b(_flat(O)), (mx * scale + torch.log(sm))[..., 0].contiguous()


def emu_block_fwd(P, x_in, B, path="chain", pad_key_weight=0.0, half_dgelu_tail=False):
    """path 'chain': residual added on the fp32 accumulator (vit_chain.hip); 'staged': acc + bias rounded to bf16 in the LDS tile of
    the generic kernel's epilogue (gemm.hip pass 1 `store4<T>(Cs ...)`); 'fused': the row-panel kernel's residual + LayerNorm
    epilogue reads its bf16 staging tile the same way (gemm_nt_kpipe_body.inc:336 `(bf16)((float)c[i] + (float)lr[..])`;
    mlp_fwd_kernel uses that epilogue, mlp_fused.hip:24) -- the same rounding points, hence one branch below.
    The two keyword defects are seeded where they would arise (tests/test_block_edges_cpu.py)."""
    A = dict(x_in=x_in)
    A["xn1"], A["mean1"], A["rstd1"] = emu_ln(x_in, P["ln1_g"], P["ln1_b"])
    A["qkv"] = _b(_f(A["xn1"]) @ _f(P["wqkv"]).T + P["bqkv"])
    A["attn"], A["lse"] = emu_attn_fwd(A["qkv"], B, 1.0 / math.sqrt(x_in.shape[1]))
    if pad_key_weight:               # one padded key (row 196 of the K / V arrays: holds other data) given weight
        A["attn"] = _b(_f(A["attn"]) * (1 - pad_key_weight) + pad_key_weight * 1.0)

    def res(a, w, b, r):
        pre = _f(a) @ _f(w).T + b
        return _b(pre + _f(r)) if path == "chain" else _b(_f(_b(pre)) + _f(r))
    A["x_mid"] = res(A["attn"], P["wproj"], P["bproj"], x_in)
    A["xn2"], A["mean2"], A["rstd2"] = emu_ln(A["x_mid"], P["ln2_g"], P["ln2_b"])
    pre = _f(_b(_f(A["xn2"]) @ _f(P["w1"]).T + P["b1"]))
    A["gl"] = _b(0.5 * pre * (1 + torch.erf(pre * SQRT1_2)))
    up = 0.5 * (1 + torch.erf(pre * SQRT1_2)) + pre * torch.exp(-0.5 * pre * pre) * (1.0 / math.sqrt(2 * math.pi))
    if half_dgelu_tail:
        up = torch.where(pre < -16.0, torch.full_like(up, 0.5), up)
    A["u"] = _b(up)
    A["x_out"] = res(A["gl"], P["w2"], P["b2"], A["x_mid"])
    return A


def emu_lnbwd(a, wt, x, mean, rstd, g, res, B, rounded=True):
    dxn = _f(a) @ _f(wt)
    if rounded:
        dxn = _f(_b(dxn))
    xh = (_f(x) - mean[:, None]) * rstd[:, None]
    gv = dxn * g
    dx = rstd[:, None] * (gv - gv.mean(1, keepdim=True) - xh * (gv * xh).mean(1, keepdim=True)) + _f(res)
    part = torch.stack([(dxn * xh).reshape(B, NTOK, -1).sum(1), dxn.reshape(B, NTOK, -1).sum(1)], 1)
    return _b(dx), part


def emu_attn_bwd(A, dattn, B, e):
    """d(qkv) from the stored qkv / attention output / lse and d(attention output): P and dS rounded to bf16 before the second products."""
    q, k, v = _heads(_f(A["qkv"]), B, 3)
    dO, O = _heads(_f(dattn), B)[0], _heads(_f(A["attn"]), B)[0]
    scale = 1.0 / math.sqrt(e)
    Pm = torch.exp((q @ k.transpose(-1, -2)) * scale - A["lse"].reshape(B, -1, NTOK)[..., None])
    D = (dO * O).sum(-1, keepdim=True)
    dS = _f(_b(Pm * (dO @ v.transpose(-1, -2) - D)))
    Pb = _f(_b(Pm))
    return _b(torch.cat([_flat(scale * (dS @ k)), _flat(scale * (dS.transpose(-1, -2) @ q)), _flat(Pb.transpose(-1, -2) @ dO)], 1))


def emu_block_bwd(P, A, dy, B, rounded=True):
    G = dict(dy=dy)
    pre = _f(dy) @ _f(P["w2"])
    G["du"] = _b(_f(_b(pre)) * _f(A["u"]))                         # every path: vit_chain_bwd.hip:506 is mlp_bwd_kernel's body
    G["dx_mid"], G["part2"] = emu_lnbwd(G["du"], P["w1"], A["x_mid"], A["mean2"], A["rstd2"], P["ln2_g"], dy, B, rounded)
    G["dattn"] = _b(_f(G["dx_mid"]) @ _f(P["wproj"]))
    G["dqkv"] = emu_attn_bwd(A, G["dattn"], B, dy.shape[1])
    G["dx"], G["part1"] = emu_lnbwd(G["dqkv"], P["wqkv"], A["x_in"], A["mean1"], A["rstd1"], P["ln1_g"], G["dx_mid"], B, rounded)
    return G


def emu_block_dw(A, G):
    W = {}
    for key, dyk, xk in (("dw2", G["dy"], A["gl"]), ("dw1", G["du"], A["xn2"]), ("dwproj", G["dx_mid"], A["attn"]),
                         ("dwqkv", G["dqkv"], A["xn1"])):
        W[key], W["db" + key[2:]] = _f(dyk).T @ _f(xk), _f(dyk).sum(0)
    dst = qkv_rows(W["dbqkv"].shape[0] // 192)
    for k in ("dwqkv", "dbqkv"):
        t = torch.empty_like(W[k])
        t[dst] = W[k]
        W[k] = t
    for ln, part in (("dln2", G["part2"]), ("dln1", G["part1"])):
        W[ln + "_g"], W[ln + "_b"] = part[:, 0].sum(0), part[:, 1].sum(0)
    return W


# ------------------------------------------------------------------------------- Python copies of the launchers' arithmetic
def cdiv(a, b):
    return -(-a // b)


# the per-operation fused path (rgbnm_vit_block_fwd_chain / rgbnm_vit_block_bwd), batches its launchers' arithmetic makes sharp:
# 41 | 42: 196 B below / above 8192 rows (generic | fused kernels); 256 | 257: 196-row panels (table GELU) | 197 (arithmetic);
# 300: the 224-row cap, 263 panels, a 112-row last one; 586: 513 panels (rgbnm_launch_nt_kpipe_res_ln / _lnbwd use the same
# rows = min(cdiv(M, 256), 224) as rgbnm_launch_mlp_fwd).  fused_dx_lnbwd (vit.hip:122) checks its workspace for
# cdiv(M, cdiv(M, 512)) panels, "up to 512": 511 at this M, two fewer than the launcher writes.  Harmless only because the
# LayerNorm region of the block workspace holds max(cdiv(M, 16), 2048) panels (rgbnm_layernorm_bwd_workspace); the guarded
# workspace of this case shows that nothing is written past it
PEROP_B = (41, 42, 256, 257, 300, 586)


def mlp_fwd_panel_rows(M):
    """rgbnm_launch_mlp_fwd (csrc/mlp_fused.hip): rows of a panel, and whether the GELU table is used (up to 196 rows)."""
    rows = min(cdiv(M, 256), 224)
    return rows, rows <= 196
