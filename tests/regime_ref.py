"""Value regimes for the stand-alone attention and LayerNorm entries: CPU generators, the bound terms they need, the per-regime
element-wise checks and fp32 emulations with seeded defects (a plain module, imported by name from tests/test_value_regimes.py
(GPU) and tests/test_value_regimes_cpu.py; in the style of tests/block_ref.py).

Why: tests/test_kernel_edges.py walks shapes on unit-scale Gaussians only (attn_case: randn * 1.5, scaled logits of std 0.65 to
2.25, |lse| < 8; ln_case: 2 randn + 0.5).  A forward without max subtraction, padded keys masked with a finite sentinel, fp16
operands flushed below 2^-14 or a one-pass variance pass every such case.  Every tensor here comes from detfill.normalish, so the
CPU file and the GPU file see the same values.

Attention regimes, one per (image, head) pair: ATTN_REGIMES[(b H + h) % 5], so one call mixes them.
- flat:     attn_case's inputs (randn * 1.5), the control.
- peaked:   q and k of the pair times 4 (logit std 10 to 36 scaled units); query rows 0, 31, 32 and N - 1 also get a planted winning
            key, a copy of the query, at key 0, N - 1 (the last valid key of a ragged tile), 32 t - 1 and 32 t (t = (N - 1) // 32).
- offset+ / offset-:  q[:, 0] = 32 and k[:, 0] = +-b, b the smallest power of two with 32 b scale >= 90 (exact in bf16 and fp16): every
            logit carries a common offset of +-90 to +-180 scaled units while the spread stays that of `flat`.  exp of the unshifted
            logit overflows fp32 (+) or makes the row sum zero (-).
- small-v:  v and dO of the pair times 2^-16: fp16 subnormal operands and outputs (harmless in bf16 / fp32, still run there).

Bound terms beyond tests/test_kernel_edges.py's  ulp_T(ref) + ATTN_C u_P mag  (ATTN_C, LSE_ULPS and LN_C are block_ref's, unchanged):
- logit error  e_ij = C_D u scale (|q_i| . |k_j|) + 4 u (|S_ij| + |lse_i|).
  C_D = 64: the raw score is a 64-term fp32 MFMA accumulation (attention.hip score_tile `mma(acc, kf, qf[c])`, attention_v2.hip
  `mma(acc, rowfrag<E>(Ks ...), qf[c])`): each term meets at most 64 fp32 roundings on its way through the chained accumulator, the
  16-bit products themselves are exact in fp32 -- gamma_64 ~ 64 u on sum_d |q_d k_d| (tests/swin_ref.py logit_err: 32 u for d = 32).
  4 u (|S| + |lse|): the forward's (s - m) * scale, the multiplication by log2 e inside __expf and the hardware exp2
  (attention.hip `__expf((s[t][r] - m) * scale)`), or c2 = scale * log2 e, mc2 = m * c2 and the FMA (attention_v2.hip
  `exp2f(fmaf(acc[r], c2, -mc2))`); the backward's `__expf(sa[r] * scale - lq)`: four roundings at the size of |S| + |lse|.
  At |raw| ~ 2000 (the offset regimes) this term is what a correct kernel's error consists of; at unit scale it is below u_P mag.
- out:  + (P o e)|v| + (sum_j P e) P|v|   (first order of softmax(S + e) V; tests/swin_ref.py win_fwd).
- lse:  ATTN_C["lse"] u lmag + LSE_ULPS fp32 ulps (block_ref's form) + sum_j P e.
- backward, on the kernel's OWN out and lse (block_ref.check_block_bwd): P_k = exp(S - lse_k) carries e, so
  dS carries P_k e |dP - D|:  dq + scale (P_k e |dP - D|) |k|,  dk + scale (P_k e |dP - D|)^T |q|,  dv + (P_k e)^T |dO|.
- subnormals of T (eta_T = 2^(emin - p): 2^-24 in fp16, 2^-133 in bf16, 2^-149 in fp32): P and dS are rounded to T before their
  second products: block_ref's terms  eta scale sum_j |k_j| (dq), eta scale sum_i |q_i| (dk), eta sum_i |dO_i| (dv); the forward's
  normalised P (attention.hip `s[t][r] *= inv` then `pfrag<T>`): + eta sum_j |v_j|.  The fp16 attn2 / attn3 forward rounds
  2^14 exp2(s - max) instead (attention_v2.hip PShift) and divides by a row sum >= 2^14: eta 2^-14 sum_j |v_j|.

LayerNorm row regimes, interleaved row by row (row i has LN regime i % R, so every 16 / 8 / 4-row workgroup pass mixes them):
unit (ln_case's 2 randn + 0.5, the control), const (exactly 2.0), nearconst (2.0 with max(1, E / 96) elements one ulp_T up, as
block_ref.make_x0), bigmean (1000 + randn in fp32; 1024 + g {-2..2} on T's grid, g = 8 in bf16 and 1 in fp16), outlier (4096 in a
unit row), tiny (randn 2^-20), and in fp16 top (randn 8192 clamped to +-60000).  dy alternates per cycle of R rows between randn and
rows proportional to x-hat, where the xh * c2 term of dx dominates.  The LayerNorm bounds are ln_case's forms with LN_C unchanged.

Measured: the largest |err| / bound of the kernels on one MI355X is 0.76 (fp32 dq, small-v), of the fp32 emulations of a correct
kernel 0.59 (fp32 dq, offset-); the 16-bit outputs sit at half an ulp.  Per (dtype, regime, tensor): the docstrings of
tests/test_value_regimes.py (kernels) and tests/test_value_regimes_cpu.py (emulations), and DESIGN.md, "Value regimes".
"""
import math

import torch

import block_ref as R
import kernel_check as KC
from block_ref import ATTN_C, LN_C, LSE_ULPS, tiny, u_p
from kernel_check import U
from rgb_no_more_amd import detfill

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
NAMES = {F32: "f32", BF16: "bf16", F16: "f16"}
C_D = R.LOGIT_C             # 64: fp32 roundings a term of the 64-term score accumulation can meet (docstring)
EPS = 1e-5
ATTN_REGIMES = ("flat", "peaked", "offset+", "offset-", "small-v")
PEAK_GAIN = 4.0
Q0 = 32.0                   # q[:, 0] of the offset regimes
SMALL_V = 2.0 ** -16
LOG2E = 1.4426950408889634


class Collect(KC.Worst):
    """A Worst that collects the violations (block_ref._cb) so that a test prints every ratio of a case before it fails."""

    def __init__(self):
        super().__init__()
        self.errors = []

    def finish(self, title):
        self.report(title)
        assert not self.errors, f"{title}: {len(self.errors)} checks out of bound\n" + "\n".join(self.errors[:8])


def _n(shape, seed, scale=1.0):
    return torch.from_numpy(detfill.normalish(tuple(shape), seed)) * scale


# ============================================================================================================== attention
def attn_scales(H):
    """the two `scale` arguments every case is run at: attn_case's 1 / sqrt(H 64), and 1 / sqrt(64)"""
    return (1.0 / math.sqrt(H * 64), 0.125)


def offset_k0(scale):
    """b of the offset regimes: the smallest power of two with 32 b scale >= 90; exact in bf16 and fp16; 90 <= offset <= 180."""
    b = R.offset_k0(scale)
    for dt in (BF16, F16):
        assert float(torch.tensor(b).to(dt)) == b and float(torch.tensor(Q0).to(dt)) == Q0
    assert 90.0 <= Q0 * b * scale <= 180.0, (scale, b)
    return b


def pair_regimes(B, H):
    """[B H] index into ATTN_REGIMES of pair (b, h)"""
    return torch.arange(B * H) % len(ATTN_REGIMES)


def planted(N):
    """[(query row, key position)] of the peaked regime: distinct rows of (0, 31, 32, N - 1) against distinct keys of
    (N - 1, 32 t, 32 t - 1, 0)."""
    t = (N - 1) // 32
    rows, keys = [], []
    for r in (0, 31, 32, N - 1):
        if 0 <= r < N and r not in rows:
            rows.append(r)
    for j in ((N - 1, 32 * t, 32 * t - 1, 0) if t else (N - 1, 0)):
        if 0 <= j < N and j not in keys:
            keys.append(j)
    return list(zip(rows, keys))


def heads(t, B, N, H, k=1):
    """[B N, k I] -> k tensors [B H, N, 64] (views where possible)"""
    I = H * 64
    return [t[:, i * I:(i + 1) * I].reshape(B, N, H, 64).permute(0, 2, 1, 3).reshape(B * H, N, 64) for i in range(k)]


def unheads(t, B, N, H):
    """[B H, N, 64] -> [B N, I]"""
    return t.reshape(B, H, N, 64).permute(0, 2, 1, 3).reshape(B * N, H * 64)


def attn_inputs(dt, B, N, H, scale, seed):
    """(qkv [B N, 3 I], dout [B N, I]) in T on the CPU, the regimes applied per (image, head) pair."""
    I = H * 64
    q, k, v = [x.clone() for x in heads(_n((B * N, 3 * I), seed, 1.5), B, N, H, 3)]
    dO = heads(_n((B * N, I), seed + 1, 1.0), B, N, H)[0].clone()
    b0 = offset_k0(scale)
    for p, r in enumerate(pair_regimes(B, H).tolist()):
        name = ATTN_REGIMES[r]
        if name == "peaked":
            q[p] *= PEAK_GAIN
            k[p] *= PEAK_GAIN
            for row, key in planted(N):
                k[p, key] = q[p, row]
        elif name in ("offset+", "offset-"):
            q[p, :, 0] = Q0
            k[p, :, 0] = b0 if name == "offset+" else -b0
        elif name == "small-v":
            v[p] *= SMALL_V
            dO[p] *= SMALL_V
    qkv = torch.cat([unheads(x, B, N, H) for x in (q, k, v)], 1).to(dt).contiguous()
    return qkv, unheads(dO, B, N, H).to(dt).contiguous()


def attn_fwd_ref(qkv, B, N, H, scale):
    """fp64 forward of the T-rounded inputs and the terms of its bounds, all [B H, N, ...]."""
    q, k, v = heads(qkv.double(), B, N, H, 3)
    S = (q @ k.transpose(-1, -2)) * scale
    A = (q.abs() @ k.abs().transpose(-1, -2)) * scale
    lse = torch.logsumexp(S, -1)
    P = torch.exp(S - lse[..., None])
    e = C_D * U * A + 4 * U * (S.abs() + lse.abs()[..., None])
    Pe = P * e
    spe = Pe.sum(-1, keepdim=True)
    mO = P @ v.abs()
    return dict(q=q, k=k, v=v, S=S, A=A, lse=lse, P=P, out=P @ v, outmag=mO, spe=spe[..., 0],
                out_logit=Pe @ v.abs() + spe * mO, vsum=v.abs().sum(-2, keepdim=True),
                lsemag=A.amax(-1) * 64 + lse.abs() + 1)


def attn_bwd_ref(f, dout, out_k, lse_k, B, N, H, scale, dt):
    """fp64 backward on the kernel's own out and lse: {dq, dk, dv: (ref, mag, extra)} [B H, N, 64]."""
    q, k, v, S, A = f["q"], f["k"], f["v"], f["S"], f["A"]
    dO, Ok = heads(dout.double(), B, N, H)[0], heads(out_k.double(), B, N, H)[0]
    lk = lse_k.double().reshape(B * H, N)
    P = torch.exp(S - lk[..., None])
    e = C_D * U * A + 4 * U * (S.abs() + lk.abs()[..., None])
    G = dO @ v.transpose(-1, -2) - (dO * Ok).sum(-1, keepdim=True)
    dS = P * G
    mdS = P * (dO.abs() @ v.abs().transpose(-1, -2) + (dO.abs() * (P @ v.abs())).sum(-1, keepdim=True))
    EdS = P * e * G.abs()
    eta = tiny(dt)
    Pt, dSt = P.transpose(-1, -2), dS.transpose(-1, -2)
    return dict(dq=(scale * dS @ k, scale * mdS @ k.abs(), scale * EdS @ k.abs() + eta * scale * k.abs().sum(-2, keepdim=True)),
                dk=(scale * dSt @ q, scale * mdS.transpose(-1, -2) @ q.abs(),
                    scale * EdS.transpose(-1, -2) @ q.abs() + eta * scale * q.abs().sum(-2, keepdim=True)),
                dv=(Pt @ dO, Pt @ dO.abs(), (P * e).transpose(-1, -2) @ dO.abs() + eta * dO.abs().sum(-2, keepdim=True)))


def finite_in(t, dt, what):
    assert bool(torch.isfinite(t).all()) and float(t.abs().max()) <= torch.finfo(dt).max, f"{what}: fp64 reference not finite in {dt}"


def attn_check(worst, key, where, dt, qkv, dout, out, lse, dqkv, B, N, H, scale, pshift=False):
    """Every element of out, lse and dqkv, per regime (keys `{key}-{regime}-{tensor}` of worst).  out / lse / dqkv: what the kernel
    (or an emulation) wrote, in its layouts.  pshift: the fp16 attn2 / attn3 forward (2^14 exp2(s - max) rounded to fp16)."""
    f = attn_fwd_ref(qkv, B, N, H, scale)
    I = H * 64
    finite_in(f["out"], dt, where + " out")
    finite_in(f["lse"], F32, where + " lse")
    eta = tiny(dt) * (2.0 ** -14 if pshift and dt == F16 else 1.0)
    got_out = heads(out, B, N, H)[0]
    got_lse = lse.reshape(B * H, N)
    if N == 1:                  # P = 1 exactly on every path (exp2(0) = 1, 2^14 / 2^14, 1 * v): bit for bit
        assert torch.equal(out, qkv[:, 2 * I:]), f"{where}: N = 1 and out != v"
    uP = u_p(dt, N)
    reg = pair_regimes(B, H).to(qkv.device)
    x_out = f["out_logit"] + eta * f["vsum"]
    sets = [(name, (reg == r).nonzero().flatten()) for r, name in enumerate(ATTN_REGIMES)]
    sets = [(name, idx) for name, idx in sets if idx.numel()]
    for name, idx in sets:
        w = f"{where} {name}"
        R._cb(worst, f"{key}-{name}-out", got_out[idx], f["out"][idx], f["outmag"][idx], dt, 1, ATTN_C["out"] * uP, w + " out",
              extra=x_out[idx], tile=(N, 64))
        R._cb(worst, f"{key}-{name}-lse", got_lse[idx], f["lse"][idx], f["lsemag"][idx], F32, LSE_ULPS, ATTN_C["lse"] * U, w + " lse",
              extra=f["spe"][idx])
    if dqkv is None:
        return f
    b = attn_bwd_ref(f, dout, out, lse, B, N, H, scale, dt)
    for i, nm in enumerate(("dq", "dk", "dv")):
        ref, mag, extra = b[nm]
        finite_in(ref, dt, f"{where} {nm}")
        got = heads(dqkv[:, i * I:(i + 1) * I], B, N, H)[0]
        for name, idx in sets:
            R._cb(worst, f"{key}-{name}-{nm}", got[idx], ref[idx], mag[idx], dt, 1, ATTN_C[nm] * uP, f"{where} {name} {nm}",
                  extra=extra[idx], tile=(N, 64))
    return f


# the (path, dtype) table of tests/test_value_regimes.py: name, dtype, runtime switches, token counts, operation order of the
# emulation, whether the forward is the persistent kernel's shape list
V1N, V2N, N10 = (1, 33, 196, 224), (1, 33, 196, 224), (225, 320)
ATTN_PATHS = [("v1-7", F32, dict(attn_v2=0), V1N, "v1"), ("v1-7", BF16, dict(attn_v2=0), V1N, "v1"),
              ("v1-7", F16, dict(f16_tuned=0), V1N, "v1"),
              ("v1-10", F32, dict(), N10, "v1"), ("v1-10", BF16, dict(), N10, "v1"), ("v1-10", F16, dict(), N10, "v1"),
              ("attn2", BF16, dict(attn_v2=1, attn_persist=0), V2N, "v2"),
              ("attn2", F16, dict(attn_v2=1, attn_persist=0, f16_tuned=2), V2N, "v2"),
              ("attn3", BF16, dict(attn_v2=1, attn_persist=1), V2N, "v2"),
              ("attn3", F16, dict(attn_v2=1, attn_persist=1, f16_tuned=2), V2N, "v2")]
ATTN3_FWD_SHAPE = (86, 33, 3)          # 258 (image, head) pairs: the smallest case that reaches attn3_fwd_kernel (>= 256 pairs)


def attn_shapes(path, ns):
    """(B, N, H): B = 2, H = 3 (6 pairs: every regime) at every N; one H = 1 (5 pairs) and one H = 12 case; attn3 also the 258 pairs."""
    n = ns[1] if len(ns) > 2 else ns[0]
    return [(2, N, 3) for N in ns] + [(5, n, 1), (1, n, 12)] + ([ATTN3_FWD_SHAPE] if path == "attn3" else [])


def attn_kernels(path, dt, B, N, H):
    """names the profiler must show: (forward, backward), each a tuple of substring tuples (test_kernel_edges.expect)"""
    if path.startswith("v1"):
        t = path[3:]
        return (("attn_fwd_kernel", t),), (("attn_bwd_dq_kernel", t), ("attn_bwd_dkv_kernel", t))
    if path == "attn2":
        return ("attn2_fwd_kernel",), ("attn2_bwd_kernel",)
    return ("attn3_fwd_kernel" if B * H >= 256 else "attn2_fwd_kernel",), ("attn3_bwd_kernel",)


LN_E = (192, 384, 512, 768, 1024)
LN_GENERIC_E = (4, 100, 768)
LN_M = 37


# ------------------------------------------------------------------------------------------- fp32 emulations of the kernels
def _r(t, dt):
    """round to T, back in fp32"""
    return t.to(dt).float()


def emu_attn_fwd(qkv, B, N, H, scale, order="v1", defect=None):
    """fp32 arithmetic of a forward kernel on the CPU.  order "v1": normalise P, round it to T, P . V (attention.hip); "v2": round
    [2^14] exp2(s - max) to T, P . V, times 1 / sum (attention_v2.hip).  defect: None, "nomax" (no max subtraction), "sentinel"
    (keys padded to the 32-token tile scored at -100 scaled units instead of -inf), "flush16" (operands of P . V below 2^-14
    flushed to zero).  Returns (out [B N, I] T, lse [B H N] fp32)."""
    dt = qkv.dtype
    q, k, v = heads(qkv.float(), B, N, H, 3)
    raw = q @ k.transpose(-1, -2)
    if defect == "sentinel":
        pad = -N % 32
        raw = torch.cat([raw, torch.full((B * H, N, pad), -100.0 / scale)], -1)
        v = torch.cat([v, torch.zeros(B * H, pad, 64)], 1)
    m = torch.zeros_like(raw[..., :1]) if defect == "nomax" else raw.amax(-1, keepdim=True)
    sc = torch.tensor(scale, dtype=F32)
    if order == "v1":
        p = torch.exp((raw - m) * sc)
        sm = p.sum(-1, keepdim=True)
        lse = m * sc + torch.log(sm)
        pt = _r(p * (1.0 / sm), dt)
        inv = 1.0
    else:
        sh = 14.0 if dt == F16 else 0.0
        c2 = sc * torch.tensor(LOG2E, dtype=F32)
        p = torch.exp2(raw * c2 - (m * c2 - sh))
        sm = p.sum(-1, keepdim=True)
        lse = m * sc + torch.log(sm * 2.0 ** -sh)
        pt = _r(p, dt)
        inv = 1.0 / sm
    if defect == "flush16":
        pt = torch.where(pt.abs() < 2.0 ** -14, torch.zeros_like(pt), pt)
        v = torch.where(v.abs() < 2.0 ** -14, torch.zeros_like(v), v)
    O = (pt @ v) * inv
    return unheads(O, B, N, H).to(dt), lse.reshape(-1).contiguous()


def emu_attn_bwd(qkv, out, dout, lse, B, N, H, scale, order="v1"):
    """fp32 arithmetic of a backward kernel from the stored out and lse: P and dS rounded to T before the second products; "v1"
    rounds scale dS (attention.hip `ds[r] = p * (da[r] - Dq) * scale`), "v2" multiplies dQ / dK by scale at the end."""
    dt = qkv.dtype
    q, k, v = heads(qkv.float(), B, N, H, 3)
    dO, O = heads(dout.float(), B, N, H)[0], heads(out.float(), B, N, H)[0]
    sc = torch.tensor(scale, dtype=F32)
    P = torch.exp((q @ k.transpose(-1, -2)) * sc - lse.reshape(B * H, N, 1))
    G = dO @ v.transpose(-1, -2) - (dO * O).sum(-1, keepdim=True)
    if order == "v1":
        ds = _r(P * G * sc, dt)
        dq, dk = ds @ k, ds.transpose(-1, -2) @ q
    else:
        ds = _r(P * G, dt)
        dq, dk = (ds @ k) * sc, (ds.transpose(-1, -2) @ q) * sc
    dv = _r(P, dt).transpose(-1, -2) @ dO
    return torch.cat([unheads(x, B, N, H) for x in (dq, dk, dv)], 1).to(dt)


# ============================================================================================================== LayerNorm
def ln_regimes(dt):
    return ("unit", "const", "nearconst", "bigmean", "outlier", "tiny") + (("top",) if dt == F16 else ())


def ln_row_regimes(dt, M):
    """[M] index into ln_regimes(dt) of row i"""
    return torch.arange(M) % len(ln_regimes(dt))


def ln_inputs(dt, M, E, seed):
    """(x, dy) [M, E] in T on the CPU: row i in LN regime i % R; dy of the odd cycles of R rows proportional to x-hat."""
    names = ln_regimes(dt)
    g = _n((M, E), seed)
    x = 2.0 * g + 0.5
    one_up = 2.0 * (1 + 2.0 * KC.U_OF[dt]) if dt != F32 else 2.0 + 2.0 ** -22          # 2.0 + one ulp_T
    grid = {F32: None, BF16: 8.0, F16: 1.0}[dt]
    for i in range(M):
        nm = names[i % len(names)]
        if nm == "const":
            x[i] = 2.0
        elif nm == "nearconst":
            x[i] = 2.0
            x[i, [(7 * i + 13 * m) % E for m in range(max(1, E // 96))]] = one_up
        elif nm == "bigmean":
            x[i] = 1000.0 + g[i] if grid is None else 1024.0 + grid * torch.clamp(torch.round(g[i]), -2, 2)
        elif nm == "outlier":
            x[i] = g[i]
            x[i, (7 * i + 5) % E] = 4096.0
        elif nm == "tiny":
            x[i] = g[i] * 2.0 ** -20
        elif nm == "top":
            x[i] = torch.clamp(g[i] * 8192.0, -60000.0, 60000.0)
    x = x.to(dt)
    dy = _n((M, E), seed + 1)
    x64 = x.double()
    mu = x64.mean(1, keepdim=True)
    xh = (x64 - mu) / torch.sqrt(((x64 - mu) ** 2).mean(1, keepdim=True) + EPS)
    cyc = (torch.arange(M) // len(names)) % 2 == 1
    dy[cyc] = (1.5 * xh[cyc]).float()
    return x, dy.to(dt)


def ln_params(E, seed):
    """gamma, beta as ln_case draws them in scale (1 + 0.2 randn, 0.2 randn), fp32"""
    return 1 + _n((E,), seed + 2, 0.2), _n((E,), seed + 3, 0.2)


def _rows(worst, key, names, reg, fn):
    for r, nm in enumerate(names):
        idx = (reg == r).nonzero().flatten()
        if idx.numel():
            fn(f"{key}-{nm}", idx, nm)


def ln_check_fwd(worst, key, where, dt, x, gamma, beta, y, mean, rstd, eps=EPS, res=None, sc=1.0):
    """ln_case's forward bounds (tests/test_kernel_edges.py), per row regime; every element."""
    M, E = x.shape
    x64, g64, b64 = x.double(), gamma.double(), beta.double()
    mu = x64.mean(1, keepdim=True)
    rs = 1.0 / torch.sqrt(((x64 - mu) ** 2).mean(1, keepdim=True) + eps)
    xh = (x64 - mu) * rs
    yref = (xh * g64 + b64) * sc
    ymag = (g64.abs() * (xh.abs() + rs * x64.abs().mean(1, keepdim=True)) + b64.abs()) * sc
    if res is not None:
        yref, ymag = yref + res.double(), ymag + res.double().abs()
    finite_in(yref, dt, where + " y")
    finite_in(rs, F32, where + " rstd")
    reg = ln_row_regimes(dt, M).to(x.device)
    xam = x64.abs().mean(1)

    def one(k, idx, nm):
        w = f"{where} {nm}"
        R._cb(worst, k + "-y", y[idx], yref[idx], ymag[idx], dt, 1, LN_C["y"] * E * U, w + " y", tile=(16, E))
        R._cb(worst, k + "-stat", mean[idx], mu[idx, 0], xam[idx], F32, 1, LN_C["stat"] * E * U, w + " mean")
        R._cb(worst, k + "-stat", rstd[idx], rs[idx, 0], rs[idx, 0], F32, 1, LN_C["stat"] * E * U, w + " rstd")
    _rows(worst, key, ln_regimes(dt), reg, one)
    return dict(rstd=rs[:, 0], mean=mu[:, 0], var=((x64 - mu) ** 2).mean(1))


def ln_check_bwd(worst, key, where, dt, x, gamma, dy, mean, rstd, dx, dg, dbt, dres=None, init=None, sc=1.0):
    """ln_case's backward bounds on the kernel's own statistics, per row regime; dgamma / dbeta over all rows.  init: (dgamma,
    dbeta) fp64 the accumulating call started from, or None."""
    M, E = x.shape
    x64, g64 = x.double(), gamma.double()
    kmu, krs = mean.double()[:, None], rstd.double()[:, None]
    xh = (x64 - kmu) * krs
    d = dy.double() * sc
    gv = d * g64
    c2 = (gv * xh).mean(1, keepdim=True)
    dxref = krs * (gv - gv.mean(1, keepdim=True) - xh * c2)
    dxmag = krs * (gv.abs() + gv.abs().mean(1, keepdim=True) + xh.abs() * (gv * xh).abs().mean(1, keepdim=True))
    if dres is not None:
        dxref, dxmag = dxref + dres.double(), dxmag + dres.double().abs()
    finite_in(dxref, dt, where + " dx")
    reg = ln_row_regimes(dt, M).to(x.device)
    _rows(worst, key, ln_regimes(dt), reg, lambda k, idx, nm: R._cb(
        worst, k + "-dx", dx[idx], dxref[idx], dxmag[idx], dt, 1, LN_C["dx"] * E * U, f"{where} {nm} dx", tile=(16, E)))
    z = 0.0
    dgref, dgmag = (d * xh).sum(0) + (init[0] if init else z), (d.abs() * xh.abs()).sum(0) + (init[0].abs() if init else z)
    dbref, dbmag = d.sum(0) + (init[1] if init else z), d.abs().sum(0) + (init[1].abs() if init else z)
    R._cb(worst, key + "-dgamma", dg, dgref, dgmag, F32, 1, (M + E) * U, where + " dgamma")
    R._cb(worst, key + "-dbeta", dbt, dbref, dbmag, F32, 1, (M + E) * U, where + " dbeta")


def emu_ln_fwd(x, gamma, beta, eps=EPS, defect=None):
    """fp32 arithmetic of the forward (layernorm.hip: the mean, then the centred sum of squares).  defect: None, "onepass"
    (E[x^2] - mean^2), "noeps" (rsqrt(var)), "sq16" (each centred square formed in fp16 before the fp32 sum: overflows above 65504),
    "acc16" (the sum of squares itself kept in fp16).  Returns (y T, mean, rstd fp32)."""
    dt = x.dtype
    xf = x.float()
    E = xf.shape[1]
    mu = xf.sum(1, keepdim=True) * (1.0 / E)
    c = xf - mu
    if defect == "onepass":
        var = (xf * xf).sum(1, keepdim=True) * (1.0 / E) - mu * mu
    elif defect == "sq16":
        var = (c * c).to(F16).float().sum(1, keepdim=True) * (1.0 / E)
    elif defect == "acc16":
        acc = torch.zeros(xf.shape[0], dtype=F16)
        for j in range(E):
            acc = acc + (c[:, j] * c[:, j]).to(F16)
        var = acc.float()[:, None] * (1.0 / E)
    else:
        var = (c * c).sum(1, keepdim=True) * (1.0 / E)
    rs = torch.rsqrt(var if defect == "noeps" else var + eps)
    return (c * rs * gamma + beta).to(dt), mu[:, 0].clone(), rs[:, 0].clone()


def emu_ln_bwd(x, gamma, dy, mean, rstd, dres=None):
    dt = x.dtype
    xh = (x.float() - mean[:, None]) * rstd[:, None]
    d = dy.float()
    gv = d * gamma
    dx = rstd[:, None] * (gv - gv.mean(1, keepdim=True) - xh * (gv * xh).mean(1, keepdim=True))
    if dres is not None:
        dx = dx + dres.float()
    return dx.to(dt), (d * xh).sum(0), d.sum(0)
