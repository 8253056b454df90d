"""fp64 reference and launch geometry of the SwinV2 window attention (csrc/swin_attn.hip) and fp64 reference, derived bound and
fp32 emulation of the sub-block embedding (csrc/swin.hip), shared by tests/test_swin_edges.py (GPU) and
tests/test_swin_edges_cpu.py.  A plain module, imported by name from the tests (not a conftest.py).

- partition(x, B, res, shift): token-major [B res^2, X] -> windows [B nW, 64, X] with torch.roll and reshapes (the layout of
  oracle/swin_torch.window_attention; nothing here shares index code with the kernel).  Window w = (image, window row, window
  column) in row-major order, which is also the window order of the kernel's lse [(w heads + h) 64 + query] and
  dscale_part [w heads + h].
- win_fwd / win_bwd: the operation in fp64 on one chunk of windows, plus the forward-error terms of the bound (see the docstring
  of tests/test_swin_edges.py for the terms).  The backward runs on the kernel's own out and lse.  Rows below F.normalize's eps
  get g / eps without the projection, as autograd does (tests/test_swin_value_regimes_cpu.py anchors that to the oracle).
- head_grid / geometry: a copy of swin_attn.hip's head_grid() and of the WA<T> LDS sizes, pinned to the C++ source by the CPU
  test (rgbnm_window_attention_bwd_workspace) and used to pick the cases that reach each launch class.
"""
import math

import torch

from oracle import swin_torch as ST

WS, WT, HD = 8, 64, 32
U = 2.0 ** -24


# ------------------------------------------------------------------------------------------------------------- geometry
def wa_lds(esz):
    """(forward LDS bytes, backward LDS bytes, forward waves, backward waves) of one workgroup: swin_attn.hip WA<T>."""
    RP, TP, BP = HD + 8, WT + 4, WT + 4
    row, tr, small = WT * RP * esz, HD * TP * esz, 5 * WT * 4
    sixteen = esz == 2
    fwd_wave = 2 * row + (row if sixteen else tr) + WT * 4
    bwd_wave = 4 * row + (0 if sixteen else 3 * tr) + (row if sixteen else 0) + small
    bwd_waves = 4 if sixteen else 2
    bias = WT * BP * 4
    return bias + 4 * fwd_wave, bias + bwd_waves * bwd_wave, 4, bwd_waves


def head_grid(nwin, heads, per_cu, waves, cus, win_xcd=1):
    """swin_attn.hip head_grid(): workgroups per head (bph), XCD groups (gpx), grid, slots; plus whether the grid was capped."""
    bph = cus * per_cu // heads
    cap = (nwin + waves - 1) // waves
    capped = bph > cap
    if capped:
        bph = cap
    bph = max(bph, 1)
    g = {"bph": bph, "gpx": 0, "grid": bph * heads, "slots": bph, "capped": capped}
    spx = cus // 8 * per_cu
    gpx = spx // heads
    if not capped and cus % 8 == 0 and gpx >= 1 and win_xcd and (spx - gpx * heads) * 100 <= 7 * spx:
        g.update(gpx=gpx, grid=8 * spx, slots=8 * gpx)
    return g


def geometry(esz, direction, B, res, heads, cus, win_xcd=1):
    """Launch geometry of one direction ("fwd" / "bwd") for element size esz: the head_grid plus the waves of a head (wph) and
    the fewest / most windows a wave walks."""
    f_lds, b_lds, f_waves, b_waves = wa_lds(esz)
    lds, waves = (f_lds, f_waves) if direction == "fwd" else (b_lds, b_waves)
    nwin = B * (res // WS) ** 2
    g = head_grid(nwin, heads, 160 * 1024 // lds, waves, cus, win_xcd)
    wph = g["slots"] * waves
    g.update(nwin=nwin, waves=waves, wph=wph, wpw_min=nwin // wph, wpw_max=-(-nwin // wph))
    return g


def classes(esz, direction, g):
    """The launch classes (a)-(e) of tests/test_swin_edges.py one launch belongs to."""
    c = set()
    if g["capped"] and g["wpw_min"] == 0:
        c.add("a")                                   # capped grid, some waves without a window
    if g["wpw_min"] == g["wpw_max"] == 1:
        c.add("b")                                   # exactly one window per wave
    if g["gpx"] == 0 and not g["capped"] and g["wpw_min"] >= 3 and g["nwin"] % g["wph"]:
        c.add("c")                                   # head-major, >= 3 windows per wave, ragged last range
    if g["gpx"] > 0 and g["wpw_max"] >= 2:
        c.add("d")                                   # XCD-aware slot map, multi-window waves
    if esz == 4 and direction == "bwd":
        c.add("e")                                   # fp32 two-wave backward
    return c


def bwd_workspace(B, res, heads, cus):
    """rgbnm_window_attention_bwd_workspace: one fp32 d(bias) slice per backward wave, the largest wave count of the dtypes."""
    nwin = B * (res // WS) ** 2
    waves = 0
    for esz in (2, 4):
        _, b_lds, _, b_waves = wa_lds(esz)
        waves = max(waves, head_grid(nwin, heads, 160 * 1024 // b_lds, b_waves, cus)["bph"] * b_waves)
    return waves * heads * WT * WT * 4


# ------------------------------------------------------------------------------------------------------------- layout
def partition(x, B, res, shift):
    """[B res^2, X] token-major -> [B nW, 64, X]: roll by -shift, 8 x 8 windows (oracle/swin_torch.window_attention)."""
    X = x.shape[-1]
    nw = res // WS
    xs = x.reshape(B, res, res, X)
    if shift:
        xs = torch.roll(xs, (-shift, -shift), (1, 2))
    return xs.reshape(B, nw, WS, nw, WS, X).permute(0, 1, 3, 2, 4, 5).reshape(B * nw * nw, WT, X)


def reverse(xw, B, res, shift):
    """partition's inverse: [B nW, 64, X] -> [B res^2, X]."""
    X = xw.shape[-1]
    nw = res // WS
    o = xw.reshape(B, nw, nw, WS, WS, X).permute(0, 1, 3, 2, 4, 5).reshape(B, res, res, X)
    if shift:
        o = torch.roll(o, (shift, shift), (1, 2))
    return o.reshape(B * res * res, X)


def split_heads(xw, heads):
    """[n, 64, heads 32] -> [n, heads, 64, 32]."""
    return xw.reshape(xw.shape[0], WT, heads, HD).permute(0, 2, 1, 3)


def window_mask(res, shift, nimg, device):
    """[nimg nW, 64, 64] shift mask (-100 across regions) of oracle/swin_torch.shift_mask, or None without a shift."""
    if not shift:
        return None
    return ST.shift_mask(res, WS, shift).to(device=device, dtype=torch.float64).repeat(nimg, 1, 1)


# ------------------------------------------------------------------------------------------------------------- fp64 math
EPS = 1e-12                                                     # F.normalize's eps


def normalize(x):
    n = x.norm(dim=-1, keepdim=True).clamp_min(EPS)            # F.normalize(eps = 1e-12)
    return x / n, n


def clamped(x):
    """[..., 1] bool: rows whose norm lies below eps.  clamp_min passes no gradient there (it does at |x| == eps)."""
    return x.norm(dim=-1, keepdim=True) < EPS


def logits(q, k, bias, scale, mask):
    """q, k [n, H, 64, 32] fp64 -> dict: q_hat, k_hat, norms, cos, A = |q_hat| |k_hat|^T, lg (natural units)."""
    qh, nq = normalize(q)
    kh, nk = normalize(k)
    cos = qh @ kh.transpose(-1, -2)
    A = qh.abs() @ kh.abs().transpose(-1, -2)
    s = scale.view(1, -1, 1, 1)
    lg = cos * s + bias[None]
    m = None
    if mask is not None:
        m = mask[:, None]
        lg = lg + m
    return {"qh": qh, "kh": kh, "nq": nq, "nk": nk, "cq": clamped(q), "ck": clamped(k), "cos": cos, "A": A, "lg": lg, "s": s, "m": m}


def logit_err(L, uT, lse):
    """Bound of the kernel's logit error (natural units), per element [n, H, 64, 64]:
    q_hat / k_hat rounded to T before the MFMA (2 u_T s A), the fp32 sum of squares + rsq of the norms (36 u s A), the fp32 MFMA
    accumulation over d (32 u s A), and the base-2 logit arithmetic / exp2 / log2 (4 u (s + |bias| + |mask| + |lse|))."""
    s = L["s"]
    e = s * L["A"] * (2 * uT + 68 * U)
    e = e + 4 * U * (s + L["lg"].abs() + (L["m"].abs() if L["m"] is not None else 0) + lse.abs()[..., None])
    return e


def win_fwd(q, k, v, bias, scale, mask, uT, uP, eta=0.0):
    """Forward of one chunk.  Returns (L, out, lse, P, E_out, E_lse): E_out is the bound's error term of out (without ulp_T):
    the logit error through the softmax, (P o e)|v| + (sum_j P e) P|v|, P rounded to T before P V (u_P P|v| + eta sum_j |v_j|,
    eta the absolute rounding error of T's subnormals) and the fp32 P V accumulation (64 u P|v|); E_lse = sum_j P e +
    4 u (|lse| + 1)."""
    L = logits(q, k, bias, scale, mask)
    lse = torch.logsumexp(L["lg"], -1)
    P = torch.exp(L["lg"] - lse[..., None])
    out = P @ v
    mO = P @ v.abs()
    e = logit_err(L, uT, lse)
    Pe = P * e
    spe = Pe.sum(-1, keepdim=True)
    E_out = Pe @ v.abs() + spe * mO + (uP + 64 * U) * mO + eta * v.abs().sum(-2, keepdim=True)
    E_lse = spe[..., 0] + 4 * U * (lse.abs() + 1)
    return L, out, lse, P, E_out, E_lse


def proj_back(nh, nrm, g, Eg, uT, clamp=None, project_clamped=False):
    """d x = (I - n n^T) g / |x| for n = x / |x| (F.normalize's backward), and its error bound: Eg through the projection, n
    rounded to T in the kernel (2 u_T), the fp32 dot product / subtraction / 1 / |x| (24 u).  Rows with clamp set (|x| < eps, nrm
    = eps) get g / eps without the projection: autograd of x / clamp_min(|x|, eps) passes nothing to the norm there.  The bound
    keeps the projection's terms on those rows too (they only add |n|^2 of it).  project_clamped: the unconditional form, kept to
    show what it misses (tests/test_swin_value_regimes_cpu.py)."""
    dot = (nh * g).sum(-1, keepdim=True)
    if clamp is not None and not project_clamped:
        dot = torch.where(clamp, torch.zeros_like(dot), dot)
    dx = (g - nh * dot) / nrm
    na = nh.abs()
    mg = g.abs() + na * (na * g.abs()).sum(-1, keepdim=True)
    E = (Eg + na * (na * Eg).sum(-1, keepdim=True) + (2 * uT + 24 * U) * mg) / nrm
    return dx, E


def win_bwd(L, v, dO, O_k, lse_k, uT, uP, eta=0.0, project_clamped=False):
    """Backward of one chunk on the kernel's own out O_k and lse lse_k (fp64 of the T values).  Returns a dict of references
    and error terms (E_*, without ulp) for dq, dk, dv [n, H, 64, 32], dS and its error term [n, H, 64, 64] (summed over windows
    by the caller into d(bias)), and the d(scale) partial per (window, head) with its error term."""
    P = torch.exp(L["lg"] - lse_k[..., None])
    dP = dO @ v.transpose(-1, -2)
    D = (dO * O_k).sum(-1, keepdim=True)
    dS = P * (dP - D)
    mdS = P * (dO.abs() @ v.abs().transpose(-1, -2) + (dO.abs() * O_k.abs()).sum(-1, keepdim=True))
    e = logit_err(L, uT, lse_k)
    # dS: P from the kernel's logits (P e |dP - D|), fp32 dO V^T and D = dO . O (40 u mdS)
    # + 2^-126 |dP - D|: the fp32 exp2 flushes P below the smallest normal to 0
    E_dS = P * e * (dP - D).abs() + 40 * U * mdS + 2.0 ** -126 * (dP - D).abs()
    s = L["s"]
    r = {"dS": dS, "E_dS": E_dS, "absdS": dS.abs()}
    cos = L["cos"]
    r["dsp"] = (dS * cos).sum((-1, -2))
    # d(scale) partial: dS error times |cos|, cos error (the logit error without s: A (2 u_T + 68 u)), 64 u of the fp32 sum
    r["E_dsp"] = (E_dS * cos.abs() + dS.abs() * L["A"] * (2 * uT + 68 * U) + 64 * U * (dS * cos).abs()).sum((-1, -2))
    r["mdsp"] = (dS * cos).abs().sum((-1, -2))
    # dq_hat = s dS k_hat: s dS rounded to T and k_hat rounded to T before the MFMA (2 u_T), 64 u of the fp32 accumulation
    dqh = s * (dS @ L["kh"])
    # (+ eta sum_j |k^_j|: s dS rounded into T's subnormals)
    E_dqh = s * (E_dS @ L["kh"].abs()) + (2 * uT + 64 * U) * s * (dS.abs() @ L["kh"].abs()) + eta * L["kh"].abs().sum(-2, keepdim=True)
    r["dq"], r["E_dq"] = proj_back(L["qh"], L["nq"], dqh, E_dqh, uT, L["cq"], project_clamped)
    dkh = s * (dS.transpose(-1, -2) @ L["qh"])
    E_dkh = (s * (E_dS.transpose(-1, -2) @ L["qh"].abs()) + (2 * uT + 64 * U) * s * (dS.abs().transpose(-1, -2) @ L["qh"].abs())
             + eta * L["qh"].abs().sum(-2, keepdim=True))
    r["dk"], r["E_dk"] = proj_back(L["kh"], L["nk"], dkh, E_dkh, uT, L["ck"], project_clamped)
    # dv = P^T dO: P from the kernel's logits (P e), P rounded to T (u_P), 64 u accumulation
    r["dv"] = P.transpose(-1, -2) @ dO
    mdv = P.transpose(-1, -2) @ dO.abs()
    r["E_dv"] = (P * e).transpose(-1, -2) @ dO.abs() + (uP + 64 * U) * mdv + eta * dO.abs().sum(-2, keepdim=True)
    return r


# ------------------------------------------------------------------------------------------------------------- embedding
# rgbnm_swin_embed (csrc/swin.hip swin_embed_kernel): every 8 x 8 DCT block X becomes A^T X A, split into 2 x 2 sub-blocks of
# 4 x 4 coefficients (luma) or 4 x 4 sub-blocks of 2 x 2 (chroma); token (2 Hb, 2 Wb) grid, 16 + 2 x 4 features per token.
EMBED_CASES = [(1, 2, 2), (1, 2, 6), (1, 6, 2), (3, 6, 10), (2, 4, 14)]       # (B, Hb, Wb)
EMBED_BLOCKS_PER_WG = 4
# The bound's c (in units of u = 2^-24), derived, not fitted.  The kernel takes t[r][c] = sum_k A[k][r] X[k][c] and then
# v[r][c] = sum_k t[r][k] A[k][c] as two sequential 8-term fp32 dot products (fma or multiply + add: each term meets at most 8
# roundings), so with g8 = 8u / (1 - 8u) (Higham, Accuracy and Stability, Lemma 3.1 / eq. 3.5):
#   |t^ - t| <= g8 (|A|^T |X|),    |v^ - sum_k t^ A| <= g8 (|t^| |A|) <= g8 (1 + g8) mag,    mag = |A|^T |X| |A|
#   |v^ - v| <= g8 mag + g8 (1 + g8) mag = (2 g8 + g8^2) mag = 16.0000114 u mag.
# The input is widened to fp32 exactly and A is the caller's fp32 matrix, so nothing else rounds before the store; the store
# rounds v^ to the output type: at most half an ulp of v^, which is at most one ulp_TO of the reference.
_G8 = 8 * U / (1 - 8 * U)
EMBED_C = (2 * _G8 + _G8 * _G8) / U


def embed_blocks(B, Hb, Wb):
    """(luma blocks, chroma blocks) of one call: the kernel numbers them luma first and gives a workgroup 4."""
    return B * Hb * Wb, B * 2 * (Hb // 2) * (Wb // 2)


def embed_matrices(dtype=torch.float64):
    """(A_luma, A_chroma): the conversion matrices the model hands the kernel (oracle/swin_torch._conv)."""
    return ST._conv(4, 2, dtype), ST._conv(2, 4, dtype)


def embed_inputs(B, Hb, Wb, seed):
    """The committed inputs of a case: detfill.normalish luma [B, 1, Hb, Wb, 8, 8] and chroma [B, 2, Hb/2, Wb/2, 8, 8], fp32."""
    from rgb_no_more_amd import detfill
    y = torch.from_numpy(detfill.normalish((B, 1, Hb, Wb, 8, 8), seed))
    c = torch.from_numpy(detfill.normalish((B, 2, Hb // 2, Wb // 2, 8, 8), seed + 1))
    return y, c


def embed_ref(y, cbcr, Ay, Ac):
    """fp64 reference and forward-error magnitude of the embedding, [B, 2 Hb, 2 Wb, 24] each: A^T X A per block and
    |A|^T |X| |A|, then the header's einops split -- rows '(p1 pdh)', columns '(p2 pdw)', coefficient-major -- written as one
    einops pattern; nothing here shares index arithmetic with the kernel.  y, cbcr: any float dtype (their values, in fp64);
    Ay, Ac: the fp32 / fp64 matrices the kernel is given."""
    import einops
    out = []
    for x, A, sub in ((y, Ay, 2), (cbcr, Ac, 4)):
        x64, A64 = x.double(), A.double()
        both = []
        for t in (A64.T @ x64 @ A64, A64.abs().T @ x64.abs() @ A64.abs()):
            both.append(einops.rearrange(t, "b c h w (p1 pdh) (p2 pdw) -> b (h pdh) (w pdw) (c p1 p2)", pdh=sub, pdw=sub))
        out.append(both)
    (fy, my), (fc, mc) = out
    return torch.cat([fy, fc], dim=3), torch.cat([my, mc], dim=3)


def embed_emulate(y, cbcr, Ay, Ac, fma=True):
    """The kernel's arithmetic on the CPU: fp32 inputs (already widened), two sequential 8-term fp32 dot products per element in
    the kernel's order, k ascending, from t = 0.  fma: one rounding per term (the product of two fp32 is exact in fp64); else
    the product is rounded to fp32 first.  Returns fp32 [B, 2 Hb, 2 Wb, 24] (laid out by embed_ref's einops pattern)."""
    import einops
    f32, f64 = torch.float32, torch.float64

    def term(a, b, acc):
        p = a.to(f64) * b.to(f64)
        if not fma:
            p = p.to(f32).to(f64)
        return (p + acc.to(f64)).to(f32)
    out = []
    for x, A, sub in ((y, Ay, 2), (cbcr, Ac, 4)):
        x, A = x.to(f32), A.to(f32)
        t = torch.zeros_like(x)
        for k in range(8):                                   # t[r][c] += A[k][r] X[k][c]
            t = term(A[k, :, None], x[..., k, None, :], t)
        v = torch.zeros_like(x)
        for k in range(8):                                   # v[r][c] += t[r][k] A[k][c]
            v = term(t[..., :, k, None], A[k, None, :], v)
        out.append(einops.rearrange(v, "b c h w (p1 pdh) (p2 pdw) -> b (h pdh) (w pdw) (c p1 p2)", pdh=sub, pdw=sub))
    return torch.cat(out, dim=3)
