"""Value regimes for the SwinV2 window attention (csrc/swin_attn.hip win_attn_fwd_kernel / win_attn_bwd_kernel): CPU input
builders, the per-regime element-wise check at weight c = 1, and an fp32 / T emulation of the kernel's rounding points with seeded
defects.  A plain module, imported by name from tests/test_swin_value_regimes.py (GPU) and tests/test_swin_value_regimes_cpu.py;
the companion of tests/regime_ref.py, which did the same for the ViT attention and LayerNorm entries.

Why: tests/test_swin_edges.py walks every launch class, but on one input recipe (win_inputs): largest logit 68 to 81 natural units
(fp32 exp overflows at 88.72), masked keys 100 below the row maximum everywhere, no norm near F.normalize's eps = 1e-12 and no zero
row.  A forward without max subtraction, a -inf mask, 1 / (|x| + eps), an unclamped rsq, squares formed in fp16 and flushed 16-bit
operands all pass it, and the backward's projection (I - n n^T) was applied below eps too, where autograd of F.normalize gives
g / eps -- in the kernel and in the test reference alike.

Regimes, one per (window, head) pair: REGIMES[(w + h) % 6], w the window index of swin_ref.partition.  Window w is in regime
w % 6 on head 0 and the assignment moves on by one per head: every wave's walk and every head's d(bias) sum mixes regimes, and
the 4-region corner window of a shifted image (w = 3 mod 4 at res 16) meets the signed regime on some head, which w % 6 alone
cannot give at res 16.  Head h keeps scale SCALES[h % 5] of tests/test_swin_edges.py (5 heads: all five values; s = 100 on head 3).
- control:    win_inputs' recipe: unit Gaussian directions, norms 10^+-2, drawn on the CPU.
- aligned:    control, with keys 63, 32, 31, 0 set to 2, 8, 4, 2 times queries 0, 31, 32, 63: cos = 1 exactly, at the tile and
              half-wave edges (the bias at those four entries is 15.999).  On the s = 100 head the logit is >= 100.
- signed:     q = a sigma d, k = -b sigma d: one direction d per pair, a, b in 2^0..5 per token, sigma = +-1 alternating over the
              window's shift-mask regions (from oracle.swin_torch.shift_mask).  cos = -1 inside a region and +1 across regions of
              opposite sigma: at s = 100 the masked keys sit at bias, the unmasked ones at bias - 100.
- degenerate: token t % 4 == 0: q row exactly 0; 1: k row exactly 0; 2: q and k below eps (bf16 / fp32: randn 2^-50 at t % 8 == 2,
              randn 2^-75 at t % 8 == 6, whose squares underflow fp32, and randn 2^-44 at t % 16 == 10: norms of 0.27 to 0.4 eps,
              where 1 / (|x| + eps) is 25 % off and the projection |n|^2 ~ 0.1, which bf16 can see too; fp16, which cannot reach
              1e-12, has subnormal rows randn 2^-16 instead); 3: control.
- extremes:   unit Gaussian directions times a power of two per token, q and k in different orders: 2^-30 .. 2^55 in bf16 / fp32
              (|x|^2 <= 2^119 stays finite in fp32), 2^-16 .. 2^13 clamped to +-60000 in fp16.
- small-v:    control with v and dO times 2^-16 (regime_ref.SMALL_V).
In fp16 the degenerate and extremes pairs carry dO times 2^-12: dq is linear in dO and 1 / |q| reaches 2^13.5 on their subnormal
rows.  Every value is exact in T.

The check (win_regime_check) is win_check's, in window layout on the kernel's own out and lse, with every derived term of
tests/swin_ref.py at weight c = 1 (the fitted WIN_C stay in force for tests/test_swin_edges.py), split per regime.  The fp64
reference of every element must be finite in T; the one exception: fp16 own-row gradients of exactly-zero q / k rows, g / eps,
where the reference lies beyond 65504 by more than the bound: there the kernel must store +-inf with the reference's sign.  On
those same rows an element whose bound interval straddles 65504 may be stored as a value inside the bound or as that +-inf
(_grad_check: 1 / eps turns the 2^-25 rounding of s dS into 3e4 per term, so the bound itself is wider than fp16's range there).
Both kinds are counted and together capped at (zero rows) 32 per pair.

Added bound terms: none.  The emulation of a correct kernel stays inside c = 1 in every regime and dtype (the CPU file prints the
ratios); see its docstring for the figures.
"""
import math

import torch

import kernel_check as KC
import swin_ref as R
import test_swin_edges as E
from block_ref import _cb
from kernel_check import U
from oracle import swin_torch as ST
from regime_ref import Collect, SMALL_V  # noqa: F401  (Collect: re-exported for the two test files)

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
NAMES = {F32: "f32", BF16: "bf16", F16: "f16"}
ESZ = {F32: 4, BF16: 2, F16: 2}
REGIMES = ("control", "aligned", "signed", "degenerate", "extremes", "small-v")
SCALES = E.SCALES
ALIGNED = ((0, 63, 2.0), (31, 32, 8.0), (32, 31, 4.0), (63, 0, 2.0))      # (query, planted key, key / query)
CLAMP_EXP = (-50, -75, -44)         # bf16 / fp32 rows below eps: t % 8 == 2, t % 8 == 6, and of those t % 16 == 10 (|x| ~ 0.3 eps)
F16_SUB_EXP = -16                   # fp16 instead: subnormal rows
EXT_EXP = {F32: (-30, 55), BF16: (-30, 55), F16: (-16, 13)}
F16_TOP = 60000.0
F16_DO = 2.0 ** -12                 # dO factor of the fp16 degenerate / extremes pairs
C1 = {k: 1.0 for k in ("out", "lse", "dq", "dk", "dv", "dbias", "dsp", "dscale")}
CASES = [(3, 16, 5, 0), (3, 16, 5, 4)]            # (B, res, heads, shift): 12 windows


def pair_regimes(nwin, heads):
    """[nwin, heads] index into REGIMES"""
    return (torch.arange(nwin)[:, None] + torch.arange(heads)[None]) % len(REGIMES)


def head_scales(heads):
    return torch.tensor([SCALES[h % len(SCALES)] for h in range(heads)], dtype=F32)


def regions(res, shift):
    """[nW, 64] region number of every token of every window of one image, read off oracle.swin_torch.shift_mask (two tokens
    share a region where the mask is 0), numbered in order of first appearance; all 0 without a shift."""
    nW = (res // 8) ** 2
    if not shift:
        return torch.zeros(nW, 64, dtype=torch.long)
    first = (ST.shift_mask(res, 8, shift) == 0).float().argmax(-1)        # the region's first token
    out = torch.zeros(nW, 64, dtype=torch.long)
    for w in range(nW):
        reps = sorted(set(first[w].tolist()))
        out[w] = torch.tensor([reps.index(int(f)) for f in first[w]])
    return out


def extreme_exponents(dt):
    lo, hi = EXT_EXP[dt]
    eq = torch.tensor([lo + round((hi - lo) * t / 63) for t in range(64)], dtype=F32)
    return eq, eq[(37 * torch.arange(64) + 11) % 64]


def win_regime_inputs(dt, B, res, heads, shift, seed):
    """dict: qkv [B res^2, 3C], dout [B res^2, C] in T, bias [heads, 64, 64], scale [heads] fp32 on the CPU, and reg [nwin, heads]."""
    nw = res // 8
    nW, nwin, C = nw * nw, B * nw * nw, heads * 32
    g = torch.Generator().manual_seed(seed)
    rt = lambda t: t.to(dt).float()                                       # noqa: E731  (round to T)
    base = torch.randn((3, nwin, heads, 64, 32), generator=g)
    spread = 10.0 ** (torch.rand((2, nwin, heads, 64, 1), generator=g) * 4 - 2)
    dO = torch.randn((nwin, heads, 64, 32), generator=g)
    bias = torch.rand((heads, 64, 64), generator=g) * 16
    bias[:, ::7, ::5] = 15.999
    bias[:, 1::9, 2::11] = 1e-3
    for qi, kj, _ in ALIGNED:
        bias[:, qi, kj] = 15.999
    dirs = rt(torch.randn((nwin, heads, 1, 32), generator=g))
    pw = 2.0 ** torch.randint(0, 6, (2, nwin, heads, 64, 1), generator=g).float()
    q, k, v = rt(base[0] * spread[0]), rt(base[1] * spread[1]), rt(base[2])
    reg = pair_regimes(nwin, heads)
    sel = lambda name: reg == REGIMES.index(name)                         # noqa: E731
    # aligned
    s = sel("aligned")
    for qi, kj, f in ALIGNED:
        k[s, kj] = q[s, qi] * f
    # signed
    s = sel("signed")
    sigma = (1.0 - 2.0 * (regions(res, shift) % 2).float()).repeat(B, 1)[:, None, :, None].expand(nwin, heads, 64, 1)
    q[s] = (pw[0] * sigma * dirs)[s]
    k[s] = (-pw[1] * sigma * dirs)[s]
    # degenerate rows
    s = sel("degenerate")
    t = torch.arange(64)
    qd, kd = q[s], k[s]
    qd[:, t % 4 == 0] = 0.0
    kd[:, t % 4 == 1] = 0.0
    bq, bk = base[0][s], base[1][s]
    if dt == F16:
        m = t % 4 == 2
        qd[:, m], kd[:, m] = bq[:, m] * 2.0 ** F16_SUB_EXP, bk[:, m] * 2.0 ** F16_SUB_EXP
    else:
        for m, e in ((t % 8 == 2, CLAMP_EXP[0]), (t % 8 == 6, CLAMP_EXP[1]), (t % 16 == 10, CLAMP_EXP[2])):
            qd[:, m], kd[:, m] = rt(bq[:, m]) * 2.0 ** e, rt(bk[:, m]) * 2.0 ** e
    q[s], k[s] = qd, kd
    # norm extremes
    s = sel("extremes")
    eq, ek = extreme_exponents(dt)
    q[s] = base[0][s] * 2.0 ** eq[:, None]
    k[s] = base[1][s] * 2.0 ** ek[:, None]
    if dt == F16:
        q, k = q.clamp(-F16_TOP, F16_TOP), k.clamp(-F16_TOP, F16_TOP)
        dO[sel("degenerate") | s] *= F16_DO
    # small-v
    s = sel("small-v")
    v[s] *= SMALL_V
    dO[s] *= SMALL_V
    tok = lambda x: x.permute(0, 2, 1, 3).reshape(nwin, 64, C)            # noqa: E731
    qkv = R.reverse(torch.cat([tok(q), tok(k), tok(v)], -1), B, res, shift).to(dt).contiguous()
    dout = R.reverse(tok(dO), B, res, shift).to(dt).contiguous()
    return {"qkv": qkv, "dout": dout, "bias": bias, "scale": head_scales(heads), "reg": reg}


def multi_window_case(esz, ncu):
    """The (B, res, heads) with the fewest (window, head) pairs for which swin_ref.geometry reports >= 3 windows per wave and a
    ragged last range, forward and backward, at win_xcd 1 and 0; None if the search finds none."""
    best = None
    for res in (16, 24, 32):
        for heads in (1, 2, 3, 4, 5, 6, 8, 12, 16, 24):
            for B in range(1, 129):
                gs = [R.geometry(esz, d, B, res, heads, ncu, x) for d in ("fwd", "bwd") for x in (1, 0)]
                if all(g["wpw_min"] >= 3 and g["nwin"] % g["wph"] for g in gs):
                    cand = (B * (res // 8) ** 2 * heads, B * res * res, B, res, heads)
                    best = cand if best is None or cand < best else best
                    break
    return best[2:] if best else None


# --------------------------------------------------------------------------------------------------------------- the check
def _finite(t, dt, what):
    assert bool(torch.isfinite(t).all()) and float(t.abs().max()) <= torch.finfo(dt).max, f"{what}: fp64 reference not finite in {dt}"


def _grad_check(worst, key, where, dt, got, ref, Eb, zero_rows, counts):
    """dq / dk of one regime's pairs [m, 64, 32].  zero_rows [m, 64]: exactly-zero input rows, whose own gradient g / eps is the
    only place where T's range max_T may be left (fp16).  With bound = ulp_T(ref) + E:
    - |ref| - bound > max_T: every value inside the bound lies beyond the range: the kernel must hold +-inf of the reference's sign;
    - |ref| - bound <= max_T < |ref| + bound: values inside the bound lie on both sides (1 / eps turns the 2^-25 rounding of s dS
      into fp16's subnormals into 3e4 per term): the kernel holds a value inside the bound, or +-inf of the reference's sign
      (either sign where bound > |ref| + max_T);
    - everything else, and every element off the zero rows: finite in T and inside the bound.
    The elements of the first two kinds are counted (`key`, `key-edge`) and together capped at (zero rows) 32 per pair."""
    fmax = torch.finfo(dt).max
    g = got.double()
    bound = KC.ulp(ref, dt) + Eb
    zr = zero_rows[..., None].expand_as(ref)
    must = zr & (ref.abs() - bound > fmax)
    edge = zr & ~must & (ref.abs() + bound > fmax)
    n, n2 = int(must.sum()), int(edge.sum())
    if n or n2:
        assert dt == F16, f"{where}: reference beyond {dt}"
        assert bool(((must | edge).sum((-1, -2)) <= zero_rows.sum(-1) * 32).all()), f"{where}: more overflow elements than (zero rows) 32"
        assert bool((torch.isinf(g[must]) & (torch.sign(g[must]) == torch.sign(ref[must]))).all()), \
            f"{where}: {n} references beyond 65504 by more than the bound, kernel value not +-inf of that sign"
        einf = edge & torch.isinf(g)
        assert bool(((torch.sign(g[einf]) == torch.sign(ref[einf])) | (bound[einf] > ref[einf].abs() + fmax)).all()), \
            f"{where}: +-inf of the wrong sign next to the fp16 range"
        counts[key] = counts.get(key, 0) + n
        counts[key + "-edge"] = counts.get(key + "-edge", 0) + n2
        gone = must | einf
        ref = torch.where(gone, torch.zeros_like(ref), ref)
        got = torch.where(gone, torch.zeros_like(got), got)
    _finite(torch.where(edge, torch.zeros_like(ref), ref), dt, where)
    _cb(worst, key, got, ref, Eb, dt, 1, 1.0, where)


def win_regime_check(worst, dt, B, res, heads, shift, qkv, dout, bias, scale, out, lse, dqkv, dbias, dsp, dsc, gb, where,
                     project_clamped=False, reg=None):
    """win_check of tests/test_swin_edges.py at c = 1, per regime: keys `{dtype}-{regime}-{output}` of worst (a Collect).  out,
    lse, dqkv, dbias, dsp, dsc: plain tensors in the kernel's layouts, on qkv's device.  Returns counts: the fp16 overflow
    elements per key, and the norms / rows the builders promise."""
    C, nw, dev = heads * 32, res // 8, qkv.device
    nW, nwin = nw * nw, B * nw * nw
    uT = KC.U_OF[dt]
    uP = 0.0 if dt == F32 else uT
    eta = E.ETA[dt]
    k = NAMES[dt]
    reg = pair_regimes(nwin, heads).to(dev) if reg is None else reg.to(dev)
    qkv_w, dout_w = R.partition(qkv, B, res, shift), R.partition(dout, B, res, shift)
    out_w, dqkv_w = R.partition(out, B, res, shift), R.partition(dqkv, B, res, shift)
    lse_k, dsp_k = lse.view(nwin, heads, 64), dsp.view(nwin, heads)
    b64, s64 = bias.double(), scale.double()
    db_ref = torch.zeros(heads, 64, 64, dtype=torch.float64, device=dev)
    db_E, db_abs = torch.zeros_like(db_ref), torch.zeros_like(db_ref)
    dsp_ref, dsp_E, dsp_mag = [], [], []
    counts = {}
    per = max(1, (1 << 23) // (nW * heads * 4096))
    for b0 in range(0, B, per):
        nimg = min(per, B - b0)
        w0, w1 = b0 * nW, (b0 + nimg) * nW
        x = qkv_w[w0:w1].double()
        q, kk, v = (R.split_heads(x[..., i * C:(i + 1) * C], heads) for i in range(3))
        mask = R.window_mask(res, shift, nimg, dev)
        Lg, o_ref, lse_ref, P, E_out, E_lse = R.win_fwd(q, kk, v, b64, s64, mask, uT, uP, eta)
        _finite(o_ref, dt, where + " out")
        _finite(lse_ref, F32, where + " lse")
        nq, nk = q.norm(dim=-1), kk.norm(dim=-1)
        for n_ in (nq, nk):                 # no norm within a factor 2 of eps: fp64 and the kernel's fp32 decide the clamp alike
            assert not bool(((n_ > R.EPS / 2) & (n_ < R.EPS * 2)).any()), where + ": a norm within a factor 2 of eps"
        O_k = R.split_heads(out_w[w0:w1], heads)
        dO = R.split_heads(dout_w[w0:w1].double(), heads)
        lk = lse_k[w0:w1]
        r = R.win_bwd(Lg, v, dO, O_k.double(), lk.double(), uT, uP, eta, project_clamped)
        dw = dqkv_w[w0:w1]
        got = {nm: R.split_heads(dw[..., i * C:(i + 1) * C], heads) for i, nm in enumerate(("dq", "dk", "dv"))}
        zero = {"dq": nq == 0, "dk": nk == 0}
        rg = reg[w0:w1]
        for ri, name in enumerate(REGIMES):
            idx = rg == ri
            if not bool(idx.any()):
                continue
            tag = f"{where} windows {w0}..{w1 - 1} {name}, element (pair of the regime, query / key, d)"
            key = f"{k}-{name}-"
            _cb(worst, key + "out", O_k[idx], o_ref[idx], E_out[idx], dt, 1, 1.0, tag + " out")
            _cb(worst, key + "lse", lk[idx], lse_ref[idx], E_lse[idx], F32, 1, 1.0, tag + " lse")
            try:
                for nm in ("dq", "dk"):
                    _grad_check(worst, key + nm, tag + " " + nm, dt, got[nm][idx], r[nm][idx], r["E_" + nm][idx], zero[nm][idx], counts)
                _finite(r["dv"][idx], dt, tag + " dv")
                _finite(r["dsp"][idx], F32, tag + " dscale_part")
            except AssertionError as e:
                # the backward's reference runs on the kernel's own out and lse: where those are already out of bound it may
                # leave T's range; that fails the case through the forward's violations, anything else is raised
                if "reference" not in str(e) or not worst.errors:
                    raise
                worst.errors.append(str(e)[:300])
                worst(key + "backward", math.inf)
                continue
            _cb(worst, key + "dv", got["dv"][idx], r["dv"][idx], r["E_dv"][idx], dt, 1, 1.0, tag + " dv")
            _cb(worst, key + "dsp", dsp_k[w0:w1][idx], r["dsp"][idx], r["E_dsp"][idx], F32, 1, 1.0, tag + " dscale_part")
        counts["clamped"] = counts.get("clamped", 0) + int(((nq < R.EPS) & (nq > 0)).sum() + ((nk < R.EPS) & (nk > 0)).sum())
        counts["zero"] = counts.get("zero", 0) + int((nq == 0).sum() + (nk == 0).sum())
        db_ref += r["dS"].sum(0)
        db_E += r["E_dS"].sum(0)
        db_abs += r["absdS"].sum(0)
        dsp_ref.append(r["dsp"])
        dsp_E.append(r["E_dsp"])
        dsp_mag.append(r["mdsp"])
        del r, Lg, P, E_out, o_ref
    S = gb["slots"] * gb["waves"]
    if not worst.errors:
        _finite(db_ref, F32, where + " dbias")
    _cb(worst, k + "-dbias", dbias.view(heads, 64, 64), db_ref, db_E + (gb["wpw_max"] + S) * U * db_abs, F32, 1, 1.0,
        where + " dbias (head, query, key)")
    dsp_ref, dsp_E, dsp_mag = torch.cat(dsp_ref), torch.cat(dsp_E), torch.cat(dsp_mag)
    _cb(worst, k + "-dscale", dsc, dsp_ref.sum(0), dsp_E.sum(0) + nwin * U * dsp_mag.sum(0), F32, 1, 1.0, where + " dscale (head)")
    return counts


# ------------------------------------------------------------------------------------- fp32 / T emulation of the kernels
LOG2E = torch.tensor(1.44269504088896340736, dtype=F32)
LN2 = torch.tensor(0.69314718055994530942, dtype=F32)
CLAMP = torch.tensor(1e12, dtype=F32)
DEFECTS = ("nomax", "infmask", "addeps", "rsq", "sq16", "flush16", "proj", "pflush")


def _r(t, dt):
    return t.to(dt).float()


def _flush(t, below=2.0 ** -14):
    return torch.where(t.abs() < below, torch.zeros_like(t), t)


def emu_norm(x, dt, order, defect):
    """x [..., 32] fp32 -> (x^ rounded to T, 1 / norm).  swin_attn.hip: every lane squares and sums its 16-byte piece (8 / 4
    elements), a xor tree adds the 4 / 8 lanes of a token (order "lanes"; "flat": one fp32 sum), inv_norm = min(rsq, 1e12)."""
    sq = x * x
    if defect == "sq16":
        sq = sq.to(F16).float()
    if order == "lanes":
        ep = 4 if dt == F32 else 8
        part = sq.reshape(*sq.shape[:-1], 32 // ep, ep)
        acc = part[..., 0]
        for e in range(1, ep):
            acc = acc + part[..., e]
        while acc.shape[-1] > 1:
            acc = acc[..., 0::2] + acc[..., 1::2]
        n2 = acc
    else:
        n2 = sq.sum(-1, keepdim=True)
    if defect == "addeps":
        inv = 1.0 / (torch.sqrt(n2) + 1e-12)
    elif defect == "rsq":
        inv = torch.rsqrt(n2)
    else:
        inv = torch.minimum(torch.rsqrt(n2), CLAMP)
    return _r(x * inv, dt), inv


def _logits2(dt, qh, kh, bias, scale, mask, defect):
    """base-2 logits [n, H, query, key] and the raw cosines"""
    sa = qh @ kh.transpose(-1, -2)
    lg = sa * (scale * LOG2E).view(1, -1, 1, 1) + (bias * LOG2E)[None]
    if mask is not None:
        pen = torch.tensor(-math.inf if defect == "infmask" else -100.0, dtype=F32) * LOG2E
        lg = torch.where(mask[:, None] != 0, lg + pen, lg)
    return lg, sa


def _operands(dt, qkv_w, heads, defect):
    C = heads * 32
    x = qkv_w.float()
    if defect == "flush16":
        x = _flush(x)
    return [R.split_heads(x[..., i * C:(i + 1) * C], heads) for i in range(3)]


def emu_fwd(dt, qkv_w, bias, scale, mask, heads, order="lanes", defect=None):
    """qkv_w [n, 64, 3C] T (window layout), mask [n, 64, 64] or None -> out [n, H, 64, 32] T, lse [n, H, 64] fp32."""
    q, k, v = _operands(dt, qkv_w, heads, defect)
    qh, _ = emu_norm(q, dt, order, defect)
    kh, _ = emu_norm(k, dt, order, defect)
    if defect == "flush16":
        qh, kh = _flush(qh), _flush(kh)
    lg, _ = _logits2(dt, qh, kh, bias, scale, mask, defect)
    m = torch.zeros_like(lg[..., :1]) if defect == "nomax" else lg.amax(-1, keepdim=True)
    p = torch.exp2(lg - m)
    sm = p.sum(-1, keepdim=True)
    lse = ((m + torch.log2(sm)) * LN2)[..., 0]
    P = _r(p * (1.0 / sm) if order == "lanes" else p / sm, dt)
    if defect == "pflush":
        P = _flush(P, 2.0 ** KC._FMT[dt][1])
    if defect == "flush16":
        P = _flush(P)
    return (P @ v).to(dt), lse


def emu_bwd(dt, qkv_w, dout_w, out, lse, bias, scale, mask, heads, order="lanes", defect=None):
    """-> dict dq, dk, dv [n, H, 64, 32] T, dbias [H, 64, 64], dsp [n, H], dscale [H] fp32, from the stored out (T) and lse."""
    q, k, v = _operands(dt, qkv_w, heads, defect)
    g = R.split_heads(dout_w.float(), heads)
    if defect == "flush16":
        g = _flush(g)
    qh, iq = emu_norm(q, dt, order, defect)
    kh, ik = emu_norm(k, dt, order, defect)
    if defect == "flush16":
        qh, kh = _flush(qh), _flush(kh)
    D = (g * out.float()).sum(-1, keepdim=True)
    lg, sa = _logits2(dt, qh, kh, bias, scale, mask, defect)
    p = torch.exp2(lg - (lse * LOG2E)[..., None])
    ds = p * (g @ v.transpose(-1, -2) - D)
    dss = _r(ds * scale.view(1, -1, 1, 1), dt)
    P = _r(p, dt)
    if defect == "flush16":
        dss, P = _flush(dss), _flush(P)
    if defect == "pflush":
        P = _flush(P, 2.0 ** KC._FMT[dt][1])

    def back(nh, inv, gh):
        proj = (nh * gh).sum(-1, keepdim=True)
        if defect != "proj":
            proj = torch.where(inv == CLAMP, torch.zeros_like(proj), proj)
        return ((gh - nh * proj) * inv).to(dt)
    dsp = (ds * sa).sum((-1, -2))
    return {"dq": back(qh, iq, dss @ kh), "dk": back(kh, ik, dss.transpose(-1, -2) @ qh), "dv": (P.transpose(-1, -2) @ g).to(dt),
            "dbias": ds.sum(0), "dsp": dsp, "dscale": dsp.sum(0)}


def emulate(dt, B, res, heads, shift, qkv, dout, bias, scale, order="lanes", defect=None):
    """Forward and backward on token-major CPU tensors; returns the kernel's outputs in the kernel's layouts:
    out [N, C], lse [nwin heads 64], dqkv [N, 3C], dbias [heads 4096], dsp [nwin heads], dsc [heads]."""
    nwin, C = B * (res // 8) ** 2, heads * 32
    mask = R.window_mask(res, shift, B, "cpu")
    qkv_w, dout_w = R.partition(qkv, B, res, shift), R.partition(dout, B, res, shift)
    tok = lambda x: x.permute(0, 2, 1, 3).reshape(nwin, 64, C)            # noqa: E731
    o, lse = emu_fwd(dt, qkv_w, bias, scale, mask, heads, order, defect)
    b = emu_bwd(dt, qkv_w, dout_w, o, lse, bias, scale, mask, heads, order, defect)
    dqkv = R.reverse(torch.cat([tok(b[n]) for n in ("dq", "dk", "dv")], -1), B, res, shift)
    return (R.reverse(tok(o), B, res, shift), lse.reshape(-1).contiguous(), dqkv, b["dbias"].reshape(-1).contiguous(),
            b["dsp"].reshape(-1).contiguous(), b["dscale"])
