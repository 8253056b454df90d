"""Stage-local fp64 references, case lists and rounding-point emulations of the three composites of csrc/vit.hip that
tests/test_composite_edges.py drives at the C ABI: the dropout encoder block (rgbnm_vit_block_fwd_drop / _bwd_drop), the class
head (rgbnm_head_fwd / _bwd) and the patch embedding (rgbnm_patch_embed_fwd[_mix] / _bwd); and the launch arithmetic of
rgbnm_dropout_apply (csrc/dropout.hip launch_apply).  A plain module (like block_ref.py / step_ends_ref.py): the GPU file passes
the kernels' outputs through the check functions below, tests/test_composite_edges_cpu.py the outputs of the emulations and of
the seeded defects -- the same calls, the same bounds.

Every tensor a call writes is compared with the fp64 result of that ONE stage applied to the tensors the same run stored
upstream (block_ref.py's design).  No bound is new: every one is ulp_T(ref) + k u mag + named terms taken from
- block_ref.py (LayerNorm, attention, GEMM + residual, GELU, LayerNorm backward behind a GEMM, weight gradients) with the
  dropout factors f = keep . scale entering as in tests/test_dropout_kernels.py nt_drop_case (block_ref.check_res / check_gelu,
  argument f): the mask multiplies the T-rounded staged value (`inter` times f) and the product with the fp32 scale is one more
  fp32 rounding (gemm.hip, `drop_one`: `v * d.scale`);
- tests/test_kernel_edges.py nt_case for the head's two epilogues: tanh (tanhf: + 2 fp32 ulps, + ulp_T(pre) where the tile is
  rounded first: gemm.hip pass 1 `store4<T>(Cs ...)`, gemm_nt_small.hip `(float)(bf16)v[e]`) and (1 - h^2) (+ 2^-23 |pre|,
  + ulp_T(pre) |1 - h^2|), and its tn terms ((M + 2) u mag, one fp32 ulp);
- step_ends_ref.py for the sub-block features (embed_check) and the head pool (pool_fwd_check / pool_bwd_check).
The masked copies dy_m = T(f2 dy) and dxmid_m = T(f0 dx_mid) are bit for bit (dropout.hip: `from_f32<T>(drop_one(d, w, to_f32(v)))`,
one fp32 product, one rounding).  Nothing is left out of any check: there is no omitted share to cap.

Masks come from dropout_ref.factor and the seed; no mask is stored anywhere.
"""
import math

import torch

import block_ref as R
import dropout_ref as D
import step_ends_ref as S
from kernel_check import U, ulp, check_bound
from oracle import vit_torch as V

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
DT = {"f32": F32, "bf16": BF16, "f16": F16}
NTOK = R.NTOK
SEEDS = (0, 0x0123456789ABCDEF, 2 ** 64 - 1, 987654321)        # tests/test_dropout_kernels.SEEDS (the GPU file asserts it)


def cdiv(a, b):
    return -(-a // b)


# ============================================================================================================= case lists
# dropout block on the generic kernels: (dtype, B, p, (d->block of the first, of the second block), index into SEEDS).  Every
# dtype meets both B and both p; the four seeds, block indices 0, 1 and 11 all occur; the second block's dx feeds the first.
DROP_GENERIC = [("f32", 1, 0.5, (0, 11), 0), ("f32", 3, 0.1, (0, 1), 1), ("f16", 1, 0.1, (0, 11), 2), ("f16", 3, 0.5, (0, 1), 3),
                ("bf16", 1, 0.1, (0, 1), 2), ("bf16", 3, 0.5, (0, 11), 1)]
DROP_FUSED_B = 42               # 196 * 42 = 8232 >= 8192: fused_dx_lnbwd's epilogues run behind the masked operands
DROP_E384 = (64, 384, 6)        # (B, E, heads): 12544 rows, a multiple of 64 -- tn_wide's one launch, or two pairs
DROP_GROUP_B = 16               # E = 192, 3136 rows (a multiple of 64): tn_group 0 / 1 / 2 are 4 / 2 / 1 weight-gradient launches

# rgbnm_dropout_apply past its grid cap: (dtype, M, N)
APPLY_CAP = 8192 * 256          # groups of 8 columns one turn of dropout_apply_kernel's grid-stride loop covers
APPLY_BIG = [("bf16", 43700, 384), ("f32", 2731, 6152), ("f16", 5501, 3083)]


def apply_regime(M, N, ldx=None, ldy=None):
    """launch_apply (csrc/dropout.hip) in Python: (grid, turns of the loop, groups in the last turn, vector path)."""
    ldx, ldy = ldx or N, ldy or N
    total = M * cdiv(N, 8)
    assert total < 2 ** 31
    grid = min(cdiv(total, 256), 8192)
    per_turn = grid * 256
    vec = N % 8 == 0 and ldx % 8 == 0 and ldy % 8 == 0          # (and 16-byte aligned bases: torch allocations are)
    return grid, cdiv(total, per_turn), total - (cdiv(total, per_turn) - 1) * per_turn, vec


# class head: (dtype, B, N, E, C, workspace 'apart' | 'shared', tn_group)
HEAD_B = (1, 3, 256, 512, 513)


def head_cases():
    out = []
    for i, B in enumerate(HEAD_B):
        for j, dt in enumerate(("f32", "bf16", "f16")):
            k = 3 * i + j
            e, n = ((192, 196), (384, 294))[(i + j) % 2]
            out.append((dt, B, n, e, (1000, 40)[i % 2], ("apart", "shared")[k % 2], (k // 2) % 2))
    return out


HEAD_CASES = head_cases()


def head_nt_kernel(dt, B):
    """rgbnm_gemm_nt's choice for the head's three GEMMs (gemm.hip launch_nt_sel): bf16 with M <= 512 rows takes
    gemm_nt_small_kernel (N % 4 == 0, K % 8 == 0 hold for every committed C and E), everything else gemm_nt_kernel."""
    return "gemm_nt_small_kernel" if dt == "bf16" and B <= 512 else "gemm_nt_kernel"


def head_ws_split(B, E, C, ws_bytes, tn_ws):
    """rgbnm_head_bwd's regions: (apart, (offset, bytes) x 3).  tn_ws(M, No, Ki) = rgbnm_gemm_tn_workspace."""
    r = lambda v: (v + 255) & ~255                             # noqa: E731
    s1, s2, s3 = r(tn_ws(B, C, E)), r(tn_ws(B, E, E)), B * 2 * E * 4
    apart = ws_bytes >= s1 + s2 + s3
    if apart:
        return True, ((0, s1), (s1, s2), (s1 + s2, ws_bytes - s1 - s2))
    return False, ((0, ws_bytes),) * 3


# patch embedding: B in PE_B, the type pairs of step_ends_ref.EMBED_BIG_PAIRS; 28 x 28 luma blocks = 196 tokens
PE_B = (1, 3, 42)
PE_GRID = (28, 28)


# ================================================================================================================ dropout
def factors(seed, p, block, M, e, device="cpu", dtype=torch.float64):
    """{site: keep . scale} of one block: sites 0 and 2 are [M, E], site 1 is [M, 4 E]."""
    return {s: torch.from_numpy(D.factor(seed, p, s, block, M, n)).to(device).to(dtype) for s, n in ((0, e), (1, 4 * e), (2, e))}


def masks_bite(f, p, where):
    """Every site drops and keeps, within 6 sigma of p at the case's size."""
    for s, t in f.items():
        n = t.numel()
        kept = int((t != 0).sum())
        assert 0 < kept < n, f"{where}: site {s} keeps {kept} of {n}"
        assert abs(kept / n - (1 - p)) <= 6 * math.sqrt(p * (1 - p) / n), f"{where}: site {s} keeps {kept / n:.4f}, p = {p}"


def masked_copy(x, f, p):
    """T(f x) as rgbnm_dropout_apply computes it: one fp32 product with the fp32 scale, one rounding; dropped elements are +0."""
    scale = float(D.threshold(p)[1])
    return torch.where(f != 0, (x.float() * scale).to(x.dtype), torch.zeros_like(x))


def check_masked_copies(where, G, f, p):
    """dy_m and dxmid_m bit for bit from the stored dy and dx_mid (raises on the first difference)."""
    for key, src, site in (("dy_m", "dy", 2), ("dxmid_m", "dx_mid", 0)):
        want = masked_copy(G[src], f[site], p)
        ok = S.same_bits(G[key], want)
        assert bool(ok.all()), f"{where}: {key} differs from T(f{site} {src}) in {int((~ok).sum())} elements, first {(~ok).nonzero()[:4].tolist()}"


def check_drop_block(worst_f, worst_b, worst_w, where, P, A, G, W, B, f, p, inter=True):
    """Forward stages, the two masked copies, backward stages and the twelve parameter gradients of one dropout block.
    Returns check_block_fwd's info (regime assertions)."""
    info = R.check_block_fwd(worst_f, where, P, A, B, inter=inter, f=f)
    if G is not None:
        check_masked_copies(where, G, f, p)
        r2, r1 = R.check_block_bwd(worst_b, where, P, A, G, B)
        if W is not None:
            R.check_block_dw(worst_w, where, A, G, W, B)
            R.check_dln_total(worst_w, where, r2, r1, W, B)
    return info


def regimes(info, M, first, where):
    """What tests/test_block_edges.py asserts of its inputs: GELU tails (the fc1 biases of block_ref.make_params put 8 columns
    below -18 and 8 above 6), near one-hot attention rows, and -- for the block that reads make_x0 -- near-constant rows."""
    pre = info["pre"]
    lo, hi, mid = int((pre < -18).sum()), int((pre > 6).sum()), int((pre.abs() < 3).sum())
    assert lo >= 4 * M and hi >= 4 * M and mid > pre.numel() // 2, f"{where}: GELU regimes {(lo, mid, hi)}"
    assert info["onehot_rows"] >= M // 10, f"{where}: one-hot rows {info['onehot_rows']}"
    if first:
        assert info["rstd1_max"] > 0.8 * R.EPS ** -0.5, f"{where}: max rstd1 {info['rstd1_max']:.4g}"


# --------------------------------------------------------------------------------------------- emulation (bf16, staged epilogues)
_f, _b = R._f, R._b


def _drop(v, f):
    """philox.h drop_one: `w >= d.thr ? v * d.scale : 0.f` -- a dropped element is +0 whatever the sign of v."""
    return torch.where(f != 0, v * f, torch.zeros_like(v))


def emu_drop_fwd(P, x_in, B, f):
    """rgbnm_vit_block_fwd_drop's rounding points (vit.hip; gemm.hip staged epilogue): acc + bias rounded to bf16 in the LDS tile,
    the mask's fp32 product, the residual added in fp32, one rounding.  f: fp32 factors {0, 1, 2}."""
    A = dict(x_in=x_in)
    A["xn1"], A["mean1"], A["rstd1"] = R.emu_ln(x_in, P["ln1_g"], P["ln1_b"])
    A["qkv"] = _b(_f(A["xn1"]) @ _f(P["wqkv"]).T + P["bqkv"])
    A["attn"], A["lse"] = R.emu_attn_fwd(A["qkv"], B, 1.0 / math.sqrt(x_in.shape[1]))

    def res(a, w, b, r, fs):
        return _b(_drop(_f(_b(_f(a) @ _f(w).T + b)), fs) + _f(r))
    A["x_mid"] = res(A["attn"], P["wproj"], P["bproj"], x_in, f[0])
    A["xn2"], A["mean2"], A["rstd2"] = R.emu_ln(A["x_mid"], P["ln2_g"], P["ln2_b"])
    pre = _f(_b(_f(A["xn2"]) @ _f(P["w1"]).T + P["b1"]))
    A["gl"] = _b(_drop(0.5 * pre * (1 + torch.erf(pre * R.SQRT1_2)), f[1]))
    A["u"] = _b(_drop(0.5 * (1 + torch.erf(pre * R.SQRT1_2)) + pre * torch.exp(-0.5 * pre * pre) * (1.0 / math.sqrt(2 * math.pi)), f[1]))
    A["x_out"] = res(A["gl"], P["w2"], P["b2"], A["x_mid"], f[2])
    return A


DROP_DEFECTS = ("residual_masked", "dw2_unmasked", "dwproj_unmasked", "mask1_twice")


def emu_drop_bwd(P, A, dy, B, f, defect=None):
    """vit.hip block_bwd with d, generic kernels: dy_m = bf16(f2 dy); du = bf16(bf16(dy_m W2) u); dx_mid = dy + LN2'(bf16(du W1));
    dxmid_m = bf16(f0 dx_mid); dattn = bf16(dxmid_m Wproj); dqkv; dx = dx_mid + LN1'(bf16(dqkv Wqkv)); then the weight gradients.
    defect: one of DROP_DEFECTS, seeded where it would arise."""
    assert defect is None or defect in DROP_DEFECTS
    G = dict(dy=dy)
    G["dy_m"] = _b(_drop(_f(dy), f[2]))
    G["du"] = _b(_f(_b(_f(G["dy_m"]) @ _f(P["w2"]))) * _f(A["u"]) * (f[1] if defect == "mask1_twice" else 1.0))
    res2 = G["dy_m"] if defect == "residual_masked" else dy
    G["dx_mid"], G["part2"] = R.emu_lnbwd(G["du"], P["w1"], A["x_mid"], A["mean2"], A["rstd2"], P["ln2_g"], res2, B)
    G["dxmid_m"] = _b(_drop(_f(G["dx_mid"]), f[0]))
    G["dattn"] = _b(_f(G["dxmid_m"]) @ _f(P["wproj"]))
    G["dqkv"] = R.emu_attn_bwd(A, G["dattn"], B, dy.shape[1])
    res1 = G["dxmid_m"] if defect == "residual_masked" else G["dx_mid"]
    G["dx"], G["part1"] = R.emu_lnbwd(G["dqkv"], P["wqkv"], A["x_in"], A["mean1"], A["rstd1"], P["ln1_g"], res1, B)
    Gw = dict(G)                         # what the weight-gradient GEMMs are handed
    Gw["dy"] = dy if defect == "dw2_unmasked" else G["dy_m"]
    Gw["dx_mid"] = G["dx_mid"] if defect == "dwproj_unmasked" else G["dxmid_m"]
    W = R.emu_block_dw(A, Gw)
    G["part2"], G["part1"] = None, None  # the per-operation paths reduce over row panels: check_dln_total
    return G, W


# =================================================================================================================== head
def head_params(E, C, seed):
    """fp32 masters on the CPU (weights are cast to the compute type by the caller): gamma, beta, w1 [E, E], b1, w2 [C, E], b2."""
    n = S.randn
    return dict(ln_g=1 + n((E,), seed, 0.2), ln_b=n((E,), seed + 1, 0.2), w1=n((E, E), seed + 2, 1.5 / math.sqrt(E)), b1=n((E,), seed + 3, 0.3),
                w2=n((C, E), seed + 4, 1.0 / math.sqrt(E)), b2=n((C,), seed + 5, 0.3))


def head_inputs(B, N, E, C, dt, seed):
    """(x [B, N, E] with every second token at mean 100 (step_ends_ref.pool_inputs), dlogits [B, C]) in the compute type."""
    x, _, _, _ = S.pool_inputs(B, N, E, dt, True, seed)
    return x, (S.randn((B, C), seed + 7) / B).to(dt)


def _tn_check(worst, key, where, dy, x, dw, db, M):
    ref, mag, rb, mb = R.tn(dy.double(), x.double())
    worst(key, check_bound(dw, ref, mag, F32, 1, (M + 2) * U, f"{where} {key}", tile=(128, 192)))
    worst("db" + key[2:], check_bound(db, rb, mb, F32, 1, (M + 2) * U, f"{where} db{key[2:]}"))


def check_head_fwd(worst, where, P, x, a, dt, eps=R.EPS):
    """P: ln_g, ln_b, b1, b2 fp32 and w1, w2 in dt; x [B, N, E]; a: pooled, mean, rstd, h1, logits as the call stored them."""
    B, N, E = x.shape
    inter = dt != F32
    S.pool_fwd_check(a["pooled"], a["mean"], a["rstd"], x, P["ln_g"], P["ln_b"], eps, dt, where, worst, "head")
    pre, mag = R.linear(a["pooled"].double(), P["w1"].double(), P["b1"].double())
    ref = torch.tanh(pre)
    worst("h1", check_bound(a["h1"], ref, mag, dt, 1, E * U, where + " h1", extra=2 * ulp(ref, F32) + (ulp(pre, dt) if inter else 0.0)))
    ref, mag = R.linear(a["h1"].double(), P["w2"].double(), P["b2"].double())
    worst("logits", check_bound(a["logits"], ref, mag, F32, 1, E * U, where + " logits"))


def check_head_bwd(worst, where, P, x, a, dl, g, dt):
    """g: dw2, db2, da, dw1, db1, dpooled, dx, dln_g, dln_b as the call stored them; dl = dlogits [B, C] in dt."""
    B, N, E = x.shape
    C = dl.shape[1]
    inter = dt != F32
    _tn_check(worst, "dw2", where, dl, a["h1"], g["dw2"], g["db2"], B)
    pre, mag = dl.double() @ P["w2"].double(), dl.double().abs() @ P["w2"].double().abs()
    fac = 1 - a["h1"].double() ** 2
    worst("da", check_bound(g["da"], pre * fac, mag * fac.abs(), dt, 1, C * U, where + " da",
                            extra=pre.abs() * 2.0 ** -23 + (ulp(pre, dt) * fac.abs() if inter else 0.0)))
    _tn_check(worst, "dw1", where, g["da"], a["pooled"], g["dw1"], g["db1"], B)
    ref, mag = g["da"].double() @ P["w1"].double(), g["da"].double().abs() @ P["w1"].double().abs()
    worst("dpooled", check_bound(g["dpooled"], ref, mag, dt, 1, E * U, where + " dpooled"))
    S.pool_bwd_check(g["dx"], g["dln_g"], g["dln_b"], g["dpooled"], x, P["ln_g"], a["mean"], a["rstd"], None, dt, where, worst, "head")


HEAD_DEFECTS = ("da_from_pooled", "dw1_from_dpooled")


def emu_head(P, x, dl, dt, eps=R.EPS, defect=None):
    """rgbnm_head_fwd / _bwd in fp32 with the entries' rounding points (pool kernels: fp32 throughout, one rounding of pooled and
    dx; GEMM tiles rounded to dt before tanh / (1 - h^2) in the 16-bit modes).  (a, g) as the check functions take them."""
    assert defect is None or defect in HEAD_DEFECTS
    t = lambda v: v.to(dt)                                       # noqa: E731
    B, N, E = x.shape
    xf = x.float()
    mu = xf.mean(2, keepdim=True)
    rs = torch.rsqrt(((xf - mu) ** 2).mean(2, keepdim=True) + eps)
    xh = (xf - mu) * rs
    a = dict(mean=mu.reshape(-1).clone(), rstd=rs.reshape(-1).clone(), pooled=t(xh.mean(1) * P["ln_g"] + P["ln_b"]))
    pre = a["pooled"].float() @ P["w1"].float().T + P["b1"]
    a["h1"] = t(torch.tanh(t(pre).float()))
    a["logits"] = a["h1"].float() @ P["w2"].float().T + P["b2"]
    g = {}
    g["dw2"], g["db2"] = dl.float().T @ a["h1"].float(), dl.float().sum(0)
    h = (a["pooled"] if defect == "da_from_pooled" else a["h1"]).float()
    g["da"] = t(t(dl.float() @ P["w2"].float()).float() * (1 - h * h))
    g["dpooled"] = t(g["da"].float() @ P["w1"].float())
    src = g["dpooled"] if defect == "dw1_from_dpooled" else g["da"]
    g["dw1"], g["db1"] = src.float().T @ a["pooled"].float(), src.float().sum(0)
    d = (g["dpooled"].float() / N)[:, None, :]
    gv = d * P["ln_g"]
    g["dx"] = t(rs * (gv - gv.mean(2, keepdim=True) - xh * (gv * xh).mean(2, keepdim=True))).reshape(B * N, E)
    g["dln_g"], g["dln_b"] = (d * xh).sum((0, 1)), g["dpooled"].float().sum(0)
    return a, g


def head64(P, x):
    """The head's stages composed in fp64 (the CPU anchor against oracle.vit_torch.class_head): (logits, saved)."""
    pooled, _, mu, rs, _ = S.pool_fwd_ref(x, P["ln_g"], P["ln_b"], R.EPS)
    h1 = torch.tanh(R.linear(pooled, P["w1"], P["b1"])[0])
    return R.linear(h1, P["w2"], P["b2"])[0], dict(pooled=pooled, mean=mu, rstd=rs, h1=h1)


def head64_bwd(P, x, sv, dl):
    g = {}
    g["dw2"], _, g["db2"], _ = R.tn(dl, sv["h1"])
    da = (dl @ P["w2"]) * (1 - sv["h1"] ** 2)
    g["dw1"], _, g["db1"], _ = R.tn(da, sv["pooled"])
    g["dx"], _, g["dln_g"], _, g["dln_b"], _ = S.pool_bwd_ref(da @ P["w1"], x, P["ln_g"], sv["mean"], sv["rstd"])
    return g


# ======================================================================================================== patch embedding
def pe_params(E, N, seed):
    """wpe [E, 384], bpe [E] and a position table [N, E] whose rows differ strongly (std 4 per element: a wrong period or row
    offset moves an element by several units, hundreds of times the bound)."""
    return dict(wpe=S.randn((E, 384), seed, 0.05), bpe=S.randn((E,), seed + 1, 0.3), pos=S.randn((N, E), seed + 2, 4.0))


def check_pe_fwd(worst, where, feat, x0, y, cbcr, A, lam, P, TI, TO, N):
    """feat through step_ends_ref.embed_check; x0 = T(feat Wpe^T + b + pos[row % N]): nt_case's EPI_POS bound (K = 384)."""
    worst("feat", S.embed_check(feat, y, cbcr, A, 0, lam, TI, TO, where + " feat"))
    M = feat.shape[0]
    pp = P["pos"].double()[torch.arange(M, device=feat.device) % N]
    ref, mag = R.linear(feat.double(), P["wpe"].double(), P["bpe"].double())
    worst("x0", check_bound(x0, ref + pp, mag + pp.abs(), TO, 1, 384 * U, where + " x0", tile=(128, 192)))


PE_DEFECTS = ("pos_period", "bias_twice")


def emu_pe_fwd(feat, P, TO, N, defect=None):
    """The EPI_POS epilogue: acc + bias + pos in fp32, one rounding (gemm.hip pass 1 / direct epilogue)."""
    assert defect is None or defect in PE_DEFECTS
    M = feat.shape[0]
    rows = torch.arange(M) % ((N - 1) if defect == "pos_period" else N)
    v = feat.float() @ P["wpe"].float().T + P["bpe"] * (2.0 if defect == "bias_twice" else 1.0) + P["pos"][rows]
    return v.to(TO)


# ==================================================================================== fp64 compositions (the CPU anchors)
def drop_block64(P, x_in, B, f):
    """The forward stages of one masked block composed in fp64 (de-interleaved wqkv / bqkv, like the kernels): saved tensors."""
    sv = dict(x_in=x_in)
    l1 = R.ln_fwd(x_in, P["ln1_g"], P["ln1_b"])
    sv["xn1"], sv["mean1"], sv["rstd1"] = l1["y"], l1["mean"], l1["rstd"]
    sv["qkv"] = R.linear(sv["xn1"], P["wqkv"], P["bqkv"])[0]
    at = R.attn_fwd(sv["qkv"], B, 1.0 / math.sqrt(x_in.shape[1]))
    sv["attn"], sv["lse"] = at["out"], at["lse"]
    sv["x_mid"] = x_in + f[0] * R.linear(sv["attn"], P["wproj"], P["bproj"])[0]
    l2 = R.ln_fwd(sv["x_mid"], P["ln2_g"], P["ln2_b"])
    sv["xn2"], sv["mean2"], sv["rstd2"] = l2["y"], l2["mean"], l2["rstd"]
    pre = R.linear(sv["xn2"], P["w1"], P["b1"])[0]
    sv["gl"], sv["u"] = f[1] * R.gelu64(pre), f[1] * R.dgelu64(pre)
    sv["x_out"] = sv["x_mid"] + f[2] * R.linear(sv["gl"], P["w2"], P["b2"])[0]
    return sv


def drop_block64_bwd(P, sv, dy, B, f):
    """The backward stages in the issue's wiring: (dx, {the twelve parameter gradients, dwqkv / dbqkv in the kernels' row order})."""
    dy_m = f[2] * dy
    du = (dy_m @ P["w2"]) * sv["u"]                                   # u carries mask 1 already
    b2 = R.ln_bwd(du @ P["w1"], sv["x_mid"], sv["mean2"], sv["rstd2"], P["ln2_g"], dy)
    dx_mid = b2["dx"]
    dxmid_m = f[0] * dx_mid
    ab = R.attn_bwd(sv["qkv"], sv["attn"], dxmid_m @ P["wproj"], sv["lse"], B, 1.0 / math.sqrt(dy.shape[1]))
    dqkv = torch.cat([ab["dq"][0], ab["dk"][0], ab["dv"][0]], 1)
    b1 = R.ln_bwd(dqkv @ P["wqkv"], sv["x_in"], sv["mean1"], sv["rstd1"], P["ln1_g"], dx_mid)
    W = dict(dln1_g=b1["dgamma"].sum(0), dln1_b=b1["dbeta"].sum(0), dln2_g=b2["dgamma"].sum(0), dln2_b=b2["dbeta"].sum(0))
    for key, dyk, xk in (("w2", dy_m, sv["gl"]), ("w1", du, sv["xn2"]), ("wproj", dxmid_m, sv["attn"]), ("wqkv", dqkv, sv["xn1"])):
        W["d" + key], _, W["db" + key[1:]], _ = R.tn(dyk, xk)
    return b1["dx"], W


def pe64(y, cbcr, wpe, bpe, pos):
    """(feat [M, 384], x0 [M, E]) in fp64: step_ends_ref.embed_ref's features, then feat Wpe^T + b + pos[row % N]."""
    luma, _, _, chroma = S.embed_ref(y, cbcr, V.conv_matrix(16, torch.float64))
    feat = torch.cat([luma, chroma], 1)
    N = pos.shape[0]
    return feat, feat @ wpe.T + bpe + pos[torch.arange(feat.shape[0]) % N]
