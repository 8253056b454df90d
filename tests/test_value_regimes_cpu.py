"""CPU tests of the machinery behind tests/test_value_regimes.py (no GPU, no rgb_no_more_amd kernel; tests/regime_ref.py):
- every generator reaches the regime it claims (logit spread, |offset|, one-hot rows at the planted keys, the fp16 subnormal share;
  rstd at eps^-1/2, mean^2 / var, overflowing squares);
- every (path, dtype) of the GPU file is listed against every regime that applies to it;
- fp32-arithmetic emulations of a correct kernel, in both operation orders (first generation: normalise P, then P . V; attn2: P . V,
  then times 1 / sum; the backward with scale inside or outside the rounding of dS), pass every bound of every case the GPU file
  runs, at both scales -- the bounds admit a correct kernel, measured on the reference side and never on a kernel;
- seeded defects PASS today's unit-scale inputs of attn_case / ln_case under today's bounds and FAIL in the named regime: the gap
  existed and is closed;
- block_ref.make_params with `offset` left at its default gives today's parameters bit for bit.

Worst |err| / bound of the emulations (pytest -s prints them per regime; the largest over paths, orders and scales),
out / lse / dq / dk / dv:
    fp32  flat .02/.04/.28/.14/.03  peaked .04/.07/.21/.11/.06  offset+ .06/.11/.56/.28/.12  offset- .03/.06/.59/.30/.08  small-v .01/.04/.22/.11/.02
    bf16  flat .35/.03/.15/.07/.23  peaked .38/.04/.25/.22/.28  offset+ .32/.09/.13/.07/.22  offset- .32/.05/.15/.09/.20  small-v .36/.03/.15/.08/.22
    fp16  flat .33/.05/.14/.07/.21  peaked .30/.07/.23/.49/.24  offset+ .23/.09/.12/.07/.20  offset- .21/.05/.13/.07/.18  small-v .47/.04/.004/.004/.47
LayerNorm (two-pass fp32), y / statistics / dx: fp32 .30/.24/.21, bf16 .50/.20/.50, fp16 .50/.29/.50; dgamma .02, dbeta .01.
Without the logit term the fp32 emulation exceeds today's out bound 9.7 times on the offset pairs (printed by its test).
"""
import math

import pytest
import torch

import block_ref as R
import kernel_check as KC
import regime_ref as G
from kernel_check import U
from regime_ref import BF16, F16, F32, NAMES

PATH_IDS = [f"{p[0]}-{NAMES[p[1]]}" for p in G.ATTN_PATHS]


Collect = G.Collect


# ======================================================================================================= attention: regimes reached
@pytest.mark.parametrize("dt", [F32, BF16, F16], ids=lambda d: NAMES[d])
@pytest.mark.parametrize("B,N,H", [(2, 33, 3), (2, 196, 3), (2, 320, 3), (5, 33, 1), (1, 33, 12)])
def test_attention_generators_reach_their_regimes(dt, B, N, H):
    for scale in G.attn_scales(H):
        qkv, dout = G.attn_inputs(dt, B, N, H, scale, 11)
        f = G.attn_fwd_ref(qkv, B, N, H, scale)
        reg = G.pair_regimes(B, H)
        assert set(reg.tolist()) == set(range(len(G.ATTN_REGIMES))), "every regime occurs in every case"
        S, P, lse = f["S"], f["P"], f["lse"]
        flat_std = 1.5 * 1.5 * 8 * scale              # std of a 64-term dot product of N(0, 1.5) values, scaled: 0.65 .. 2.25
        for p, r in enumerate(reg.tolist()):
            name, s = G.ATTN_REGIMES[r], S[p]
            spread = float(s.std()) if N > 1 else 0.0
            if name in ("flat", "small-v"):
                assert spread <= 1.3 * flat_std and float(lse[p].abs().max()) < 6 * flat_std + math.log(N) + 1
            if name == "peaked":
                assert N == 1 or spread >= 8 * flat_std, (spread, flat_std)
                pairs = G.planted(N)
                assert len(pairs) == min(N, 4) or (N == 33 and len(pairs) == 3)
                for row, key in pairs:              # the planted key wins its row: near one-hot, at the tile-edge positions
                    assert float(P[p, row, key]) > 0.99, (row, key, float(P[p, row, key]))
                assert int((P[p].amax(-1) > 0.9).sum()) >= len(pairs)
                keys = {k for _, k in pairs}
                assert {0, N - 1} <= keys and (N <= 32 or {32 * ((N - 1) // 32)} <= keys)
            if name in ("offset+", "offset-"):
                off = G.Q0 * G.offset_k0(scale) * scale
                assert 90 <= off <= 180
                sign = 1 if name == "offset+" else -1
                assert float((s * sign).min()) > off - 8 * flat_std - 1 and float((s * sign).max()) < off + 8 * flat_std + 1
                assert spread <= 1.3 * flat_std, "the spread stays that of the flat regime"
                e32 = torch.exp(s.float())           # what a kernel without max subtraction forms
                if sign > 0:
                    assert bool(torch.isinf(e32).all()), "exp of the unshifted logit overflows fp32"
                else:
                    assert float(e32.sum(-1).max()) == 0.0, "the unshifted row sum flushes to zero"
                q, k = G.heads(qkv, B, N, H, 3)[:2]
                assert bool((q[p, :, 0].float() == G.Q0).all()) and bool((k[p, :, 0].float().abs() == G.offset_k0(scale)).all())
            if name == "small-v":
                v = G.heads(qkv, B, N, H, 3)[2][p].float().abs()
                share = float(((v < 2.0 ** -14) & (v > 0)).float().mean())
                assert share > 0.9, share
                if dt == F16:                       # subnormal outputs too
                    assert float((f["out"][p].abs() < 2.0 ** -14).float().mean()) > 0.9


def test_every_path_is_listed_against_every_regime():
    """The table the GPU file walks: three dtypes on both first-generation tile counts, bf16 and fp16 on attn2 and attn3; every case of
    every path holds all five regimes and both scales; attn3's forward is reached by the 258-pair case only."""
    assert {(p[0], p[1]) for p in G.ATTN_PATHS} == {(a, d) for a in ("v1-7", "v1-10") for d in (F32, BF16, F16)} | {
        (a, d) for a in ("attn2", "attn3") for d in (BF16, F16)}
    for path, dt, opts, ns, order in G.ATTN_PATHS:
        shapes = G.attn_shapes(path, ns)
        assert {n for _, n, _ in shapes} >= set(ns) and {h for _, _, h in shapes} == {1, 3, 12}
        for B, N, H in shapes:
            assert set(G.pair_regimes(B, H).tolist()) == set(range(5)), (path, B, N, H)
            assert (N > 224) == (path == "v1-10")
        fw = [G.attn_kernels(path, dt, *s)[0] for s in shapes]
        assert (("attn3_fwd_kernel",) in fw) == (path == "attn3")
        if dt == F16 and path.startswith("attn"):
            assert opts["f16_tuned"] == 2
    assert G.ATTN3_FWD_SHAPE[0] * G.ATTN3_FWD_SHAPE[2] >= 256 > (G.ATTN3_FWD_SHAPE[0] - 1) * G.ATTN3_FWD_SHAPE[2]
    for dt in (F32, BF16, F16):
        R_ = len(G.ln_regimes(dt))
        assert G.LN_M >= 2 * R_ + 16                    # both dy cycles of every regime, and more than one 16-row pass
        assert ("top" in G.ln_regimes(dt)) == (dt == F16)


# ============================================================================================ attention: emulations pass every bound
@pytest.mark.parametrize("path", G.ATTN_PATHS, ids=PATH_IDS)
def test_emulated_correct_kernel_passes_every_bound(path):
    """Both operation orders on every (path, dtype)'s cases: the bounds must admit either, whichever the kernel takes."""
    name, dt, _, ns, _ = path
    worst = Collect()
    for i, (B, N, H) in enumerate(G.attn_shapes(name, ns)):
        if B > 8:
            B = 7                                       # (the 258-pair case differs in launch geometry only; 21 pairs here)
        for j, scale in enumerate(G.attn_scales(H)):
            qkv, dout = G.attn_inputs(dt, B, N, H, scale, 100 + 10 * i + j)
            for order in ("v1", "v2"):
                out, lse = G.emu_attn_fwd(qkv, B, N, H, scale, order)
                dqkv = G.emu_attn_bwd(qkv, out, dout, lse, B, N, H, scale, order)
                G.attn_check(worst, order, f"emulation {order} {NAMES[dt]} B={B} N={N} H={H} scale={scale:.4f}", dt, qkv, dout, out, lse,
                             dqkv, B, N, H, scale, pshift=(order == "v2"))
    worst.report(f"emulated {name} {NAMES[dt]}")
    assert not worst.errors, "\n".join(worst.errors[:8])


# ================================================================================================================ seeded defects
def today_attn_fwd(dt, qkv, out, lse, B, N, H, scale):
    """attn_case's forward bounds as they stand (no logit term, lse without the ulps), on CPU tensors; worst ratios."""
    f = G.attn_fwd_ref(qkv, B, N, H, scale)
    r1 = KC.check_bound(G.heads(out, B, N, H)[0], f["out"], f["outmag"], dt, 1, R.ATTN_C["out"] * R.u_p(dt, N), "out")
    r2 = KC.check_bound(lse.reshape(B * H, N), f["lse"], f["lsemag"], F32, 0, R.ATTN_C["lse"] * U, "lse")
    return r1, r2


def today_attn_inputs(dt, B, N, H, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B * N, 3 * H * 64, generator=g) * 1.5).to(dt)


def regime_fails(worst, key_part):
    return any(v > 1 for k, v in worst.d.items() if key_part in k)


ATTN_DEFECTS = [("nomax", F32, 33, ("offset+", "offset-")), ("nomax", BF16, 196, ("offset+", "offset-")),
                ("sentinel", F32, 33, ("offset-",)), ("sentinel", BF16, 33, ("offset-",)), ("flush16", F16, 33, ("small-v",)),
                ("flush16", F16, 196, ("small-v",))]


@pytest.mark.parametrize("defect,dt,N,fails_in", ATTN_DEFECTS, ids=[f"{d[0]}-{NAMES[d[1]]}-N{d[2]}" for d in ATTN_DEFECTS])
@pytest.mark.parametrize("order", ["v1", "v2"])
def test_attention_defect_passes_todays_inputs_and_fails_its_regime(defect, dt, N, fails_in, order):
    B, H = 2, 3
    for scale in G.attn_scales(H)[:1]:                  # attn_case calls at 1 / sqrt(H 64) only
        for seed in (40, 41, 42):                       # three of attn_case's draws
            qkv = today_attn_inputs(dt, B, N, H, seed)
            out, lse = G.emu_attn_fwd(qkv, B, N, H, scale, order, defect)
            today_attn_fwd(dt, qkv, out, lse, B, N, H, scale)      # raises if the defect showed
    for scale in G.attn_scales(H):
        qkv, dout = G.attn_inputs(dt, B, N, H, scale, 7)
        out, lse = G.emu_attn_fwd(qkv, B, N, H, scale, order, defect)
        worst = Collect()
        G.attn_check(worst, "d", f"{defect} N={N}", dt, qkv, dout, out, lse, None, B, N, H, scale, pshift=(order == "v2"))
        for name in fails_in:
            assert regime_fails(worst, f"-{name}-"), (defect, name, scale, worst.d)
        if defect != "flush16":           # (flushed probabilities also show on flat rows once scale = 0.125 spreads them over e^14)
            assert not regime_fails(worst, "-flat-"), "the control regime stays in bound"


def test_non_finite_output_counts_as_a_failure():
    """A NaN / inf where the reference is finite is a violation (kernel_check.check_bound: `~(err <= bound)`)."""
    B, N, H, scale = 2, 33, 3, 0.125
    qkv, dout = G.attn_inputs(F32, B, N, H, scale, 7)
    out, lse = G.emu_attn_fwd(qkv, B, N, H, scale, "v1", "nomax")
    assert not bool(torch.isfinite(out).all())
    worst = Collect()
    G.attn_check(worst, "d", "nomax", F32, qkv, dout, out, lse, None, B, N, H, scale)
    assert worst.d["d-offset+-out"] == math.inf and worst.errors


# ===================================================================================================================== LayerNorm
@pytest.mark.parametrize("dt", [F32, BF16, F16], ids=lambda d: NAMES[d])
@pytest.mark.parametrize("E", sorted(set(G.LN_E + G.LN_GENERIC_E)))
def test_layernorm_rows_reach_their_regimes_and_the_emulation_passes(dt, E):
    M = G.LN_M
    x, dy = G.ln_inputs(dt, M, E, 50 + E)
    gamma, beta = G.ln_params(E, 50 + E)
    names = G.ln_regimes(dt)
    worst = Collect()
    y, mean, rstd = G.emu_ln_fwd(x, gamma, beta)
    st = G.ln_check_fwd(worst, "ln", f"emulation {NAMES[dt]} E={E}", dt, x, gamma, beta, y, mean, rstd)
    dres = G._n((M, E), 999).to(dt)
    dx, dg, dbt = G.emu_ln_bwd(x, gamma, dy, mean, rstd, dres)
    G.ln_check_bwd(worst, "ln", f"emulation {NAMES[dt]} E={E}", dt, x, gamma, dy, mean, rstd, dx, dg, dbt, dres=dres)
    worst.report(f"emulated layernorm {NAMES[dt]} E={E}")
    assert not worst.errors, "\n".join(worst.errors[:8])
    top = G.EPS ** -0.5
    x64 = x.double()
    for i in range(M):
        nm = names[i % len(names)]
        rs, mu, var = float(st["rstd"][i]), float(st["mean"][i]), float(st["var"][i])
        if nm == "const":
            assert var == 0.0 and abs(rs - top) <= 1e-9 * top
        elif nm == "nearconst":
            assert (rs > 0.8 * top or E < 100) and var > 0 and bool(((x64[i] == 2.0) | (x64[i] == 2.0 + KC.ulp(torch.tensor(2.0), dt))).all())
        elif nm == "bigmean":
            assert (var == 0 and E < 100) or mu * mu / var > 1e4, (mu, var)
        elif nm == "outlier":
            assert float(x64[i].abs().max()) == 4096.0 and int((x64[i].abs() > 8).sum()) == 1
        elif nm == "tiny":
            assert var < 1e-10 and rs > 0.99 * top
        elif nm == "top":
            assert float(x64[i].abs().max()) <= 60000 and float(((x64[i] - mu) ** 2).max()) > 65504 or E < 16
    # the dy regime: on the rows proportional to x-hat the xh * c2 term carries the row
    cyc = ((torch.arange(M) // len(names)) % 2 == 1) & (st["var"] > 0)
    xh = (x64 - st["mean"][:, None]) * st["rstd"][:, None]
    gv = dy.double() * gamma.double()
    c1, c2 = gv.mean(1).abs(), (gv * xh).mean(1).abs()
    live = cyc & (st["var"] > 10 * G.EPS)
    assert int(live.sum()) >= 3 and bool((c2[live] > 3 * c1[live]).all())


# fp32 near-constant rows are 2.0 and 2.0 + 2^-22: their squares and sums are exact in fp32, so the one-pass form is exact there too and
# only the large-mean rows show it; in bf16 / fp16 the bumped rows' mean is not a power of two and both regimes show it.
# "sq16" (each centred square formed in fp16, summed in fp32: inf above 65504) is an fp16 sum of squares in the one form that
# passes today's rows, and only at E >= 768, where the 2^-11 of every square averages out below 1.4 E u; see the test after this one.
LN_DEFECTS = [("onepass", F32, ("bigmean",)), ("onepass", BF16, ("nearconst", "bigmean")),
              ("onepass", F16, ("nearconst", "bigmean")), ("noeps", F32, ("const",)), ("noeps", BF16, ("const",)),
              ("sq16", F16, ("top",))]


@pytest.mark.parametrize("defect,dt,fails_in", LN_DEFECTS, ids=[f"{d[0]}-{NAMES[d[1]]}" for d in LN_DEFECTS])
@pytest.mark.parametrize("E", [192, 768, 1024])
def test_layernorm_defect_passes_todays_inputs_and_fails_its_regime(defect, dt, fails_in, E):
    M = G.LN_M
    if defect == "sq16" and E < 768:
        return                                            # (the note above LN_DEFECTS)
    gamma, beta = G.ln_params(E, 3)
    for seed in (200, 201, 202):                          # ln_case: x = 2 randn + 0.5 (every row is "unit": regime labels are moot)
        g = torch.Generator().manual_seed(seed)
        x = (torch.randn(M, E, generator=g) * 2.0 + 0.5).to(dt)
        y, mean, rstd = G.emu_ln_fwd(x, gamma, beta, defect=defect)
        G.ln_check_fwd(KC.Worst(), "today", f"{defect} on ln_case's inputs", dt, x, gamma, beta, y, mean, rstd)     # raises if it showed
    x, _ = G.ln_inputs(dt, M, E, 60)
    y, mean, rstd = G.emu_ln_fwd(x, gamma, beta, defect=defect)
    worst = Collect()
    G.ln_check_fwd(worst, "d", defect, dt, x, gamma, beta, y, mean, rstd)
    for name in fails_in:
        assert regime_fails(worst, f"-{name}-"), (defect, name, worst.d)
    assert not regime_fails(worst, "-unit-"), "the control rows stay in bound"


def test_fp16_accumulated_sum_of_squares_fails_the_top_range_rows():
    """The sum of squares kept in an fp16 accumulator: inf on the top-range rows (rstd = 0 where the reference is 1e-4).  Unlike the
    defects above it does NOT pass ln_case's unit-scale rows either -- 192 fp16 additions lose 1e-3 of the sum against a bound of
    1.4 E u = 1.6e-5 on rstd -- so it is no evidence of the gap; "sq16" (fp16 squares, fp32 sum) is the variant that is."""
    E, M = 192, G.LN_M
    gamma, beta = G.ln_params(E, 3)
    x, _ = G.ln_inputs(F16, M, E, 60)
    y, mean, rstd = G.emu_ln_fwd(x, gamma, beta, defect="acc16")
    worst = Collect()
    G.ln_check_fwd(worst, "d", "acc16", F16, x, gamma, beta, y, mean, rstd)
    assert regime_fails(worst, "-top-")
    g = torch.Generator().manual_seed(200)
    x = (torch.randn(M, E, generator=g) * 2.0 + 0.5).to(F16)
    y, mean, rstd = G.emu_ln_fwd(x, gamma, beta, defect="acc16")
    worst = Collect()
    G.ln_check_fwd(worst, "d", "acc16", F16, x, gamma, beta, y, mean, rstd)
    assert worst.errors, "today's rstd bound already rejects an fp16 accumulator"


# ============================================================================================================ block parameters
@pytest.mark.parametrize("depth,seed,e,heads", [(1, 1, 192, 3), (2, 1, 192, 3), (12, 3, 192, 3), (2, 1, 384, 6)])
def test_make_params_default_is_unchanged(depth, seed, e, heads):
    """`offset` left at its default: bit for bit the parameters every existing case gets.  Pinned against the values written
    out here from the recipe's own formula (seed base, scales), independent of the new branch."""
    a = R.make_params(depth, seed, e, heads)
    b = R.make_params(depth, seed, e, heads, offset=None)
    for pa, pb in zip(a, b):
        assert pa.keys() == pb.keys()
        for k in pa:
            assert pa[k].dtype == pb[k].dtype and torch.equal(pa[k], pb[k]), k
    s = 1000 * seed
    inner, sw = heads * 64, 0.07 * math.sqrt(192 / e)
    w = R._n((3 * inner, e), s + 5, sw)
    w[0:64] *= 4.0
    w[inner:inner + 64] *= 4.0
    assert torch.equal(a[0]["wqkv"], w.to(BF16)) and torch.equal(a[0]["bqkv"], R._n((3 * inner,), s + 6, 0.2))


@pytest.mark.parametrize("e,heads", [(192, 3), (384, 6)])
def test_make_params_offset_sets_the_logit_offset_through_the_parameters(e, heads):
    scale = 1.0 / math.sqrt(e)
    b0 = G.offset_k0(scale)
    for sign in (1, -1):
        P = R.make_params(1, 1, e, heads, offset=sign)[0]
        base = R.make_params(1, 1, e, heads)[0]
        inner = heads * 64
        for h in range(heads):
            assert not P["wqkv"][h * 64].any() and not P["wqkv"][inner + h * 64].any()
            assert float(P["bqkv"][h * 64]) == G.Q0 and float(P["bqkv"][inner + h * 64]) == sign * b0
        keep = torch.ones(3 * inner, dtype=torch.bool)
        keep[torch.arange(heads) * 64] = False
        keep[inner + torch.arange(heads) * 64] = False
        assert torch.equal(P["wqkv"][keep], base["wqkv"][keep]) and torch.equal(P["bqkv"][keep], base["bqkv"][keep])
        assert all(torch.equal(P[k], base[k]) for k in P if k not in ("wqkv", "bqkv"))
        # through one emulated block forward: every lse carries the offset
        A = R.emu_block_fwd(P, R.make_x0(2, e=e), 2)
        off = G.Q0 * b0 * scale
        lse = A["lse"].double() * sign
        # (head 0's q / k rows x 4 spread its logits by up to +-40 around the offset; the other heads stay within ln 196 + 3 of it)
        assert 90 <= off <= 180 and float(lse.min()) > 70 and float((lse - off).abs().max()) < 60, (off, lse.min(), lse.max())
        assert float((lse[:, 1:] - off).abs().max()) < 10


@pytest.mark.parametrize("sign", [1, -1])
def test_emulated_block_with_a_logit_offset_passes_the_stage_checks(sign):
    """block_ref's torch emulation of the one-launch block (fp32 accumulation, bf16 where the path stores) on the offset parameters
    passes every stage with logit=True and reaches the regime.  In bf16 the term is small next to u_P = 2^-8 (the plain ratios are
    printed); it is the fp32 kernels that need it (test_todays_out_bound_rejects_a_correct_fp32_kernel_in_the_offset_regimes)."""
    B = 2
    P = R.make_params(1, 1, offset=sign)[0]
    A = R.emu_block_fwd(P, R.make_x0(B), B)
    Gd = R.emu_block_bwd(P, A, R.make_dy(B), B)
    worst = Collect()
    info = R.check_block_fwd(worst, "offset emulation", P, A, B, logit=True)
    R.check_block_bwd(worst, "offset emulation", P, A, Gd, B, logit=True)
    worst.finish(f"emulated block, offset {sign:+d}")
    assert info["lse_absmin"] > 70 and info["onehot_rows"] >= B * R.NTOK // 10
    plain = Collect()
    R.check_block_fwd(plain, "offset emulation, no logit term", P, A, B)
    print("without the logit term:", {k: round(v, 3) for k, v in plain.d.items() if k in ("attn", "lse")})


def test_todays_out_bound_rejects_a_correct_fp32_kernel_in_the_offset_regimes():
    """Why the bound form grows a term instead of ATTN_C growing: at |raw score| ~ 2000 the rounding of the 64-term dot product
    (64 u |q|.|k| scale ~ 1e-3 scaled units) shows through the softmax, and a correct max-subtracted fp32 emulation exceeds
    ulp + 2.5 N u P|v| several times over on the offset pairs while it sits far inside it on the flat ones."""
    B, N, H = 2, 33, 3
    worst_ratio = 0.0
    for scale in G.attn_scales(H):
        qkv, _ = G.attn_inputs(F32, B, N, H, scale, 7)
        out, lse = G.emu_attn_fwd(qkv, B, N, H, scale, "v1")
        f = G.attn_fwd_ref(qkv, B, N, H, scale)
        err = (G.heads(out, B, N, H)[0].double() - f["out"]).abs()
        ratio = (err / (KC.ulp(f["out"], F32) + R.ATTN_C["out"] * N * U * f["outmag"])).amax((-1, -2))
        reg = G.pair_regimes(B, H)
        off = ratio[(reg == 2) | (reg == 3)]
        assert float(off.max()) > 2 and float(ratio[reg == 0].max()) < 0.5, ratio
        worst_ratio = max(worst_ratio, float(off.max()))
    print(f"today's out bound, fp32 emulation, offset pairs: worst ratio {worst_ratio:.3g}")
