"""CPU tests of the machinery behind tests/test_swin_value_regimes.py (no GPU; tests/swin_regime_ref.py):
- win_case's new keywords left at their defaults give the tensors of the recipe before them, bit for bit;
- every builder reaches the regime it claims, with the conditions asserted from the fp64 reference and the oracle's shift mask;
- the fp64 reference equals autograd through oracle/swin_torch.window_attention on the regime inputs, rows below eps included,
  to 1e-10 of each row's magnitude; the unconditional projection (the reference and kernel before this file) does not;
- an fp32 / T emulation of a correct kernel, in two summation orders, passes every regime and dtype at c = 1;
- seeded defects PASS three draws of today's win_inputs under today's WIN_C and FAIL their regime.

Worst |err| / bound of the emulation at c = 1 (pytest -s prints them; the larger of the two orders and of shift 0 / 4),
out / lse / dq / dk / dv / d(scale) partial:
    fp32  control .05/.13/.05/.05/.11/.001  aligned .05/.12/.06/.07/.12/.003  signed .03/.12/.004/.01/.10/.001
          degenerate .06/.14/.06/.07/.14/.004  extremes .04/.12/.04/.05/.10/.003  small-v .04/.12/.06/.05/.11/.003  d(bias) .09
    bf16  control .36/.26/.31/.27/.43/.02  aligned .38/.28/.37/.31/.44/.01  signed .31/.26/.003/.05/.44/.0001
          degenerate .65/.25/.60/.47/.66/.02  extremes .32/.32/.27/.28/.40/.02  small-v .38/.27/.27/.35/.45/.02  d(bias) .35
    fp16  control .31/.24/.28/.31/.39/.03  aligned .37/.26/.33/.34/.48/.03  signed .27/.17/.0002/.05/.38/.00003
          degenerate .66/.31/.49/.49/.56/.04  extremes .35/.27/.50/.50/.48/.02  small-v .47/.24/.09/.06/.50/.02  d(bias) .31
No term had to be added: nothing exceeds 0.66.  fp16, 12 windows x 5 heads: of the 5120 own-row gradient elements of the zero q
rows 5107 lie beyond 65504 by more than the bound (the emulation holds +-inf of the reference's sign on each) and 13 straddle
it; of the zero k rows' 5120, 4067 and 1053.
Defects (test_defect_passes_todays_inputs_and_fails_its_regime): no max subtraction, the -inf mask, 1 / (|x| + eps), the unclamped rsq
and the unconditional projection each pass three draws of today's inputs under WIN_C and fail their regime, in every dtype listed.
The projection and 1 / (|x| + eps) show in bf16 through the rows of norm 0.3 eps only (the 2^-50 rows differ by |n|^2 = 2.5e-5).
Three defects do not pass today's fp16 inputs in the first place: test_fp16_defects_that_todays_inputs_already_reject has the figures.
"""
import math
import types

import pytest
import torch
import torch.nn.functional as F

import kernel_check as KC
import swin_ref as R
import swin_regime_ref as G
import test_swin_edges as E
from kernel_check import U, nan_padded
from oracle import swin_torch as ST
from swin_regime_ref import BF16, F16, F32, NAMES, REGIMES

DTS = [F32, BF16, F16]
ids = lambda d: NAMES[d]                                                  # noqa: E731
S100 = 3                                                                  # the head with s = 100 (5 heads)


def old_win_inputs(dt, B, res, heads, seed, DEV):
    """tests/test_swin_edges.py win_inputs as it stood before win_case took caller inputs (a copy, on DEV)."""
    C = heads * 32
    N = B * res * res
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.randn((N, 3, heads, 32), generator=g, device=DEV)
    x[:, :2] *= 10.0 ** (torch.rand((N, 2, heads, 1), generator=g, device=DEV) * 4 - 2)
    qkv = nan_padded(x.reshape(N, 3 * C).to(dt), extra_rows=7)
    dout = nan_padded(torch.randn((N, C), generator=g, device=DEV).to(dt), extra_rows=5)
    bias = torch.rand((heads, 64, 64), generator=g, device=DEV) * 16
    bias[:, ::7, ::5] = 15.999
    bias[:, 1::9, 2::11] = 1e-3
    bias = nan_padded(bias.reshape(heads * 64, 64), extra_rows=64).view(heads, 64, 64)
    scale = nan_padded(torch.tensor([E.SCALES[(h + seed) % len(E.SCALES)] for h in range(heads)], device=DEV).view(heads, 1),
                       extra_rows=3).view(heads)
    return qkv, dout, bias, scale


@pytest.mark.parametrize("dt", DTS, ids=ids)
def test_default_win_case_recipe_is_unchanged(dt):
    """win_inputs, which win_case calls when qkv / dout / bias / scale are left at None, against the copy above: the same bits,
    storage behind the views included; c = None keeps WIN_C and check = None keeps win_check."""
    import inspect
    for B, res, heads, seed in ((1, 8, 3, 700), (2, 16, 5, 710), (2, 24, 6, 730)):
        new, old = E.win_inputs(dt, B, res, heads, seed, device="cpu"), old_win_inputs(dt, B, res, heads, seed, "cpu")
        for a, b in zip(new, old):
            assert a.dtype == b.dtype and a.shape == b.shape and a.stride() == b.stride()
            assert torch.equal(E.bits(a), E.bits(b))
            assert a._base.shape == b._base.shape and torch.equal(E.bits(a._base), E.bits(b._base))      # the NaN rows behind
    sig = inspect.signature(E.win_case).parameters
    assert all(sig[k].default is None for k in ("qkv", "dout", "bias", "scale", "c", "check"))
    assert inspect.signature(E.win_inputs).parameters["device"].default == E.DEV
    assert inspect.signature(E.win_check).parameters["c"].default is None
    assert E.WIN_C[BF16]["out"] == 0.78 and E.WIN_C[F32]["dbias"] == 1.8 and E.WIN_C[F16]["dsp"] == 0.10


def _ref(dt, B, res, heads, shift, d):
    C = heads * 32
    xw = R.partition(d["qkv"].double(), B, res, shift)
    q, k, v = (R.split_heads(xw[..., i * C:(i + 1) * C], heads) for i in range(3))
    mask = R.window_mask(res, shift, B, "cpu")
    uT = KC.U_OF[dt]
    Lg, out, lse, P, _, _ = R.win_fwd(q, k, v, d["bias"].double(), d["scale"].double(), mask, uT, uT, E.ETA[dt])
    return q, k, v, mask, Lg, out, lse, P


@pytest.mark.parametrize("dt", DTS, ids=ids)
@pytest.mark.parametrize("B,res,heads,shift", G.CASES)
def test_builders_reach_their_regimes(dt, B, res, heads, shift):
    d = G.win_regime_inputs(dt, B, res, heads, shift, 31)
    reg = d["reg"]
    nW = (res // 8) ** 2
    assert [float(s) for s in d["scale"]] == [0.5, 5.0, 30.0, 100.0, 2.0] and float(d["scale"][S100]) == 100.0
    assert set(reg.flatten().tolist()) == set(range(6)) and bool((reg[:, 0] == torch.arange(B * nW) % 6).all())
    for h in range(heads):
        assert set(reg[:, h].tolist()) == set(range(6)), "every head's d(bias) sum mixes all regimes"
    q, k, v, mask, Lg, out, lse, P = _ref(dt, B, res, heads, shift, d)
    if shift:
        m1 = ST.shift_mask(res, 8, shift)
        nreg = torch.tensor([len(set(r.tolist())) for r in G.regions(res, shift)])
        masked = (m1 != 0).any(-1).any(-1)
        assert nreg.tolist() == [1, 2, 2, 4] and masked.tolist() == [False, True, True, True]
        # every regime lands in a masked window; the 4-region corner window is signed on some head
        for ri in range(6):
            assert any(bool(masked[w % nW]) for w in range(B * nW) if bool((reg[w] == ri).any())), REGIMES[ri]
        corner = [w for w in range(B * nW) if nreg[w % nW] == 4]
        assert any(int(reg[w, h]) == 2 for w in corner for h in range(heads))
        assert any(int(reg[w, S100]) == 2 for w in corner), "and on the s = 100 head"
    x = d["qkv"]
    assert torch.equal(x.to(dt), x) and bool(torch.isfinite(x.float()).all())
    sel = lambda name: (reg == REGIMES.index(name)).nonzero().tolist()       # noqa: E731
    # aligned: cos = 1 exactly at the planted keys; on the s = 100 head exp(float32(logit)) = inf and P > 0.99 where unmasked
    seen = 0
    for w, h in sel("aligned"):
        for qi, kj, f in G.ALIGNED:
            assert torch.equal(k[w, h, kj], q[w, h, qi] * f)
            assert abs(float(Lg["cos"][w, h, qi, kj]) - 1.0) < 1e-15
            if h == S100 and (mask is None or float(mask[w, qi, kj]) == 0.0):
                lg = Lg["lg"][w, h, qi, kj]
                assert float(lg) >= 100.0 and math.isinf(float(torch.exp(lg.float()))) and float(P[w, h, qi, kj]) > 0.99
                seen += 1
    assert seen >= (8 if not shift else 0)
    # signed: cos = -+1; in masked windows at s = 100 every row puts > 0.99 of its mass on masked keys; unmasked: lse near -82
    for w, h in sel("signed"):
        c = Lg["cos"][w, h]
        assert float((c.abs() - 1).abs().max()) < 1e-15
        rg = G.regions(res, shift)[w % nW]
        same = rg[:, None] == rg[None]
        assert bool((c[same] < 0).all())
        opp = (rg[:, None] - rg[None]) % 2 == 1
        assert bool((c[opp] > 0).all())
        if h == S100:
            if mask is not None and bool((mask[w] != 0).any()):
                mass = (P[w, h] * (mask[w] != 0)).sum(-1)
                assert float(mass.min()) > 0.99, float(mass.min())
            else:
                assert -86 < float(lse[w, h].min()) and float(lse[w, h].max()) < -78, (lse[w, h].min(), lse[w, h].max())
    # degenerate rows
    t = torch.arange(64)
    nq, nk = q.norm(dim=-1), k.norm(dim=-1)
    for w, h in sel("degenerate"):
        assert bool((q[w, h, t % 4 == 0] == 0).all()) and bool((k[w, h, t % 4 == 1] == 0).all())
        assert bool((nq[w, h, t % 4 != 0] > 0).all()) and bool((nk[w, h, t % 4 != 1] > 0).all())
        if dt == F16:                       # cannot reach eps: subnormal rows instead
            sub = q[w, h, t % 4 == 2].abs()
            assert float(sub.max()) < 2.0 ** -14 and float(nq[w, h, t % 4 == 2].min()) > 1e-7
        else:
            for m, lo, hi in (((t % 8 == 2) & (t % 16 != 10), 1e-16, 1e-13), (t % 8 == 6, 1e-24, 1e-21), (t % 16 == 10, 2e-13, 5e-13)):
                assert lo < float(nq[w, h, m].min()) and float(nq[w, h, m].max()) < hi
                assert lo < float(nk[w, h, m].min()) and float(nk[w, h, m].max()) < hi
            n2 = (q[w, h, t % 8 == 6].float() ** 2).sum(-1)
            assert float(n2.max()) < 2.0 ** -140, "the fp32 sum of squares underflows"
    for n_ in (nq, nk):
        assert not bool(((n_ > R.EPS / 2) & (n_ < R.EPS * 2)).any())
    # norm extremes
    lo, hi = G.EXT_EXP[dt]
    for w, h in sel("extremes"):
        n2 = (q[w, h].float() ** 2).sum(-1)
        assert bool(torch.isfinite(n2).all())
        assert float(nq[w, h].max()) > 2.0 ** (hi - 1) and float(nq[w, h].min()) < 2.0 ** (lo + 4)
        if dt == F16:
            assert float(q[w, h].abs().max()) <= G.F16_TOP and float((q[w, h].float() ** 2).max()) > 65504
    for w, h in sel("small-v"):
        assert float(v[w, h].abs().max()) < 2.0 ** -13


class _Torch:
    def __init__(self, caught):
        self.caught = caught

    def __getattr__(self, name):
        return getattr(torch, name)

    def softmax(self, a, dim):
        self.caught["att"] = a
        return torch.softmax(a, dim)


class _F:
    """oracle/swin_torch's `F` with the qkv Linear replaced by the caller's leaf tensor (its gradient is dqkv in window layout)."""

    def __init__(self, leaf):
        self.leaf = leaf

    def __getattr__(self, name):
        return getattr(F, name)

    def linear(self, x, w, b=None):
        if w.shape[0] == self.leaf.shape[-1]:
            return self.leaf
        return F.linear(x, w, b)


@pytest.mark.parametrize("dt", [BF16, F16], ids=ids)
@pytest.mark.parametrize("B,res,heads,shift", G.CASES)
def test_reference_is_autograd_on_the_regime_inputs(monkeypatch, dt, B, res, heads, shift):
    """oracle/swin_torch.window_attention in fp64 under autograd on the regime inputs (the qkv Linear replaced by the inputs, the
    projection by the identity): out, dq, dk, dv, d(bias), d(scale) of tests/swin_ref.py agree to 1e-10 of each row's magnitude
    s mag(dS) |k^| / max(|q|, eps), mag(dS) = P (|dO||v|^T + |dO|.|O|).  With the projection applied below eps as well -- win_bwd(project_clamped=True), the reference
    and kernel before this file -- the rows below eps differ by |n|^2 relative; an exactly-zero row is the same in both forms."""
    C = heads * 32
    d = G.win_regime_inputs(dt, B, res, heads, shift, 31)
    leaf = R.partition(d["qkv"].double(), B, res, shift).clone().requires_grad_(True)
    pb = d["bias"].double().requires_grad_(True)
    ls = torch.log(d["scale"].double()).view(heads, 1, 1).requires_grad_(True)
    p = {"a.qkv.weight": torch.zeros(3 * C, C, dtype=torch.float64), "a.q_bias": torch.zeros(C, dtype=torch.float64),
         "a.v_bias": torch.zeros(C, dtype=torch.float64), "a.logit_scale": ls, "a.proj.weight": torch.eye(C, dtype=torch.float64),
         "a.proj.bias": torch.zeros(C, dtype=torch.float64)}
    caught = {}
    monkeypatch.setattr(ST, "position_bias", lambda *a: pb)
    monkeypatch.setattr(ST, "F", _F(leaf))
    monkeypatch.setattr(ST, "torch", _Torch(caught))
    o = ST.window_attention(p, "a.", torch.zeros(B, res * res, C, dtype=torch.float64), res, 8, shift, heads)
    w = d["dout"].double().reshape(B, res * res, C)
    (o * w).sum().backward()
    monkeypatch.undo()
    q, k, v, mask, Lg, out, lse, P = _ref(dt, B, res, heads, shift, d)
    nwin = B * (res // 8) ** 2
    merged = lambda t: t.permute(0, 2, 1, 3).reshape(nwin, 64, C)        # noqa: E731
    assert (R.reverse(merged(out), B, res, shift) - o.detach().reshape(-1, C)).abs().max() <= 1e-12 * out.abs().max()
    dO = R.split_heads(R.partition(d["dout"].double(), B, res, shift), heads)
    gq = leaf.grad
    auto = {nm: R.split_heads(gq[..., i * C:(i + 1) * C], heads) for i, nm in enumerate(("dq", "dk", "dv"))}
    s = Lg["s"]
    for proj_all in (False, True):
        r = R.win_bwd(Lg, v, dO, out, lse, U, 0.0, project_clamped=proj_all)
        # |dS| as a magnitude: P (|dO||v|^T + |dO|.|O|) -- on one-hot rows dP - D cancels and fp64 itself rounds at this size
        mdS = P * (dO.abs() @ v.abs().transpose(-1, -2) + (dO.abs() * out.abs()).sum(-1, keepdim=True))
        mag = {"dq": s * (mdS @ Lg["kh"].abs()) / Lg["nq"], "dk": s * (mdS.transpose(-1, -2) @ Lg["qh"].abs()) / Lg["nk"],
               "dv": P.transpose(-1, -2) @ dO.abs()}
        bad = {}
        for nm in ("dq", "dk", "dv"):
            tol = 1e-10 * mag[nm].amax(-1, keepdim=True) + 1e-300
            bad[nm] = ((r[nm] - auto[nm]).abs() > tol).any(-1)          # [nwin, heads, token]
        if not proj_all:
            assert not any(bool(b.any()) for b in bad.values()), {nm: int(b.sum()) for nm, b in bad.items()}
            assert (r["dS"].sum(0) - pb.grad).abs().max() <= 1e-10 * pb.grad.abs().max()
            dls = r["dsp"].sum(0) * d["scale"].double()
            assert (dls - ls.grad.view(-1)).abs().max() <= 1e-10 * ls.grad.abs().max()
        else:
            assert not bool(bad["dv"].any())
            for nm, c in (("dq", Lg["cq"]), ("dk", Lg["ck"])):
                below = c[..., 0] & ((q if nm == "dq" else k).norm(dim=-1) > 0)       # clamped by F.normalize and not exactly zero
                assert not bool((bad[nm] & ~below).any()), "only rows below eps differ"
                if dt == F16:
                    assert not bool(below.any())
                else:
                    first = below & (q.norm(dim=-1) > 1e-16 if nm == "dq" else k.norm(dim=-1) > 1e-16)       # the 2^-50 and 2^-44 rows
                    assert int(first.sum()) > 0 and bool(bad[nm][first].all()), "the projected form misses every 2^-50 and 2^-44 row"
                    rel = ((r[nm] - auto[nm]).abs().amax(-1) / mag[nm].amax(-1))[first]
                    print(f"{NAMES[dt]} shift {shift} {nm}: projected form off by {float(rel.min()):.3g} .. {float(rel.max()):.3g} "
                          f"of the row magnitude on {int(first.sum())} rows of norm 5e-15 / 3e-13 (|n|^2 = 2.5e-5 / 0.1)")


# ------------------------------------------------------------------------------------------------------ the emulation passes
def run_regime(dt, B, res, heads, shift, order, defect, seed=31):
    d = G.win_regime_inputs(dt, B, res, heads, shift, seed)
    outs = G.emulate(dt, B, res, heads, shift, d["qkv"], d["dout"], d["bias"], d["scale"], order, defect)
    worst = G.Collect()
    gb = R.geometry(G.ESZ[dt], "bwd", B, res, heads, 256, 1)
    counts = G.win_regime_check(worst, dt, B, res, heads, shift, d["qkv"], d["dout"], d["bias"], d["scale"], *outs, gb,
                                f"emulation {NAMES[dt]} {order} {defect} shift={shift}")
    return worst, counts


@pytest.mark.parametrize("dt", DTS, ids=ids)
@pytest.mark.parametrize("order", ["lanes", "flat"])
def test_emulated_correct_kernel_passes_every_regime_at_c1(dt, order):
    for B, res, heads, shift in G.CASES:
        worst, counts = run_regime(dt, B, res, heads, shift, order, None)
        worst.report(f"emulated window attention {NAMES[dt]} {order} shift={shift}")
        print("counts:", counts)
        assert not worst.errors, "\n".join(worst.errors[:8])
        assert max(worst.d.values()) <= 1.0
        over = sum(v for k_, v in counts.items() if k_.endswith(("-dq", "-dk", "-edge")))
        assert (over > 0) == (dt == F16), "fp16 and only fp16 has own-row gradients of zero rows beyond its range"
        assert counts["zero"] > 0 and (counts["clamped"] > 0) == (dt != F16)


# ------------------------------------------------------------------------------------------------------------ seeded defects
def today(dt, defect, order="lanes"):
    """Three draws of today's win_inputs (B = 2, res 16, 5 heads, shift 4) through the emulation with the defect and today's
    win_check under WIN_C: None if all pass, else the first violation."""
    B, res, heads, shift = 2, 16, 5, 4
    ns = types.SimpleNamespace
    for seed in (700, 710, 720):
        qkv, dout, bias, scale = E.win_inputs(dt, B, res, heads, seed, device="cpu")
        out, lse, dqkv, dbias, dsp, dsc = G.emulate(dt, B, res, heads, shift, qkv, dout, bias, scale, order, defect)
        gb = R.geometry(G.ESZ[dt], "bwd", B, res, heads, 256, 1)
        try:
            E.win_check(dt, B, res, heads, shift, qkv, dout, bias, scale, ns(t=out), ns(t=lse), ns(t=dqkv), ns(t=dbias), ns(t=dsp),
                        ns(t=dsc), gb, E.Fit(), f"today {defect} seed {seed}")
        except AssertionError as e:
            return str(e)[:300]
    return None


def fails(worst, regime):
    return sorted(k for k, v in worst.d.items() if f"-{regime}-" in k and v > 1)


DEFECTS = [("nomax", F32, "aligned"), ("nomax", BF16, "aligned"), ("nomax", F16, "aligned"), ("infmask", F32, "signed"),
           ("infmask", BF16, "signed"), ("infmask", F16, "signed"), ("addeps", F32, "degenerate"), ("addeps", BF16, "degenerate"),
           ("rsq", F32, "degenerate"), ("rsq", BF16, "degenerate"), ("rsq", F16, "degenerate"), ("proj", F32, "degenerate"),
           ("proj", BF16, "degenerate")]


@pytest.mark.parametrize("defect,dt,regime", DEFECTS, ids=[f"{d[0]}-{NAMES[d[1]]}" for d in DEFECTS])
def test_defect_passes_todays_inputs_and_fails_its_regime(defect, dt, regime):
    assert today(dt, None) is None, "the emulation of a correct kernel passes today's test"
    assert today(dt, defect) is None, f"{defect} passes today's inputs under today's WIN_C: the gap"
    hit = []
    for B, res, heads, shift in G.CASES:
        worst, _ = run_regime(dt, B, res, heads, shift, "lanes", defect)
        hit += fails(worst, regime)
        if defect not in ("infmask",) or not shift:
            assert not fails(worst, "control"), (defect, worst.d)
    print(defect, NAMES[dt], "fails", sorted(set(hit)))
    assert hit, (defect, regime)
    if defect == "infmask":
        worst, _ = run_regime(dt, 3, 16, 5, 0, "lanes", defect)
        assert not worst.errors, "without a shift there is no mask to get wrong"


def test_fp16_defects_that_todays_inputs_already_reject():
    """Three of the listed defects do NOT pass today's win_inputs in fp16, so they are no evidence of the gap; the regimes reject
    them as well, and differently from what was expected in one case (figures: B = 2, res 16, 5 heads, shift 4, seed 700).
    - squares formed in fp16 ("sq16"): today's norms of 10^+-2 put elements up to 450 into q and k, whose squares pass 65504:
      1 / |x| = 0 on those rows and 1959 of 81920 out elements leave today's bound (worst ratio 558).  It fails the top of the
      norm extremes (and every regime built on win_inputs' recipe).
    - 16-bit operands below 2^-14 flushed ("flush16") and P flushed below fp16's normal range before P V ("pflush"): 9 of 81920
      out elements leave today's bound, worst ratio 3.99 -- rows of the s = 5 and s = 30 heads with mass on keys of P < 2^-14.
      flush16 fails the fp16 degenerate rows (the subnormal rows become zero rows) and small-v (v itself is flushed).  pflush
      does NOT fail small-v: there out is subnormal in fp16 and its ulp, 2^-24, is 2^-7 of |out|, while the flushed mass is at
      most 63 x 2^-14 = 2^-8; it shows on dv of the unit-scale regimes instead.  In bf16 and fp32 "below the normal range"
      means P < 2^-126, which exp2 has flushed already (the bound's 2^-126 term): no defect, every check passes."""
    for defect in ("sq16", "flush16", "pflush"):
        assert today(F16, None) is None and today(F16, defect) is not None, defect
    case = G.CASES[1]
    assert fails(run_regime(F16, *case, "lanes", "sq16")[0], "extremes")
    w = run_regime(F16, *case, "lanes", "flush16")[0]
    assert fails(w, "degenerate") and fails(w, "small-v")
    w = run_regime(F16, *case, "lanes", "pflush")[0]
    print("pflush f16:", {k: v for k, v in w.d.items() if v > 1})
    assert not fails(w, "small-v") and "f16-control-dv" in fails(w, "control")
    for dt in (F32, BF16):
        assert today(dt, "pflush") is None and not run_regime(dt, *case, "lanes", "pflush")[0].errors


@pytest.mark.parametrize("esz", [2, 4])
def test_multi_window_case_at_256_compute_units(esz):
    """The search the GPU file runs on the device's CU count, at 256: both directions walk >= 3 windows per wave with a ragged
    last range, at win_xcd 1 and 0, and the case holds every regime on every head."""
    B, res, heads = G.multi_window_case(esz, 256)
    for d in ("fwd", "bwd"):
        for x in (1, 0):
            g = R.geometry(esz, d, B, res, heads, 256, x)
            assert g["wpw_min"] >= 3 and g["nwin"] % g["wph"] and not g["capped"], (d, x, g)
    reg = G.pair_regimes(B * (res // 8) ** 2, heads)
    assert all(set(reg[:, h].tolist()) == set(range(6)) for h in range(heads))
    print(f"esz {esz}: B={B} res={res} heads={heads}: {reg.numel()} (window, head) pairs")

