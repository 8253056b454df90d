"""CPU tests of the machinery behind tests/test_step_ends.py (no GPU, no rgb_no_more_amd kernel):
- every fp64 reference of tests/step_ends_ref.py is anchored to an independent implementation, to 1e-12 relative in fp64;
- an fp32 emulation of each kernel's operation order (256 strided partial sums, wave and four-way combines, libm exp / log)
  runs on the inputs of the GPU cases and has to satisfy the very check functions the GPU test calls: the inputs and the
  bounds are compatible.  This is measured on the reference side, never on a kernel;
- defects that the suite's older bars let pass are seeded into the emulation and have to be rejected by those checks;
- a Python copy of each launcher's grid formula asserts that the committed case lists reach the regimes they claim.
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

import kernel_check as KC
import step_ends_ref as R
from oracle import vit_torch as V
from step_ends_ref import F32, BF16, F16, NAMES, cdiv

RTOL = 1e-12


def close(a, b, what):
    a, b = a.double(), b.double()
    err = float((a - b).abs().max())
    scale = float(b.abs().max()) + 1e-300
    assert err <= RTOL * scale, f"{what}: max |diff| {err:.3g} at scale {scale:.3g}"


# ================================================================================================ anchors of the references
@pytest.mark.parametrize("kind", ["hard", "soft", "mix"])
def test_ref_cross_entropy_matches_torch(kind):
    B, C = 37, 53
    z = R.sx_logits(B, C, "n3", 1)
    zz = z.double().requires_grad_(True)
    if kind == "hard":
        lab = R.sx_labels(B, C, 2)
        t = Fn.one_hot(lab, C).double()
        loss = Fn.cross_entropy(zz, lab)
    elif kind == "soft":
        t = torch.softmax(R.randn((B, C), 3).double(), 1)                # mass 1: torch's soft-target loss assumes nothing else
        loss = Fn.cross_entropy(zz, t)
    else:
        lab = R.sx_labels(B, C, 2, equal_neighbours=True)
        lam = R.lam_pair(4)
        oh = Fn.one_hot(lab, C).double()
        t = float(lam[0]) * oh + float(lam[1]) * oh.roll(1, 0)
        close(R.mixup_target_ref(lab, lam, C), t, "mixed target")        # (fp32 sums of two fp32 numbers: exact here or not,
        t = R.mixup_target_ref(lab, lam, C).double()                     #  the reference consumes the fp32 target)
        loss = Fn.cross_entropy(zz, t)
    loss.backward()
    g = R.f32(0.37 / B)
    r = R.softxent_ref(z, t, g)
    close(r["loss"], loss.detach(), "loss")
    close(r["rows"], -(t * torch.log_softmax(z.double(), 1)).sum(1), "rows")
    if kind != "mix":
        close(r["dl"], zz.grad * B * g, "dlogits")
    close(r["lse"], torch.logsumexp(z.double(), 1), "lse")
    if kind == "mix":                                                    # mass lam0 + lam1 is 1 only up to fp32 rounding
        tt = t / t.sum(1, keepdim=True)
        z2 = z.double().requires_grad_(True)
        Fn.cross_entropy(z2, tt).backward()
        close(R.softxent_ref(z, tt, g)["dl"], z2.grad * B * g, "dlogits mix")


def test_ref_cross_entropy_mass_not_one():
    """rows = lse T - sum t z and dl = (p T - t) g for a row of mass 0.9: the gradient of the row's loss by autograd."""
    z = R.sx_logits(5, 11, "n3", 5)
    t = R.sx_soft_target(5, 11, 6).double()
    zz = z.double().requires_grad_(True)
    rows = -(t * torch.log_softmax(zz, 1)).sum(1)
    rows.sum().backward()
    r = R.softxent_ref(z, t, 1.0)
    close(r["rows"], rows.detach(), "rows")
    close(r["dl"], zz.grad, "dlogits")
    assert abs(float(t[2].sum()) - 0.9) < 1e-6


@pytest.mark.parametrize("step,max_norm", [(1, 1.0), (2, 0.0), (1000, 1.0), (7, 100.0)])
def test_ref_adamw_matches_torch_optim_and_oracle(step, max_norm):
    from rgb_no_more_amd.custom_optims import WeightDecay
    sizes, decay = [256, 768, 512, 256], [1, 0, 1, 0]
    n = sum(sizes)
    h = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, wd_factor=0.05)
    p0, m0, v0, _ = R.adam_state(n, 11)
    g0 = R.adam_grad(n, 1.0 if max_norm != 100.0 else 0.01, 12)
    flags = torch.tensor(sum(([d] * (s // 256) for s, d in zip(sizes, decay)), []), dtype=torch.uint8)
    r = R.adamw_ref(p0, g0, m0, v0, flags, step, max_norm, exact_scalars=True, **h)
    ps = [t.clone().double().requires_grad_(True) for t in p0.split(sizes)]
    for p, g in zip(ps, g0.double().split(sizes)):
        p.grad = g.clone()
    if max_norm > 0:
        norm = torch.nn.utils.clip_grad_norm_(ps, max_norm)
        close(r["norm"], norm, "norm")
    opt = torch.optim.AdamW(ps, lr=h["lr"], betas=(h["beta1"], h["beta2"]), eps=h["eps"], weight_decay=0.0)
    for p, m, v in zip(ps, m0.double().split(sizes), v0.double().split(sizes)):
        opt.state[p] = dict(step=torch.tensor(float(step - 1)), exp_avg=m.clone(), exp_avg_sq=v.clone())
    opt.step()
    wd = WeightDecay([p for p, d in zip(ps, decay) if d], lr=h["lr"], weight_decay=h["wd_factor"])
    wd.step()
    close(r["p"], torch.cat([p.detach() for p in ps]), "p vs torch.optim")
    close(r["m"], torch.cat([opt.state[p]["exp_avg"] for p in ps]), "m vs torch.optim")
    close(r["v"], torch.cat([opt.state[p]["exp_avg_sq"] for p in ps]), "v vs torch.optim")
    # the oracle's restatement (numpy, float64); its max_norm has no "off": compared where clipping is on
    if max_norm > 0:
        P = [t.double().numpy().copy() for t in p0.split(sizes)]
        M = [t.double().numpy().copy() for t in m0.split(sizes)]
        Vv = [t.double().numpy().copy() for t in v0.split(sizes)]
        G = [t.double().numpy() for t in g0.split(sizes)]
        tot = V.clip_adamw_wd_step(P, G, M, Vv, step, h["lr"], h["lr"], h["wd_factor"], decay, max_norm=max_norm,
                                   beta1=h["beta1"], beta2=h["beta2"], eps=h["eps"])
        assert abs(tot - float(r["norm"])) <= 1e-12 * tot
        # (the oracle rounds coef to fp32 before it scales the gradient: 6e-8 relative when clipping is active)
        tol = 1e-12 if r["coef"] == 1.0 else 2e-7
        for got, want, nm in ((r["p"], P, "p"), (r["m"], M, "m"), (r["v"], Vv, "v")):
            w = torch.from_numpy(np.concatenate(want))
            assert float((got - w).abs().max()) <= tol * float(w.abs().max()), nm


def test_ref_adamw_fp32_scalars_are_the_launchers():
    """bc1 / bc2_sqrt as the launcher rounds them, 1.f - beta as an fp32 difference: a step differs from the exact-scalar one by
    fp32 rounding of the scalars only."""
    n = 512
    p0, m0, v0, fl = R.adam_state(n, 21)
    g0 = R.adam_grad(n, 1.0, 22)
    a = R.adamw_ref(p0, g0, m0, v0, fl, 3, 1.0, **R.ADAM_HYPER)
    b = R.adamw_ref(p0, g0, m0, v0, fl, 3, 1.0, exact_scalars=True, **R.ADAM_HYPER)
    d = float((a["p"] - b["p"]).abs().max())
    assert 0 < d <= 1e-6                    # (beta2 = 0.999 in fp32 moves 1 - beta2 by 1.3e-5 relative; the update is ~1e-3)
    assert R.f32(1.0 - R.f32(0.999)) != 1.0 - 0.999


def test_ref_embed_matches_oracle_and_golden(golden):
    from rgb_no_more_amd import detfill
    for (B, Hb, Wb, tr) in [(2, 4, 6, 0), (3, 6, 2, 0), (1, 8, 8, 0)]:
        y, c = R.embed_inputs(B, Hb, Wb, F32, "dct", 31)
        A = V.conv_matrix(16)
        luma, mag, _, chroma = R.embed_ref(y, c, A, tr)
        want = V.subblock_features(y.double(), c.double()).reshape(-1, 384)
        close(luma, want[:, :256], "luma vs oracle")
        assert torch.equal(chroma, want[:, 256:])
        lt, _, _, _ = R.embed_ref(y, c, A.T.contiguous(), True)
        close(lt, luma, "transpose_a")
        assert bool((mag >= luma.abs() * (1 - 1e-12)).all())
    g = golden("g9_subblock.npz")
    y = torch.from_numpy(detfill.normalish((2, 1, 4, 6, 8, 8), 61))
    c = torch.from_numpy(detfill.normalish((2, 2, 2, 3, 8, 8), 62))
    A = torch.from_numpy(g["convY"])
    luma, _, _, chroma = R.embed_ref(y, c, A, False)
    ref = torch.from_numpy(g["feat"]).reshape(12, 384).double()
    assert torch.equal(chroma, ref[:, 256:])
    assert float((luma - ref[:, :256]).abs().max()) < 5e-6               # the golden itself was computed in fp32


def test_ref_mixup_matches_roll():
    x = R.randn((7, 40), 41).to(BF16)
    lam = R.lam_pair(42)
    ref, mag, rt = R.mixup_ref(x, lam, BF16)
    l0, l1 = float(lam[0]), float(lam[1])
    close(ref, l0 * x.double() + l1 * torch.roll(x.double(), 1, 0), "mixup")
    assert rt.dtype == BF16
    lo, hi = R.mix_fp32(x, lam)
    assert float((lo.double() - ref).abs().max()) <= 2 * KC.U * float(mag.max())
    assert int((lo != hi).sum()) == 0
    lab = torch.tensor([3, 3, 0, 9])
    t = R.mixup_target_ref(lab, lam, 10)
    oh = Fn.one_hot(lab, 10).float()
    assert torch.equal(t, oh * lam[0] + oh.roll(1, 0) * lam[1])
    assert float(t[1, 3]) == float(lam[0] + lam[1])


def test_ref_pool_matches_layer_norm_and_autograd():
    B, N, E, eps = 3, 9, 192, 1e-5
    x, gamma, beta, dp = R.pool_inputs(B, N, E, F32, True, 51)
    xx = x.double().requires_grad_(True)
    gg, bb = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    pooled = Fn.layer_norm(xx, (E,), gg, bb, eps).mean(1)
    pooled.backward(dp.double())
    pref, pmag, mu, rs, ax = R.pool_fwd_ref(x, gamma, beta, eps)
    close(pref, pooled.detach(), "pooled")
    close(mu, x.double().mean(2), "mean")
    close(rs, 1 / torch.sqrt(x.double().var(2, unbiased=False) + eps), "rstd")
    dx, _, dg, _, db, _ = R.pool_bwd_ref(dp, x, gamma, mu, rs)
    assert float((dx - xx.grad).abs().max()) <= 1e-10 * float(xx.grad.abs().max())     # (cancellation at mean 100)
    close(dg, gg.grad, "dgamma")
    close(db, bb.grad, "dbeta")


# ================================================================================================= fp32 emulations
def strided_sum(x):
    """The kernels' row sum: 256 strided partial sums in element order, a wave reduction by halves, the four waves in order.
    x [R, n] fp32 -> [R]."""
    Rr, n = x.shape
    K = cdiv(n, 256)
    xp = torch.zeros(Rr, K * 256, dtype=F32)
    xp[:, :n] = x
    xp = xp.view(Rr, K, 256)
    acc = torch.zeros(Rr, 256, dtype=F32)
    for k in range(K):
        acc = acc + xp[:, k]
    w = acc.view(Rr, 4, 64)
    for h in (32, 16, 8, 4, 2, 1):
        w = w[..., :h] + w[..., h:2 * h]
    w = w[..., 0]
    return ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]


def sx_emul(z, t, g, dt, defect=None):
    """softxent_loss_kernel + softxent_grad_kernel in fp32 with libm exp / log.  defect 'lse': lse one bf16 ulp off; 'mass':
    the target mass taken as 1."""
    B = z.shape[0]
    m = z.amax(1)
    se = strided_sum(torch.exp(z - m[:, None]))
    st = strided_sum(t)
    stz = strided_sum(t * z)
    lse = m + torch.log(se)
    if defect == "lse":
        lse = lse * (1 + 2.0 ** -8)
    if defect == "mass":
        st = torch.ones_like(st)
    rows = lse * st - stz
    loss = strided_sum(rows[None, :])[0] / B
    dl = ((torch.exp(z - lse[:, None]) * st[:, None] - t) * torch.tensor(g, dtype=F32)).to(dt)
    return dict(lse=lse, T=st, rows=rows, loss=loss, dl=dl)


def sqnorm_emul(g, drop_last=False):
    n = g.numel()
    S = cdiv(n, R.NORM_STRIDE)
    gp = torch.zeros(S * R.NORM_STRIDE, dtype=F32)
    gp[:n] = g
    gp = gp.view(S, R.NORM_STRIDE // 4, 4)
    acc = torch.zeros(R.NORM_STRIDE // 4, dtype=F32)
    for s in range(S - 1 if drop_last else S):
        q = gp[s] * gp[s]
        acc = acc + (((q[:, 0] + q[:, 1]) + q[:, 2]) + q[:, 3])
    part = strided_sum(acc.view(256, 256))
    return torch.sqrt(strided_sum(part[None, :])[0])


def adam_emul(p, g, m, v, flags, step, max_norm, lr, beta1, beta2, eps, wd_factor, defect=None):
    """sqnorm_kernel + adamw_kernel in fp32, operation by operation.  defect 'stride': the last stride of the norm dropped;
    'flag': the decay flag of chunk 1 ignored."""
    t = lambda x: torch.tensor(x, dtype=F32)
    total = sqnorm_emul(g, drop_last=(defect == "stride"))
    mn = t(max_norm)
    c = mn / (total + t(1e-6)) if max_norm > 0 else t(1.0)
    coef = torch.minimum(c, t(1.0))
    b1, b2 = t(beta1), t(beta2)
    bc1 = t(1.0 - float(b1) ** step)
    bc2s = t(math.sqrt(1.0 - float(b2) ** step))
    stp = t(lr) / bc1
    gc = g * coef
    m1 = b1 * m + (t(1.0) - b1) * gc
    v1 = b2 * v + (t(1.0) - b2) * gc * gc
    p1 = p - stp * (m1 / (torch.sqrt(v1) / bc2s + t(eps)))
    fl = flags.clone()
    if defect == "flag":
        fl[1] = 0
    dec = fl.bool().repeat_interleave(256)
    p2 = torch.where(dec, p1 - t(wd_factor) * p1, p1)
    return dict(p=p2, m=m1, v=v1, norm=total)


def pool_fwd_emul(x, gamma, beta, eps, dt, defect=None):
    """pool_fwd_kernel in fp32: per-row two-pass statistics, each of the G row groups folding its rows in ascending order, the
    groups summed in order.  defect 'clamp': the clamped prefetch rows of the last turn folded in; 'moment': rstd from the
    uncentred second moment."""
    B, N, E = x.shape
    G = R.pool_rows(E)
    xf = x.float()
    mu = xf.sum(2, keepdim=True) * F32_(1.0 / E)
    if defect == "moment":
        var = (xf * xf).sum(2, keepdim=True) * F32_(1.0 / E) - mu * mu
    else:
        var = ((xf - mu) ** 2).sum(2, keepdim=True) * F32_(1.0 / E)
    rs = 1.0 / torch.sqrt(var + F32_(eps))
    xh = (xf - mu) * rs
    span = R.POOL_FWD_UNR * G
    Np = cdiv(N, span) * span
    xp = torch.zeros(B, Np, E, dtype=F32)
    xp[:, :N] = xh
    if defect == "clamp":
        xp[:, N:] = xh[:, N - 1:N]
    xp = xp.view(B, Np // G, G, E)
    acc = torch.zeros(B, G, E, dtype=F32)
    for k in range(Np // G):
        acc = acc + xp[:, k]
    a = torch.zeros(B, E, dtype=F32)
    for r in range(G):
        a = a + acc[:, r]
    pooled = (a * F32_(1.0 / N) * gamma + beta).to(dt)
    return pooled, mu.reshape(-1), rs.reshape(-1)


def F32_(x):
    return torch.tensor(x, dtype=F32)


def pool_bwd_emul(dp, x, gamma, mean, rstd, init, dt):
    B, N, E = x.shape
    xf = x.float()
    d = (dp.float() * F32_(1.0 / N))[:, None, :]
    mu, rs = mean.view(B, N, 1), rstd.view(B, N, 1)
    xh = (xf - mu) * rs
    gv = d * gamma
    c1 = gv.sum(2, keepdim=True) * F32_(1.0 / E)
    c2 = (gv * xh).sum(2, keepdim=True) * F32_(1.0 / E)
    dx = (rs * (gv - c1 - xh * c2)).to(dt)
    part = torch.zeros(B, E, dtype=F32)
    for tkn in range(N):
        part = part + d[:, 0] * xh[:, tkn]
    dg, db = torch.zeros(E, dtype=F32), torch.zeros(E, dtype=F32)
    for b in range(B):
        dg = dg + part[b]
        db = db + dp[b].float()
    if init is not None:
        dg, db = dg + init[0].float(), db + init[1].float()
    return dx.reshape(B * N, E), dg, db


def embed_emul(y, c, A, tr, lam, TI, TO, defect=None):
    """subblock_embed_kernel in fp32: gather, mix (the fp32 product and fma, rounded to TI), two fp32 matrix products.  defect
    'roll': the partner is image b + 1; 'position': at b = 0 the partner (image B - 1) is taken from the previous position of
    the patch list instead of the same one."""
    B = y.shape[0]
    X = R.gather_x(y.float())
    shape = X.shape
    npos = shape[1] * shape[2]
    X = X.reshape(B, npos, 256)
    Cq = c.float().permute(0, 2, 3, 1, 4, 5).reshape(B, npos, 128)
    if lam is not None:
        def mix(a):
            p = a.roll(-1 if defect == "roll" else 1, 0)
            if defect == "position":
                p = p.clone()
                p[0] = a[B - 1].roll(1, 0)
            return (p.double() * lam[1].double() + (a * lam[0]).double()).float().to(TI).float()
        X, Cq = mix(X), mix(Cq)
    Af = A.float()
    Af = Af.T if tr else Af
    Z = (Af @ X.reshape(shape)) @ Af.T
    return torch.cat([Z.reshape(B * npos, 256), Cq.reshape(B * npos, 128)], 1).to(TO)


# ================================================================================================= accept: honest arithmetic
@pytest.mark.parametrize("TI,TO", R.EMBED_PAIRS, ids=lambda t: NAMES[t])
def test_bounds_accept_embed_emulation(TI, TO):
    worst = KC.Worst()
    j = R.EMBED_PAIRS.index((TI, TO))
    A = V.conv_matrix(16).contiguous()
    for i, (B, Hb, Wb, tr) in enumerate(R.EMBED_CASES):
        if B > 43 or (B == 43 and (TI, TO) not in R.EMBED_BIG_PAIRS):
            continue                                                     # (the two largest: a few pairs only, for the time)
        for mixed in (False, True):
            kind = "dct" if (i + j + int(mixed)) % 2 else "normal"
            y, c = R.embed_inputs(B, Hb, Wb, TI, kind, 100 + 10 * i)
            lam = R.lam_pair(100 + 10 * i + 5) if mixed else None
            feat = embed_emul(y, c, A, tr, lam, TI, TO)
            worst(NAMES[TO], R.embed_check(feat, y, c, A, tr, lam, TI, TO, f"emulation {B} {Hb} {Wb} {tr} {mixed}"))
    worst.report(f"embed emulation {NAMES[TI]}->{NAMES[TO]}")


@pytest.mark.parametrize("TI,TO", R.MIXUP_PAIRS, ids=lambda t: NAMES[t])
def test_bounds_accept_mixup_emulation(TI, TO):
    cases = [(B, per) for per in R.MIXUP_PER for B in R.MIXUP_B] + ([R.MIXUP_BIG] if TI == F32 and TO == BF16 else [])
    for i, (B, per) in enumerate(cases):
        x = R.randn((B, per), 300 + i, 3.0).to(TI)
        lam = R.lam_pair(301 + i)
        lo, _ = R.mix_fp32(x, lam)
        R.mixup_check(lo.to(TO), x, lam, TI, TO, f"emulation {B} {per}")
        plain = (x.float() * lam[0] + x.float().roll(1, 0) * lam[1]).to(TO)          # two roundings instead of the fma
        KC.check_bound(plain, *R.mixup_ref(x, lam)[:2], TO, 1, 2 * KC.U, "unfused emulation")


@pytest.mark.parametrize("fam", ["one", "two", "mix"])
def test_bounds_accept_softxent_emulation(fam):
    worst = KC.Worst()
    for (B, C, kind, f, tk, dt, gout, seed) in R.sx_plan():
        if f != fam or (B * C > 1_100_000 and kind != "n30"):
            continue
        z, t, _, _, _ = R.sx_case_inputs(B, C, kind, tk, seed)
        gs = R.f32(1.0 / B)
        g = float(F32_(gs) * F32_(gout)) if gout is not None else gs
        got = sx_emul(z, t, g, dt)
        if fam == "one":
            got.pop("lse"), got.pop("T")
        R.sx_check(got, R.softxent_ref(z, t, g), C, dt, f"emulation {fam} B={B} C={C} {kind} {tk}", worst)
    worst.report(f"softxent emulation {fam}")
    assert max(worst.d.values()) < 1.0


def test_bounds_accept_adamw_emulation():
    worst = KC.Worst()
    for (ch, name, gs, mn, step0, with_norm, seed) in R.adam_plan():
        n = ch * 256
        p, m, v, flags = R.adam_state(n, seed, zero_moments=(name == "tiny"))
        for k in range(3):
            g = R.adam_grad(n, gs, seed + 10 + k)
            r = R.adamw_ref(p, g, m, v, flags, step0 + k, mn, **R.ADAM_HYPER)
            got = adam_emul(p, g, m, v, flags, step0 + k, mn, **R.ADAM_HYPER)
            if not with_norm:
                got["norm"] = None
            R.adam_check(got, r, f"emulation n/256={ch} {name} step={step0 + k}", worst)
            p, m, v = got["p"], got["m"], got["v"]
    worst.report("clip_adamw_wd emulation")


@pytest.mark.parametrize("dt", [F32, BF16, F16], ids=lambda t: NAMES[t])
@pytest.mark.parametrize("E", R.POOL_E)
def test_bounds_accept_pool_emulation(dt, E):
    worst = KC.Worst()
    for (B, N, acc, offset, seed) in R.pool_plan(E):
        if B * N * E > 3_000_000:
            continue
        x, gamma, beta, dp = R.pool_inputs(B, N, E, dt, offset, seed)
        pooled, mean, rstd = pool_fwd_emul(x, gamma, beta, 1e-5, dt)
        where = f"emulation {NAMES[dt]} E={E} B={B} N={N}"
        R.pool_fwd_check(pooled, mean, rstd, x, gamma, beta, 1e-5, dt, where, worst, "pool")
        init = (R.randn((E,), seed + 6).double(), R.randn((E,), seed + 7).double()) if acc else None
        dx, dg, db = pool_bwd_emul(dp, x, gamma, mean, rstd, init, dt)
        R.pool_bwd_check(dx, dg, db, dp, x, gamma, mean, rstd, init, dt, where, worst, "pool")
    worst.report(f"head_pool emulation {NAMES[dt]} E={E}")


# ================================================================================================= reject: seeded defects
def rejected(fn):
    with pytest.raises(AssertionError):
        fn()


def test_bounds_reject_embed_defects():
    A = V.conv_matrix(16).contiguous()
    for (TI, TO) in ((F32, F32), (BF16, BF16), (F16, F16)):
        for (B, Hb, Wb) in ((3, 28, 28), (7, 4, 6)):
            y, c = R.embed_inputs(B, Hb, Wb, TI, "normal", 61)
            lam = R.lam_pair(62)
            R.embed_check(embed_emul(y, c, A, 0, lam, TI, TO), y, c, A, 0, lam, TI, TO, "honest")
            for defect in ("roll", "position"):
                rejected(lambda: R.embed_check(embed_emul(y, c, A, 0, lam, TI, TO, defect), y, c, A, 0, lam, TI, TO, defect))
    # B = 2: a roll by +1 is a roll by -1 -- the lists need B >= 3 for this defect to show, and have B = 3 and 7
    assert any(B >= 3 for B, _, _, _ in R.EMBED_CASES)
    x = R.randn((3, 64), 63)
    lam = R.lam_pair(64)
    wrong = (x * lam[0] + x.roll(-1, 0) * lam[1])
    rejected(lambda: R.mixup_check(wrong, x, lam, F32, F32, "roll"))
    lab = torch.tensor([1, 2, 3])
    assert not torch.equal(R.mixup_target_ref(lab, lam, 5), R.mixup_target_ref(lab.flip(0), lam, 5).flip(0))


def test_bounds_reject_softxent_defects():
    for (B, C, kind, tk) in ((37, 1000, "n3", "soft"), (257, 256, "n5+50", "soft"), (19, 63, "n0.01", "soft")):
        z, t, _, _, _ = R.sx_case_inputs(B, C, kind, tk, 71)
        g = R.f32(1.0 / B)
        r = R.softxent_ref(z, t, g)
        for dt in (F32, BF16):
            R.sx_check(sx_emul(z, t, g, dt), r, C, dt, "honest", KC.Worst())
            for defect in ("lse", "mass"):
                rejected(lambda: R.sx_check(sx_emul(z, t, g, dt, defect), r, C, dt, defect, KC.Worst()))
        # each output on its own: the defect is not only caught through one of them
        bad = sx_emul(z, t, g, F32, "mass")
        good = sx_emul(z, t, g, F32)
        for k in ("T", "rows", "dl"):
            rejected(lambda: R.sx_check({**good, k: bad[k]}, r, C, F32, "mass " + k, KC.Worst()))
        bad = sx_emul(z, t, g, F32, "lse")
        for k in ("lse", "rows", "dl"):
            rejected(lambda: R.sx_check({**good, k: bad[k]}, r, C, F32, "lse " + k, KC.Worst()))


def test_bounds_reject_adamw_defects():
    for ch, gs, mn in ((1025, 1.0, 1.0), (4097, 1e3, 1.0), (2049, 1.0, 0.0)):
        n = ch * 256
        p, m, v, flags = R.adam_state(n, 81)
        flags[1] = 1
        g = R.adam_grad(n, gs, 82)
        g.view(-1, 256)[1] = R.randn((256,), 83, gs)                      # chunk 1 is not a zero chunk here
        g[-256:] = R.randn((256,), 84, gs * 30)                           # the last stride carries weight in the norm
        r = R.adamw_ref(p, g, m, v, flags, 5, mn, **R.ADAM_HYPER)
        R.adam_check(adam_emul(p, g, m, v, flags, 5, mn, **R.ADAM_HYPER), r, "honest", KC.Worst())
        rejected(lambda: R.adam_check(adam_emul(p, g, m, v, flags, 5, mn, defect="flag", **R.ADAM_HYPER), r, "flag", KC.Worst()))
        bad = adam_emul(p, g, m, v, flags, 5, mn, defect="stride", **R.ADAM_HYPER)
        rejected(lambda: R.adam_check(bad, r, "stride", KC.Worst()))
        if mn > 0:                                                        # and through p alone, with norm_out NULL
            bad["norm"] = None
            rejected(lambda: R.adam_check(bad, r, "stride, no norm_out", KC.Worst()))


def test_bounds_reject_pool_defects():
    for dt, E in ((F32, 192), (BF16, 768), (F16, 384)):
        G = R.pool_rows(E)
        B, N = 3, 8 * G + 1
        x, gamma, beta, dp = R.pool_inputs(B, N, E, dt, True, 91)
        args = (x, gamma, beta, 1e-5, dt)
        R.pool_fwd_check(*pool_fwd_emul(*args), *args, "honest", KC.Worst(), "pool")
        for defect in ("clamp", "moment"):
            rejected(lambda: R.pool_fwd_check(*pool_fwd_emul(*args, defect=defect), *args, defect, KC.Worst(), "pool"))
        pooled, mean, rstd = pool_fwd_emul(*args)
        _, _, bad_rs = pool_fwd_emul(*args, defect="moment")
        rejected(lambda: R.pool_fwd_check(pooled, mean, bad_rs, *args, "rstd alone", KC.Worst(), "pool"))


# ================================================================================================= the regimes the lists reach
def test_regimes_embed():
    info = {c: R.embed_launch(*c[:3]) for c in R.EMBED_CASES}
    npatch = lambda c: c[0] * (c[1] // 2) * (c[2] // 2)
    assert any(npatch(c) < 4 and any(q0 >= q1 for q0, q1 in runs) for c, (_, _, runs) in info.items()), "waves with empty runs"
    assert any(npatch(c) % (4 * grid) for c, (grid, _, _) in info.items()), "npatch not a multiple of the wave count"
    assert (1, 28, 28, 0) in info, "B = 1 with mixing"
    for B in (3, 7):                               # one-patch runs: the partner is re-fetched, as b - 1 and (b == 0) as B - 1
        c = next(c for c in R.EMBED_CASES if c[:3] == (B, 28, 28))
        _, per, runs = info[c]
        starts = {q0 % B for q0, q1 in runs if q0 < q1}
        assert per == 1 and 0 in starts and len(starts - {0}) > 0
    capped = [c for c, (grid, per, _) in info.items() if npatch(c) > 8192]
    assert capped
    for c in capped:
        grid, per, runs = info[c]
        B = c[0]
        assert grid == 2048 and per > 1 and B % per != 0
        live = [(q0, q1) for q0, q1 in runs if q0 < q1]
        assert any(q0 % B for q0, _ in live), "a run starts mid-position"
        # both partner paths: a predecessor in the run (q > q0, b != 0), and a re-fetch inside a run (q > q0, b == 0)
        assert any((q % B) != 0 for q0, q1 in live for q in range(q0 + 1, q1))
        assert any((q % B) == 0 for q0, q1 in live for q in range(q0 + 1, q1))
        assert sum(q1 - q0 for q0, q1 in live) == npatch(c)
    assert any(c[1] != c[2] for c in R.EMBED_CASES)
    assert (2, 64, 64, 1) in info
    assert {c[3] for c in R.EMBED_CASES} == {0, 1}
    assert len(R.EMBED_PAIRS) == 7 and (F16, F16) in R.EMBED_PAIRS
    for j in range(7):                             # each pair meets both input kinds, mixed and unmixed
        kinds = {((i + j + mx) % 2, mx) for i in range(len(R.EMBED_CASES) - 1) for mx in (0, 1)}
        assert len(kinds) == 4


def test_regimes_mixup_and_target():
    for per in R.MIXUP_PER:
        assert per % 4 == 0
    assert set(R.MIXUP_PER) == {4, 1020, 1024, 1028, 50176} and set(R.MIXUP_B) == {1, 2, 7}
    turns = {R.mixup_regime(B * per)[1] for per in R.MIXUP_PER for B in R.MIXUP_B}
    assert turns == {1}
    n = R.MIXUP_BIG[0] * R.MIXUP_BIG[1]
    assert n > 4096 * 1024 * 2 and R.mixup_regime(n) == (4096, 3)
    assert {R.mixup_regime(B * per)[0] for per in (1020, 1024, 1028) for B in (1,)} == {1, 2}
    big = [(B, C) for B, C in R.TARGET_CASES if B * C > 2048 * 256]
    assert big and all(R.target_regime(B * C) == (2048, 2) for B, C in big)
    assert {B for B, _ in R.TARGET_CASES} >= {1, 2, 257} and {C for _, C in R.TARGET_CASES} >= {1, 10, 1000}


def test_regimes_softxent():
    assert {C for _, C in R.SX_SHAPES} == set(R.SX_C) and {B for B, _ in R.SX_SHAPES} >= set(R.SX_B)
    plan = R.sx_plan()
    assert len(plan) == len(R.SX_SHAPES) * 6 * 3
    for fam in ("one", "two", "mix"):
        mine = [p for p in plan if p[3] == fam]
        assert {p[5] for p in mine} == set(R.SX_DTS)
        assert {(p[0], p[1], p[2]) for p in mine} == {(B, C, k) for B, C in R.SX_SHAPES for k in R.SX_LOGITS}
        if fam != "mix":
            assert {p[4] for p in mine} == {"soft", "hard"}
        if fam != "one":
            assert {p[6] for p in mine} == set(R.SX_GOUT)
    # the last workgroup's strided row sum turns twice from B = 257, five times at 1024; K = ceil(C / 256) from 1 to 86
    assert {cdiv(B, 256) for B in R.SX_B} == {1, 2, 4} and {cdiv(C, 256) for C in R.SX_C} == {1, 2, 4, 86}
    lab = R.sx_labels(257, 1000, 5, equal_neighbours=True)
    assert lab[0] == 0 and lab[-1] == 999 and lab[1] == lab[0]
    assert R.sx_labels(1, 7, 3)[0] == 6 and R.sx_labels(1, 7, 4)[0] == 0
    t = R.sx_soft_target(6, 50, 1).double().sum(1)
    assert abs(float(t[0]) - 1) < 1e-6 and abs(float(t[1]) - 1) < 1e-6 and abs(float(t[2]) - 0.9) < 1e-6
    z = R.sx_logits(4, 300, "dominant", 1)
    assert float(z[0].max() - z[0].sort().values[-2]) > 70 and float(z[1].max()) < 10
    for kind in R.SX_LOGITS:
        assert bool(torch.isfinite(R.sx_logits(3, 1000, kind, 2)).all())


def test_regimes_adamw():
    ch = set(R.ADAM_CHUNKS)
    assert ch >= {1, 4, 255, 256, 257, 1024, 1025, 4096, 4097, 4096 * 3 + 5}
    last = {}
    for c in R.ADAM_CHUNKS:
        u, turns = R.sqnorm_regime(c * 256)
        last.setdefault((u, turns), []).append(c)
    assert {u for (u, t) in last if t == 1} == {0, 1, 2, 3}, last          # each stride u is the last one present
    assert R.sqnorm_regime(1024 * 256) == (0, 1) and R.sqnorm_regime(1025 * 256) == (1, 1)
    assert R.sqnorm_regime(4096 * 256) == (3, 1) and R.sqnorm_regime(4097 * 256) == (0, 2)
    assert any(t >= 2 for (_, t) in last)
    assert R.adamw_regime(4096 * 256) == (4096, 1) and R.adamw_regime(4097 * 256) == (4096, 2)
    assert R.adamw_regime((4096 * 3 + 5) * 256) == (4096, 4)
    plan = R.adam_plan()
    assert {p[1] for p in plan} == {m[0] for m in R.ADAM_MODES}
    assert {p[4] for p in plan} == set(R.ADAM_STEPS)
    assert {p[5] for p in plan} == {True, False}
    assert {p[1] for p in plan if p[0] > 4096} >= {"active", "off"}       # clipping on and off where both loops turn again
    assert any(p[3] == 0.0 for p in plan)
    _, _, _, flags = R.adam_state(4096 * 256, 1)
    assert 0 < int(flags.sum()) < flags.numel() and list(flags[:4]) == [1, 0, 1, 1]
    g = R.adam_grad(1024 * 256, 1.0, 3)
    assert bool((g.view(-1, 256)[1] == 0).all()) and bool((g[::7] == 0).all()) and float(g.abs().max()) > 0
    assert R.ADAM_HYPER["wd_factor"] > 0


def test_regimes_pool():
    for E in R.POOL_E:
        G = R.pool_rows(E)
        assert G == (16 if E <= 384 else 4)
        ns = R.pool_ns(E)
        assert set(ns) >= {1, G - 1, G, G + 1, 4 * G - 1, 4 * G, 4 * G + 1, 8 * G, 8 * G + 1, 196, 294} - {0}
        assert {cdiv(N, 8 * G) for N in ns} >= {1, 2} and {cdiv(N, 4 * G) for N in ns} >= {1, 2, 3}
        plan = R.pool_plan(E)
        assert {p[0] for p in plan} == set(R.POOL_B) and {p[2] for p in plan} == {0, 1} and {p[3] for p in plan} == {True, False}
        # a clamped prefetch row exists (N is not a multiple of the rows per turn) on both sides of each turn edge
        assert any(N % (8 * G) for N in ns) and any(N % (8 * G) == 0 for N in ns)
