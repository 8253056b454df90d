"""Element-wise edge tests of the kernels a train step enters and leaves through: rgbnm_subblock_embed[_mix], rgbnm_mixup,
rgbnm_mixup_target, the three soft cross-entropy families, rgbnm_clip_adamw_wd_step (csrc/embed_tail.hip) and
rgbnm_head_pool_fwd / _bwd (csrc/layernorm.hip), in the conventions of test_kernel_edges.py: guarded outputs checked bit-wise,
NaN behind every floating-point input, workspaces of exactly the size asked for, the device kernel asserted, every element
checked against the fp64 references of tests/step_ends_ref.py.  The bounds are derived in that module's header; the case lists
live there too, and tests/test_step_ends_cpu.py asserts the launch regimes they reach.

ASSUMPTION behind the exp / log terms: v_exp_f32 and v_log_f32 are accurate to 1 ulp of their result (AMD's ISA manual, quoted
from memory; not measured here).  The bounds carry no fitted factor (EXPLOG = ADAM_F = 1).

Worst ratios |got - ref| / bound measured on one MI355X (the keys -s prints) are in MEASURED below and beside each bound in
the header of step_ends_ref.py.
"""
import pytest
import torch

import kernel_check as KC
import step_ends_ref as R
from kernel_check import guarded, check_bound, launched, ran
from oracle import vit_torch as V
from rgb_no_more_amd import lib as L
from step_ends_ref import F32, BF16, F16, NAMES

pytestmark = pytest.mark.gpu

DEV = "cuda"
EINVAL, EWORKSPACE = -1, -3      # RGBNM_EINVAL, RGBNM_EWORKSPACE

# worst ratios measured on one MI355X (bound = 1), in the bracket style of test_kernel_edges.ATTN_C; 0.5 is half an ulp of a
# 16-bit output, where the fp32 arithmetic in front of the rounding does not show
MEASURED = {
    "embed luma": "[f32->f32 0.291, bf16->f32 0.303, f32->bf16 0.5, bf16->bf16 0.5, f32->f16 0.499, bf16->f16 0.499, f16->f16 0.66]",
    "mixup": "[f32->f32 0.487, f32->bf16 0.5, bf16->bf16 0.5]",
    "softxent": "[lse 0.474, T 0.221, rows 0.203, loss 0.061, dl f32 0.556, dl bf16 0.5, dl f16 0.5]",
    "clip_adamw_wd": "[p 0.47, m 0.39, v 0.356, norm 0.031]",
    "head_pool": "[pooled 0.0057 f32 / 0.497 16-bit, mean and rstd 0.011, dx 0.012 f32 / 0.499 16-bit, dgamma 0.011, dbeta 0.274]",
}


def expect(names, want, where):
    for w in want:
        assert ran(names, w), f"{where}: kernel {w} did not run; ran {sorted(set(names))}"


def nan_tail(x, pad=256):
    """x copied to the device into a buffer with `pad` NaN elements behind its last one (floating point only)."""
    buf = torch.full((x.numel() + pad,), float("nan"), dtype=x.dtype, device=DEV)
    buf[:x.numel()] = x.reshape(-1).to(DEV)
    return buf[:x.numel()].view(x.shape)


def gvec(n, dtype):
    return guarded(n, None, dtype)


same_bits = R.same_bits


# --------------------------------------------------------------------------------------------------------------- embedding
def embed_case(TI, TO, B, Hb, Wb, tr, mixed, kind, seed, worst):
    A = V.conv_matrix(16).contiguous()
    y, c = R.embed_inputs(B, Hb, Wb, TI, kind, seed)
    lam = R.lam_pair(seed + 5) if mixed else None
    yd, cd, Ad = nan_tail(y), nan_tail(c), nan_tail(A)
    lamd = nan_tail(lam) if mixed else None
    npatch = B * (Hb // 2) * (Wb // 2)
    feat = guarded(npatch, 384, TO)
    lib = L.lib()

    def call():
        if mixed:
            L.check(lib.rgbnm_subblock_embed_mix(L.dt_of(TI), L.dt_of(TO), yd.data_ptr(), cd.data_ptr(), lamd.data_ptr(),
                                                 Ad.data_ptr(), feat.t.data_ptr(), B, Hb, Wb, tr, L.stream()))
        else:
            L.check(lib.rgbnm_subblock_embed(L.dt_of(TI), L.dt_of(TO), yd.data_ptr(), cd.data_ptr(), Ad.data_ptr(),
                                             feat.t.data_ptr(), B, Hb, Wb, tr, L.stream()))
    _, names = launched(call)
    where = f"subblock_embed {NAMES[TI]}->{NAMES[TO]} B={B} Hb={Hb} Wb={Wb} tr={tr} mixed={int(mixed)} {kind}"
    expect(names, ("subblock_embed_kernel",), where)
    feat.check(where)
    key = f"embed luma {NAMES[TI]}->{NAMES[TO]}"
    worst(key, R.embed_check(feat.t, yd, cd, Ad, tr, lam, TI, TO, where))


@pytest.mark.parametrize("TI,TO", R.EMBED_PAIRS, ids=lambda t: NAMES[t])
def test_subblock_embed_edges(TI, TO):
    """subblock_embed_kernel: one wave per run of `per` patches taken position-major, grid min(ceil(npatch / 4), 2048); every
    case with lam NULL and set, unit-normal and DCT-like inputs alternating."""
    worst = KC.Worst()
    j = R.EMBED_PAIRS.index((TI, TO))
    for i, (B, Hb, Wb, tr) in enumerate(R.EMBED_CASES):
        if B == 131 and (TI, TO) not in R.EMBED_BIG_PAIRS:
            continue
        for mixed in (False, True):
            kind = "dct" if (i + j + int(mixed)) % 2 else "normal"
            embed_case(TI, TO, B, Hb, Wb, tr, mixed, kind, 100 + 10 * i, worst)
    worst.report(f"subblock_embed {NAMES[TI]}->{NAMES[TO]}")


def test_subblock_embed_refusals():
    """Odd block grids, empty batches, type pairs outside the seven and a feature matrix beyond 32-bit indexing: EINVAL on
    the host, the output untouched."""
    lib = L.lib()
    A = V.conv_matrix(16).contiguous().to(DEV)
    y = torch.zeros(2 * 4 * 6 * 64, device=DEV)
    feat = guarded(12, 384, F32)
    p = (y.data_ptr(), y.data_ptr(), A.data_ptr(), feat.t.data_ptr())
    assert lib.rgbnm_subblock_embed(0, 0, *p, 2, 3, 6, 0, L.stream()) == EINVAL
    assert lib.rgbnm_subblock_embed(0, 0, *p, 2, 4, 5, 0, L.stream()) == EINVAL
    assert lib.rgbnm_subblock_embed(0, 0, *p, 0, 4, 6, 0, L.stream()) == EINVAL
    assert lib.rgbnm_subblock_embed(2, 0, *p, 2, 4, 6, 0, L.stream()) == EINVAL        # fp16 -> fp32
    assert lib.rgbnm_subblock_embed(2, 1, *p, 2, 4, 6, 0, L.stream()) == EINVAL        # fp16 -> bf16
    assert lib.rgbnm_subblock_embed(0, 0, *p, 28540, 28, 28, 0, L.stream()) == EINVAL  # npatch * 384 >= 2^31
    torch.cuda.synchronize()
    feat.check("subblock_embed refusals", written=False)
    assert bool((feat.raw == feat.canary).all())


# ------------------------------------------------------------------------------------------------------------------ mixup
def mixup_case(TI, TO, B, per, seed, worst):
    x = R.randn((B, per), seed, 3.0).to(TI)
    lam = R.lam_pair(seed + 1)
    xd, lamd = nan_tail(x), nan_tail(lam)
    out = guarded(B, per, TO)

    def call():
        L.check(L.lib().rgbnm_mixup(L.dt_of(TI), L.dt_of(TO), xd.data_ptr(), out.t.data_ptr(), lamd.data_ptr(), B, per, L.stream()))
    _, names = launched(call)
    where = f"mixup {NAMES[TI]}->{NAMES[TO]} B={B} per={per}"
    expect(names, ("mixup_kernel",), where)
    out.check(where)
    worst(f"mixup {NAMES[TI]}->{NAMES[TO]}", R.mixup_check(out.t, xd, lam, TI, TO, where))


@pytest.mark.parametrize("TI,TO", R.MIXUP_PAIRS, ids=lambda t: NAMES[t])
def test_mixup_edges(TI, TO):
    """mixup_kernel: four elements per thread, grid min(4096, ceil(n / 1024)); the last case turns the stride loop 3 times."""
    worst = KC.Worst()
    for i, per in enumerate(R.MIXUP_PER):
        for B in R.MIXUP_B:
            mixup_case(TI, TO, B, per, 300 + 10 * i + B, worst)
    mixup_case(TI, TO, *R.MIXUP_BIG, 399, worst)
    worst.report(f"mixup {NAMES[TI]}->{NAMES[TO]}")


def test_mixup_refusals():
    """fp16, per_sample % 4 != 0 and bf16 -> fp32 are refused on the host; the guarded output stays untouched."""
    lib = L.lib()
    x = torch.zeros(4096, device=DEV)
    lam = R.lam_pair(1).to(DEV)
    out = guarded(2, 1024, F32)
    for ti, to, per in ((2, 2, 1024), (0, 2, 1024), (2, 0, 1024), (0, 0, 1022), (0, 0, 1023), (1, 0, 1024), (0, 0, 0)):
        assert lib.rgbnm_mixup(ti, to, x.data_ptr(), out.t.data_ptr(), lam.data_ptr(), 2, per, L.stream()) == EINVAL, (ti, to, per)
    assert lib.rgbnm_mixup(0, 0, x.data_ptr(), out.t.data_ptr(), lam.data_ptr(), 0, 1024, L.stream()) == EINVAL
    torch.cuda.synchronize()
    assert bool((out.raw == out.canary).all())


def test_mixup_target_bit_exact():
    """mixup_target_kernel against the expression in fp32, bit for bit: non-dyadic lam, equal neighbouring labels, B = 1, and
    B C > 2048 * 256 for the stride loop."""
    for i, (B, C) in enumerate(R.TARGET_CASES):
        lab = R.sx_labels(B, C, 400 + i, equal_neighbours=True).to(DEV)
        lam = R.lam_pair(450 + i)
        lamd = nan_tail(lam)
        out = guarded(B, C, F32)

        def call():
            L.check(L.lib().rgbnm_mixup_target(lab.data_ptr(), out.t.data_ptr(), lamd.data_ptr(), B, C, L.stream()))
        _, names = launched(call)
        where = f"mixup_target B={B} C={C}"
        expect(names, ("mixup_target_kernel",), where)
        out.check(where)
        ok = same_bits(out.t, R.mixup_target_ref(lab, lam, C))
        assert bool(ok.all()), f"{where}: {int((~ok).sum())} elements differ, first {(~ok).nonzero()[:4].tolist()}"


# ---------------------------------------------------------------------------------------------------------- cross entropy
def sx_case(B, C, kind, fam, tk, dt, gout, seed, worst, ticket):
    lib = L.lib()
    z, t, soft, lab, lam = R.sx_case_inputs(B, C, kind, tk, seed)
    zd = nan_tail(z)
    td = t.to(DEV)
    softd = nan_tail(soft) if soft is not None else None
    labd = lab.to(DEV) if lab is not None else None
    lamd = nan_tail(lam) if lam is not None else None
    gscale = R.f32(1.0 / B)
    rows, loss, dl = gvec(B, F32), gvec(1, F32), guarded(B, C, dt)
    stat = gvec(2 * B, F32)
    where = f"softxent {fam} B={B} C={C} {kind} {tk} dl={NAMES[dt]} gout={gout}"
    if fam == "one":
        if tk == "mix":                             # rgbnm_softxent takes the mixed target dense
            dense = nan_tail(t)

        def call():
            L.check(lib.rgbnm_softxent(L.dt_of(dt), zd.data_ptr(), dense.data_ptr() if tk == "mix" else L.ptr(softd),
                                       L.ptr(labd) if tk != "mix" else None, rows.t.data_ptr(), loss.t.data_ptr(), dl.t.data_ptr(),
                                       B, C, gscale, L.stream()))
        _, names = launched(call)
        expect(names, ("softxent_kernel", "mean_kernel"), where)
        g = gscale
    else:
        goutd = nan_tail(torch.tensor([gout], dtype=F32)) if gout is not None else None

        def fwd():
            if fam == "mix":
                L.check(lib.rgbnm_softxent_loss_mix(zd.data_ptr(), labd.data_ptr(), lamd.data_ptr(), rows.t.data_ptr(),
                                                    stat.t.data_ptr(), loss.t.data_ptr(), ticket.t.data_ptr(), B, C, L.stream()))
            else:
                L.check(lib.rgbnm_softxent_loss(zd.data_ptr(), L.ptr(softd), L.ptr(labd), rows.t.data_ptr(), stat.t.data_ptr(),
                                                loss.t.data_ptr(), ticket.t.data_ptr(), B, C, L.stream()))

        def bwd():
            if fam == "mix":
                L.check(lib.rgbnm_softxent_grad_mix(L.dt_of(dt), zd.data_ptr(), labd.data_ptr(), lamd.data_ptr(), stat.t.data_ptr(),
                                                    L.ptr(goutd), dl.t.data_ptr(), B, C, gscale, L.stream()))
            else:
                L.check(lib.rgbnm_softxent_grad(L.dt_of(dt), zd.data_ptr(), L.ptr(softd), L.ptr(labd), stat.t.data_ptr(),
                                                L.ptr(goutd), dl.t.data_ptr(), B, C, gscale, L.stream()))

        def ticket_now():
            return int(ticket.t.view(torch.int32)[0])

        def both():                                 # the same ticket twice: the first launch has to leave it ready
            fwd()
            t1, first = ticket_now(), (rows.t.clone(), loss.t.clone())
            fwd()
            t2, same = ticket_now(), torch.equal(first[0], rows.t) and torch.equal(first[1], loss.t)
            bwd()
            return t1, t2, same
        (t1, t2, same), names = launched(both)
        expect(names, ("softxent_loss_kernel", "softxent_grad_kernel"), where)
        assert t1 == 0, f"{where}: ticket not zero after the first launch"
        assert t2 == 0, f"{where}: ticket not zero after the second launch"
        assert same, f"{where}: the second launch on the same ticket differs"
        ticket.check(where + " ticket", written=False)
        stat.check(where + " row_stats")
        g = float(torch.tensor(gscale, dtype=F32) * torch.tensor(gout, dtype=F32)) if gout is not None else gscale
    for o, nm in ((rows, "loss_rows"), (loss, "loss"), (dl, "dlogits")):
        o.check(where + " " + nm)
    r = R.softxent_ref(zd, td, g)
    got = dict(rows=rows.t, loss=loss.t, dl=dl.t)
    if fam != "one":
        st = stat.t.view(B, 2)
        got.update(lse=st[:, 0], T=st[:, 1])
    R.sx_check(got, r, C, dt, where, worst)


@pytest.mark.parametrize("fam", ["one", "two", "mix"])
def test_softxent_edges(fam):
    """softxent_kernel + mean_kernel, softxent_loss_kernel + softxent_grad_kernel, and the pair with the mixed target built
    where it is read: one workgroup per row, 256 strided partial sums; C walks the 256-class stride, B the 256-row stride of
    the last workgroup's row sum; each family against fp64, not against another family."""
    worst = KC.Worst()
    ticket = gvec(1, F32)
    ticket.raw[ticket.off] = 0
    for (B, C, kind, f, tk, dt, gout, seed) in R.sx_plan():
        if f == fam:
            sx_case(B, C, kind, fam, tk, dt, gout, seed, worst, ticket)
    if fam == "one":                                # the dense mixed target through the one-launch entry as well
        sx_case(257, 1000, "n3", "one", "mix", F32, None, 7777, worst, ticket)
    worst.report(f"softxent {fam}")


def test_softxent_label_out_of_range_is_a_zero_row():
    """include/rgbnm.h: a hard label outside [0, C) matches no class: target mass 0, loss row 0, dlogits 0, and with mixing
    the in-range partner alone counts.  All three families."""
    lib = L.lib()
    B, C = 4, 300
    z = nan_tail(R.sx_logits(B, C, "n3", 77))
    lab = torch.tensor([5, C, -1, 299], dtype=torch.int64, device=DEV)
    lam = R.lam_pair(78)
    lamd = nan_tail(lam)
    ticket = torch.zeros(1, dtype=torch.int32, device=DEV)
    for fam in ("one", "two", "mix"):
        rows, loss, dl, stat = gvec(B, F32), gvec(1, F32), guarded(B, C, F32), gvec(2 * B, F32)
        if fam == "one":
            L.check(lib.rgbnm_softxent(0, z.data_ptr(), None, lab.data_ptr(), rows.t.data_ptr(), loss.t.data_ptr(),
                                       dl.t.data_ptr(), B, C, 1.0, L.stream()))
        elif fam == "two":
            L.check(lib.rgbnm_softxent_loss(z.data_ptr(), None, lab.data_ptr(), rows.t.data_ptr(), stat.t.data_ptr(),
                                            loss.t.data_ptr(), ticket.data_ptr(), B, C, L.stream()))
            L.check(lib.rgbnm_softxent_grad(0, z.data_ptr(), None, lab.data_ptr(), stat.t.data_ptr(), None, dl.t.data_ptr(),
                                            B, C, 1.0, L.stream()))
        else:
            L.check(lib.rgbnm_softxent_loss_mix(z.data_ptr(), lab.data_ptr(), lamd.data_ptr(), rows.t.data_ptr(),
                                                stat.t.data_ptr(), loss.t.data_ptr(), ticket.data_ptr(), B, C, L.stream()))
            L.check(lib.rgbnm_softxent_grad_mix(0, z.data_ptr(), lab.data_ptr(), lamd.data_ptr(), stat.t.data_ptr(), None,
                                                dl.t.data_ptr(), B, C, 1.0, L.stream()))
        torch.cuda.synchronize()
        for o in (rows, loss, dl):
            o.check(f"out-of-range labels {fam}")
        if fam != "mix":
            assert float(rows.t[1]) == 0.0 and float(rows.t[2]) == 0.0
            assert bool((dl.t[1:3] == 0).all())
            assert float(rows.t[0]) > 0 and float(rows.t[3]) > 0
        else:                                       # row 1 = lam0 [C] + lam1 [5]: the partner alone; row 2: no class at all
            t = torch.zeros(B, C, device=DEV)
            t[0, 5], t[0, 299], t[1, 5], t[3, 299] = lam[0], lam[1], lam[1], lam[0]
            r = R.softxent_ref(z, t, 1.0)
            b = R.sx_bounds(r, C, F32)
            check_bound(rows.t, r["rows"], None, F32, 0, 0, "out-of-range labels mix rows", extra=b[2])
            check_bound(dl.t, r["dl"], None, F32, 0, 0, "out-of-range labels mix dlogits", extra=b[4])
            assert float(rows.t[2]) == 0.0 and bool((dl.t[2] == 0).all())


def test_softxent_refusals():
    lib = L.lib()
    z = torch.zeros(8, 16, device=DEV)
    lab = torch.zeros(8, dtype=torch.int64, device=DEV)
    o = guarded(8, 16, F32)
    p = o.t.data_ptr()
    assert lib.rgbnm_softxent(0, z.data_ptr(), None, None, p, p, p, 8, 16, 1.0, L.stream()) == EINVAL       # no target
    assert lib.rgbnm_softxent(3, z.data_ptr(), None, lab.data_ptr(), p, p, p, 8, 16, 1.0, L.stream()) == EINVAL
    assert lib.rgbnm_softxent(0, z.data_ptr(), None, lab.data_ptr(), p, p, p, 0, 16, 1.0, L.stream()) == EINVAL
    assert lib.rgbnm_softxent(0, z.data_ptr(), None, lab.data_ptr(), p, p, p, 8, 0, 1.0, L.stream()) == EINVAL
    assert lib.rgbnm_softxent_loss(z.data_ptr(), None, lab.data_ptr(), p, p, p, None, 8, 16, L.stream()) == EINVAL   # no ticket
    assert lib.rgbnm_softxent_grad(3, z.data_ptr(), None, lab.data_ptr(), p, None, p, 8, 16, 1.0, L.stream()) == EINVAL
    assert lib.rgbnm_softxent_loss_mix(z.data_ptr(), lab.data_ptr(), None, p, p, p, p, 8, 16, L.stream()) == EINVAL  # no lam
    assert lib.rgbnm_softxent_grad_mix(0, z.data_ptr(), lab.data_ptr(), None, p, None, p, 8, 16, 1.0, L.stream()) == EINVAL
    torch.cuda.synchronize()
    assert bool((o.raw == o.canary).all())


# ------------------------------------------------------------------------------------------------------------------ AdamW
def adam_case(ch, name, gs, max_norm, step0, with_norm, seed, worst):
    lib = L.lib()
    n = ch * 256
    p0, m0, v0, flags = R.adam_state(n, seed, zero_moments=(name == "tiny"))
    p, m, v = gvec(n, F32).fill_(p0.to(DEV)), gvec(n, F32).fill_(m0.to(DEV)), gvec(n, F32).fill_(v0.to(DEV))
    fl = torch.empty(ch + 2 * KC.GUARD_BYTES, dtype=torch.uint8, device=DEV).fill_(0xA5)      # guarded flag bytes
    fl[KC.GUARD_BYTES:KC.GUARD_BYTES + ch] = flags.to(DEV)
    flv = fl[KC.GUARD_BYTES:KC.GUARD_BYTES + ch]
    wsb = lib.rgbnm_clip_adamw_wd_workspace()
    assert wsb == 1024
    ws = gvec(wsb // 4, F32)
    h = R.ADAM_HYPER
    grads = [nan_tail(R.adam_grad(n, gs, seed + 10 + k)) for k in range(3)]
    norms = [gvec(1, F32) if with_norm else None for _ in range(3)]
    snaps = []

    def three_steps():                              # one profiled region; the state before and after each step is kept
        for k in range(3):
            before = (p.t.clone(), m.t.clone(), v.t.clone())
            L.check(lib.rgbnm_clip_adamw_wd_step(p.t.data_ptr(), grads[k].data_ptr(), m.t.data_ptr(), v.t.data_ptr(),
                                                 flv.data_ptr(), n, h["lr"], h["beta1"], h["beta2"], h["eps"], step0 + k,
                                                 h["wd_factor"], max_norm, norms[k].t.data_ptr() if with_norm else None,
                                                 ws.t.data_ptr(), wsb, L.stream()))
            snaps.append((before, (p.t.clone(), m.t.clone(), v.t.clone())))
    _, names = launched(three_steps)
    base = f"clip_adamw_wd n/256={ch} {name} max_norm={max_norm} norm_out={int(with_norm)}"
    expect(names, ("sqnorm_kernel", "adamw_kernel"), base)
    assert sum("adamw_kernel" in nm for nm in names) == 3 and sum("sqnorm_kernel" in nm for nm in names) == 3, base
    for o, nm in ((p, "p"), (m, "m"), (v, "v"), (ws, "workspace")):
        o.check(base + " " + nm)
    assert bool((fl[:KC.GUARD_BYTES] == 0xA5).all()) and bool((fl[KC.GUARD_BYTES + ch:] == 0xA5).all()), base + " flags"
    assert torch.equal(flv.cpu(), flags), base + " flags changed"
    for k, (before, after) in enumerate(snaps):
        where = f"{base} step={step0 + k}"
        r = R.adamw_ref(before[0], grads[k], before[1], before[2], flags, step0 + k, max_norm, **h)
        if name == "active":
            assert r["coef"] < 0.5, where
        elif name == "inactive":
            assert r["coef"] == 1.0 and float(r["norm"]) < max_norm, where
        if with_norm:
            norms[k].check(where + " norm_out")
        R.adam_check(dict(p=after[0], m=after[1], v=after[2], norm=norms[k].t if with_norm else None), r, where, worst)


def test_clip_adamw_wd_edges():
    """sqnorm_kernel (256 workgroups, four strides of 262144 elements per turn) and adamw_kernel (grid min(4096, n / 256), one
    256-element chunk per turn): three consecutive steps per case from the kernel's own fp32 state, p, m, v and the norm
    checked per element."""
    worst = KC.Worst()
    for case in R.adam_plan():
        adam_case(*case, worst)
    worst.report("clip_adamw_wd")


def test_clip_adamw_wd_refusals():
    """n % 256 != 0, step < 1 and a short workspace are refused on the host; the state stays untouched."""
    lib = L.lib()
    n = 512
    p = gvec(n, F32)
    g = torch.zeros(n, device=DEV)
    fl = torch.zeros(2, dtype=torch.uint8, device=DEV)
    ws = gvec(256, F32)

    def step(n_, step_, wsb):
        return lib.rgbnm_clip_adamw_wd_step(p.t.data_ptr(), g.data_ptr(), p.t.data_ptr(), p.t.data_ptr(), fl.data_ptr(), n_, 1e-3,
                                            0.9, 0.999, 1e-8, step_, 0.0, 1.0, None, ws.t.data_ptr(), wsb, L.stream())
    assert step(500, 1, 1024) == EINVAL
    assert step(0, 1, 1024) == EINVAL
    assert step(n, 0, 1024) == EINVAL
    assert step(n, -3, 1024) == EINVAL
    assert step(n, 1, 1020) == EWORKSPACE
    assert step(n, 1, 0) == EWORKSPACE
    torch.cuda.synchronize()
    assert bool((p.raw == p.canary).all()) and bool((ws.raw == ws.canary).all())


# -------------------------------------------------------------------------------------------------------------------- pool
def pool_case(dt, E, B, N, acc, offset, seed, worst):
    lib = L.lib()
    eps = 1e-5
    x, gamma, beta, dp = R.pool_inputs(B, N, E, dt, offset, seed)
    xd, gd, bd, dpd = nan_tail(x), nan_tail(gamma), nan_tail(beta), nan_tail(dp)
    pooled = guarded(B, E, dt)
    mean, rstd = gvec(B * N, F32), gvec(B * N, F32)
    dx = guarded(B * N, E, dt)
    dg, db = gvec(E, F32), gvec(E, F32)
    if acc:
        dg.fill_(R.randn((E,), seed + 6).to(DEV))
        db.fill_(R.randn((E,), seed + 7).to(DEV))
    init = (dg.t.double().clone(), db.t.double().clone()) if acc else None
    wsb = B * 2 * E * 4
    ws = gvec(wsb // 4, F32)

    def both():                                     # the backward runs on the forward's own mean / rstd
        L.check(lib.rgbnm_head_pool_fwd(L.dt_of(dt), xd.data_ptr(), gd.data_ptr(), bd.data_ptr(), pooled.t.data_ptr(),
                                        mean.t.data_ptr(), rstd.t.data_ptr(), B, N, E, eps, L.stream()))
        L.check(lib.rgbnm_head_pool_bwd(L.dt_of(dt), dpd.data_ptr(), xd.data_ptr(), gd.data_ptr(), mean.t.data_ptr(),
                                        rstd.t.data_ptr(), dx.t.data_ptr(), dg.t.data_ptr(), db.t.data_ptr(), B, N, E, acc,
                                        ws.t.data_ptr(), wsb, L.stream()))
    _, names = launched(both)
    where = f"head_pool {NAMES[dt]} E={E} B={B} N={N} acc={acc} offset={int(offset)}"
    expect(names, ("pool_fwd_kernel", "pool_bwd_kernel"), where)
    for o, nm in ((pooled, "pooled"), (mean, "mean"), (rstd, "rstd"), (dx, "dx"), (dg, "dgamma"), (db, "dbeta"),
                  (ws, "workspace")):
        o.check(where + " " + nm)
    k = f"E={E}"
    R.pool_fwd_check(pooled.t, mean.t, rstd.t, xd, gd, bd, eps, dt, where, worst, k)
    R.pool_bwd_check(dx.t, dg.t, db.t, dpd, xd, gd, mean.t, rstd.t, init, dt, where, worst, k)


@pytest.mark.parametrize("dt", [F32, BF16, F16], ids=lambda t: NAMES[t])
@pytest.mark.parametrize("E", R.POOL_E)
def test_head_pool_edges(dt, E):
    """pool_fwd_kernel takes 8 G rows per turn, pool_bwd_kernel 4 G (G = 16 up to E = 384, 4 above), prefetch rows clamped to
    N - 1: N walks those turns; mean and rstd are outputs; dgamma / dbeta accumulate into pre-filled vectors."""
    worst = KC.Worst()
    for (B, N, acc, offset, seed) in R.pool_plan(E):
        pool_case(dt, E, B, N, acc, offset, seed, worst)
    worst.report(f"head_pool {NAMES[dt]} E={E}")


def test_head_pool_refusals():
    """_bwd refuses B <= 0 and N <= 0 as _fwd does (N = 0 would divide by zero on the device), an unknown width and a short
    workspace; nothing is launched and the outputs stay untouched."""
    lib = L.lib()
    E = 192
    x = torch.zeros(2 * 4 * E, device=DEV)
    o = guarded(8, E, F32)
    p, xp = o.t.data_ptr(), x.data_ptr()

    def bwd(B, N, E_, wsb):
        return lib.rgbnm_head_pool_bwd(0, xp, xp, xp, xp, xp, p, p, p, B, N, E_, 0, p, wsb, L.stream())

    def fwd(B, N, E_):
        return lib.rgbnm_head_pool_fwd(0, xp, xp, xp, p, p, p, B, N, E_, 1e-5, L.stream())
    big = 1 << 20
    for B, N in ((0, 4), (-1, 4), (2, 0), (2, -5)):
        assert bwd(B, N, E, big) == EINVAL, (B, N)
        assert fwd(B, N, E) == EINVAL, (B, N)
    assert bwd(2, 4, 200, big) == EINVAL and fwd(2, 4, 200) == EINVAL
    assert bwd(2, 4, E, 2 * 2 * E * 4 - 4) == EWORKSPACE
    torch.cuda.synchronize()
    assert bool((o.raw == o.canary).all())
