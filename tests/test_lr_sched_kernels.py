"""Tests of rgbnm_clip_adamw_wd_step_sched (csrc/embed_tail.hip: sqnorm_unscale_sched_kernel, adamw_sched_kernel) in the
conventions of test_loss_scale_kernels.py: guarded p / m / v / flags / workspace / norm_out and both state blocks, NaN behind the
gradients, a workspace of exactly the size asked for, the device kernels counted by name.

The reference is the scaled entry itself.  Both kernel pairs are instances of one norm body and one update body (the sched
instance differs in where lr and wd_factor come from), so this entry performs rgbnm_clip_adamw_wd_step_scaled's arithmetic on an (lr,
wd_factor) pair formed on the device by the IEEE operations the host performs for that entry -- fp32(lr_d) and
fp32((lr_d / base_lr) * weight_decay), one fp64 divide, one fp64 multiply, one rounding -- so a twin set of buffers stepped by the
scaled entry with those two floats (formed here in numpy float64) must hold the same BITS after every call: p, m, v, norm_out and
the whole loss-scale block.  No tolerance anywhere in that comparison.

Sizes (in chunks of 256): 1 (one workgroup), 257 (a norm-stride tail), 4097 (a second turn of the update grid).  Ten calls per
size over an 8-entry table, so that calls 9 and 10 take the clamp to the last entry; call 6 gets a non-finite gradient; the scale
grows at call 4 (growth_interval 4) and backs off at call 6, so the blocks change in every field.

One run under the neutral block (scale 1, factors 1, clamp [1, 1]) is also held to the plain entry rgbnm_clip_adamw_wd_step: m, v
and the norm bit for bit (a product with 1.0f is exact), p through step_ends_ref.adamw_ref with loss_scale_ref.BC_EXTRA |update|
added for the device-side bias corrections, the bound test_loss_scale_kernels.py uses for the scaled entry.
"""
from fractions import Fraction

import numpy as np
import pytest
import torch

import kernel_check as KC
import loss_scale_ref as LS
import step_ends_ref as R
from kernel_check import guarded, launched
from rgb_no_more_amd import lib as L
from step_ends_ref import F32

pytestmark = pytest.mark.gpu

DEV = "cuda"
EINVAL, EWORKSPACE = -1, -3
CHUNKS = (1, 257, 4097)
GROWTH, BACKOFF, SMIN, SMAX = 1.6, 0.625, 2.0 ** -4, 2.0 ** 18
H = R.ADAM_HYPER
BASE_LR, WD = 3e-3, 0.05
TABLE = (2e-3, 3e-3, 1e-3, 0.0, 2.9e-3, 7.3e-4, 1e-4, 2.5e-4)
CALLS, BAD_CALL, INTERVAL = 10, 5, 4


def lr_pair(k):
    """(fp32(lr_d), fp32((lr_d / base_lr) * weight_decay)) of call k (0-based), as Python floats, formed in float64."""
    lr_d = np.float64(TABLE[min(k, len(TABLE) - 1)])
    return float(np.float32(lr_d)), float(np.float32((lr_d / np.float64(BASE_LR)) * np.float64(WD)))


def test_the_table_has_the_cases():
    assert len(TABLE) == 8 and 0.0 in TABLE and len(set(TABLE)) == 8
    assert any(float(np.float32(x)) != x for x in TABLE)                                     # not an fp32 number
    assert any(Fraction(x) / Fraction(BASE_LR) != Fraction(float(np.float64(x) / np.float64(BASE_LR))) for x in TABLE)
    # the single rounding matters: rounding lr to fp32 first gives another wd_factor for some entry
    assert any(float(np.float32((np.float64(np.float32(x)) / BASE_LR) * WD)) != lr_pair(k)[1] for k, x in enumerate(TABLE))


class Bufs:
    """p, m, v, the flags, the workspace, norm_out and the state block(s) of one size, all guarded."""

    def __init__(self, ch, seed, sched):
        lib = L.lib()
        self.ch, self.n, self.sched_entry = ch, ch * 256, sched
        n = self.n
        p0, m0, v0, flags = R.adam_state(n, seed)
        self.flags = flags
        self.p, self.m, self.v = (guarded(n, None, F32).fill_(x.to(DEV)) for x in (p0, m0, v0))
        self.fl = torch.empty(ch + 2 * KC.GUARD_BYTES, dtype=torch.uint8, device=DEV).fill_(0xA5)
        self.fl[KC.GUARD_BYTES:KC.GUARD_BYTES + ch] = flags.to(DEV)
        self.flv = self.fl[KC.GUARD_BYTES:KC.GUARD_BYTES + ch]
        self.wsb = lib.rgbnm_clip_adamw_wd_sched_workspace() if sched else lib.rgbnm_clip_adamw_wd_scaled_workspace()
        self.ws = guarded(self.wsb // 4, None, F32)
        self.norm = guarded(1, None, F32)
        self.state = guarded(8, None, F32)
        self.sched = guarded(8, None, F32)
        self.table = torch.full((len(TABLE) + 64,), float("nan"), dtype=torch.float64, device=DEV)     # NaN behind the table
        self.table[:len(TABLE)] = torch.tensor(TABLE, dtype=torch.float64)

    def set_state(self, scale, tracker, step, skipped):
        w = np.zeros(8, dtype=np.int32)
        w[:1].view(np.float32)[0] = scale
        w[1:4] = (tracker, step, skipped)
        w[4:5].view(np.float32)[0] = 0.5            # found_inf: neither 0 nor 1 before the first call
        self.state.raw[self.state.off:self.state.off + 8] = torch.from_numpy(w).to(DEV)

    def set_sched(self, it):
        w = np.zeros(8, dtype=np.int32)
        w[0] = it
        w[1:3].view(np.float32)[:] = (-1.0, -1.0)   # lr, wd_factor: values no call leaves
        self.sched.raw[self.sched.off:self.sched.off + 8] = torch.from_numpy(w).to(DEV)

    def state_words(self):
        return self.state.raw[self.state.off:self.state.off + 8].clone()

    def sched_words(self):
        return self.sched.raw[self.sched.off:self.sched.off + 8].clone()

    def call_sched(self, g, max_norm=1.0, interval=INTERVAL, growth=GROWTH, backoff=BACKOFF, smin=SMIN, smax=SMAX, tlen=len(TABLE)):
        L.check(L.lib().rgbnm_clip_adamw_wd_step_sched(
            self.p.t.data_ptr(), g.data_ptr(), self.m.t.data_ptr(), self.v.t.data_ptr(), self.flv.data_ptr(), self.n,
            self.table.data_ptr(), tlen, BASE_LR, WD, H["beta1"], H["beta2"], H["eps"], max_norm, self.norm.t.data_ptr(),
            self.state.t.data_ptr(), self.sched.t.data_ptr(), growth, backoff, interval, smin, smax, self.ws.t.data_ptr(),
            self.wsb, L.stream()))

    def call_scaled(self, g, lr, wd_factor, max_norm=1.0, interval=INTERVAL, growth=GROWTH, backoff=BACKOFF, smin=SMIN, smax=SMAX):
        L.check(L.lib().rgbnm_clip_adamw_wd_step_scaled(
            self.p.t.data_ptr(), g.data_ptr(), self.m.t.data_ptr(), self.v.t.data_ptr(), self.flv.data_ptr(), self.n, lr,
            H["beta1"], H["beta2"], H["eps"], wd_factor, max_norm, self.norm.t.data_ptr(), self.state.t.data_ptr(), growth,
            backoff, interval, smin, smax, self.ws.t.data_ptr(), self.wsb, L.stream()))

    def snapshot(self):
        return self.p.t.clone(), self.m.t.clone(), self.v.t.clone(), self.norm.t.clone(), self.state_words()

    def check_guards(self, where):
        outs = [(self.p, "p"), (self.m, "m"), (self.v, "v"), (self.ws, "workspace"), (self.state, "state"), (self.norm, "norm_out")]
        if self.sched_entry:
            outs.append((self.sched, "sched"))
        for o, nm in outs:
            o.check(f"{where} {nm}")
        G = KC.GUARD_BYTES
        assert bool((self.fl[:G] == 0xA5).all()) and bool((self.fl[G + self.ch:] == 0xA5).all()), where + " flag guards"
        assert torch.equal(self.flv.cpu(), self.flags), where + " flags changed"
        assert bool(torch.isnan(self.table[len(TABLE):]).all()), where + " table tail"
        assert self.table[:len(TABLE)].tolist() == list(TABLE), where + " table changed"


def grad(n, scale, seed, bad=False):
    """g * scale in fp32 with NaN behind it; bad: one inf in the middle."""
    g = R.adam_grad(n, 1.0, seed) * torch.tensor(scale, dtype=F32)
    dev = torch.full((n + 256,), float("nan"), dtype=F32, device=DEV)
    dev[:n] = g.to(DEV)
    if bad:
        dev[n // 2] = float("inf")
    return dev[:n]


def same(a, b):
    return bool(R.same_bits(a, b).all())


def f32_bits(x):
    return int(np.array([x], dtype=np.float32).view(np.int32)[0])


def tail_kernels(names):
    return [nm for nm in names if "sqnorm" in nm or "adamw" in nm]         # the kernels of all three tail entries


@pytest.mark.parametrize("ch", CHUNKS)
def test_ten_calls_equal_the_scaled_entry_bit_for_bit(ch):
    a, b = Bufs(ch, 3000 + ch, True), Bufs(ch, 3000 + ch, False)
    scale, tracker, step0, skipped0 = 65536.0, 0, 11, 2
    for c in (a, b):
        c.set_state(scale, tracker, step0, skipped0)
    a.set_sched(0)
    grads, bads = [], []
    for k in range(CALLS):                       # every call's gradients carry the scale of that call
        bad = k == BAD_CALL
        grads.append(grad(a.n, scale, 3100 + ch + k, bad))
        bads.append(bad)
        scale, tracker = LS.update_scale(scale, tracker, bad, GROWTH, BACKOFF, INTERVAL, SMIN, SMAX)
    snaps_a, scheds, snaps_b = [], [], []

    def run():
        for k in range(CALLS):
            a.call_sched(grads[k])
            snaps_a.append(a.snapshot())
            scheds.append(a.sched_words())
    _, names = launched(run)
    ours = tail_kernels(names)
    assert (sum("sqnorm_unscale_sched_kernel" in nm for nm in ours), sum("adamw_sched_kernel" in nm for nm in ours),
            len(ours)) == (CALLS, CALLS, 2 * CALLS), f"n/256={ch}: {CALLS} calls launched {ours}"
    for k in range(CALLS):
        b.call_scaled(grads[k], *lr_pair(k))
        snaps_b.append(b.snapshot())
    a.check_guards(f"step_sched n/256={ch}")
    b.check_guards(f"step_scaled twin n/256={ch}")
    prev = None
    for k in range(CALLS):
        where = f"step_sched n/256={ch} call {k + 1}"
        for x, y, nm in zip(snaps_a[k], snaps_b[k], ("p", "m", "v", "norm_out", "loss-scale block")):
            assert same(x, y), f"{where}: {nm} differs from the scaled entry's"
        w = scheds[k].cpu().numpy()
        lr, wdf = lr_pair(k)
        assert int(w[0]) == k + 1, (where, w)
        assert (int(w[1]), int(w[2])) == (f32_bits(lr), f32_bits(wdf)), (where, w[1:3].view(np.float32), lr, wdf)
        assert w[3:].tolist() == [0] * 5, (where, w)
        st = snaps_a[k][4].cpu().numpy()
        if bads[k]:                              # iter advanced (above), the Adam step did not, nothing was written
            assert int(st[2]) == int(prev[4].cpu().numpy()[2]) and int(st[3]) == skipped0 + 1, (where, st)
            assert all(same(x, y) for x, y in zip(snaps_a[k][:3], prev[:3])), where + ": p, m, v written on a skipped step"
            assert not bool(torch.isfinite(snaps_a[k][3]).any()), where
        else:
            assert int(st[2]) == step0 + k + 1 - (k > BAD_CALL), (where, st)
            if prev is not None and lr_pair(k)[0] > 0:
                assert not same(snaps_a[k][0], prev[0]), where + ": p did not move"
        prev = snaps_a[k]
    # the scale changed along the way (growth at call 4, backoff at call 6), so the comparison saw more than one unscale factor
    scales = [float(s[4].cpu().numpy()[:1].view(np.float32)[0]) for s in snaps_a]
    assert scales[2] == 65536.0 and scales[3] == LS.update_scale(65536.0, 3, False, GROWTH, BACKOFF, INTERVAL)[0]
    assert scales[BAD_CALL] == LS.update_scale(scales[3], 1, True, GROWTH, BACKOFF, INTERVAL)[0] and scales[-1] == scale


def test_the_neutral_block_is_the_plain_step():
    """scale 1, factors 1, clamp [1, 1]: what FusedClipAdamWWD passes when no DeviceLossScaler is given."""
    lib = L.lib()
    worst = KC.Worst()
    ch = 257
    a, b, c = Bufs(ch, 4000, True), Bufs(ch, 4000, False), Bufs(ch, 4000, False)
    for x in (a, b):
        x.set_state(1.0, 0, 0, 0)
    a.set_sched(0)
    neutral = dict(interval=600, growth=1.0, backoff=1.0, smin=1.0, smax=1.0)
    plain_ws = guarded(lib.rgbnm_clip_adamw_wd_workspace() // 4, None, F32)
    for k in range(3):
        g = grad(a.n, 1.0, 4100 + k)
        lr, wdf = lr_pair(k)
        before = c.snapshot()
        a.call_sched(g, **neutral)
        b.call_scaled(g, lr, wdf, **neutral)
        L.check(lib.rgbnm_clip_adamw_wd_step(c.p.t.data_ptr(), g.data_ptr(), c.m.t.data_ptr(), c.v.t.data_ptr(), c.flv.data_ptr(),
                                             c.n, lr, H["beta1"], H["beta2"], H["eps"], k + 1, wdf, 1.0, c.norm.t.data_ptr(),
                                             plain_ws.t.data_ptr(), lib.rgbnm_clip_adamw_wd_workspace(), L.stream()))
        where = f"neutral block call {k + 1}"
        sa, sb, sc = a.snapshot(), b.snapshot(), c.snapshot()
        for x, y, nm in zip(sa, sb, ("p", "m", "v", "norm_out", "loss-scale block")):
            assert same(x, y), f"{where}: {nm} differs from the scaled entry's"
        for i, nm in ((1, "m"), (2, "v"), (3, "norm_out")):
            assert same(sa[i], sc[i]), f"{where}: {nm} differs from the plain entry's"
        st = sa[4].cpu().numpy()
        assert float(st[:1].view(np.float32)[0]) == 1.0 and st[1:4].tolist() == [k + 1, k + 1, 0], (where, st)
        # p: the plain entry's fp64 reference and bound, plus BC_EXTRA |update| for the device-side bias corrections
        hyper = dict(H, lr=lr, wd_factor=wdf)
        r = R.adamw_ref(before[0], g, before[1], before[2], c.flags, k + 1, 1.0, **hyper)
        R.adam_check(dict(p=sc[0], m=sc[1], v=sc[2], norm=sc[3]), r, where + " plain", worst)
        r["dp"] = r["dp"] + LS.bias_correction_extra(r, before[0], c.flags, k + 1, **hyper)
        R.adam_check(dict(p=sa[0], m=sa[1], v=sa[2], norm=sa[3]), r, where + " sched", worst)
    a.check_guards("neutral block")
    worst.report("step_sched neutral block")


def test_refusals_launch_nothing_and_leave_both_blocks_untouched():
    lib = L.lib()
    c = Bufs(2, 5000, True)
    g = grad(c.n, 65536.0, 5001)
    c.set_state(65536.0, 1, 2, 3)
    c.set_sched(4)
    want_state, want_sched, before = c.state_words(), c.sched_words(), c.snapshot()

    def call(n=c.n, state=True, sched=True, table=True, tlen=len(TABLE), base_lr=BASE_LR, wd=WD, interval=600, growth=GROWTH,
             backoff=BACKOFF, smin=SMIN, smax=SMAX, wsb=c.wsb, gp=True):
        return lib.rgbnm_clip_adamw_wd_step_sched(
            c.p.t.data_ptr(), g.data_ptr() if gp else None, c.m.t.data_ptr(), c.v.t.data_ptr(), c.flv.data_ptr(), n,
            c.table.data_ptr() if table else None, tlen, base_lr, wd, H["beta1"], H["beta2"], H["eps"], 1.0, None,
            c.state.t.data_ptr() if state else None, c.sched.t.data_ptr() if sched else None, growth, backoff, interval, smin, smax,
            c.ws.t.data_ptr(), wsb, L.stream())

    def refusals():
        assert call(table=False) == EINVAL and call(sched=False) == EINVAL
        assert call(tlen=0) == EINVAL and call(tlen=-3) == EINVAL
        assert call(base_lr=0.0) == EINVAL and call(base_lr=-1e-3) == EINVAL and call(base_lr=float("nan")) == EINVAL
        assert call(wd=float("nan")) == EINVAL and call(wd=-0.05) == EINVAL
        # ... and everything the scaled entry refuses
        assert call(gp=False) == EINVAL and call(state=False) == EINVAL
        assert call(n=500) == EINVAL and call(n=0) == EINVAL
        assert call(interval=0) == EINVAL
        assert call(growth=0.0) == EINVAL and call(backoff=-0.5) == EINVAL
        assert call(smin=4.0, smax=2.0) == EINVAL
        assert call(wsb=1024) == EWORKSPACE and call(wsb=c.wsb - 4) == EWORKSPACE
        assert call(wsb=lib.rgbnm_clip_adamw_wd_scaled_workspace()) == EWORKSPACE
    _, names = launched(refusals)
    assert tail_kernels(names) == [], names
    assert torch.equal(c.state_words(), want_state) and torch.equal(c.sched_words(), want_sched)
    assert all(same(x, y) for x, y in zip(before[:3], c.snapshot()[:3]))
    assert bool((c.ws.raw == c.ws.canary).all()) and bool((c.norm.raw == c.norm.canary).all())
