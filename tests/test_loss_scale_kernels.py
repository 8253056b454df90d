"""Element-wise tests of rgbnm_clip_adamw_wd_step_scaled (csrc/embed_tail.hip: sqnorm_unscale_kernel, adamw_scaled_kernel) in
the conventions of test_step_ends.py: guarded state and outputs, NaN behind the gradients, a workspace of exactly the size
asked for, the device kernels counted, every element against the fp64 reference of step_ends_ref.adamw_ref, the state block
against tests/loss_scale_ref.py after every call.

The reference gets fp32(g_scaled * inv), formed on the host with the kernel's two fp32 operations (inv = fp32(1 / fp64(scale)),
one fp32 product), so adamw_ref's bounds for p, m, v and the norm apply unchanged -- plus, on p only, loss_scale_ref.BC_EXTRA
|update| for the bias corrections, which the kernel takes from an fp64 pow on the device: at most one fp32 ulp each on bc1 and
bc2_sqrt next to a rounding tie (derivation in loss_scale_ref's header).

Sizes (in chunks of 256): 1, 4, 257, 1025, 4097, 4096 * 3 + 5 -- every stride tail of the norm loop (262144 elements per stride,
four strides per turn) and one to four turns of the update's grid of at most 4096 workgroups.

Worst ratios |got - ref| / bound measured on one MI355X (the keys -s prints): [p 0.469, m 0.387, v 0.346, norm 0.046].
"""
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
CHUNKS = (1, 4, 257, 1025, 4097, 4096 * 3 + 5)
STRIDE = R.NORM_STRIDE                      # 262144 elements
GROWTH, BACKOFF, SMIN, SMAX = 1.6, 0.625, 2.0 ** -4, 2.0 ** 18
SCALE_16 = LS.update_scale(65536.0, 0, False, GROWTH, BACKOFF, 1)[0]        # f32(65536 * 1.6) = 104857.6015625
H = R.ADAM_HYPER


class Case:
    """p, m, v, the flags, the workspace, norm_out and the state block of one size, all guarded."""

    def __init__(self, ch, seed):
        lib = L.lib()
        self.ch, self.n = ch, ch * 256
        n = self.n
        p0, m0, v0, flags = R.adam_state(n, seed)
        self.flags = flags
        self.p, self.m, self.v = (guarded(n, None, F32).fill_(x.to(DEV)) for x in (p0, m0, v0))
        self.fl = torch.empty(ch + 2 * KC.GUARD_BYTES, dtype=torch.uint8, device=DEV).fill_(0xA5)
        self.fl[KC.GUARD_BYTES:KC.GUARD_BYTES + ch] = flags.to(DEV)
        self.flv = self.fl[KC.GUARD_BYTES:KC.GUARD_BYTES + ch]
        self.wsb = lib.rgbnm_clip_adamw_wd_scaled_workspace()
        self.ws = guarded(self.wsb // 4, None, F32)
        self.norm = guarded(1, None, F32)
        self.state = guarded(8, None, F32)

    def set_state(self, scale, tracker, step, skipped):
        w = np.zeros(8, dtype=np.int32)
        w[:1].view(np.float32)[0] = scale
        w[1:4] = (tracker, step, skipped)
        w[4:5].view(np.float32)[0] = 0.5            # found_inf: neither 0 nor 1 before the first call
        self.state.raw[self.state.off:self.state.off + 8] = torch.from_numpy(w).to(DEV)

    def get_state(self):
        w = self.state.raw[self.state.off:self.state.off + 8].cpu().numpy()
        return dict(scale=float(w[:1].view(np.float32)[0]), tracker=int(w[1]), step=int(w[2]), skipped=int(w[3]),
                    found_inf=float(w[4:5].view(np.float32)[0]), reserved=w[5:].tolist())

    def call(self, g, max_norm=1.0, interval=600, smin=SMIN, smax=SMAX, with_norm=True):
        L.check(L.lib().rgbnm_clip_adamw_wd_step_scaled(
            self.p.t.data_ptr(), g.data_ptr(), self.m.t.data_ptr(), self.v.t.data_ptr(), self.flv.data_ptr(), self.n, H["lr"],
            H["beta1"], H["beta2"], H["eps"], H["wd_factor"], max_norm, self.norm.t.data_ptr() if with_norm else None,
            self.state.t.data_ptr(), GROWTH, BACKOFF, interval, smin, smax, self.ws.t.data_ptr(), self.wsb, L.stream()))

    def snapshot(self):
        return self.p.t.clone(), self.m.t.clone(), self.v.t.clone()

    def check_guards(self, where, norm_written=True):
        for o, nm in ((self.p, "p"), (self.m, "m"), (self.v, "v"), (self.ws, "workspace"), (self.state, "state")):
            o.check(f"{where} {nm}")
        self.norm.check(f"{where} norm_out", written=norm_written)
        G = KC.GUARD_BYTES
        assert bool((self.fl[:G] == 0xA5).all()) and bool((self.fl[G + self.ch:] == 0xA5).all()), where + " flag guards"
        assert torch.equal(self.flv.cpu(), self.flags), where + " flags changed"


def scaled_grad(n, scale, seed):
    """(the upload g * scale in fp32 with NaN behind it, fp32(upload * inv): what the reference is given)."""
    g = R.adam_grad(n, 1.0, seed)
    up = g * torch.tensor(scale, dtype=F32)
    dev = torch.full((n + 256,), float("nan"), dtype=F32, device=DEV)
    dev[:n] = up.to(DEV)
    unscaled = dev[:n] * torch.tensor(LS.inv_of(scale), dtype=F32, device=DEV)
    return dev[:n], unscaled


def count_launches(names, steps, where):
    # every kernel of the library sits in an unnamed namespace; "sqnorm" / "adamw" also name the unscaled entry's pair
    ours = [nm for nm in names if any(s in nm for s in ("anonymous namespace", "_GLOBAL__N_", "rgbnm", "sqnorm", "adamw"))]
    nn = sum("sqnorm_unscale_kernel" in nm for nm in ours)
    na = sum("adamw_scaled_kernel" in nm for nm in ours)
    assert nn == steps and na == steps and len(ours) == 2 * steps, f"{where}: {steps} steps launched {ours}"


def same(a, b):
    return bool(R.same_bits(a, b).all())


def check_step(c, before, after, unscaled, step, max_norm, where, worst, with_norm=True):
    r = R.adamw_ref(before[0], unscaled, before[1], before[2], c.flags, step, max_norm, **H)
    r["dp"] = r["dp"] + LS.bias_correction_extra(r, before[0], c.flags, step, **H)
    R.adam_check(dict(p=after[0], m=after[1], v=after[2], norm=c.norm.t.clone() if with_norm else None), r, where, worst)
    return r


def finite_run(c, scale, step0, steps, seed, worst, max_norm=1.0):
    c.set_state(scale, 3, step0, 1)
    grads = [scaled_grad(c.n, scale, seed + k) for k in range(steps)]
    snaps, states, norms = [], [], []

    def run():
        for k in range(steps):
            before = c.snapshot()
            c.call(grads[k][0], max_norm=max_norm)
            snaps.append((before, c.snapshot()))
            norms.append(c.norm.t.clone())
            states.append(c.get_state())
    _, names = launched(run)
    where = f"step_scaled n/256={c.ch} scale={scale} max_norm={max_norm}"
    count_launches(names, steps, where)
    c.check_guards(where)
    for k, (before, after) in enumerate(snaps):
        w = f"{where} step={step0 + k + 1}"
        c.norm.t.copy_(norms[k])
        r = check_step(c, before, after, grads[k][1], step0 + k + 1, max_norm, w, worst)
        if max_norm > 0:
            assert r["coef"] < 0.5, w                  # the clip is active: the unscaled norm is far above 1
        st = states[k]
        assert st == dict(scale=scale, tracker=3 + k + 1, step=step0 + k + 1, skipped=1, found_inf=0.0, reserved=[0, 0, 0]), (w, st)


@pytest.mark.parametrize("ch", CHUNKS)
def test_finite_steps(ch):
    """Three consecutive steps from the kernel's own state at scale 2^16, then one at f32(65536 * 1.6) (an inv that is not a
    power of two) from a late step count; exactly one norm and one update launch per step."""
    worst = KC.Worst()
    c = Case(ch, 6000 + ch)
    finite_run(c, 65536.0, 0, 3, 6100 + ch, worst)
    finite_run(c, SCALE_16, 999, 1, 6200 + ch, worst)
    worst.report(f"step_scaled n/256={ch}")


def positions(n):
    pos = [0, n - 1]
    for b in range(STRIDE, n, STRIDE):
        pos += [b - 1, b]
    return sorted(set(pos))


@pytest.mark.parametrize("ch", CHUNKS)
def test_nonfinite_is_detected_everywhere_and_the_step_is_skipped(ch):
    """One inf, then one NaN, at index 0, at n - 1 and on both sides of every stride boundary of the norm loop."""
    c = Case(ch, 7000 + ch)
    n = c.n
    g, unscaled = scaled_grad(n, 65536.0, 7100 + ch)
    before = c.snapshot()
    want_scale, want_tracker = LS.update_scale(65536.0, 5, True, GROWTH, BACKOFF, 600, SMIN, SMAX)
    assert (want_scale, want_tracker) == (40960.0, 0)
    skipped = 2
    for idx in positions(n):
        for bad in (float("inf"), float("nan"), float("-inf")):
            keep = g[idx].clone()
            g[idx] = bad
            c.set_state(65536.0, 5, 7, skipped)
            c.call(g)
            st = c.get_state()
            g[idx] = keep
            where = f"step_scaled n/256={ch} g[{idx}]={bad}"
            skipped += 1
            assert st == dict(scale=want_scale, tracker=want_tracker, step=7, skipped=skipped, found_inf=1.0,
                              reserved=[0, 0, 0]), (where, st)
            assert not bool(torch.isfinite(c.norm.t).any()), where + " norm_out is finite"
            assert same(c.p.t, before[0]) and same(c.m.t, before[1]) and same(c.v.t, before[2]), where + ": state written"
    c.check_guards(f"step_scaled n/256={ch} non-finite")
    # the restored gradient takes the step on the same buffers
    c.set_state(65536.0, 5, 7, skipped)
    c.call(g)
    st = c.get_state()
    assert st == dict(scale=65536.0, tracker=6, step=8, skipped=skipped, found_inf=0.0, reserved=[0, 0, 0]), st
    check_step(c, before, c.snapshot(), unscaled, 8, 1.0, f"step_scaled n/256={ch} after the skips", KC.Worst())


def test_scale_sequence_with_a_scale_that_changes_every_step():
    """growth_interval 1 at the largest size: ok, ok, inf, ok.  Every step's gradients carry the scale of that step; an update
    workgroup that read the state after workgroup 0 rewrote it would unscale by the next scale (a factor 1.6 or 0.625)."""
    worst = KC.Worst()
    ch = CHUNKS[-1]
    c = Case(ch, 8000)
    scale, tracker, step, skipped = 65536.0, 0, 0, 0
    c.set_state(scale, tracker, step, skipped)
    for k, found in enumerate((0, 0, 1, 0)):
        g, unscaled = scaled_grad(c.n, scale, 8100 + k)
        if found:
            g[c.n // 2] = float("inf")
        before = c.snapshot()
        _, names = launched(lambda: c.call(g, interval=1))
        where = f"scale sequence call {k} scale={scale}"
        count_launches(names, 1, where)
        after = c.snapshot()
        scale, tracker = LS.update_scale(scale, tracker, bool(found), GROWTH, BACKOFF, 1, SMIN, SMAX)
        step, skipped = step + (not found), skipped + found
        st = c.get_state()
        assert st == dict(scale=scale, tracker=tracker, step=step, skipped=skipped, found_inf=float(found),
                          reserved=[0, 0, 0]), (where, st)
        if found:
            assert all(same(a, b) for a, b in zip(before, after)), where + ": state written on a skipped step"
            assert not bool(torch.isfinite(c.norm.t).any()), where
        else:
            check_step(c, before, after, unscaled, step, 1.0, where, worst)
    assert scale == LS.run_sequence(65536.0, (0, 0, 1, 0), GROWTH, BACKOFF, 1, SMIN, SMAX)[-1][0] == 167772.15625
    c.check_guards("scale sequence")
    worst.report("step_scaled scale sequence")


def test_clamp_on_the_device():
    """A growth from 2^18 stays at 2^18, a backoff from 2^-4 stays at 2^-4; scale_max = inf lets 2^40 back off to 2^40 * 0.625."""
    c = Case(4, 8500)
    g, _ = scaled_grad(c.n, 1.0, 8501)
    c.set_state(2.0 ** 18, 0, 0, 0)
    c.call(g, interval=1)
    assert c.get_state()["scale"] == 2.0 ** 18 and c.get_state()["found_inf"] == 0.0
    bad = g.clone()
    bad[5] = float("nan")
    c.set_state(2.0 ** -4, 0, 0, 0)
    c.call(bad, interval=1)
    assert c.get_state()["scale"] == 2.0 ** -4 and c.get_state()["skipped"] == 1
    c.set_state(2.0 ** 40, 0, 0, 0)
    c.call(bad)
    assert c.get_state()["scale"] == 2.0 ** 18
    c.set_state(2.0 ** 40, 0, 0, 0)
    c.call(bad, smax=float("inf"))
    assert c.get_state()["scale"] == 2.0 ** 40 * 0.625
    c.check_guards("clamp")


def test_no_clip_still_unscales_and_still_checks():
    worst = KC.Worst()
    c = Case(257, 9000)
    finite_run(c, SCALE_16, 4, 2, 9100, worst, max_norm=0.0)
    g, _ = scaled_grad(c.n, SCALE_16, 9200)
    g[c.n - 1] = float("inf")
    before = c.snapshot()
    c.set_state(SCALE_16, 0, 6, 0)
    c.call(g, max_norm=0.0, with_norm=False)
    st = c.get_state()
    assert st["found_inf"] == 1.0 and st["skipped"] == 1 and st["step"] == 6, st
    assert st["scale"] == LS.update_scale(SCALE_16, 0, True, GROWTH, BACKOFF, 600, SMIN, SMAX)[0]
    assert all(same(a, b) for a, b in zip(before, c.snapshot()))
    worst.report("step_scaled max_norm=0")


def test_refusals_leave_the_state_untouched():
    lib = L.lib()
    c = Case(2, 9500)
    g, _ = scaled_grad(c.n, 65536.0, 9501)
    c.set_state(65536.0, 1, 2, 3)
    want = c.get_state()
    before = c.snapshot()

    def call(n=c.n, state=True, interval=600, growth=GROWTH, backoff=BACKOFF, smin=SMIN, smax=SMAX, wsb=c.wsb, gp=True):
        return lib.rgbnm_clip_adamw_wd_step_scaled(
            c.p.t.data_ptr(), g.data_ptr() if gp else None, c.m.t.data_ptr(), c.v.t.data_ptr(), c.flv.data_ptr(), n, H["lr"],
            H["beta1"], H["beta2"], H["eps"], H["wd_factor"], 1.0, None, c.state.t.data_ptr() if state else None, growth, backoff,
            interval, smin, smax, c.ws.t.data_ptr(), wsb, L.stream())
    assert call(gp=False) == EINVAL and call(state=False) == EINVAL
    assert call(n=500) == EINVAL and call(n=0) == EINVAL
    assert call(wsb=1024) == EWORKSPACE and call(wsb=c.wsb - 4) == EWORKSPACE
    assert call(interval=0) == EINVAL
    assert call(growth=0.0) == EINVAL and call(backoff=-0.5) == EINVAL
    assert call(smin=4.0, smax=2.0) == EINVAL
    torch.cuda.synchronize()
    assert c.get_state() == want
    assert all(same(a, b) for a, b in zip(before, c.snapshot()))
    assert bool((c.ws.raw == c.ws.canary).all()) and bool((c.norm.raw == c.norm.canary).all())
