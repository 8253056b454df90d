"""train.py's AMP step (train.py:146-176) with the loss scaler on the device: DeviceLossScaler + FusedClipAdamWWD.

    scaler.scale(loss).backward(); scaler.step(optimizer); scaler.update()

replaces GradScaler.scale / unscale_ / clip_grad_norm_ / step / step / update / clip_gradscaler.  The model, inputs and oracle
are those of tests/test_train_loop_amp.py (depth 2, B = 8), the bars of the fp16 run those of tests/test_fp16_train_loop.py."""
import copy

import numpy as np
import pytest
import torch

import rgb_no_more_amd as rg
from rgb_no_more_amd.custom_optims import DeviceLossScaler, FusedClipAdamWWD
from test_train_loop_amp import LR, WARMUP, WD, build, oracle_steps

pytestmark = pytest.mark.gpu
F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16


def make_opt(m):
    return FusedClipAdamWWD(m, lr=LR, eps=1e-8, weight_decay=WD, max_norm=1.0)


def forward_loss(m, y, c, tgt, cdt):
    if cdt == F32:
        m.compute_dtype = F32
        logits = m(y, c)
    else:
        with torch.autocast("cuda", dtype=cdt):
            logits = m(y, c)
    return rg.cls_transforms.cross_entropy(logits, tgt, grad_dtype=cdt)


def loop_step(m, opt, scaler, y, c, tgt, itr, cdt):
    """train.py:146-167 with the device scaler; the warm-up learning rate of oracle_steps."""
    opt.zero_grad(set_to_none=True)
    if itr < WARMUP:
        opt.param_groups[0]["lr"] = LR * (itr + 1) / WARMUP
    loss = forward_loss(m, y, c, tgt, cdt)
    scaler.scale(loss).backward()
    scaler.step(opt)
    scaler.update()
    return loss


def weights(m):
    return {k: v.detach().clone() for k, v in m.state_dict().items()}


def run(cdt, steps, **scaler_args):
    m, sd, y, c, tgt = build()
    m.train()
    opt, scaler = make_opt(m), DeviceLossScaler(**scaler_args)
    losses = [loop_step(m, opt, scaler, y, c, tgt, i, cdt).item() for i in range(steps)]
    return m, opt, scaler, losses, (sd, y, c, tgt)


def test_fp32_power_of_two_scale_is_exact():
    """fp32 compute: scaling by 2^16 and unscaling are exact, so three steps equal three steps through the same entry at
    scale 1, bit for bit."""
    m1, o1, s1, l1, _ = run(F32, 3, init_scale=1.0)
    m2, o2, s2, l2, _ = run(F32, 3, init_scale=2.0 ** 16)
    assert l1 == l2
    w1, w2 = weights(m1), weights(m2)
    for k in w1:
        assert torch.equal(w1[k], w2[k]), k
    assert torch.equal(o1._exp_avg, o2._exp_avg) and torch.equal(o1._exp_avg_sq, o2._exp_avg_sq)
    assert float(o1._exp_avg.abs().sum()) > 0
    assert torch.equal(o1.last_norm, o2.last_norm) and bool(torch.isfinite(o2.last_norm).all())
    assert (s1.get_scale(), s2.get_scale()) == (1.0, 65536.0) and s1.skipped_steps() == s2.skipped_steps() == 0
    assert float(o2.state_dict()["state"][0]["step"]) == 3.0


def test_disabled_scaler_is_the_plain_step():
    m1, _, y, c, tgt = build()
    m2, _, _, _, _ = build()
    m1.train(), m2.train()
    o1, o2, off = make_opt(m1), make_opt(m2), DeviceLossScaler(enabled=False)
    for i in range(2):
        loop_step(m1, o1, off, y, c, tgt, i, F32)
        o2.zero_grad(set_to_none=True)
        o2.param_groups[0]["lr"] = LR * (i + 1) / WARMUP
        forward_loss(m2, y, c, tgt, F32).backward()
        o2.step()
    w1, w2 = weights(m1), weights(m2)
    for k in w1:
        assert torch.equal(w1[k], w2[k]), k
    assert off.get_scale() == 1.0 and off.state_dict() == {}


def test_fp16_loop_tracks_oracle():
    m, opt, scaler, losses, (sd, y, c, tgt) = run(F16, 3)
    assert m._cur_dtype == F16
    ol, ow = oracle_steps(sd, y.cpu(), c.cpu(), tgt.cpu(), 3)
    got = {k: v.detach().cpu().numpy() for k, v in m.state_dict().items()}
    diffs = np.concatenate([np.abs(got[k] - ow[k]).reshape(-1) for k in ow])
    print(f"fp16 device scaler: losses {losses} oracle {ol}; |w - w_oracle| median {np.median(diffs):.3e} max {diffs.max():.3e}; "
          f"scale {scaler.get_scale()} norm {float(opt.last_norm):.4f}")
    for a, b in zip(losses, ol):
        assert abs(a - b) < 2e-2, (losses, ol)
    assert np.median(diffs) < 5e-5 and diffs.max() < 6.5e-3
    assert scaler.get_scale() == 65536.0 and scaler.skipped_steps() == 0
    assert float(opt.state_dict()["state"][0]["step"]) == 3.0


@pytest.mark.parametrize("scale_max", [2.0 ** 18, float("inf")])
def test_fp16_overflow_skips_backs_off_and_trains_on(scale_max):
    m, sd, y, c, tgt = build()
    m.train()
    opt, scaler = make_opt(m), DeviceLossScaler(init_scale=2.0 ** 40, scale_max=scale_max)
    before = weights(m)
    loop_step(m, opt, scaler, y, c, tgt, 0, F16)
    for k, v in m.state_dict().items():
        assert torch.equal(v, before[k]), k
    assert not bool(opt._exp_avg.any()) and not bool(opt._exp_avg_sq.any())
    assert scaler.skipped_steps() == 1
    assert not bool(torch.isfinite(opt.last_norm).any())
    if scale_max == float("inf"):
        assert scaler.get_scale() == 2.0 ** 40 * 0.625
        return
    assert scaler.get_scale() == 2.0 ** 18                   # backed off, then clamped
    l2 = loop_step(m, opt, scaler, y, c, tgt, 1, F16).item()
    assert np.isfinite(l2)
    assert any(not torch.equal(v, before[k]) for k, v in m.state_dict().items())
    assert scaler.skipped_steps() == 1
    assert float(opt.state_dict()["state"][0]["step"]) == 1.0          # the skipped step did not count


def test_bf16_takes_the_step_at_the_same_scale():
    m, sd, y, c, tgt = build()
    m.train()
    opt, scaler = make_opt(m), DeviceLossScaler(init_scale=2.0 ** 40)
    before = weights(m)
    loss = loop_step(m, opt, scaler, y, c, tgt, 0, BF16).item()
    assert np.isfinite(loss) and scaler.skipped_steps() == 0
    assert any(not torch.equal(v, before[k]) for k, v in m.state_dict().items())
    assert float(opt.state_dict()["state"][0]["step"]) == 1.0


def test_the_step_does_not_sync_the_host():
    m, sd, y, c, tgt = build()
    m.train()
    opt, scaler = make_opt(m), DeviceLossScaler()
    loop_step(m, opt, scaler, y, c, tgt, 0, F16)
    opt.zero_grad(set_to_none=True)
    loss = forward_loss(m, y, c, tgt, F16)
    torch.cuda.synchronize()
    old = torch.cuda.get_sync_debug_mode()
    try:
        torch.cuda.set_sync_debug_mode("error")
    except Exception as e:                                   # a build without the mode
        pytest.skip(f"torch.cuda.set_sync_debug_mode('error') rejected: {e}")
    try:
        scaler.scale(loss).backward()
        scaler.step(opt)
        scaler.update()
    finally:
        torch.cuda.set_sync_debug_mode(old)
    torch.cuda.synchronize()
    assert scaler.skipped_steps() == 0 and float(opt.state_dict()["state"][0]["step"]) == 2.0


def test_checkpoint_resume_is_bit_exact():
    """growth_interval 2: after two steps the scale has grown to f32(65536 * 1.6), so the resumed third step needs the scale,
    the tracker and the device step count back exactly."""
    m, sd, y, c, tgt = build()
    m.train()
    opt, scaler = make_opt(m), DeviceLossScaler(growth_interval=2)
    for i in range(2):
        loop_step(m, opt, scaler, y, c, tgt, i, F16)
    ck_model, ck_opt, ck_scaler = copy.deepcopy(m.state_dict()), copy.deepcopy(opt.state_dict()), copy.deepcopy(scaler.state_dict())
    assert ck_scaler == {"scale": 104857.6015625, "growth_factor": 1.6, "backoff_factor": 0.625, "growth_interval": 2,
                         "_growth_tracker": 0}
    assert float(ck_opt["state"][0]["step"]) == 2.0
    cont = loop_step(m, opt, scaler, y, c, tgt, 2, F16).item()
    want = weights(m)

    m2, _, _, _, _ = build()
    m2.load_state_dict(ck_model)
    m2.train()
    opt2, scaler2 = make_opt(m2), DeviceLossScaler()
    opt2.load_state_dict(ck_opt)
    scaler2.load_state_dict(ck_scaler)
    resumed = loop_step(m2, opt2, scaler2, y, c, tgt, 2, F16).item()
    assert resumed == cont
    for k, v in m2.state_dict().items():
        assert torch.equal(v, want[k]), k
    assert torch.equal(opt2._exp_avg, opt._exp_avg) and torch.equal(opt2._exp_avg_sq, opt._exp_avg_sq)
    assert scaler2.state_dict() == scaler.state_dict()
    assert float(opt2.state_dict()["state"][0]["step"]) == 3.0
    # and the state is torch.amp.GradScaler's: the reference's checkpoint code can carry it
    ref = torch.amp.GradScaler("cuda", growth_factor=1.6, backoff_factor=0.625, growth_interval=600)
    ref.load_state_dict(scaler.state_dict())
    assert ref.state_dict() == scaler.state_dict()


def test_swinv2_fp16_step(golden):
    from test_swin_fp16_train_loop import _sw3
    m, names, y, c, tgt = _sw3(golden)
    m.train()
    opt, scaler = make_opt(m), DeviceLossScaler()
    before = weights(m)
    loss = loop_step(m, opt, scaler, y, c, tgt, 0, F16).item()
    assert np.isfinite(loss)
    assert scaler.skipped_steps() == 0 and scaler.get_scale() == 65536.0
    assert bool(torch.isfinite(opt.last_norm).all())
    assert any(not torch.equal(v, before[k]) for k, v in m.state_dict().items())
