"""The reference's unchanged training step (train.py:146-176) with its default AMP dtype, float16: autocast(float16) ->
torch CrossEntropyLoss -> GradScaler(1.6, 0.625, 600) -> AdamW + WeightDecay, on the HIP model computing in fp16.  The scaler
now matters: at an absurd initial scale the fp16 gradients overflow and the step must be skipped, which bf16 (8-bit exponent)
never does at that scale.  Also the reference's eval entry with its hard-coded float16 autocast (eval.py:36)."""
import numpy as np
import pytest
import torch

from rgb_no_more_amd import eval as rg_eval
from test_train_loop_amp import LR, WARMUP, build, clip_gradscaler, oracle_steps, reference_objects

pytestmark = pytest.mark.gpu
DEV = "cuda"
SCALE = {}          # the scaler's scale right after update(), before the clamp of clip_gradscaler


def train_py_step(m, y, c, tgt, criterion, optimizer, weight_decayer, gradscaler, itr, dtype=torch.float16):
    """train.py:146-172, verbatim structure, autocast(dtype)."""
    optimizer.zero_grad()
    weight_decayer.zero_grad()
    if itr < WARMUP:
        for g in optimizer.param_groups:
            g["lr"] = LR * (itr + 1) / WARMUP
        for g in weight_decayer.param_groups:
            g["lr"] = optimizer.param_groups[0]["lr"]
    with torch.autocast("cuda", dtype=dtype):
        outputs = m(y, c)
        loss = criterion(outputs, tgt)
    gradscaler.scale(loss).backward()
    gradscaler.unscale_(optimizer)
    torch.nn.utils.clip_grad_norm_(m.parameters(), max_norm=1)
    gradscaler.step(optimizer)
    gradscaler.step(weight_decayer)
    gradscaler.update()
    SCALE["after_update"] = gradscaler.get_scale()        # (before pipeline_utils' clamp to [2^-4, 2^18])
    clip_gradscaler(gradscaler)
    return loss.item()


def test_fp16_train_py_step_tracks_oracle():
    """Default scale 65536, no step skipped, within the bars of tests/test_train_loop_amp.py (bf16 amp)."""
    m, sd, y, c, tgt = build()
    criterion, optimizer, weight_decayer, gradscaler = reference_objects(m)
    m.train()
    losses = [train_py_step(m, y, c, tgt, criterion, optimizer, weight_decayer, gradscaler, i) for i in range(3)]
    assert m._cur_dtype == torch.float16
    ol, ow = oracle_steps(sd, y.cpu(), c.cpu(), tgt.cpu(), 3)
    got = {k: v.detach().cpu().numpy() for k, v in m.state_dict().items()}
    diffs = np.concatenate([np.abs(got[k] - ow[k]).reshape(-1) for k in ow])
    print(f"fp16: losses {losses} oracle {ol}; |w - w_oracle| median {np.median(diffs):.3e} max {diffs.max():.3e}; "
          f"scale {gradscaler.get_scale()}")
    for a, b in zip(losses, ol):
        assert abs(a - b) < 2e-2, (losses, ol)
    assert gradscaler.get_scale() == 65536.0                 # no inf/nan step was skipped
    assert np.median(diffs) < 5e-5 and diffs.max() < 6.5e-3


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_huge_scale_overflows_fp16_only(dtype):
    """init_scale 2^40: the scaled fp16 gradients overflow -> both optimizers skipped, weights bit-unchanged, scale x0.625,
    and the next step trains.  bf16 carries the same scale without overflowing (the control)."""
    m, sd, y, c, tgt = build()
    criterion, optimizer, weight_decayer, _ = reference_objects(m)
    gradscaler = torch.amp.GradScaler("cuda", init_scale=2.0 ** 40, growth_factor=1.6, backoff_factor=0.625, growth_interval=600)
    m.train()
    before = {k: v.detach().clone() for k, v in m.state_dict().items()}
    train_py_step(m, y, c, tgt, criterion, optimizer, weight_decayer, gradscaler, 0, dtype)
    unchanged = all(torch.equal(v, before[k]) for k, v in m.state_dict().items())
    if dtype == torch.bfloat16:
        assert SCALE["after_update"] == 2.0 ** 40
        assert not unchanged
        return
    assert unchanged
    assert SCALE["after_update"] == 2.0 ** 40 * 0.625
    assert optimizer.state == {} or all(len(s) == 0 for s in optimizer.state.values())
    l2 = train_py_step(m, y, c, tgt, criterion, optimizer, weight_decayer, gradscaler, 1, dtype)
    assert np.isfinite(l2)
    assert any(not torch.equal(v, before[k]) for k, v in m.state_dict().items())


def test_fp16_gradients_overflow_at_a_huge_scale():
    """The overflow itself: the fp16 parameter gradients of a 2^40-scaled loss are non-finite."""
    m, sd, y, c, tgt = build()
    m.train()
    with torch.autocast("cuda", dtype=torch.float16):
        loss = torch.nn.CrossEntropyLoss()(m(y, c), tgt)
    (loss * 2.0 ** 40).backward()
    torch.cuda.synchronize()
    assert not all(torch.isfinite(p.grad).all() for p in m.parameters())


def test_evaluate_model_with_the_reference_fp16_eval_autocast():
    m, sd, y, c, tgt = build(B=8)
    labels = tgt.argmax(1)
    batches = [((y, c), labels)]
    acc16, loss16 = rg_eval.evaluate_model(m, batches, amp_dtype=torch.float16)
    acc32, loss32 = rg_eval.evaluate_model(m, batches, amp_dtype=None)
    assert np.isfinite(loss16) and abs(loss16 - loss32) < 1e-3
    assert abs(acc16 - acc32) <= 1 / 8
