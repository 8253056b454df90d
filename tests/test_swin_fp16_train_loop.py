"""The reference's unchanged training step (train.py:146-176) with its default AMP dtype, float16, driving SwinV2 -- the dtype
the reference's `--model-arch swinv2` recipe trains in (configs.py:18: AMPDTYPE 'fp16'): autocast(float16) -> torch
CrossEntropyLoss -> GradScaler(1.6, 0.625, 600) -> AdamW + WeightDecay, against the fp32 oracle (oracle/swin_torch.py) on the CPU.
At an absurd initial scale the fp16 gradients overflow and the step must be skipped.  Also the reference's eval entry with its
hard-coded float16 autocast (eval.py:36)."""
import numpy as np
import pytest
import torch

from rgb_no_more_amd import detfill
from rgb_no_more_amd import eval as rg_eval
from oracle import swin_torch as S
from oracle import vit_torch as V
from test_fp16_train_loop import SCALE, train_py_step
from test_swin import CASES, _load, _model
from test_train_loop_amp import LR, WARMUP, WD, reference_objects

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _sw3(golden):
    g = golden("g15_swin.npz")
    m, *_ = _model("sw3", DEV)
    names, y, c, tgt = _load(m, "sw3", g)
    return m, names, y, c, tgt


def oracle_steps(m, names, y, c, tgt, nsteps):
    """train.py's step in fp32 on the CPU: oracle forward, clip_grad_norm_(1), AdamW(weight_decay=0), WeightDecay."""
    img, depths, heads, B = CASES["sw3"]
    sd = {n: p.detach().cpu().numpy().copy() for n, p in m.named_parameters()}
    p = {k: torch.from_numpy(v.copy()).requires_grad_(True) for k, v in sd.items()}
    mm = [np.zeros_like(sd[k]) for k in names]
    vv = [np.zeros_like(sd[k]) for k in names]
    mask = [(".weight" in n) and ("lrnorm" not in n) for n in names]
    losses = []
    for step in range(1, nsteps + 1):
        lr = LR * step / WARMUP if step - 1 < WARMUP else LR
        for k in names:
            p[k].grad = None
        lo = V.soft_xent(S.swin_forward(p, y, c, depths, heads), tgt)
        lo.backward()
        losses.append(lo.item())
        V.clip_adamw_wd_step([p[k].detach().numpy() for k in names], [p[k].grad.numpy() for k in names], mm, vv, step,
                             lr, LR, WD, mask)
    return losses, {k: p[k].detach().numpy() for k in names}


def test_fp16_train_py_step_tracks_oracle(golden):
    """Default scale 65536, no step skipped, within the bars of tests/test_fp16_train_loop.py (the ViT in fp16)."""
    m, names, y, c, tgt = _sw3(golden)
    names = [n for n, _ in m.named_parameters()]
    ol, ow = oracle_steps(m, names, y.cpu(), c.cpu(), tgt.cpu(), 3)
    criterion, optimizer, weight_decayer, gradscaler = reference_objects(m)
    m.train()
    losses = [train_py_step(m, y, c, tgt, criterion, optimizer, weight_decayer, gradscaler, i) for i in range(3)]
    got = {n: p.detach().cpu().numpy() for n, p in m.named_parameters()}
    diffs = np.concatenate([np.abs(got[k] - ow[k]).reshape(-1) for k in ow])
    print(f"swin fp16: losses {losses} oracle {ol}; |w - w_oracle| median {np.median(diffs):.3e} max {diffs.max():.3e}; "
          f"scale {gradscaler.get_scale()}")
    for a, b in zip(losses, ol):
        assert abs(a - b) < 2e-2, (losses, ol)
    assert gradscaler.get_scale() == 65536.0                 # no inf/nan step was skipped
    assert np.median(diffs) < 5e-5 and diffs.max() < 6.5e-3


def test_huge_scale_overflows_fp16_and_the_step_is_skipped(golden):
    """init_scale 2^40: the scaled fp16 gradients overflow -> both optimizers skipped, weights bit-unchanged, scale x0.625, and the
    next step trains."""
    m, names, y, c, tgt = _sw3(golden)
    criterion, optimizer, weight_decayer, _ = reference_objects(m)
    gradscaler = torch.amp.GradScaler("cuda", init_scale=2.0 ** 40, growth_factor=1.6, backoff_factor=0.625, growth_interval=600)
    m.train()
    before = {k: v.detach().clone() for k, v in m.state_dict().items()}
    train_py_step(m, y, c, tgt, criterion, optimizer, weight_decayer, gradscaler, 0)
    assert not all(torch.isfinite(p.grad).all() for p in m.parameters())
    assert all(torch.equal(v, before[k]) for k, v in m.state_dict().items())
    assert SCALE["after_update"] == 2.0 ** 40 * 0.625
    assert optimizer.state == {} or all(len(s) == 0 for s in optimizer.state.values())
    l2 = train_py_step(m, y, c, tgt, criterion, optimizer, weight_decayer, gradscaler, 1)
    assert np.isfinite(l2)
    assert any(not torch.equal(v, before[k]) for k, v in m.state_dict().items())


def test_evaluate_model_with_the_reference_fp16_eval_autocast(golden):
    m, *_ = _sw3(golden)
    B, nb = 8, CASES["sw3"][0] // 8
    y = torch.from_numpy(detfill.normalish((B, 1, nb, nb, 8, 8), 181)).to(DEV)
    c = torch.from_numpy(detfill.normalish((B, 2, nb // 2, nb // 2, 8, 8), 182)).to(DEV)
    with torch.no_grad():
        m.compute_dtype = torch.float32
        labels = m(y, c).argmax(1)
    m.compute_dtype = None
    batches = [((y, c), labels)]
    acc16, loss16 = rg_eval.evaluate_model(m, batches, amp_dtype=torch.float16)
    acc32, loss32 = rg_eval.evaluate_model(m, batches, amp_dtype=None)
    print(f"swin eval: fp16 top-1 {acc16} loss {loss16:.6f}; fp32 top-1 {acc32} loss {loss32:.6f}")
    assert acc32 == 1.0
    assert np.isfinite(loss16) and abs(loss16 - loss32) < 5e-3
    assert abs(acc16 - acc32) <= 1 / B
