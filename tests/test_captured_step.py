"""The whole train step as one HIP graph (rgb_no_more_amd.graphstep.CapturedTrainStep) against today's eager loop.

The eager loop is the host-driven one through the EXISTING entries: param_groups[0]['lr'] set from the schedule's table before
every step, DeviceLossScaler + FusedClipAdamWWD.step (rgbnm_clip_adamw_wd_step_scaled), no schedule attached.  The captured loop
is capture() + replay() on static inputs refreshed in place, lr and wd_factor looked up on the device
(rgbnm_clip_adamw_wd_step_sched).  Every comparison is bit equality, after every step: the flat weights, both moment buffers,
the loss -- and under fp16 the scale, the skipped count and the Adam step.

ViT JPEG-Ti shape with depth 2, B = 4, 10 classes; warmup_cosine(LR, 3, 6): six steps cross the warm-up / cosine boundary and end
at lr 0.  SwinV2: the small three-stage model of tests/test_swin.py, drop_path_rate 0, two steps."""
import copy
import functools

import pytest
import torch

import rgb_no_more_amd as rg
from rgb_no_more_amd import detfill
from rgb_no_more_amd.custom_optims import DeviceLossScaler, DeviceLRSchedule, FusedClipAdamWWD

pytestmark = pytest.mark.gpu
DEV = "cuda"
F16, BF16 = torch.float16, torch.bfloat16
LR, WD, WARMUP, STEPS, B, NCLS = 1e-3, 0.05, 3, 6, 4, 10
NEUTRAL = dict(init_scale=1.0, growth_factor=1.0, backoff_factor=1.0, scale_min=1.0, scale_max=1.0)


def build_vit(cdt):
    m = rg.ViT(3, 16, 192, depth=2, n_classes=NCLS, drop_p=0.0, device=DEV, num_heads=3, head_size=64, pixel_space="DCT", ver=1,
               use_subblock=True)
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    m.load_state_dict({k: torch.from_numpy(v) for k, v in detfill.fill_state_dict(shapes, base_seed=1).items()})
    m.compute_dtype = cdt
    m.train()
    m._ensure_flat()
    return m


@functools.lru_cache(maxsize=None)
def vit_batches():
    out = []
    for k in range(STEPS):
        y = torch.from_numpy(detfill.normalish((B, 1, 28, 28, 8, 8), 710 + k)).to(DEV)
        c = torch.from_numpy(detfill.normalish((B, 2, 14, 14, 8, 8), 720 + k)).to(DEV)
        t = detfill.uniform((B, NCLS), 730 + k, 0.0, 1.0)
        out.append((y, c, torch.from_numpy(t / t.sum(1, keepdims=True)).to(DEV)))
    return out


def make_opt(m):
    return FusedClipAdamWWD(m, lr=LR, eps=1e-8, weight_decay=WD, max_norm=1.0)


def record(m, opt, loss, scaler):
    r = dict(w=m._flat.clone(), m=opt._exp_avg.clone(), v=opt._exp_avg_sq.clone(), loss=loss.detach().clone())
    if scaler is not None:
        r["scaler"] = scaler._device_state(m._flat.device)[:4].clone()          # scale, tracker, Adam step, skipped
    return r


def assert_same(got, want, where):
    for k in want:
        assert torch.equal(got[k], want[k]), f"{where}: {k} differs"


def eager_steps(m, batches, table, scaler, cdt, first=0):
    """Today's loop: a host-driven lr, the existing fused entries."""
    opt = make_opt(m)
    out = []
    for k, (y, c, t) in enumerate(batches):
        opt.param_groups[0]["lr"] = table[first + k]
        opt.zero_grad(set_to_none=True)
        loss = rg.cls_transforms.cross_entropy(m(y, c), t, grad_dtype=cdt)
        scaler.scale(loss).backward()
        scaler.step(opt)
        scaler.update()
        out.append(record(m, opt, loss, scaler))
    return out, opt


def captured_steps(m, opt, sched, scaler, batches):
    """capture() on static buffers, then one replay() per batch copied into them.  Everything on one side stream."""
    out = []
    torch.cuda.synchronize()
    with torch.cuda.stream(torch.cuda.Stream()):
        static = tuple(torch.zeros_like(x) for x in batches[0])
        for s, x in zip(static, batches[0]):
            s.copy_(x)
        step = rg.CapturedTrainStep(m, opt, sched, loss_scaler=scaler).capture(*static)
        for batch in batches:
            for s, x in zip(static, batch):
                s.copy_(x)
            loss = step.replay()
            out.append(record(m, opt, loss, scaler if scaler is not None else opt._neutral))
        torch.cuda.synchronize()
    return out, step


def table():
    return DeviceLRSchedule.warmup_cosine(LR, WARMUP, STEPS).values()


@functools.lru_cache(maxsize=None)
def eager_fp16(init_scale):
    scaler = DeviceLossScaler(init_scale=init_scale, growth_interval=2)
    return eager_steps(build_vit(F16), vit_batches(), table(), scaler, F16)[0]


def test_bf16_six_replays_equal_six_eager_steps():
    want, _ = eager_steps(build_vit(BF16), vit_batches(), table(), DeviceLossScaler(**NEUTRAL), BF16)
    m = build_vit(BF16)
    w0 = m._flat.clone()
    opt, sched = make_opt(m), DeviceLRSchedule.warmup_cosine(LR, WARMUP, STEPS)
    got, step = captured_steps(m, opt, sched, None, vit_batches())
    for k in range(STEPS):
        assert_same(got[k], want[k], f"bf16 step {k + 1}")
    assert sched.iteration() == STEPS and sched.state_dict() == {"iter": STEPS, "table_len": STEPS}
    assert sched.get_last_lr() == [0.0]
    assert not torch.equal(got[0]["w"], w0) and not torch.equal(got[4]["w"], got[3]["w"])
    assert torch.equal(got[5]["w"], got[4]["w"]) and not torch.equal(got[5]["m"], got[4]["m"])      # lr 0: only the moments move
    assert opt.skipped_steps() == 0 and float(opt.state_dict()["state"][0]["step"]) == float(STEPS)
    assert len({float(r["loss"]) for r in got}) == STEPS and step.loss is not None
    # the device goes on counting after a checkpoint read the count: a later state_dict() is not stale
    step.replay()
    torch.cuda.synchronize()
    assert float(opt.state_dict()["state"][0]["step"]) == float(STEPS + 1) and sched.iteration() == STEPS + 1


@pytest.mark.parametrize("init_scale", [2.0 ** 16, 2.0 ** 40])
def test_fp16_replays_follow_the_scale(init_scale):
    """growth_interval 2: the scale changes between replays; from 2^40 the first step overflows and is skipped."""
    want = eager_fp16(init_scale)
    m = build_vit(F16)
    opt, sched = make_opt(m), DeviceLRSchedule.warmup_cosine(LR, WARMUP, STEPS)
    scaler = DeviceLossScaler(init_scale=init_scale, growth_interval=2)
    got, _ = captured_steps(m, opt, sched, scaler, vit_batches())
    for k in range(STEPS):
        assert_same(got[k], want[k], f"fp16 init_scale={init_scale} step {k + 1}")
    assert sched.iteration() == STEPS
    skipped = scaler.skipped_steps()
    assert float(opt.state_dict()["state"][0]["step"]) == float(STEPS - skipped)
    scales = [init_scale] + [float(r["scaler"][:1].view(torch.float32)) for r in got]      # what each replay read, and the last
    assert len(set(scales[:-1])) > 1 and scaler.get_scale() == scales[-1]     # the replays saw more than one scale
    if init_scale == 2.0 ** 40:                  # the first replay overflowed: skipped, backed off and clamped, nothing written
        assert [int(x) for x in got[0]["scaler"][1:4]] == [0, 0, 1] and scales[1] == 2.0 ** 18
        assert not bool(got[0]["m"].any()) and skipped >= 1
    else:
        assert skipped == 0


def test_resume_after_three_replays_is_bit_exact():
    want = eager_fp16(2.0 ** 16)
    m = build_vit(F16)
    opt, sched = make_opt(m), DeviceLRSchedule.warmup_cosine(LR, WARMUP, STEPS)
    scaler = DeviceLossScaler(growth_interval=2)
    got, _ = captured_steps(m, opt, sched, scaler, vit_batches()[:3])
    assert_same(got[2], want[2], "before the checkpoint")
    ck = [copy.deepcopy(x.state_dict()) for x in (m, opt, scaler, sched)]
    assert ck[3] == {"iter": 3, "table_len": STEPS} and float(ck[1]["state"][0]["step"]) == 3.0

    m2 = build_vit(F16)
    m2.load_state_dict(ck[0])
    opt2, sched2, scaler2 = make_opt(m2), DeviceLRSchedule.warmup_cosine(LR, WARMUP, STEPS), DeviceLossScaler()
    opt2.load_state_dict(ck[1])
    scaler2.load_state_dict(ck[2])
    sched2.load_state_dict(ck[3])
    got2, _ = captured_steps(m2, opt2, sched2, scaler2, vit_batches()[3:])
    for k in range(3):
        for key in ("w", "m", "v", "loss"):
            assert torch.equal(got2[k][key], want[3 + k][key]), f"resumed step {4 + k}: {key} differs"
        assert torch.equal(got2[k]["scaler"][:3], want[3 + k]["scaler"][:3]), f"resumed step {4 + k}: scale / tracker / step"
    assert sched2.iteration() == STEPS and float(opt2.state_dict()["state"][0]["step"]) == float(STEPS)
    with pytest.raises(ValueError):
        DeviceLRSchedule.warmup_cosine(LR, WARMUP, STEPS + 1).load_state_dict(ck[3])


def test_refusals_and_the_attached_schedule_owns_the_lr():
    m = build_vit(BF16)
    opt, sched = make_opt(m), DeviceLRSchedule.warmup_cosine(LR, WARMUP, STEPS)
    m._grad_sync = object()
    with pytest.raises(RuntimeError, match="_grad_sync"):
        rg.CapturedTrainStep(m, opt, sched)
    m._grad_sync = None
    m.train_dropout = True
    with pytest.raises(RuntimeError, match="train_dropout"):
        rg.CapturedTrainStep(m, opt, sched)
    m.train_dropout = False
    with pytest.raises(RuntimeError, match="non-default stream"):
        rg.CapturedTrainStep(m, opt, sched).capture(*vit_batches()[0])
    with pytest.raises(TypeError):
        rg.CapturedTrainStep(m, torch.optim.AdamW(m.parameters()), sched)

    # an eager step with the schedule attached: param_groups[0]['lr'] is not read
    y, c, t = vit_batches()[0]
    results = []
    for host_lr in (LR, 123.0):
        mm = build_vit(BF16)
        o = make_opt(mm)
        o.attach_schedule(DeviceLRSchedule.warmup_cosine(LR, WARMUP, STEPS))
        o.param_groups[0]["lr"] = host_lr
        w0 = mm._flat.clone()
        rg.cls_transforms.cross_entropy(mm(y, c), t, grad_dtype=BF16).backward()
        o.step()
        results.append(mm._flat.clone())
        assert not torch.equal(results[-1], w0)
    assert torch.equal(results[0], results[1])
    # ... and it is the table's first entry that was used: the host loop with that lr gives the same weights
    want, _ = eager_steps(build_vit(BF16), vit_batches()[:1], table(), DeviceLossScaler(**NEUTRAL), BF16)
    assert torch.equal(results[0], want[0]["w"])
    # detached again, the host lr counts
    o.detach_schedule()
    assert float(o.state_dict()["state"][0]["step"]) == 1.0


def test_swinv2_two_replays_equal_two_eager_steps(golden):
    from test_swin import _load, _model
    g = golden("g15_swin.npz")

    def build():
        m, *_ = _model("sw3", DEV)                   # drop_path_rate 0: the masks would advance with the replays
        _, y, c, tgt = _load(m, "sw3", g)
        m.compute_dtype = BF16
        m.train()
        m._ensure_flat()
        return m, [(y, c, tgt), (y.flip(0).contiguous(), c.flip(0).contiguous(), tgt)]
    tab = table()
    m1, batches = build()
    want, _ = eager_steps(m1, batches, tab, DeviceLossScaler(**NEUTRAL), BF16)
    m2, _ = build()
    opt, sched = make_opt(m2), DeviceLRSchedule.warmup_cosine(LR, WARMUP, STEPS)
    got, _ = captured_steps(m2, opt, sched, None, batches)
    for k in range(2):
        assert_same(got[k], want[k], f"swinv2 step {k + 1}")
    assert sched.iteration() == 2 and not torch.equal(got[1]["w"], got[0]["w"])
