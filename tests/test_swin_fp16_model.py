"""SwinV2 in fp16 compute mode (autocast(float16) or compute_dtype = torch.float16), forward and backward, against the reference
goldens (g15 sw3, g20 swt_b64, g21 swt_b256).  The bars calibrate themselves, as in tests/test_fp16_model.py: the same test measures
the bf16 mode on the same weights and inputs, and fp16 must come in at a quarter of its error or better -- for the logits, for the
gradients (the median over parameter tensors of the relative error against the fp32 mode's gradients; measured ratio 0.12 - 0.13)
and for g21's gradient slices (0.20).  The median error of the gradient NORMS against the reference shrinks less: measured fp16 / bf16
ratios 0.25 (g20, g21) and 0.31 (g15 sw3) -- the fp32 mode's own error is 5e-7, no floor -- so that bar is a third.  At the timed batch
(g21, B = 256) every logit must also be within 5e-3 of the reference (measured 2.4e-3)."""
import warnings

import numpy as np
import pytest
import torch

import rgb_no_more_amd as rg
from rgb_no_more_amd import detfill
from oracle import swin_torch as S
from test_swin import _load, _model

pytestmark = pytest.mark.gpu
DEV = "cuda"
LOSS_SCALE = 2.0 ** 16      # train.py's GradScaler starts here: without a scale, fp16 activation gradients underflow


def _swt(g, tag, B):
    m, img, depths, heads, _ = _model("swt", DEV)
    names = [str(n) for n in g[tag + "_names"]]
    shapes = S.param_shapes(depths, heads)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in S.fill_params({n: shapes[n] for n in names}).items()}, strict=False)
    nb = img // 8
    y = torch.from_numpy(detfill.normalish((B, 1, nb, nb, 8, 8), 171)).to(DEV)
    c = torch.from_numpy(detfill.normalish((B, 2, nb // 2, nb // 2, 8, 8), 172)).to(DEV)
    tgt = detfill.uniform((B, 1000), 173, 0.0, 1.0)
    tgt = torch.from_numpy(tgt / tgt.sum(1, keepdims=True)).to(DEV)
    return m, names, y, c, tgt


def step(m, y, c, tgt, dt):
    """forward under autocast(dt) (fp32: no autocast), the package's loss with a gradient in dt, backward of the loss scaled by
    LOSS_SCALE (a power of two: the same for every dtype), gradients unscaled."""
    m.train()
    m.compute_dtype = None
    m.zero_grad(set_to_none=True)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        with torch.autocast("cuda", dtype=dt, enabled=dt != torch.float32):
            logits = m(y, c)
    assert not [w for w in caught if "rgb-no-more_amd" in str(w.message)], [str(w.message) for w in caught]
    assert logits.dtype == dt
    loss = rg.cls_transforms.cross_entropy(logits, tgt, grad_dtype=dt)
    (loss * LOSS_SCALE).backward()
    torch.cuda.synchronize()
    grads = {n: p.grad.detach().double() / LOSS_SCALE for n, p in m.named_parameters()}
    return logits.detach().float().cpu().numpy(), loss.item(), grads


def _compare(g, tag, m, names, y, c, tgt, slices=False):
    """-> {dtype: (max |dlogit|, median grad-norm rel error, max grad-norm rel error, worst gradient slice rel error, |dloss|,
    median over tensors of the gradient rel error against the fp32 mode)}, every figure against the reference golden but the last."""
    out = {}
    g32 = None
    for dt in (torch.float32, torch.float16, torch.bfloat16):
        logits, loss, grads = step(m, y, c, tgt, dt)
        if dt == torch.float32:
            g32 = grads
        vs32 = np.median([((grads[n] - g32[n]).norm() / (g32[n].norm() + 1e-30)).item() for n in names])
        err = np.abs(logits - g[tag + "_logits"]).max()
        gn = np.array([grads[n].norm().item() for n in names])
        rel = np.abs(gn - g[tag + "_gradnorms"]) / (g[tag + "_gradnorms"] + 1e-9)
        worst = 0.0
        if slices:
            for nm in [str(x) for x in g[tag + "_slice_names"]]:
                got = grads[nm].reshape(-1)[::37].cpu().numpy()
                want = g[tag + "_grad_" + nm].astype(np.float64)
                worst = max(worst, float(np.linalg.norm(got - want) / (np.linalg.norm(want) + 1e-30)))
        dloss = abs(loss - float(g[tag + "_loss"]))
        assert np.isfinite(loss) and all(torch.isfinite(v).all() for v in grads.values())
        out[dt] = (err, np.median(rel), rel.max(), worst, dloss, vs32)
        print(f"[{tag} {dt}] max |dlogit| {err:.3e}, |dloss| {dloss:.2e}, grad-norm rel median {np.median(rel):.3e} "
              f"max {rel.max():.3e}" + (f", worst gradient slice rel {worst:.3e}" if slices else "") +
              f"; gradients vs the fp32 mode: median rel {vs32:.3e}")
    return out[torch.float16], out[torch.bfloat16], out[torch.float32]


def _bars(h, b, f):
    assert f[0] <= 1e-4                                  # the fp32 mode: the reference's logits
    assert h[0] <= b[0] / 4                              # logits
    assert h[5] <= b[5] / 4                              # gradients, against the fp32 mode
    assert h[1] <= b[1] / 3                              # gradient norms against the reference (see the module docstring)
    assert h[4] < 1e-3


def test_sw3_fp16_vs_reference_golden_and_bf16(golden):
    g = golden("g15_swin.npz")
    m, *_ = _model("sw3", DEV)
    names, y, c, tgt = _load(m, "sw3", g)
    _bars(*_compare(g, "sw3", m, names, y, c, tgt))


def test_swinv2t_b64_fp16_vs_reference_golden_and_bf16(golden):
    g = golden("g20_fullsize.npz")
    m, names, y, c, tgt = _swt(g, "swt_b64", 64)
    _bars(*_compare(g, "swt_b64", m, names, y, c, tgt))


def test_swinv2t_timed_batch_256_fp16_vs_reference_golden_and_bf16(golden):
    g = golden("g21_b256.npz")
    m, names, y, c, tgt = _swt(g, "swt_b256", 256)
    h, b, f = _compare(g, "swt_b256", m, names, y, c, tgt, slices=True)
    assert h[0] <= 5e-3                      # every one of the 256 x 1000 logits (measured 2.4e-3)
    _bars(h, b, f)
    assert h[3] <= b[3] / 4                  # the gradient slices


def test_autocast_and_compute_dtype_select_the_same_fp16_mode(golden):
    g = golden("g15_swin.npz")
    m, *_ = _model("sw3", DEV)
    names, y, c, tgt = _load(m, "sw3", g)
    m.eval()
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            a = m(y, c)
        m.compute_dtype = torch.float16
        with torch.no_grad():
            b = m(y, c)
            b2 = m(y.half(), c.half())           # fp16 inputs
    assert not [w for w in caught if "rgb-no-more_amd" in str(w.message)], [str(w.message) for w in caught]
    assert a.dtype == b.dtype == torch.float16
    assert torch.equal(a, b)
    assert torch.isfinite(b2).all()
    # fp16 inputs are widened exactly: the logits of the same values fed as fp32
    with torch.no_grad():
        b3 = m(y.half().float(), c.half().float())
    assert torch.equal(b2, b3)
    assert np.abs(b.float().cpu().numpy() - g["sw3_logits"]).max() < 1e-2


def test_fp16_training_forward_with_drop_path(golden):
    g = golden("g15_swin.npz")
    m, *_ = _model("sw3", DEV)
    names, y, c, tgt = _load(m, "sw3", g)
    for ly in m.layers:
        for blk in ly.blocks:
            blk.drop_path_p = 0.5
    m.train()
    m.compute_dtype = torch.float16
    torch.manual_seed(0)
    a = m(y, c)
    rg.cls_transforms.cross_entropy(a, tgt, grad_dtype=torch.float16).backward()
    b = m(y, c)
    torch.cuda.synchronize()
    assert a.dtype == torch.float16 and torch.isfinite(a).all() and torch.isfinite(b).all()
    assert not torch.equal(a, b)                 # other samples dropped
    assert all(torch.isfinite(p.grad).all() for p in m.parameters() if p.grad is not None)


def test_fp16_step_is_bit_reproducible(golden):
    g = golden("g15_swin.npz")
    m, *_ = _model("swt", DEV)
    names, y, c, tgt = _load(m, "swt", g)
    m.train()
    m.compute_dtype = torch.float16
    runs = []
    for _ in range(3):
        for p in m.parameters():
            p.grad = None
        logits = m(y, c)
        rg.cls_transforms.cross_entropy(logits, tgt, grad_dtype=torch.float16).backward()
        torch.cuda.synchronize()
        runs.append((logits.detach().clone(), {n: p.grad.detach().clone() for n, p in m.named_parameters()}))
    for k in (1, 2):
        assert torch.equal(runs[0][0], runs[k][0])
        bad = [n for n in runs[0][1] if not torch.equal(runs[0][1][n], runs[k][1][n])]
        assert not bad, bad[:5]


def test_fp16_graph_replay_equals_the_eager_pass():
    """forward + backward in fp16 captured into a HIP graph after one eager pass: every replay gives the eager pass's bits."""
    B = 8
    ws = torch.cuda.Stream()
    with torch.cuda.stream(ws):
        m, img, depths, heads, _ = _model("swt", DEV)
        nb = img // 8
        y = torch.from_numpy(detfill.normalish((B, 1, nb, nb, 8, 8), 391)).to(DEV).half()
        c = torch.from_numpy(detfill.normalish((B, 2, nb // 2, nb // 2, 8, 8), 392)).to(DEV).half()
        tgt = detfill.uniform((B, 1000), 393, 0.0, 1.0)
        tgt = torch.from_numpy(tgt / tgt.sum(1, keepdims=True)).to(DEV)
        m.eval()
        m.compute_dtype = torch.float16
        m.group_dw_backward = True              # bf16 only: fp16 must take the per-Linear path inside the capture too
        out = {}

        def part():
            logits = m(y, c)
            rg.cls_transforms.cross_entropy(logits, tgt, grad_dtype=torch.float16).backward()
            out["logits"] = logits

        m.zero_grad(set_to_none=True)
        part()
        torch.cuda.synchronize()
        ref_logits = out["logits"].detach().clone()
        ref = {n: p.grad.clone() for n, p in m.named_parameters()}
        m.zero_grad(set_to_none=True)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=ws):
            part()
        for r in range(3):
            g.replay()
            torch.cuda.synchronize()
            assert torch.equal(out["logits"], ref_logits), r
            bad = [n for n, p in m.named_parameters() if not torch.equal(ref[n], p.grad)]
            assert not bad, (r, bad[:5])
        del g
