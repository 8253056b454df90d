"""The ViT in fp16 compute mode (autocast(float16) or compute_dtype = torch.float16), forward and backward, against the fp32
oracle.  The bars calibrate themselves: the same test measures the bf16 mode's error on the same weights and inputs, and fp16
(3 more mantissa bits: 8x finer rounding) must come in at a quarter of it or better.  At the bench configuration every logit
must meet the north-star bar of 1e-3 that bf16 misses."""
import warnings

import numpy as np
import pytest
import torch

import rgb_no_more_amd as rg
from rgb_no_more_amd import detfill
from oracle import vit_torch as V

pytestmark = pytest.mark.gpu
DEV = "cuda"

# tag: emb, heads, depth, B, ver
CASES = {"ti_d2": (192, 3, 2, 8, 1), "ti_d12": (192, 3, 12, 8, 1), "s_d2": (384, 6, 2, 8, 1),
         "ti_d2_v2": (192, 3, 2, 2, 2), "ti_d2_v3": (192, 3, 2, 2, 3)}
GOLDEN_V = {2: ("g14_model_v2.npz", "ti_d2_v2"), 3: ("g18_model_v3.npz", "ti_d2_v3")}


def build(emb, heads, depth, B, ver):
    m = rg.ViT(3, 16, emb, depth=depth, n_classes=1000, drop_p=0.0, device=DEV, num_heads=heads, head_size=64,
               pixel_space="DCT", ver=ver, use_subblock=True)
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    sd = detfill.fill_state_dict(shapes, base_seed=1)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    y = torch.from_numpy(detfill.normalish((B, 1, 28, 28, 8, 8), 71)).to(DEV)
    c = torch.from_numpy(detfill.normalish((B, 2, 14, 14, 8, 8), 72)).to(DEV)
    t = detfill.uniform((B, 1000), 73, 0.0, 1.0)
    tgt = torch.from_numpy(t / t.sum(1, keepdims=True)).to(DEV)
    return m, sd, y, c, tgt


LOSS_SCALE = 2.0 ** 16      # train.py's GradScaler starts here: without a scale, fp16 activation gradients underflow


def step(m, y, c, tgt, dt):
    """forward under autocast(dt) (fp32: no autocast), the package's loss with a gradient in dt, backward of the loss scaled by
    LOSS_SCALE (a power of two: the same for every dtype; GradScaler's job in training), gradients unscaled."""
    m.train()
    m.zero_grad(set_to_none=True)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        with torch.autocast("cuda", dtype=dt, enabled=dt != torch.float32):
            logits = m(y, c)
    if dt == torch.float16:                                 # fp16 is no longer announced (and run) as bf16
        assert not [w for w in caught if "rgb-no-more_amd" in str(w.message)], [str(w.message) for w in caught]
    loss = rg.cls_transforms.cross_entropy(logits, tgt, grad_dtype=dt)
    (loss * LOSS_SCALE).backward()
    torch.cuda.synchronize()
    grads = {n: p.grad.detach().double().cpu() / LOSS_SCALE for n, p in m.named_parameters()}
    return logits.detach().float().cpu().numpy(), loss.item(), grads


@pytest.mark.parametrize("tag", list(CASES))
def test_fp16_logits_and_gradients_vs_oracle_and_bf16(golden, tag):
    emb, heads, depth, B, ver = CASES[tag]
    m, sd, y, c, tgt = build(emb, heads, depth, B, ver)
    if ver == 1:
        p = {k: torch.from_numpy(v) for k, v in sd.items()}
        ref = V.vit_forward(p, y.cpu(), c.cpu(), depth, heads, emb).numpy()
    else:
        fname, key = GOLDEN_V[ver]
        ref = golden(fname)[key + "_logits"]
    l32, _, g32 = step(m, y, c, tgt, torch.float32)         # gradients: the fp32 mode (tests/test_vit_model.py: rtol 1e-3)
    assert np.abs(l32 - ref).max() < 1e-4
    l16, loss16, g16 = step(m, y, c, tgt, torch.float16)
    assert m._cur_dtype == torch.float16
    lbf, _, gbf = step(m, y, c, tgt, torch.bfloat16)
    e16, ebf = np.abs(l16 - ref).max(), np.abs(lbf - ref).max()
    print(f"[{tag}] max |dlogit| fp16 {e16:.3e} bf16 {ebf:.3e} (ratio {e16 / ebf:.3f})")
    assert np.isfinite(loss16)
    assert e16 <= 1e-3
    assert e16 <= ebf / 4
    worst = []
    for n in g32:
        r16 = ((g16[n] - g32[n]).norm() / (g32[n].norm() + 1e-30)).item()
        rbf = ((gbf[n] - g32[n]).norm() / (g32[n].norm() + 1e-30)).item()
        worst.append((r16 / max(rbf, 1e-12), n, r16, rbf))
    worst.sort(reverse=True)
    print(f"[{tag}] worst gradient ratios fp16 / bf16: " + ", ".join(f"{n} {a:.2e}/{b:.2e}" for _, n, a, b in worst[:3]))
    for _, n, r16, rbf in worst:
        assert r16 <= rbf / 4 + 1e-6, (n, r16, rbf)


def test_compute_dtype_float16_without_autocast():
    m, sd, y, c, tgt = build(192, 3, 2, 4, 1)
    m.compute_dtype = torch.float16
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        logits = m(y, c)
    assert not [w for w in caught if "rgb-no-more_amd" in str(w.message)]
    p = {k: torch.from_numpy(v) for k, v in sd.items()}
    ref = V.vit_forward(p, y.cpu(), c.cpu(), 2, 3, 192).numpy()
    assert logits.dtype == torch.float32
    assert np.abs(logits.detach().cpu().numpy() - ref).max() <= 1e-3
    # the head hands out an fp16 gradient edge for the package's loss
    assert getattr(logits, "_rgbnm_grad_edge").dtype == torch.float16


def test_every_logit_at_the_bench_configuration(golden):
    """g20: all 256 x 1000 logits of the reference, JPEG-Ti depth 12, B = 256 -- the north-star bar 1e-3, and no worse than
    twice torch's own fp16 autocast of the oracle (run on the CPU) plus 2e-4."""
    g = golden("g20_fullsize.npz")
    m, sd, y, c, tgt = build(192, 3, 12, 256, 1)
    m.train()
    with torch.autocast("cuda", dtype=torch.float16):
        logits = m(y, c)
    rg.cls_transforms.cross_entropy(logits, tgt, grad_dtype=torch.float16).backward()
    torch.cuda.synchronize()
    got = logits.detach().cpu().numpy()
    ref = g["ti_d12_b256_logits"]
    assert got.shape == ref.shape == (256, 1000)
    err = np.abs(got - ref).max()
    p = {k: torch.from_numpy(v) for k, v in sd.items()}
    with torch.no_grad(), torch.autocast("cpu", dtype=torch.float16):
        tref = V.vit_forward(p, y.cpu(), c.cpu(), 12, 3, 192)
    terr = np.abs(tref.float().numpy() - ref).max()
    print(f"B=256 fp16: max |dlogit| {err:.3e} (mean {np.abs(got - ref).mean():.3e}); torch CPU fp16 autocast {terr:.3e}")
    assert err <= 1e-3
    assert err <= 2 * terr + 2e-4
    assert all(torch.isfinite(p.grad).all() for p in m.parameters())
