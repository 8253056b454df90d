"""The models in fp16 with the library option f16_tuned = 2: besides the tuned plain GEMMs of level 1, attention v2, the fused MLP and
the LayerNorm-chained row-panel epilogues run in their fp16 instantiations (the whole per-block tuned path; the one-launch encoder
stays bf16 only).  Accuracy is held against the fp32 mode with the bars of tests/test_fp16_tuned_model.py / tests/test_fp16_model.py
(fp16 at a quarter of bf16's error or better, bf16 measured on the same per-block kernel set); the fused MLP must give the bits of
the two-GEMM path; a captured forward + backward replays the eager bits; three training steps under DeviceLossScaler; SwinV2, which
has none of the three families, is bit-identical at level 1 and level 2.

Measured on one MI355X (pytest -s prints the figures; DESIGN.md section 7 repeats them): max |dlogit| against the fp32 mode 4.2e-4
(E = 192, depth 2) / 3.7e-4 (E = 384, depth 1) for fp16 at level 2 against 3.0e-3 / 3.2e-3 for bf16 (x0.14 / x0.11); worst gradient
ratio x0.16 (qkv of block 0: 5.4e-4 against 3.4e-3); three scaled steps: losses 6.9223, 6.9147, 6.9104, scale 65536, nothing skipped.

The fused MLP equals the two-GEMM path bit for bit since the fp16 kernel pins Q before Phi = 1 - Q (mlp_fused.hip gelu_pair_pinned);
with common.h gelu_pair_fast, whose 1 - Q the compiler contracts into an fma in the fused kernel only, gelu(u) of block 0 differed by
one fp16 ulp in 115 of 9 633 792 elements (gelu'(u) in none) and logits by up to 1.3e-4.
"""
import numpy as np
import pytest
import torch

import kernel_check as KC
import rgb_no_more_amd as rg
from rgb_no_more_amd import lib as L
from rgb_no_more_amd.custom_optims import DeviceLossScaler
from test_fp16_model import build, step as vit_step
from test_fp16_tuned_kernels import is_f16
from test_fp16_tuned_model import f16_kernels
from test_loss_scale_train_loop import loop_step, make_opt, weights
from test_swin import _model, _load
from test_swin_fp16_model import step as swin_step
from test_hip_kernels import option  # noqa: F401  (fixture: set a runtime switch for one test)

pytestmark = pytest.mark.gpu
DEV = "cuda"
F16 = torch.float16
FUSED = ("mlp_fwd_kernel", "mlp_bwd_kernel")
ATTN1 = ("attn_fwd_kernel", "attn_bwd_dq_kernel", "attn_bwd_dkv_kernel")


@pytest.fixture
def per_block(option):
    """The per-block kernels in every mode: the one-launch encoder (bf16 only) is off, so that bf16 runs the kernel set fp16 runs."""
    option("fwd_chain", 0)
    option("bwd_chain", 0)


@pytest.mark.parametrize("tag,emb,heads,depth", [("ti_d2", 192, 3, 2), ("s_d1", 384, 6, 1)])
def test_vit_fp16_fused_logits_and_gradients_vs_fp32_and_bf16(option, per_block, tag, emb, heads, depth):
    B = 64                                                   # 12544 rows
    m, sd, y, c, tgt = build(emb, heads, depth, B, 1)
    l32, _, g32 = vit_step(m, y, c, tgt, torch.float32)
    option("f16_tuned", 2)
    (l16, loss16, g16), names = KC.launched(lambda: vit_step(m, y, c, tgt, F16))
    assert m._cur_dtype == F16
    option("f16_tuned", 0)
    (lbf, _, gbf), names_bf = KC.launched(lambda: vit_step(m, y, c, tgt, torch.bfloat16))
    e16, ebf = np.abs(l16 - l32).max(), np.abs(lbf - l32).max()
    print(f"[{tag} B={B} f16_tuned=2] max |dlogit| vs the fp32 mode: fp16 {e16:.3e} bf16 {ebf:.3e} (ratio {e16 / ebf:.3f})")
    assert np.isfinite(loss16)
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
    # the fp16 step ran the three families in their fp16 instantiations and no generic attention; bf16 ran the same kernels
    kinds = sorted({n.split("(")[0][-70:] for n in names})
    # (attn_persist, on by default: the persistent backward always, the persistent forward from 256 (image, head) pairs)
    for k in ("attn3_fwd_kernel" if B * heads >= 256 else "attn2_fwd_kernel", "attn3_bwd_kernel"):
        hits = [n for n in names if k in n]
        assert hits and all(is_f16(n) for n in hits), (k, kinds)
    assert not any(any(k in n for k in ATTN1) for n in names), kinds
    assert f16_kernels(names, "gemm_nt_kpipe", "gemm_nt_wres_kernel"), kinds
    if emb == 192:
        for k in FUSED:
            hits = [n for n in names if k in n]
            assert hits and all(is_f16(n) for n in hits), (k, kinds)
            assert any(k in n for n in names_bf), k
    else:
        assert not any(any(k in n for k in FUSED) for n in names), kinds
    assert not any("vit_chain" in n for n in names + names_bf), kinds


def test_fused_mlp_equals_the_two_gemm_path_in_fp16(option, per_block):
    """tests/test_fastpath_model.py test_fused_mlp_forward_equals_the_two_gemm_path for fp16 at level 2: mlp_fuse 1 and 0 give
    bit-identical saved activations, residual stream, chained LayerNorm output, statistics, logits and gradients; mlp_dmast flipped
    gives the same bits three times."""
    option("f16_tuned", 2)
    m, sd, y, c, tgt = build(192, 3, 2, 64, 1)
    m.compute_dtype = F16
    m.train()

    def snapshot():
        m.zero_grad()
        logits = m(y, c)
        ar = logits.grad_fn.st.arena
        torch.cuda.synchronize()
        snap = {"gl0": ar.blk[0]["gl"].clone(), "gp0": ar.blk[0]["u"].clone(), "x1": ar.x[1].clone(),
                "xn1_1": ar.blk[1]["xn1"].clone(), "mean1_1": ar.blk[1]["mean1"].clone(), "rstd1_1": ar.blk[1]["rstd1"].clone(),
                "gl1": ar.blk[1]["gl"].clone(), "x2": ar.x[2].clone(), "logits": logits.detach().clone()}
        (rg.cls_transforms.cross_entropy(logits, tgt, grad_dtype=F16) * 65536.0).backward()
        snap["grads"] = torch.cat([p.grad.reshape(-1) for p in m.parameters()]).clone()
        return snap

    (fused, names) = KC.launched(snapshot)
    assert f16_kernels(names, "mlp_fwd_kernel") and f16_kernels(names, "mlp_bwd_kernel"), sorted(set(names))
    assert fused["x1"].dtype == F16 and bool(torch.isfinite(fused["grads"]).all())
    option("mlp_fuse", 0)
    plain, names = KC.launched(snapshot)
    assert not any("mlp_fwd_kernel" in n for n in names), sorted(set(names))
    option("mlp_fuse", 1)
    for k in fused:
        a, b = fused[k].float(), plain[k].float()
        nd = int((a != b).sum())
        print(f"{k:8s} max |d| {float((a - b).abs().max()):.3e}  differing elements {nd} / {a.numel()}")
    for k in fused:
        assert torch.equal(fused[k], plain[k]), k
    option("mlp_dmast", 1 - L.get_option("mlp_dmast"))
    for rep in range(3):
        other = snapshot()
        for k in other:
            assert torch.equal(other[k], plain[k]), (k, rep)


def test_captured_forward_backward_replays_the_eager_bits(option):
    """fp16, level 2, fwd_chain / bwd_chain left at their defaults (the one-launch encoder does not apply to fp16): forward +
    backward captured into a HIP graph after one eager pass; three replays give the eager pass's logits and gradients."""
    option("f16_tuned", 2)
    ws = torch.cuda.Stream()
    with torch.cuda.stream(ws):
        m, sd, y, c, tgt = build(192, 3, 2, 64, 1)
        m.train()
        m.compute_dtype = F16
        out = {}

        def part():
            logits = m(y, c)
            (rg.cls_transforms.cross_entropy(logits, tgt, grad_dtype=F16) * 65536.0).backward()
            out["logits"] = logits

        m.zero_grad(set_to_none=True)
        _, names = KC.launched(part)
        torch.cuda.synchronize()
        assert f16_kernels(names, "mlp_fwd_kernel") and f16_kernels(names, "attn3_bwd_kernel", "attn2_bwd_kernel"), sorted(set(names))
        ref_logits = out["logits"].detach().clone()
        ref = {n: p.grad.clone() for n, p in m.named_parameters()}
        assert all(bool(torch.isfinite(v).all()) for v in ref.values())
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


def test_three_training_steps_under_the_device_loss_scaler(option):
    """tests/test_loss_scale_train_loop.py's step at the smallest batch that reaches 8192 rows (B = 42), fp16 at level 2: no step
    skipped at scale 65536, finite losses; at 2^40 step 1 overflows and is skipped."""
    option("f16_tuned", 2)
    m, sd, y, c, tgt = build(192, 3, 2, 42, 1)
    m.train()
    opt, scaler = make_opt(m), DeviceLossScaler()
    (losses, names) = KC.launched(lambda: [loop_step(m, opt, scaler, y, c, tgt, i, F16).item() for i in range(3)])
    assert m._cur_dtype == F16
    assert f16_kernels(names, "mlp_fwd_kernel") and f16_kernels(names, "mlp_bwd_kernel"), sorted(set(names))
    print(f"fp16 level 2, device scaler: losses {losses}; scale {scaler.get_scale()} norm {float(opt.last_norm):.4f}")
    assert all(np.isfinite(v) for v in losses)
    assert scaler.get_scale() == 65536.0 and scaler.skipped_steps() == 0
    assert float(opt.state_dict()["state"][0]["step"]) == 3.0
    m2, _, _, _, _ = build(192, 3, 2, 42, 1)
    m2.train()
    opt2, big = make_opt(m2), DeviceLossScaler(init_scale=2.0 ** 40)
    before = weights(m2)
    loop_step(m2, opt2, big, y, c, tgt, 0, F16)
    assert big.skipped_steps() == 1
    for k, v in m2.state_dict().items():
        assert torch.equal(v, before[k]), k


def test_swinv2_is_bit_identical_at_level_1_and_level_2(golden, option):
    g = golden("g15_swin.npz")
    m, *_ = _model("sw3", DEV)
    names, y, c, tgt = _load(m, "sw3", g)
    res = {}
    for level in (1, 2):
        option("f16_tuned", level)
        res[level] = swin_step(m, y, c, tgt, F16)
    assert np.array_equal(res[1][0], res[2][0])
    assert res[1][1] == res[2][1]
    for n in res[1][2]:
        assert torch.equal(res[1][2][n], res[2][2][n]), n
