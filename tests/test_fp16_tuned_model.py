"""The models in fp16 with the library option f16_tuned = 1: the GEMMs of the step run on the kernels tuned for 16-bit operands
(gemm_nt_small / _wres / _kpipe, gemm_tn_pipe, the grouped weight-gradient launches) and must keep the accuracy the fp16 mode has
on the generic kernels.  The bars are those of tests/test_fp16_model.py and tests/test_swin_fp16_model.py: the same test measures
the bf16 mode on the same weights and inputs, and fp16 must come in at a quarter of its error or better -- here against the fp32
mode of the same model (those files hold it to 1e-4 of the reference's logits), at batch sizes large enough for every tuned kernel:
12544 rows for the ViT (>= 8192: row panels, >= 4096: weight-resident, a multiple of 64: pipelined dW)."""
import numpy as np
import pytest
import torch

import kernel_check as KC
import rgb_no_more_amd as rg
from rgb_no_more_amd import detfill
from test_fp16_model import build, step as vit_step
from test_swin_fp16_model import _swt, step as swin_step
from test_swin import _model
from test_fp16_tuned_kernels import is_f16
from test_hip_kernels import option  # noqa: F401  (fixture: set a runtime switch for one test)

pytestmark = pytest.mark.gpu
DEV = "cuda"


def f16_kernels(names, *subs):
    return [n for n in names if any(s in n for s in subs) and is_f16(n)]


@pytest.mark.parametrize("tag,emb,heads,depth", [("ti_d2", 192, 3, 2), ("s_d1", 384, 6, 1)])
def test_vit_fp16_tuned_logits_and_gradients_vs_fp32_and_bf16(option, tag, emb, heads, depth):
    B = 64
    m, sd, y, c, tgt = build(emb, heads, depth, B, 1)
    l32, _, g32 = vit_step(m, y, c, tgt, torch.float32)
    option("f16_tuned", 1)
    (l16, loss16, g16), names = KC.launched(lambda: vit_step(m, y, c, tgt, torch.float16))
    assert m._cur_dtype == torch.float16
    option("f16_tuned", 0)
    lbf, _, gbf = vit_step(m, y, c, tgt, torch.bfloat16)
    e16, ebf = np.abs(l16 - l32).max(), np.abs(lbf - l32).max()
    print(f"[{tag} B={B} f16_tuned] max |dlogit| vs the fp32 mode: fp16 {e16:.3e} bf16 {ebf:.3e} (ratio {e16 / ebf:.3f})")
    assert np.isfinite(loss16)                       # (loss scale 2^16, test_fp16_model.LOSS_SCALE)
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
    # the step ran on the tuned kernels, in their fp16 instantiations
    kinds = sorted({n.split("(")[0][-70:] for n in names if "gemm_" in n})
    assert f16_kernels(names, "gemm_nt_kpipe", "gemm_nt_wres_kernel"), kinds
    assert f16_kernels(names, "gemm_tn_pipe_kernel", "gemm_tn_wide_kernel"), kinds
    assert f16_kernels(names, "gemm_nt_small_kernel"), kinds


def tn_launches(names):
    """The weight-gradient launches of a step in their fp16 instantiation (pipelined / wide: one launch per GEMM, or per group)."""
    return f16_kernels(names, "gemm_tn_pipe_kernel", "gemm_tn_wide_kernel")


def test_swin_fp16_tuned_logits_and_gradients_vs_fp32_and_bf16(golden, option):
    """fp16 with the option on, twice: per-Linear weight gradients (group_dw_backward off, the model's default) and the backward-wide
    bracket with held reductions (group_dw_backward = hold_reductions = True: grouped launches, those without a token split writing
    dW / db themselves).  Both against the fp32 mode with the bars of tests/test_swin_fp16_model.py; the grouped pass must need far
    fewer weight-gradient launches than the per-Linear one, and no generic gemm_tn launch more."""
    g = golden("g20_fullsize.npz")                   # (parameter names of the "swt" configuration; B = 8 has no stored logits)
    m, names, y, c, tgt = _swt(g, "swt_b64", 8)
    assert m.group_dw_backward is False
    out, kern = {}, {}
    for tag, dt, grouped in (("fp32", torch.float32, False), ("fp16", torch.float16, False), ("fp16-grouped", torch.float16, True),
                             ("bf16", torch.bfloat16, False)):
        m.group_dw_backward = grouped
        m.hold_reductions = True
        try:
            if dt == torch.float16:
                option("f16_tuned", 1)
                (logits, loss, grads), kern[tag] = KC.launched(lambda: swin_step(m, y, c, tgt, dt))
                option("f16_tuned", 0)
            else:
                logits, loss, grads = swin_step(m, y, c, tgt, dt)
        finally:
            m.group_dw_backward = False
        if dt == torch.float32:
            l32, g32 = logits, grads
        assert np.isfinite(loss) and all(torch.isfinite(v).all() for v in grads.values())
        rel = {n: ((grads[n] - g32[n]).norm() / (g32[n].norm() + 1e-30)).item() for n in names}
        out[tag] = (np.abs(logits - l32).max(), np.median(list(rel.values())), rel)
        print(f"[swt B=8 {tag}] vs the fp32 mode: max |dlogit| {out[tag][0]:.3e}, gradients median rel {out[tag][1]:.3e}, "
              f"max rel {max(rel.values()):.3e}")
    b = out["bf16"]
    for tag in ("fp16", "fp16-grouped"):
        h = out[tag]
        assert h[0] <= b[0] / 4, tag                 # logits
        assert h[1] <= b[1] / 4, tag                 # gradients (median over the parameter tensors, as in that file)
        kinds = sorted({n.split("(")[0][-70:] for n in kern[tag] if "gemm_" in n})
        assert f16_kernels(kern[tag], "gemm_nt_kpipe", "gemm_nt_wres_kernel"), kinds
        assert tn_launches(kern[tag]), kinds
    # every parameter tensor of the grouped pass, not only their median: no worse than twice the per-Linear pass's error plus a
    # tenth of bf16's (another summation order -- token splits and where they are added up -- is all that may differ)
    hu, hg = out["fp16"][2], out["fp16-grouped"][2]
    bad = [(n, hg[n], hu[n]) for n in names if hg[n] > 2 * hu[n] + 0.1 * b[2][n] + 1e-6]
    assert not bad, bad[:5]
    nu, ng = len(tn_launches(kern["fp16"])), len(tn_launches(kern["fp16-grouped"]))
    gu = sum("gemm_tn_kernel" in n for n in kern["fp16"])
    gg = sum("gemm_tn_kernel" in n for n in kern["fp16-grouped"])
    print(f"[swt B=8] fp16 weight-gradient launches: per-Linear {nu} (+ {gu} generic), grouped {ng} (+ {gg} generic)")
    assert 2 * ng <= nu, (ng, nu)
    assert gg <= gu, (gg, gu)


def test_swin_fp16_tuned_grouped_graph_replay_equals_the_eager_pass(option):
    """forward + backward in fp16 with f16_tuned and group_dw_backward, captured into a HIP graph after one eager pass: every replay
    gives the eager pass's bits, and the step that was captured holds grouped weight-gradient launches in their fp16 instantiation:
    at most half as many as the same function launches with the bracket off.  (The profiler lists no kernel of a graph replay here
    -- measured: an empty list -- so the launches are read off an eager run of the very function the graph captured, after the
    replays; the replays' gradients equal that function's bit for bit.  The grouped gradients' values are checked against the fp32
    mode in the test above.)"""
    option("f16_tuned", 1)
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
        m.group_dw_backward = True
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
        m.zero_grad(set_to_none=True)
        _, names = KC.launched(part)
        assert torch.equal(out["logits"], ref_logits)
        bad = [n for n, p in m.named_parameters() if not torch.equal(ref[n], p.grad)]
        assert not bad, bad[:5]
        # grouped: far fewer weight-gradient launches than the same function needs with the bracket off
        m.group_dw_backward = False
        m.zero_grad(set_to_none=True)
        _, single = KC.launched(part)
        ng, nu = len(tn_launches(names)), len(tn_launches(single))
        assert ng and 2 * ng <= nu, (ng, nu)
