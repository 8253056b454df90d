"""ViT training with dropout p > 0 (ViT.train_dropout = True) against a masked reference: oracle.vit_torch's patch embedding,
attention and class head composed with the three dropout sites of each block (plainvit.py:485-529), whose masks are rebuilt from
the forward's seed with tests/dropout_ref.py."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dropout_ref as D
import rgb_no_more_amd as rg
from rgb_no_more_amd import detfill
from oracle import vit_torch as V

pytestmark = pytest.mark.gpu
DEV = "cuda"
P = 0.1
LOSS_SCALE = 2.0 ** 16
CASES = {"ti": (192, 3), "s": (384, 6)}
DTS = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}


def build(emb, heads, B=16, depth=2, p=P):
    m = rg.ViT(3, 16, emb, depth=depth, n_classes=1000, drop_p=p, device=DEV, num_heads=heads, head_size=64,
               pixel_space="DCT", ver=1, use_subblock=True)
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    sd = detfill.fill_state_dict(shapes, base_seed=1)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    m.train_dropout = True
    y = torch.from_numpy(detfill.normalish((B, 1, 28, 28, 8, 8), 71)).to(DEV)
    c = torch.from_numpy(detfill.normalish((B, 2, 14, 14, 8, 8), 72)).to(DEV)
    t = detfill.uniform((B, 1000), 73, 0.0, 1.0)
    tgt = torch.from_numpy(t / t.sum(1, keepdims=True)).to(DEV)
    return m, sd, y, c, tgt


def seed_of(m):
    return int(m.last_dropout_seed.item()) & (2 ** 64 - 1)


def masked_forward(p, y, cbcr, depth, heads, emb, seed, pd):
    """The reference forward with nn.Dropout's three sites per block, masks from the contract."""
    x = V.patch_embed(p, y, cbcr)
    B, N, E = x.shape
    M = B * N
    f = lambda site, i, n: torch.from_numpy(D.factor(seed, pd, site, i, M, n)).to(x.dtype).view(B, N, n)  # noqa: E731
    for i in range(depth):
        a, b = f"encoder.{i}.0.fn.", f"encoder.{i}.1.fn."
        h = F.layer_norm(x, (emb,), p[a + "eb_lrnorm1.weight"], p[a + "eb_lrnorm1.bias"], 1e-5)
        x = x + V.attention(p, a + "eb_mha.", h, heads, emb) * f(0, i, E)
        h = F.layer_norm(x, (emb,), p[b + "eb_lrnorm2.weight"], p[b + "eb_lrnorm2.bias"], 1e-5)
        h = F.gelu(F.linear(h, p[b + "eb_ffb.0.weight"], p[b + "eb_ffb.0.bias"])) * f(1, i, 4 * E)
        x = x + F.linear(h, p[b + "eb_ffb.3.weight"], p[b + "eb_ffb.3.bias"]) * f(2, i, E)
    return V.class_head(p, x, emb)


def reference(sd, y, c, tgt, depth, heads, emb, seed, pd=P):
    """(logits, loss, grads) of the masked reference in fp64."""
    p = {k: torch.from_numpy(v).double().requires_grad_(True) for k, v in sd.items()}
    logits = masked_forward(p, y.cpu().double(), c.cpu().double(), depth, heads, emb, seed, pd)
    loss = V.soft_xent(logits, tgt.cpu().double())
    loss.backward()
    return logits.detach().numpy(), loss.item(), {k: v.grad for k, v in p.items()}


def fwd(m, y, c, dt):
    with torch.autocast("cuda", dtype=dt, enabled=dt != torch.float32):
        return m(y, c)


def bwd(m, logits, tgt, dt):
    loss = rg.cls_transforms.cross_entropy(logits, tgt, grad_dtype=dt)
    (loss * LOSS_SCALE).backward()
    torch.cuda.synchronize()
    return loss.item(), {n: q.grad.detach().double().cpu() / LOSS_SCALE for n, q in m.named_parameters()}


def grad_errors(g, gref):
    return {n: ((g[n] - gref[n]).norm() / (gref[n].norm() + 1e-30)).item() for n in gref}


# bars of tests/test_vit_model.py (fp32, bf16) and tests/test_fp16_model.py (fp16: logits 1e-3, gradients 4x finer than bf16)
BARS = {"f32": (1e-4, 1e-3), "bf16": (1e-2, 0.15), "f16": (1e-3, 0.15 / 4)}


@pytest.mark.parametrize("dtn", list(DTS))
@pytest.mark.parametrize("tag", list(CASES))
def test_logits_and_gradients_match_the_masked_reference(tag, dtn):
    emb, heads = CASES[tag]
    dt = DTS[dtn]
    m, sd, y, c, tgt = build(emb, heads)
    m.train()
    m.zero_grad(set_to_none=True)
    logits = fwd(m, y, c, dt)
    seed = seed_of(m)
    loss, g = bwd(m, logits, tgt, dt)
    lref, loss_ref, gref = reference(sd, y, c, tgt, 2, heads, emb, seed)
    err = np.abs(logits.detach().float().cpu().numpy() - lref).max()
    ge = grad_errors(g, gref)
    worst = max(ge, key=ge.get)
    print(f"[{tag} {dtn}] max |dlogit| {err:.3e}; loss {loss:.6f} ref {loss_ref:.6f}; worst grad rel {ge[worst]:.3e} ({worst}); "
          f"median {np.median(list(ge.values())):.3e}")
    lbar, gbar = BARS[dtn]
    assert err <= lbar
    assert ge[worst] <= gbar, (worst, ge[worst])
    if dtn != "f32":
        assert np.median(list(ge.values())) < (2e-2 if dtn == "bf16" else 5e-3)
    # the masks did bite: the unmasked oracle is several times further away than our error
    plain = V.vit_forward({k: torch.from_numpy(v) for k, v in sd.items()}, y.cpu(), c.cpu(), 2, heads, emb).numpy()
    assert np.abs(plain - lref).max() > max(4 * err, 1e-3)


@pytest.mark.parametrize("dtn", ["f32", "f16"])
def test_p0_and_a_threshold_of_zero_give_the_bits_of_the_default_path(dtn):
    """p = 0 with the switch on takes the default path; p = 2^-40 (threshold 0, scale 1: every element kept) runs the dropout
    kernels and must give the same bits (fp32 / fp16 run the same generic kernels on both paths)."""
    dt = DTS[dtn]
    res = []
    for p, on in ((0.0, False), (0.0, True), (2.0 ** -40, True)):
        m, sd, y, c, tgt = build(192, 3, B=4, p=p)
        m.train_dropout = on
        m.train()
        logits = fwd(m, y, c, dt)
        _, g = bwd(m, logits, tgt, dt)
        res.append((logits.detach().cpu(), g, m.last_dropout_seed))
    assert res[0][2] is None and res[1][2] is None and res[2][2] is not None
    for r in res[1:]:
        assert torch.equal(r[0], res[0][0])
        assert all(torch.equal(r[1][n], res[0][1][n]) for n in res[0][1])


def test_held_reductions_on_the_dropout_path():
    """defer_grad_reduction (held split-sum reductions, rgbnm.h rgbnm_reduce_hold_*) with the per-block dropout backward."""
    m, sd, y, c, tgt = build(192, 3)
    m.defer_grad_reduction = True
    m.train()
    m.zero_grad(set_to_none=True)
    logits = fwd(m, y, c, torch.bfloat16)
    seed = seed_of(m)
    _, g = bwd(m, logits, tgt, torch.bfloat16)
    _, _, gref = reference(sd, y, c, tgt, 2, 3, 192, seed)
    ge = grad_errors(g, gref)
    assert max(ge.values()) <= BARS["bf16"][1] and np.median(list(ge.values())) < 2e-2


def test_eval_is_the_identity_and_the_switch_off_refuses():
    m, sd, y, c, tgt = build(192, 3, B=2)
    m0, _, _, _, _ = build(192, 3, B=2, p=0.0)
    m.eval()
    m0.eval()
    with torch.no_grad():
        assert torch.equal(m(y, c), m0(y, c))
    assert m.last_dropout_seed is None
    m.train()
    m.train_dropout = False
    with pytest.raises(NotImplementedError, match="dropout"):
        m(y, c)


def test_manual_seed_reproduces_and_steps_differ():
    m, sd, y, c, tgt = build(192, 3, B=4)
    m.train()
    runs = []
    for s in (5, 5):
        torch.manual_seed(s)
        a = m(y, c).detach().clone()
        sa = seed_of(m)
        b = m(y, c).detach().clone()
        runs.append((a, sa, b, seed_of(m)))
    assert torch.equal(runs[0][0], runs[1][0]) and runs[0][1] == runs[1][1]
    assert torch.equal(runs[0][2], runs[1][2]) and runs[0][3] == runs[1][3]
    assert runs[0][1] != runs[0][3]
    assert not torch.equal(runs[0][0], runs[0][2])


def test_two_forwards_then_two_backwards_use_their_own_masks():
    m, sd, y, c, tgt = build(192, 3, B=4)
    m.train()
    m.zero_grad(set_to_none=True)
    la = m(y, c)
    sa = seed_of(m)
    lb = m(y, c)
    sb = seed_of(m)
    assert sa != sb
    _, ga = bwd(m, la, tgt, torch.float32)
    m.zero_grad(set_to_none=True)
    _, gb = bwd(m, lb, tgt, torch.float32)
    for logits, g, s in ((la, ga, sa), (lb, gb, sb)):
        lref, _, gref = reference(sd, y, c, tgt, 2, 3, 192, s)
        assert np.abs(logits.detach().cpu().numpy() - lref).max() <= 1e-4
        ge = grad_errors(g, gref)
        assert max(ge.values()) <= 1e-3, max(ge, key=ge.get)


def test_graph_replays_draw_fresh_seeds():
    B = 4
    ws = torch.cuda.Stream()
    ws.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(ws):
        m, sd, y, c, tgt = build(192, 3, B=B)
        m.train()
        out = {}

        def part():
            logits = m(y, c)
            rg.cls_transforms.cross_entropy(logits, tgt).backward()
            out["logits"] = logits
            out["seed"] = m.last_dropout_seed

        m.zero_grad(set_to_none=True)
        part()                                            # warm-up (arenas, shadows) outside the capture
        torch.cuda.synchronize()
        m.zero_grad(set_to_none=True)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=ws):
            part()
        seen = []
        for r in range(2):
            g.replay()
            torch.cuda.synchronize()
            s = int(out["seed"].item()) & (2 ** 64 - 1)
            seen.append(s)
            lref, _, gref = reference(sd, y, c, tgt, 2, 3, 192, s)
            assert np.abs(out["logits"].detach().cpu().numpy() - lref).max() <= 1e-4, r
            ge = grad_errors({n: q.grad.detach().double().cpu() for n, q in m.named_parameters()}, gref)
            assert max(ge.values()) <= 1e-3, (r, max(ge, key=ge.get))
        assert seen[0] != seen[1]
        del g
    torch.cuda.current_stream().wait_stream(ws)


def test_training_steps_track_the_masked_oracle_fp32():
    """3 optimizer steps (clip + AdamW + WeightDecay) with dropout: loss and weights follow the oracle fed each step's masks."""
    emb, heads, depth = 192, 3, 2
    m, sd, y, c, tgt = build(emb, heads, B=4)
    m.train()
    opt = rg.custom_optims.FusedClipAdamWWD(m, lr=3e-3, eps=1e-8, weight_decay=1e-4, max_norm=1.0)
    names = list(sd.keys())
    p = {k: torch.from_numpy(v.copy()).requires_grad_(True) for k, v in sd.items()}
    mm = [np.zeros_like(sd[k]) for k in names]
    vv = [np.zeros_like(sd[k]) for k in names]
    mask = [(".weight" in n) and ("lrnorm" not in n) for n in names]
    yc, cc, tc = y.cpu(), c.cpu(), tgt.cpu()
    for step in range(1, 4):
        opt.zero_grad()
        loss = rg.cls_transforms.cross_entropy(m(y, c), tgt)
        seed = seed_of(m)
        loss.backward()
        opt.step()
        for k in names:
            p[k].grad = None
        lo = V.soft_xent(masked_forward(p, yc, cc, depth, heads, emb, seed, P), tc)
        lo.backward()
        assert abs(loss.item() - lo.item()) < 2e-5, (step, loss.item(), lo.item())
        params = [p[k].detach().numpy() for k in names]
        grads = [p[k].grad.numpy() for k in names]
        tn = V.clip_adamw_wd_step(params, grads, mm, vv, step, 3e-3, 3e-3, 1e-4, mask)
        assert abs(opt.last_norm.item() - tn) < 1e-3 * max(1.0, tn)
    got = {k: v.detach().cpu().numpy() for k, v in m.state_dict().items()}
    worst = max(np.abs(got[k] - p[k].detach().numpy()).max() for k in names)
    print(f"max |w - w_oracle| after 3 steps = {worst:.3e}")
    assert worst < 2e-3
    med = np.median(np.concatenate([np.abs(got[k] - p[k].detach().numpy()).reshape(-1) for k in names]))
    assert med < 1e-6
