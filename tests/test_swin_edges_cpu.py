"""CPU checks of the window-attention test machinery of tests/test_swin_edges.py (tests/swin_ref.py):
- the fp64 reference (torch.roll / reshape partition, oracle shift mask) equals oracle/swin_torch.window_attention in fp64, the
  outputs and the gradients autograd takes through the oracle, and its lse / d(scale) partial layouts are the oracle's;
- the Python copy of head_grid() reproduces rgbnm_window_attention_bwd_workspace at 256 CUs for every case of the GPU list, and
  that list reaches every launch class at 256 CUs;
- the element-wise bound accepts the reference rounded to T and rejects defects that the norm-wise bars of tests/test_swin.py
  let through.
"""
import math

import pytest
import torch
import torch.nn.functional as F

import kernel_check as KC
import swin_ref as R
import test_swin_edges as E
from kernel_check import U, check_bound
from oracle import swin_torch as ST
from rgb_no_more_amd import lib as L

F64, BF16 = torch.float64, torch.bfloat16
EINVAL = -1


class _Torch:
    """oracle/swin_torch's `torch`, with softmax keeping its input (the logits) for autograd to fill in."""

    def __init__(self, caught):
        self.caught = caught

    def __getattr__(self, name):
        return getattr(torch, name)

    def softmax(self, a, dim):
        a.retain_grad()
        self.caught["att"] = a
        return torch.softmax(a, dim)


class _F:
    """oracle/swin_torch's `F`, with the qkv Linear's output kept (its gradient is dqkv in window layout)."""

    def __init__(self, caught, n_qkv):
        self.caught, self.n_qkv = caught, n_qkv

    def __getattr__(self, name):
        return getattr(F, name)

    def linear(self, x, w, b=None):
        y = F.linear(x, w, b)
        if w.shape[0] == self.n_qkv and "qkv" not in self.caught:
            y.retain_grad()
            self.caught["qkv"] = y
        return y


@pytest.mark.parametrize("res,shift", [(16, 0), (16, 4), (24, 0), (24, 4), (24, 2), (16, 2)])
def test_fp64_reference_is_the_oracle(monkeypatch, res, shift):
    B, heads = 2, 3
    C = heads * 32
    g = torch.Generator().manual_seed(res + shift)
    pre = "a."
    ls = torch.log(torch.tensor([0.5, 5.0, 30.0], dtype=F64)).view(heads, 1, 1).requires_grad_(True)
    p = {pre + "qkv.weight": torch.randn(3 * C, C, generator=g, dtype=F64) * 0.3,
         pre + "q_bias": torch.randn(C, generator=g, dtype=F64) * 0.1, pre + "v_bias": torch.randn(C, generator=g, dtype=F64) * 0.1,
         pre + "logit_scale": ls,
         pre + "cpb_mlp.0.weight": torch.randn(512, 2, generator=g),            # fp32: the oracle's coords_table is fp32
         pre + "cpb_mlp.0.bias": torch.randn(512, generator=g) * 0.5,
         pre + "cpb_mlp.2.weight": torch.randn(heads, 512, generator=g) * 0.1,
         pre + "proj.weight": torch.eye(C, dtype=F64), pre + "proj.bias": torch.zeros(C, dtype=F64)}
    x = torch.randn(B, res * res, C, generator=g, dtype=F64) * 10.0 ** (torch.rand(B, res * res, 1, generator=g, dtype=F64) * 2 - 1)
    x.requires_grad_(True)
    caught = {}
    pb = ST.position_bias(p, pre, 8, heads).detach().double().requires_grad_(True)
    monkeypatch.setattr(ST, "position_bias", lambda *a: pb)
    monkeypatch.setattr(ST, "F", _F(caught, 3 * C))
    monkeypatch.setattr(ST, "torch", _Torch(caught))
    o = ST.window_attention(p, pre, x, res, 8, shift, heads)
    w = torch.randn(o.shape, generator=g, dtype=F64)
    (o * w).sum().backward()
    monkeypatch.undo()
    # the reference, token-major qkv of the oracle's own Linear (per token: it commutes with the roll)
    bias_cat = torch.cat([p[pre + "q_bias"], torch.zeros(C, dtype=F64), p[pre + "v_bias"]])
    qkv = F.linear(x.detach().reshape(-1, C), p[pre + "qkv.weight"], bias_cat)
    xw = R.partition(qkv, B, res, shift)
    assert torch.allclose(xw, caught["qkv"].detach(), rtol=0, atol=1e-12)
    q, k, v = (R.split_heads(xw[..., i * C:(i + 1) * C], heads) for i in range(3))
    scale = torch.exp(ls.detach().clamp(max=math.log(100.0))).view(-1)
    nwin = B * (res // 8) ** 2
    Lg, out, lse, P, _, _ = R.win_fwd(q, k, v, pb.detach(), scale, R.window_mask(res, shift, B, "cpu"), U, 0.0)
    merged = lambda t: t.permute(0, 2, 1, 3).reshape(nwin, 64, C)        # noqa: E731
    out_tok = R.reverse(merged(out), B, res, shift)
    assert (out_tok - o.detach().reshape(-1, C)).abs().max() < 1e-12
    att = caught["att"]
    # lse [(window heads + h) 64 + query] is the oracle's logsumexp of its logits, flattened
    assert (lse.reshape(-1) - torch.logsumexp(att.detach(), -1).reshape(-1)).abs().max() < 1e-12
    dO = R.split_heads(R.partition(w.reshape(-1, C), B, res, shift), heads)
    r = R.win_bwd(Lg, v, dO, out, lse, U, 0.0)
    dqkv = torch.cat([merged(r[nm]) for nm in ("dq", "dk", "dv")], -1)
    gq = caught["qkv"].grad
    assert (dqkv - gq).abs().max() <= 1e-10 * gq.abs().max()
    assert (r["dS"].sum(0) - pb.grad).abs().max() <= 1e-10 * pb.grad.abs().max()
    # d(logit_scale) = d(scale) exp(logit_scale) inside the clamp
    dscale = r["dsp"].sum(0)
    assert (dscale * scale - ls.grad.view(-1)).abs().max() <= 1e-10 * ls.grad.abs().max()
    # d(scale) partial per (window, head) = sum over the window's logits of dS cos, cos taken from the oracle's logits
    m = R.window_mask(res, shift, B, "cpu")
    cos = (att.detach() - pb.detach()[None] - (m[:, None] if m is not None else 0)) / scale.view(1, -1, 1, 1)
    per_window = (att.grad * cos).sum((-1, -2))
    assert per_window.shape == (nwin, heads)
    assert (r["dsp"] - per_window).abs().max() <= 1e-10 * per_window.abs().max()


def test_head_grid_copy_reproduces_the_workspace_entry():
    """At 256 CUs (what the library assumes without a device) the Python head_grid() gives rgbnm_window_attention_bwd_workspace
    for every case of the GPU list and more, and the GPU list reaches every launch class with every dtype."""
    cases = [c[:3] for c in E.win_cases(256)] + [(256, 64, 3), (1, 8, 1), (64, 64, 3), (7, 24, 24), (64, 8, 24), (256, 32, 6),
                                                 (256, 16, 12), (256, 8, 24), (5, 32, 1)]
    for B, res, heads in cases:
        assert L.lib().rgbnm_window_attention_bwd_workspace(B, res, heads) == R.bwd_workspace(B, res, heads, 256), (B, res, heads)
    for esz, want in ((4, set("abcde")), (2, set("abcd"))):
        seen = set()
        for B, res, heads, _, xcd in E.win_cases(256):
            for d in ("fwd", "bwd"):
                seen |= R.classes(esz, d, R.geometry(esz, d, B, res, heads, 256, xcd))
        assert want <= seen, (esz, sorted(want - seen))
    g = R.geometry(2, "fwd", 256, 64, 3, 256)
    assert g["gpx"] > 0 and g["wpw_max"] >= 24          # the bench's stage 1: about 24 windows per forward wave


def test_shift_argument_is_checked():
    """The entries take 0 <= shift < 8 (include/rgbnm.h); anything else is RGBNM_EINVAL before a launch."""
    lib = L.lib()
    for shift in (-1, 8):
        assert lib.rgbnm_window_attention_fwd(1, 16, 16, 16, 16, 16, 1, 8, 32, 1, shift, None) == EINVAL
        assert lib.rgbnm_window_attention_bwd(1, 16, 16, 16, 16, None, 16, 16, 16, 16, 16, 1, 8, 32, 1, shift, 16, 1 << 30,
                                              None) == EINVAL


def _case(B, res, heads, scales, seed, v_positive=False, tile=False):
    """bf16 inputs (as the GPU test draws them) and the fp64 forward + backward of tests/swin_ref.py."""
    C = heads * 32
    g = torch.Generator().manual_seed(seed)
    nwin = B * (res // 8) ** 2
    n = 64 if tile else B * res * res
    x = torch.randn(n, 3, heads, 32, generator=g)
    x[:, :2] *= 10.0 ** (torch.rand(n, 2, heads, 1, generator=g) * 4 - 2)
    if v_positive:
        x[:, 2] = x[:, 2].abs() + 0.5
    dout = torch.randn(n, C, generator=g)
    if tile:                                          # every window the same tokens: d(bias) grows with the window count
        x = R.reverse(x.reshape(1, 64, 3 * C).expand(nwin, 64, 3 * C), B, res, 0).reshape(-1, 3, heads, 32)
        dout = R.reverse(dout.reshape(1, 64, C).expand(nwin, 64, C), B, res, 0)
    qkv = x.reshape(-1, 3 * C).to(BF16)
    bias = torch.rand(heads, 64, 64, generator=g) * 16
    scale = torch.tensor(scales, dtype=torch.float32)
    xw = R.partition(qkv.double(), B, res, 0)
    q, k, v = (R.split_heads(xw[..., i * C:(i + 1) * C], heads) for i in range(3))
    uT, eta = KC.U_OF[BF16], E.ETA[BF16]
    Lg, out, lse, P, E_out, _ = R.win_fwd(q, k, v, bias.double(), scale.double(), None, uT, uT, eta)
    O_k = out.to(BF16).double()
    lse_k = lse.float().double()
    dO = R.split_heads(R.partition(dout.to(BF16).double(), B, res, 0), heads)
    r = R.win_bwd(Lg, v, dO, O_k, lse_k, uT, uT, eta)
    return {"out": out, "E_out": E_out, "O_k": O_k, "r": r, "nq": Lg["nq"], "nwin": nwin}


def test_bound_accepts_rounded_reference_and_rejects_defects():
    """The bf16 bounds of tests/test_swin_edges.py accept the reference rounded to bf16 (out, dq) / fp32 (d(bias)) and reject:
    one (window, head) with out x 1.01; one wave's d(bias) slice missing; one token's dq without the 1 / |q| of F.normalize's
    backward -- each of which stays inside the norm-wise bars of test_swin.py (max |d out| < 6e-2, Frobenius 3e-2)."""
    c = E.WIN_C[BF16]
    # out: a head whose logit error sits below the rounding of P (s = 0.1), positive values (P|v| = |out|)
    a = _case(1, 16, 2, [0.1, 5.0], 11, v_positive=True)
    O_k, ref = a["O_k"], a["out"]
    check_bound(O_k, ref, a["E_out"], BF16, 1, c["out"], "out rounded to bf16")
    bad = O_k.clone()
    bad[2, 0] *= 1.01
    assert (bad - ref).abs().max() < 6e-2
    with pytest.raises(AssertionError, match=r"\(2, 0, "):
        check_bound(bad.to(BF16), ref, a["E_out"], BF16, 1, c["out"], "out x 1.01 in window 2, head 0")
    # dq: one token (|q| away from 1) with the chain through |q| dropped
    r = a["r"]
    dq = r["dq"]
    check_bound(dq.to(BF16), dq, r["E_dq"], BF16, 1, c["dq"], "dq rounded to bf16")
    nq = a["nq"][..., 0]
    w, h, t = (int(i) for i in ((nq - 0.5).abs() < 0.2).nonzero()[0])
    bad = dq.clone()
    bad[w, h, t] *= nq[w, h, t]
    dqkv = torch.cat([r["dq"], r["dk"], r["dv"]], -1)
    bad_all = torch.cat([bad, r["dk"], r["dv"]], -1)
    assert float((bad_all - dqkv).norm() / dqkv.norm()) < 3e-2
    with pytest.raises(AssertionError, match=rf"\({w}, {h}, {t}, "):
        check_bound(bad.to(BF16), dq, r["E_dq"], BF16, 1, c["dq"], f"dq of (window {w}, head {h}, token {t}) without 1 / |q|")
    # d(bias): 64 identical windows at res 64, one window per wave; the slice of wave 5 missing
    b = _case(1, 64, 1, [0.5], 12, tile=True)
    r = b["r"]
    geo = R.geometry(2, "bwd", 1, 64, 1, 256)
    assert geo["capped"] and geo["wpw_max"] == 1
    S = geo["slots"] * geo["waves"]
    ref = r["dS"].sum(0)
    Eb = r["E_dS"].sum(0) + (geo["wpw_max"] + S) * U * r["absdS"].sum(0)
    check_bound(ref.float(), ref, Eb, torch.float32, 1, c["dbias"], "dbias rounded to fp32")
    lo, hi = b["nwin"] * 5 // geo["wph"], b["nwin"] * 6 // geo["wph"]
    bad = ref - r["dS"][lo:hi].sum(0)
    assert float((bad - ref).norm() / ref.norm()) < 3e-2
    with pytest.raises(AssertionError, match="out of bound"):
        check_bound(bad.float(), ref, Eb, torch.float32, 1, c["dbias"], "dbias without the slice of wave 5")
