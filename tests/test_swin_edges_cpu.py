"""CPU checks of the window-attention test machinery of tests/test_swin_edges.py (tests/swin_ref.py):
- the fp64 reference (torch.roll / reshape partition, oracle shift mask) equals oracle/swin_torch.window_attention in fp64, the
  outputs and the gradients autograd takes through the oracle, and its lse / d(scale) partial layouts are the oracle's;
- the Python copy of head_grid() reproduces rgbnm_window_attention_bwd_workspace at 256 CUs for every case of the GPU list, and
  that list reaches every launch class at 256 CUs;
- the element-wise bound accepts the reference rounded to T and rejects defects that the norm-wise bars of tests/test_swin.py
  let through;
- the embedding's reference equals the oracle in fp64, its derived bound accepts an fp32 emulation in the kernel's order and
  rejects layout defects, and the case list reaches both tails a 4-block workgroup can have.
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


# ------------------------------------------------------------------------------------------------------------- embedding
def test_embed_reference_is_the_oracle_in_fp64():
    """swin_ref.embed_ref (one einops pattern) equals oracle/swin_torch.decompose_features in fp64, bit for bit, on every case."""
    Ay, Ac = R.embed_matrices()
    for i, (B, Hb, Wb) in enumerate(R.EMBED_CASES):
        y, c = (t.double() for t in R.embed_inputs(B, Hb, Wb, 50 + 2 * i))
        ref, mag = R.embed_ref(y, c, Ay, Ac)
        assert ref.shape == (B, 2 * Hb, 2 * Wb, 24)
        assert torch.equal(ref, ST.decompose_features(y, c)), (B, Hb, Wb)
        assert bool((mag >= ref.abs()).all())


def test_embed_cases_and_the_workgroup_tail():
    """A workgroup takes 4 blocks, luma first.  With Hb and Wb even -- odd ones are refused -- a call has 4m luma and 2m chroma
    blocks: the luma / chroma boundary always falls between workgroups and the last workgroup is either full or holds two
    blocks; remainders 1 and 3 cannot occur.  The cases reach both, with Hb < Wb, Hb > Wb and Hb = Wb, B = 1 and B > 1."""
    rem = set()
    for B, Hb, Wb in R.EMBED_CASES:
        ny, nc = R.embed_blocks(B, Hb, Wb)
        assert ny % R.EMBED_BLOCKS_PER_WG == 0 and nc * 2 == ny
        rem.add((ny + nc) % R.EMBED_BLOCKS_PER_WG)
    assert rem == {0, 2}
    assert all((6 * m) % 4 in (0, 2) for m in range(1, 100))
    assert {(Hb > Wb) - (Hb < Wb) for _, Hb, Wb in R.EMBED_CASES} == {-1, 0, 1}
    assert {B > 1 for B, _, _ in R.EMBED_CASES} == {False, True}
    assert R.EMBED_CASES == [(1, 2, 2), (1, 2, 6), (1, 6, 2), (3, 6, 10), (2, 4, 14)]


@pytest.mark.parametrize("ti", [torch.float32, torch.bfloat16, torch.float16])
def test_embed_bound_accepts_the_kernels_arithmetic_and_rejects_defects(ti):
    """An fp32 emulation in the kernel's order (fma and multiply + add) passes ulp_TO(ref) + EMBED_C u mag on the committed inputs
    for every output type; H for W in the token pitch, sub-block row and column exchanged, the sub-block-major split and a store two ulps off do not
    (the bound's one ulp_TO admits any rounding direction of the store: the bits of that rounding are pinned by
    tests/test_swin_fp16_kernels.py)."""
    assert 16 < R.EMBED_C < 16.00002
    Ay, Ac = (a.float() for a in R.embed_matrices())
    for i, (B, Hb, Wb) in enumerate(R.EMBED_CASES):
        y, c = (t.to(ti) for t in R.embed_inputs(B, Hb, Wb, 50 + 2 * i))
        ref, mag = R.embed_ref(y, c, Ay, Ac)
        for fma in (True, False):
            emu = R.embed_emulate(y.float(), c.float(), Ay, Ac, fma)
            for to in (torch.float32, torch.bfloat16, torch.float16):
                assert check_bound(emu.to(to), ref, mag, to, 1, R.EMBED_C * U, f"emulation fma={fma}", verbose=False) <= 1.0
        emu = R.embed_emulate(y.float(), c.float(), Ay, Ac)
        if Hb < Wb:                                          # token pitch 2 Hb instead of 2 Wb: rows overlap, the tail is never written
            flat = torch.full((B * 4 * Hb * Wb, 24), float("nan"))
            i, j = torch.meshgrid(torch.arange(B * 2 * Hb), torch.arange(2 * Wb), indexing="ij")
            flat[(i * 2 * Hb + j).reshape(-1)] = emu.reshape(-1, 24)
            with pytest.raises(AssertionError):
                check_bound(flat.reshape(ref.shape), ref, mag, torch.float32, 1, R.EMBED_C * U, "token pitch")
        swapped = emu.clone()                                # sub-block row and column exchanged in the token arithmetic
        swapped[..., :16] = emu[..., :16].reshape(B, Hb, 2, Wb, 2, 16).transpose(2, 4).reshape(B, 2 * Hb, 2 * Wb, 16)
        with pytest.raises(AssertionError):
            check_bound(swapped, ref, mag, torch.float32, 1, R.EMBED_C * U, "pdh / pdw exchanged")
        wrong = emu.clone()                                  # luma rows split '(pdh p1)' instead of '(p1 pdh)'
        ty = (Ay.double().T @ y.double() @ Ay.double()).float()
        wrong[..., :16] = ty.reshape(B, 1, Hb, Wb, 2, 4, 2, 4).permute(0, 2, 4, 3, 6, 1, 5, 7).reshape(B, 2 * Hb, 2 * Wb, 16)
        with pytest.raises(AssertionError):
            check_bound(wrong, ref, mag, torch.float32, 1, R.EMBED_C * U, "sub-block-major")
        off = (emu.double() + 2 * KC.ulp(ref, torch.bfloat16)).to(torch.bfloat16)             # two bf16 ulps off
        with pytest.raises(AssertionError):
            check_bound(off, ref, mag, torch.bfloat16, 1, R.EMBED_C * U, "two ulps")


def test_embed_refusals_return_before_any_device_call():
    lib = L.lib()

    def call(B=2, Hb=4, Wb=6, ti=0, to=0, **kw):
        p = dict(y=0x1000, c=0x2000, ay=0x3000, ac=0x4000, out=0x5000)
        p.update(kw)
        return lib.rgbnm_swin_embed(ti, to, p["y"], p["c"], p["ay"], p["ac"], p["out"], B, Hb, Wb, None)
    for Hb, Wb in ((3, 4), (4, 3), (5, 7), (1, 2), (2, 1)):
        assert call(Hb=Hb, Wb=Wb) == EINVAL, (Hb, Wb)
    for B in (0, -1):
        assert call(B=B) == EINVAL, B
    for k in ("y", "c", "ay", "ac", "out"):
        assert call(**{k: None}) == EINVAL, k
