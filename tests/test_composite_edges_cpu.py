"""CPU tests of the machinery behind tests/test_composite_edges.py and the past-the-cap case of tests/test_dropout_kernels.py
(no GPU, no rgb_no_more_amd kernel):
- anchors: the fp64 stage functions of tests/composite_ref.py composed into a whole masked block, a whole masked model forward
  and backward, the class head and the patch embedding reproduce tests/test_dropout_model.masked_forward and
  oracle.vit_torch.class_head / patch_embed under fp64 autograd, every gradient included, to 1e-12 relative: stage-local checks
  + these anchors = whole-composite correctness;
- emulations: fp32 / 16-bit emulations of each composite's rounding points, in the entries' order of operations, pass every check
  function the GPU file calls (16-bit outputs sit at half an ulp);
- seeded defects: each wiring defect of the list below is REJECTED by those checks.  MODEL_BARS_ACCEPT records, per defect, whether
  the whole-tensor norm bar of tests/test_dropout_model.py (bf16: relative gradient error 0.15) would have accepted it; the test
  asserts the record from the emulation's own gradients;
- the committed case lists reach the launch regimes they name (Python copies of the launchers' arithmetic).
"""
import pytest
import torch

import block_ref as R
import composite_ref as CR
import kernel_check as KC
import step_ends_ref as S
from block_ref import BF16, E, HEADS, NTOK
from oracle import vit_torch as V
from test_dropout_model import BARS, masked_forward

RTOL = 1e-12
SEED, P_DROP = CR.SEEDS[1], 0.1


def close(a, b, what):
    a, b = a.double(), b.double()
    err = float((a - b).abs().max())
    scale = float(b.abs().max()) + 1e-300
    assert err <= RTOL * scale, f"{what}: max |diff| {err:.3g} at scale {scale:.3g}"


# ================================================================================================================ anchors
def _block_params(p, i):
    a, b = f"encoder.{i}.0.fn.", f"encoder.{i}.1.fn."
    rows = R.qkv_rows()
    d = lambda k: p[k].detach()                                   # noqa: E731
    return dict(ln1_g=d(a + "eb_lrnorm1.weight"), ln1_b=d(a + "eb_lrnorm1.bias"), ln2_g=d(b + "eb_lrnorm2.weight"),
                ln2_b=d(b + "eb_lrnorm2.bias"), wqkv=d(a + "eb_mha.qkv.weight")[rows], bqkv=d(a + "eb_mha.qkv.bias")[rows],
                wproj=d(a + "eb_mha.projection.weight"), bproj=d(a + "eb_mha.projection.bias"), w1=d(b + "eb_ffb.0.weight"),
                b1=d(b + "eb_ffb.0.bias"), w2=d(b + "eb_ffb.3.weight"), b2=d(b + "eb_ffb.3.bias"))


def _block_grad_names(i):
    a, b = f"encoder.{i}.0.fn.", f"encoder.{i}.1.fn."
    return {"dln1_g": a + "eb_lrnorm1.weight", "dln1_b": a + "eb_lrnorm1.bias", "dln2_g": b + "eb_lrnorm2.weight",
            "dln2_b": b + "eb_lrnorm2.bias", "dwqkv": a + "eb_mha.qkv.weight", "dbqkv": a + "eb_mha.qkv.bias",
            "dwproj": a + "eb_mha.projection.weight", "dbproj": a + "eb_mha.projection.bias", "dw1": b + "eb_ffb.0.weight",
            "db1": b + "eb_ffb.0.bias", "dw2": b + "eb_ffb.3.weight", "db2": b + "eb_ffb.3.bias"}


def _head_params(p):
    d = lambda k: p["classhead." + k].detach()                    # noqa: E731
    return dict(ln_g=d("ch_lrnorm.weight"), ln_b=d("ch_lrnorm.bias"), w1=d("ch_linear1.weight"), b1=d("ch_linear1.bias"),
                w2=d("ch_linear2.weight"), b2=d("ch_linear2.bias"))


def test_composed_stages_reproduce_the_masked_model_and_its_gradients():
    """Patch embedding -> two masked blocks -> head, forward and backward, against masked_forward under fp64 autograd."""
    B, depth, ncls = 2, 2, 40
    g = torch.Generator().manual_seed(11)
    p = {k: torch.randn(s, generator=g, dtype=torch.float64) * (0.1 if len(s) > 1 else 0.3)
         for k, s in V.param_shapes(depth=depth, n_classes=ncls).items()}
    for k in p:
        if "lrnorm" in k and k.endswith("weight"):
            p[k] = p[k] + 1.0
        p[k].requires_grad_(True)
    y = torch.randn(B, 1, 28, 28, 8, 8, generator=g, dtype=torch.float64)
    cb = torch.randn(B, 2, 14, 14, 8, 8, generator=g, dtype=torch.float64)
    dl = torch.randn(B, ncls, generator=g, dtype=torch.float64)
    logits = masked_forward(p, y, cb, depth, HEADS, E, SEED, P_DROP)
    (logits * dl).sum().backward()
    # forward
    M = B * NTOK
    feat, x = CR.pe64(y, cb, p["patchembed.projection.0.weight"].detach(), p["patchembed.projection.0.bias"].detach(),
                      V.sincos_table(14, 14, E, torch.float64))
    Ps = [_block_params(p, i) for i in range(depth)]
    fs = [CR.factors(SEED, P_DROP, i, M, E) for i in range(depth)]
    for f in fs:
        CR.masks_bite(f, P_DROP, "anchor")
    saved = []
    for i in range(depth):
        saved.append(CR.drop_block64(Ps[i], x, B, fs[i]))
        x = saved[-1]["x_out"]
    hp = _head_params(p)
    got_logits, hs = CR.head64(hp, x.reshape(B, NTOK, E))
    close(got_logits, logits.detach(), "logits")
    # backward
    got = {}
    hg = CR.head64_bwd(hp, x.reshape(B, NTOK, E), hs, dl)
    for k, nm in (("dln_g", "ch_lrnorm.weight"), ("dln_b", "ch_lrnorm.bias"), ("dw1", "ch_linear1.weight"), ("db1", "ch_linear1.bias"),
                  ("dw2", "ch_linear2.weight"), ("db2", "ch_linear2.bias")):
        got["classhead." + nm] = hg[k]
    dy = hg["dx"].reshape(M, E)
    rows = R.qkv_rows()
    for i in range(depth - 1, -1, -1):
        dy, W = CR.drop_block64_bwd(Ps[i], saved[i], dy, B, fs[i])
        for k, nm in _block_grad_names(i).items():
            t = W[k]
            if k in ("dwqkv", "dbqkv"):                           # the kernels' de-interleaved rows -> the reference layout
                t2 = torch.empty_like(t)
                t2[rows] = t
                t = t2
            got[nm] = t
    got["patchembed.projection.0.weight"], _, got["patchembed.projection.0.bias"], _ = R.tn(dy, feat)
    assert sorted(got) == sorted(p)
    for k in p:
        close(got[k], p[k].grad, k)


def test_head_and_patch_embedding_stages_reproduce_the_oracle():
    B, ncls = 3, 40
    g = torch.Generator().manual_seed(12)
    p = {k: (torch.randn(s, generator=g, dtype=torch.float64) * (0.1 if len(s) > 1 else 0.3)).requires_grad_(True)
         for k, s in V.param_shapes(depth=0, n_classes=ncls).items()}
    x = (torch.randn(B, NTOK, E, generator=g, dtype=torch.float64) * 2 + 0.5).requires_grad_(True)
    dl = torch.randn(B, ncls, generator=g, dtype=torch.float64)
    out = V.class_head(p, x, E)
    (out * dl).sum().backward()
    hp = _head_params(p)
    logits, sv = CR.head64(hp, x.detach())
    close(logits, out.detach(), "head logits")
    hg = CR.head64_bwd(hp, x.detach(), sv, dl)
    close(hg["dx"], x.grad, "head dx")
    for k, nm in (("dln_g", "ch_lrnorm.weight"), ("dln_b", "ch_lrnorm.bias"), ("dw1", "ch_linear1.weight"), ("db1", "ch_linear1.bias"),
                  ("dw2", "ch_linear2.weight"), ("db2", "ch_linear2.bias")):
        close(hg[k], p["classhead." + nm].grad, nm)
    y = torch.randn(B, 1, 28, 28, 8, 8, generator=g, dtype=torch.float64)
    cb = torch.randn(B, 2, 14, 14, 8, 8, generator=g, dtype=torch.float64)
    x0 = V.patch_embed(p, y, cb)
    dx0 = torch.randn(B * NTOK, E, generator=g, dtype=torch.float64)
    (x0.reshape(-1, E) * dx0).sum().backward()
    wk, bk = "patchembed.projection.0.weight", "patchembed.projection.0.bias"
    feat, got = CR.pe64(y, cb, p[wk].detach(), p[bk].detach(), V.sincos_table(14, 14, E, torch.float64))
    close(got, x0.detach().reshape(-1, E), "x0")
    dw, _, db, _ = R.tn(dx0, feat)
    close(dw, p[wk].grad, wk)
    close(db, p[bk].grad, bk)


# ============================================================================================================= emulations
B_EMU = 2


def emulate_drop(fwd_f=None, bwd_f=None, defect=None, blocks=(0, 11), p=P_DROP):
    """Two blocks in sequence on the bf16 emulation; fwd_f / bwd_f(i, true factors) -> the factors the emulated kernels use
    (a defect in the masks); the checks always get the contract's.  [(P, A, G, W, f64)] per block."""
    Ps = R.make_params(2)
    M = B_EMU * NTOK
    true = [CR.factors(SEED, p, b, M, E) for b in blocks]
    use = lambda fn, i: {k: v.float() for k, v in (fn(i, true[i]) if fn else true[i]).items()}      # noqa: E731
    x = R.make_x0(B_EMU)
    fw = []
    for i in range(2):
        fw.append(CR.emu_drop_fwd(Ps[i], x, B_EMU, use(fwd_f, i)))
        x = fw[-1]["x_out"]
    dy = R.make_dy(B_EMU)
    out = [None, None]
    for i in (1, 0):
        G, W = CR.emu_drop_bwd(Ps[i], fw[i], dy, B_EMU, use(bwd_f or fwd_f, i), defect)
        out[i] = (Ps[i], fw[i], G, W, true[i])
        dy = G["dx"]
    return out


_GOOD = {}


def good_drop():
    if "d" not in _GOOD:
        _GOOD["d"] = emulate_drop()
    return _GOOD["d"]


def check_drop(blocks, worst=None, p=P_DROP):
    worst = worst or KC.Worst()
    for i, (P, A, G, W, f) in enumerate(blocks):
        info = CR.check_drop_block(worst, worst, worst, f"emulation block {i}", P, A, G, W, B_EMU, f, p)
        CR.regimes(info, B_EMU * NTOK, i == 0, f"emulation block {i}")
    return worst


def test_dropout_block_emulation_passes_every_stage():
    worst = check_drop(good_drop())
    worst.report("dropout block emulation (bf16, staged epilogues)")
    assert max(worst.d.values()) <= 1.0


def test_dropout_block_emulation_passes_at_p_one_half():
    worst = check_drop(emulate_drop(p=0.5, blocks=(0, 1)), p=0.5)
    assert max(worst.d.values()) <= 1.0


def head_case(dt, B=3, N=NTOK, e=E, ncls=40, seed=77, defect=None):
    P = CR.head_params(e, ncls, seed)
    P = {k: v.to(dt) if k in ("w1", "w2") else v for k, v in P.items()}
    x, dl = CR.head_inputs(B, N, e, ncls, dt, seed + 20)
    a, g = CR.emu_head(P, x, dl, dt, defect=defect)
    return P, x, dl, a, g


@pytest.mark.parametrize("dtn,N,e", [("f32", 196, 192), ("bf16", 294, 384), ("f16", 196, 192)])
def test_head_emulation_passes_every_stage(dtn, N, e):
    dt = CR.DT[dtn]
    worst = KC.Worst()
    P, x, dl, a, g = head_case(dt, N=N, e=e)
    CR.check_head_fwd(worst, f"head emulation {dtn}", P, x, a, dt)
    CR.check_head_bwd(worst, f"head emulation {dtn}", P, x, a, dl, g, dt)
    worst.report(f"head emulation {dtn}")
    assert max(worst.d.values()) <= 1.0


def pe_case(TI, TO, B=2, seed=90, defect=None):
    y, c = S.embed_inputs(B, 28, 28, TI, "dct", seed)
    A = V.conv_matrix(16).contiguous()
    P = CR.pe_params(E, NTOK, seed + 3)
    P["wpe"] = P["wpe"].to(TO)
    X = S.gather_x(y.float())                                     # subblock_embed_kernel: two fp32 products, one rounding
    luma = ((A @ X) @ A.T).reshape(-1, 256)
    feat = torch.cat([luma, c.float().permute(0, 2, 3, 1, 4, 5).reshape(-1, 128)], 1).to(TO)
    return y, c, A, P, feat, CR.emu_pe_fwd(feat, P, TO, NTOK, defect)


@pytest.mark.parametrize("TI,TO", S.EMBED_BIG_PAIRS, ids=lambda t: S.NAMES[t])
def test_patch_embedding_emulation_passes(TI, TO):
    worst = KC.Worst()
    y, c, A, P, feat, x0 = pe_case(TI, TO)
    CR.check_pe_fwd(worst, "patch embedding emulation", feat, x0, y, c, A, None, P, TI, TO, NTOK)
    dx0 = R.make_dy(2).to(TO)
    R.check_pe_dw(worst, "patch embedding emulation", dx0, feat, dx0.float().T @ feat.float(), dx0.float().sum(0), 2)
    worst.report(f"patch embedding emulation {S.NAMES[TI]}->{S.NAMES[TO]}")
    assert max(worst.d.values()) <= 1.0


# ========================================================================================================= seeded defects
# defect -> does the whole-tensor bar of tests/test_dropout_model.py (bf16: gradient relative error <= 0.15) accept it?  Measured
# below on the emulation: the worst norm-relative error over the block's twelve parameter gradients and dx (what the blocks in
# front of it receive), or over the head's / patch embedding's outputs.
MODEL_BARS_ACCEPT = {
    # measured norm-relative errors: 0.66, 0.34, 0.32, 1.11, 1.26 | 0.12, 1.42, 0.034 | 0.24, 1.81 | 0.055, 0.005
    "residual_masked": False, "dw2_unmasked": False, "dwproj_unmasked": False, "sites_0_2_swapped": False, "block_index_off_by_one": False,
    "mask1_twice": True, "mask_col_row": False, "scale_in_16_bits": True,
    "da_from_pooled": False, "dw1_from_dpooled": False,
    "pos_period": True, "bias_twice": True,
}
# Four of the twelve pass a 0.15 norm bar: the second mask on du (p = 0.1 zeroes a tenth of a tensor that is mostly small), the
# 16-bit scale, and both patch-embedding defects (x0 is dominated by the DC terms of the features; its whole-tensor error stays at
# 5.5 % and 0.5 %).  (A wrong mask that forward and backward share is still a valid dropout step: the model test rejects those
# only because it rebuilds the masks from the contract, as the stage-local checks do.)


def norm_rel(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-300))


def drop_bar(blocks):
    """worst gradient norm error of the defective run against the good emulation (block 1 ran first: its dx feeds block 0)."""
    worst = 0.0
    for (_, _, G, W, _), (_, _, G0, W0, _) in zip(blocks, good_drop()):
        worst = max([worst, norm_rel(G["dx"], G0["dx"])] + [norm_rel(W[k], W0[k]) for k in W0])
    return worst


def record(name, err):
    accepted = err <= BARS["bf16"][1]
    print(f"defect {name}: worst norm-relative error {err:.3g} -> the model bar {'accepts' if accepted else 'rejects'} it")
    assert MODEL_BARS_ACCEPT[name] == accepted, (name, err)


def rejected(blocks, match, p=P_DROP):
    with pytest.raises(AssertionError, match=match):
        check_drop(blocks, p=p)


@pytest.mark.parametrize("defect,match", [("residual_masked", "dx_mid"), ("dw2_unmasked", "dw2"), ("dwproj_unmasked", "dwproj"),
                                          ("mask1_twice", " du")])
def test_defect_in_the_backward_wiring(defect, match):
    blocks = emulate_drop(defect=defect)
    rejected(blocks, match)
    record(defect, drop_bar(blocks))


def test_defect_sites_0_and_2_swapped():
    blocks = emulate_drop(fwd_f=lambda i, f: {0: f[2], 1: f[1], 2: f[0]})
    rejected(blocks, "x_mid")
    record("sites_0_2_swapped", drop_bar(blocks))


def test_defect_block_index_off_by_one():
    M = B_EMU * NTOK
    blocks = emulate_drop(fwd_f=lambda i, f: CR.factors(SEED, P_DROP, (0, 11)[i] + 1, M, E))
    rejected(blocks, "x_mid")
    record("block_index_off_by_one", drop_bar(blocks))


def test_defect_mask_indexed_col_row():
    import dropout_ref as D
    M = B_EMU * NTOK

    def swapped(i, f):
        return {s: torch.from_numpy(D.factor(SEED, P_DROP, s, (0, 11)[i], t.shape[1], M)).T.contiguous().double() for s, t in f.items()}
    blocks = emulate_drop(fwd_f=swapped)
    rejected(blocks, "x_mid")
    record("mask_col_row", drop_bar(blocks))


def test_defect_scale_taken_in_the_16_bit_type():
    """1 / (1 - p) rounded to bf16 (1.109375 for p = 0.1, 0.16 % low): inside every forward-error bound of a bf16 tensor, and far
    inside the model bars -- the bit-for-bit masked copies are what rejects it."""
    def low(i, f):
        return {s: torch.where(t != 0, t.to(BF16).double(), t) for s, t in f.items()}
    blocks = emulate_drop(fwd_f=low)
    rejected(blocks, "dy_m differs|dxmid_m differs")
    record("scale_in_16_bits", drop_bar(blocks))


@pytest.mark.parametrize("defect,match", [("da_from_pooled", " da"), ("dw1_from_dpooled", "dw1")])
def test_defect_in_the_head(defect, match):
    P, x, dl, a, g = head_case(BF16, defect=defect)
    with pytest.raises(AssertionError, match=match):
        CR.check_head_bwd(KC.Worst(), "defect", P, x, a, dl, g, BF16)
    _, _, _, _, g0 = head_case(BF16)
    record(defect, max(norm_rel(g[k], g0[k]) for k in g0))


@pytest.mark.parametrize("defect", CR.PE_DEFECTS)
def test_defect_in_the_patch_embedding(defect):
    y, c, A, P, feat, x0 = pe_case(BF16, BF16, defect=defect)
    with pytest.raises(AssertionError, match="x0"):
        CR.check_pe_fwd(KC.Worst(), "defect", feat, x0, y, c, A, None, P, BF16, BF16, NTOK)
    good = pe_case(BF16, BF16)[5]
    err = norm_rel(x0, good)
    print(f"defect {defect}: x0 norm-relative error {err:.3g} (the logits bar of the model test is 1e-2)")
    record(defect, err)


# ================================================================================================================ regimes
def test_apply_cases_turn_the_loop_twice_with_a_ragged_last_turn():
    regs = {dtn: CR.apply_regime(M, N) for dtn, M, N in CR.APPLY_BIG}
    for dtn, (grid, turns, last, vec) in regs.items():
        assert grid == 8192 and turns == 2 and 0 < last < CR.APPLY_CAP, (dtn, grid, turns, last)
    assert regs["bf16"][3] and regs["f32"][3] and not regs["f16"][3]          # one 16-bit and one fp32 vector case, one element case
    for dtn, M, N in CR.APPLY_BIG:
        assert M * CR.cdiv(N, 8) > CR.APPLY_CAP and M % 8 and M * N < 2 ** 31
    # the cases of test_apply_on_ones_is_keep_times_scale_bit_for_bit all stay inside one turn: these are the only ones past it
    for M, N in [(1, 1), (37, 13), (300, 200), (512, 192), (129, 768), (7, 4096)]:
        assert CR.apply_regime(M, N)[1] == 1
    assert CR.apply_regime(50176, 384)[1] == 2                                 # JPEG-S's own gradient: [256 * 196, 384]


def test_head_cases_cover_both_sides_of_every_switch():
    cases = CR.HEAD_CASES
    assert {c[1] for c in cases} == set(CR.HEAD_B) and 512 in CR.HEAD_B and 513 in CR.HEAD_B
    for dtn in ("f32", "bf16", "f16"):
        mine = [c for c in cases if c[0] == dtn]
        assert {c[4] for c in mine} == {1000, 40} and {(c[3], c[2]) for c in mine} == {(192, 196), (384, 294)}
        assert {c[5] for c in mine} == {"apart", "shared"} and {c[6] for c in mine} == {0, 1}
    assert all(c[4] % 8 == 0 for c in cases)
    assert {CR.head_nt_kernel("bf16", B) for B in (512, 513)} == {"gemm_nt_small_kernel", "gemm_nt_kernel"}
    assert {CR.head_nt_kernel(d, 1) for d in ("f32", "f16")} == {"gemm_nt_kernel"}
    # a grouped weight-gradient launch (bf16, regions apart, tn_group on, B % 64 == 0) is among the cases
    assert any(c[0] == "bf16" and c[5] == "apart" and c[6] and c[1] % 64 == 0 for c in cases)
    tn_ws = lambda M, No, Ki: 128 * (No * Ki + No) * 4              # noqa: E731  (rgbnm_gemm_tn_workspace: RGBNM_TN_MAX_SPLIT slices)
    for _, B, N, e, ncls, _, _ in cases:
        small = max(tn_ws(B, ncls, e), tn_ws(B, e, e), B * 2 * e * 4)
        assert not CR.head_ws_split(B, e, ncls, small, tn_ws)[0]
        full = sum(b for _, b in CR.head_ws_split(B, e, ncls, 10 ** 12, tn_ws)[1][:2]) + B * 2 * e * 4
        assert CR.head_ws_split(B, e, ncls, full, tn_ws)[0] and not CR.head_ws_split(B, e, ncls, full - 1, tn_ws)[0]


def test_dropout_cases_reach_their_regimes():
    assert {c[0] for c in CR.DROP_GENERIC} == {"f32", "f16", "bf16"}
    for dtn in ("f32", "f16", "bf16"):
        mine = [c for c in CR.DROP_GENERIC if c[0] == dtn]
        assert {c[1] for c in mine} == {1, 3} and {c[2] for c in mine} == {0.1, 0.5}
    assert {b for c in CR.DROP_GENERIC for b in c[3]} == {0, 1, 11} and {c[4] for c in CR.DROP_GENERIC} == {0, 1, 2, 3}
    assert 2 ** 64 - 1 in CR.SEEDS
    assert (CR.DROP_FUSED_B - 1) * NTOK < 8192 <= CR.DROP_FUSED_B * NTOK       # rgbnm_vit_ln_chain / kp7: M >= 8192
    assert (CR.DROP_FUSED_B * NTOK) % 64 != 0                                  # ... and no grouped weight-gradient launch there
    B, e, heads = CR.DROP_E384
    assert e % 384 == 0 and (heads * 64) % 384 == 0 and (B * NTOK) % 64 == 0   # vit.hip block_bwd: wide4
    assert (CR.DROP_GROUP_B * NTOK) % 64 == 0 and (3 * NTOK) % 64 != 0         # gemm.hip tn_groupable
    assert set(CR.PE_B) == {1, 3, 42} and 42 * NTOK >= 8192 and CR.PE_GRID[0] // 2 * (CR.PE_GRID[1] // 2) == NTOK
