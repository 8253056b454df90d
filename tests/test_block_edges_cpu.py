"""CPU tests of the machinery behind tests/test_block_edges.py (no GPU, no rgb_no_more_amd kernel):
- composing the stage references of tests/block_ref.py in fp64 reproduces oracle/vit_torch's encoder block and its fp64 autograd
  gradients (every parameter and dx) to 1e-12 relative: stage-local checks + this anchor = whole-block correctness;
- a torch emulation of each path's rounding points (fp32 accumulation, bf16 where the path stores or stages) runs on the committed
  case inputs through the very check functions the GPU test calls and passes EVERY stage: the bounds admit a correct kernel.
  This is measured on the reference side, never on a kernel.  Worst ratios of the emulations (B = 2, depth 2; |err| / bound),
  chain | staged (= the fused per-operation path: same rounding points, one emulation):
      xn1, xn2 0.50 | 0.50 (statistics 0.01)   qkv 0.50 | 0.50   attn 0.38 | 0.33   lse 0.26 | 0.26   x_mid 0.50 | 0.50
      gl 0.49 | 0.49   u 0.49 | 0.49   x_out 0.49 | 0.49   du 0.50 | 0.50   dx_mid 0.46 | 0.46   dattn 0.50 | 0.50   dq 0.22 | 0.27
      dk 0.18 | 0.15   dv 0.27 | 0.27   dx 0.49 | 0.49   per-image parts 0.11 | 0.14   dW 0.012 | 0.009   db 0.002 | 0.002
      dln 0.17 | 0.17                       (the 16-bit outputs sit at half an ulp: round-to-nearest of a nearly exact value)
  The staged emulation FAILS the chain's residual bound (test_staged_rounding_fails_the_chain_bound): the `inter` term is real.
- defects that the suite's older bars let pass are seeded into the emulation and have to be rejected by those checks;
- the committed case lists reach the regimes they claim (launcher arithmetic copied in Python, table tails, denormal-free).
"""
import numpy as np
import pytest
import torch

import block_ref as R
import kernel_check as KC
from block_ref import BF16, E, HEADS, HID, INNER, NTOK
from oracle import vit_torch as V

RTOL = 1e-12


def close(a, b, what):
    a, b = a.double(), b.double()
    err = float((a - b).abs().max())
    scale = float(b.abs().max()) + 1e-300
    assert err <= RTOL * scale, f"{what}: max |diff| {err:.3g} at scale {scale:.3g}"


def rel(a, b):
    """the max-norm relative error of tests/test_chain_fwd.py"""
    a, b = a.double(), b.double()
    return float((a - b).abs().max() / b.abs().max())


# ================================================================================================================= anchor
def test_composed_stage_references_reproduce_the_oracle_block_and_its_gradients():
    B = 2
    g = torch.Generator().manual_seed(5)
    p = {k: torch.randn(s, generator=g, dtype=torch.float64) * (0.1 if len(s) > 1 else 0.3)
         for k, s in V.param_shapes(depth=1).items() if k.startswith("encoder.0.")}
    for k in p:
        if "lrnorm" in k and k.endswith("weight"):
            p[k] = p[k] + 1.0
        p[k].requires_grad_(True)
    x = (torch.randn(B, NTOK, E, generator=g, dtype=torch.float64) * 2).requires_grad_(True)
    dy = torch.randn(B * NTOK, E, generator=g, dtype=torch.float64)
    out = V.encoder_block(p, 0, x, HEADS, E)
    (out.reshape(-1, E) * dy).sum().backward()
    a, b = "encoder.0.0.fn.", "encoder.0.1.fn."
    rows = R.qkv_rows()
    d = lambda k: p[k].detach()                                   # noqa: E731
    P = dict(ln1_g=d(a + "eb_lrnorm1.weight"), ln1_b=d(a + "eb_lrnorm1.bias"), ln2_g=d(b + "eb_lrnorm2.weight"),
             ln2_b=d(b + "eb_lrnorm2.bias"), wqkv=d(a + "eb_mha.qkv.weight")[rows], bqkv=d(a + "eb_mha.qkv.bias")[rows],
             wproj=d(a + "eb_mha.projection.weight"), bproj=d(a + "eb_mha.projection.bias"), w1=d(b + "eb_ffb.0.weight"),
             b1=d(b + "eb_ffb.0.bias"), w2=d(b + "eb_ffb.3.weight"), b2=d(b + "eb_ffb.3.bias"))
    # forward stages 1 - 7
    x_in = x.detach().reshape(-1, E)
    l1 = R.ln_fwd(x_in, P["ln1_g"], P["ln1_b"])
    qkv = R.linear(l1["y"], P["wqkv"], P["bqkv"])[0]
    at = R.attn_fwd(qkv, B)
    x_mid = x_in + R.linear(at["out"], P["wproj"], P["bproj"])[0]
    l2 = R.ln_fwd(x_mid, P["ln2_g"], P["ln2_b"])
    pre = R.linear(l2["y"], P["w1"], P["b1"])[0]
    gl, u = R.gelu64(pre), R.dgelu64(pre)
    x_out = x_mid + R.linear(gl, P["w2"], P["b2"])[0]
    close(x_out, out.detach().reshape(-1, E), "block output")
    # backward stages 1 - 7
    du = (dy @ P["w2"]) * u
    b2_ = R.ln_bwd(du @ P["w1"], x_mid, l2["mean"], l2["rstd"], P["ln2_g"], dy)
    dx_mid = b2_["dx"]
    dattn = dx_mid @ P["wproj"]
    ab = R.attn_bwd(qkv, at["out"], dattn, at["lse"], B)
    dqkv = torch.cat([ab["dq"][0], ab["dk"][0], ab["dv"][0]], 1)
    b1_ = R.ln_bwd(dqkv @ P["wqkv"], x_in, l1["mean"], l1["rstd"], P["ln1_g"], dx_mid)
    close(b1_["dx"], x.grad.reshape(-1, E), "dx")
    got = {a + "eb_lrnorm1.weight": b1_["dgamma"].sum(0), a + "eb_lrnorm1.bias": b1_["dbeta"].sum(0),
           b + "eb_lrnorm2.weight": b2_["dgamma"].sum(0), b + "eb_lrnorm2.bias": b2_["dbeta"].sum(0)}
    for wk, bk, dyk, xk, perm in ((b + "eb_ffb.3.", None, dy, gl, False), (b + "eb_ffb.0.", None, du, l2["y"], False),
                                  (a + "eb_mha.projection.", None, dx_mid, at["out"], False),
                                  (a + "eb_mha.qkv.", None, dqkv, l1["y"], True)):
        dw, _, db, _ = R.tn(dyk, xk)
        if perm:
            dw2, db2 = torch.empty_like(dw), torch.empty_like(db)
            dw2[rows], db2[rows] = dw, db
            dw, db = dw2, db2
        got[wk + "weight"], got[wk + "bias"] = dw, db
    assert sorted(got) == sorted(p)
    for k in p:
        close(got[k], p[k].grad, k)


# ============================================================================================================== emulation
def emulate(path, B=2, depth=2, rounded=True, e=E, heads=HEADS, **defect):
    """The blocks of one committed case on the emulation of `path`: [(P, A, G, W)] per block, hand-offs as the kernels'."""
    Ps = R.make_params(depth, 1, e, heads)
    x = R.make_x0(B, 1, e)
    fw = []
    for P in Ps:
        A = R.emu_block_fwd(P, x, B, path, **defect)
        fw.append(A)
        x = A["x_out"]
    dy = R.make_dy(B, 1, e)
    out = [None] * depth
    for i in range(depth - 1, -1, -1):
        G = R.emu_block_bwd(Ps[i], fw[i], dy, B, rounded)
        out[i] = (Ps[i], fw[i], G, R.emu_block_dw(fw[i], G))
        dy = G["dx"]
    return out


_CACHE = {}


def emulated(path):
    if path not in _CACHE:
        _CACHE[path] = emulate(path)
    return _CACHE[path]


def check_all(blocks, B, inter, worst):
    infos = []
    for i, (P, A, G, W) in enumerate(blocks):
        where = f"emulation block {i}"
        infos.append(R.check_block_fwd(worst, where, P, A, B, inter=inter))
        r2, r1 = R.check_block_bwd(worst, where, P, A, G, B)
        R.check_block_dw(worst, where, A, G, W, B)
        R.check_dln_total(worst, where, r2, r1, W, B)                 # (the per-operation paths' form of the same sums)
    return infos


@pytest.mark.parametrize("path", ["chain", "staged"])
def test_emulation_of_each_path_passes_every_stage(path):
    """The per-operation staged and fused paths round at the same points (block_ref.emu_block_fwd names the source lines:
    gemm.hip pass 1, gemm_nt_kpipe_body.inc:336, mlp_fused.hip:24), so one emulation, 'staged', is the proof for both."""
    worst = KC.Worst()
    check_all(emulated(path), 2, path != "chain", worst)
    worst.report(f"emulation {path}")
    assert max(worst.d.values()) <= 1.0


def test_chain_emulation_also_passes_at_one_image_and_three_block_hand_offs():
    worst = KC.Worst()
    blocks = emulate("chain", B=1, depth=3)
    check_all(blocks, 1, False, worst)
    for P, A, G, W in blocks:            # d(attention output) not kept (one scratch for all blocks): its GEMM bound is propagated
        R.check_block_bwd(worst, "emulation, dattn not stored", P, A, dict(G, dattn=None), 1)
    worst.report("emulation chain B=1 depth=3")


def test_staged_emulation_passes_at_e384_six_heads():
    """The widths of the E = 384 composite case of the GPU file: the references and checks take them from the tensors."""
    worst = KC.Worst()
    check_all(emulate("staged", B=1, depth=1, e=384, heads=6), 1, True, worst)
    worst.report("emulation staged E=384")


def test_staged_rounding_fails_the_chain_bound():
    """The residual epilogue's `inter` term is real: the per-operation rounding order does not fit the chain's tighter bound."""
    P, A, G, W = emulated("staged")[0]
    with pytest.raises(AssertionError, match="x_mid"):
        R.check_res(KC.Worst(), "x_mid", "staged under the chain bound", A["attn"], P["wproj"], P["bproj"], A["x_in"], A["x_mid"],
                    False, 2)


# ========================================================================================================= seeded defects
def ulps(t, n):
    return (t.double() + n * KC.ulp(t, BF16)).to(BF16)


def test_defect_one_token_row_of_x_mid_off_by_four_ulps():
    P, A, G, W = emulated("chain")[0]
    x = A["x_mid"].clone()
    row = NTOK + 77                                               # image 1, token 77
    assert float(x[row].abs().max()) < 16
    x[row] = ulps(x[row], 4)
    assert rel(x, A["x_mid"]) < 6e-2                              # tests/test_chain_fwd.py: the bar of every block's saved tensors
    with pytest.raises(AssertionError, match="x_mid"):
        R.check_res(KC.Worst(), "x_mid", "defect", A["attn"], P["wproj"], P["bproj"], A["x_in"], x, False, 2)


def test_defect_one_padded_key_with_weight_2_pow_minus_10():
    P = R.make_params(1)[0]
    x = R.make_x0(2)
    good = R.emu_block_fwd(P, x, 2)
    A = R.emu_block_fwd(P, x, 2, pad_key_weight=2.0 ** -10)
    A["lse"] = A["lse"] + float(np.log1p(2.0 ** -10))
    assert rel(A["attn"], good["attn"]) < 2e-2 and rel(A["x_out"], good["x_out"]) < 1e-2       # the old bars accept it
    with pytest.raises(AssertionError, match="lse"):
        R.check_bound(A["lse"].reshape(2, HEADS, NTOK), *[R.attn_fwd(A["qkv"].double(), 2)[k] for k in ("lse", "lsemag")],
                      R.F32, 2, R.ATTN_C["lse"] * KC.U, "defect lse")
    A["lse"] = good["lse"]                                        # the output alone: rows whose mass sits on small |v|
    with pytest.raises(AssertionError, match="attn"):
        R.check_attn_fwd(KC.Worst(), "defect", A["qkv"], A["attn"], A["lse"], 2)


def test_defect_half_dgelu_in_the_negative_tail():
    P = R.make_params(1)[0]
    A = R.emu_block_fwd(P, R.make_x0(2), 2, half_dgelu_tail=True)
    with pytest.raises(AssertionError, match=" u"):
        R.check_gelu(KC.Worst(), "defect", A["xn2"], P["w1"], P["b1"], A["gl"], A["u"], 2)


def test_defect_residual_added_before_the_bias_at_one_tile():
    """x_mid = bf16(bf16(x + acc) + bias) in one 32-row tile: two roundings, the first one in the binade of x + acc.  The chain
    bound (no `inter`) rejects it; the per-operation bound, which allows one intermediate rounding, does not."""
    P, A, G, W = emulated("chain")[0]
    x = A["x_mid"].clone()
    t = slice(64, 96)
    acc = A["attn"][t].float() @ P["wproj"].float().T
    x[t] = ((acc + A["x_in"][t].float()).to(BF16).float() + P["bproj"]).to(BF16)
    assert rel(x, A["x_mid"]) < 1e-2
    with pytest.raises(AssertionError, match="x_mid"):
        R.check_res(KC.Worst(), "x_mid", "defect", A["attn"], P["wproj"], P["bproj"], A["x_in"], x, False, 2)


def test_defect_part2_of_one_image_over_192_tokens():
    P, A, G, W = emulated("chain")[0]
    G2 = dict(G)
    dxn = (G["du"].float() @ P["w1"].float()).to(BF16).float()
    xh = (A["x_mid"].float() - A["mean2"][:, None]) * A["rstd2"][:, None]
    part = G["part2"].clone()
    part[1, 0] = (dxn * xh)[NTOK:NTOK + 192].sum(0)
    part[1, 1] = dxn[NTOK:NTOK + 192].sum(0)
    G2["part2"] = part
    with pytest.raises(AssertionError, match="dx_mid-part|dx_mid part"):
        R.check_block_bwd(KC.Worst(), "defect", P, A, G2, 2)


def test_defect_dw1_missing_the_last_four_tokens_of_one_image():
    P, A, G, W = emulated("chain")[0]
    W2 = dict(W)
    keep = torch.ones(2 * NTOK, dtype=torch.bool)
    keep[192:196] = False
    W2["dw1"] = G["du"].float()[keep].T @ A["xn2"].float()[keep]
    n0, n1 = float(W["dw1"].double().norm()), float(W2["dw1"].double().norm())
    print(f"dW1 norm: {n0:.6g} -> {n1:.6g} ({abs(n1 - n0) / n0:.3g} relative)")
    assert abs(n1 - n0) / n0 < 6e-3                               # tests/test_chain_bwd.py: the bar of the golden gradient norms
    with pytest.raises(AssertionError, match="dw1"):
        R.check_block_dw(KC.Worst(), "defect", A, G, W2, 2)


def test_defect_dwqkv_left_de_interleaved():
    P, A, G, W = emulated("chain")[0]
    W2 = dict(W)
    W2["dwqkv"] = G["dqkv"].float().T @ A["xn1"].float()
    assert float(W2["dwqkv"].double().norm()) == pytest.approx(float(W["dwqkv"].double().norm()), rel=1e-6)   # a norm cannot see it
    with pytest.raises(AssertionError, match="dwqkv"):
        R.check_block_dw(KC.Worst(), "defect", A, G, W2, 2)


def test_unrounded_staging_tile_passes():
    """Not a defect: a LayerNorm backward that reads the GEMM result in fp32 is more accurate and must stay inside the bound."""
    worst = KC.Worst()
    for P, A, G, W in emulate("chain", rounded=False):
        R.check_block_bwd(worst, "unrounded staging", P, A, G, 2)
    worst.report("unrounded staging tile")


# ================================================================================================================ regimes
def test_case_lists_name_every_batch_and_depth():
    assert {b for b, _ in R.CHAIN_CASES} >= set(R.CHAIN_B) and {d for _, d in R.CHAIN_CASES} == set(R.CHAIN_DEPTHS)
    big = [(b, d) for b, d in R.CHAIN_CASES if d == 12 and R.resolve_b(b) > 16]
    assert big == [(300, 12)]                                     # the large B x depth 12 product: one case
    # the grouped pipelined weight-gradient launch needs 196 B % 64 == 0: every n of DW_N reaches it
    assert {d for b, d in R.CHAIN_CASES if R.resolve_b(b) % 16 == 0} == set(R.DW_N)


def test_launcher_arithmetic_of_the_fused_forward_edges():
    rows = {B: R.mlp_fwd_panel_rows(B * NTOK) for B in R.PEROP_B}
    assert rows == {41: (32, True), 42: (33, True), 256: (196, True), 257: (197, False), 300: (224, False), 586: (224, False)}
    assert R.cdiv(586 * NTOK, 224) == 513 and R.cdiv(585 * NTOK, 224) == 512
    assert R.cdiv(300 * NTOK, 224) == 263 and 300 * NTOK - 262 * 224 == 112
    assert 41 * NTOK < 8192 <= 42 * NTOK


@pytest.mark.parametrize("B,depth", [(1, 12), (2, 2)])
def test_committed_inputs_reach_their_regimes(B, depth):
    Ps = R.make_params(depth)
    x = R.make_x0(B)
    for i, P in enumerate(Ps):
        A = R.emu_block_fwd(P, x, B)
        info = R.check_block_fwd(KC.Worst(), f"regimes block {i}", P, A, B)
        pre = info["pre"]
        assert float(pre.abs().min()) >= R.DENORMAL_FREE
        # the table's window measured on the MI355X ends at -16 and 4 (mlp_fused.hip); the GPU test asserts the populations from
        # rgbnm_gelu_table_info itself
        assert int((pre < -18).sum()) >= 8 * B * NTOK // 2 and int((pre > 6).sum()) >= 8 * B * NTOK // 2
        assert int((pre.abs() < 3).sum()) > pre.numel() // 2
        assert info["onehot_rows"] >= B * NTOK // 10, info["onehot_rows"]
        if i == 0:
            assert info["rstd1_max"] > 0.8 * R.EPS ** -0.5, info["rstd1_max"]
            assert float(x.float().std()) > 2.5                   # the scale of the deep blocks' residual stream
        x = A["x_out"]
