"""fp16 on the per-block fused kernels (option f16_tuned = 2): attention v2 (attn2 / persistent attn3 kernels), the fused MLP forward
and backward, and the row-panel GEMM's LayerNorm epilogues, element-wise at their launch edges.  The cases, guards and fp64 bounds
are those of tests/test_kernel_edges.py (attn_case) and tests/block_ref.py (check_block_fwd / _bwd / _dw / _dln_total), which take
the unit roundoff, the ulp and the subnormal spacing from the element type of what the kernel stored: nothing is fitted here.  Every
tuned case asserts through the profiler that the named kernels ran in their fp16 instantiation and the generic ones did not; at
f16_tuned = 1 the same entries must stay on what they launched before level 2 existed.

The driver of the per-block path is tests/test_block_edges.py per_operation with the fp16 expectations: fp16 instantiations of
mlp_fwd_kernel (the arithmetic one: there is no fp16 GELU table, so no table-regime expectation either), mlp_bwd_kernel and
gemm_nt_kpipe, one ln_fwd_kernel launch and no ln_bwd_kernel; dxn stays untouched; guarded buffers, NaN rows behind x0 / dy and the
exact-size workspace as there.

Largest |got - ref| / bound measured on one MI355X (pytest -s prints them; DESIGN.md section 7 repeats them):
    attention v2, either persist setting: out 0.35, lse 0.53, dq 0.20, dk 0.12, dv 0.24; N = 225 (generic): 0.32 / 0.19 / 0.15 / 0.05 / 0.14
    per-block path, all batches and E = 384: xn1, xn2 0.49  qkv 0.49  attn 0.42  lse 0.78  x_mid, x_out 0.49  gl 0.60  u 0.45  du 0.49
    dx_mid 0.44  dattn 0.49  dq 0.34  dk 0.38  dv 0.29  dx 0.48  dln 0.009  dW 1.6e-4  db 1.1e-4
Before the forward kernels shifted their probabilities out of fp16's subnormal range (attention_v2.hip, PShift) the attention output
of block 1 at B = 257 missed its bound in 2 of 9 671 424 elements, by a factor 1.19.
"""
import ctypes as C

import pytest
import torch

import block_ref as R
import kernel_check as KC
import test_kernel_edges as TE
from block_ref import F32, NTOK
from kernel_check import guarded, launched, ran
from rgb_no_more_amd import lib as L
from test_block_edges import Case, GRAD_SHAPES, collecting, finish, _untouched
from test_fp16_tuned_kernels import is_f16, launches  # noqa: F401  (launches: fixture)
from test_hip_kernels import option  # noqa: F401  (fixture: set a runtime switch for one test)

pytestmark = pytest.mark.gpu
F16 = torch.float16
EINVAL = -1
ATTN_N = (1, 31, 32, 33, 63, 64, 65, 196, 223, 224)


@pytest.fixture(scope="module", autouse=True)
def gelu_table():
    """As tests/test_block_edges.py: the table exists on this device, so that fp16 not taking it is the library's choice."""
    L.check(L.lib().rgbnm_gelu_table_init(L.stream()), "gelu_table_init")


# ------------------------------------------------------------------------------------------------------------- attention
@pytest.mark.parametrize("persist", [0, 1])
def test_attention_v2_fp16(option, launches, persist):
    """test_kernel_edges.test_attention_v2_edges in fp16 at level 2, plus N = 225, which stays on the generic fp16 kernels."""
    option("f16_tuned", 2)
    option("attn_v2", 1)
    option("attn_persist", persist)
    worst = KC.Worst()
    cases = [(2, n, 3) for n in ATTN_N] + [(3, 65, h) for h in (1, 6, 12)]
    if persist:
        cases += [(85, 196, 3), (256, 65, 1), (257, 33, 1), (257, 224, 1), (43, 196, 6)]
    for i, (B, N, H) in enumerate(cases):
        if persist:
            wf = "attn3_fwd_kernel" if B * H >= 256 else "attn2_fwd_kernel"
            wb = "attn3_bwd_kernel"
        else:
            wf, wb = "attn2_fwd_kernel", "attn2_bwd_kernel"
        TE.attn_case(F16, B, N, H, 80 + i, (wf,), (wb,), worst, "bh>=256" if B * H >= 256 else "v2")
        fwd_names, bwd_names = launches[-2], launches[-1]
        for names, kern in ((fwd_names, wf), (bwd_names, wb)):
            hits = [n for n in names if kern in n]
            assert hits and all(is_f16(n) for n in hits), (B, N, H, hits)
            assert not ran(names, "attn_fwd_kernel") and not ran(names, "attn_bwd_dq_kernel") and not ran(names, "attn_bwd_dkv_kernel"), \
                (B, N, H, sorted(set(names)))
    # 225 tokens: above the 224 rows of the LDS arrays -> the generic kernels with 10 tiles, in fp16
    TE.attn_case(F16, 2, 225, 3, 300, (("attn_fwd_kernel", "10"),), (("attn_bwd_dq_kernel", "10"), ("attn_bwd_dkv_kernel", "10")),
                 worst, "n225")
    for names in (launches[-2], launches[-1]):
        assert not any("attn2_" in n or "attn3_" in n for n in names), sorted(set(names))
        assert all(is_f16(n) for n in names if "attn_" in n), sorted(set(names))
    worst.report(f"fp16 fused: attention v2 persist={persist}")


def test_attention_level_1_stays_on_the_generic_kernels(option, launches):
    """f16_tuned = 1 (and 0): fp16 attention launches the first-generation kernels, as before level 2 existed, and both levels
    give the same bits."""
    option("attn_v2", 1)
    worst = KC.Worst()
    B, N, H = 3, 196, 3
    I = H * 64
    outs = {}
    for level in (1, 0):
        option("f16_tuned", level)
        TE.attn_case(F16, B, N, H, 500, (("attn_fwd_kernel", "7"),), (("attn_bwd_dq_kernel", "7"), ("attn_bwd_dkv_kernel", "7")),
                     worst, f"level{level}")
        for names in (launches[-2], launches[-1]):
            assert not any("attn2_" in n or "attn3_" in n for n in names), sorted(set(names))
        qkv = TE.rnd((B * N, 3 * I), 501, 1.5, F16)
        out, lse = torch.empty(B * N, I, device="cuda", dtype=F16), torch.empty(B * H * N, device="cuda")
        L.check(L.lib().rgbnm_attention_fwd(L.dt_of(F16), qkv.data_ptr(), out.data_ptr(), lse.data_ptr(), B, N, H, I ** -0.5, L.stream()))
        torch.cuda.synchronize()
        outs[level] = (out, lse)
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    worst.report("fp16 attention at f16_tuned = 1 / 0 (generic kernels)")


# ---------------------------------------------------------------------------------------------- per-block fused path
def is_table(n):
    return "mlp_fwd_kernel" in n and ("mlp_fwd_kernel<true" in n or "<(bool)1" in n or "mlp_fwd_kernelILb1" in n)


def per_block(c, where, fused, attn2=None, logit=False):
    """tests/test_block_edges.py per_operation for an fp16 Case.  fused True: the E = 192 fused kernels are expected in their fp16
    instantiations; False: none of them may run (LayerNorm-chained epilogues, fused MLP); None: E = 384, only attention is asked.
    attn2: True / False / None -- attention v2 in its fp16 instantiation is expected / forbidden / not asked."""
    lib, B = L.lib(), c.B
    HID, INNER, E = 4 * c.e, c.inner, c.e
    wf, wb, wd = collecting("perop-fwd", "perop-bwd", "perop-dw")
    soft = []
    lnchain = lib.rgbnm_vit_ln_chain(C.byref(c.cfg))
    if fused is not None:
        assert lnchain == int(fused)
    acts = c.new_acts()
    bp = [L.BlockParams(*[p[k].data_ptr() for k in ("ln1_g", "ln1_b", "ln2_g", "ln2_b", "bqkv", "bproj", "b1", "b2")],
                        *[t.data_ptr() for k in ("wqkv", "wproj", "w1", "w2") for t in (p[k], p[k + "_t"])]) for p in c.P]
    ba = [L.BlockActs(*[c.act_tensors(acts, i)[k].data_ptr() for k, _ in L.BlockActs._fields_]) for i in range(2)]

    def fwd():
        L.check(lib.rgbnm_vit_block_fwd_chain(C.byref(c.cfg), C.byref(bp[0]), C.byref(ba[0]), 0, C.byref(bp[1]), C.byref(ba[1]),
                                              L.stream()), "block 0")
        L.check(lib.rgbnm_vit_block_fwd_chain(C.byref(c.cfg), C.byref(bp[1]), C.byref(ba[1]), lnchain, None, None, L.stream()),
                "block 1")
    _, names = launched(fwd)

    def expect(cond, what, names):
        if not cond:
            soft.append(f"{where}: {what}; ran {sorted(set(names))}")

    def all_f16(names, sub):
        hits = [n for n in names if sub in n]
        return bool(hits) and all(is_f16(n) for n in hits)

    def attention(names, v2kern, what):
        if attn2 is None:
            return
        if attn2:
            expect(any(all_f16(names, k) for k in v2kern) and not ran(names, "attn_fwd_kernel") and not ran(names, "attn_bwd_dq_kernel"),
                   what + ": attention v2 in fp16", names)
        else:
            expect(not any("attn2_" in n or "attn3_" in n for n in names), what + ": generic attention", names)
    attention(names, ("attn2_fwd_kernel", "attn3_fwd_kernel"), "forward")
    if fused:
        expect(all_f16(names, "mlp_fwd_kernel") and not any(is_table(n) for n in names), "fp16 arithmetic mlp_fwd_kernel", names)
        expect(all_f16(names, "gemm_nt_kpipe"), "gemm_nt_kpipe in fp16", names)
        expect(sum("ln_fwd_kernel" in n for n in names) == 1, "block 0's LN1 only: every other LayerNorm is fused", names)
    elif fused is False:
        expect(not ran(names, "mlp_fwd_kernel"), "no fused MLP", names)
        expect(sum("ln_fwd_kernel" in n for n in names) == 4 and ran(names, "gemm_nt"), "four LayerNorm launches, plain GEMMs", names)
    for i in range(2):
        for k, g in acts[i].items():
            g.check(f"{where} block {i} {k}")
        info = R.check_block_fwd(wf, f"{where} block {i}", c.P[i], c.act_tensors(acts, i), B, inter=True, logit=logit)
        if logit and info["lse_absmin"] < 70:
            soft.append(f"{where} block {i}: min |lse| {info['lse_absmin']:.4g}, no logit offset")
        if info["onehot_rows"] < c.M // 10 or (i == 0 and info["rstd1_max"] <= 0.8 * R.EPS ** -0.5):
            soft.append(f"{where} block {i}: one-hot rows {info['onehot_rows']}, max rstd1 {info['rstd1_max']:.4g}")
        del info
    # backward: block 1, then block 0 on the dx it left
    wsb = lib.rgbnm_vit_workspace(C.byref(c.cfg))
    dy = c.dy
    for i in (1, 0):
        sc = dict(du=guarded(c.M, HID, c.dt), dxn=guarded(c.M, E, c.dt), dx_mid=guarded(c.M, E, c.dt), dattn=guarded(c.M, INNER, c.dt),
                  dqkv=guarded(c.M, 3 * INNER, c.dt), ws=guarded(wsb // 4, None, F32), dx=guarded(c.M, E, c.dt))
        k_ = E // 192                                       # (GRAD_SHAPES are those of E = 192)
        grads = {k: guarded(sh[0] * k_, sh[1] * k_ if len(sh) > 1 else None, F32) for k, sh in GRAD_SHAPES}
        bg = L.BlockGrads(*[grads[k].t.data_ptr() for k, _ in L.BlockGrads._fields_])
        bs = L.BlockScratch(*[sc[k].t.data_ptr() for k in ("du", "dxn", "dx_mid", "dattn", "dqkv", "ws")], wsb)
        rc, names = launched(lambda: lib.rgbnm_vit_block_bwd(C.byref(c.cfg), C.byref(bp[i]), C.byref(ba[i]), C.byref(bg), C.byref(bs),
                                                             dy.data_ptr(), sc["dx"].t.data_ptr(), L.stream()))
        assert rc == 0, (where, rc)
        attention(names, ("attn2_bwd_kernel", "attn3_bwd_kernel"), "backward")
        if fused:
            expect(all_f16(names, "mlp_bwd_kernel") and all_f16(names, "gemm_nt_kpipe"), "fused backward kernels in fp16", names)
            expect(not ran(names, "ln_bwd_kernel"), "no LayerNorm backward kernel", names)
        elif fused is False:
            expect(not ran(names, "mlp_bwd_kernel") and ran(names, "ln_bwd_kernel"), "unfused backward", names)
        w = f"{where} bwd block {i}"
        for k, g in sc.items():
            if k == "dxn" and fused:                      # the fused forms keep du . W1 / dqkv . Wqkv in LDS
                assert bool((g.raw == g.canary).all()), f"{w}: dxn was written"
            else:
                g.check(f"{w} {k}", written=(k != "ws"))
        for k, g in grads.items():
            g.check(f"{w} {k}")
        A = c.act_tensors(acts, i)
        G = dict(dy=dy, du=sc["du"].t, dx_mid=sc["dx_mid"].t, dattn=sc["dattn"].t, dqkv=sc["dqkv"].t, dx=sc["dx"].t)
        r2, r1 = R.check_block_bwd(wb, w, c.P[i], A, G, B, logit=logit)
        Wg = {k: g.t for k, g in grads.items()}
        R.check_block_dw(wd, w, A, G, Wg, B)
        R.check_dln_total(wd, w, r2, r1, Wg, B)
        dy = sc["dx"].t
        del r2, r1
    finish(where, ("perop-fwd", "perop-bwd", "perop-dw"), soft)


@pytest.mark.parametrize("B,dmast", [(41, None), (42, None), (257, None), (300, None), (42, 0), (42, 1)])
def test_per_block_fused_path_fp16(option, B, dmast):
    """B = 41: 8036 rows, below the 8192-row threshold: nothing fused may run.  B = 42: the first eligible batch (33-row panels).
    B = 257: 197-row panels, 256 panels, ragged last panel.  B = 300: the 224-row cap, more panels than CUs.  mlp_dmast both ways
    at B = 42."""
    option("f16_tuned", 2)
    if dmast is not None:
        option("mlp_dmast", dmast)
    per_block(Case(B, 2, images=False, dt=F16), f"fp16 per-block B={B}" + ("" if dmast is None else f" mlp_dmast={dmast}"),
              B * NTOK >= 8192, attn2=True)


def test_per_block_fused_path_fp16_with_a_logit_offset(option):
    """B = 42 at level 2 with block_ref.make_params(offset=+1): q[:, 0] = 32 and k[:, 0] = 64 in every head (exact in fp16), every
    logit and lse at +148 scaled units, through the fp16 attn2 forward (the 2^14 shift) and backward inside the block; the stage
    checks of the case above plus block_ref.logit_err."""
    option("f16_tuned", 2)
    per_block(Case(42, 2, images=False, dt=F16, offset=1), "fp16 per-block B=42 offset=+1", True, attn2=True, logit=True)


def test_per_block_level_1_runs_none_of_the_fused_kernels(option):
    """f16_tuned = 1 at the first eligible batch: rgbnm_vit_ln_chain says no, the MLP and the LayerNorms run unfused and attention
    on the generic kernels -- what level 1 launched before level 2 existed."""
    option("f16_tuned", 1)
    per_block(Case(42, 2, images=False, dt=F16), "fp16 per-block B=42 f16_tuned=1", False, attn2=False)


def test_e384_fp16_takes_attention_v2_only(option):
    """E = 384, 6 heads, B = 64 (12544 rows): attention v2 in its fp16 instantiation; the fused MLP and the LayerNorm epilogues are
    E = 192 only."""
    option("f16_tuned", 2)
    c = Case(64, 2, images=False, e=384, heads=6, dt=F16)
    assert L.lib().rgbnm_vit_ln_chain(C.byref(c.cfg)) == 0
    per_block(c, "fp16 E=384 B=64", None, attn2=True)


def test_chain_flag_is_refused_below_the_row_threshold_and_writes_nothing(option):
    """Level 2, fp16, B = 41: rgbnm_vit_block_fwd_chain with flags & 1 ("LN1 was chained in") returns RGBNM_EINVAL, launches nothing
    and writes nothing -- as bf16 does."""
    option("f16_tuned", 2)
    lib = L.lib()
    for dt in (F16, torch.bfloat16):
        c = Case(41, 1, images=False, dt=dt)
        assert lib.rgbnm_vit_ln_chain(C.byref(c.cfg)) == 0
        acts = c.new_acts()
        p = c.P[0]
        bp = L.BlockParams(*[p[k].data_ptr() for k in ("ln1_g", "ln1_b", "ln2_g", "ln2_b", "bqkv", "bproj", "b1", "b2")],
                           *[t.data_ptr() for k in ("wqkv", "wproj", "w1", "w2") for t in (p[k], p[k + "_t"])])
        ba = L.BlockActs(*[c.act_tensors(acts, 0)[k].data_ptr() for k, _ in L.BlockActs._fields_])
        rc, names = launched(lambda: lib.rgbnm_vit_block_fwd_chain(C.byref(c.cfg), C.byref(bp), C.byref(ba), 1, None, None, L.stream()))
        assert rc == EINVAL and names == [], (dt, rc, names)
        _untouched([(k, g) for k, g in acts[0].items()], f"flags & 1 at B = 41 {dt}")
