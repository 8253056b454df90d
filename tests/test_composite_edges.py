"""Element-wise tests of the composites of csrc/vit.hip that only the model used to reach: the dropout encoder block
(rgbnm_vit_block_fwd_drop / _bwd_drop), the class head (rgbnm_head_fwd / _bwd) and the patch embedding (rgbnm_patch_embed_fwd,
_fwd_mix, _bwd), at the C ABI (include/rgbnm.h), against the stage-local fp64 references and bounds of tests/composite_ref.py
(read its docstring first; tests/test_composite_edges_cpu.py proves on the CPU that the bounds admit a correct kernel and reject
the seeded wiring defects).  rgbnm_dropout_apply past its grid cap is in tests/test_dropout_kernels.py.

Conventions of tests/test_kernel_edges.py: every output, scratch buffer and workspace is kernel_check.guarded (margins and
unwritten elements are checked bit-wise), inputs are followed by NaN, workspaces have exactly the size the library asks for, the
device kernels are asserted, every element is checked, the worst bound ratio per stage is printed (-s).  Masks are rebuilt from
the seed with tests/dropout_ref.py; the tests assert that they bite.

Worst |err| / bound measured on one MI355X are in DESIGN.md ("Dropout blocks, class head and patch embedding, element-wise").
"""
import ctypes as C
import math

import pytest
import torch

import block_ref as R
import composite_ref as CR
import kernel_check as KC
import step_ends_ref as S
import test_dropout_kernels as TDK
from block_ref import BF16, F32, NTOK
from kernel_check import guarded, launched, ran
from oracle import vit_torch as V
from rgb_no_more_amd import lib as L
from test_block_edges import Case, GENERIC_OFF, GRAD_SHAPES
from test_block_edges import gelu_table  # noqa: F401  (module fixture: the one-launch kernels of the last patch-embedding test need the table)
from test_hip_kernels import option  # noqa: F401  (fixture: set a runtime switch for one test)
from test_step_ends import gvec, nan_tail

pytestmark = pytest.mark.gpu
DEV = "cuda"
EINVAL, EWORKSPACE = -1, -3
WORST = {k: KC.Worst() for k in ("drop-fwd", "drop-bwd", "drop-dw", "head", "patch-embed")}


def collecting(*keys):
    for k in keys:
        WORST[k].errors = []
    return [WORST[k] for k in keys]


def finish(where, keys):
    errs = []
    for k in keys:
        WORST[k].report(f"{k} (so far)")
        errs += WORST[k].errors
        WORST[k].errors = None
    assert not errs, f"{where}: {len(errs)} checks failed:\n" + "\n".join(errs[:12])


def test_the_seed_list_is_the_dropout_kernels():
    assert tuple(TDK.SEEDS) == CR.SEEDS


# ================================================================================================== dropout block, set-up
def count(names, sub):
    return sum(sub in n for n in names)


class DropRun:
    """The blocks of Case c through rgbnm_vit_block_fwd_drop (first to last) and rgbnm_vit_block_bwd_drop (last to first, each on
    the dx the one behind it left); plain: rgbnm_vit_block_fwd / _bwd instead; bracket: the backward inside a
    rgbnm_reduce_hold_begin / _end pair.  Every block has its own scratch, gradients and workspace, all guarded."""

    def __init__(self, c, p, seed, blocks, plain=False, bracket=False, where=""):
        lib, M, E, HID, INNER = L.lib(), c.M, c.e, 4 * c.e, c.inner
        n = len(blocks)
        assert n == c.depth
        self.c, self.p, self.seed, self.blocks, self.where = c, p, seed, blocks, where
        st = TDK.seed_tensor(seed)
        self.acts = acts = c.new_acts()
        bp = [L.BlockParams(*[q[k].data_ptr() for k in ("ln1_g", "ln1_b", "ln2_g", "ln2_b", "bqkv", "bproj", "b1", "b2")],
                            *[t.data_ptr() for k in ("wqkv", "wproj", "w1", "w2") for t in (q[k], q[k + "_t"])]) for q in c.P]
        ba = [L.BlockActs(*[c.act_tensors(acts, i)[k].data_ptr() for k, _ in L.BlockActs._fields_]) for i in range(n)]
        wsb = lib.rgbnm_vit_workspace(C.byref(c.cfg))
        self.sc = [dict(du=guarded(M, HID, c.dt), dxn=guarded(M, E, c.dt), dx_mid=guarded(M, E, c.dt), dattn=guarded(M, INNER, c.dt),
                        dqkv=guarded(M, 3 * INNER, c.dt), ws=guarded(wsb // 4, None, F32), dx=guarded(M, E, c.dt),
                        dy_m=guarded(M, E, c.dt), dxmid_m=guarded(M, E, c.dt)) for _ in range(n)]
        k_ = E // 192
        self.grads = [{k: guarded(sh[0] * k_, sh[1] * k_ if len(sh) > 1 else None, F32) for k, sh in GRAD_SHAPES} for _ in range(n)]
        dr = [L.Dropout(st.data_ptr(), p, blocks[i], self.sc[i]["dy_m"].t.data_ptr(), self.sc[i]["dxmid_m"].t.data_ptr())
              for i in range(n)]

        def fwd():
            for i in range(n):
                if plain:
                    L.check(lib.rgbnm_vit_block_fwd(C.byref(c.cfg), C.byref(bp[i]), C.byref(ba[i]), L.stream()), f"block {i}")
                else:
                    L.check(lib.rgbnm_vit_block_fwd_drop(C.byref(c.cfg), C.byref(bp[i]), C.byref(ba[i]), C.byref(dr[i]), L.stream()),
                            f"block {i}")
        _, self.fwd_names = launched(fwd)
        for i in range(n):
            for k, g in acts[i].items():
                g.check(f"{where} block {i} {k}")
        if bracket:
            table = torch.zeros(lib.rgbnm_reduce_hold_table_bytes(), dtype=torch.uint8, device=DEV)
            table_host = torch.zeros(table.numel(), dtype=torch.uint8)
            L.check(lib.rgbnm_reduce_hold_begin(), "hold_begin")
        self.bwd_names = [None] * n
        try:
            for i in range(n - 1, -1, -1):
                bg = L.BlockGrads(*[self.grads[i][k].t.data_ptr() for k, _ in L.BlockGrads._fields_])
                bs = L.BlockScratch(*[self.sc[i][k].t.data_ptr() for k in ("du", "dxn", "dx_mid", "dattn", "dqkv", "ws")], wsb)
                dy, dx = self.dy_of(i), self.sc[i]["dx"].t
                if plain:
                    call = lambda: lib.rgbnm_vit_block_bwd(C.byref(c.cfg), C.byref(bp[i]), C.byref(ba[i]), C.byref(bg), C.byref(bs),  # noqa: E731
                                                           dy.data_ptr(), dx.data_ptr(), L.stream())
                else:
                    call = lambda: lib.rgbnm_vit_block_bwd_drop(C.byref(c.cfg), C.byref(bp[i]), C.byref(ba[i]), C.byref(bg),   # noqa: E731
                                                                C.byref(bs), C.byref(dr[i]), dy.data_ptr(), dx.data_ptr(), L.stream())
                rc, self.bwd_names[i] = launched(call)
                assert rc == 0, (where, i, rc)
        except BaseException:
            if bracket:
                lib.rgbnm_reduce_hold_cancel()
            raise
        if bracket:
            rc, self.end_names = launched(lambda: lib.rgbnm_reduce_hold_end(table.data_ptr(), table_host.data_ptr(), table.numel(), L.stream()))
            assert rc == 0, (where, "hold_end", rc)
        self.keep = (st, bp, ba, dr)

    def dy_of(self, i):
        return self.c.dy if i == len(self.blocks) - 1 else self.sc[i + 1]["dx"].t

    def check_guards(self, dxn_written, plain=False):
        for i in range(len(self.blocks)):
            w = f"{self.where} bwd block {i}"
            for k, g in self.sc[i].items():
                if (k == "dxn" and not dxn_written) or (plain and k in ("dy_m", "dxmid_m")):
                    assert bool((g.raw == g.canary).all()), f"{w}: {k} was written"
                else:
                    g.check(f"{w} {k}", written=(k != "ws"))
            for k, g in self.grads[i].items():
                g.check(f"{w} {k}")

    def tensors(self, i):
        A = self.c.act_tensors(self.acts, i)
        G = {k: self.sc[i][k].t for k in ("du", "dx_mid", "dattn", "dqkv", "dx", "dy_m", "dxmid_m")}
        G["dy"] = self.dy_of(i)
        return A, G, {k: g.t for k, g in self.grads[i].items()}

    def check(self, fwd_only=False):
        """Every stage of every block against fp64; the masks bite; the inputs reach block_ref's regimes."""
        c = self.c
        wf, wb, wd = collecting("drop-fwd", "drop-bwd", "drop-dw")
        for i, blk in enumerate(self.blocks):
            A, G, W = self.tensors(i)
            f = CR.factors(self.seed, self.p, blk, c.M, c.e, DEV)
            w = f"{self.where} block {i} (index {blk})"
            CR.masks_bite(f, self.p, w)
            info = CR.check_drop_block(wf, wb, wd, w, c.P[i], A, None if fwd_only else G, None if fwd_only else W, c.B, f, self.p)
            CR.regimes(info, c.M, i == 0, w)
            del f, info
        finish(self.where, ("drop-fwd", "drop-bwd", "drop-dw"))

    def same_bits(self, other, what, skip=()):
        for i in range(len(self.blocks)):
            for nm, mine, theirs in (("acts", self.acts[i], other.acts[i]), ("scratch", self.sc[i], other.sc[i]),
                                     ("grads", self.grads[i], other.grads[i])):
                for k in mine:
                    if k in skip or k == "ws":
                        continue
                    assert torch.equal(mine[k].t.view(KC._INT[mine[k].esz]), theirs[k].t.view(KC._INT[mine[k].esz])), \
                        f"{what}: block {i} {nm}.{k} differs"


# ================================================================================================== dropout block, cases
@pytest.mark.parametrize("dtn,B,p,blocks,si", CR.DROP_GENERIC)
def test_dropout_blocks_on_the_generic_kernels(option, dtn, B, p, blocks, si):
    """Every fast option off: the dropout wiring of vit.hip (block_bwd with d) on kernels tests/test_kernel_edges.py and
    tests/test_dropout_kernels.py cover one by one.  Two blocks in sequence (the second one's dx is the first one's dy), the
    counter words of block_index 0 / 1 / 11 and of the four 64-bit seeds."""
    for o in GENERIC_OFF:
        option(o, 0)
    where = f"drop generic {dtn} B={B} p={p} blocks={blocks} seed={CR.SEEDS[si]:#x}"
    r = DropRun(Case(B, 2, images=False, dt=CR.DT[dtn]), p, CR.SEEDS[si], blocks, where=where)
    assert count(r.fwd_names, "gemm_nt_kernel") == 8 and count(r.fwd_names, "ln_fwd_kernel") == 4, sorted(set(r.fwd_names))
    for names in r.bwd_names:
        assert count(names, "dropout_apply_kernel") == 2 and count(names, "gemm_tn_kernel") == 4 and ran(names, "ln_bwd_kernel"), \
            (where, sorted(set(names)))
        assert not ran(names, "mlp_bwd_kernel") and not ran(names, "gemm_tn_pipe") and not ran(names, "kpipe"), sorted(set(names))
    r.check_guards(dxn_written=True)
    r.check()


def test_dropout_block_with_the_fused_layernorm_backward(option):
    """B = 42, bf16, default options: 8232 rows >= 8192, so both LayerNorm backwards run in the epilogue of their GEMM
    (fused_dx_lnbwd) with the UNMASKED residual behind masked operands; the fused FeedForwardBlock kernels must stay out (they read
    one dy as operand and residual), and every forward GEMM that draws a mask is the generic kernel."""
    where = f"drop fused-LN B={CR.DROP_FUSED_B}"
    c = Case(CR.DROP_FUSED_B, 2, images=False)
    assert L.lib().rgbnm_vit_ln_chain(C.byref(c.cfg)) == 1
    r = DropRun(c, 0.1, CR.SEEDS[1], (0, 1), where=where)
    fn = r.fwd_names
    assert not ran(fn, "mlp_fwd_kernel") and not ran(fn, "res_ln"), sorted(set(fn))
    gemms = [n for n in fn if "gemm" in n]
    assert len(gemms) == 8 and count(gemms, "gemm_nt_kernel") >= 6, sorted(set(fn))        # (qkv is free to take a tuned kernel)
    for names in r.bwd_names:
        assert not ran(names, "mlp_bwd_kernel") and not ran(names, "mlp_fwd_kernel"), sorted(set(names))
        assert ran(names, "gemm_nt_kpipe") and not ran(names, "ln_bwd_kernel"), sorted(set(names))
        assert count(names, "dropout_apply_kernel") == 2, sorted(set(names))
    r.check_guards(dxn_written=False)
    r.check()


@pytest.mark.parametrize("wide", [1, 0])
def test_dropout_block_at_e384_groups_its_weight_gradients(option, wide):
    """E = 384, 6 heads, bf16, B = 64: with tn_wide one grouped launch at the END of the block reads dy_m and dxmid_m (they
    must have stayed intact); without it tn_group falls from 2 to 1 and the pairs fc2 + fc1 / proj + qkv run.  tn_group = 1 asked
    for outright only regroups nothing: the same bits."""
    B, e, heads = CR.DROP_E384
    option("tn_wide", wide)
    where = f"drop E={e} B={B} tn_wide={wide}"
    c = Case(B, 1, images=False, e=e, heads=heads)
    r = DropRun(c, 0.1, CR.SEEDS[3], (11,), where=where)
    names = r.bwd_names[0]
    want = {"gemm_tn_wide_kernel": 1, "gemm_tn_pipe_kernel": 0} if wide else {"gemm_tn_wide_kernel": 0, "gemm_tn_pipe_kernel": 2}
    for k, v in dict(want, gemm_tn_kernel=0).items():
        assert count(names, k) == v, (where, k, sorted(set(names)))
    r.check_guards(dxn_written=True)
    r.check()
    if not wide:
        option("tn_group", 1)
        r.same_bits(DropRun(c, 0.1, CR.SEEDS[3], (11,), where=where + " tn_group=1"), where + " tn_group 2 -> 1")


def test_dropout_block_under_every_tn_group_setting(option):
    """E = 192.  B = 16 (3136 rows, a multiple of 64): tn_group 0 / 1 / 2 are four, two and one weight-gradient launch with
    different token splits -- every one within the same bounds.  B = 3 (588 rows, not groupable): the settings change nothing,
    so they must give the same bits."""
    c = Case(CR.DROP_GROUP_B, 1, images=False)
    for group, launches in ((0, 4), (1, 2), (2, 1)):
        option("tn_group", group)
        where = f"drop B={CR.DROP_GROUP_B} tn_group={group}"
        r = DropRun(c, 0.5, CR.SEEDS[2], (0,), where=where)
        assert count(r.bwd_names[0], "gemm_tn") == launches, (where, sorted(set(r.bwd_names[0])))
        r.check_guards(dxn_written=True)
        r.check()
    c = Case(3, 1, images=False)
    runs = []
    for group in (0, 1, 2):
        option("tn_group", group)
        runs.append(DropRun(c, 0.5, CR.SEEDS[2], (0,), where=f"drop B=3 tn_group={group}"))
    for r in runs[1:]:
        runs[0].same_bits(r, "B = 3: tn_group regroups nothing")


@pytest.mark.parametrize("dtn", ["f32", "f16", "bf16"])
def test_dropout_block_at_p0_gives_the_bits_of_the_plain_block(option, dtn):
    for o in GENERIC_OFF:
        option(o, 0)
    c = Case(3, 2, images=False, dt=CR.DT[dtn])
    plain = DropRun(c, 0.0, CR.SEEDS[1], (0, 1), plain=True, where=f"plain {dtn}")
    drop = DropRun(c, 0.0, CR.SEEDS[1], (0, 1), where=f"drop p=0 {dtn}")
    plain.check_guards(dxn_written=True, plain=True)
    drop.check_guards(dxn_written=True)
    drop.same_bits(plain, f"p = 0 {dtn}", skip=("dy_m", "dxmid_m"))
    for i in range(2):                                           # ... and the masked copies are copies
        assert torch.equal(drop.sc[i]["dy_m"].t, drop.dy_of(i)) and torch.equal(drop.sc[i]["dxmid_m"].t, drop.sc[i]["dx_mid"].t)


def test_dropout_block_inside_a_held_bracket_keeps_its_bits():
    """rgbnm_reduce_hold_begin / _end around both backward calls, a workspace per block: the gradients hold nothing until _end,
    then the bits of the unbracketed calls."""
    c = Case(3, 2, images=False)
    base = DropRun(c, 0.1, CR.SEEDS[2], (0, 11), where="unbracketed")
    held = DropRun(c, 0.1, CR.SEEDS[2], (0, 11), bracket=True, where="bracketed")
    assert ran(held.end_names, "reduce_table_kernel"), held.end_names
    held.check_guards(dxn_written=True)
    held.same_bits(base, "held bracket")


def test_dropout_block_refusals_launch_nothing(option):
    """NULL d, NULL dy_m, dy_m == dxmid_m, p = 1 and a workspace one byte short: the error code of include/rgbnm.h, no kernel
    launched, every guarded buffer untouched."""
    lib = L.lib()
    c = Case(1, 1, images=False)
    M, E = c.M, c.e
    acts = c.new_acts()
    p0 = c.P[0]
    bp = L.BlockParams(*[p0[k].data_ptr() for k in ("ln1_g", "ln1_b", "ln2_g", "ln2_b", "bqkv", "bproj", "b1", "b2")],
                       *[t.data_ptr() for k in ("wqkv", "wproj", "w1", "w2") for t in (p0[k], p0[k + "_t"])])
    ba = L.BlockActs(*[c.act_tensors(acts, 0)[k].data_ptr() for k, _ in L.BlockActs._fields_])
    wsb = lib.rgbnm_vit_workspace(C.byref(c.cfg))
    sc = dict(du=guarded(M, 4 * E, BF16), dxn=guarded(M, E, BF16), dx_mid=guarded(M, E, BF16), dattn=guarded(M, E, BF16),
              dqkv=guarded(M, 3 * E, BF16), ws=guarded(wsb // 4, None, F32), dx=guarded(M, E, BF16), dy_m=guarded(M, E, BF16),
              dxmid_m=guarded(M, E, BF16))
    grads = {k: guarded(sh[0], sh[1] if len(sh) > 1 else None, F32) for k, sh in GRAD_SHAPES}
    bg = L.BlockGrads(*[grads[k].t.data_ptr() for k, _ in L.BlockGrads._fields_])
    st = TDK.seed_tensor(7)
    pm, pxm = sc["dy_m"].t.data_ptr(), sc["dxmid_m"].t.data_ptr()

    def scratch(nbytes=wsb):
        return L.BlockScratch(*[sc[k].t.data_ptr() for k in ("du", "dxn", "dx_mid", "dattn", "dqkv", "ws")], nbytes)
    ok = L.Dropout(st.data_ptr(), 0.1, 0, pm, pxm)
    bad = [("NULL dy_m", L.Dropout(st.data_ptr(), 0.1, 0, None, pxm), wsb, EINVAL),
           ("NULL dxmid_m", L.Dropout(st.data_ptr(), 0.1, 0, pm, None), wsb, EINVAL),
           ("dy_m == dxmid_m", L.Dropout(st.data_ptr(), 0.1, 0, pm, pm), wsb, EINVAL),
           ("p = 1", L.Dropout(st.data_ptr(), 1.0, 0, pm, pxm), wsb, EINVAL),
           ("p < 0", L.Dropout(st.data_ptr(), -0.1, 0, pm, pxm), wsb, EINVAL),
           ("NULL seed", L.Dropout(None, 0.1, 0, pm, pxm), wsb, EINVAL),
           ("block -1", L.Dropout(st.data_ptr(), 0.1, -1, pm, pxm), wsb, EINVAL),
           ("workspace one byte short", ok, wsb - 1, EWORKSPACE)]
    bufs = list(acts[0].items()) + list(sc.items()) + list(grads.items())

    def untouched(what):
        torch.cuda.synchronize()
        for k, g in bufs:
            assert bool((g.raw == g.canary).all()), f"{what}: {k} was written"
    for what, d, nbytes, code in bad:
        bs = scratch(nbytes)
        rc, names = launched(lambda: lib.rgbnm_vit_block_bwd_drop(C.byref(c.cfg), C.byref(bp), C.byref(ba), C.byref(bg), C.byref(bs),
                                                                  C.byref(d), c.dy.data_ptr(), sc["dx"].t.data_ptr(), L.stream()))
        assert rc == code and names == [], (what, rc, names)
        if code == EINVAL and "dy_m" not in what and "dxmid_m" not in what:        # the forward takes no masked copies
            rc, names = launched(lambda: lib.rgbnm_vit_block_fwd_drop(C.byref(c.cfg), C.byref(bp), C.byref(ba), C.byref(d), L.stream()))
            assert rc == EINVAL and names == [], (what, "forward", rc, names)
        untouched(what)
    bs = scratch()
    rc, names = launched(lambda: lib.rgbnm_vit_block_bwd_drop(C.byref(c.cfg), C.byref(bp), C.byref(ba), C.byref(bg), C.byref(bs), None,
                                                              c.dy.data_ptr(), sc["dx"].t.data_ptr(), L.stream()))
    assert rc == EINVAL and names == [], ("NULL d", rc, names)
    rc, names = launched(lambda: lib.rgbnm_vit_block_fwd_drop(C.byref(c.cfg), C.byref(bp), C.byref(ba), None, L.stream()))
    assert rc == EINVAL and names == [], ("NULL d forward", rc, names)
    untouched("NULL d")


# ============================================================================================================= class head
class Head:
    def __init__(self, dtn, B, N, E, C_, seed):
        self.dt = dt = CR.DT[dtn]
        self.dtn, self.B, self.N, self.E, self.C = dtn, B, N, E, C_
        P = CR.head_params(E, C_, seed)
        self.P = {k: v.to(DEV).to(dt if k in ("w1", "w2") else F32) for k, v in P.items()}
        self.wt = {k: self.P[k].T.contiguous() for k in ("w1", "w2")}
        x, dl = CR.head_inputs(B, N, E, C_, dt, seed + 20)
        self.x, self.dl = nan_tail(x), nan_tail(dl)
        self.cfg = L.VitCfg(L.dt_of(dt), B, N, E, E // 64, R.EPS, 1.0 / math.sqrt(E))
        q = self.P
        self.hp = L.HeadParams(q["ln_g"].data_ptr(), q["ln_b"].data_ptr(), q["b1"].data_ptr(), q["b2"].data_ptr(), q["w1"].data_ptr(),
                               self.wt["w1"].data_ptr(), q["w2"].data_ptr(), self.wt["w2"].data_ptr(), C_, 0)
        self.where = f"head {dtn} B={B} N={N} E={E} C={C_}"

    def ws_bytes(self, kind):
        """'apart': rgbnm_head_bwd_workspace; 'shared': the largest of the three producers' regions (they run one after another)."""
        lib, B, E, C_ = L.lib(), self.B, self.E, self.C
        full = lib.rgbnm_head_bwd_workspace(C.byref(self.cfg), C_)
        if kind == "apart":
            return full
        small = max(lib.rgbnm_gemm_tn_workspace(B, C_, E), lib.rgbnm_gemm_tn_workspace(B, E, E), B * 2 * E * 4)
        assert small < full and not CR.head_ws_split(B, E, C_, small, lib.rgbnm_gemm_tn_workspace)[0]
        return small

    def forward(self):
        B, N, E, dt = self.B, self.N, self.E, self.dt
        self.a = dict(mean=gvec(B * N, F32), rstd=gvec(B * N, F32), pooled=guarded(B, E, dt), h1=guarded(B, E, dt),
                      logits=guarded(B, self.C, F32))
        a = self.a
        self.ha = L.HeadActs(self.x.data_ptr(), a["mean"].t.data_ptr(), a["rstd"].t.data_ptr(), a["pooled"].t.data_ptr(),
                             a["h1"].t.data_ptr(), a["logits"].t.data_ptr())
        rc, names = launched(lambda: L.lib().rgbnm_head_fwd(C.byref(self.cfg), C.byref(self.hp), C.byref(self.ha), L.stream()))
        assert rc == 0, (self.where, rc)
        for k, g in a.items():
            g.check(f"{self.where} {k}")
        return names

    def new_bwd(self, ws_kind):
        B, N, E, dt, C_ = self.B, self.N, self.E, self.dt, self.C
        g = dict(dln_g=gvec(E, F32), dln_b=gvec(E, F32), dw1=guarded(E, E, F32), db1=gvec(E, F32), dw2=guarded(C_, E, F32),
                 db2=gvec(C_, F32), da=guarded(B, E, dt), dpooled=guarded(B, E, dt), dx=guarded(B * N, E, dt))
        wsb = self.ws_bytes(ws_kind)
        g["ws"] = guarded(cdiv4(wsb), None, F32)
        hg = L.HeadGrads(*[g[k].t.data_ptr() for k, _ in L.HeadGrads._fields_])
        return g, hg, wsb

    def backward(self, ws_kind, g=None):
        g, hg, wsb = self.new_bwd(ws_kind) if g is None else g
        rc, names = launched(lambda: L.lib().rgbnm_head_bwd(C.byref(self.cfg), C.byref(self.hp), C.byref(self.ha), C.byref(hg),
                                                            self.dl.data_ptr(), g["da"].t.data_ptr(), g["dpooled"].t.data_ptr(),
                                                            g["dx"].t.data_ptr(), g["ws"].t.data_ptr(), wsb, L.stream()))
        return rc, names, g

    def act_t(self):
        return {k: v.t for k, v in self.a.items()}


def cdiv4(nbytes):
    assert nbytes % 4 == 0
    return nbytes // 4


@pytest.mark.parametrize("dtn,B,N,E,C_,ws_kind,group", CR.HEAD_CASES)
def test_class_head_edges(option, dtn, B, N, E, C_, ws_kind, group):
    """rgbnm_head_fwd and rgbnm_head_bwd stage by stage: both sides of gemm_nt_small's M <= 512, C = 1000 and 40, the two token
    counts, the three producers of split sums side by side or in one shared region, the two weight-gradient GEMMs grouped or
    not."""
    option("tn_group", group)
    h = Head(dtn, B, N, E, C_, 3000 + 17 * B + E)
    (worst,) = collecting("head")
    names = h.forward()
    kern = CR.head_nt_kernel(dtn, B)
    other = "gemm_nt_kernel" if kern == "gemm_nt_small_kernel" else "gemm_nt_small_kernel"
    assert ran(names, "pool_fwd_kernel") and count(names, kern) == 2 and not ran(names, other), (h.where, sorted(set(names)))
    CR.check_head_fwd(worst, h.where, h.P, h.x, h.act_t(), h.dt)
    rc, names, g = h.backward(ws_kind)
    where = f"{h.where} ws={ws_kind} tn_group={group}"
    assert rc == 0, (where, rc)
    assert ran(names, "pool_bwd_kernel") and count(names, kern) == 2 and not ran(names, other), (where, sorted(set(names)))
    grouped = dtn == "bf16" and ws_kind == "apart" and group and B % 64 == 0
    assert count(names, "gemm_tn") == (1 if grouped else 2), (where, sorted(set(names)))
    for k, t in g.items():
        t.check(f"{where} {k}", written=(k != "ws"))
    CR.check_head_bwd(worst, where, h.P, h.x, h.act_t(), h.dl, {k: v.t for k, v in g.items()}, h.dt)
    finish(where, ("head",))


@pytest.mark.parametrize("dtn,B", [("bf16", 256), ("f32", 3)])
def test_class_head_inside_a_held_bracket(dtn, B):
    """With rgbnm_head_bwd_workspace bytes: the bits of the unbracketed call, once _end has run.  With less, the three producers
    would share one region whose first partial sums the later ones overwrite before _end reads them: RGBNM_EWORKSPACE, nothing
    launched (include/rgbnm.h)."""
    lib = L.lib()
    h = Head(dtn, B, NTOK, 192, 1000, 4100 + B)
    h.forward()
    rc, _, base = h.backward("apart")
    assert rc == 0
    table = torch.zeros(lib.rgbnm_reduce_hold_table_bytes(), dtype=torch.uint8, device=DEV)
    table_host = torch.zeros(table.numel(), dtype=torch.uint8)
    small = h.new_bwd("shared")
    L.check(lib.rgbnm_reduce_hold_begin(), "hold_begin")
    try:
        rc, names, g = h.backward("shared", small)
        assert rc == EWORKSPACE and names == [], (rc, names)
        torch.cuda.synchronize()
        for k, t in g.items():
            assert bool((t.raw == t.canary).all()), f"refused head backward wrote {k}"
        rc, names, held = h.backward("apart")
        assert rc == 0 and not ran(names, "reduce_multi_kernel"), (rc, sorted(set(names)))
    except BaseException:
        lib.rgbnm_reduce_hold_cancel()
        raise
    rc, names = launched(lambda: lib.rgbnm_reduce_hold_end(table.data_ptr(), table_host.data_ptr(), table.numel(), L.stream()))
    assert rc == 0 and ran(names, "reduce_table_kernel"), (rc, names)
    for k, t in held.items():
        t.check(f"held head {k}", written=(k != "ws"))
        if k != "ws":
            assert torch.equal(t.raw, base[k].raw), f"held head backward: {k} differs"
    # the same small workspace outside a bracket is the documented in-place mode
    rc, names, g = h.backward("shared", small)
    assert rc == 0
    for k in ("dw1", "db1", "dw2", "db2", "dln_g", "dln_b", "dx"):
        g[k].check(f"shared, unbracketed {k}")


def test_class_head_refusals_launch_nothing():
    """NULL arguments: RGBNM_EINVAL.  A head width that is not a whole number of 16-byte rows of dlogits (C % 8 in the 16-bit
    modes, C % 4 in fp32) is outside rgbnm_head_bwd's contract: RGBNM_EINVAL (the forward takes any C)."""
    lib = L.lib()
    h = Head("bf16", 3, NTOK, 192, 40, 4300)
    h.forward()
    g, hg, wsb = h.new_bwd("apart")
    full = [C.byref(h.cfg), C.byref(h.hp), C.byref(h.ha), C.byref(hg), h.dl.data_ptr(), g["da"].t.data_ptr(), g["dpooled"].t.data_ptr(),
            g["dx"].t.data_ptr(), g["ws"].t.data_ptr(), wsb, L.stream()]
    for i in list(range(8)) + [8]:
        args = list(full)
        args[i] = None
        rc, names = launched(lambda: lib.rgbnm_head_bwd(*args))
        assert rc == EINVAL and names == [], (i, rc, names)
    a2 = {k: (gvec(v.rows, v.dtype) if v.cols is None else guarded(v.rows, v.cols, v.dtype)) for k, v in h.a.items()}
    ha2 = L.HeadActs(h.x.data_ptr(), *[a2[k].t.data_ptr() for k in ("mean", "rstd", "pooled", "h1", "logits")])
    for args in ((None, C.byref(h.hp), C.byref(ha2)), (C.byref(h.cfg), None, C.byref(ha2)), (C.byref(h.cfg), C.byref(h.hp), None)):
        rc, names = launched(lambda: lib.rgbnm_head_fwd(*args, L.stream()))
        assert rc == EINVAL and names == [], (rc, names)
    for dtn, C_ in (("bf16", 1004), ("f16", 44), ("f32", 42)):
        hh = Head(dtn, 3, NTOK, 192, C_, 4400)
        hh.forward()                                            # accepted: C is only the logits' width there
        g2, hg2, wsb2 = hh.new_bwd("apart")
        rc, names, _ = hh.backward("apart", (g2, hg2, wsb2))
        assert rc == EINVAL and names == [], (dtn, C_, rc, names)
        g.update({f"{dtn}.{k}": v for k, v in g2.items()})
    torch.cuda.synchronize()
    for k, t in list(g.items()) + list(a2.items()):
        assert bool((t.raw == t.canary).all()), f"refused head call wrote {k}"


# ======================================================================================================== patch embedding
class PatchEmbed:
    def __init__(self, TI, TO, B, seed, E=192):
        Hb, Wb = CR.PE_GRID
        self.TI, self.TO, self.B, self.E, self.N, self.Hb, self.Wb = TI, TO, B, E, (Hb // 2) * (Wb // 2), Hb, Wb
        self.M = B * self.N
        self.A = nan_tail(V.conv_matrix(16).contiguous())
        y, c = S.embed_inputs(B, Hb, Wb, TI, "dct" if seed % 2 else "normal", seed)
        self.y, self.cb = nan_tail(y), nan_tail(c)
        P = CR.pe_params(E, self.N, seed + 3)
        self.P = {k: nan_tail(v.to(TO) if k == "wpe" else v) for k, v in P.items()}
        self.cfg = L.VitCfg(L.dt_of(TO), B, self.N, E, E // 64, R.EPS, 1.0 / math.sqrt(E))
        self.where = f"patch_embed {S.NAMES[TI]}->{S.NAMES[TO]} B={B}"

    def forward(self, lam=None, mix_entry=False):
        lib, q = L.lib(), self.P
        feat, x0 = guarded(self.M, 384, self.TO), guarded(self.M, self.E, self.TO)
        tail = (self.A.data_ptr(), q["wpe"].data_ptr(), q["bpe"].data_ptr(), q["pos"].data_ptr(), feat.t.data_ptr(), x0.t.data_ptr(),
                self.Hb, self.Wb, L.stream())
        head = (C.byref(self.cfg), L.dt_of(self.TI), self.y.data_ptr(), self.cb.data_ptr())
        if mix_entry:
            rc, names = launched(lambda: lib.rgbnm_patch_embed_fwd_mix(*head, L.ptr(lam), *tail))
        else:
            rc, names = launched(lambda: lib.rgbnm_patch_embed_fwd(*head, *tail))
        assert rc == 0, (self.where, rc)
        feat.check(self.where + " feat")
        x0.check(self.where + " x0")
        return feat, x0, names


@pytest.mark.parametrize("TI,TO", S.EMBED_BIG_PAIRS, ids=lambda t: S.NAMES[t])
@pytest.mark.parametrize("B", CR.PE_B)
def test_patch_embedding_edges(B, TI, TO):
    """rgbnm_patch_embed_fwd, _fwd_mix (device lambda; NULL lambda = the bits of _fwd) and _bwd.  The position table's rows differ
    by several units: a wrong period or row offset behind the sub-block kernel is hundreds of bounds away.  B = 42: the 8232-row
    EPI_POS call stays on the generic kernel (the row-panel and weight-resident kernels take no position table:
    gemm.hip launch_nt_sel, `!p.pos`)."""
    pe = PatchEmbed(TI, TO, B, 5000 + 10 * B)
    (worst,) = collecting("patch-embed")
    feat, x0, names = pe.forward()
    assert ran(names, "subblock_embed_kernel") and count(names, "gemm_nt_kernel") == 1 and len(names) == 2, (pe.where, names)
    CR.check_pe_fwd(worst, pe.where, feat.t, x0.t, pe.y, pe.cb, pe.A, None, pe.P, TI, TO, pe.N)
    f2, x2, _ = pe.forward(None, mix_entry=True)
    assert torch.equal(f2.raw, feat.raw) and torch.equal(x2.raw, x0.raw), pe.where + ": _fwd_mix with a NULL lambda"
    lam = S.lam_pair(5100 + B)
    fm, xm, names = pe.forward(nan_tail(lam), mix_entry=True)
    assert ran(names, "subblock_embed_kernel") and count(names, "gemm_nt_kernel") == 1, (pe.where, names)
    CR.check_pe_fwd(worst, pe.where + " mixed", fm.t, xm.t, pe.y, pe.cb, pe.A, lam, pe.P, TI, TO, pe.N)
    # backward: dW = dx0^T feat, db = column sums of dx0
    dx0 = nan_tail((S.randn((pe.M, pe.E), 5200 + B)).to(TO))
    wsb = L.lib().rgbnm_gemm_tn_workspace(pe.M, pe.E, 384)
    dw, db, ws = guarded(pe.E, 384, F32), gvec(pe.E, F32), guarded(wsb // 4, None, F32)
    rc, names = launched(lambda: L.lib().rgbnm_patch_embed_bwd(C.byref(pe.cfg), dx0.data_ptr(), feat.t.data_ptr(), dw.t.data_ptr(),
                                                               db.t.data_ptr(), ws.t.data_ptr(), wsb, L.stream()))
    assert rc == 0 and ran(names, "gemm_tn"), (pe.where, rc, names)
    for g, nm in ((dw, "dwpe"), (db, "dbpe")):
        g.check(f"{pe.where} {nm}")
    ws.check(pe.where + " workspace", written=False)
    R.check_pe_dw(worst, pe.where, dx0, feat.t, dw.t, db.t, B)
    finish(pe.where, ("patch-embed",))


def test_patch_embedding_backward_is_the_pe_job_of_the_grouped_launch():
    """B = 3 (588 rows: no grouped pipelined launch, so rgbnm_vit_blocks_bwd_dw_pe runs its jobs one by one): the patch embedding's
    job there and rgbnm_patch_embed_bwd split the token axis alike and must give the same bits; both are inside check_pe_dw."""
    c = Case(3, 1)
    acts = c.run_fwd()
    bw, dattn = c.run_bwd(acts)
    _, (feat, pe_dw, pe_db), names = c.run_dw(acts, bw, dattn, pe=True)
    assert not ran(names, "gemm_tn_pipe_kernel")
    lib = L.lib()
    wsb = lib.rgbnm_vit_workspace(C.byref(c.cfg))                 # the workspace size run_dw gave the job
    dw, db, ws = guarded(192, 384, F32), gvec(192, F32), guarded(wsb // 4, None, F32)
    L.check(lib.rgbnm_patch_embed_bwd(C.byref(c.cfg), bw[0]["dx"].t.data_ptr(), feat.data_ptr(), dw.t.data_ptr(), db.t.data_ptr(),
                                      ws.t.data_ptr(), wsb, L.stream()), "patch_embed_bwd")
    torch.cuda.synchronize()
    dw.check("patch_embed_bwd dw")
    db.check("patch_embed_bwd db")
    assert torch.equal(dw.t, pe_dw) and torch.equal(db.t, pe_db)
    (worst,) = collecting("patch-embed")
    R.check_pe_dw(worst, "patch_embed_bwd B=3", bw[0]["dx"].t, feat, dw.t, db.t, 3)
    finish("patch_embed_bwd vs pe job", ("patch-embed",))


def test_patch_embedding_refusals_launch_nothing():
    lib = L.lib()
    pe = PatchEmbed(F32, F32, 1, 5300)
    q = pe.P
    feat, x0 = guarded(pe.M, 384, F32), guarded(pe.M, pe.E, F32)

    def fwd(cfg, Hb, Wb, mix):
        tail = (pe.A.data_ptr(), q["wpe"].data_ptr(), q["bpe"].data_ptr(), q["pos"].data_ptr(), feat.t.data_ptr(), x0.t.data_ptr(),
                Hb, Wb, L.stream())
        if mix:
            return lib.rgbnm_patch_embed_fwd_mix(cfg, 0, pe.y.data_ptr(), pe.cb.data_ptr(), None, *tail)
        return lib.rgbnm_patch_embed_fwd(cfg, 0, pe.y.data_ptr(), pe.cb.data_ptr(), *tail)
    for mix in (False, True):
        for cfg, Hb, Wb in ((None, 28, 28), (C.byref(pe.cfg), 28, 26), (C.byref(pe.cfg), 26, 28), (C.byref(pe.cfg), 14, 14)):
            rc, names = launched(lambda: fwd(cfg, Hb, Wb, mix))
            assert rc == EINVAL and names == [], (mix, Hb, Wb, rc, names)
    dw, db, ws = guarded(pe.E, 384, F32), gvec(pe.E, F32), gvec(1024, F32)
    rc, names = launched(lambda: lib.rgbnm_patch_embed_bwd(None, x0.t.data_ptr(), feat.t.data_ptr(), dw.t.data_ptr(), db.t.data_ptr(),
                                                           ws.t.data_ptr(), 4096, L.stream()))
    assert rc == EINVAL and names == [], (rc, names)
    torch.cuda.synchronize()
    for k, g in (("feat", feat), ("x0", x0), ("dw", dw), ("db", db), ("ws", ws)):
        assert bool((g.raw == g.canary).all()), f"refused patch-embedding call wrote {k}"
