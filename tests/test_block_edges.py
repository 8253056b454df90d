"""Element-wise tests of everything that computes an encoder BLOCK, at the C ABI (include/rgbnm.h), against the stage-local
fp64 references and bounds of tests/block_ref.py (read its docstring first; tests/test_block_edges_cpu.py proves on the CPU that
the bounds admit a correct kernel and reject the seeded defects).

Conventions of tests/test_kernel_edges.py: every output and scratch buffer is kernel_check.guarded (margins and unwritten
elements are checked bit-wise), the residual stream and dy are followed by NaN rows, workspaces have exactly the size the library
asks for, the device kernels are asserted, every element is checked, the worst bound ratio per (path, stage) is printed (-s).
Chain images are built here from arbitrary weights with chain.block_index / block_index_bwd and rgbnm_chain_gather (the layout's
definition; tests/test_chain_fwd.py pins the prep kernel to it).  Inputs come from block_ref's CPU generators: the CPU file asserts
the regimes on the very same tensors.

Measured on one MI355X (worst |err| / bound over all cases, one-launch | per-operation; the bounds are derived, none is fitted):
    xn1, xn2 0.50 | 0.50   mean, rstd 0.03 | 0.01   qkv 0.50 | 0.50   attn 0.40 | 0.51   lse 0.55 | 0.58   x_mid, x_out 0.50 | 0.50
    gl 0.50 | 0.50   u 0.49 | 0.49   du 0.50 | 0.50   dx_mid 0.54 | 0.51   dattn 0.50 | 0.50   dq 0.32 | 0.33   dk 0.22 | 0.35
    dv 0.35 | 0.29   dx 0.53 | 0.50   dxn - | 0.50   part2, part1 0.25   dln 0.17 | 0.07   dW 0.015 | 0.003   db 0.013 | 0.004
    pe_dw 0.03   pe_db 0.01                              (dxn exists on the generic paths only; the fused forms keep it in LDS)
The 31 tests take 62 s there ("Encoder blocks, element-wise", says which cases cost it and why they stay).
Two later cases run block_ref.make_params(offset=+-1) -- every logit and lse at +-148 scaled units -- with the same stage checks plus
block_ref.logit_err: the one-launch forward + backward at B = 2 and the per-operation path at B = 42 (0.09 s and 0.20 s; attention
output 0.34, lse 0.05, dq 0.27, dk 0.22, dv 0.27 of their bounds; DESIGN.md, "Value regimes").
"""
import ctypes as C

import numpy as np
import pytest
import torch

import block_ref as R
import kernel_check as KC
from block_ref import BF16, F32, E, HEADS, HID, INNER, NTOK
from kernel_check import guarded, nan_padded, launched, ran
from rgb_no_more_amd import chain
from rgb_no_more_amd import lib as L
from test_hip_kernels import option  # noqa: F401  (fixture: set a runtime switch for one test)

pytestmark = pytest.mark.gpu
DEV = "cuda"
EINVAL = -1
ACT_SHAPES = (("xn1", E, BF16), ("mean1", None, F32), ("rstd1", None, F32), ("qkv", 3 * INNER, BF16), ("lse", None, F32),
              ("attn", INNER, BF16), ("x_mid", E, BF16), ("xn2", E, BF16), ("mean2", None, F32), ("rstd2", None, F32),
              ("u", HID, BF16), ("gl", HID, BF16), ("x_out", E, BF16))
GRAD_SHAPES = (("dln1_g", (E,)), ("dln1_b", (E,)), ("dln2_g", (E,)), ("dln2_b", (E,)), ("dwqkv", (3 * INNER, E)),
               ("dbqkv", (3 * INNER,)), ("dwproj", (E, INNER)), ("dbproj", (E,)), ("dw1", (HID, E)), ("db1", (HID,)),
               ("dw2", (E, HID)), ("db2", (E,)))


def cu_count():
    return torch.cuda.get_device_properties(0).multi_processor_count


def cfg_of(B, dtype=L.DT_BF16, N=NTOK, e=E, heads=HEADS):
    return L.VitCfg(dtype, B, N, e, heads, R.EPS, R.SCALE)


@pytest.fixture(scope="module", autouse=True)
def gelu_table():
    L.check(L.lib().rgbnm_gelu_table_init(L.stream()), "gelu_table_init")


# ------------------------------------------------------------------------------------------------------------ case set-up
class Case:
    """Parameters, chain images and inputs of one (B, depth) on the device; everything the kernels write is guarded."""

    def __init__(self, B, depth, seed=1, images=True, dt=BF16, e=E, heads=HEADS, offset=None):
        self.B, self.depth, self.M, self.dt, self.e, self.inner, self.heads = B, depth, B * NTOK, dt, e, heads * 64, heads
        wk = ("wqkv", "wproj", "w1", "w2")
        self.P = [{k: v.to(DEV).to(dt if k in wk else F32) for k, v in p.items()} for p in R.make_params(depth, seed, e, heads, offset)]
        self.x0 = nan_padded(R.make_x0(B, seed, e).to(DEV).to(dt), extra_rows=8)
        self.dy = nan_padded(R.make_dy(B, seed, e).to(DEV).to(dt), extra_rows=8)
        self.cfg = L.VitCfg(L.dt_of(dt), B, NTOK, e, heads, R.EPS, 1.0 / e ** 0.5)
        for p in self.P:
            for k in ("wqkv", "wproj", "w1", "w2"):
                p[k + "_t"] = p[k].T.contiguous()
        if not images:
            return
        # operand shadows of every block side by side, [N, K] and transposed: the source of rgbnm_chain_gather
        parts, idx_f, idx_b, off = [], [], [], 0
        for p in self.P:
            o = {}
            for k in ("wqkv", "wproj", "w1", "w2"):
                o[k], o[k + "_t"] = off, off + p[k].numel()
                parts += [p[k].reshape(-1), p[k + "_t"].reshape(-1)]
                off += 2 * p[k].numel()
            idx_f.append(chain.block_index(o["wqkv"], o["wproj"], o["w1"], o["w2"]))
            idx_b.append(chain.block_index_bwd(o["wqkv_t"], o["wproj_t"], o["w1_t"], o["w2_t"]))
        shadow = torch.cat(parts)
        assert off < 2 ** 31 and chain.BLOCK_ELEMS == L.lib().rgbnm_chain_image_elems()
        self.img, self.img_bwd = (self._gather(shadow, np.concatenate(t)) for t in (idx_f, idx_b))

    @staticmethod
    def _gather(shadow, idx):
        g = guarded(idx.size, None, BF16)
        it = torch.from_numpy(idx.astype(np.int32)).to(DEV)
        L.check(L.lib().rgbnm_chain_gather(shadow.data_ptr(), it.data_ptr(), g.t.data_ptr(), idx.size, L.stream()), "chain_gather")
        torch.cuda.synchronize()
        g.check("chain image")
        assert torch.equal(g.t, shadow[it.long()])
        return g

    def new_acts(self):
        M, B, s = self.M, self.B, self.e // E                  # (ACT_SHAPES are those of E = 192, 3 heads: inner = E, hidden = 4 E)
        return [{k: guarded(M, c * s, self.dt) if c else guarded(B * self.heads * NTOK if k == "lse" else M, None, F32)
                 for k, c, _ in ACT_SHAPES} for _ in range(self.depth)]

    def fwd_table(self, acts, depth=None):
        depth = self.depth if depth is None else depth
        blocks = (L.ChainBlock * depth)()
        for i in range(depth):
            p, a = self.P[i % self.depth], acts[i % self.depth]
            blocks[i] = L.ChainBlock(self.img.t.data_ptr() + (i % self.depth) * chain.BLOCK_ELEMS * 2,
                                     *[p[k].data_ptr() for k in ("ln1_g", "ln1_b", "ln2_g", "ln2_b", "bqkv", "bproj", "b1", "b2")],
                                     *[a[k].t.data_ptr() for k, _, _ in ACT_SHAPES])
        return blocks

    def run_fwd(self):
        acts = self.new_acts()
        blocks = self.fwd_table(acts)
        rc, names = launched(lambda: L.lib().rgbnm_vit_chain_fwd(C.byref(self.cfg), blocks, self.depth, self.x0.data_ptr(), L.stream()))
        assert rc == 0, rc
        assert names == ["vit_chain_fwd_kernel"] or (len(names) == 1 and "vit_chain_fwd_kernel" in names[0]), names
        for i, a in enumerate(acts):
            for k, g in a.items():
                g.check(f"chain fwd B={self.B} depth={self.depth} block {i} {k}")
        return acts

    def act_tensors(self, acts, i):
        A = {k: g.t for k, g in acts[i].items()}
        A["x_in"] = self.x0 if i == 0 else acts[i - 1]["x_out"].t
        return A

    def new_bwd(self):
        M, B = self.M, self.B
        return [dict(du=guarded(M, HID, BF16), dx_mid=guarded(M, E, BF16), dqkv=guarded(M, 3 * INNER, BF16), dx=guarded(M, E, BF16),
                     part2=guarded(B * 2 * E, None, F32), part1=guarded(B * 2 * E, None, F32)) for _ in range(self.depth)]

    def dy_of(self, bw, i):
        return self.dy if i == self.depth - 1 else bw[i + 1]["dx"].t

    def bwd_table(self, acts, bw, depth=None):
        depth = self.depth if depth is None else depth
        blocks = (L.ChainBwdBlock * depth)()
        for j in range(depth):
            i = j % self.depth
            p, A, g = self.P[i], self.act_tensors(acts, i), bw[i]
            blocks[j] = L.ChainBwdBlock(self.img_bwd.t.data_ptr() + i * chain.BLOCK_ELEMS * 2, p["ln1_g"].data_ptr(), p["ln2_g"].data_ptr(),
                                        *[A[k].data_ptr() for k in ("x_in", "mean1", "rstd1", "qkv", "lse", "attn", "x_mid", "mean2",
                                                                    "rstd2", "u")],
                                        self.dy_of(bw, i).data_ptr(),
                                        *[g[k].t.data_ptr() for k in ("du", "dx_mid", "dqkv", "dx", "part2", "part1")])
        return blocks

    def run_bwd(self, acts):
        bw = self.new_bwd()
        dattn = guarded(self.M, INNER, BF16)
        blocks = self.bwd_table(acts, bw)
        rc, names = launched(lambda: L.lib().rgbnm_vit_chain_bwd(C.byref(self.cfg), blocks, self.depth, dattn.t.data_ptr(), L.stream()))
        assert rc == 0, rc
        assert len(names) == 1 and "vit_chain_bwd_kernel" in names[0], names
        dattn.check(f"chain bwd B={self.B} depth={self.depth} dattn scratch")
        for i, g in enumerate(bw):
            for k, t in g.items():
                t.check(f"chain bwd B={self.B} depth={self.depth} block {i} {k}")
        return bw, dattn

    def bwd_tensors(self, bw, dattn, i):
        G = {k: g.t for k, g in bw[i].items()}
        G["part2"], G["part1"] = G["part2"].view(self.B, 2, E), G["part1"].view(self.B, 2, E)
        G["dy"] = self.dy_of(bw, i)
        G["dattn"] = dattn.t if i == 0 else None          # one scratch for all blocks: block 0 ran last
        return G

    def run_dw(self, acts, bw, dattn, pe=False, single=False):
        """rgbnm_vit_blocks_bwd_dw[_pe] over all blocks of the case (last block first, as the model calls it); single (depth 1):
        rgbnm_vit_block_bwd_dw, the one-block entry."""
        lib, n, order = L.lib(), self.depth, list(range(self.depth - 1, -1, -1))
        wsb = lib.rgbnm_vit_workspace(C.byref(self.cfg))
        grads = [{k: guarded(s[0], s[1] if len(s) > 1 else None, F32) for k, s in GRAD_SHAPES} for _ in range(n)]
        wss = [guarded(wsb // 4, None, F32) for _ in range(n)]
        dxn = guarded(self.M, E, BF16)
        keep = []
        As = [L.BlockActs(*[self.act_tensors(acts, i)[k].data_ptr() for k, _ in L.BlockActs._fields_]) for i in order]
        Gs = [L.BlockGrads(*[grads[i][k].t.data_ptr() for k, _ in L.BlockGrads._fields_]) for i in order]
        Ss = [L.BlockScratch(bw[i]["du"].t.data_ptr(), dxn.t.data_ptr(), bw[i]["dx_mid"].t.data_ptr(), dattn.t.data_ptr(),
                             bw[i]["dqkv"].t.data_ptr(), wss[i].t.data_ptr(), wsb) for i in order]
        keep += [As, Gs, Ss]
        pa = (C.POINTER(L.BlockActs) * n)(*[C.pointer(x) for x in As])
        pg = (C.POINTER(L.BlockGrads) * n)(*[C.pointer(x) for x in Gs])
        ps = (C.POINTER(L.BlockScratch) * n)(*[C.pointer(x) for x in Ss])
        pdy = (C.c_void_p * n)(*[self.dy_of(bw, i).data_ptr() for i in order])
        p2 = (C.c_void_p * n)(*[bw[i]["part2"].t.data_ptr() for i in order])
        p1 = (C.c_void_p * n)(*[bw[i]["part1"].t.data_ptr() for i in order])
        where = f"blocks_bwd_dw B={self.B} n={n} pe={int(pe)}"
        if pe:
            feat = nan_padded(R.make_feat(self.B).to(DEV), extra_rows=8)
            pe_dw, pe_db, pe_ws = guarded(E, 384, F32), guarded(E, None, F32), guarded(wsb // 4, None, F32)
            rc, names = launched(lambda: lib.rgbnm_vit_blocks_bwd_dw_pe(
                C.byref(self.cfg), n, pa, pg, ps, pdy, p2, p1, bw[0]["dx"].t.data_ptr(), feat.data_ptr(), pe_dw.t.data_ptr(),
                pe_db.t.data_ptr(), pe_ws.t.data_ptr(), wsb, L.stream()))
        elif single:
            assert n == 1
            rc, names = launched(lambda: lib.rgbnm_vit_block_bwd_dw(C.byref(self.cfg), C.byref(As[0]), C.byref(Gs[0]), C.byref(Ss[0]),
                                                                    pdy[0], p2[0], p1[0], L.stream()))
        else:
            rc, names = launched(lambda: lib.rgbnm_vit_blocks_bwd_dw(C.byref(self.cfg), n, pa, pg, ps, pdy, p2, p1, L.stream()))
        assert rc == 0, (where, rc)
        # the grouped pipelined launch takes token counts that are multiples of 64 (B % 16 == 0); the others run job by job
        grouped = self.M % 64 == 0
        assert ran(names, "gemm_tn_pipe_kernel") == grouped and ran(names, "gemm_tn_kernel") != grouped, (where, sorted(set(names)))
        if grouped:
            assert sum("gemm_tn_pipe_kernel" in x for x in names) == 1, (where, names)
        dxn.check(where + " dxn (not this call's)", written=False)
        assert bool((dxn.raw == dxn.canary).all())
        for i in range(n):
            wss[i].check(f"{where} workspace {i}", written=False)
            for k, g in grads[i].items():
                g.check(f"{where} block {i} {k}")
        out = [{k: g.t for k, g in grads[i].items()} for i in range(n)]
        if pe:
            for g, nm in ((pe_dw, "pe_dw"), (pe_db, "pe_db")):
                g.check(f"{where} {nm}")
            pe_ws.check(where + " pe workspace", written=False)
            return out, (feat, pe_dw.t, pe_db.t), names
        return out, None, names


WORST = {k: KC.Worst() for k in ("chain-fwd", "chain-bwd", "chain-dw", "perop-fwd", "perop-bwd", "perop-dw")}


def collecting(*keys):
    """The Worst collectors of `keys` with an empty error list each: a case checks every stage, then fails with all of them."""
    for k in keys:
        WORST[k].errors = []
    return [WORST[k] for k in keys]


def finish(where, keys, soft=()):
    errs = list(soft)
    for k in keys:
        WORST[k].report(f"{k} (so far)")
        errs += WORST[k].errors
    assert not errs, f"{where}: {len(errs)} checks failed:\n" + "\n".join(errs[:12])


def table_regimes(pre):
    """(negative tail, window, positive tail) populations of the fc1 pre-activations, from the table's own ends."""
    win = (C.c_int * 16)()
    L.check(L.lib().rgbnm_gelu_table_info(win, None))
    valid, A0, P1, N1 = list(win)[:4]
    assert valid == 1
    bits = pre.to(BF16).view(torch.int16).to(torch.int32) & 0xFFFF
    mag, neg = bits & 0x7FFF, bits >= 0x8000
    return (int((neg & (mag >= N1)).sum()), int(((mag >= A0) & (mag < torch.where(neg, N1, P1))).sum()),
            int((~neg & (mag >= P1)).sum()))


# ------------------------------------------------------------------------------------- one-launch forward, backward, dW
@pytest.mark.parametrize("b,depth", R.CHAIN_CASES)
def test_chain_forward_backward_and_weight_gradients(option, b, depth):
    """vit_chain_fwd_kernel -> vit_chain_bwd_kernel -> the grouped weight-gradient launch (n = depth blocks: the token axis is
    split 256 / (21 n) ways; with the patch-embedding job; tn_direct both ways), every stage of every block from what the run
    stored.  B = CU count and CU count + 1: one workgroup per CU, and one image left for a second round."""
    B = R.resolve_b(b, cu_count())
    c = Case(B, depth)
    where = f"chain B={B} depth={depth}"
    wf, wb, wd = collecting("chain-fwd", "chain-bwd", "chain-dw")
    soft = []
    acts = c.run_fwd()
    for i in range(depth):
        info = R.check_block_fwd(wf, f"{where} block {i}", c.P[i], c.act_tensors(acts, i), B)
        lo, mid, hi = table_regimes(info["pre"])
        if not (lo >= 4 * c.M and hi >= 4 * c.M and mid > info["pre"].numel() // 2):
            soft.append(f"{where} block {i}: table regimes (negative tail, window, positive tail) = {(lo, mid, hi)}")
        if info["onehot_rows"] < c.M // 10 or (i == 0 and info["rstd1_max"] <= 0.8 * R.EPS ** -0.5):
            soft.append(f"{where} block {i}: one-hot rows {info['onehot_rows']}, max rstd1 {info['rstd1_max']:.4g}")
        del info
    bw, dattn = c.run_bwd(acts)
    for i in range(depth):
        if i < depth - 1:
            assert c.dy_of(bw, i).data_ptr() == bw[i + 1]["dx"].t.data_ptr()          # blk[i].dy == blk[i + 1].dx
        R.check_block_bwd(wb, f"{where} block {i}", c.P[i], c.act_tensors(acts, i), c.bwd_tensors(bw, dattn, i), B)
    variants = [(1, False, False), (0, False, False), (1, True, False), (0, True, False)] + ([(1, False, True)] if depth == 1 else [])
    for direct, pe, single in variants:
        option("tn_direct", direct)
        W, pex, names = c.run_dw(acts, bw, dattn, pe, single)
        for i in range(depth):
            R.check_block_dw(wd, f"{where} tn_direct={direct} pe={int(pe)} single={int(single)} block {i}", c.act_tensors(acts, i),
                             c.bwd_tensors(bw, dattn, i), W[i], B)
        if pex:
            R.check_pe_dw(wd, f"{where} tn_direct={direct}", bw[0]["dx"].t, pex[0], pex[1], pex[2], B)
        del W, pex
    finish(where, ("chain-fwd", "chain-bwd", "chain-dw"), soft)


def test_chain_forward_backward_with_a_logit_offset():
    """B = 2, depth 1 with make_params(offset=+1): q[:, 0] = 32 and k[:, 0] = 64 in every head, so every logit and lse of the
    one-launch forward carries +148 scaled units (exp of it overflows fp32 without the max subtraction) and the backward rebuilds P
    from an lse of that size.  The stage checks of the case above plus block_ref.logit_err."""
    B = 2
    c = Case(B, 1, offset=1)
    where = f"chain B={B} depth=1 offset=+1"
    wf, wb = collecting("chain-fwd", "chain-bwd")
    acts = c.run_fwd()
    info = R.check_block_fwd(wf, f"{where} block 0", c.P[0], c.act_tensors(acts, 0), B, logit=True)
    soft = [] if info["lse_absmin"] >= 70 and info["onehot_rows"] >= c.M // 10 else [
        f"{where}: min |lse| {info['lse_absmin']:.4g}, one-hot rows {info['onehot_rows']}"]
    del info
    bw, dattn = c.run_bwd(acts)
    R.check_block_bwd(wb, f"{where} block 0", c.P[0], c.act_tensors(acts, 0), c.bwd_tensors(bw, dattn, 0), B, logit=True)
    finish(where, ("chain-fwd", "chain-bwd"), soft)


def test_chain_backward_twice_gives_the_same_bits():
    c = Case(cu_count() + 1, 2)
    acts = c.run_fwd()
    a, da = c.run_bwd(acts)
    b, db = c.run_bwd(acts)
    for i in range(2):
        for k in a[i]:
            assert torch.equal(a[i][k].raw, b[i][k].raw), (i, k)
    assert torch.equal(da.raw, db.raw)


# ------------------------------------------------------------------------------------------- per-operation fused path
def table_kernel(names):
    return any("mlp_fwd_kernel" in n and ("<true>" in n or "<(bool)1>" in n) for n in names)


def per_operation(c, where, fused, tn_kernels=None, logit=False):
    """rgbnm_vit_block_fwd_chain (block 0 with a next block, block 1 without -- its LN1 comes out of block 0's fc2 epilogue when
    rgbnm_vit_ln_chain says so) and rgbnm_vit_block_bwd over the two blocks of Case c; every stage of both from what the run
    stored, residual epilogues with the `inter` term of the per-operation kernels.  fused: the E = 192 row-panel kernels with
    the LayerNorm epilogues and the fused FeedForwardBlock are expected (True), must not run (False), or neither (None)."""
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
    if fused is not None:
        expect(ran(names, "mlp_fwd_kernel") == fused and ran(names, "gemm_nt_kpipe") == fused, "forward kernels", names)
    if fused:
        expect(table_kernel(names) == R.mlp_fwd_panel_rows(B * NTOK)[1], "table / arithmetic GELU kernel", names)
        expect(sum("ln_fwd_kernel" in n for n in names) == 1, "block 0's LN1 only: every other LayerNorm is fused", names)
    else:
        expect(sum("ln_fwd_kernel" in n for n in names) == 4 and ran(names, "gemm_nt"), "generic forward kernels", names)
    for i in range(2):
        for k, g in acts[i].items():
            g.check(f"{where} block {i} {k}")
        info = R.check_block_fwd(wf, f"{where} block {i}", c.P[i], c.act_tensors(acts, i), B, inter=True, logit=logit)
        if logit and info["lse_absmin"] < 70:
            soft.append(f"{where} block {i}: min |lse| {info['lse_absmin']:.4g}, no logit offset")
        lo, mid, hi = table_regimes(info["pre"])
        if not (lo >= 4 * c.M and hi >= 4 * c.M and mid > info["pre"].numel() // 2):
            soft.append(f"{where} block {i}: table regimes {(lo, mid, hi)}")
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
        if fused is not None:
            expect(ran(names, "mlp_bwd_kernel") == fused and ran(names, "gemm_nt_kpipe") == fused, "fused backward kernels", names)
        expect(ran(names, "ln_bwd_kernel") == (not fused), "LayerNorm backward kernel", names)
        for kn, cnt in (tn_kernels or {}).items():           # name -> launches per block backward (None: at least one)
            got = sum(kn in x for x in names)
            expect(got >= 1 if cnt is None else got == cnt, f"weight-gradient kernel {kn}: {got} launches, expected {cnt}", names)
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
        if not fused:                                     # the generic path's last dxn: dqkv . Wqkv rounded to bf16 (gemm_nt, no epilogue)
            ref, mag = G["dqkv"].double() @ c.P[i]["wqkv"].double(), G["dqkv"].double().abs() @ c.P[i]["wqkv"].double().abs()
            R._chk(wb, "dxn", sc["dxn"].t, ref, mag, 3 * INNER * KC.U, w, B=B)
        dy = sc["dx"].t
        del r2, r1
    finish(where, ("perop-fwd", "perop-bwd", "perop-dw"), soft)


@pytest.mark.parametrize("B,dmast", [(b, None) for b in R.PEROP_B] + [(42, 0), (42, 1)])
def test_per_operation_blocks_at_their_launchers_edges(option, B, dmast):
    """The fused per-operation path (bf16, E = 192) at the batches of block_ref.PEROP_B; mlp_dmast both ways at B = 42."""
    if dmast is not None:
        option("mlp_dmast", dmast)
    per_operation(Case(B, 2, images=False), f"per-operation B={B}" + ("" if dmast is None else f" mlp_dmast={dmast}"),
                  B * NTOK >= 8192)


def test_per_operation_blocks_with_a_logit_offset(option):
    """The fused per-operation path at its first eligible batch (B = 42, bf16) with make_params(offset=-1): every logit carries -148
    scaled units, where exp of the unshifted logit is zero in fp32; attention v2 forward and backward inside the block."""
    per_operation(Case(42, 2, images=False, offset=-1), "per-operation B=42 offset=-1", True, logit=True)


GENERIC_OFF = ("nt_small", "nt_kpipe", "nt_wres", "nt_staged", "ln_fuse", "tn_pipe", "tn_group", "tn_direct", "tn_wide", "attn_v2",
               "attn_persist", "mlp_fuse", "mlp_bwd", "gelu_table")


@pytest.mark.parametrize("dt", [F32, torch.float16, BF16])
def test_composite_wiring_on_the_generic_kernels(option, dt):
    """Every fast option off: the composites' own wiring -- workspace regions, reduction flush, the dW-qkv row permutation -- on
    kernels that tests/test_kernel_edges.py already covers, in the three element types (B = 3: 588 rows)."""
    for o in GENERIC_OFF:
        option(o, 0)
    per_operation(Case(3, 2, images=False, dt=dt), f"generic {dt} B=3", False,
                  tn_kernels={"gemm_tn_kernel": 4, "gemm_tn_pipe_kernel": 0, "gemm_tn_wide_kernel": 0})


@pytest.mark.parametrize("wide", [1, 0])
def test_composite_wiring_at_e384(option, wide):
    """E = 384, 6 heads, bf16, B = 64 (12544 rows, a multiple of 64).  vit.hip block_bwd: with tn_wide the block's four
    weight-gradient GEMMs are ONE launch of 192 x 384 tiles; without it tn_group falls from 2 to 1 at E > 192 and they run as
    the pairs fc2 + fc1 / proj + qkv, two launches of the pipelined kernel.  The generic kernel runs in neither."""
    option("tn_wide", wide)
    kern = {"gemm_tn_wide_kernel": 1, "gemm_tn_pipe_kernel": 0} if wide else {"gemm_tn_wide_kernel": 0, "gemm_tn_pipe_kernel": 2}
    per_operation(Case(64, 2, images=False, e=384, heads=6), f"E=384 B=64 tn_wide={wide}", None,
                  tn_kernels=dict(kern, gemm_tn_kernel=0))


# -------------------------------------------------------------------------------------------------------------- refusals
def _untouched(bufs, where):
    torch.cuda.synchronize()
    for k, g in bufs:
        assert bool((g.raw == g.canary).all()), f"{where}: {k} was written"


def test_chain_entries_refuse_what_they_do_not_cover_and_touch_nothing():
    """include/rgbnm.h: depth 13, fp32, E 384 and N 197 return 1 (the caller runs the blocks one by one); a NULL argument returns
    RGBNM_EINVAL; either way no kernel is launched and no buffer is written."""
    lib = L.lib()
    c = Case(2, 1)
    acts, bw = c.new_acts(), c.new_bwd()
    dattn = guarded(c.M, INNER, BF16)
    bufs = [(f"acts.{k}", g) for k, g in acts[0].items()] + [(f"bwd.{k}", g) for k, g in bw[0].items()] + [("dattn", dattn)]
    full_acts = [{k: torch.zeros_like(g.t) for k, g in acts[0].items()}]          # what a backward would read (never reached)

    class Z:
        def __init__(self, t):
            self.t = t
    facts = [{k: Z(t) for k, t in full_acts[0].items()}]
    cases = [("depth 13", c.cfg, 13), ("fp32", cfg_of(2, L.DT_F32), 1), ("E 384", cfg_of(2, e=384, heads=6), 1),
             ("N 197", cfg_of(2, N=197), 1), ("2 heads", cfg_of(2, heads=2), 1)]
    for what, cfg, depth in cases:
        ft, bt = c.fwd_table(acts, depth), c.bwd_table(facts, bw, depth)
        rc, names = launched(lambda: lib.rgbnm_vit_chain_fwd(C.byref(cfg), ft, depth, c.x0.data_ptr(), L.stream()))
        assert rc == 1 and names == [], (what, rc, names)
        rc, names = launched(lambda: lib.rgbnm_vit_chain_bwd(C.byref(cfg), bt, depth, dattn.t.data_ptr(), L.stream()))
        assert rc == 1 and names == [], (what, rc, names)
        _untouched(bufs, what)
    ft, bt = c.fwd_table(acts), c.bwd_table(facts, bw)
    nulls = [lambda: lib.rgbnm_vit_chain_fwd(None, ft, 1, c.x0.data_ptr(), L.stream()),
             lambda: lib.rgbnm_vit_chain_fwd(C.byref(c.cfg), None, 1, c.x0.data_ptr(), L.stream()),
             lambda: lib.rgbnm_vit_chain_fwd(C.byref(c.cfg), ft, 1, None, L.stream()),
             lambda: lib.rgbnm_vit_chain_fwd(C.byref(c.cfg), ft, 0, c.x0.data_ptr(), L.stream()),
             lambda: lib.rgbnm_vit_chain_bwd(None, bt, 1, dattn.t.data_ptr(), L.stream()),
             lambda: lib.rgbnm_vit_chain_bwd(C.byref(c.cfg), None, 1, dattn.t.data_ptr(), L.stream()),
             lambda: lib.rgbnm_vit_chain_bwd(C.byref(c.cfg), bt, 1, None, L.stream()),
             lambda: lib.rgbnm_vit_chain_bwd(C.byref(c.cfg), bt, 0, dattn.t.data_ptr(), L.stream())]
    for i, fn in enumerate(nulls):
        rc, names = launched(fn)
        assert rc == EINVAL and names == [], (i, rc, names)
    _untouched(bufs, "NULL arguments")
