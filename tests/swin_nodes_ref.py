"""fp64 stage references, per-element bounds and graph-walking helpers for SwinV2's autograd nodes (rgb_no_more_amd/swinv2.py:
_LinearFn, _MlpFn, _LNFn, _WinAttnFn, _MergeFn, _MeanFn, _CpbFn, _QkvBiasFn).  A plain module, imported by name from
tests/test_swin_nodes.py (GPU) and tests/test_swin_nodes_cpu.py; the conventions are those of tests/block_ref.py.

Design: a run is turned into a RECORD -- one dict per node with the tensors it saved, the gradients it received and the
gradients it returned -- and check_record() compares every tensor of the record with the fp64 result of that ONE stage applied to
the tensors the same run stored upstream:  |got - ref| <= ulp_T(ref) + k u mag + named terms  (kernel_check.check_bound).
The stage structure is oracle/swin_torch's (block, window_attention, patch_merge, swin_forward).

Where a record comes from:
- on the GPU, from the autograd graph itself (topology() walks next_functions from logits.grad_fn and asserts the wiring;
  observe() reads each node's saved_tensors / ctx attributes and hooks each node for the gradients it receives and returns);
- on the CPU, from Engine: the whole model, forward and hand-written backward, stage by stage.  With T = float64 it IS the
  composition of the stage references (tests/test_swin_nodes_cpu.py holds it to oracle/swin_torch and its autograd gradients at
  1e-12); with T = bf16 / fp16 / fp32 it rounds where the nodes store or stage (fp32 statistics, weight gradients and parameter
  sums; T activations; the staged `inter` roundings; the row-paired views and the fold of the [2N, 2K] product) and accepts seeded
  defects.

Every forward tensor is the saved input of its consumer (qkv, out, lse: _WinAttnFn; g, gp, x: _MlpFn; x, mean, rstd, sscale: _LNFn;
x: _LinearFn).  Saved by nobody: the last LayerNorm output of a stage -- recovered by inverting the merge permutation (the
reference's neighbour order) on the reduction Linear's saved x, which is exact and is also what checks the merge order -- and the
output of the final norm, checked through the pooled tensor the head saves.

Bounds reuse the terms of tests/test_kernel_edges.py (nt_case: K u mag, `inter`, the GELU terms; tn: (M + 2) u mag; ln_case: LN_C),
tests/test_swin_edges.py (WIN_C, CPB_C, ETA and their error terms in tests/swin_ref.py, EMBED_C) and tests/block_ref.py (du):
- paired Linear: the reference is x W^T + b on [M, N]; the zero blocks of diag(W, W) add exact zeros, K stays the layer's own.
  The fold dW[:N, :K] + dW[N:, K:] adds one fp32 rounding: + ulp_fp32(ref); each half sums M / 2 tokens, together (M + 2) u mag.
- _MlpFn: du = T(T(dy W2) gp) is not stored; dx, dW1 and db1 are referenced to the fp64 du and its rounding
  delta = ulp_T(du) + N u mag + ulp_T(dy W2) |gp| (16-bit: `inter`) is propagated linearly: delta |W1| (dx), delta^T |x| (dW1),
  sum delta (db1).
- position bias: tests/test_swin_edges.py folds the sigmoid's arithmetic into the fitted CPB_C (0.13 x 4 u bias), which its inputs
  allow: there the table error E_t dominates.  With the model's parameters (|t| ~ 0.01, E_t ~ 0) the three fp32 roundings of
  16 / (1 + expf(-t)) are all there is, and 0.52 u bias does not hold them (measured on the MI355X: 1.53 u bias at bias = 7.96
  against ulp + 0.52 u = 1.52).  Added as a derived term at weight 1: (2 (1 - s) + 1) u bias (cpb64, S_bias).
- final norm through the pooled tensor: mean over tokens of the LayerNorm bound (ulp_T(y) + LN_C.y E u ymag) + N u mean|y|.
"""
import math

import torch

import block_ref as BR
import kernel_check as KC
import swin_ref as R
from block_ref import _cb, d64, gelu64, dgelu64
from kernel_check import U, ulp
from oracle import swin_torch as ST

F32, BF16, F16, F64 = torch.float32, torch.bfloat16, torch.float16, torch.float64
WS = 8
LN100 = math.log(100.0)
LN_C = BR.LN_C
# tests/test_swin_edges.py (measured there on the kernels, NOT refitted here)
WIN_C = {
    F32: {"out": 0.12, "lse": 0.16, "dq": 0.16, "dk": 0.14, "dv": 0.28, "dbias": 1.8, "dscale": 0.0018},
    BF16: {"out": 0.78, "lse": 0.84, "dq": 0.92, "dk": 0.84, "dv": 1.0, "dbias": 1.2, "dscale": 0.027},
    F16: {"out": 0.68, "lse": 0.77, "dq": 0.88, "dk": 0.84, "dv": 0.96, "dbias": 1.7, "dscale": 0.027},
}
CPB_C = {"bias": 0.13, "dw2": 0.16, "db1": 0.017, "dw1": 0.017}
ETA = {F32: 2.0 ** -126, BF16: 2.0 ** -126, F16: 2.0 ** -25}
ESZ = {F32: 4, BF16: 2, F16: 2}

# the cases of tests/test_swin_nodes.py: (img_size, depths, heads, B)
SMALL = dict(img=64, depths=(2, 2), heads=(3, 6), B=2)
# B = 4, not 2: gemm_nt_kpipe needs 8192 rows (stage 1's paired fc2: 16384 / 2) and gemm_nt_wres 4096 at K = 192
FOUR = dict(img=256, depths=(2, 2, 2, 2), heads=(3, 6, 12, 24), B=4)
DROP = dict(img=64, depths=(2, 2), heads=(3, 6), B=8)


# =================================================================================================== parameters and inputs
def make_params(depths, heads, n_classes=1000):
    """oracle.swin_torch.fill_params (q_bias / v_bias non-zero, LayerNorm gammas of order 1) with head 1 of block 1's
    logit_scale put on the clamp (ln 100 + 0.3).  {name: fp32 tensor}."""
    shapes = ST.param_shapes(depths, heads, n_classes=n_classes)
    sd = {k: torch.from_numpy(v).clone() for k, v in ST.fill_params(shapes).items()}
    sd["layers.0.blocks.1.attn.logit_scale"][1] = LN100 + 0.3
    return sd


def make_inputs(img, B):
    from rgb_no_more_amd import detfill
    nb = img // 8
    y = torch.from_numpy(detfill.normalish((B, 1, nb, nb, 8, 8), 171))
    c = torch.from_numpy(detfill.normalish((B, 2, nb // 2, nb // 2, 8, 8), 172))
    tgt = detfill.uniform((B, 1000), 173, 0.0, 1.0)
    return y, c, torch.from_numpy(tgt / tgt.sum(1, keepdims=True))


def block_list(depths, heads, img, embed=96):
    """[(prefix, stage, C, res, heads, shift)] in model order: shift 0 on even blocks, 4 on odd, 0 where the grid is the window."""
    out, C, res = [], embed, img // 4
    for li, (d, h) in enumerate(zip(depths, heads)):
        for bi in range(d):
            out.append((f"layers.{li}.blocks.{bi}.", li, C, res, h, 0 if (bi % 2 == 0 or res <= WS) else WS // 2))
        C, res = 2 * C, res // 2
    return out


def is_paired(N, K):
    """swinv2.py _flatten: widths that are multiples of 96 but not both of 192, up to 384."""
    return N % 96 == 0 and K % 96 == 0 and (N % 192 != 0 or K % 192 != 0) and max(N, K) <= 384


# ========================================================================================================= fp64 stages
def merge_ref(x, B, res, C):
    xr = x.reshape(B, res, res, C)
    return torch.cat([xr[:, 0::2, 0::2], xr[:, 1::2, 0::2], xr[:, 0::2, 1::2], xr[:, 1::2, 1::2]], -1).reshape(-1, 4 * C)


def scatter_ref(y, B, res, C, order=(0, 1, 2, 3)):
    """merge_ref's inverse (order: which quarter of the 4 C columns feeds the reference's neighbours 0..3)."""
    y4 = y.reshape(B, res // 2, res // 2, 4 * C)
    q = [y4[..., i * C:(i + 1) * C] for i in order]
    z = torch.empty(B, res, res, C, dtype=y.dtype, device=y.device)
    z[:, 0::2, 0::2], z[:, 1::2, 0::2], z[:, 0::2, 1::2], z[:, 1::2, 1::2] = q
    return z.reshape(B * res * res, C)


def ln64(x, g, b, res=None, sc=None):
    """y = [res +] [sc *] LN(x); dict(y, ymag, mean, rstd, meanmag, xh).  sc: [M, 1] fp64 or None."""
    r = BR.ln_fwd(x, g, b)
    y, m = r["y"], r["ymag"]
    if sc is not None:
        y, m = y * sc, m * sc
    if res is not None:
        y, m = y + res, m + res.abs()
    r["y"], r["ymag"] = y, m
    return r


def ln_bwd64(dy, x, mean, rstd, g, sc=None):
    """tests/test_kernel_edges.py ln_case's backward on the saved statistics: dict(dx, dxmag, dg, dgmag, db, dbmag)."""
    mu, rs = mean[:, None], rstd[:, None]
    xh = (x - mu) * rs
    d = dy if sc is None else dy * sc
    gv = d * g
    dx = rs * (gv - gv.mean(1, keepdim=True) - xh * (gv * xh).mean(1, keepdim=True))
    mag = rs * (gv.abs() + gv.abs().mean(1, keepdim=True) + xh.abs() * (gv * xh).abs().mean(1, keepdim=True))
    return dict(dx=dx, dxmag=mag, dg=(d * xh).sum(0), dgmag=(d * xh).abs().sum(0), db=d.sum(0), dbmag=d.abs().sum(0))


def row_scale(ss, rps, M):
    """s_b of every row: sscale[row // rows_per_sample], [M, 1] fp64 (None without DropPath)."""
    if ss is None:
        return None
    return d64(ss)[torch.arange(M, device=ss.device) // rps][:, None]


def _unheads(t):
    """[n, H, 64, 32] -> [n, 64, H 32]"""
    return t.permute(0, 2, 1, 3).reshape(t.shape[0], 64, -1)


def win64(qkv, bias, scale, B, res, heads, shift, dt, dout=None, out_k=None, lse_k=None, roll=None):
    """Window attention in fp64 from token-major qkv [B res^2, 3 C] (swin_ref.win_fwd / win_bwd on all windows), with the error
    terms for element type dt.  Forward: out, E_out [B res^2, C] token-major, lse, E_lse [windows, heads, 64].  With dout (and the
    run's own out / lse): dqkv, E_dqkv [B res^2, 3 C], dbias, E_dbias, absdS [heads, 64, 64], dscale, E_dscale, mdsp [heads].
    roll: the shift the tokens are rolled by (default: shift; the engine's seeded defect rolls the other way)."""
    C = heads * 32
    roll = shift if roll is None else roll
    uT = KC.U_OF[dt] if dt in KC.U_OF else 0.0
    uP = 0.0 if dt in (F32, F64) else uT
    eta = ETA.get(dt, 0.0)
    xw = R.partition(qkv, B, res, roll)
    q, k, v = (R.split_heads(xw[..., i * C:(i + 1) * C], heads) for i in range(3))
    mask = R.window_mask(res, shift, B, qkv.device)
    Lg, o, lse, P, E_out, E_lse = R.win_fwd(q, k, v, bias, scale, mask, uT, uP, eta)
    r = dict(out=R.reverse(_unheads(o), B, res, roll), E_out=R.reverse(_unheads(E_out), B, res, roll), lse=lse, E_lse=E_lse)
    if dout is None:
        return r
    del P, E_out, o
    dO = R.split_heads(R.partition(dout, B, res, roll), heads)
    O_k = R.split_heads(R.partition(out_k, B, res, roll), heads)
    b = R.win_bwd(Lg, v, dO, O_k, lse_k.reshape(lse.shape), uT, uP, eta)
    cat = lambda a, bb, c: R.reverse(torch.cat([_unheads(a), _unheads(bb), _unheads(c)], -1), B, res, roll)    # noqa: E731
    r.update(dqkv=cat(b["dq"], b["dk"], b["dv"]), E_dqkv=cat(b["E_dq"], b["E_dk"], b["E_dv"]),
             dbias=b["dS"].sum(0), E_dbias=b["E_dS"].sum(0), absdS=b["absdS"].sum(0),
             dscale=b["dsp"].sum(0), E_dscale=b["E_dsp"].sum(0), mdsp=b["mdsp"].sum(0))
    return r


def cpb64(w1, b1, w2, ls, dbias=None, dscale=None):
    """Position bias [h, 64, 64] and logit scale [h] of one block in fp64 with the error terms of tests/test_swin_edges.py
    cpb_case; with dbias [h, 64, 64] / dscale [h]: dw1, db1, dw2, dls and theirs."""
    h = w2.shape[0]
    tab = ST.coords_table(8).double().reshape(-1, 2).to(w1.device)
    pidx = ST.position_index(8).reshape(-1).to(w1.device)
    ls = ls.reshape(-1)
    pre = tab @ w1.T + b1
    Hm = tab.abs() @ w1.abs().T + b1.abs()
    hid = pre.clamp_min(0)
    t = hid @ w2.T
    E_t = 18 * U * (Hm @ w2.abs().T)
    sg = torch.sigmoid(t)
    d1 = 16 * sg * (1 - sg)
    sc = torch.exp(ls.clamp(max=LN100))
    # S_bias: the sigmoid's own arithmetic, 16.f / (1.f + expf(-t)) (csrc/swin.hip cpb_bias_kernel) -- expf to 1 ulp = 2 u of
    # e = exp(-t), which reaches the quotient with weight e / (1 + e) = 1 - s, and the fp32 add: (2 (1 - s) + 1) u bias (the divide's
    # rounding is the bound's ulp term).  Derived, at weight 1; see the module docstring.
    r = dict(bias=(16 * sg)[pidx].T.reshape(h, 64, 64), E_bias=(d1 * E_t + 4 * U * 16 * sg)[pidx].T.reshape(h, 64, 64), scale=sc,
             E_scale=4 * U * sc, S_bias=((3 - 2 * sg) * U * 16 * sg)[pidx].T.reshape(h, 64, 64))
    if dbias is None:
        return r
    dbias = dbias.reshape(h, 4096)
    Gs = torch.zeros(225, h, dtype=F64, device=w1.device).index_add_(0, pidx, dbias.T)
    Gm = torch.zeros(225, h, dtype=F64, device=w1.device).index_add_(0, pidx, dbias.abs().T)
    dt_ = d1 * Gs
    E_dt = d1 * 64 * U * Gm + Gs.abs() * (d1 * (1 - 2 * sg)).abs() * E_t + 4 * U * dt_.abs()
    dh = dt_ @ w2
    E_dh = E_dt @ w2.abs() + 24 * U * (dt_.abs() @ w2.abs())
    on = (pre > 0).double()
    inside = ls <= LN100
    dls = torch.where(inside, dscale.reshape(-1) * torch.exp(ls), torch.zeros_like(ls))
    r.update(dw2=dt_.T @ hid, E_dw2=E_dt.T @ hid + dt_.abs().T @ (2 * U * Hm) + 40 * U * (dt_.abs().T @ hid),
             db1=(dh * on).sum(0), E_db1=(E_dh * on).sum(0) + 40 * U * (dh.abs() * on).sum(0),
             dw1=(dh * on).T @ tab, E_dw1=(E_dh * on).T @ tab.abs() + 40 * U * ((dh.abs() * on).T @ tab.abs()),
             dls=dls, E_dls=4 * U * dls.abs(), inside=inside)
    return r


# ====================================================================================================== the record's checks
class Worst(KC.Worst):
    """kernel_check.Worst that collects violations (block_ref._cb) so that a case reports every stage before it fails."""

    def __init__(self):
        super().__init__()
        self.errors = []

    def same(self, key, a, b, where):
        """bit for bit (NaN-free tensors: +0 and -0 differ)"""
        ok = a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(bits(a), bits(b)))
        self(key, 0.0 if ok else math.inf)
        if not ok:
            self.errors.append(f"{where}: not bit-identical")

    def ok(self):
        return not self.errors and all(v <= 1.0 for v in self.d.values())


def bits(t):
    t = t.detach().contiguous()
    return t.view({1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def _inter(pre, dt):
    return ulp(pre, dt) if dt in (BF16, F16) else None


def check_lin_fwd(w, key, where, x, W, b, y):
    """y = T(x W^T + b), tests/test_kernel_edges.py nt_case E_NONE: ulp_T + K u mag."""
    ref, mag = BR.linear(d64(x), d64(W), None if b is None else d64(b))
    _cb(w, key, y, ref, mag, y.dtype, 1, x.shape[1] * U, f"{where} {key}", tile=(128, 192))


def check_lin_bwd(w, key, where, n, bracket=False):
    dy, x, W = d64(n["dy"]), d64(n["x"]), d64(n["W"])
    dt = n["x"].dtype
    M, N = dy.shape
    if n["dx"] is not None:
        pre, mag = dy @ W, dy.abs() @ W.abs()
        extra = None
        if n["dxs"] is not None:
            extra = _inter(pre, dt)
            pre, mag = pre + d64(n["dxs"]), mag + d64(n["dxs"]).abs()
        _cb(w, key + "-dx", n["dx"], pre, mag, dt, 1, N * U, f"{where} {key} dx", extra=extra, tile=(128, 192))
    if not bracket:
        check_tn(w, key + "-dW", f"{where} {key}", dy, x, n["dW"], n["db"], n["pair"])


def check_tn(w, key, where, dy, x, dW, db, pair, pW=None, pb=None):
    """dW = dy^T x, db = column sums (fp64 operands): (M + 2) u mag; the paired fold: + one fp32 rounding.  pW / pb: propagated
    operand error (the _MlpFn du)."""
    M = dy.shape[0]
    ref, mag, rb, mb = BR.tn(dy, x)
    fold = (lambda r: ulp(r, F32)) if pair else (lambda r: 0.0)
    _cb(w, key, dW, ref, mag, F32, 1, (M + 2) * U, where + " dW", extra=fold(ref) + (pW if pW is not None else 0.0), tile=(128, 192))
    if db is not None:
        _cb(w, key.replace("dW", "db"), db, rb, mb, F32, 1, (M + 2) * U, where + " db", extra=fold(rb) + (pb if pb is not None else 0.0))


def check_mlp_fwd(w, where, n, y):
    x, W1, b1 = d64(n["x"]), d64(n["W1"]), d64(n["b1"])
    dt = n["x"].dtype
    pre, mag = BR.linear(x, W1, b1)
    assert float(pre.abs().min()) >= BR.DENORMAL_FREE, f"{where}: a pre-activation below 2^-120 (the GELU table's exception)"
    up, K = ulp(pre, dt), x.shape[1]
    ref, ref2 = gelu64(pre), dgelu64(pre)
    _cb(w, "g", n["g"], ref, 1.13 * mag, dt, 1, K * U, where + " g", extra=1.13 * up + 2.0 ** -22 * pre.abs() + 2 * ulp(ref, F32),
        tile=(128, 192))
    _cb(w, "gp", n["gp"], ref2, 0.8 * mag, dt, 1, K * U, where + " gp", extra=0.8 * up + 2.0 ** -21 + 2 * ulp(ref2, F32),
        tile=(128, 192))
    check_lin_fwd(w, "fc2", where, n["g"], n["W2"], n["b2"], y)


def check_mlp_bwd(w, where, n, bracket=False):
    dy, x, g, gp = d64(n["dy"]), d64(n["x"]), d64(n["g"]), d64(n["gp"])
    W1, W2 = d64(n["W1"]), d64(n["W2"])
    dt = n["x"].dtype
    M, N = dy.shape
    pre, mag = dy @ W2, dy.abs() @ W2.abs()
    du = pre * gp
    delta = ulp(du, dt) + N * U * mag * gp.abs()
    if dt in (BF16, F16):
        delta = delta + ulp(pre, dt) * gp.abs()
    del pre, mag
    ref, rmag = du @ W1, du.abs() @ W1.abs()
    extra = delta @ W1.abs()
    if n["dxs"] is not None:
        it = _inter(ref, dt)
        extra = extra + (it if it is not None else 0.0)
        ref, rmag = ref + d64(n["dxs"]), rmag + d64(n["dxs"]).abs()
    _cb(w, "mlp-dx", n["dx"], ref, rmag, dt, 1, du.shape[1] * U, where + " mlp dx", extra=extra, tile=(128, 192))
    if not bracket:
        check_tn(w, "fc2-dW", where + " fc2", dy, g, n["dW2"], n["db2"], n["p2"])
        check_tn(w, "fc1-dW", where + " fc1", du, x, n["dW1"], n["db1"], n["p1"], pW=delta.T @ x.abs(), pb=delta.sum(0))


def check_ln_fwd(w, key, where, n, res, y):
    """y = T(res + s_b LN(x)) with ln_case's terms; mean / rstd as there.  y None: statistics only."""
    x = d64(n["x"])
    M, E = x.shape
    sc = row_scale(n["ss"], n["rps"], M)
    r = ln64(x, d64(n["gamma"]), d64(n["beta"]), None if res is None else d64(res), sc)
    if y is not None:
        _cb(w, key, y, r["y"], r["ymag"], y.dtype, 1, LN_C["y"] * E * U, f"{where} {key} y", tile=(16, E))
    _cb(w, key + "-stat", n["mean"], r["mean"], r["meanmag"], F32, 1, LN_C["stat"] * E * U, f"{where} {key} mean")
    _cb(w, key + "-stat", n["rstd"], r["rstd"], r["rstd"], F32, 1, LN_C["stat"] * E * U, f"{where} {key} rstd")
    return r


def check_ln_bwd(w, key, where, n, bracket=False):
    x = d64(n["x"])
    M, E = x.shape
    sc = row_scale(n["ss"], n["rps"], M)
    r = ln_bwd64(d64(n["dy"]), x, d64(n["mean"]), d64(n["rstd"]), d64(n["gamma"]), sc)
    _cb(w, key + "-dx", n["dx"], r["dx"], r["dxmag"], n["x"].dtype, 1, LN_C["dx"] * E * U, f"{where} {key} dx", tile=(16, E))
    if not bracket:
        _cb(w, key + "-dgamma", n["dg"], r["dg"], r["dgmag"], F32, 1, (M + E) * U, f"{where} {key} dgamma")
        _cb(w, key + "-dbeta", n["dbeta"], r["db"], r["dbmag"], F32, 1, (M + E) * U, f"{where} {key} dbeta")
    if n["has_res"]:
        w.same(key + "-dres", n["dres"], n["dy"].contiguous(), f"{where} {key} dres")
    else:
        assert n["dres"] is None, f"{where} {key}: a residual gradient without a residual"


def check_attn(w, where, n, cus=256, bracket=False):
    """_WinAttnFn forward and backward: swin_ref.win_fwd / win_bwd with WIN_C, as tests/test_swin_edges.py win_check."""
    B, res, C, heads, shift = n["geo"]
    dt = n["qkv"].dtype
    cw = WIN_C[dt]
    r = win64(d64(n["qkv"]), d64(n["bias"]), d64(n["scale"]), B, res, heads, shift, dt, d64(n["dout"]), d64(n["out"]), d64(n["lse"]))
    _cb(w, "attn-out", n["out"], r["out"], r["E_out"], dt, 1, cw["out"], where + " attn out")
    _cb(w, "attn-lse", n["lse"].reshape(r["lse"].shape), r["lse"], r["E_lse"], F32, 1, cw["lse"], where + " attn lse")
    for i, nm in enumerate(("dq", "dk", "dv")):
        s = slice(i * C, (i + 1) * C)
        _cb(w, "attn-" + nm, n["dqkv"][:, s], r["dqkv"][:, s], r["E_dqkv"][:, s], dt, 1, cw[nm], f"{where} attn {nm}")
    if bracket:
        return
    gb = R.geometry(ESZ[dt], "bwd", B, res, heads, cus)
    S = gb["slots"] * gb["waves"]
    _cb(w, "attn-dbias", n["dbias"], r["dbias"], r["E_dbias"] + (gb["wpw_max"] + S) * U * r["absdS"], F32, 1, cw["dbias"],
        where + " attn dbias")
    _cb(w, "attn-dscale", n["dscale"], r["dscale"], r["E_dscale"] + gb["nwin"] * U * r["mdsp"], F32, 1, cw["dscale"],
        where + " attn dscale")


def check_cpb(w, where, blk, attn):
    """One block's share of _CpbFn: (w1, b1, w2, ls) -> the bias / scale its _WinAttnFn saved; the gradients it received are that
    node's d(bias) / d(scale) bit for bit; dw1, db1, dw2, dls with cpb_case's terms."""
    r = cpb64(d64(blk["w1"]), d64(blk["b1"]), d64(blk["w2"]), d64(blk["ls"]), d64(blk["dbias"]), d64(blk["dscale"]))
    _cb(w, "cpb-bias", attn["bias"], r["bias"], r["E_bias"], F32, 1, CPB_C["bias"], where + " cpb bias", extra=r["S_bias"])
    _cb(w, "cpb-scale", attn["scale"], r["scale"], r["E_scale"], F32, 1, 1.0, where + " cpb scale")
    w.same("cpb-route", blk["dbias"].reshape(-1), attn["dbias"].reshape(-1), where + " cpb received dbias")
    w.same("cpb-route", blk["dscale"].reshape(-1), attn["dscale"].reshape(-1), where + " cpb received dscale")
    for nm, shape in (("dw2", r["dw2"].shape), ("db1", (512,)), ("dw1", (512, 2))):
        _cb(w, "cpb-" + nm, blk[nm].reshape(shape), r[nm], r["E_" + nm], F32, 1, CPB_C[nm], f"{where} cpb {nm}")
    _cb(w, "cpb-dls", blk["dls"].reshape(-1), r["dls"], r["E_dls"], F32, 1, 1.0, where + " cpb dls")
    assert bool((blk["dls"].reshape(-1)[~r["inside"]] == 0).all()), where + ": d(logit_scale) beyond ln 100 not exactly 0"


def check_bias_operand(w, where, n, q_bias=None, v_bias=None):
    """The bias operand as the prep launch wrote it (n["bias_op"], fp32, twice for a paired layer): the layer's bias bit for bit;
    the qkv Linear's is q_bias | +0 | v_bias."""
    op = n.get("bias_op")
    if op is None:
        return
    if q_bias is not None:
        want = torch.cat([q_bias.detach().float(), torch.zeros_like(v_bias.detach().float()), v_bias.detach().float()])
    else:
        want = n["b"].detach().float()
    if n["pair"]:
        want = torch.cat([want, want])
    w.same("bias-operand", op.to(want.device), want, where + " bias operand")


@torch.no_grad()
def check_record(rec, w, cus=256, bracket=False):
    """Sections 2 and 3 of the issue on one record: every stored tensor and every returned gradient, stage-local.
    bracket: the hooks' dW / db / d(bias) are unfilled by contract and are not looked at (rec["grads"] is, by check_grads)."""
    cfg, N = rec["cfg"], rec["nodes"]
    B, dt = cfg["B"], cfg["dt"]
    blocks = block_list(cfg["depths"], cfg["heads"], cfg["img"])
    # embedding features
    Ay, Ac = (a.to(rec["y"].device) for a in R.embed_matrices(F32))
    ref, mag = R.embed_ref(rec["y"], rec["c"], Ay, Ac)
    _cb(w, "embed", N["pe.lin"]["x"], ref.reshape(-1, 24), mag.reshape(-1, 24), dt, 1, R.EMBED_C * U, "embed features")
    check_lin_fwd(w, "pe-lin", "patch embed", N["pe.lin"]["x"], N["pe.lin"]["W"], N["pe.lin"]["b"], N["pe.ln"]["x"])
    check_lin_bwd(w, "pe-lin", "patch embed", N["pe.lin"], bracket)
    check_bias_operand(w, "patch embed", N["pe.lin"])
    check_ln_fwd(w, "pe-ln", "patch embed", N["pe.ln"], None, N["b0.qkv"]["x"])
    check_ln_bwd(w, "pe-ln", "patch embed", N["pe.ln"], bracket)
    for k, (pre, li, C, res, heads, shift) in enumerate(blocks):
        where = f"block {k} (stage {li})"
        q, a, p, l1, m, l2 = (N[f"b{k}.{s}"] for s in ("qkv", "attn", "proj", "ln1", "mlp", "ln2"))
        assert a["geo"] == (B, res, C, heads, shift), (where, a["geo"])
        check_bias_operand(w, where + " qkv", q, rec["params"][pre + "attn.q_bias"], rec["params"][pre + "attn.v_bias"])
        check_bias_operand(w, where + " proj", p)
        check_lin_fwd(w, "qkv", where, q["x"], q["W"], q["b"], a["qkv"])
        check_attn(w, where, a, cus, bracket)
        if not bracket:
            check_cpb(w, where, N["cpb"][k], a)
        check_lin_fwd(w, "proj", where, a["out"], p["W"], p["b"], l1["x"])
        w.same("proj-x", p["x"], a["out"], where + " proj input")
        check_ln_fwd(w, "ln1", where, l1, q["x"], m["x"])                 # res: the block input
        check_mlp_fwd(w, where, m, l2["x"])
        last = k + 1 == len(blocks) or blocks[k + 1][1] != li
        if not last:
            y2 = N[f"b{k + 1}.qkv"]["x"]
        elif k + 1 == len(blocks):
            y2 = N["norm"]["x"]
        else:                                                            # invert the merge on the reduction Linear's saved x
            y2 = scatter_ref(N[f"m{li}.red"]["x"], B, res, C)
        check_ln_fwd(w, "ln2", where, l2, m["x"], y2)                     # res: LN1's output
        for nm, n in (("qkv", q), ("proj", p)):
            check_lin_bwd(w, nm, where, n, bracket)
        check_mlp_bwd(w, where, m, bracket)
        check_ln_bwd(w, "ln1", where, l1, bracket)
        check_ln_bwd(w, "ln2", where, l2, bracket)
        if last and k + 1 < len(blocks):
            where = f"merge {li}"
            mg, rd, ln = N[f"m{li}.merge"], N[f"m{li}.red"], N[f"m{li}.ln"]
            assert mg["geo"] == (B, res, C), (where, mg["geo"])
            w.same("merge-bwd", mg["dx"], scatter_ref(mg["dy"].contiguous(), B, res, C), where + " backward")
            check_lin_fwd(w, "red", where, rd["x"], rd["W"], None, ln["x"])
            check_lin_bwd(w, "red", where, rd, bracket)
            check_ln_fwd(w, "merge-ln", where, ln, None, N[f"b{k + 1}.qkv"]["x"])
            check_ln_bwd(w, "merge-ln", where, ln, bracket)
    # final norm through the pooled tensor, token mean, head
    nm_, mn, hd = N["norm"], N["mean"], N["head"]
    Bm, Ntok, Cf = mn["geo"]
    r = check_ln_fwd(w, "norm", "final norm", nm_, None, None)
    pool = lambda t: t.reshape(Bm, Ntok, Cf).mean(1)                     # noqa: E731
    _cb(w, "pooled", hd["x"], pool(r["y"]), pool(r["ymag"]), dt, 1, (LN_C["y"] * Cf + Ntok) * U, "pooled", extra=pool(ulp(r["y"], dt)))
    check_ln_bwd(w, "norm", "final norm", nm_, bracket)
    ref = (d64(mn["dy"]) / Ntok)[:, None, :].expand(Bm, Ntok, Cf).reshape(Bm * Ntok, Cf)
    _cb(w, "mean-bwd", mn["dx"], ref, ref.abs(), dt, 1, Ntok * U, "token mean backward")
    check_lin_fwd(w, "head", "head", hd["x"], hd["W"], hd["b"], rec["logits"])
    check_lin_bwd(w, "head", "head", hd, bracket)
    check_bias_operand(w, "head", hd)


def grad_sources(rec):
    """{parameter name: the tensor its node returned for it} (the q_bias / v_bias gradients are slices of the qkv Linear's db)."""
    cfg, N = rec["cfg"], rec["nodes"]
    src = {}

    def lin(pre, n):
        src[pre + "weight"] = n["dW"]
        if n["b"] is not None:
            src[pre + "bias"] = n["db"]

    def ln(pre, n):
        src[pre + "weight"], src[pre + "bias"] = n["dg"], n["dbeta"]
    lin("patch_embed.projection.0.", N["pe.lin"])
    ln("patch_embed.norm.", N["pe.ln"])
    blocks = block_list(cfg["depths"], cfg["heads"], cfg["img"])
    for k, (pre, li, C, res, heads, shift) in enumerate(blocks):
        q = N[f"b{k}.qkv"]
        src[pre + "attn.qkv.weight"] = q["dW"]
        src[pre + "attn.q_bias"], src[pre + "attn.v_bias"] = q["db"][:C], q["db"][2 * C:3 * C]
        lin(pre + "attn.proj.", N[f"b{k}.proj"])
        ln(pre + "norm1.", N[f"b{k}.ln1"])
        ln(pre + "norm2.", N[f"b{k}.ln2"])
        m = N[f"b{k}.mlp"]
        src[pre + "mlp.fc1.weight"], src[pre + "mlp.fc1.bias"] = m["dW1"], m["db1"]
        src[pre + "mlp.fc2.weight"], src[pre + "mlp.fc2.bias"] = m["dW2"], m["db2"]
        cb = N["cpb"][k]
        src[pre + "attn.cpb_mlp.0.weight"], src[pre + "attn.cpb_mlp.0.bias"] = cb["dw1"], cb["db1"]
        src[pre + "attn.cpb_mlp.2.weight"], src[pre + "attn.logit_scale"] = cb["dw2"], cb["dls"]
        if k + 1 < len(blocks) and blocks[k + 1][1] != li:
            src[f"layers.{li}.downsample.reduction.weight"] = N[f"m{li}.red"]["dW"]
            ln(f"layers.{li}.downsample.norm.", N[f"m{li}.ln"])
    ln("norm.", N["norm"])
    lin("head.", N["head"])
    return src


@torch.no_grad()
def check_grads(rec, w):
    """Every parameter's .grad is what its node returned, bit for bit."""
    src = grad_sources(rec)
    assert sorted(src) == sorted(rec["grads"]), sorted(set(src) ^ set(rec["grads"]))
    for name, g in rec["grads"].items():
        w.same("grad-route", g.reshape(-1), src[name].reshape(-1).to(g.device), f".grad of {name}")


def with_grads(rec, grads):
    """A copy of the record whose returned parameter gradients are replaced by `grads` ({name: tensor}): the bracket run's final
    .grad tensors go through the first run's fp64 bounds this way (check_record on the result)."""
    out = dict(rec, nodes={k: (dict(v) if isinstance(v, dict) else [dict(b) for b in v]) for k, v in rec["nodes"].items()})
    N, cfg = out["nodes"], rec["cfg"]

    def lin(pre, n):
        n["dW"] = grads[pre + "weight"]
        if n["b"] is not None:
            n["db"] = grads[pre + "bias"]

    def ln(pre, n):
        n["dg"], n["dbeta"] = grads[pre + "weight"], grads[pre + "bias"]
    lin("patch_embed.projection.0.", N["pe.lin"])
    ln("patch_embed.norm.", N["pe.ln"])
    blocks = block_list(cfg["depths"], cfg["heads"], cfg["img"])
    for k, (pre, li, C, res, heads, shift) in enumerate(blocks):
        q = N[f"b{k}.qkv"]
        q["dW"] = grads[pre + "attn.qkv.weight"]
        db = q["db"].clone()                    # the k third of the vector's gradient reaches no parameter: the first run's
        db[:C], db[2 * C:3 * C] = grads[pre + "attn.q_bias"], grads[pre + "attn.v_bias"]
        q["db"] = db
        lin(pre + "attn.proj.", N[f"b{k}.proj"])
        ln(pre + "norm1.", N[f"b{k}.ln1"])
        ln(pre + "norm2.", N[f"b{k}.ln2"])
        m = N[f"b{k}.mlp"]
        m["dW1"], m["db1"] = grads[pre + "mlp.fc1.weight"], grads[pre + "mlp.fc1.bias"]
        m["dW2"], m["db2"] = grads[pre + "mlp.fc2.weight"], grads[pre + "mlp.fc2.bias"]
        cb = N["cpb"][k]
        cb["dw1"], cb["db1"] = grads[pre + "attn.cpb_mlp.0.weight"], grads[pre + "attn.cpb_mlp.0.bias"]
        cb["dw2"], cb["dls"] = grads[pre + "attn.cpb_mlp.2.weight"], grads[pre + "attn.logit_scale"]
        if k + 1 < len(blocks) and blocks[k + 1][1] != li:
            N[f"m{li}.red"]["dW"] = grads[f"layers.{li}.downsample.reduction.weight"]
            ln(f"layers.{li}.downsample.norm.", N[f"m{li}.ln"])
    ln("norm.", N["norm"])
    lin("head.", N["head"])
    return out


DX_KEYS = {"lin": ("dx",), "mlp": ("dx",), "ln": ("dx", "dres"), "attn": ("dqkv",), "merge": ("dx",), "mean": ("dx",)}


@torch.no_grad()
def same_dx(rec_a, rec_b, w):
    """Every node's dx / dqkv of run b is run a's, bit for bit (section 4)."""
    for name, n in rec_a["nodes"].items():
        if name == "cpb":
            continue
        for key in DX_KEYS[n["kind"]]:
            a, b = n[key], rec_b["nodes"][name][key]
            if a is None or b is None:
                assert a is None and b is None, (name, key)
                continue
            w.same("bracket-dx", a, b, f"{name} {key} (bracket run against the default run)")


# ============================================================================================== the graph as the record
def _nm(fn):
    return type(fn).__name__


def _is(fn, cls):
    assert fn is not None and _nm(fn) == cls + "Backward", f"expected a {cls} node, found {_nm(fn) if fn is not None else None}"
    return fn


def _param_of(edge, p, what):
    """edge = (AccumulateGrad node, 0) of parameter p, possibly behind views (logit_scale.view(-1))."""
    fn = edge[0]
    while fn is not None and not hasattr(fn, "variable"):
        assert len(fn.next_functions) == 1, (what, _nm(fn))
        fn = fn.next_functions[0][0]
    assert fn is not None and fn.variable is p, f"{what}: not the expected parameter"


def topology(model, logits):
    """Section 1: walk the graph from logits.grad_fn, assert the node sequence and the (node, output index) edges, and return
    {record name: node} ("cpb": the one _CpbFn node; f"b{k}.qb": block k's _QkvBiasFn)."""
    T = {}
    head = T["head"] = _is(logits.grad_fn, "_LinearFn")
    _param_of(head.next_functions[1], model.head.weight, "head weight")
    _param_of(head.next_functions[2], model.head.bias, "head bias")
    assert head.next_functions[0][1] == 0
    mean = T["mean"] = _is(head.next_functions[0][0], "_MeanFn")
    assert mean.next_functions[0][1] == 0
    norm = T["norm"] = _is(mean.next_functions[0][0], "_LNFn")
    _param_of(norm.next_functions[1], model.norm.weight, "norm weight")
    assert not norm.has_res and len(norm.next_functions) == 3
    cur = norm.next_functions[0]
    k = sum(len(ly.blocks) for ly in model.layers)
    cpb = None
    res0 = model.patches_resolution[0]
    for li in range(len(model.layers) - 1, -1, -1):
        ly = model.layers[li]
        res = res0 >> li
        if ly.downsample is not None:
            ln = T[f"m{li}.ln"] = _is(cur[0], "_LNFn")
            assert cur[1] == 0 and not ln.has_res and ln.next_functions[0][1] == 0
            _param_of(ln.next_functions[1], ly.downsample.norm.weight, f"merge {li} norm")
            red = T[f"m{li}.red"] = _is(ln.next_functions[0][0], "_LinearFn")
            assert len(red.next_functions) == 2 and red.next_functions[0][1] == 0 and not red.has_b      # no bias
            _param_of(red.next_functions[1], ly.downsample.reduction.weight, f"merge {li} reduction")
            mg = T[f"m{li}.merge"] = _is(red.next_functions[0][0], "_MergeFn")
            cur = mg.next_functions[0]
        for bi in range(len(ly.blocks) - 1, -1, -1):
            k -= 1
            blk, where = ly.blocks[bi], f"block {k}"
            ln2 = T[f"b{k}.ln2"] = _is(cur[0], "_LNFn")
            assert cur[1] == 0, where
            mlp = T[f"b{k}.mlp"] = _is(ln2.next_functions[0][0], "_MlpFn")
            assert ln2.next_functions[0] == (mlp, 0) and ln2.next_functions[3] == (mlp, 1), where + ": LN2's x / shortcut"
            assert ln2.has_res and ln2.rps == res * res, where
            _param_of(ln2.next_functions[1], blk.norm2.weight, where + " norm2")
            for i, p in enumerate((blk.mlp.fc1.weight, blk.mlp.fc1.bias, blk.mlp.fc2.weight, blk.mlp.fc2.bias)):
                _param_of(mlp.next_functions[1 + i], p, f"{where} mlp parameter {i}")
            ln1 = T[f"b{k}.ln1"] = _is(mlp.next_functions[0][0], "_LNFn")
            assert mlp.next_functions[0][1] == 0 and ln1.has_res and ln1.rps == res * res, where
            _param_of(ln1.next_functions[1], blk.norm1.weight, where + " norm1")
            proj = T[f"b{k}.proj"] = _is(ln1.next_functions[0][0], "_LinearFn")
            assert ln1.next_functions[0][1] == 0, where
            _param_of(proj.next_functions[1], blk.attn.proj.weight, where + " proj weight")
            _param_of(proj.next_functions[2], blk.attn.proj.bias, where + " proj bias")
            attn = T[f"b{k}.attn"] = _is(proj.next_functions[0][0], "_WinAttnFn")
            assert proj.next_functions[0][1] == 0, where
            qkv = T[f"b{k}.qkv"] = _is(attn.next_functions[0][0], "_LinearFn")
            assert attn.next_functions[0] == (qkv, 0) and ln1.next_functions[3] == (qkv, 1), where + ": the shortcut fork"
            _param_of(qkv.next_functions[1], blk.attn.qkv.weight, where + " qkv weight")
            c = _is(attn.next_functions[1][0], "_CpbFn")
            cpb = c if cpb is None else cpb
            assert c is cpb and attn.next_functions[1] == (cpb, 2 * k) and attn.next_functions[2] == (cpb, 2 * k + 1), where + ": cpb"
            qb = T[f"b{k}.qb"] = _is(qkv.next_functions[2][0], "_QkvBiasFn")
            _param_of(qb.next_functions[0], blk.attn.q_bias, where + " q_bias")
            _param_of(qb.next_functions[1], blk.attn.v_bias, where + " v_bias")
            want = 0 if (bi % 2 == 0 or res == WS) else WS // 2
            assert attn.geo[1] == res and attn.geo[3] == blk.num_heads and attn.geo[4] == want, (where, attn.geo, want)
            cur = qkv.next_functions[0]
    assert k == 0
    T["cpb"] = cpb
    allb = [b for ly in model.layers for b in ly.blocks]
    for i, b in enumerate(allb):
        for j, p in enumerate((b.attn.cpb_mlp[0].weight, b.attn.cpb_mlp[0].bias, b.attn.cpb_mlp[2].weight, b.attn.logit_scale)):
            _param_of(cpb.next_functions[4 * i + j], p, f"cpb input {4 * i + j}")
    pln = T["pe.ln"] = _is(cur[0], "_LNFn")
    assert cur[1] == 0 and not pln.has_res
    _param_of(pln.next_functions[1], model.patch_embed.norm.weight, "patch embed norm")
    pl = T["pe.lin"] = _is(pln.next_functions[0][0], "_LinearFn")
    assert pl.next_functions[0][0] is None                               # the features: no gradient
    _param_of(pl.next_functions[1], model.patch_embed.projection[0].weight, "patch embed weight")
    return T


PARAM_GRAD_KEYS = ("dW", "db", "dW1", "db1", "dW2", "db2", "dg", "dbeta", "dbias", "dscale", "dw1", "dw2", "dls")


def observe(model, T, dt, bracket=False):
    """Read every node's saved tensors and ctx attributes NOW (before backward) and hook it; returns the nodes dict of a record,
    whose gradient fields the hooks fill during backward().
    bracket: a run inside the weight-gradient bracket.  The parameter gradients a node returns there are still unwritten and
    AccumulateGrad must ADOPT them (swinv2.py _tn_finish); a second reference would make it copy the unwritten contents into
    .grad instead, so the hooks keep none: those fields are None."""
    P = dict(model.named_parameters())
    N = {}

    def W(name):
        return P[name].detach().to(dt)

    def hook(fn, fill, *nodes):
        def run(gi, go):
            fill(gi, go)
            if bracket:
                for n in nodes:
                    n.update({key: None for key in PARAM_GRAD_KEYS if key in n})
        fn.register_hook(run)

    def lin(name, pname, has_b=True, b=None):
        fn = T[name]
        n = N[name] = dict(kind="lin", x=fn.saved_tensors[0], W=W(pname + ".weight"), pair=fn.pair,
                           b=(b if b is not None else P[pname + ".bias"].detach()) if has_b else None,
                           bias_op=fn.sh[2] if len(fn.sh) > 2 and fn.sh[2] is not None else None)
        assert fn.pair == is_paired(*n["W"].shape), (name, n["W"].shape)
        if fn.pair:                                   # the shadow operand IS diag(W, W)
            assert torch.equal(bits(fn.sh[0]), bits(torch.block_diag(n["W"].float(), n["W"].float()).to(dt))), name + ": shadow"
        else:
            assert torch.equal(bits(fn.sh[0]), bits(n["W"])), name + ": shadow"

        def fill(gi, go):
            n.update(dy=go[0], dxs=go[1] if len(go) > 1 else None, dx=gi[0], dW=gi[1], db=gi[2] if has_b else None)
        hook(fn, fill, n)

    def ln(name):
        fn = T[name]
        x, g, mean, rstd, ss = fn.saved_tensors
        n = N[name] = dict(kind="ln", x=x, gamma=g, mean=mean, rstd=rstd, ss=ss, rps=fn.rps, has_res=fn.has_res)

        def fill(gi, go):
            n.update(dy=go[0], dx=gi[0], dg=gi[1], dbeta=gi[2], dres=gi[3] if len(gi) > 3 else None)
        hook(fn, fill, n)
        return n

    lin("pe.lin", "patch_embed.projection.0")
    ln("pe.ln")["beta"] = P["patch_embed.norm.bias"].detach()
    k = 0
    N["cpb"] = []
    for li, ly in enumerate(model.layers):
        for bi, blk in enumerate(ly.blocks):
            pre = f"layers.{li}.blocks.{bi}."
            C = blk.dim
            qb = torch.cat([blk.attn.q_bias.detach(), torch.zeros_like(blk.attn.v_bias.detach()), blk.attn.v_bias.detach()])
            lin(f"b{k}.qkv", pre + "attn.qkv", True, qb)
            fn = T[f"b{k}.attn"]
            qkv, out, bias, scale, lse = fn.saved_tensors
            a = N[f"b{k}.attn"] = dict(kind="attn", qkv=qkv, out=out, bias=bias, scale=scale, lse=lse, geo=tuple(fn.geo))

            def fill_a(gi, go, a=a):
                a.update(dout=go[0], dqkv=gi[0], dbias=gi[1], dscale=gi[2])
            hook(fn, fill_a, a)
            lin(f"b{k}.proj", pre + "attn.proj")
            ln(f"b{k}.ln1")["beta"] = P[pre + "norm1.bias"].detach()
            fn = T[f"b{k}.mlp"]
            x, g, gp = fn.saved_tensors
            m = N[f"b{k}.mlp"] = dict(kind="mlp", x=x, g=g, gp=gp, W1=W(pre + "mlp.fc1.weight"), b1=P[pre + "mlp.fc1.bias"].detach(),
                                      W2=W(pre + "mlp.fc2.weight"), b2=P[pre + "mlp.fc2.bias"].detach(), p1=fn.p1, p2=fn.p2)
            assert fn.p1 == is_paired(4 * C, C) and fn.p2 == is_paired(C, 4 * C), pre

            def fill_m(gi, go, m=m):
                m.update(dy=go[0], dxs=go[1] if len(go) > 1 else None, dx=gi[0], dW1=gi[1], db1=gi[2], dW2=gi[3], db2=gi[4])
            hook(fn, fill_m, m)
            ln(f"b{k}.ln2")["beta"] = P[pre + "norm2.bias"].detach()
            at = blk.attn
            N["cpb"].append(dict(w1=at.cpb_mlp[0].weight.detach(), b1=at.cpb_mlp[0].bias.detach(), w2=at.cpb_mlp[2].weight.detach(),
                                 ls=at.logit_scale.detach().reshape(-1)))
            k += 1
        if ly.downsample is not None:
            fn = T[f"m{li}.merge"]
            mg = N[f"m{li}.merge"] = dict(kind="merge", geo=tuple(fn.geo))

            def fill_g(gi, go, mg=mg):
                mg.update(dy=go[0], dx=gi[0])
            hook(fn, fill_g, mg)
            lin(f"m{li}.red", f"layers.{li}.downsample.reduction", False)
            ln(f"m{li}.ln")["beta"] = P[f"layers.{li}.downsample.norm.bias"].detach()
    ln("norm")["beta"] = P["norm.bias"].detach()
    fn = T["mean"]
    mn = N["mean"] = dict(kind="mean", geo=tuple(fn.geo))

    def fill_mean(gi, go):
        mn.update(dy=go[0], dx=gi[0])
    hook(fn, fill_mean, mn)
    lin("head", "head")

    def fill_c(gi, go):
        for i, b in enumerate(N["cpb"]):
            b.update(dbias=go[2 * i], dscale=go[2 * i + 1], dw1=gi[4 * i], db1=gi[4 * i + 1], dw2=gi[4 * i + 2], dls=gi[4 * i + 3])
    hook(T["cpb"], fill_c, *N["cpb"])
    return N


# ================================================================================================================ engine
DEFECTS = ("bias_twice_second_half", "fold_off_diagonal", "ln1_res_from_proj", "drop_scale_on_residual", "drop_scale_row_mod_B",
           "shift_rolled_wrong_way", "fork_grad_dropped", "fork_grad_twice", "qv_bias_grads_swapped", "nonzero_k_bias",
           "merge_neighbours_swapped", "mean_div_previous_N")


class Engine:
    """The whole model, forward and hand-written backward, stage by stage, producing a record.  T = float64: the composed stage
    references.  T = bf16 / fp16 / fp32: the nodes' rounding points (module docstring), exact arithmetic in between.
    defect: one of DEFECTS, seeded where it would arise in swinv2.py.  drops: [blocks][2][B] fp64 DropPath scales or None."""

    def __init__(self, params, cfg, T, defect=None, drops=None):
        assert defect is None or defect in DEFECTS, defect
        self.cfg, self.T, self.defect, self.drops = dict(cfg, dt=T), T, defect, drops
        self.F = F64 if T == F64 else F32
        self.P = {k: v.double() for k, v in params.items()}
        self.N = {"cpb": []}

    # ---- rounding
    def t(self, x):
        return x.to(self.T)

    def f(self, x):
        return x.to(self.F)

    def wT(self, name):
        return self.t(self.P[name])                  # the shadow: W in the compute dtype

    # ---- stages
    def lin_fwd(self, name, x, pname, b=None, has_b=True):
        W = self.wT(pname + ".weight")
        if has_b and b is None:
            b = self.f(self.P[pname + ".bias"])
        Nn, Kk = W.shape
        pair = is_paired(Nn, Kk)
        op = None if b is None else (torch.cat([b, b]) if pair else b)
        if pair:                                     # the [M / 2, 2 K] view times diag(W, W)^T, the bias written twice
            M = x.shape[0]
            W2 = torch.block_diag(d64(W), d64(W))
            y = d64(x).view(M // 2, 2 * Kk) @ W2.T
            if b is not None:
                y = y + d64(op)
                if self.defect == "bias_twice_second_half":
                    y[:, Nn:] += d64(b)
            y = y.view(M, Nn)
        else:
            y = d64(x) @ d64(W).T + (d64(b) if b is not None else 0.0)
        self.N[name] = dict(kind="lin", x=x, W=W, b=b, pair=pair, bias_op=None if op is None else op.float())
        return self.t(y)

    def tn(self, dy, x, pair, want_b=True):
        """(dW, db) in F; the paired layer's [2N, 2K] product of the row-parity views and the fold of its diagonal blocks."""
        dy, x = d64(dy), d64(x)
        M, N = dy.shape
        K = x.shape[1]
        if not pair:
            return self.f(dy.T @ x), self.f(dy.sum(0)) if want_b else None
        big = self.f(dy.view(M // 2, 2 * N).T @ x.view(M // 2, 2 * K))
        bb = self.f(dy.view(M // 2, 2 * N).sum(0))
        second = big[N:, :K] if self.defect == "fold_off_diagonal" else big[N:, K:]
        return self.f(d64(big[:N, :K]) + d64(second)), self.f(d64(bb[:N]) + d64(bb[N:])) if want_b else None

    def res_epi(self, pre, dxs):
        """EPI_RES: T(T(pre) + R) in the 16-bit modes (the staged epilogue), T(pre + R) otherwise."""
        if dxs is None:
            return self.t(pre)
        if self.defect == "fork_grad_dropped":
            return self.t(pre)
        r = d64(dxs) * (2.0 if self.defect == "fork_grad_twice" else 1.0)
        return self.t(d64(self.t(pre)) + r) if self.T in (BF16, F16) else self.t(pre + r)

    def lin_bwd(self, name, dy, dxs=None, need_dx=True):
        n = self.N[name]
        dW, db = self.tn(dy, n["x"], n["pair"], n["b"] is not None)
        dx = self.res_epi(d64(dy) @ d64(n["W"]), dxs) if need_dx else None
        n.update(dy=dy, dxs=dxs, dx=dx, dW=dW, db=db)
        return dx

    def ln_fwd(self, name, x, pname, res=None, ss=None, rps=1):
        g, b = self.f(self.P[pname + ".weight"]), self.f(self.P[pname + ".bias"])
        x64 = d64(x)
        M = x.shape[0]
        mu = x64.mean(1, keepdim=True)
        rs = 1.0 / torch.sqrt(((x64 - mu) ** 2).mean(1, keepdim=True) + 1e-5)
        mean, rstd = self.f(mu[:, 0]), self.f(rs[:, 0])
        y = (x64 - d64(mean)[:, None]) * d64(rstd)[:, None] * d64(g) + d64(b)
        sc = None
        if ss is not None:
            if self.defect == "drop_scale_row_mod_B":
                sc = d64(ss)[torch.arange(M) % ss.numel()][:, None]
            else:
                sc = row_scale(ss, rps, M)
            y = y * sc
        if res is not None:
            y = y + d64(res) * (sc if (sc is not None and self.defect == "drop_scale_on_residual") else 1.0)
        self.N[name] = dict(kind="ln", x=x, gamma=g, beta=b, mean=mean, rstd=rstd, ss=None if ss is None else ss.float(), rps=rps,
                            has_res=res is not None, _sc=sc)
        return self.t(y)

    def ln_bwd(self, name, dy):
        n = self.N[name]
        r = ln_bwd64(d64(dy), d64(n["x"]), d64(n["mean"]), d64(n["rstd"]), d64(n["gamma"]), n["_sc"])
        dres = None
        if n["has_res"]:
            dres = dy if self.defect != "drop_scale_on_residual" or n["_sc"] is None else self.t(d64(dy) * n["_sc"])
        n.update(dy=dy, dx=self.t(r["dx"]), dg=self.f(r["dg"]), dbeta=self.f(r["db"]), dres=dres)
        return n["dx"], dres

    def attn_fwd(self, name, qkv, bias, scale, geo):
        B, res, C, heads, shift = geo
        roll = -shift if self.defect == "shift_rolled_wrong_way" else shift
        r = win64(d64(qkv), d64(bias), d64(scale), B, res, heads, shift, F64, roll=roll)
        self.N[name] = dict(kind="attn", qkv=qkv, out=self.t(r["out"]), bias=bias, scale=scale, lse=self.f(r["lse"]).reshape(-1),
                            geo=geo, _roll=roll)
        return self.N[name]["out"]

    def attn_bwd(self, name, dout):
        n = self.N[name]
        B, res, C, heads, shift = n["geo"]
        r = win64(d64(n["qkv"]), d64(n["bias"]), d64(n["scale"]), B, res, heads, shift, F64, d64(dout), d64(n["out"]), d64(n["lse"]),
                  roll=n["_roll"])
        n.update(dout=dout, dqkv=self.t(r["dqkv"]), dbias=self.f(r["dbias"]), dscale=self.f(r["dscale"]))
        return n["dqkv"]

    def mlp_fwd(self, name, x, pre):
        W1, W2 = self.wT(pre + "fc1.weight"), self.wT(pre + "fc2.weight")
        b1, b2 = self.f(self.P[pre + "fc1.bias"]), self.f(self.P[pre + "fc2.bias"])
        p = d64(self.t(d64(x) @ d64(W1).T + d64(b1)))               # the pre-activation is rounded to T on every path
        g, gp = self.t(gelu64(p)), self.t(dgelu64(p))
        y = self.t(d64(g) @ d64(W2).T + d64(b2))
        self.N[name] = dict(kind="mlp", x=x, g=g, gp=gp, W1=W1, b1=b1, W2=W2, b2=b2, p1=is_paired(*W1.shape), p2=is_paired(*W2.shape))
        return y

    def mlp_bwd(self, name, dy, dxs):
        n = self.N[name]
        du = self.t(d64(self.t(d64(dy) @ d64(n["W2"]))) * d64(n["gp"]))
        dW2, db2 = self.tn(dy, n["g"], n["p2"])
        dW1, db1 = self.tn(du, n["x"], n["p1"])
        dx = self.res_epi(d64(du) @ d64(n["W1"]), dxs)
        n.update(dy=dy, dxs=dxs, dx=dx, dW1=dW1, db1=db1, dW2=dW2, db2=db2)
        return dx

    # ---- the model
    def run(self, y, c, dlogits):
        """dlogits: the gradient the head receives ([B, classes], rounded to T), or a function of the logits that returns it."""
        cfg, P, N = self.cfg, self.P, self.N
        B = cfg["B"]
        blocks = block_list(cfg["depths"], cfg["heads"], cfg["img"])
        Ay, Ac = R.embed_matrices(self.F)
        feat = self.t(R.embed_ref(y, c, Ay, Ac)[0].reshape(-1, 24))
        x = self.lin_fwd("pe.lin", feat, "patch_embed.projection.0")
        x = self.ln_fwd("pe.ln", x, "patch_embed.norm")
        for k, (pre, li, C, res, heads, shift) in enumerate(blocks):
            a = pre + "attn."
            cp = dict(w1=self.f(P[a + "cpb_mlp.0.weight"]), b1=self.f(P[a + "cpb_mlp.0.bias"]), w2=self.f(P[a + "cpb_mlp.2.weight"]),
                      ls=self.f(P[a + "logit_scale"]).reshape(-1))
            r = cpb64(*(d64(cp[s]) for s in ("w1", "b1", "w2", "ls")))
            N["cpb"].append(cp)
            kb = self.f(P[a + "q_bias"]) if self.defect == "nonzero_k_bias" else torch.zeros(C, dtype=self.F)
            qb = torch.cat([self.f(P[a + "q_bias"]), kb, self.f(P[a + "v_bias"])])
            xs = x
            qkv = self.lin_fwd(f"b{k}.qkv", x, a + "qkv", b=qb)
            o = self.attn_fwd(f"b{k}.attn", qkv, self.f(r["bias"]), self.f(r["scale"]), (B, res, C, heads, shift))
            o = self.lin_fwd(f"b{k}.proj", o, a + "proj")
            dr = (None, None) if self.drops is None else self.drops[k]
            x = self.ln_fwd(f"b{k}.ln1", o, pre + "norm1", o if self.defect == "ln1_res_from_proj" else xs, dr[0], res * res)
            h = self.mlp_fwd(f"b{k}.mlp", x, pre + "mlp.")
            x = self.ln_fwd(f"b{k}.ln2", h, pre + "norm2", x, dr[1], res * res)
            if k + 1 < len(blocks) and blocks[k + 1][1] != li:
                N[f"m{li}.merge"] = dict(kind="merge", geo=(B, res, C))
                m = merge_ref(x, B, res, C)
                if self.defect == "merge_neighbours_swapped":
                    m = torch.cat([m[:, :C], m[:, 2 * C:3 * C], m[:, C:2 * C], m[:, 3 * C:]], 1)
                m = self.lin_fwd(f"m{li}.red", m.contiguous(), f"layers.{li}.downsample.reduction", has_b=False)
                x = self.ln_fwd(f"m{li}.ln", m, f"layers.{li}.downsample.norm")
        pre, li, C, res, heads, shift = blocks[-1]
        Ntok = res * res
        x = self.ln_fwd("norm", x, "norm")
        div = Ntok * 4 if self.defect == "mean_div_previous_N" else Ntok
        N["mean"] = dict(kind="mean", geo=(B, Ntok, C))
        pooled = self.t(d64(x).reshape(B, Ntok, C).sum(1) / div)
        logits = self.lin_fwd("head", pooled, "head")
        # ------------------------------------------------------------------------------------------------ backward
        d = self.lin_bwd("head", self.t(dlogits(logits) if callable(dlogits) else dlogits))
        N["mean"].update(dy=d, dx=self.t((d64(d) / div)[:, None, :].expand(B, Ntok, C).reshape(B * Ntok, C)))
        d, _ = self.ln_bwd("norm", N["mean"]["dx"])
        for k in range(len(blocks) - 1, -1, -1):
            pre, li, C, res, heads, shift = blocks[k]
            if k + 1 < len(blocks) and blocks[k + 1][1] != li:
                d, _ = self.ln_bwd(f"m{li}.ln", d)
                d = self.lin_bwd(f"m{li}.red", d)
                order = (0, 2, 1, 3) if self.defect == "merge_neighbours_swapped" else (0, 1, 2, 3)
                N[f"m{li}.merge"].update(dy=d, dx=scatter_ref(d, B, res, C, order))
                d = N[f"m{li}.merge"]["dx"]
            d, dres = self.ln_bwd(f"b{k}.ln2", d)
            d = self.mlp_bwd(f"b{k}.mlp", d, dres)
            d, dres = self.ln_bwd(f"b{k}.ln1", d)
            if self.defect == "ln1_res_from_proj":           # the shortcut's gradient goes where the residual came from
                d, dres = self.t(d64(d) + d64(dres)), None
            d = self.lin_bwd(f"b{k}.proj", d)
            d = self.attn_bwd(f"b{k}.attn", d)
            d = self.lin_bwd(f"b{k}.qkv", d, dres)
            a, cp = N[f"b{k}.attn"], N["cpb"][k]
            r = cpb64(*(d64(cp[s]) for s in ("w1", "b1", "w2", "ls")), d64(a["dbias"]), d64(a["dscale"]))
            cp.update(dbias=a["dbias"], dscale=a["dscale"], dw1=self.f(r["dw1"]), db1=self.f(r["db1"]), dw2=self.f(r["dw2"]),
                      dls=self.f(r["dls"]))
        d, _ = self.ln_bwd("pe.ln", d)
        self.lin_bwd("pe.lin", d, need_dx=False)
        rec = dict(cfg=self.cfg, nodes=N, y=y, c=c, logits=logits, params={k: v.float() for k, v in P.items()})
        src = grad_sources(rec)
        if self.defect == "qv_bias_grads_swapped":
            for pre, *_ in blocks:
                q, v = pre + "attn.q_bias", pre + "attn.v_bias"
                src[q], src[v] = src[v], src[q]
        rec["grads"] = {k: v.clone() for k, v in src.items()}
        return rec
