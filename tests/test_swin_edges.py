"""Element-wise edge tests of SwinV2's own kernels (tests/kernel_check.py): window attention forward / backward, the
lanes-per-row LayerNorm past its grid caps, the continuous position bias at model block counts, merge gather, token mean and
the sub-block embedding.

Every case writes into canary-filled guarded outputs, reads inputs whose trailing rows are NaN, gets a workspace of exactly the
size its *_workspace() entry returns (checked for margin writes only), asserts the device kernel it was meant to reach, and is
checked element by element against fp64 of the T-rounded inputs:  |got - ref| <= ulp_T(ref) + c E, E the sum of the named terms
below (tests/swin_ref.py computes them), c fitted per (dtype, output): twice the worst measured on one MI355X or less, measured
value in brackets.  Window attention compares in window layout, so a violation names (window, head, query / key, d).

Window attention (u = 2^-24, u_T = 2^-8 bf16 / 2^-11 fp16 / u fp32, A = |q^||k^|^T, s = exp(min(logit_scale, ln 100))):
- logit error e: q^ and k^ rounded to T before the MFMA, s times that rounding: 2 u_T s A; the fp32 norms (sum of squares + rsq):
  36 u s A; the fp32 MFMA over d: 32 u s A; base-2 logit arithmetic, exp2, log2: 4 u (s + |logit| + |mask| + |lse|).
- out: (P o e)|v| + (sum_j P e) P|v| (the logit error through the softmax); P rounded to T before P V: u_T P|v| (16-bit);
  fp32 P V accumulation: 64 u P|v|.   lse: sum_j P e + 4 u (|lse| + 1).
- backward, on the kernel's own out and lse: dS = P (dO V^T - dO . O): P e |dP - D| + 40 u P (|dO||V|^T + |dO| . |O|).
  dq^ = s dS k^: s E_dS |k^| + (2 u_T + 64 u) s |dS||k^| (s dS and k^ rounded to T before the MFMA); dq = (I - q^q^^T) dq^ / |q|
  (dq^ / eps where |q| < eps = 1e-12, as autograd of F.normalize: include/rgbnm.h):
  E through the projection + (2 u_T + 24 u)(|dq^| + |q^| (|q^| . |dq^|)) / |q| (q^ rounded to T, fp32 projection); dk likewise.
  dv = P^T dO: (P o e)^T |dO| + (u_T + 64 u) P^T |dO|.
  d(bias)[h] = sum over windows of dS: sum E_dS + (most windows per wave + slices) u sum |dS| (the wave's running sum, then
  the fixed-order reduction over the per-wave slices).  d(scale) partial: sum_ij E_dS |cos| + |dS| A (2 u_T + 68 u) +
  64 u |dS cos|; d(scale): sum of the partials' terms + (windows) u sum |dS cos|.
Geometry: a Python copy of head_grid() / WA<T> (tests/swin_ref.py, pinned by tests/test_swin_edges_cpu.py) picks cases from the
device's CU count; every dtype must reach (a) a capped grid with idle waves, (b) exactly one window per wave, (c) a head-major
grid whose waves walk >= 3 windows with a ragged last range, (d) the XCD-aware slot map with multi-window waves, and fp32
(e) its two-wave backward.

Position bias: table t = relu(coords W1^T + b1) W2^T: 18 u |W2| (|coords||W1|^T + |b1|) (two fma, a 512-term fp32 dot
product); bias = 16 sigmoid(t): 16 s(1-s) E_t + 4 u bias; d table: 16 s(1-s) 64 u sum|dbias| + |sum dbias| 16 |s(1-s)(1-2s)| E_t
+ 4 u |dt|; dW2 / db1 / dW1 sums over the 225 entries: E_dt through the sums + 40 u of the sums' magnitudes.

Embedding (rgbnm_swin_embed): A^T X A per 8 x 8 block as two sequential 8-term fp32 dot products, then the einops split into
sub-block tokens: ulp_TO(ref) + EMBED_C u |A|^T |X| |A| with EMBED_C = 2 g8 + g8^2 = 16.0000114 DERIVED in tests/swin_ref.py, not
fitted; all nine in / out type pairs at grids with Hb != Wb, NaN behind both inputs, single-coefficient probes for luma and each
chroma channel.  Worst ratio on one MI355X: 0.201 into fp32, 0.500 / 0.499 into bf16 / fp16; the eleven tests take 2 s.
"""
import math

import pytest
import torch

import kernel_check as KC
import swin_ref as R
from kernel_check import U, guarded, nan_padded, check_bound, launched, ulp
from rgb_no_more_amd import lib as L, swinv2 as SW
from oracle import swin_torch as ST
from test_hip_kernels import option  # noqa: F401  (fixture: set a runtime switch for one test)
from test_kernel_edges import ln_case, expect

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
DTS3 = [F32, BF16, F16]
NAMES = {F32: "f32", BF16: "bf16", F16: "f16"}
ESZ = {F32: 4, BF16: 2, F16: 2}

# c of the bound ulp_T + c E per (dtype, output): twice the worst measured on one MI355X or less (measured in brackets)
WIN_C = {
    F32: {"out": 0.12,      # [0.0631]
          "lse": 0.16,      # [0.0846]
          "dq": 0.16,       # [0.0821]
          "dk": 0.14,       # [0.0728]
          "dv": 0.28,       # [0.144]
          "dbias": 1.8,     # [0.949]
          "dsp": 0.0096,    # [0.00485]
          "dscale": 0.0018},  # [0.000923]
    BF16: {"out": 0.78,     # [0.394]
           "lse": 0.84,     # [0.420]
           "dq": 0.92,      # [0.462]
           "dk": 0.84,      # [0.424]
           "dv": 1.0,       # [0.518]
           "dbias": 1.2,    # [0.607]
           "dsp": 0.10,     # [0.0524]
           "dscale": 0.027},  # [0.0138]
    F16: {"out": 0.68,      # [0.342]
          "lse": 0.77,      # [0.389]
          "dq": 0.88,       # [0.444]
          "dk": 0.84,       # [0.422]
          "dv": 0.96,       # [0.484]
          "dbias": 1.7,     # [0.893]
          "dsp": 0.10,      # [0.0511]
          "dscale": 0.027},  # [0.0136]
}
CPB_C = {"bias": 0.13,     # [0.0667]
         "dw2": 0.16,      # [0.0836]
         "db1": 0.017,     # [0.00857]
         "dw1": 0.017}     # [0.00895]
# absolute error of P and s dS before their MFMAs below T's normal range: fp16 rounds into its subnormals (half the smallest,
# 2^-25); the fp32 exp2 flushes P below 2^-126 to 0 (bf16 holds fp32's exponent range)
ETA = {F32: 2.0 ** -126, BF16: 2.0 ** -126, F16: 2.0 ** -25}
SCALES = (0.5, 5.0, 30.0, 100.0, 2.0)           # per head, cycling: the clamp's ceiling and the small end


def rnd(shape, seed, scale=1.0, dt=F32):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return (torch.randn(shape, generator=g, device=DEV) * scale).to(dt)


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


class Fit:
    """Worst ratio per key and the measured c: max over elements of (|got - ref| - a ulp_T(ref)) / E."""

    def __init__(self):
        self.ratio, self.c = {}, {}

    def __call__(self, key, got, ref, E, dtype, a, c, where):
        err = (got.double() - ref).abs()
        over = (err - a * ulp(ref, dtype)).clamp_min(0)
        m = torch.where(over > 0, over / E, torch.zeros_like(over)).nan_to_num(nan=math.inf)
        if m.numel():
            self.c[key] = max(self.c.get(key, 0.0), float(m.max()))
        r = check_bound(got, ref, E, dtype, a, c, where)
        self.ratio[key] = max(self.ratio.get(key, 0.0), r)

    def report(self, title):
        print(f"\n[{title}] worst bound ratios: " + ", ".join(f"{k}={v:.3g}" for k, v in sorted(self.ratio.items())))
        print(f"[{title}] measured c: " + ", ".join(f"{k}={v:.3g}" for k, v in sorted(self.c.items())))


# ------------------------------------------------------------------------------------------------------------- window attention
def win_inputs(dt, B, res, heads, seed, device=DEV):
    """The default inputs of win_case.  device: where the generator draws (the CPU file compares this recipe with its copy of
    the one before the keyword existed, bit for bit)."""
    C = heads * 32
    N = B * res * res
    g = torch.Generator(device=device).manual_seed(seed)
    x = torch.randn((N, 3, heads, 32), generator=g, device=device)
    # q / k norms over four orders of magnitude per (token, head): cosine attention must not see them
    x[:, :2] *= 10.0 ** (torch.rand((N, 2, heads, 1), generator=g, device=device) * 4 - 2)
    qkv = nan_padded(x.reshape(N, 3 * C).to(dt), extra_rows=7)
    dout = nan_padded(torch.randn((N, C), generator=g, device=device).to(dt), extra_rows=5)
    bias = torch.rand((heads, 64, 64), generator=g, device=device) * 16
    bias[:, ::7, ::5] = 15.999                      # the top of 16 sigmoid
    bias[:, 1::9, 2::11] = 1e-3
    bias = nan_padded(bias.reshape(heads * 64, 64), extra_rows=64).view(heads, 64, 64)
    scale = nan_padded(torch.tensor([SCALES[(h + seed) % len(SCALES)] for h in range(heads)], device=device).view(heads, 1),
                       extra_rows=3).view(heads)
    return qkv, dout, bias, scale


def win_fwd_call(dt, qkv, bias, scale, out, lse, B, res, heads, shift):
    L.check(L.lib().rgbnm_window_attention_fwd(L.dt_of(dt), qkv.data_ptr(), bias.data_ptr(), scale.data_ptr(), out.data_ptr(),
                                               lse.data_ptr(), B, res, heads * 32, heads, shift, L.stream()))


def win_bwd_call(dt, qkv, out, dout, bias, dscale, scale, lse, dqkv, dbias, dsp, B, res, heads, shift, ws, wsb):
    L.check(L.lib().rgbnm_window_attention_bwd(L.dt_of(dt), qkv.data_ptr(), out.data_ptr(), dout.data_ptr(), bias.data_ptr(),
                                               L.ptr(dscale), scale.data_ptr(), lse.data_ptr(), dqkv.data_ptr(),
                                               dbias.data_ptr(), dsp.data_ptr(), B, res, heads * 32, heads, shift,
                                               ws.data_ptr(), wsb, L.stream()))


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32).clone()


def win_case(dt, B, res, heads, shift, seed, fit, seen, xcd=1, twice=False, qkv=None, dout=None, bias=None, scale=None, c=None,
             check=None):
    """One forward + backward of the window attention, checked element-wise; returns the launch classes it reached.
    qkv / dout / bias / scale: the caller's device tensors (with NaN behind them) in place of win_inputs(seed)'s, each on its own;
    c: the bound's weights per output in place of WIN_C[dt]; check: called with win_check's arguments in its place (the value
    regimes of tests/test_swin_value_regimes.py).  The defaults are the tensors and bounds from before the keywords existed."""
    C = heads * 32
    N = B * res * res
    nw = res // 8
    nwin = B * nw * nw
    where = f"window attention {NAMES[dt]} B={B} res={res} heads={heads} shift={shift} win_xcd={xcd}"
    ncu = cus()
    gf = R.geometry(ESZ[dt], "fwd", B, res, heads, ncu, xcd)
    gb = R.geometry(ESZ[dt], "bwd", B, res, heads, ncu, xcd)
    seen.update(R.classes(ESZ[dt], "fwd", gf) | R.classes(ESZ[dt], "bwd", gb))
    if qkv is None or dout is None or bias is None or scale is None:
        own = win_inputs(dt, B, res, heads, seed)
        qkv, dout, bias, scale = (o if t is None else t for t, o in zip((qkv, dout, bias, scale), own))
    out = guarded(N, C, dt)
    lse = guarded(nwin * heads * 64, None, F32)
    _, nf = launched(lambda: win_fwd_call(dt, qkv, bias, scale, out.t, lse.t, B, res, heads, shift))
    expect(nf, ("win_attn_fwd_kernel",), where + " fwd")
    out.check(where + " out")
    lse.check(where + " lse")
    wsb = L.lib().rgbnm_window_attention_bwd_workspace(B, res, heads)
    ws = guarded(wsb // 4, None, F32)
    dqkv = guarded(N, 3 * C, dt)
    dbias = guarded(heads * 4096, None, F32)
    dsp = guarded(nwin * heads, None, F32)
    dsc = guarded(heads, None, F32)

    def bwd(dscale, dsp_t):
        win_bwd_call(dt, qkv, out.t, dout, bias, dscale, scale, lse.t, dqkv.t, dbias.t, dsp_t, B, res, heads, shift, ws.t, wsb)
    _, nb = launched(lambda: bwd(dsc.t, dsp.t))
    expect(nb, ("win_attn_bwd_kernel",), where + " bwd")
    for t, nm in ((dqkv, "dqkv"), (dbias, "dbias"), (dsp, "dscale_part"), (dsc, "dscale")):
        t.check(where + " " + nm)
    ws.check(where + " workspace", written=False)
    first = (bits(dqkv.t), bits(dbias.t), bits(dsc.t))
    # dscale = NULL: the same partials, nothing else written
    dsp2 = guarded(nwin * heads, None, F32)
    dsc2 = guarded(heads, None, F32)
    bwd(None, dsp2.t)
    dsp2.check(where + " dscale_part (dscale NULL)")
    assert bool((dsc2.raw == dsc2.canary).all()), where + ": dscale written"
    assert torch.equal(bits(dsp2.t), bits(dsp.t)), where + ": dscale_part differs between dscale NULL and not"
    assert torch.equal(bits(dqkv.t), first[0]) and torch.equal(bits(dbias.t), first[1]), where + ": backward not reproducible"
    if twice:
        bwd(dsc.t, dsp.t)
        assert torch.equal(bits(dbias.t), first[1]) and torch.equal(bits(dsc.t), first[2]), where + ": d(bias) / d(scale) bits differ"
        print(f"{where}: d(bias) and d(scale) identical bits over two launches")
    ws.check(where + " workspace", written=False)
    if check is not None:
        check(dt, B, res, heads, shift, qkv, dout, bias, scale, out, lse, dqkv, dbias, dsp, dsc, gb, fit, where)
    else:
        win_check(dt, B, res, heads, shift, qkv, dout, bias, scale, out, lse, dqkv, dbias, dsp, dsc, gb, fit, where, c)
    return R.classes(ESZ[dt], "fwd", gf) | R.classes(ESZ[dt], "bwd", gb)


def win_check(dt, B, res, heads, shift, qkv, dout, bias, scale, out, lse, dqkv, dbias, dsp, dsc, gb, fit, where, c=None):
    C = heads * 32
    nw = res // 8
    nwin = B * nw * nw
    uT = KC.U_OF[dt]
    uP = 0.0 if dt == F32 else uT
    cw = WIN_C[dt] if c is None else c
    k = NAMES[dt]
    qkv_w, dout_w = R.partition(qkv, B, res, shift), R.partition(dout, B, res, shift)
    out_w, dqkv_w = R.partition(out.t, B, res, shift), R.partition(dqkv.t, B, res, shift)
    lse_k = lse.t.view(nwin, heads, 64)
    dsp_k = dsp.t.view(nwin, heads)
    b64, s64 = bias.double(), scale.double()
    db_ref = torch.zeros(heads, 64, 64, dtype=torch.float64, device=qkv.device)
    db_E, db_abs = torch.zeros_like(db_ref), torch.zeros_like(db_ref)
    dsp_ref, dsp_E, dsp_mag = [], [], []
    per = max(1, (1 << 24) // (nw * nw * heads * 4096))      # images per chunk: 128 MB per [windows, heads, 64, 64] fp64 tensor
    for b0 in range(0, B, per):
        nimg = min(per, B - b0)
        w0, w1 = b0 * nw * nw, (b0 + nimg) * nw * nw
        tag = f"{where} windows {w0}..{w1 - 1}, element (window - {w0}, head, query, d)"
        x = qkv_w[w0:w1].double()
        q, kk, v = (R.split_heads(x[..., i * C:(i + 1) * C], heads) for i in range(3))
        mask = R.window_mask(res, shift, nimg, qkv.device)
        Lg, o_ref, lse_ref, P, E_out, E_lse = R.win_fwd(q, kk, v, b64, s64, mask, uT, uP, ETA[dt])
        O_k = R.split_heads(out_w[w0:w1], heads)
        fit(k + "-out", O_k, o_ref, E_out, dt, 1, cw["out"], tag + " out")
        fit(k + "-lse", lse_k[w0:w1], lse_ref, E_lse, F32, 1, cw["lse"], tag + " lse (window, head, query)")
        del P, E_out, o_ref
        dO = R.split_heads(dout_w[w0:w1].double(), heads)
        r = R.win_bwd(Lg, v, dO, O_k.double(), lse_k[w0:w1].double(), uT, uP, ETA[dt])
        dw = dqkv_w[w0:w1]
        for i, nm in enumerate(("dq", "dk", "dv")):
            fit(k + "-" + nm, R.split_heads(dw[..., i * C:(i + 1) * C], heads), r[nm], r["E_" + nm], dt, 1, cw[nm],
                tag + " " + nm)
        fit(k + "-dsp", dsp_k[w0:w1], r["dsp"], r["E_dsp"], F32, 1, cw["dsp"], tag + " dscale_part (window, head)")
        db_ref += r["dS"].sum(0)
        db_E += r["E_dS"].sum(0)
        db_abs += r["absdS"].sum(0)
        dsp_ref.append(r["dsp"])
        dsp_E.append(r["E_dsp"])
        dsp_mag.append(r["mdsp"])
        del r, Lg
    S = gb["slots"] * gb["waves"]
    fit(k + "-dbias", dbias.t.view(heads, 64, 64), db_ref, db_E + (gb["wpw_max"] + S) * U * db_abs, F32, 1, cw["dbias"],
        where + " dbias (head, query, key)")
    dsp_ref, dsp_E, dsp_mag = torch.cat(dsp_ref), torch.cat(dsp_E), torch.cat(dsp_mag)
    fit(k + "-dscale", dsc.t, dsp_ref.sum(0), dsp_E.sum(0) + nwin * U * dsp_mag.sum(0), F32, 1, cw["dscale"],
        where + " dscale (head)")


def win_cases(ncu):
    """(B, res, heads, shift, win_xcd): res 8 / 16 / 24 / 32 / 64, heads 1 / 3 / 6 / 12 / 24, shift 0 / 2 / 4 / 7."""
    return [(1, 8, 3, 0, 1),            # one window, three idle forward waves: (a)
            (1, 8, 6, 4, 1),            # the one window is masked
            (2, 16, 1, 0, 1),           # eight windows, eight waves: (b)
            (2, 24, 6, 4, 1),           # three windows per side
            (3, 24, 3, 2, 1),           # shift 2
            (2, 32, 12, 7, 1),          # shift 7
            (4, 64, 24, 4, 1),          # head-major, >= 3 windows per wave, ragged: (c)
            (16, 64, 3, 0, 1),          # XCD-aware map, multi-window waves: (d)
            (16, 64, 3, 4, 0)]          # the same launch head-major


@pytest.mark.parametrize("dt", DTS3)
def test_window_attention_edges(option, dt):
    """rgbnm_window_attention_fwd / _bwd element-wise at the launch classes (a)-(e) of the persistent window walk."""
    fit = Fit()
    seen = set()
    for i, (B, res, heads, shift, xcd) in enumerate(win_cases(cus())):
        option("win_xcd", xcd)
        win_case(dt, B, res, heads, shift, 700 + 10 * i, fit, seen, xcd)
    option("win_xcd", 1)
    fit.report(f"window attention {NAMES[dt]}")
    want = {"a", "b", "c", "d"} | ({"e"} if dt == F32 else set())
    print(f"[window attention {NAMES[dt]}] launch classes reached: {sorted(seen)}")
    assert want <= seen, (NAMES[dt], sorted(want - seen))


def test_window_attention_bench_stage1(option):
    """bf16 at the benchmark's stage-1 geometry (B = 256, res 64, heads 3: about 24 windows per forward wave), reference in
    window chunks; the backward twice: identical d(bias) and d(scale) bits."""
    option("win_xcd", 1)
    fit = Fit()
    seen = set()
    win_case(BF16, 256, 64, 3, 4, 990, fit, seen, 1, twice=True)
    fit.report("window attention bf16 B=256 stage 1")
    print(f"[window attention bf16 B=256] launch classes reached: {sorted(seen)}")
    assert "d" in seen


# ------------------------------------------------------------------------------------------------------------- LayerNorm rows
LPR = {96: 8, 192: 16, 384: 32, 768: 64}


@pytest.mark.parametrize("dt", DTS3)
@pytest.mark.parametrize("E", [96, 192, 384, 768])
def test_ln_rows_stage_widths_past_grid_caps(option, dt, E):
    """ln_rows_fwd_kernel / ln_rows_bwd_kernel (option ln_rows) at the four SwinV2 stage widths: G = 256 / lanes-per-row rows
    per workgroup pass; M = 1, G - 1, G + 1, 2048 G + 1 (the backward grid takes two row passes per workgroup) and 8192 G + 1
    (the forward grid cap of 8192 workgroups: two passes; the backward five)."""
    option("ln_rows", 1)
    worst = KC.Worst()
    G = 256 // LPR[E]
    rows = [1, G - 1, G + 1, 2048 * G + 1, 8192 * G + 1]
    fwd_pass = [-(-(-(-M // G)) // min(-(-M // G), 8192)) for M in rows]
    bwd_pass = [-(-(-(-M // G)) // 2048) for M in rows]
    assert max(fwd_pass) >= 2 and max(bwd_pass) >= 2, (fwd_pass, bwd_pass)
    for i, M in enumerate(rows):
        ln_case(dt, M, E, False, i % 2, 1500 + 10 * i + E, worst, f"rows-{E}", generic=True, res_on=(i % 2 == 0),
                ss_on=(i % 3 != 1), want=("ln_rows_fwd_kernel", "ln_rows_bwd_kernel"))
    worst.report(f"ln_rows {NAMES[dt]} E={E}")


# ------------------------------------------------------------------------------------------------------------- position bias
def cpb_consts():
    blk = SW.SwinTransformerBlock(96, (16, 16), 3, 8, 0, 0.0, device=DEV)
    a = blk.attn
    idx = a.relative_position_index.view(-1)
    return (a.relative_coords_table.detach().reshape(-1, 2).float().contiguous(), idx.to(torch.int32).contiguous(),
            SW.inverse_index(idx, 225).contiguous())


def cpb_case(heads, seed, fit, span=None, ls_low=()):
    """span: W2 of every block rescaled so that its table spans +-span (saturation of 16 sigmoid; the bias must then be exactly
    0.0 / 16.0 where the fp32 rounding of the fp64 value is, nothing may be NaN, and d(table) exactly 0 where 16 s (1 - s) rounds
    to 0 in fp32); ls_low: blocks whose logit_scale is -20.  Returns the number of (exactly 0, exactly 16) bias elements."""
    n = len(heads)
    coords, index, inv = cpb_consts()
    where = f"position bias {n} blocks" + (f" span {span}" if span else "")
    sat = [0, 0]
    lib = L.lib()
    P, O = [], []
    for i, h in enumerate(heads):
        s = seed + 10 * i
        w1, b1, w2 = rnd((512, 2), s), rnd((512,), s + 1, 0.5), rnd((h, 512), s + 2, 0.1)
        ls = torch.rand(h, device=DEV, generator=torch.Generator(device=DEV).manual_seed(s + 3)) * 4 + 1.5   # some > ln 100
        ls[ls.sub(math.log(100.0)).abs() < 1e-3] += 2e-3
        if i in ls_low:
            ls[:] = -20.0
        if span:
            t0 = (ST.coords_table(8).double().reshape(-1, 2).to(DEV) @ w1.double().T + b1.double()).clamp_min(0) @ w2.double().T
            w2 = (w2.double() * (span / t0.abs().amax(0))[:, None]).float()          # per head: max |table| = span
        dbias, dscale = rnd((h, 4096), s + 4), rnd((h,), s + 5)
        P.append([nan_padded(t.view(t.shape[0], -1) if t.dim() > 1 else t.view(-1, 1), extra_rows=3) for t in
                  (w1, b1, w2, ls, dbias, dscale)])
        O.append({nm: guarded(m, None, F32) for nm, m in (("bias", h * 4096), ("scale", h), ("dw1", 1024), ("db1", 512),
                                                           ("dw2", h * 512), ("dls", h))})
    te = lib.rgbnm_swin_cpb_table_elems(n)
    table, dtable = guarded(te, None, F32), guarded(te, None, F32)
    blocks = (L.CpbBlock * n)()
    for i, h in enumerate(heads):
        w1, b1, w2, ls, dbias, dscale = P[i]
        o = O[i]
        blocks[i] = L.CpbBlock(w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), ls.data_ptr(), o["bias"].t.data_ptr(),
                               o["scale"].t.data_ptr(), dbias.data_ptr(), dscale.data_ptr(), o["dw1"].t.data_ptr(),
                               o["db1"].t.data_ptr(), o["dw2"].t.data_ptr(), o["dls"].t.data_ptr(), h, 0)
    _, nf = launched(lambda: L.check(lib.rgbnm_swin_cpb_fwd(blocks, n, coords.data_ptr(), index.data_ptr(), table.t.data_ptr(),
                                                             L.stream())))
    _, nb = launched(lambda: L.check(lib.rgbnm_swin_cpb_bwd(blocks, n, coords.data_ptr(), inv.data_ptr(), table.t.data_ptr(),
                                                             dtable.t.data_ptr(), L.stream())))
    chunks = -(-n // 16)
    for names, kern in ((nf, "cpb_table_kernel"), (nf, "cpb_bias_kernel"), (nb, "cpb_dtable_kernel"), (nb, "cpb_mlp_bwd_kernel")):
        cnt = sum(1 for x in names if kern in x)
        assert cnt == chunks, (where, kern, cnt, chunks)
    table.check(where + " table", written=False)
    dtable.check(where + " dtable", written=False)
    # the oracle's own table and index, fp64
    tab = ST.coords_table(8).double().reshape(-1, 2).to(DEV)
    pidx = ST.position_index(8).reshape(-1).to(DEV)
    for i, h in enumerate(heads):
        w1, b1, w2, ls, dbias, dscale = (t.double().reshape(-1) for t in P[i])
        w1, w2, dbias = w1.view(512, 2), w2.view(h, 512), dbias.view(h, 4096)
        o = O[i]
        tg = f"{where}: block {i} (heads {h})"
        for nm, g in o.items():
            g.check(tg + " " + nm)
        pre = tab @ w1.T + b1
        Hm = tab.abs() @ w1.abs().T + b1.abs()
        hid = pre.clamp_min(0)
        t = hid @ w2.T                                          # [225, h]
        E_t = 18 * U * (Hm @ w2.abs().T)
        sg = torch.sigmoid(t)
        ea = torch.exp(-t.abs())
        d1 = 16 * ea / (1 + ea) ** 2                            # 16 s (1 - s) without the cancellation of 1 - s beyond t = 37
        bias_ref = (16 * sg)[pidx].T                            # [h, 4096]
        E_b = (d1 * E_t + 4 * U * 16 * sg)[pidx].T
        fit("bias", o["bias"].t.view(h, 4096), bias_ref, E_b, F32, 1, CPB_C["bias"], tg + " bias (head, position)")
        if span:
            got_b = o["bias"].t.view(h, 4096)
            assert float(t.abs().max()) > 0.999 * span and all(bool(torch.isfinite(g.t).all()) for g in o.values()), tg
            for v_, j in ((0.0, 0), (16.0, 1)):
                at = bias_ref.float() == v_
                assert bool((got_b[at] == v_).all()), f"{tg}: bias not exactly {v_} where fp32 rounds there"
                sat[j] += int(at.sum())
            dtk = dtable.t.view(-1, 24, 225)[i, :h].T                  # scratch of the backward: d table [225, h]
            flat = (16 * torch.exp(-t.abs())).float() == 0             # 16 s (1 - s) = 16 e^-|t| (1 + e^-|t|)^-2 rounds to 0 in fp32: |t| > 106.7
            assert bool((dtk[flat] == 0).all()) and int(flat.sum()) > 0, f"{tg}: d(table) not exactly 0 at saturation"
        sc_ref = torch.exp(ls.clamp(max=math.log(100.0)))
        fit("scale", o["scale"].t, sc_ref, 4 * U * sc_ref, F32, 1, 1.0, tg + " scale (head)")
        Gs = torch.zeros(225, h, dtype=torch.float64, device=DEV).index_add_(0, pidx, dbias.T)
        Gm = torch.zeros(225, h, dtype=torch.float64, device=DEV).index_add_(0, pidx, dbias.abs().T)
        dt_ = d1 * Gs
        E_dt = d1 * 64 * U * Gm + Gs.abs() * (d1 * (1 - 2 * sg)).abs() * E_t + 4 * U * dt_.abs()
        dh = dt_ @ w2                                          # [225, 512]
        E_dh = E_dt @ w2.abs() + 24 * U * (dt_.abs() @ w2.abs())
        dw2_ref = dt_.T @ hid
        E_dw2 = E_dt.T @ hid + dt_.abs().T @ (2 * U * Hm) + 40 * U * (dt_.abs().T @ hid)
        fit("dw2", o["dw2"].t.view(h, 512), dw2_ref, E_dw2, F32, 1, CPB_C["dw2"], tg + " dw2 (head, hidden)")
        on = (pre > 0).double()
        db1_ref = (dh * on).sum(0)
        E_db1 = (E_dh * on).sum(0) + 40 * U * (dh.abs() * on).sum(0)
        fit("db1", o["db1"].t, db1_ref, E_db1, F32, 1, CPB_C["db1"], tg + " db1 (hidden)")
        dw1_ref = (dh * on).T @ tab                            # [512, 2]
        E_dw1 = (E_dh * on).T @ tab.abs() + 40 * U * ((dh.abs() * on).T @ tab.abs())
        fit("dw1", o["dw1"].t.view(512, 2), dw1_ref, E_dw1, F32, 1, CPB_C["dw1"], tg + " dw1 (hidden, coordinate)")
        inside = ls <= math.log(100.0)
        dls_ref = torch.where(inside, dscale * torch.exp(ls), torch.zeros_like(ls))
        fit("dls", o["dls"].t, dls_ref, 4 * U * dls_ref.abs(), F32, 1, 1.0, tg + " dls (head)")
        assert bool((o["dls"].t[~inside] == 0).all()), tg + ": d(logit_scale) beyond ln 100 not exactly 0"
    return tuple(sat)


def test_position_bias_at_model_block_counts():
    """rgbnm_swin_cpb_fwd / _bwd on the 12 blocks of SwinV2-T (heads 3, 3, 6, 6, 12 x 6, 24, 24) and on 17 blocks (chunks of
    16 and 1), every output guarded, scratch of exactly rgbnm_swin_cpb_table_elems(n) elements, element-wise against fp64 of
    oracle/swin_torch's coords_table / position_index."""
    fit = Fit()
    swin_t = [3, 3, 6, 6] + [12] * 6 + [24, 24]
    cpb_case(swin_t, 2000, fit)
    cpb_case(swin_t + [3, 6, 12, 24, 1], 3000, fit)
    fit.report("position bias")


# ------------------------------------------------------------------------------------------------------------- merge / mean
def merge_ref(x, B, res, C):
    xr = x.reshape(B, res, res, C)
    return torch.cat([xr[:, 0::2, 0::2], xr[:, 1::2, 0::2], xr[:, 0::2, 1::2], xr[:, 1::2, 1::2]], -1).reshape(-1, 4 * C)


def scatter_ref(y, B, res, C):
    y4 = y.reshape(B, res // 2, res // 2, 4 * C)
    z = torch.empty(B, res, res, C, dtype=y.dtype, device=y.device)
    z[:, 0::2, 0::2], z[:, 1::2, 0::2] = y4[..., :C], y4[..., C:2 * C]
    z[:, 0::2, 1::2], z[:, 1::2, 1::2] = y4[..., 2 * C:3 * C], y4[..., 3 * C:]
    return z.reshape(B * res * res, C)


@pytest.mark.parametrize("dt", DTS3)
def test_merge_gather_both_directions_bit_exact(dt):
    """rgbnm_merge_gather at (256, 64, 96) -- 8192 workgroups walk the grid-stride loop 12 times -- (3, 32, 192) and (1, 2, 4)."""
    for i, (B, res, C) in enumerate([(256, 64, 96), (3, 32, 192), (1, 2, 4)]):
        where = f"merge_gather {NAMES[dt]} B={B} res={res} C={C}"
        x = nan_padded(rnd((B * res * res, C), 40 + i, 1.0, dt), extra_rows=3)
        out = guarded(B * (res // 2) ** 2, 4 * C, dt)
        _, names = launched(lambda: L.check(L.lib().rgbnm_merge_gather(L.dt_of(dt), x.data_ptr(), out.t.data_ptr(), B, res, C, 0,
                                                                      L.stream())))
        expect(names, ("merge_gather_kernel",), where)
        out.check(where + " out")
        assert torch.equal(bits(out.t), bits(merge_ref(x, B, res, C))), where
        y = nan_padded(rnd((B * (res // 2) ** 2, 4 * C), 50 + i, 1.0, dt), extra_rows=3)
        back = guarded(B * res * res, C, dt)
        _, names = launched(lambda: L.check(L.lib().rgbnm_merge_gather(L.dt_of(dt), y.data_ptr(), back.t.data_ptr(), B, res, C,
                                                                      1, L.stream())))
        expect(names, ("merge_gather_kernel",), where + " inverse")
        back.check(where + " inverse")
        assert torch.equal(bits(back.t), bits(scatter_ref(y, B, res, C))), where + " inverse"


@pytest.mark.parametrize("dt", DTS3)
def test_token_mean_paths(dt):
    """rgbnm_token_mean forward / backward: the bench shape N = 64, C = 768 (bf16 / fp16: two row groups; fp32: one), C / EPV > 256
    (the multi-pass loop), C not a multiple of the 16-byte vector (scalar kernels), N = 1."""
    worst = KC.Worst()
    epv = 16 // ESZ[dt]
    cases = [(4, 64, 768), (3, 5, epv * 258), (2, 7, 770), (3, 1, 768), (2, 65, 8 * epv)]
    for i, (B, N, C) in enumerate(cases):
        vec = C % epv == 0
        nvec = C // epv
        if (N, C) == (64, 768):
            assert (256 // nvec if nvec < 256 else 1) == (2 if dt != F32 else 1)
        where = f"token_mean {NAMES[dt]} B={B} N={N} C={C}"
        x = nan_padded(rnd((B * N, C), 60 + i, 1.0, dt), extra_rows=3)
        y = guarded(B, C, dt)
        _, names = launched(lambda: L.check(L.lib().rgbnm_token_mean(L.dt_of(dt), x.data_ptr(), y.t.data_ptr(), B, N, C, 0,
                                                                    L.stream())))
        kf = "token_mean_fwd_kernel" if vec else "token_mean_fwd_scalar_kernel"
        expect(names, (kf,), where, forbid=("token_mean_fwd_scalar_kernel",) if vec else ("token_mean_fwd_kernel",))
        y.check(where + " y")
        x64 = x.double().view(B, N, C)
        worst("fwd", check_bound(y.t, x64.mean(1), x64.abs().mean(1), dt, 1, N * U, where + " y (image, column)"))
        dy = nan_padded(rnd((B, C), 70 + i, 1.0, dt), extra_rows=3)
        dx = guarded(B * N, C, dt)
        _, names = launched(lambda: L.check(L.lib().rgbnm_token_mean(L.dt_of(dt), dy.data_ptr(), dx.t.data_ptr(), B, N, C, 1,
                                                                    L.stream())))
        kb = "token_mean_bwd_kernel" if vec else "token_mean_bwd_scalar_kernel"
        expect(names, (kb,), where, forbid=("token_mean_bwd_scalar_kernel",) if vec else ("token_mean_bwd_kernel",))
        dx.check(where + " dx")
        ref = (dy.double() / N)[:, None, :].expand(B, N, C).reshape(B * N, C)
        worst("bwd", check_bound(dx.t, ref, ref.abs(), dt, 1, N * U, where + " dx (row, column)"))
    worst.report(f"token_mean {NAMES[dt]}")


# ------------------------------------------------------------------------------------------------------------- embedding
EMBED_MARKS = {"float": F32, "f": F32, "__bf16": BF16, "DF16b": BF16, "_Float16": F16, "DF16_": F16}


def embed_instantiation(names):
    """(TI, TO) of the one swin_embed_kernel a call dispatched, from the demangled or the mangled name."""
    import re
    hits = [n for n in names if "swin_embed_kernel" in n]
    assert len(hits) == 1 and len(names) == 1, sorted(set(names))
    m = (re.search(r"swin_embed_kernel<\s*([\w ]+?)\s*,\s*([\w ]+?)\s*>", hits[0])
         or re.search(r"swin_embed_kernelI(f|DF16b|DF16_)(f|DF16b|DF16_)E", hits[0]))
    assert m, hits[0]
    return EMBED_MARKS[m.group(1)], EMBED_MARKS[m.group(2)]


def embed_call(y, c, Ay, Ac, to, B, Hb, Wb, where):
    """One launch on inputs with NaN behind them, into a guarded [B 2Hb 2Wb, 24] output."""
    yb = nan_padded(y.reshape(-1, 64), None, 7)
    cb = nan_padded(c.reshape(-1, 64), None, 7)
    out = guarded(B * 4 * Hb * Wb, 24, to)
    rc, names = launched(lambda: L.lib().rgbnm_swin_embed(L.dt_of(y.dtype), L.dt_of(to), yb.data_ptr(), cb.data_ptr(),
                                                          Ay.data_ptr(), Ac.data_ptr(), out.t.data_ptr(), B, Hb, Wb, L.stream()))
    L.check(rc, where)
    assert embed_instantiation(names) == (y.dtype, to), (where, names)
    out.check(where)                                       # margins intact, every (token, feature) element written
    return out.t.reshape(B, 2 * Hb, 2 * Wb, 24)


@pytest.mark.parametrize("to", DTS3, ids=lambda t: "out-" + NAMES[t])
@pytest.mark.parametrize("ti", DTS3, ids=lambda t: "in-" + NAMES[t])
def test_swin_embed_edges(ti, to):
    """swin_embed_kernel, all nine in / out type pairs, at grids with Hb != Wb (the token arithmetic takes H and W apart, for luma
    and for chroma) and block counts that fill the last workgroup (4 blocks each) and leave it half empty: every element within
    ulp_TO(ref) + EMBED_C u mag of the fp64 result of the TI-rounded inputs (swin_ref.py derives EMBED_C = 16.0000114).
    Worst ratio measured on one MI355X: 0.201 into fp32 (0.173 / 0.185 / 0.201 from fp32 / bf16 / fp16), 0.500 into bf16 and
    0.499 into fp16 (the store's half ulp); the eleven embedding tests take 2 s."""
    worst = KC.Worst()
    Ay, Ac = (a.float().to(DEV) for a in R.embed_matrices())
    for i, (B, Hb, Wb) in enumerate(R.EMBED_CASES):
        y, c = (t.to(DEV).to(ti) for t in R.embed_inputs(B, Hb, Wb, 50 + 2 * i))
        where = f"swin_embed {NAMES[ti]}->{NAMES[to]} B={B} Hb={Hb} Wb={Wb}"
        got = embed_call(y, c, Ay, Ac, to, B, Hb, Wb, where)
        ref, mag = R.embed_ref(y, c, Ay, Ac)
        worst(f"{NAMES[ti]}->{NAMES[to]}", check_bound(got, ref, mag, to, 1, R.EMBED_C * U, where))
    worst.report("swin_embed")


@pytest.mark.parametrize("B,Hb,Wb", [(1, 2, 6), (2, 6, 2)])
def test_swin_embed_single_coefficient_probes(B, Hb, Wb):
    """One non-zero coefficient in one block, luma and each chroma channel, on non-square grids: it reaches exactly the tokens and
    features the einops split dictates -- the non-zero pattern is the reference's -- and nothing else is non-zero."""
    Ay, Ac = (a.float().to(DEV) for a in R.embed_matrices())
    b = B - 1
    probes = [("luma", 0, (b, 0, Hb - 1, Wb - 2, 3, 5)), ("luma-dc", 0, (b, 0, 1, 0, 0, 0)),
              ("cb", 1, (b, 0, Hb // 2 - 1, Wb // 2 - 1, 5, 2)), ("cr", 1, (b, 1, 0, Wb // 2 - 1, 6, 7))]
    for name, which, at in probes:
        y = torch.zeros(B, 1, Hb, Wb, 8, 8, device=DEV)
        c = torch.zeros(B, 2, Hb // 2, Wb // 2, 8, 8, device=DEV)
        (y, c)[which][at] = 1.0
        where = f"swin_embed probe {name} B={B} Hb={Hb} Wb={Wb} at {at}"
        got = embed_call(y, c, Ay, Ac, F32, B, Hb, Wb, where)
        ref, mag = R.embed_ref(y, c, Ay, Ac)
        sub = 2 if which == 0 else 4
        assert int((ref != 0).sum()) == 64 and int((ref != 0).any(-1).sum()) == sub * sub, where       # (the probe's own reach)
        assert torch.equal(got != 0, ref != 0), f"{where}: non-zero pattern differs from the einops split's"
        check_bound(got, ref, mag, F32, 1, R.EMBED_C * U, where)
