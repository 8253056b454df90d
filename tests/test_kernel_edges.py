"""Element-wise edge tests of the GEMM, attention and LayerNorm kernels (tests/kernel_check.py).

Every case writes into canary-filled guarded outputs (margins, ld gaps and unwritten elements are checked bit-wise), reads
inputs whose ld gaps and trailing rows are NaN, gets a workspace of exactly the size its *_workspace() entry returns, and is
checked element by element against an fp64 reference of the T-rounded inputs:  |got - ref| <= ulp_T(ref) + c_u mag [+ the
terms named at the case].  Each case also asserts the device kernel it was meant to reach (torch.profiler), so a shape that
falls off its path fails.  Shapes walk each path's tile edges; the worst bound ratio per (path, dtype) is printed (-s).

Terms beyond ulp_T(ref) + k u mag, each where the code rounds or approximates:
- inter: the 16-bit staged epilogues round acc + bias [+ pos] to T before the residual / product / activation (gemm.hip,
  pass 1 `store4<T>(Cs ...)`; gemm_nt_small.hip `(float)(bf16)v[e]`; the row-panel and weight-resident kernels give the same
  bits): + ulp_T(pre) times the epilogue's sensitivity to it.
- GELU: the pre-activation is rounded to T on every path (gemm.hip direct epilogue `to_f32(from_f32<T>(v))`): + 1.13 ulp_T(pre)
  for gelu (max |gelu'| = 1.13), + 0.8 ulp_T(pre) for gelu' (max |gelu''| = 2 phi(0) = 0.80); the erf of common.h (A&S 7.1.26,
  |err| <= 1.5e-7) or erff: + 2^-22 |pre| (gelu), 2^-21 (gelu'), + 2 fp32 ulps of the result.
- tanh / (1 - h^2): tanhf + 2 fp32 ulps; 1 - h*h in fp32: + 2^-23 |pre|.
"""
import math

import pytest
import torch

import kernel_check as KC
from kernel_check import U, guarded, nan_padded, check_bound, launched, ran, ulp
from rgb_no_more_amd import lib as L
from test_hip_kernels import option  # noqa: F401  (fixture: set a runtime switch for one test)

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
DTS3 = [F32, BF16, F16]
NAMES = {F32: "f32", BF16: "bf16", F16: "f16"}
E_NONE, E_RES, E_GELU, E_POS, E_DGELU, E_TANH, E_DTANH = range(7)
EPI_NAMES = ["none", "res", "gelu", "pos", "dgelu", "tanh", "dtanh"]
SQRT1_2 = 1.0 / math.sqrt(2.0)


def rnd(shape, seed, scale=1.0, dt=F32):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return (torch.randn(shape, generator=g, device=DEV) * scale).to(dt)


def u32(x):
    return 2.0 * ulp(x, F32)


def gelu64(x):
    return 0.5 * x * (1.0 + torch.special.erf(x * SQRT1_2))


def dgelu64(x):
    return 0.5 * (1.0 + torch.special.erf(x * SQRT1_2)) + x * torch.exp(-0.5 * x * x) / math.sqrt(2 * math.pi)


def expect(names, want, where, forbid=()):
    for w in want:
        ws = w if isinstance(w, tuple) else (w,)
        assert ran(names, *ws), f"{where}: kernel {ws} did not run; ran {sorted(set(names))}"
    for f in forbid:
        assert not ran(names, f), f"{where}: kernel {f} ran; ran {sorted(set(names))}"


# ------------------------------------------------------------------------------------------------------------- GEMM NT
def nt_case(dt, epi, M, N, K, *, c_f32=False, pad=False, inter=False, seed=1, want=("gemm_nt_kernel",), forbid=(),
            worst=None, key=""):
    lda, ldw, ldc, ldr, ldc2 = (K + 16, K + 24, N + 8, N + 16, N + 24) if pad else (K, K, N, N, N)
    A = nan_padded(rnd((M, K), seed, 1.0, dt), lda, 3)
    W = nan_padded(rnd((N, K), seed + 1, 0.1, dt), ldw, 3)
    bias = None if epi in (E_DGELU, E_DTANH) or (epi == E_NONE and seed % 2) else rnd((N,), seed + 2, 0.5)
    R = None
    if epi in (E_RES, E_DGELU):
        R = nan_padded(rnd((M, N), seed + 3, 1.0, dt), ldr, 3)
    elif epi == E_DTANH:
        R = nan_padded(torch.tanh(rnd((M, N), seed + 3, 1.5)).to(dt), ldr, 3)
    period = 7
    pos = rnd((period, N), seed + 4, 0.5) if epi == E_POS else None
    odt = F32 if c_f32 else dt
    C = guarded(M, N, odt, ldc)
    C2 = guarded(M, N, dt, ldc2) if epi == E_GELU else None

    def call():
        L.check(L.lib().rgbnm_gemm_nt(L.dt_of(dt), epi, A.data_ptr(), lda, W.data_ptr(), ldw, C.t.data_ptr(), ldc, L.ptr(bias),
                                      L.ptr(R), ldr, C2.t.data_ptr() if C2 else None, ldc2, L.ptr(pos), period, M, N, K,
                                      int(c_f32), L.stream()))
    _, names = launched(call)
    where = f"gemm_nt {NAMES[dt]} {EPI_NAMES[epi]} M={M} N={N} K={K} c_f32={int(c_f32)} pad={int(pad)}"
    expect(names, want, where, forbid)
    C.check(where)
    if C2:
        C2.check(where + " C2")
    A64, W64 = A.double(), W.double()
    pre = A64 @ W64.T
    mag = A64.abs() @ W64.abs().T
    del A64, W64
    if bias is not None:
        pre += bias.double()
        mag += bias.double().abs()
    if pos is not None:
        pp = pos.double()[torch.arange(M, device=DEV) % period]
        pre += pp
        mag += pp.abs()
    inter = inter and not c_f32 and dt != F32
    extra = None
    if epi in (E_NONE, E_POS):
        ref = pre
    elif epi == E_RES:
        r = R.double()
        ref = pre + r
        mag += r.abs()
        extra = ulp(pre, dt) if inter else None
    elif epi == E_DGELU:
        r = R.double()
        ref = pre * r
        mag *= r.abs()
        extra = ulp(pre, dt) * r.abs() if inter else None
    elif epi == E_TANH:
        ref = torch.tanh(pre)
        extra = u32(ref) + (ulp(pre, dt) if inter else 0)
    elif epi == E_DTANH:
        h = R.double()
        f = 1 - h * h
        ref = pre * f
        mag *= f.abs()
        extra = pre.abs() * 2.0 ** -23 + (ulp(pre, dt) * f.abs() if inter else 0)
    else:
        ref = gelu64(pre)
        ref2 = dgelu64(pre)
        up = ulp(pre, dt)
        r2 = check_bound(C2.t, ref2, 0.8 * mag, dt, 1, K * U, where + " C2", extra=0.8 * up + 2.0 ** -21 + u32(ref2),
                         tile=(128, 192 if N % 192 == 0 else 128))
        if worst is not None:
            worst(key, r2)
        extra = 1.13 * up + 2.0 ** -22 * pre.abs() + u32(ref)
        mag *= 1.13
    r = check_bound(C.t, ref, mag, odt, 1, K * U, where, extra=extra, tile=(128, 192 if N % 192 == 0 else 128))
    if worst is not None:
        worst(key, r)
    return C, C2


def nt_generic_opts(option, staged):
    option("nt_small", 0)
    option("nt_kpipe", 0)
    option("nt_wres", 0)
    option("nt_staged", staged)


@pytest.mark.parametrize("dt,staged", [(F32, 0), (BF16, 0), (BF16, 1), (F16, 0), (F16, 1)])
def test_gemm_nt_generic_tile_edges(option, dt, staged):
    """gemm_nt_kernel: 128-row tiles x 128 (NB = 2) or 192 (NB = 3, N % 192 == 0) columns; K walks the 64-element (16-bit) /
    32-element (fp32) k-tile.  All seven epilogues at every shape, the fp32-output mode, padded strides."""
    nt_generic_opts(option, staged)
    worst = KC.Worst()
    inter = bool(staged)
    shapes = [(m, 192, 64) for m in (1, 127, 128, 129)]
    shapes += [(129, n, 64) for n in (8, 120, 128, 136, 184, 192, 200, 1000)]
    shapes += [(129, 200, k) for k in (8, 56, 64, 72, 1000)]
    shapes += [(257, 1000, 72), (1, 8, 8), (255, 136, 1000)]            # all-ragged corners
    if dt == F32:
        shapes += [(129, 200, 4), (129, 192, 12)]
    for i, (M, N, K) in enumerate(shapes):
        for epi in range(7):
            nt_case(dt, epi, M, N, K, inter=inter, seed=10 * i + epi, worst=worst, key=f"{EPI_NAMES[epi]}")
        if dt != F32:
            nt_case(dt, E_NONE, M, N, K, c_f32=True, seed=7 * i, worst=worst, key="none-c_f32")
    for epi in range(7):
        nt_case(dt, epi, 129, 200, 72, pad=True, inter=inter, seed=500 + epi, worst=worst, key=EPI_NAMES[epi])
        nt_case(dt, epi, 257, 192, 64, pad=True, inter=inter, seed=600 + epi, worst=worst, key=EPI_NAMES[epi])
        if dt != F32:
            nt_case(dt, epi, 129, 192, 64, c_f32=True, pad=bool(epi % 2), seed=700 + epi, worst=worst, key="c_f32")
    worst.report(f"gemm_nt generic {NAMES[dt]} staged={staged}")


def test_gemm_nt_small_m_tile_edges(option):
    """gemm_nt_small_kernel (bf16, M <= 512, N % 4 == 0): 32 x 32 tiles; none / tanh / (1 - h^2) with bf16 and fp32
    outputs; the epilogues it does not take and M = 513 fall back to the generic kernel."""
    nt_generic_opts(option, 1)
    option("nt_small", 1)
    worst = KC.Worst()
    shapes = [(m, 1000, 72) for m in (1, 31, 32, 33, 511, 512)] + [(33, 4, 8), (77, 36, 1000), (32, 1000, 192)]
    for i, (M, N, K) in enumerate(shapes):
        for epi in (E_NONE, E_TANH, E_DTANH):
            for c_f32 in (False, True):
                nt_case(BF16, epi, M, N, K, c_f32=c_f32, inter=True, seed=30 * i + epi, want=("gemm_nt_small_kernel",),
                        forbid=("gemm_nt_kernel",), worst=worst, key=f"{EPI_NAMES[epi]}-c_f32={int(c_f32)}")
    for epi in (E_NONE, E_TANH, E_DTANH):
        nt_case(BF16, epi, 33, 1000, 72, pad=True, inter=True, seed=900 + epi, want=("gemm_nt_small_kernel",),
                worst=worst, key=EPI_NAMES[epi])
    nt_case(BF16, E_RES, 33, 192, 72, inter=True, seed=950, want=("gemm_nt_kernel",), forbid=("gemm_nt_small_kernel",))
    nt_case(BF16, E_NONE, 513, 192, 72, inter=True, seed=951, want=("gemm_nt_kernel",), forbid=("gemm_nt_small_kernel",))
    worst.report("gemm_nt small-M bf16")


WRES_EPIS = (E_NONE, E_RES, E_GELU, E_DGELU)


def test_gemm_nt_weight_resident_tile_edges(option):
    """gemm_nt_wres_kernel: K = 192, N % 192 == 0, M % 32 == 0, M >= 4096 (gemm_nt_wres.hip:283-295); one workgroup per CU
    with msplit = (256 / column tiles) rounded down to 8 -- N = 6336 (33 tiles) leaves msplit < 8 and must fall back, as
    must M = 4064 (< 4096) and M = 4100 (M % 32)."""
    nt_generic_opts(option, 1)
    option("nt_wres", 1)
    worst = KC.Worst()
    cases = [(m, 576) for m in (4096, 4128)] + [(4096, n) for n in (192, 768, 6144)] + [(32 * 201, 192)]
    for i, (M, N) in enumerate(cases):
        for epi in WRES_EPIS:
            nt_case(BF16, epi, M, N, 192, inter=True, seed=40 * i + epi, want=("gemm_nt_wres_kernel",),
                    forbid=("gemm_nt_kernel",), worst=worst, key=EPI_NAMES[epi])
    for epi in WRES_EPIS:
        nt_case(BF16, epi, 4128, 576, 192, pad=True, inter=True, seed=990 + epi, want=("gemm_nt_wres_kernel",),
                worst=worst, key=EPI_NAMES[epi] + "-pad")
    for M, N in [(4064, 576), (4100, 576), (4096, 6336)]:
        nt_case(BF16, E_RES, M, N, 192, inter=True, seed=M + N, want=("gemm_nt_kernel",), forbid=("gemm_nt_wres_kernel",))
    # the tanh epilogue is not the weight-resident kernel's: generic kernel
    nt_case(BF16, E_TANH, 4096, 576, 192, inter=True, seed=77, want=("gemm_nt_kernel",), forbid=("gemm_nt_wres_kernel",))
    worst.report("gemm_nt weight-resident bf16")


KP_EPIS = (E_NONE, E_RES, E_GELU, E_DGELU)


@pytest.mark.parametrize("persist", [0, 1])
def test_gemm_nt_row_panel_tile_edges(option, persist):
    """kp7 (gemm_nt_kpipe_body.inc:755-758: N % 192, K % 64, K >= 256, M >= 8192): 224-row panels, ragged last panel
    M = 224 k + {0, 1, 17, 223}; several column tiles take the persistent kernel with kp_persist = 1.  M = 8191 falls
    back to the generic kernel."""
    nt_generic_opts(option, 1)
    option("nt_kpipe", 1)
    option("kp_persist", persist)
    option("kp8", 0)
    worst = KC.Worst()
    k37 = 224 * 37
    cases = [(k37 + r, 384, 256) for r in (0, 1, 17, 223)]
    cases += [(k37 + 17, n, 320) for n in (192, 1152)]
    cases += [(k37 + 1, 192, k) for k in (768, 3072)]
    for i, (M, N, K) in enumerate(cases):
        kern = "gemm_nt_kpipe_persist_kernel" if (persist and N > 192) else "gemm_nt_kpipe_kernel"
        for epi in KP_EPIS:
            nt_case(BF16, epi, M, N, K, inter=True, seed=50 * i + epi, want=(("kp7", kern),), forbid=("gemm_nt_kernel",),
                    worst=worst, key=EPI_NAMES[epi])
    for epi in KP_EPIS:
        nt_case(BF16, epi, k37 + 223, 384, 256, pad=True, inter=True, seed=1100 + epi, want=("kp7",), worst=worst,
                key=EPI_NAMES[epi] + "-pad")
    nt_case(BF16, E_RES, 8191, 384, 256, inter=True, seed=1200, want=("gemm_nt_kernel",), forbid=("gemm_nt_kpipe",))
    worst.report(f"gemm_nt row-panel kp7 persist={persist}")


def test_gemm_nt_row_panel_kp8(option):
    """kp8 (use_kp8, gemm_nt_kpipe.hip:42-50): M a multiple of 256 and not of 224, where 256-row panels fill the rounds."""
    nt_generic_opts(option, 1)
    option("nt_kpipe", 1)
    option("kp8", 1)
    worst = KC.Worst()
    for i, (M, N, K) in enumerate([(16384, 768, 256), (65536, 768, 256)]):
        for epi in KP_EPIS:
            nt_case(BF16, epi, M, N, K, inter=True, seed=60 * i + epi, want=(("kp8", "gemm_nt_kpipe"),),
                    forbid=("gemm_nt_kernel", "kp7"), worst=worst, key=EPI_NAMES[epi])
    nt_case(BF16, E_RES, 16384, 768, 256, pad=True, inter=True, seed=1300, want=("kp8",), worst=worst, key="res-pad")
    worst.report("gemm_nt row-panel kp8")


# ------------------------------------------------------------------------------------------------------------- GEMM TN
def qkv_rows(No, heads):
    n = torch.arange(No, device=DEV)
    inner = heads * 64
    s3, rem = n // inner, n % inner
    return (rem // 64) * 192 + (rem % 64) * 3 + s3


def tn_operands(dt, M, No, Ki, seed, pad):
    ldy, ldx = (No + 8, Ki + 16) if pad else (No, Ki)
    dY = nan_padded(rnd((M, No), seed, 1.0, dt), ldy, 5)
    X = nan_padded(rnd((M, Ki), seed + 1, 1.0, dt), ldx, 5)
    return dY, X, ldy, ldx


def tn_outputs(No, Ki, acc, with_db, seed):
    dW = guarded(No, Ki, F32)
    db = guarded(No, None, F32) if with_db else None
    if acc:
        dW.fill_(rnd((No, Ki), seed + 7))
        if db:
            db.fill_(rnd((No,), seed + 8))
    return dW, db


def tn_check(dY, X, dW, db, heads, acc, init, where, worst, key):
    M = dY.shape[0]
    dW.check(where + " dW")
    y64, x64 = dY.double(), X.double()
    ref = y64.T @ x64
    mag = y64.abs().T @ x64.abs()
    rb = y64.sum(0)
    mb = y64.abs().sum(0)
    if heads:
        dst = qkv_rows(ref.shape[0], heads)
        for t in (ref, mag, rb, mb):
            t[dst] = t.clone()
    if acc:
        ref += init[0]
        mag += init[0].abs()
        if db:
            rb += init[1]
            mb += init[1].abs()
    worst(key, check_bound(dW.t, ref, mag, F32, 1, (M + 2) * U, where + " dW", tile=(128, 192)))
    if db:
        db.check(where + " db")
        worst(key + "-db", check_bound(db.t, rb, mb, F32, 1, (M + 2) * U, where + " db", tile=(128,)))


def tn_case(dt, M, No, Ki, heads=0, acc=0, with_db=True, pad=False, seed=1, want=("gemm_tn_kernel",), forbid=(),
            worst=None, key=""):
    dY, X, ldy, ldx = tn_operands(dt, M, No, Ki, seed, pad)
    dW, db = tn_outputs(No, Ki, acc, with_db, seed)
    init = (dW.t.double().clone(), db.t.double().clone() if db else None) if acc else None
    wsb = L.lib().rgbnm_gemm_tn_workspace(M, No, Ki)
    ws = guarded(wsb // 4, None, F32)

    def call():
        L.check(L.lib().rgbnm_gemm_tn(L.dt_of(dt), dY.data_ptr(), ldy, X.data_ptr(), ldx, dW.t.data_ptr(),
                                      db.t.data_ptr() if db else None, M, No, Ki, heads, acc, ws.t.data_ptr(), wsb, L.stream()))
    _, names = launched(call)
    where = f"gemm_tn {NAMES[dt]} M={M} No={No} Ki={Ki} heads={heads} acc={acc} db={int(with_db)} pad={int(pad)}"
    expect(names, want, where, forbid)
    ws.check(where + " workspace", written=False)
    tn_check(dY, X, dW, db, heads, acc, init, where, worst, key)


def tn_tiles(No, Ki):
    return -(-No // 128) * (Ki // 192 if Ki % 192 == 0 else -(-Ki // 128))


@pytest.mark.parametrize("dt,tr", [(BF16, 0), (BF16, 1), (F16, 0), (F16, 1), (F32, 0)])
def test_gemm_tn_generic_splits_and_edges(option, dt, tr):
    """gemm_tn_kernel: 128 x 192 (Ki % 192 == 0) or 128 x 128 output tiles, k-tiles of TK = 64 tokens (16-bit) / 32 (fp32)
    (gemm.hip:387); tn_wgs sets the token split: S = 1, S = 2 and a last split holding one k-tile.  Ragged token counts
    M in {1, TK - 1, TK, TK + 1}, the qkv row permutation, accumulation into non-zero dW / db, db = NULL, padded strides."""
    option("tn_pipe", 0)
    if dt != F32:
        option("tn_tr", tr)
    worst = KC.Worst()
    TK = 32 if dt == F32 else 64
    cases = []
    for Ki in (192, 136):
        for M in (1, TK - 1, TK, TK + 1):
            cases.append((M, 192, Ki, 0, 1))
        cases.append((2 * TK + 3, 200, Ki, 0, 2))              # S = 2
        cases.append((5 * TK - 7, 192, Ki, 0, 4))              # splits of 2, 2, 1 k-tiles
    cases += [(3 * TK + 5, 576, 192, 3, 2), (4 * TK, 1152, 384, 6, 4), (TK + 1, 8, 8, 0, 1), (1000, 136, 1000, 0, 8)]
    for i, (M, No, Ki, heads, s) in enumerate(cases):
        option("tn_wgs", s * tn_tiles(No, Ki))
        for acc, with_db in ((0, True), (1, True), (0, False)):
            tn_case(dt, M, No, Ki, heads, acc, with_db, pad=(i % 3 == 2), seed=20 * i + acc, worst=worst,
                    key=f"S<={s}")
    worst.report(f"gemm_tn generic {NAMES[dt]} tr={tr}")


@pytest.mark.parametrize("wide", [0, 1])
def test_gemm_tn_pipelined_and_wide(option, wide):
    """gemm_tn_pipe_kernel (bf16, M % 64, Ki % 192) and gemm_tn_wide_kernel (tn_wide: No % 192, Ki % 384): the qkv
    permutation, accumulation, db = NULL, padded strides; M % 64 != 0 falls back to the generic kernel."""
    option("tn_pipe", 1)
    option("tn_wide", wide)
    worst = KC.Worst()
    if wide:
        cases = [(64 * 49, 1152, 384, 6), (64 * 9, 3072, 768, 0), (64 * 49, 1536, 384, 0), (64 * 49, 384, 1536, 0)]
        kern = "gemm_tn_wide_kernel"
    else:
        cases = [(64, 192, 192, 0), (64 * 7, 200, 384, 0), (64 * 49, 576, 192, 3), (64 * 100, 1152, 384, 6)]
        kern = "gemm_tn_pipe_kernel"
    for i, (M, No, Ki, heads) in enumerate(cases):
        for acc, with_db in ((0, True), (1, True), (0, False)):
            tn_case(BF16, M, No, Ki, heads, acc, with_db, pad=(i % 2 == 1), seed=30 * i + acc, want=(kern,),
                    forbid=("gemm_tn_kernel",), worst=worst, key=kern)
    tn_case(BF16, 64 * 7 + 1, 192, 384, seed=999, want=("gemm_tn_kernel",), forbid=(kern,), worst=worst, key="fallback")
    worst.report(f"gemm_tn pipelined wide={wide}")


def test_gemm_tn_group_bracket_flushes(option):
    """rgbnm_gemm_tn_group_begin_n / _end (include/rgbnm.h:117-131): one bracket whose jobs force every flush cause -- a row
    count change, more than 256 tiles, max_jobs reached, and _end -- mixing the qkv permutation, accumulation and db = NULL;
    every queued job brings the workspace rgbnm_gemm_tn_workspace_splits sizes for it.  Checked after _end, element-wise."""
    option("tn_pipe", 1)
    lib = L.lib()
    # (M, No, Ki, heads, acc, db): queue after each  [1] [1,2] | [3] [3,4] | [5] [5,6] [5,6,7] [5..8]=cap | [9] _end
    jobs = [(1024, 576, 192, 3, 0, True), (1024, 192, 768, 0, 1, True),
            (2048, 1536, 1536, 0, 0, True), (2048, 1536, 1536, 0, 1, False),
            (2048, 1536, 1536, 0, 0, True), (2048, 192, 192, 0, 1, True), (2048, 192, 384, 0, 0, False),
            (2048, 384, 192, 0, 0, True),
            (2048, 576, 192, 3, 1, True)]
    state = []
    for i, (M, No, Ki, heads, acc, with_db) in enumerate(jobs):
        dY, X, ldy, ldx = tn_operands(BF16, M, No, Ki, 100 + 10 * i, pad=(i % 2 == 1))
        dW, db = tn_outputs(No, Ki, acc, with_db, 100 + 10 * i)
        init = (dW.t.double().clone(), db.t.double().clone() if db else None) if acc else None
        jt = -(-No // 128) * (Ki // 192)
        wsb = lib.rgbnm_gemm_tn_workspace_splits(No, Ki, max(1, 256 // jt))
        ws = guarded(wsb // 4, None, F32)
        state.append((dY, X, ldy, ldx, dW, db, init, ws, wsb, M, No, Ki, heads, acc))

    def bracket():
        lib.rgbnm_gemm_tn_group_begin_n(4)
        for (dY, X, ldy, ldx, dW, db, init, ws, wsb, M, No, Ki, heads, acc) in state:
            L.check(lib.rgbnm_gemm_tn(L.dt_of(BF16), dY.data_ptr(), ldy, X.data_ptr(), ldx, dW.t.data_ptr(),
                                      db.t.data_ptr() if db else None, M, No, Ki, heads, acc, ws.t.data_ptr(), wsb, L.stream()))
        L.check(lib.rgbnm_gemm_tn_group_end(L.stream()))
    _, names = launched(bracket)
    nlaunch = sum(1 for n in names if "gemm_tn_pipe_kernel" in n or "gemm_tn_wide_kernel" in n)
    assert nlaunch == 4, (nlaunch, sorted(set(names)))
    assert not ran(names, "gemm_tn_kernel"), sorted(set(names))
    worst = KC.Worst()
    for i, (dY, X, ldy, ldx, dW, db, init, ws, wsb, M, No, Ki, heads, acc) in enumerate(state):
        where = f"group job {i}: M={M} No={No} Ki={Ki} heads={heads} acc={acc}"
        ws.check(where + " workspace", written=False)
        tn_check(dY, X, dW, db, heads, acc, init, where, worst, "group")
    worst.report("gemm_tn group bracket")


# ------------------------------------------------------------------------------------------------------------- attention
# c of the bound c u_P mag: twice the worst measured on one MI355X (measured c in brackets, all paths and types; fp32 sets them)
ATTN_C = {"out": 2.5,    # [1.22]
          "lse": 0.13,   # [0.064]  of u (64 scale max_j |q||k| + |lse| + 1), absolute
          "dq": 1.0,     # [0.48]
          "dk": 2.0,     # [0.96]
          "dv": 4.6}     # [2.27]


def attn_case(dt, B, N, H, seed, want_f, want_b, worst, key, *, qkv=None, dout=None, scale=None, check=None):
    """qkv, dout, scale: the caller's inputs in place of the unit-scale draws.  check(where, qkv, dout, out, lse, dqkv, scale): the
    caller's bounds (its added terms included) in place of the ones below (tests/test_value_regimes.py); the launches, the guards
    and the asserted kernels are the same.  The defaults give the tensors and bounds this case always had."""
    I = H * 64
    scale = 1.0 / math.sqrt(I) if scale is None else scale
    qkv = rnd((B * N, 3 * I), seed, 1.5, dt) if qkv is None else qkv
    dout = rnd((B * N, I), seed + 1, 1.0, dt) if dout is None else dout
    out = guarded(B * N, I, dt)
    lse = guarded(B * H * N, None, F32)
    dqkv = guarded(B * N, 3 * I, dt)

    def fwd():
        L.check(L.lib().rgbnm_attention_fwd(L.dt_of(dt), qkv.data_ptr(), out.t.data_ptr(), lse.t.data_ptr(), B, N, H, scale,
                                            L.stream()))

    def bwd():
        L.check(L.lib().rgbnm_attention_bwd(L.dt_of(dt), qkv.data_ptr(), out.t.data_ptr(), dout.data_ptr(), lse.t.data_ptr(),
                                            dqkv.t.data_ptr(), B, N, H, scale, L.stream()))
    where = f"attention {NAMES[dt]} B={B} N={N} H={H}"
    _, nf = launched(fwd)
    expect(nf, want_f, where + " fwd")
    _, nb = launched(bwd)
    expect(nb, want_b, where + " bwd")
    out.check(where + " out")
    lse.check(where + " lse")
    dqkv.check(where + " dqkv")
    if check is not None:
        return check(where, qkv, dout, out.t, lse.t, dqkv.t, scale)
    uP = KC.U_OF[dt] if dt != F32 else N * U

    def heads(t):                                    # [B*N, 3I] -> three [B, H, N, 64]
        return [t[:, i * I:(i + 1) * I].reshape(B, N, H, 64).permute(0, 2, 1, 3) for i in range(t.shape[1] // I)]

    def flat(t):
        return t.permute(0, 2, 1, 3).reshape(B * N, I)
    q, k, v = heads(qkv.double())
    S = (q @ k.transpose(-1, -2)) * scale
    lse_ref = torch.logsumexp(S, -1)
    P = torch.exp(S - lse_ref[..., None])
    O = P @ v
    mO = P @ v.abs()
    worst(key + "-out", check_bound(out.t, flat(O), flat(mO), dt, 1, ATTN_C["out"] * uP, where + " out", tile=(N, 64)))
    lmag = (scale * (q.abs() @ k.abs().transpose(-1, -2))).amax(-1) * 64 + lse_ref.abs() + 1
    worst(key + "-lse", check_bound(lse.t.view(B, H, N), lse_ref, lmag, F32, 0, ATTN_C["lse"] * U, where + " lse"))
    dO = heads(dout.double())[0]
    D = (dO * O).sum(-1, keepdim=True)
    dS = P * (dO @ v.transpose(-1, -2) - D)
    mD = (dO.abs() * mO).sum(-1, keepdim=True)
    mdS = P * (dO.abs() @ v.abs().transpose(-1, -2) + mD)
    del S
    refs = {"dq": (scale * dS @ k, scale * mdS @ k.abs(), 0), "dk": (scale * dS.transpose(-1, -2) @ q,
            scale * mdS.transpose(-1, -2) @ q.abs(), 1), "dv": (P.transpose(-1, -2) @ dO, P.transpose(-1, -2) @ dO.abs(), 2)}
    for nm, (r, m, s) in refs.items():
        got = dqkv.t[:, s * I:(s + 1) * I]
        worst(key + "-" + nm, check_bound(got, flat(r), flat(m), dt, 1, ATTN_C[nm] * uP, where + " " + nm, tile=(N, 64)))


ATTN_N = (1, 31, 32, 33, 63, 64, 65, 196, 223, 224, 225, 288, 319, 320)


@pytest.mark.parametrize("dt", DTS3)
def test_attention_v1_edges(option, dt):
    """First-generation attention kernels (attn_fwd_kernel / attn_bwd_dq_kernel / attn_bwd_dkv_kernel): 7 tiles of 32
    tokens up to N = 224, 10 tiles above.  N walks the 32-token tiles and the 224 / 320 limits, H in {1, 3, 6, 12}."""
    option("attn_v2", 0)
    worst = KC.Worst()
    cases = [(2, n, 3) for n in ATTN_N] + [(3, 65, h) for h in (1, 6, 12)] + [(1, 320, 12)]
    for i, (B, N, H) in enumerate(cases):
        tiles = "10" if N > 224 else "7"
        wf = (("attn_fwd_kernel", tiles),)
        wb = (("attn_bwd_dq_kernel", tiles), ("attn_bwd_dkv_kernel", tiles))
        attn_case(dt, B, N, H, 40 + i, wf, wb, worst, "v1")
    worst.report(f"attention v1 {NAMES[dt]}")


@pytest.mark.parametrize("persist", [0, 1])
def test_attention_v2_edges(option, persist):
    """attn_v2 (bf16, N <= 224): one workgroup per (image, head), or with attn_persist the persistent kernels -- the
    backward always, the forward from 256 (image, head) pairs: B H in {255, 256, 257} walks that edge."""
    option("attn_v2", 1)
    option("attn_persist", persist)
    worst = KC.Worst()
    cases = [(2, n, 3) for n in ATTN_N if n <= 224] + [(3, 65, h) for h in (1, 6, 12)]
    if persist:
        cases += [(85, 196, 3), (256, 65, 1), (257, 33, 1), (257, 224, 1), (43, 196, 6)]
    for i, (B, N, H) in enumerate(cases):
        if persist:
            wf = ("attn3_fwd_kernel",) if B * H >= 256 else ("attn2_fwd_kernel",)
            wb = ("attn3_bwd_kernel",)
        else:
            wf, wb = ("attn2_fwd_kernel",), ("attn2_bwd_kernel",)
        attn_case(BF16, B, N, H, 80 + i, wf, wb, worst, f"bh>=256" if B * H >= 256 else "v2")
    worst.report(f"attention v2 persist={persist}")


# ------------------------------------------------------------------------------------------------------------- LayerNorm
# c of the bound c E u mag: twice the worst measured on one MI355X (measured c in brackets; the fp32 runs set them, the 16-bit
# ones sit at half an ulp of T)
LN_C = {"y": 1.2,        # [0.59]
        "stat": 1.4,     # [0.67]
        "dx": 1.3}       # [0.62]


def ln_ref_fwd(x64, g64, b64, eps):
    E = x64.shape[1]
    mu = x64.mean(1, keepdim=True)
    var = ((x64 - mu) ** 2).mean(1, keepdim=True)
    rs = 1.0 / torch.sqrt(var + eps)
    xh = (x64 - mu) * rs
    return mu, rs, xh


def ln_case(dt, M, E, dres_on, acc, seed, worst, key, generic=False, res_on=False, ss_on=False, rps=7, want=None, *, x=None,
            dy=None, check=None):
    """x, dy: the caller's rows in place of the unit-scale draws.  check: an object whose fwd(...) and bwd(...) take the place of the
    bounds below, which are the same forms stated per row regime (tests/regime_ref.py ln_check_fwd / ln_check_bwd); the launches, the
    guards and the asserted kernels are the same.  The defaults give the tensors and bounds this case always had."""
    eps = 1e-5
    x = (rnd((M, E), seed, 2.0) + 0.5).to(dt) if x is None else x
    gamma = 1 + rnd((E,), seed + 1, 0.2)
    beta = rnd((E,), seed + 2, 0.2)
    res = rnd((M, E), seed + 3, 1.0, dt) if res_on else None
    ss = (torch.rand(-(-M // rps), device=DEV) + 0.5) if ss_on else None
    y = guarded(M, E, dt)
    mean, rstd = guarded(M, None, F32), guarded(M, None, F32)
    lib = L.lib()

    def fwd():
        if generic:
            L.check(lib.rgbnm_ln_generic_fwd(L.dt_of(dt), x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), L.ptr(res), L.ptr(ss),
                                             rps, y.t.data_ptr(), mean.t.data_ptr(), rstd.t.data_ptr(), M, E, eps, L.stream()))
        else:
            L.check(lib.rgbnm_layernorm_fwd(L.dt_of(dt), x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), y.t.data_ptr(),
                                            mean.t.data_ptr(), rstd.t.data_ptr(), M, E, eps, L.stream()))
    where = f"layernorm{' generic' if generic else ''} {NAMES[dt]} M={M} E={E} dres={int(dres_on)} acc={acc}"
    _, nf = launched(fwd)
    expect(nf, (want[0],), where + " fwd")
    for t, nm in ((y, "y"), (mean, "mean"), (rstd, "rstd")):
        t.check(where + " " + nm)
    x64, g64, b64 = x.double(), gamma.double(), beta.double()
    sc = ss.double()[torch.arange(M, device=DEV) // rps][:, None] if ss_on else 1.0
    if check is not None:
        check.fwd(where, x, gamma, beta, y.t, mean.t, rstd.t, eps, res, sc)
    mu, rs, xh = ln_ref_fwd(x64, g64, b64, eps)
    yref = (xh * g64 + b64) * sc
    ymag = (g64.abs() * (xh.abs() + rs * x64.abs().mean(1, keepdim=True)) + b64.abs()) * sc
    if res_on:
        yref = yref + res.double()
        ymag = ymag + res.double().abs()
    cE = LN_C["y"] * E * U
    if check is None:
        worst(key + "-y", check_bound(y.t, yref, ymag, dt, 1, cE, where + " y", tile=(16, E)))
        worst(key + "-stat", check_bound(mean.t, mu[:, 0], x64.abs().mean(1), F32, 1, LN_C["stat"] * E * U, where + " mean"))
        worst(key + "-stat", check_bound(rstd.t, rs[:, 0], rs[:, 0], F32, 1, LN_C["stat"] * E * U, where + " rstd"))
    del yref, ymag
    # backward on the kernel's own statistics (inputs of the operation: exact in the reference)
    dy = rnd((M, E), seed + 4, 1.0, dt) if dy is None else dy
    dres = rnd((M, E), seed + 5, 1.0, dt) if dres_on else None
    dx = guarded(M, E, dt)
    dg, dbt = guarded(E, None, F32), guarded(E, None, F32)
    if acc:
        dg.fill_(rnd((E,), seed + 6))
        dbt.fill_(rnd((E,), seed + 7))
    init = (dg.t.double().clone(), dbt.t.double().clone())
    wsb = lib.rgbnm_ln_generic_bwd_workspace(M, E) if generic else lib.rgbnm_layernorm_bwd_workspace(M, E)
    ws = guarded(wsb // 4, None, F32)

    def bwd():
        if generic:
            L.check(lib.rgbnm_ln_generic_bwd(L.dt_of(dt), dy.data_ptr(), x.data_ptr(), gamma.data_ptr(), mean.t.data_ptr(),
                                             rstd.t.data_ptr(), L.ptr(ss), rps, dx.t.data_ptr(), dg.t.data_ptr(), dbt.t.data_ptr(),
                                             M, E, acc, ws.t.data_ptr(), wsb, L.stream()))
        else:
            L.check(lib.rgbnm_layernorm_bwd(L.dt_of(dt), dy.data_ptr(), x.data_ptr(), gamma.data_ptr(), mean.t.data_ptr(),
                                            rstd.t.data_ptr(), L.ptr(dres), dx.t.data_ptr(), dg.t.data_ptr(), dbt.t.data_ptr(),
                                            M, E, acc, ws.t.data_ptr(), wsb, L.stream()))
    _, nb = launched(bwd)
    expect(nb, (want[1],), where + " bwd")
    for t, nm in ((dx, "dx"), (dg, "dgamma"), (dbt, "dbeta"), (ws, "workspace")):
        t.check(where + " " + nm, written=(nm != "workspace"))
    if check is not None:
        return check.bwd(where, x, gamma, dy, mean.t, rstd.t, dx.t, dg.t, dbt.t, dres, init if acc else None, sc)
    kmu, krs = mean.t.double()[:, None], rstd.t.double()[:, None]
    xh = (x64 - kmu) * krs
    d = dy.double() * sc
    gv = d * g64
    c1 = gv.mean(1, keepdim=True)
    c2 = (gv * xh).mean(1, keepdim=True)
    dxref = krs * (gv - c1 - xh * c2)
    dxmag = krs * (gv.abs() + gv.abs().mean(1, keepdim=True) + xh.abs() * (gv * xh).abs().mean(1, keepdim=True))
    if dres_on:
        dxref = dxref + dres.double()
        dxmag = dxmag + dres.double().abs()
    worst(key + "-dx", check_bound(dx.t, dxref, dxmag, dt, 1, LN_C["dx"] * E * U, where + " dx", tile=(16, E)))
    dgref = (d * xh).sum(0) + (init[0] if acc else 0)
    dgmag = (d.abs() * xh.abs()).sum(0) + (init[0].abs() if acc else 0)
    dbref = d.sum(0) + (init[1] if acc else 0)
    dbmag = d.abs().sum(0) + (init[1].abs() if acc else 0)
    worst(key + "-dgamma", check_bound(dg.t, dgref, dgmag, F32, 1, (M + E) * U, where + " dgamma"))
    worst(key + "-dbeta", check_bound(dbt.t, dbref, dbmag, F32, 1, (M + E) * U, where + " dbeta"))


@pytest.mark.parametrize("dt", DTS3)
@pytest.mark.parametrize("E", [192, 384, 512, 768, 1024])
def test_layernorm_widths_and_grid_loops(dt, E):
    """rgbnm_layernorm_fwd / _bwd at every width they dispatch (layernorm.hip:321-325, 337-341).  Rows per workgroup pass:
    forward 16 (E <= 384) / 4, backward 16 / 8 (E = 384) / 4.  The forward grid is capped at 4096 workgroups and the
    backward at LN_BWD_BLOCKS = 2048: the last row counts make every grid-stride loop run more than once."""
    worst = KC.Worst()
    gf = 16 if E <= 384 else 4
    gb = 16 if E == 192 else 8 if E == 384 else 4
    rows = sorted({1, gf - 1, gf + 1, gb - 1, gb + 1, 3 * gb + 2})
    big_f = 4096 * gf + 1
    big_b = 2048 * gb + 1
    cases = [(m, i % 2, (i // 2) % 2) for i, m in enumerate(rows)] + [(big_f, 1, 1), (big_b, 0, 1)]
    for i, (M, dres_on, acc) in enumerate(cases):
        ln_case(dt, M, E, dres_on, acc, 200 + 10 * i, worst, f"E={E}", want=("ln_fwd_kernel", "ln_bwd_kernel"))
    worst.report(f"layernorm {NAMES[dt]} E={E}")


@pytest.mark.parametrize("dt", DTS3)
def test_layernorm_any_width(option, dt):
    """rgbnm_ln_generic_fwd / _bwd (one wave per row, four rows per pass; forward grid capped at 4096, backward at 1024) at
    E in {4, 12, 100, 764, 768}, with the residual and the per-sample scale; E = 768 also on the lanes-per-row kernels."""
    worst = KC.Worst()
    option("ln_rows", 0)
    for i, E in enumerate((4, 12, 100, 764, 768)):
        for j, M in enumerate((1, 5, 4 * 4096 + 1)):
            ln_case(dt, M, E, False, (i + j) % 2, 300 + 10 * i + j, worst, f"E={E}", generic=True, res_on=bool(j % 2 == 0),
                    ss_on=bool((i + j) % 2 == 0), want=("ln_generic_fwd_kernel", "ln_generic_bwd_kernel"))
    option("ln_rows", 1)
    for j, M in enumerate((1, 5, 4 * 4096 + 1)):
        ln_case(dt, M, 768, False, j % 2, 400 + j, worst, "rows-768", generic=True, res_on=True, ss_on=True,
                want=("ln_rows_fwd_kernel", "ln_rows_bwd_kernel"))
    worst.report(f"layernorm any-width {NAMES[dt]}")
