"""fp64 references, inputs, case lists and forward-error bounds of the kernels a train step enters and leaves through
(csrc/embed_tail.hip and the head-pool pair of csrc/layernorm.hip).  A plain module: tests/test_step_ends.py runs the kernels
against it on the GPU, tests/test_step_ends_cpu.py anchors every reference to an independent implementation, runs an fp32
emulation of each kernel's operation order through the same bounds and checks that the case lists reach the launch regimes
they name.  Plain torch on whatever device the inputs live on: no rgb_no_more_amd kernel, nothing of the reference project.

Every reference takes inputs already rounded to their storage type and returns fp64.  Inputs are drawn on the CPU from seeded
generators (the same numbers on every machine) and moved to the device by the caller.

Where the bounds come from (u = 2^-24, the unit roundoff of the fp32 accumulators; K = ceil(C / 256)):

sub-block embedding (subblock_embed_kernel): Z = A.X.A^T as two 16-term fp32 matrix products on the matrix pipe.
  |got - ref| <= ulp_T(ref) + 32 u mag + (ulp32(T)/2) |A|^T, mag = |A| |X| |A|^T: 16 products and 16 sums per product, twice;
  the last term is the rounding of the intermediate T = A.X to fp32 (`t` of the kernel) carried through the second product.
  [measured on one MI355X: 0.30 with fp32 output; 0.50 with 16-bit output, half an ulp of it; 0.66 for fp16 -> fp16]
  The chroma half is a copy: one rounding to T of a value that is in TI, bit for bit.  With mixing the kernel's X is
  round_TI(fmaf(x[b-1], lam1, x[b] * lam0)); mix_fp32() evaluates exactly that (the product of two fp32 numbers is exact in fp64),
  and returns two candidates that differ only where the fp64 sum sits on an fp32 rounding tie.

mixup (mixup_kernel): one fp32 product, one fma, one rounding to TO:  ulp_TO(ref) + 2 u (|lam0 x| + |lam1 x'|).  [0.49; 16-bit 0.50]

soft cross entropy (softxent_kernel, softxent_loss_kernel, softxent_grad_kernel): 256 strided partial sums of K terms, 6 wave
  steps, a four-way combine: (K + 8) u on each sum.  __expf / __logf are the hardware base-2 instructions and one fp32 multiply
  (v_mul by log2 e, v_exp_f32; v_log_f32, v_mul by ln 2: seen in the disassembly of embed_tail.hip for gfx950).  ASSUMPTION, not
  measured here: v_exp_f32 / v_log_f32 are good to 1 ulp of their result (AMD's ISA manual, from memory).  Then
  exp(x): relative 2^-23 + |x| 2^-24 (the instruction, and the rounding of x log2 e), log(s): relative 2^-23 + 2^-24.
    lse   : ulp32(ref) + u (K + 10) + EXPLOG u (3 L + 2 S + 2)       L = lse - max, S = sum_c p_c |z_c - max|      [0.47]
    T     : ulp32(ref) + (K + 8) u sum|t|                                                                          [0.22]
    rows  : ulp32(ref) + (K + 16) u (|lse| T + sum|t z| + T) + EXPLOG u T (3 L + 2 S + 2)                            [0.20]
    loss  : ulp32(ref) + (ceil(B / 256) + 9) u mean|rows| + mean(bound of rows)                                      [0.06]
    dlogits: ulp_T(ref) + 2 u |g| (p T (|z - lse| + |max| + L + 2 (K + 8) + 6) + |t|) + 2 * 2^-126 |g| T    [0.56; 16-bit 0.50]
  The last term: v_exp_f32 returns zero for a result below the smallest normal, 2^-126 (no denormal scaling around it in the
  disassembly).  A result just under that threshold is lost whole, so 2^-126 |g| T is attained (measured: 1.00 of it, in the fp32
  and bf16 dlogits of the N(0, 30^2) logits); the term carries the allowance of two for the exp / log terms so that the printed
  ratio says something about the rest.  EXPLOG = 1 otherwise: no margin was needed.

clip + AdamW + weight decay (sqnorm_kernel, adamw_kernel): first-order propagation of
  dcoef = (n / 65536 + 24) u coef  (n / 65536 four-term squares per thread, 6 + 2 + 6 + 2 combine steps, sqrt, add, divide) when
  max_norm > 0 and the norm is not clearly below it, through m (3 roundings), v (4), the denominator (sqrt, two divides, an
  add), the quotient and the update, each with its fp64 magnitude; a decayed chunk adds the product and the difference.
  The norm gets sqrt(n 2^-126) more: squares below the smallest normal lose bits (g = 1e-20).  ADAM_F = 1 (the allowance is 2).
  [p 0.47, m 0.39, v 0.36, norm 0.03]

head pool (pool_fwd_kernel, pool_bwd_kernel): the terms of the LayerNorm edge tests (test_kernel_edges.LN_C, c E u mag with the
  same magnitudes), plus (ceil(N / G) + G + 2) u for the token sum; dgamma sums N tokens and B images, dbeta B images.
  [pooled 0.006 in fp32 / 0.50 16-bit, mean and rstd 0.011, dx 0.012 / 0.50, dgamma 0.011, dbeta 0.27]
"""
import functools
import math

import torch

from kernel_check import U, ulp, check_bound

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
NAMES = {F32: "f32", BF16: "bf16", F16: "f16"}
INF = float("inf")
EXPLOG = 1.0      # factor on the __expf / __logf terms (allowed: up to 2)
ADAM_F = 1.0      # factor on the AdamW propagation (allowed: up to 2)
LN_C = {"y": 1.2, "stat": 1.4, "dx": 1.3}     # test_kernel_edges.LN_C, reused unchanged


def cdiv(a, b):
    return -(-a // b)


def f32(x):
    """The fp32 rounding of a Python float, as a Python float: a scalar as the kernel receives it."""
    return float(torch.tensor(float(x), dtype=F32))


def randn(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=F32) * scale


@functools.lru_cache(maxsize=8)
def randn_shared(shape, seed):
    """The unit draw behind the AdamW state and gradients: the three runs of one size share it (callers scale, never write)."""
    return randn(shape, seed)


def randint(lo, hi, shape, seed):
    return torch.randint(lo, hi, shape, generator=torch.Generator().manual_seed(seed), dtype=torch.int64)


def ulp32(x):
    return ulp(x, F32)


# ------------------------------------------------------------------------------------------------------------------ mixup
def lam_pair(seed):
    """A non-dyadic (lam0, lam1 = 1 - lam0) pair in fp32, lam0 >= lam1 (cls_transforms sorts them descending)."""
    l0 = 0.5 + 0.45 * float(torch.rand(1, generator=torch.Generator().manual_seed(seed)))
    lam = torch.tensor([l0, 1.0 - l0], dtype=F32)
    return lam


def mix_fp32(x, lam):
    """fmaf(x[b-1], lam1, x[b] * lam0) as the kernels evaluate it, for x [B, ...] of any float type: (lo, hi) fp32 candidates.
    lo == hi except where the fp64 sum is within one fp64 ulp of an fp32 rounding tie (either is accepted there)."""
    lam = lam.to(x.device)
    a = x.float()
    t = a * lam[0]                                            # fp32 product
    s = a.roll(1, 0).double() * lam[1].double() + t.double()  # exact product, one fp64 rounding of the sum
    lo = torch.nextafter(s, torch.full_like(s, -INF)).float()
    hi = torch.nextafter(s, torch.full_like(s, INF)).float()
    return lo, hi


def mixup_ref(x, lam, TI=None):
    """(ref, mag, ref rounded to TI): round_TI(lam0 x[b] + lam1 x[b-1 mod B]) with ref the unrounded fp64 value."""
    lam = lam.double().to(x.device)
    a = x.double()
    r = a.roll(1, 0)
    ref = lam[0] * a + lam[1] * r
    mag = lam[0] * a.abs() + lam[1] * r.abs()
    return ref, mag, (ref.to(TI) if TI is not None else None)


def mixup_target_ref(lab, lam, C):
    """target[b][c] = (lab[b] == c ? lam0 : 0) + (lab[b-1] == c ? lam1 : 0), evaluated in fp32; [B, C] fp32."""
    lam = lam.to(lab.device)
    c = torch.arange(C, device=lab.device)[None, :]
    z = torch.zeros((), dtype=F32, device=lab.device)
    return torch.where(lab[:, None] == c, lam[0], z) + torch.where(lab.roll(1, 0)[:, None] == c, lam[1], z)


# -------------------------------------------------------------------------------------------------------------- embedding
def gather_x(y):
    """y [B, 1, Hb, Wb, 8, 8] -> X [B, Hb/2, Wb/2, 16, 16], X[8 pdh + p1][8 pdw + p2] = y[b, 0, 2 ph + pdh, 2 pw + pdw, p1, p2]."""
    B, _, Hb, Wb = y.shape[:4]
    return y[:, 0].reshape(B, Hb // 2, 2, Wb // 2, 2, 8, 8).permute(0, 1, 3, 2, 5, 4, 6).reshape(B, Hb // 2, Wb // 2, 16, 16)


def embed_ref(y, cbcr, A, transpose_a=False):
    """(luma [npatch, 256], mag, extraT, chroma [npatch, 128]) in fp64 from y, cbcr holding storage-type values.
    Z = A.X.A^T (A^T.X.A with transpose_a), rows 'b h w', the feature row is [Z row-major | Cb | Cr]."""
    A = A.double().to(y.device)
    A = A.T if transpose_a else A
    X = gather_x(y.double())
    T = A @ X
    Z = T @ A.T
    mag = (A.abs() @ X.abs()) @ A.abs().T
    extra = (0.5 * ulp32(T)) @ A.abs().T
    n = X.shape[0] * X.shape[1] * X.shape[2]
    chroma = cbcr.double().permute(0, 2, 3, 1, 4, 5).reshape(n, 128)
    return Z.reshape(n, 256), mag.reshape(n, 256), extra.reshape(n, 256), chroma


def embed_inputs(B, Hb, Wb, TI, kind, seed):
    """y [B,1,Hb,Wb,8,8], cbcr [B,2,Hb/2,Wb/2,8,8] in TI.  kind 'dct': DC terms are integers in [-1024, 1016], AC terms decay
    with frequency to near zero, as de-quantised JPEG coefficients do; 'normal': unit normals."""
    y, c = _embed_raw(B, Hb, Wb, kind, seed)
    return y.to(TI), c.to(TI)


@functools.lru_cache(maxsize=48)
def _embed_raw(B, Hb, Wb, kind, seed):
    """The fp32 draw behind embed_inputs (shared by the type pairs of a case; callers do not write to it)."""
    y = randn((B, 1, Hb, Wb, 8, 8), seed)
    c = randn((B, 2, Hb // 2, Wb // 2, 8, 8), seed + 1)
    if kind == "dct":
        f = torch.arange(8, dtype=F32)
        decay = 40.0 / (1.0 + f[:, None] + f[None, :]) ** 3
        y, c = y * decay, c * decay
        y[..., 0, 0] = randint(-1024, 1017, y.shape[:-2], seed + 2).float()
        c[..., 0, 0] = randint(-1024, 1017, c.shape[:-2], seed + 3).float()
    return y, c


EMBED_PAIRS = [(F32, F32), (F32, BF16), (BF16, BF16), (BF16, F32), (F32, F16), (BF16, F16), (F16, F16)]
# (B, Hb, Wb, transpose_a)
EMBED_CASES = [(1, 2, 2, 0),       # one patch: three of the four waves have empty runs
               (3, 2, 2, 0),       # three patches
               (1, 4, 6, 1),       # six patches on eight waves
               (5, 2, 6, 0),       # 15 patches on 16 waves, Hb != Wb
               (2, 4, 6, 1),       # the golden's shape
               (1, 28, 28, 0),     # B = 1: the roll maps an image to itself
               (3, 28, 28, 0),     # one-patch runs that start mid-position: partner b - 1 and, at b = 0, B - 1
               (7, 28, 28, 1),
               (2, 64, 64, 1),     # the SwinV2 grid
               (43, 28, 28, 0),    # 8428 patches: the 2048 cap binds, per = 2 does not divide 43
               (131, 28, 28, 0)]   # 25676 patches: per = 4 does not divide 131
EMBED_BIG_PAIRS = [(F32, F32), (BF16, BF16), (F16, F16)]       # (131, 28, 28) runs on these pairs only


def embed_launch(B, Hb, Wb):
    """The launcher's grid and the kernel's runs: (grid, per, [(q0, q1) per wave]) over q = pos * B + b."""
    npatch = B * (Hb // 2) * (Wb // 2)
    grid = min(cdiv(npatch, 4), 2048)
    nw = grid * 4
    per = cdiv(npatch, nw)
    return grid, per, [(w * per, min(w * per + per, npatch)) for w in range(nw)]


def embed_bound_extra(A, transpose_a, lo, hi, TI):
    """|A| |dX| |A|^T for the elements where the fp32 mix has two candidates (a rounding tie): zero almost everywhere."""
    A = A.double().to(lo.device)
    A = (A.T if transpose_a else A).abs()
    d = gather_x((hi.to(TI).double() - lo.to(TI).double()).abs())
    return ((A @ d) @ A.T).reshape(-1, 256)


# ---------------------------------------------------------------------------------------------------------- cross entropy
SX_C = (1, 2, 63, 255, 256, 257, 1000, 1024, 21841)
SX_B = (1, 2, 255, 256, 257, 1024)
SX_SHAPES = [(1, 1), (2, 2), (255, 63), (256, 255), (257, 256), (1024, 257), (2, 1000), (257, 1000), (1024, 1000), (1, 1024),
             (256, 1024), (2, 21841), (19, 21841), (1, 21841)]
SX_LOGITS = ("n3", "n0.01", "n30", "n5+50", "n5-40", "dominant")
SX_GOUT = (None, 1.0, 0.37, 65536.0)
SX_DTS = (F32, BF16, F16)


@functools.lru_cache(maxsize=128)
def sx_logits(B, C, kind, seed):
    """fp32 logits [B, C] of one of SX_LOGITS (the three families share the draws of a shape, about 60 MB in all; callers do not write to them)."""
    z = randn((B, C), seed)
    if kind == "n3":
        z *= 3.0
    elif kind == "n0.01":
        z *= 0.01
    elif kind == "n30":
        z *= 30.0
    elif kind == "n5+50":
        z = z * 5.0 + 50.0
    elif kind == "n5-40":
        z = z * 5.0 - 40.0
    else:                                       # every third row: one logit 80 above the rest
        rows = torch.arange(0, B, 3)
        z[rows, (7 * rows + 3) % C] += 80.0
    return z


def sx_soft_target(B, C, seed):
    """Row b % 3 == 0: a distribution (mass 1 up to fp32 rounding); == 1: a label-smoothed one-hot; == 2: mass 0.9."""
    t = torch.softmax(randn((B, C), seed), 1)
    lab = randint(0, C, (B,), seed + 1)
    sm = torch.full((B, C), 0.1 / C, dtype=F32)
    sm[torch.arange(B), lab] += 0.9
    k = torch.arange(B)[:, None] % 3
    return torch.where(k == 0, t, torch.where(k == 1, sm, 0.9 * t))


def sx_labels(B, C, seed, equal_neighbours=False):
    lab = randint(0, C, (B,), seed)
    lab[0] = 0 if (seed % 2 == 0 or B > 1) else C - 1
    lab[B - 1] = C - 1 if B > 1 else lab[0]
    if equal_neighbours and B > 2:
        lab[1] = lab[0]                        # row 1 mixes a label with itself: t = lam0 + lam1 at one class
    return lab


def sx_plan():
    """The committed run list: (B, C, logits kind, family, target kind, dl dtype, gout, seed).  Families: 'one' = rgbnm_softxent,
    'two' = _loss + _grad, 'mix' = _loss_mix + _grad_mix.  Every shape meets every logit set and every family; target kind,
    dl dtype and gout rotate so that each family meets each of them (asserted by the CPU regime test)."""
    plan = []
    for si, (B, C) in enumerate(SX_SHAPES):
        for li, kind in enumerate(SX_LOGITS):
            i = 6 * si + li
            for fi, fam in enumerate(("one", "two", "mix")):
                tk = "mix" if fam == "mix" else ("soft", "hard")[(si + li + fi) % 2]
                dt = SX_DTS[(si + li + 2 * fi) % 3]
                gout = SX_GOUT[(si + 3 * li + fi) % 4] if fam != "one" else None
                if dt == F16 and gout == 65536.0 and B == 1:
                    gout = 0.37                  # |dlogits| reaches gout / B: 65536 is beyond fp16's largest number
                plan.append((B, C, kind, fam, tk, dt, gout, 1000 + 7 * i))
    return plan


def sx_case_inputs(B, C, kind, tk, seed):
    """(logits fp32, dense fp32 target, soft target or None, labels or None, lam or None), on the CPU."""
    z = sx_logits(B, C, kind, seed)
    soft = lab = lam = None
    if tk == "soft":
        soft = sx_soft_target(B, C, seed + 1)
        t = soft
    elif tk == "hard":
        lab = sx_labels(B, C, seed + 1)
        t = torch.nn.functional.one_hot(lab, C).float()
    else:
        lab = sx_labels(B, C, seed + 1, equal_neighbours=True)
        lam = lam_pair(seed + 2)
        t = mixup_target_ref(lab, lam, C)
    return z, t, soft, lab, lam


def softxent_ref(z, t, g):
    """z [B, C] fp32 logits, t [B, C] the dense target (fp32 values), g the fp32 scale of dlogits.  A dict of fp64 tensors:
    lse, T (target mass), rows = lse T - sum t z, loss = mean(rows), dl = (exp(z - lse) T - t) g, and the bounds' terms."""
    z, t = z.double(), t.double()
    m = z.amax(1)
    lse = torch.logsumexp(z, 1)
    T = t.sum(1)
    tz = (t * z).sum(1)
    rows = lse * T - tz
    p = torch.exp(z - lse[:, None])
    return dict(z=z, t=t, m=m, lse=lse, T=T, rows=rows, loss=rows.mean(), p=p, dl=(p * T[:, None] - t) * g, g=abs(g),
                L=lse - m, S=(p * (z - m[:, None]).abs()).sum(1), aT=t.abs().sum(1), atz=(t * z).abs().sum(1))


def sx_bounds(r, C, dl_dtype):
    """fp64 bounds (lse, T, rows, loss, dl) of the kernel's outputs around softxent_ref's, as derived in the header."""
    K = cdiv(C, 256)
    B = r["rows"].numel()
    el = EXPLOG * U * (3 * r["L"] + 2 * r["S"] + 2)
    b_lse = ulp32(r["lse"]) + U * (K + 10) + el
    b_T = ulp32(r["T"]) + (K + 8) * U * r["aT"]
    b_rows = ulp32(r["rows"]) + (K + 16) * U * (r["lse"].abs() * r["aT"] + r["atz"] + r["aT"]) + el * r["aT"]
    b_loss = ulp32(r["loss"]) + (cdiv(B, 256) + 9) * U * r["rows"].abs().mean() + b_rows.mean()
    zl = (r["z"] - r["lse"][:, None]).abs()
    per_row = (r["m"].abs() + r["L"] + 2 * (K + 8) + 6)[:, None]
    b_dl = (ulp(r["dl"], dl_dtype) + 2 * U * r["g"] * (r["p"] * r["aT"][:, None] * (zl + per_row) + r["t"].abs())
            + 2 * 2.0 ** -126 * r["g"] * r["aT"][:, None])
    return b_lse, b_T, b_rows, b_loss, b_dl


# ------------------------------------------------------------------------------------------------------------------ AdamW
NORM_BLOCKS = 256
NORM_STRIDE = NORM_BLOCKS * 256 * 4
# n / 256; 2049 and 3073 are added to the issue's list so that the u = 2 and u = 3 strides are each the last one present
ADAM_CHUNKS = (1, 4, 255, 256, 257, 1024, 1025, 2049, 3073, 4096, 4097, 4096 * 3 + 5)
# (gradient scale, max_norm): clipping active (norm >> 1), inactive (norm < max_norm), off; tiny and huge gradients
ADAM_MODES = (("active", 1.0, 1.0), ("inactive", None, 1.0), ("off", 1.0, 0.0), ("tiny", 1e-20, 1.0), ("huge", 1e3, 1.0))
ADAM_STEPS = (1, 2, 1000, 100000)


def adam_plan():
    """(chunks, mode name, gradient scale, max_norm, first step, norm_out present, seed): three modes per size, rotating; the
    runs of one size scale the same unit draws."""
    plan = []
    for i, ch in enumerate(ADAM_CHUNKS):
        for j in range(3):
            name, gs, mn = ADAM_MODES[(i + 2 * j) % 5]
            n = ch * 256
            if gs is None:
                gs = 0.3 / math.sqrt(n)                  # norm about 0.3 < max_norm: coef = 1
            plan.append((ch, name, gs, mn, ADAM_STEPS[(i + j) % 4], (i + j) % 3 != 0, 5000 + 31 * i))
    return plan


def sqnorm_regime(n):
    """(index u of the last stride present in the last turn, number of turns) of sqnorm_kernel's four-stride loop."""
    strides = cdiv(n, NORM_STRIDE)
    return (strides - 1) % 4, cdiv(strides, 4)


def adamw_regime(n):
    """(grid, turns of the chunk loop) of adamw_kernel."""
    grid = min(4096, n // 256)
    return grid, cdiv(n // 256, grid)


def adam_state(n, seed, zero_moments=False):
    """p, m, v fp32 and the per-chunk decay flags (uint8), in a pattern that changes from chunk to chunk.  zero_moments: the
    state of a first step (with gradients of 1e-20, v stays far below eps^2)."""
    p = randn_shared((n,), seed) * 0.05
    m = randn_shared((n,), seed + 1) * (0.0 if zero_moments else 0.01)
    v = (randn_shared((n,), seed + 2) * (0.0 if zero_moments else 0.01)) ** 2
    flags = (randint(0, 3, (n // 256,), seed + 3) > 0).to(torch.uint8)
    if n >= 1024:
        flags[:4] = torch.tensor([1, 0, 1, 1], dtype=torch.uint8)
    return p, m, v, flags


def adam_grad(n, scale, seed):
    """Gradients with exact zeros (every 7th element) and whole zero chunks (every 5th chunk from the second)."""
    g = randn_shared((n,), seed) * scale
    g[::7] = 0.0
    g.view(-1, 256)[1::5] = 0.0
    return g


ADAM_HYPER = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, wd_factor=0.05)


def adamw_ref(p, g, m, v, flags, step, max_norm, lr, beta1, beta2, eps, wd_factor, exact_scalars=False):
    """One step in fp64 from the fp32 state.  Scalars as the kernel gets them: lr, beta*, eps, wd_factor, max_norm as fp32,
    bc1 / bc2_sqrt the fp32 roundings of the launcher's double expressions, 1.f - beta an fp32 difference.
    exact_scalars: every scalar in double instead (the arithmetic of torch.optim, to anchor this function against it).
    A dict: p, m, v, norm (fp64) and the bounds dp, dm, dv, dnorm."""
    n = p.numel()
    rnd = float if exact_scalars else f32
    lr, beta1, beta2, eps, wd, max_norm = (rnd(x) for x in (lr, beta1, beta2, eps, wd_factor, max_norm))
    omb1, omb2 = rnd(1.0 - beta1), rnd(1.0 - beta2)
    bc1 = rnd(1.0 - beta1 ** step)
    bc2s = rnd(math.sqrt(1.0 - beta2 ** step))
    p, g, m, v = p.double(), g.double(), m.double(), v.double()
    norm = torch.sqrt((g * g).sum())
    cn = (n / 65536 + 24) * U
    coef, dc = 1.0, U
    if max_norm > 0:
        c = max_norm / (float(norm) + rnd(1e-6))
        coef = min(c, 1.0)
        if c < 1.0 + 1e-3:
            dc = cn + U
    gc = g * coef
    t1, t2 = beta1 * m.abs(), omb1 * gc.abs()
    m1 = beta1 * m + omb1 * gc
    dm = t2 * dc + 3 * U * (t1 + t2)
    v1 = beta2 * v + omb2 * gc * gc
    dv = omb2 * gc * gc * 2 * dc + 4 * U * v1 + 2.0 ** -147                 # (fp32 denormals: g = 1e-20 squares to 1e-40)
    sq = torch.sqrt(v1)
    den = sq / bc2s + eps
    dsq = torch.minimum(dv / (2 * sq).clamp_min(1e-300), torch.sqrt(dv))   # |sqrt a - sqrt b| <= sqrt|a - b|
    dden = dsq / bc2s + 3 * U * den
    q = m1 / den
    dq = dm / den + q.abs() * dden / den + U * q.abs()
    stp = lr / bc1
    upd = stp * q
    p1 = p - upd
    dp = stp * dq + 2 * U * upd.abs() + U * p1.abs()
    dec = flags.to(p.device).bool().repeat_interleave(256)
    p2 = torch.where(dec, p1 - wd * p1, p1)
    dp = torch.where(dec, dp * (1 + wd) + U * wd * p1.abs() + U * p2.abs(), dp)
    return dict(p=p2, m=m1, v=v1, norm=norm, dp=ADAM_F * dp, dm=ADAM_F * dm, dv=ADAM_F * dv, dnorm=cn * norm + math.sqrt(n * 2.0 ** -126), coef=coef)


# ------------------------------------------------------------------------------------------------------------------- pool
POOL_E = (192, 384, 512, 768, 1024)
POOL_B = (1, 3, 67)
POOL_FWD_UNR, POOL_BWD_UNR = 8, 4


def pool_rows(E):
    """G: rows per workgroup pass of pool_fwd_kernel / pool_bwd_kernel (16 lanes per row up to E = 384, 64 above)."""
    return 16 if E <= 384 else 4


def pool_ns(E):
    G = pool_rows(E)
    return sorted({1, G - 1, G, G + 1, 4 * G - 1, 4 * G, 4 * G + 1, 8 * G, 8 * G + 1, 196, 294} - {0})


def pool_plan(E):
    """(B, N, accumulate, offset rows, seed): B, accumulate and the mean-100 rows rotate over the N list."""
    return [(POOL_B[i % 3], N, (i // 2) % 2, i % 2 == 1, 9000 + 13 * i + E) for i, N in enumerate(pool_ns(E))]


def pool_inputs(B, N, E, dt, offset, seed):
    x = randn((B, N, E), seed, 2.0) + 0.5
    if offset:
        x[:, ::2] = randn((B, (N + 1) // 2, E), seed + 9) + 100.0       # mean 100, std 1: the two-pass variance matters
    gamma = 1 + randn((E,), seed + 1, 0.2)
    beta = randn((E,), seed + 2, 0.2)
    dp = randn((B, E), seed + 3).to(dt)
    return x.to(dt), gamma, beta, dp


def pool_fwd_ref(x, gamma, beta, eps):
    """x [B, N, E].  (pooled, mag, mean [B, N], rstd [B, N], mean|x| [B, N]) in fp64."""
    x, g, b = x.double(), gamma.double(), beta.double()
    mu = x.mean(2, keepdim=True)
    var = ((x - mu) ** 2).mean(2, keepdim=True)
    rs = 1.0 / torch.sqrt(var + eps)
    xh = (x - mu) * rs
    ax = x.abs().mean(2, keepdim=True)
    pooled = g * xh.mean(1) + b
    mag = g.abs() * (xh.abs() + rs * ax).mean(1) + b.abs()
    return pooled, mag, mu[..., 0], rs[..., 0], ax[..., 0]


def pool_bwd_ref(dp, x, gamma, mean, rstd, init=None):
    """The backward on the statistics given (the kernel's own: inputs of the operation).  dy = dpooled / N for every token.
    (dx, dxmag, dgamma, dgmag, dbeta, dbmag) in fp64."""
    x, g = x.double(), gamma.double()
    N = x.shape[1]
    d = (dp.double() / N)[:, None, :]
    mu, rs = mean.double()[..., None], rstd.double()[..., None]
    xh = (x - mu) * rs
    gv = d * g
    c1 = gv.mean(2, keepdim=True)
    c2 = (gv * xh).mean(2, keepdim=True)
    dx = rs * (gv - c1 - xh * c2)
    dxmag = rs * (gv.abs() + gv.abs().mean(2, keepdim=True) + xh.abs() * (gv * xh).abs().mean(2, keepdim=True))
    dg, dgm = (d * xh).sum((0, 1)), (d.abs() * xh.abs()).sum((0, 1))
    db, dbm = dp.double().sum(0), dp.double().abs().sum(0)
    if init is not None:
        dg, dgm = dg + init[0], dgm + init[0].abs()
        db, dbm = db + init[1], dbm + init[1].abs()
    return dx, dxmag, dg, dgm, db, dbm


def pool_c(N, E):
    """c_u of the pooled bound: the LayerNorm y term and the token sum."""
    G = pool_rows(E)
    return (LN_C["y"] * E + cdiv(N, G) + G + 2) * U


# ---------------------------------------------------------------------------------------------------------- mixup cases
MIXUP_PAIRS = [(F32, F32), (F32, BF16), (BF16, BF16)]
MIXUP_PER = (4, 1020, 1024, 1028, 50176)
MIXUP_B = (1, 2, 7)
MIXUP_BIG = (43, 200704)                       # 8 630 272 elements > 4096 * 1024 * 2: three turns of the stride loop
TARGET_CASES = [(B, C) for B in (1, 2, 257) for C in (1, 10, 1000)] + [(1024, 1000)]   # the last: B C > 2048 * 256


def mixup_regime(n):
    """(grid, turns of the stride loop) of mixup_kernel (four elements per thread)."""
    grid = min(4096, cdiv(n, 1024))
    return grid, cdiv(n, grid * 1024)


def target_regime(n):
    grid = min(2048, cdiv(n, 256))
    return grid, cdiv(n, grid * 256)


# ------------------------------------------------------------------------------------------------------------------ checks
# One function per kernel holds the check_bound calls: the GPU test passes the kernel's outputs, the CPU test the outputs of
# its fp32 emulation (and of its seeded defects) -- the same calls, the same bounds.
def same_bits(a, b):
    it = {2: torch.int16, 4: torch.int32}[a.element_size()]
    return a.contiguous().view(it) == b.contiguous().view(it)


def embed_check(feat, y, cbcr, A, tr, lam, TI, TO, where):
    """feat [npatch, 384] of type TO against the references of y, cbcr (TI, unmixed) and lam (None: no mixing).  Chroma bit
    for bit, luma by the bound of the header.  Returns the luma's worst ratio."""
    npatch = feat.shape[0]
    extra_mix = 0
    if lam is not None:
        ylo, yhi = mix_fp32(y, lam)
        clo, chi = mix_fp32(cbcr, lam)
        extra_mix = embed_bound_extra(A, tr, ylo, yhi, TI)
        yx, cx, cx2 = ylo.to(TI), clo.to(TI), chi.to(TI)
    else:
        yx, cx, cx2 = y, cbcr, cbcr
    luma, mag, extra_t, _ = embed_ref(yx, cx, A, bool(tr))
    want1 = cx.permute(0, 2, 3, 1, 4, 5).reshape(npatch, 128).float().to(TO)
    want2 = cx2.permute(0, 2, 3, 1, 4, 5).reshape(npatch, 128).float().to(TO)
    got = feat[:, 256:]
    ok = same_bits(got, want1) | same_bits(got, want2)
    assert bool(ok.all()), f"{where}: {int((~ok).sum())} chroma elements differ, first {(~ok).nonzero()[:4].tolist()}"
    return check_bound(feat[:, :256], luma, mag, TO, 1, 32 * U, where + " luma", extra=extra_t + extra_mix, tile=(1, 256))


def mixup_check(out, x, lam, TI, TO, where):
    ref, mag, _ = mixup_ref(x, lam)
    r = check_bound(out, ref, mag, TO, 1, 2 * U, where)
    if TI == TO:                                    # what rgbnm_subblock_embed_mix is defined by: the fp32 fma, rounded once
        lo, hi = mix_fp32(x, lam)
        ok = same_bits(out, lo.to(TO)) | same_bits(out, hi.to(TO))
        assert bool(ok.all()), f"{where}: {int((~ok).sum())} elements differ from the fp32 fma"
    return r


def sx_check(got, r, C, dt, where, worst):
    """got: dict with rows, loss, dl and (two-launch families) lse, T."""
    b_lse, b_T, b_rows, b_loss, b_dl = sx_bounds(r, C, dt)
    if "lse" in got:
        worst("lse", check_bound(got["lse"], r["lse"], None, F32, 0, 0, where + " lse", extra=b_lse))
        worst("T", check_bound(got["T"], r["T"], None, F32, 0, 0, where + " T", extra=b_T))
    worst("rows", check_bound(got["rows"], r["rows"], None, F32, 0, 0, where + " rows", extra=b_rows))
    worst("loss", check_bound(got["loss"].reshape(1), r["loss"].reshape(1), None, F32, 0, 0, where + " loss",
                              extra=b_loss.reshape(1)))
    worst(f"dl {NAMES[dt]}", check_bound(got["dl"], r["dl"], None, dt, 0, 0, where + " dlogits", extra=b_dl, tile=(1, 256)))


def adam_check(got, r, where, worst):
    """got: dict with p, m, v and, where norm_out was given, norm."""
    if got.get("norm") is not None:
        worst("norm", check_bound(got["norm"].reshape(1), r["norm"].reshape(1), None, F32, 1, 0, where + " norm",
                                  extra=r["dnorm"].reshape(1)))
    worst("p", check_bound(got["p"], r["p"], None, F32, 1, 0, where + " p", extra=r["dp"], tile=(256,)))
    worst("m", check_bound(got["m"], r["m"], None, F32, 1, 0, where + " m", extra=r["dm"], tile=(256,)))
    worst("v", check_bound(got["v"], r["v"], None, F32, 1, 0, where + " v", extra=r["dv"], tile=(256,)))


def pool_fwd_check(pooled, mean, rstd, x, gamma, beta, eps, dt, where, worst, key):
    B, N, E = x.shape
    pref, pmag, mu, rs, ax = pool_fwd_ref(x, gamma, beta, eps)
    worst(key + "-pooled", check_bound(pooled, pref, pmag, dt, 1, pool_c(N, E), where + " pooled"))
    cs = LN_C["stat"] * E * U
    worst(key + "-stat", check_bound(mean.view(B, N), mu, ax, F32, 1, cs, where + " mean"))
    worst(key + "-stat", check_bound(rstd.view(B, N), rs, rs, F32, 1, cs, where + " rstd"))


def pool_bwd_check(dx, dg, db, dp, x, gamma, mean, rstd, init, dt, where, worst, key):
    B, N, E = x.shape
    dxr, dxm, dgr, dgm, dbr, dbm = pool_bwd_ref(dp, x, gamma, mean.view(B, N), rstd.view(B, N), init)
    worst(key + "-dx", check_bound(dx.view(B, N, E), dxr, dxm, dt, 1, LN_C["dx"] * E * U, where + " dx"))
    worst(key + "-dgamma", check_bound(dg, dgr, dgm, F32, 1, (N + B + E) * U, where + " dgamma"))
    worst(key + "-dbeta", check_bound(db, dbr, dbm, F32, 1, (B + 2) * U, where + " dbeta"))
