"""Every 16-bit pre-activation through each GELU and tanh epilogue (tests/act_sweep_ref.py: sets, layouts, references, bounds;
tests/test_act_sweep_cpu.py proves the coverage, the bounds on an emulation and the seeded defects).

Delivery: A[m, k] = (k == m % K), W[n, k] = value, bias NULL, so u[m, n] = W[n, m % K] with no rounding; two passes put every value at
both column parities and into two row tiles; non-finite patterns and the tie set go through the fp32 bias with A = W = 0.  The
precondition -- the same operands under RGBNM_EPI_NONE return the bits put in -- is asserted per path and dtype before anything else; no
path flushes subnormal MFMA operands (had one, deliver() would send that class through the bias and record it), the only change is
-0 -> +0, so the sign of the result for -0 is not examined.  Block level: BlockSweep below.  Every output is guarded, inputs are NaN
padded, every path's kernel is asserted through the profiler (fp16 instantiations by their mangled type).

Measured on one MI355X (pytest -s prints every figure before the bit comparison is asserted); window A0 = 0x3A80, P1 = 0x4080,
N1 = 0x4180.  Worst |got - ref| / bound, gelu / gelu' (bits that differ from full65536, per pass):
    gemm_nt_kernel direct   bf16 0.9989 / 0.9996 (0, 0; 194, 194 before the fix below) f16 1.0000 / 0.9984   f32 0.1917 / 0.1501
    gemm_nt_kernel staged   bf16 0.9989 / 0.9996 (0, 0)                               f16 1.0000 / 0.9984
    gemm_nt_wres_kernel     bf16 0.9989 / 0.9996 (0, 0)                               f16 1.0000 / 0.9984
    kp7 resident            bf16 table=1 and 0: 0.9989 / 0.9996 (0, 0)                f16 1.0000 / 0.9984   (never takes the table)
    kp7 persistent          bf16 table=1 and 0: 0.9989 / 0.9996 (0, 0)                f16 1.0000 / 0.9984
    kp8                     bf16 table=1: 0.9989 / 0.9996 (0)
    mlp_fwd_kernel B=42     bf16 table=1 and 0: 0.9989 / 0.9996 (0, 0)                f16 1.0000 / 0.9984
    mlp_fwd_kernel B=257    0.9762 / 0.9840 on the window-edge slice (0): arithmetic although gelu_table = 1
    vit_chain_fwd_kernel    0.9989 / 0.9996 (0, 0); B = 2 depth 1 equals the B = 1 tables
    tanh                    bf16 0.9968 (direct, staged, small kernel)   f16 0.9994   f32 0.4891
(1.0000: the rounding tie at the smallest fp16 subnormal, inside the bound; the figures equal those of the CPU emulation.)
Non-finite inputs, gelu / gelu': arithmetic paths +inf -> +inf / NaN, -inf -> NaN / NaN, NaN -> NaN / NaN (0xFFC0, 0xFE00 staged;
0x7FC0, 0x7E00 from a NaN bias on the direct epilogue); table paths +inf -> +inf / 1, -inf -> -0 / 0, +NaN -> itself / 1, -NaN -> NaN / 0; the block-level MFMA hands
every NaN on as 0xFFC0.  tanh(+-inf) = +-1.
Found and fixed: the table lookup gave gelu = -0 for the 127 NaN patterns with the sign bit set (clamped to N1 like every large
negative input) on kp7 persistent, kp8, mlp_fwd_kernel<true> and the chain forward, and for all 254 NaN patterns on the last two;
gelu_table.h, mlp_fused.hip and vit_chain.hip now take sat(u_bits - 0xFF80) off the magnitude before the subtraction (DESIGN.md,
"Activation sweeps").  And the direct epilogue of gemm_nt_kernel spelled GELU with erff for bf16 / fp16 too: 194 bf16 inputs of the
left tail (-3.14 >= u >= -13.2) were one bf16 ulp off full65536 in gelu or gelu'; the 16-bit direct instantiations now run
gelu_pair_fast like every other 16-bit path (fp32 keeps erff), 0 differences.  Where a path may look GELU up, what ran is asserted by
gelu / gelu'(-inf): -0 / gelu'(-large) from the lookup, NaN from the arithmetic (the kernel name does not tell).
"""
import ctypes as C

import numpy as np
import pytest
import torch

import act_sweep_ref as S
import dropout_ref as D
from act_sweep_ref import BF16, F16, F32, NAMES
from kernel_check import guarded, nan_padded, launched, ran
from rgb_no_more_amd import lib as L
from test_hip_kernels import option  # noqa: F401  (fixture: set a runtime switch for one test)

pytestmark = pytest.mark.gpu
DEV = "cuda"
E_NONE, E_RES, E_GELU, E_POS, E_DGELU, E_TANH, E_DTANH = range(7)
E_GELU_DROP = 8
F16_MARKS = ("_Float16", "DF16_", "__half")          # tests/test_fp16_tuned_kernels.py
BF16_MARKS = ("__bf16", "DF16b", "bfloat16")
TAB = {}                                             # the device's full65536 and window, read once


@pytest.fixture(scope="module", autouse=True)
def gelu_table():
    lib = L.lib()
    L.check(lib.rgbnm_gelu_table_init(L.stream()), "gelu_table_init")
    win = (C.c_int * 16)()
    full = np.zeros(65536, dtype=np.uint32)
    L.check(lib.rgbnm_gelu_table_info(win, full.ctypes.data))
    assert win[0] == 1
    TAB["full"] = torch.from_numpy(full.astype(np.int64)).to(DEV)
    TAB["win"] = (win[1], win[2], win[3])
    TAB["gpn"] = win[5]
    print(f"\n[act sweep] table window A0=0x{win[1]:04X} P1=0x{win[2]:04X} N1=0x{win[3]:04X} gelu'(-large)=0x{win[5]:04X}")


def is_f16(name):
    return any(m in name for m in F16_MARKS) and not any(m in name for m in BF16_MARKS)


def obits(t):
    """Raw patterns of an output matrix as int32 (16-bit types: 0 .. 65535)."""
    return S.bits32(t) if t.dtype == F32 else S.to_bits(t)


def ibits(v):
    return S.bits32(v) if v.dtype == F32 else S.to_bits(v)


def neg_zero(dt):
    return -2 ** 31 if dt == F32 else 0x8000


def is_sub(bits, dt):
    if dt == F32:
        mag = bits & 0x7FFFFFFF
        return (mag > 0) & (mag < 0x00800000)
    return S.is_subnormal_bits(bits, dt)


def is_nan_bits(bits, dt):
    ex, full = (0x7F800000, 0x7FFFFFFF) if dt == F32 else (S._EXP[dt], 0x7FFF)
    return (bits & full) > ex


# ------------------------------------------------------------------------------------------------------------ GEMM delivery
class Path:
    """One kernel path of rgbnm_gemm_nt / rgbnm_gemm_nt_drop at one shape: runs an epilogue on given operands into guarded outputs
    and asserts the kernel that ran."""

    def __init__(self, name, dt, M, N, K, want, forbid=(), f16=False, drop=None):
        self.name, self.dt, self.M, self.N, self.K, self.want, self.forbid, self.f16, self.drop = name, dt, M, N, K, want, forbid, f16, drop
        self.flushed = None            # inputs the precondition found flushed in the MFMA operands (then delivered through the bias)
        self.neg_zero_lost = False     # the precondition saw -0 come back as +0 (the one change it allows)

    def run(self, epi, A, W, bias, N=None, R=None, drop=None, written=True):
        """written=False: an input is a NaN with the canary's payload, so "still holds the canary" proves nothing there."""
        dt, M, K = self.dt, self.M, self.K
        N = self.N if N is None else N
        A = nan_padded(A, K + 16, 3)
        W = nan_padded(W, K + 24, 3)
        Cg = guarded(M, N, dt)
        C2 = guarded(M, N, dt) if epi in (E_GELU, E_GELU_DROP) else None
        args = (L.dt_of(dt), epi, A.data_ptr(), K + 16, W.data_ptr(), K + 24, Cg.t.data_ptr(), N, L.ptr(bias), L.ptr(R), N,
                C2.t.data_ptr() if C2 else None, N, None, 0, M, N, K, 0)

        def call():
            if drop is None:
                L.check(L.lib().rgbnm_gemm_nt(*args, L.stream()))
            else:
                L.check(L.lib().rgbnm_gemm_nt_drop(*args, drop[0].data_ptr(), drop[1], drop[2], drop[3], L.stream()))
        _, names = launched(call)
        where = f"{self.name} {NAMES[dt]} epi={epi} M={M} N={N} K={K}"
        for w in self.want:
            ws = w if isinstance(w, tuple) else (w,)
            hits = [n for n in names if all(s in n for s in ws)]
            assert hits, f"{where}: kernel {ws} did not run; ran {sorted(set(names))}"
            if self.f16:
                assert all(is_f16(n) for n in hits), hits
        for f in self.forbid:
            assert not ran(names, f), f"{where}: kernel {f} ran; ran {sorted(set(names))}"
        Cg.check(where, written)
        outs = [obits(Cg.t)]
        if C2:
            C2.check(where + " C2", written)
            outs.append(obits(C2.t))
        return outs


def via_w(path, epi, vals, pass_, R=None):
    """Values through W (act_sweep_ref.gemm_operands).  Asserts on the device that every row m equals row m % K; returns per output
    the int32 patterns per value."""
    A, W, k, n = S.gemm_operands(vals, path.M, path.N, path.K, pass_)
    outs = path.run(epi, A, W, None, R=R)
    rows = torch.arange(path.M, device=DEV) % path.K
    res = []
    for o in outs:
        assert torch.equal(o, o[rows]), f"{path.name} epi={epi} pass {pass_}: rows m and m % K differ"
        res.append(o[k, n])
    return res


def via_bias(path, epi, vals32):
    """fp32 values through the bias with A = 0, W = 0, in chunks of 1535 (N = 3072): value j at the two columns of
    act_sweep_ref.bias_vector (different parities).  Asserts that all rows equal row 0; returns per output (patterns at the first
    columns, at the second)."""
    CH, N = 1535, 3072
    parts = None
    A = torch.zeros(path.M, path.K, dtype=path.dt, device=DEV)
    W = torch.zeros(N, path.K, dtype=path.dt, device=DEV)
    for c0 in range(0, vals32.numel(), CH):
        v = vals32[c0:c0 + CH]
        bias, off = S.bias_vector(v, N)
        outs = path.run(epi, A, W, bias, N=N, written=not bool(torch.isnan(v).any()))
        if parts is None:
            parts = [([], []) for _ in outs]
        for o, (p0, p1) in zip(outs, parts):
            assert bool((o == o[0]).all()), f"{path.name} epi={epi}: rows differ on the bias delivery"
            p0.append(o[0, :v.numel()])
            p1.append(o[0, off:off + v.numel()])
    return [(torch.cat(p0), torch.cat(p1)) for p0, p1 in parts]


def intended_bits(vals):
    """What EPI_NONE must return for values delivered through W (non-finite ones are replaced by 0 there)."""
    return ibits(torch.where(torch.isfinite(vals), vals, torch.zeros_like(vals)))


def same_or_pos_zero(got, want, dt):
    return (got == want) | ((want == neg_zero(dt)) & (got == 0))


def deliver(path, epi, vals, passes=2, R=None):
    """The precondition (EPI_NONE returns the intended bits; only -0 -> +0 allowed) on the same operands, then `epi`.  Values the
    MFMA operands cannot carry go through the bias: non-finite ones always, and the SUBNORMAL class when the precondition shows that
    the path flushes it (recorded in path.flushed).  Returns [pass][output] -> int32 patterns per value."""
    dt = path.dt
    vb = ibits(vals)
    fin = torch.isfinite(vals)
    want = intended_bits(vals)
    by_bias = ~fin
    for p in range(passes):
        got = via_w(path, E_NONE, vals, p)[0]
        bad = ~same_or_pos_zero(got, want, dt)
        path.neg_zero_lost = path.neg_zero_lost or bool(((want == neg_zero(dt)) & (got == 0)).any())
        if bool(bad.any()):
            sub = is_sub(vb, dt)
            assert bool((bad & ~sub).sum() == 0), (f"{path.name} {NAMES[dt]} pass {p}: EPI_NONE does not return "
                                                    f"{int((bad & ~sub).sum())} normal values, first bits {vb[bad & ~sub][:6].tolist()}")
            by_bias = by_bias | sub
            path.flushed = int(bad.sum())
    res = [via_w(path, epi, vals, p, R=R) for p in range(passes)]
    if bool(by_bias.any()) and R is None:
        v32 = vals[by_bias].float()
        pre = via_bias(path, E_NONE, v32)[0]
        wb = vb[by_bias]
        for q in range(2):
            ok = (pre[q] == wb) | (is_nan_bits(wb, dt) & is_nan_bits(pre[q], dt))
            assert bool(ok.all()), f"{path.name} {NAMES[dt]}: the bias delivery does not return bits {wb[~ok][:6].tolist()}"
        act = via_bias(path, epi, v32)
        for p in range(passes):
            for o in range(len(res[p])):
                res[p][o][by_bias] = act[o][p]
    return res


def ties(path, epi, tabs):
    """S_tie through the bias: the rounding itself (EPI_NONE gives rne_T(u)), then the epilogue's result for it."""
    dt = path.dt
    u, want = S.s_tie(dt, DEV)
    pre = via_bias(path, E_NONE, u)[0]
    act = via_bias(path, epi, u)
    for q in range(2):
        S.assert_ties(f"{path.name} {NAMES[dt]} rounding, column parity {q}", dt, want, pre[q], torch.arange(65536, device=DEV, dtype=torch.int32))
        for o in range(len(act)):
            tab = tabs[q][o]
            if path.neg_zero_lost:               # the table's entry for -0 is the result for +0 (deliver): the epilogue's results are odd at 0
                tab = tab.clone()
                tab[0x8000] = tab[0] ^ (0x8000 if o == 0 else 0)
            S.assert_ties(f"{path.name} {NAMES[dt]} epi={epi} output {o}, column parity {q}", dt, want, act[o][q], tab)


def report(where, **kw):
    print(f"\n[act sweep] {where}: " + ", ".join(f"{k}={v}" for k, v in kw.items()))


def gelu_sweep_16(path, with_ties=False, passes=2, table=False):
    """Assertions 1 - 6 for one 16-bit path: both passes (column parities), every pattern.  The bit comparison with full65536 and
    the non-finite inputs come last so that every figure is printed first.  table: the path is expected to look GELU up.  Table and
    arithmetic give the same bits for finite inputs and the kernel name is the same, so what ran is told by gelu / gelu' of -inf:
    -0 / gelu'(-large) from the lookup, NaN from the arithmetic -- asserted either way."""
    dt = path.dt
    vals = S.all_patterns(dt, DEV)
    res = deliver(path, E_GELU, vals, passes)
    ndiff, worst = [], {}
    for p in range(passes):
        g, d = res[p]
        where = f"{path.name} {NAMES[dt]} pass {p} (value j at column parity {'j' if p == 0 else 'j + 1'})"
        w = S.check_gelu_tables(where, dt, g, d, exact=False, nonfinite=False, neg_zero_lost=path.neg_zero_lost)
        worst = {k: max(v, worst.get(k, 0.0)) for k, v in w.items()}
        if dt == BF16:
            ndiff.append(int(S.count_full_diffs(g, d, TAB["full"]).numel()))
    report(f"{path.name} {NAMES[dt]}", worst={k: f"{v:.4f}" for k, v in worst.items()}, full65536_diffs=ndiff,
           nonfinite=S.nonfinite_summary(dt, *res[0]), flushed_mfma_operands=path.flushed, neg_zero_lost=path.neg_zero_lost)
    if with_ties:
        ties(path, E_GELU, res if passes == 2 else [res[0], res[0]])
    for p in range(passes):
        where = f"{path.name} {NAMES[dt]} pass {p}"
        if dt == BF16:
            S.assert_full_bits(where, res[p][0], res[p][1], TAB["full"], TAB["win"])
        S.assert_nonfinite(where, dt, res[p][0])
        assert_lookup_ran(where, dt, res[p], table)
    return res


def assert_lookup_ran(where, dt, tabs, table):
    ninf = 0x8000 | S._EXP[dt]
    g, d = int(tabs[0][ninf]), int(tabs[1][ninf])
    if table:
        assert (g, d) == (0x8000, TAB["gpn"]), f"{where}: gelu / gelu'(-inf) = 0x{g:04X} / 0x{d:04X}: the table lookup did not run"
    else:
        assert is_nan_bits(torch.tensor(g), dt), f"{where}: gelu(-inf) = 0x{g:04X}: the arithmetic did not run"


def generic_opts(option, staged):
    for o in ("nt_small", "nt_kpipe", "nt_wres"):
        option(o, 0)
    option("nt_staged", staged)


# ------------------------------------------------------------------------------------------------------------------ paths 1, 2
@pytest.mark.parametrize("dt,staged", [(BF16, 0), (F16, 0), (BF16, 1), (F16, 1)], ids=lambda v: NAMES.get(v, str(v)))
def test_generic_kernel_gelu(option, dt, staged):
    """gemm_nt_kernel, direct and staged epilogue (gelu_pair_fast in both for the 16-bit types), M = N = K = 256: one call holds a
    whole set."""
    generic_opts(option, staged)
    path = Path(f"gemm_nt_kernel staged={staged}", dt, 256, 256, 256, ("gemm_nt_kernel",))
    gelu_sweep_16(path, with_ties=bool(staged))


def test_generic_kernel_gelu_fp32(option):
    """The direct fp32 epilogue on S_f32 (the finite values of both 16-bit sets), two chunks of <= 65 536 values, two passes each."""
    generic_opts(option, 0)
    path = Path("gemm_nt_kernel direct", F32, 256, 256, 256, ("gemm_nt_kernel",))
    vals = S.s_f32(DEV)
    special = torch.tensor([float("inf"), float("-inf"), float("nan")], device=DEV)
    worst = {}
    chunks = [deliver(path, E_GELU, vals[c0:c0 + 65536]) for c0 in range(0, vals.numel(), 65536)]
    for p in range(2):
        g, d = (torch.cat([c[p][o].view(F32) for c in chunks]) for o in range(2))
        where = f"gemm_nt_kernel direct f32 pass {p}"
        w = {"gelu": S.assert_bound(where, "gelu", vals, g, F32), "gelu'": S.assert_bound(where, "dgelu", vals, d, F32)}
        S.assert_gelu_properties(where, vals, g, skip=(S.bits32(vals) == neg_zero(F32)) if path.neg_zero_lost else None)
        worst = {k: max(v, worst.get(k, 0.0)) for k, v in w.items()}
    sp = via_bias(path, E_GELU, special)
    gs, ds = sp[0][0].view(F32), sp[1][0].view(F32)
    report("gemm_nt_kernel direct f32", worst={k: f"{v:.4f}" for k, v in worst.items()}, flushed_mfma_operands=path.flushed,
           nonfinite=dict(zip(("+inf", "-inf", "nan"), zip(gs.tolist(), ds.tolist()))))
    assert float(gs[0]) == float("inf") and bool(torch.isnan(gs[2]))


# ---------------------------------------------------------------------------------------------------------------- paths 3, 4
def tuned_opts(option, dt):
    generic_opts(option, 1)
    if dt == F16:
        option("f16_tuned", 1)


@pytest.mark.parametrize("dt", [BF16, F16], ids=lambda v: NAMES[v])
def test_weight_resident_gelu(option, dt):
    """gemm_nt_wres_kernel (M = 4096, N = 384, K = 192): rows k and k + 192 carry the same values, 21 times over."""
    tuned_opts(option, dt)
    option("nt_wres", 1)
    path = Path("gemm_nt_wres_kernel", dt, 4096, 384, 192, ("gemm_nt_wres_kernel",), ("gemm_nt_kernel",), f16=(dt == F16))
    gelu_sweep_16(path, with_ties=True)


@pytest.mark.parametrize("dt,table", [(BF16, 1), (BF16, 0), (F16, 0)], ids=lambda v: NAMES.get(v, str(v)))
@pytest.mark.parametrize("persist", [0, 1])
def test_row_panel_kp7_gelu(option, persist, dt, table):
    """kp7 resident / persistent (M = 8193, N = 384, K = 256), bf16 by table and by arithmetic, the fp16 instantiation (arithmetic)."""
    tuned_opts(option, dt)
    option("nt_kpipe", 1)
    option("kp_persist", persist)
    option("kp8", 0)
    option("gelu_table", table)
    kern = "gemm_nt_kpipe_persist_kernel" if persist else "gemm_nt_kpipe_kernel"
    path = Path(f"kp7 persist={persist} table={table}", dt, 8193, 384, 256, (("kp7", kern),), ("gemm_nt_kernel",), f16=(dt == F16))
    gelu_sweep_16(path, with_ties=True, table=bool(table and persist))     # the resident kp7 kernel has no room for the image


def test_row_panel_kp8_gelu(option):
    """kp8 (M = 16384, N = 768, K = 256), table, one pass of S_bf16."""
    tuned_opts(option, BF16)
    option("nt_kpipe", 1)
    option("kp8", 1)
    option("gelu_table", 1)
    path = Path("kp8 table=1", BF16, 16384, 768, 256, (("kp8", "gemm_nt_kpipe"),), ("gemm_nt_kernel", "kp7"))
    gelu_sweep_16(path, with_ties=True, passes=1, table=True)


# -------------------------------------------------------------------------------------------------------------------- path 7
def seed_tensor(seed):
    return torch.tensor([seed], dtype=torch.int64, device=DEV)


@pytest.mark.parametrize("dt,staged", [(F32, 0), (BF16, 0), (F16, 0), (BF16, 1), (F16, 1)], ids=lambda v: NAMES.get(v, str(v)))
def test_gelu_drop_epilogue(option, dt, staged):
    """rgbnm_gemm_nt_drop RGBNM_EPI_GELU_DROP.  p = 0: the bits of the same path's RGBNM_EPI_GELU, both outputs, whole matrices.
    p = 0.5 (scale 2): dropped elements are +0 in both outputs; kept ones are exactly twice the p = 0 value wherever that doubling is
    exact in T -- the p = 0 value T(x) lies ABOVE the smallest normal and its double is finite: rounding is monotone, so the fp32 x it
    came from is normal in T too and T(2 x) = 2 T(x).  (A subnormal, zero or smallest-normal T(x) may come from an x with bits that
    T(2 x) keeps and T(x) lost: 2^-133 x 255 / 2 rounds to 2^-126, its double is exact.)  fp32: S_f32 in two calls.  No EPI_NONE
    precondition here: kernel, shape and operands are those whose delivery test_generic_kernel_gelu proves; non-finite inputs
    stay out (W holds 0 for them)."""
    generic_opts(option, staged)
    M = N = K = 256
    path = Path(f"gemm_nt_drop staged={staged}", dt, M, N, K, ("gemm_nt_kernel",))
    sets = [S.all_patterns(dt, DEV)] if dt != F32 else list(S.s_f32(DEV).split(65536))
    seed, site, block = 0x0123456789ABCDEF, 1, 3
    st = seed_tensor(seed)
    keep = torch.from_numpy(D.keep(seed, 0.5, site, block, M, N)).to(DEV)
    minnorm = {F32: 2.0 ** -126, BF16: 2.0 ** -126, F16: 2.0 ** -14}[dt]
    for p, vals in [(p, v) for v in sets for p in range(2)]:
        A, W, k, n = S.gemm_operands(vals, M, N, K, p)
        base = path.run(E_GELU, A, W, None)
        p0 = path.run(E_GELU_DROP, A, W, None, drop=(st, 0.0, site, block))
        p5 = path.run(E_GELU_DROP, A, W, None, drop=(st, 0.5, site, block))
        for o, nm in enumerate(("gelu", "gelu'")):
            where = f"gemm_nt_drop {NAMES[dt]} staged={staged} pass {p} {nm}"
            assert torch.equal(base[o], p0[o]), f"{where}: p = 0 differs from RGBNM_EPI_GELU at {int((base[o] != p0[o]).sum())} elements"
            assert bool((p5[o][~keep] == 0).all()), f"{where}: a dropped element is not +0"
            x0 = (base[o].view(F32) if dt == F32 else S.from_bits(base[o].flatten(), dt, DEV).view(M, N)).double()
            x5 = (p5[o].view(F32) if dt == F32 else S.from_bits(p5[o].flatten(), dt, DEV).view(M, N)).double()
            exact = keep & torch.isfinite((2 * x0).to(dt).double()) & (x0.abs() > minnorm)
            bad = exact & (x5 != 2 * x0)
            assert int(bad.sum()) == 0, f"{where}: {int(bad.sum())} kept elements are not twice the p = 0 value, first {bad.nonzero()[:4].tolist()}"
            assert int(exact.sum()) > 15000, int(exact.sum())


# ----------------------------------------------------------------------------------------------------------------- paths 8, 9
def tanh_sweep_16(path):
    dt = path.dt
    vals = S.all_patterns(dt, DEV)
    res = deliver(path, E_TANH, vals)
    worst = 0.0
    for p in range(2):
        where = f"{path.name} {NAMES[dt]} tanh pass {p}"
        worst = max(worst, S.check_tanh_table(where, dt, res[p][0], path.neg_zero_lost)["tanh"])
    h = res[0][0]
    report(f"{path.name} {NAMES[dt]}", worst_tanh=f"{worst:.4f}", flushed_mfma_operands=path.flushed,
           nonfinite={k: f"0x{int(h[i]):04X}" for k, i in (("+inf", S._EXP[dt]), ("-inf", 0x8000 | S._EXP[dt]))})
    return res


@pytest.mark.parametrize("dt,staged", [(BF16, 0), (F16, 0), (BF16, 1), (F16, 1)], ids=lambda v: NAMES.get(v, str(v)))
def test_generic_kernel_tanh(option, dt, staged):
    """RGBNM_EPI_TANH on gemm_nt_kernel, direct and staged, M = N = K = 256."""
    generic_opts(option, staged)
    path = Path(f"gemm_nt_kernel staged={staged}", dt, 256, 256, 256, ("gemm_nt_kernel",))
    res = tanh_sweep_16(path)
    if staged:
        ties(path, E_TANH, res)


def test_generic_kernel_tanh_fp32(option):
    generic_opts(option, 0)
    path = Path("gemm_nt_kernel direct", F32, 256, 256, 256, ("gemm_nt_kernel",))
    vals = S.s_f32(DEV)
    key = S.bits32(vals).to(torch.int64)
    key = torch.where(key < 0, -(key & 0x7FFFFFFF) - 1, key)
    nkey = S.bits32(-vals).to(torch.int64)
    neg_of = torch.searchsorted(key, torch.where(nkey < 0, -(nkey & 0x7FFFFFFF) - 1, nkey))
    worst = 0.0
    chunks = [deliver(path, E_TANH, vals[c0:c0 + 65536]) for c0 in range(0, vals.numel(), 65536)]
    for p in range(2):
        h = torch.cat([c[p][0].view(F32) for c in chunks])
        where = f"gemm_nt_kernel direct f32 tanh pass {p}"
        worst = max(worst, S.assert_bound(where, "tanh", vals, h, F32))
        S.assert_tanh_properties(where, vals, h, neg_of, skip=(S.bits32(vals) == neg_zero(F32)) if path.neg_zero_lost else None)
    sp = via_bias(path, E_TANH, torch.tensor([float("inf"), float("-inf"), float("nan")], device=DEV))[0][0].view(F32)
    report("gemm_nt_kernel direct f32", worst_tanh=f"{worst:.4f}", nonfinite=sp.tolist(), flushed_mfma_operands=path.flushed)
    assert sp[:2].tolist() == [1.0, -1.0] and bool(torch.isnan(sp[2]))


def test_small_kernel_tanh_and_dtanh(option):
    """gemm_nt_small_kernel (bf16, M = N = K = 256, 32 x 32 tiles): RGBNM_EPI_TANH, and RGBNM_EPI_DTANH with R = +-1 (the product
    is 0 for every finite pre-activation) and R = 0 (the product is the pre-activation, bit for bit)."""
    generic_opts(option, 1)
    option("nt_small", 1)
    path = Path("gemm_nt_small_kernel", BF16, 256, 256, 256, ("gemm_nt_small_kernel",), ("gemm_nt_kernel",))
    res = tanh_sweep_16(path)
    ties(path, E_TANH, res)
    vals = S.all_patterns(BF16, DEV)
    fin = torch.isfinite(vals)
    want = intended_bits(vals)
    for r in (1.0, -1.0, 0.0):
        R = torch.full((256, 256), r, dtype=BF16, device=DEV)
        out = deliver(path, E_DTANH, vals, R=R)
        for p in range(2):
            got = out[p][0]
            if r:
                assert bool(((got & 0x7FFF) == 0)[fin].all()), f"dtanh R={r} pass {p}: pre * (1 - R^2) is not 0"
            else:
                ok = same_or_pos_zero(got, want, BF16) | (S.is_subnormal_bits(want, BF16) if path.flushed else False)
                assert bool(ok[fin].all()), f"dtanh R=0 pass {p}: {int((~ok)[fin].sum())} products differ from the pre-activation"


# ------------------------------------------------------------------------------------------------------------ paths 5a, 5b, 6
import block_ref as R                    # noqa: E402
import test_block_edges as TB            # noqa: E402
from rgb_no_more_amd import chain        # noqa: E402

HID, EMB = S.HID, R.E
VECS = ("ln1_g", "ln1_b", "ln2_g", "ln2_b", "bqkv", "bproj", "b1", "b2")
MATS = ("wqkv", "wproj", "w1", "w2")


class BlockSweep:
    """One (B, depth) case of tests/test_block_edges.py with ln2_g = 0, ln2_b = e_0 (every row of xn2 is e_0: asserted on the stored
    xn2), w1[n, 0] = value_n and nothing else, b1 = 0 (or the tie values with w1 = 0), w2 = 0, b2 = 0: u[:, n] = value_n, and x_out =
    x_mid stays finite for the next block.  1 * (-0) + 0 + ... = +0: the input -0 is delivered as +0 (neg_zero_lost)."""
    neg_zero_lost = True

    def __init__(self, B, depth, dt=BF16):
        orig = R.make_params

        def mp(depth_, seed=1, e=R.E, heads=R.HEADS, offset=None):
            P = orig(depth_, seed, e, heads, offset)
            for p in P:
                p["ln2_g"], p["ln2_b"] = torch.zeros(e), torch.zeros(e)
                p["ln2_b"][0] = 1.0
                p["w1"], p["b1"], p["w2"], p["b2"] = torch.zeros(4 * e, e), torch.zeros(4 * e), torch.zeros(e, 4 * e), torch.zeros(e)
            return P
        R.make_params = mp
        try:
            self.c = TB.Case(B, depth, images=False, dt=dt)
        finally:
            R.make_params = orig
        self.dt, self.depth, self.B = dt, depth, B
        self.idx = None

    def load(self, slices, biases=None):
        """slices / biases: per block a [768] tensor of dt / fp32 (or None: zeros)."""
        for i, p in enumerate(self.c.P):
            p["w1"].zero_()
            p["b1"].zero_()
            if slices is not None and i < len(slices):
                p["w1"][:, 0] = slices[i]
            if biases is not None and i < len(biases):
                p["b1"].copy_(biases[i])
            p["w1_t"] = p["w1"].T.contiguous()

    def read(self, acts, nblk, where, written=True):
        """Per block (gelu, gelu') patterns of row 0 after asserting, on the device, xn2 = e_0 and that all rows equal row 0."""
        out = []
        for i in range(nblk):
            a = acts[i]
            for k in ("xn2", "gl", "u"):
                a[k].check(f"{where} block {i} {k}", written)
            xn2 = a["xn2"].t
            assert bool((xn2[:, 0] == 1).all()) and bool((xn2[:, 1:] == 0).all()), f"{where} block {i}: xn2 is not e_0"
            g, d = S.to_bits(a["gl"].t), S.to_bits(a["u"].t)
            assert bool((g == g[0]).all()) and bool((d == d[0]).all()), f"{where} block {i}: rows differ"
            out.append((g[0].clone(), d[0].clone()))
        return out

    # the per-operation entry, one block per launch
    def run_perop(self, where, expect=None, written=True):
        c, lib = self.c, L.lib()
        acts = c.new_acts()
        p = c.P[0]
        bp = L.BlockParams(*[p[k].data_ptr() for k in VECS], *[t.data_ptr() for k in MATS for t in (p[k], p[k + "_t"])])
        ba = L.BlockActs(*[c.act_tensors(acts, 0)[k].data_ptr() for k, _ in L.BlockActs._fields_])

        def call():
            L.check(lib.rgbnm_vit_block_fwd(C.byref(c.cfg), C.byref(bp), C.byref(ba), L.stream()), where)
        if expect is not None:
            _, names = launched(call)
            expect(names)
        else:
            call()
        return self.read(acts, 1, where, written)

    # the one-launch forward, `depth` blocks per launch
    def run_chain(self, where, written=True):
        c = self.c
        if self.idx is None:
            off, idx = 0, []
            for p in c.P:
                o = {}
                for k in MATS:
                    o[k] = off
                    off += 2 * p[k].numel()
                idx.append(chain.block_index(o["wqkv"], o["wproj"], o["w1"], o["w2"]))
            assert chain.BLOCK_ELEMS == L.lib().rgbnm_chain_image_elems()
            self.idx = torch.from_numpy(np.concatenate(idx).astype(np.int32)).to(DEV)
        shadow = torch.cat([t.reshape(-1) for p in c.P for k in MATS for t in (p[k], p[k + "_t"])])
        img = guarded(self.idx.numel(), None, BF16)
        L.check(L.lib().rgbnm_chain_gather(shadow.data_ptr(), self.idx.data_ptr(), img.t.data_ptr(), self.idx.numel(), L.stream()), "chain_gather")
        torch.cuda.synchronize()
        img.check("chain image", written=False)
        assert torch.equal(S.to_bits(img.t), S.to_bits(shadow[self.idx.long()]))
        c.img = img
        acts = c.new_acts()
        blocks = c.fwd_table(acts)
        rc, names = launched(lambda: L.lib().rgbnm_vit_chain_fwd(C.byref(c.cfg), blocks, self.depth, c.x0.data_ptr(), L.stream()))
        assert rc == 0, rc
        assert len(names) == 1 and "vit_chain_fwd_kernel" in names[0], names
        return self.read(acts, self.depth, where, written)


def finite_or_zero(v):
    return torch.where(torch.isfinite(v), v, torch.zeros_like(v))


BLOCK_CH = 383          # values of a bias_vector slice of HID = 768 columns (2 x 383 <= 768)


def block_sweep_tables(bs, run, where, passes=2):
    """All 65 536 patterns of bs.dt through `run` (a launch of bs.depth blocks): the finite ones in slices of 768, the second pass
    one column on; the non-finite ones in launches of their own, 383 at a time at the two columns of act_sweep_ref.bias_vector, in the LAST block only
    (their NaN reaches x_out, which nobody reads).  Returns [pass] -> (gelu table, gelu' table)."""
    dt, depth = bs.dt, bs.depth
    vals = S.all_patterns(dt, DEV)
    fin = torch.isfinite(vals)
    res = []
    for p in range(passes):
        blk, col, nblk = S.block_slots(65536, p)
        slot = (blk * HID + col).to(DEV)
        nl = -(-nblk // depth)
        V = torch.zeros(nl * depth * HID, dtype=dt, device=DEV)
        V[slot] = finite_or_zero(vals)
        G, Dv = [], []
        for l in range(nl):
            bs.load([V[(l * depth + i) * HID:(l * depth + i + 1) * HID] for i in range(depth)])
            for g, d in run(f"{where} pass {p} launch {l}"):
                G.append(g)
                Dv.append(d)
        res.append([torch.cat(G)[slot], torch.cat(Dv)[slot]])
    nf = (~fin).nonzero().flatten()
    zero = torch.zeros(HID, dtype=dt, device=DEV)
    for c0 in range(0, nf.numel(), BLOCK_CH):
        ix = nf[c0:c0 + BLOCK_CH]
        sl, off = S.bias_vector(vals[ix], HID)
        bs.load([zero] * (depth - 1) + [sl])
        g, d = run(f"{where} non-finite {c0}", written=False)[-1]
        for p in range(passes):
            o = off * p
            res[p][0][ix], res[p][1][ix] = g[o:o + ix.numel()], d[o:o + ix.numel()]
    return res


def block_ties(bs, run, where, tabs):
    dt, depth = bs.dt, bs.depth
    u, want = S.s_tie(dt, DEV)
    chunks = [(c0, u[c0:c0 + BLOCK_CH]) for c0 in range(0, u.numel(), BLOCK_CH)]
    got = [[torch.zeros_like(want), torch.zeros_like(want)] for _ in range(2)]
    for l0 in range(0, len(chunks), depth):
        biases, offs = zip(*[S.bias_vector(v, HID) for _, v in chunks[l0:l0 + depth]])
        bs.load(None, biases)
        outs = run(f"{where} ties launch {l0 // depth}")
        for (c0, v), off, (g, d) in zip(chunks[l0:l0 + depth], offs, outs):
            for q in range(2):
                got[q][0][c0:c0 + v.numel()] = g[off * q:off * q + v.numel()]
                got[q][1][c0:c0 + v.numel()] = d[off * q:off * q + v.numel()]
    for q in range(2):
        for o in range(2):
            tab = tabs[q][o].clone()
            tab[0x8000] = tab[0] ^ (0x8000 if o == 0 else 0)          # -0 never reached the tables (BlockSweep); gelu is odd at 0
            S.assert_ties(f"{where} output {o}, column parity {q}", dt, want, got[q][o], tab)


def block_checks(name, dt, res, table, passes=2):
    ndiff, worst = [], {}
    for p in range(passes):
        g, d = res[p]
        w = S.check_gelu_tables(f"{name} pass {p}", dt, g, d, exact=False, nonfinite=False, neg_zero_lost=True)
        worst = {k: max(v, worst.get(k, 0.0)) for k, v in w.items()}
        if dt == BF16:
            ndiff.append(int(S.count_full_diffs(g, d, TAB["full"]).numel()))
    report(f"{name} {NAMES[dt]}", worst={k: f"{v:.4f}" for k, v in worst.items()}, full65536_diffs=ndiff,
           nonfinite=S.nonfinite_summary(dt, *res[0]))
    for p in range(passes):
        if dt == BF16:
            S.assert_full_bits(f"{name} bf16 pass {p}", res[p][0], res[p][1], TAB["full"], TAB["win"])
        S.assert_nonfinite(f"{name} pass {p}", dt, res[p][0])
        assert_lookup_ran(f"{name} pass {p}", dt, res[p], table)


@pytest.mark.parametrize("dt,table", [(BF16, 1), (BF16, 0), (F16, 0)], ids=lambda v: NAMES.get(v, str(v)))
def test_fused_mlp_forward_gelu(option, dt, table):
    """mlp_fwd_kernel through rgbnm_vit_block_fwd at B = 42 (8232 rows, 33 per panel: the table kernel with gelu_table = 1), the
    arithmetic kernel with gelu_table = 0, and its fp16 instantiation (f16_tuned = 2)."""
    option("fwd_chain", 0)
    option("gelu_table", table)
    if dt == F16:
        option("f16_tuned", 2)
    bs = BlockSweep(42, 1, dt)
    seen = []

    def expect(names):
        hits = [n for n in names if "mlp_fwd_kernel" in n]
        assert hits, sorted(set(names))
        assert TB.table_kernel(names) == bool(table), sorted(set(names))
        if dt == F16:
            assert all(is_f16(n) for n in hits), hits
        seen.append(1)

    def run(where, written=True):
        return bs.run_perop(where, expect if not seen else None, written)
    name = f"mlp_fwd_kernel B=42 table={table}"
    res = block_sweep_tables(bs, run, name)
    block_checks(name, dt, res, bool(table))
    block_ties(bs, run, name, res)


def test_fused_mlp_forward_above_the_table_rows(option):
    """B = 257: 197 rows per panel, above F_TAB_ROWS, so the arithmetic kernel runs although gelu_table is on.  One launch, one
    768-value slice with A0-1, A0, P1-1, P1, N1-1, N1 of both signs at both column parities: the bits of full65536 and the bound."""
    option("fwd_chain", 0)
    option("gelu_table", 1)
    bs = BlockSweep(257, 1)
    assert R.mlp_fwd_panel_rows(257 * R.NTOK) == (197, False)
    sl = S.edge_slice(*TAB["win"])
    vals = S.from_bits(sl, BF16, DEV)
    bs.load([vals])

    def expect(names):
        assert ran(names, "mlp_fwd_kernel") and not TB.table_kernel(names), sorted(set(names))
    g, d = bs.run_perop("mlp_fwd_kernel B=257", expect)[0]
    slb = torch.from_numpy(sl).to(DEV)
    got = g.to(torch.int64) | (d.to(torch.int64) << 16)
    want = TAB["full"][slb]
    nz = slb != 0                                                    # (the filler 0 between the two copies of the edges)
    wg = S.assert_bound("mlp_fwd_kernel B=257", "gelu", vals, S.from_bits(g, BF16, DEV), BF16, nz)
    wd = S.assert_bound("mlp_fwd_kernel B=257", "dgelu", vals, S.from_bits(d, BF16, DEV), BF16, nz)
    bad = (nz & (got != want)).nonzero().flatten()
    edges = {v: k for k, v in S.window_edges(*TAB["win"]).items()}
    report("mlp_fwd_kernel B=257 (arithmetic although gelu_table = 1)", worst_gelu=f"{wg:.4f}", worst_dgelu=f"{wd:.4f}", full65536_diffs=int(bad.numel()))
    assert bad.numel() == 0, "differs from full65536 at " + ", ".join(
        f"u=0x{int(slb[i]):04X} ({edges.get(int(slb[i]), '-')}, column {int(i)}) got=0x{int(got[i]):08X} want=0x{int(want[i]):08X}" for i in bad[:8].tolist())


def test_chain_forward_gelu(option):
    """vit_chain_fwd_kernel at B = 1, depth = 12 (9216 values per launch, eight launches per pass), and once more at B = 2,
    depth = 1 with the window-edge slice."""
    bs = BlockSweep(1, 12)
    name = "vit_chain_fwd_kernel B=1 depth=12"
    res = block_sweep_tables(bs, bs.run_chain, name)
    block_checks(name, BF16, res, True)
    block_ties(bs, bs.run_chain, name, res)
    b2 = BlockSweep(2, 1)
    sl = S.edge_slice(*TAB["win"])
    b2.load([S.from_bits(sl, BF16, DEV)])
    g, d = b2.run_chain("vit_chain_fwd_kernel B=2 depth=1")[0]
    slb = torch.from_numpy(sl).to(DEV)
    nz = slb != 0
    assert torch.equal(g[nz], res[0][0][slb][nz]) and torch.equal(d[nz], res[0][1][slb][nz]), "B = 2 differs from the B = 1 tables"
    got = g.to(torch.int64) | (d.to(torch.int64) << 16)
    assert torch.equal(got[nz], TAB["full"][slb][nz])
