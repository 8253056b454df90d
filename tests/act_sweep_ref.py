"""Inputs, layouts, fp64 references, bounds and an fp32 emulation for the activation sweeps (a plain module, imported by name from
tests/test_act_sweep.py and tests/test_act_sweep_cpu.py; everything here runs on whatever device its tensors are on).

A pre-activation of the bf16 / fp16 paths is 16 bits, so a sweep hands EVERY pattern to an epilogue, exactly, and reads back a
result table  tab[bits of u] = (gelu, gelu')  or  tanh.  The assertions below are stated on such tables.

Sets.  S_bf16 / S_f16: all 65 536 patterns (index = bits).  S_f32: the finite values of both, as fp32 (direct fp32 epilogue).
S_tie(T): for every 16th positive magnitude a and both signs the fp32 midpoint of (a, a + 1) and one fp32 ulp either side of it;
the expected result is the path's own result for rne_T(u) (a is even: the midpoint goes to a).

Layouts.  GEMM: A[m, k] = (k == m % K), W[n, k] = value, so u[m, n] = W[n, m % K] (one non-zero product, exact).  Value j sits at
k = j / N, n = j % N in the first pass and at (k + K / 2) % K, (n + 1) % N in the second: the other column parity (N is even), K / 2
rows on (another row tile where M = K; where M >= 2 K rows k and k + K already lie in different tiles).  Block level: xn2 = e_0,
w1[n, 0] = value, so u[:, n] = value; block b of a launch takes the 768-value slice b, the second pass shifted by one column.

Bounds (assertion 4 of the sweep).  |got - ref| <= ulp_T(|ref| + E) / 2 + E, ref in fp64 (gelu64 / dgelu64 below: the formulas of
tests/test_kernel_edges.py with erfc(-x / sqrt 2) for 1 + erf(x / sqrt 2), which keeps the left tail's relative precision).  E is that
file's constants for the same approximations without its input-rounding term (the input is exact):
    gelu:  2^-22 |u| + 2 ulp_f32(ref)        gelu': 2^-21 + 2 ulp_f32(ref)        tanh: 2 ulp_f32(ref)
plus, for gelu / gelu', a term for the hardware v_rcp_f32 and v_exp_f32 of common.h gelu_pair_fast (one ulp each by the ISA manual,
i.e. relative errors d1, d2 <= 2^-23), DERIVED here and fixed before any device run:
    Q = P(t) e,  P(t) = sum_{i=1..5} a_i t^i,  t = rcp(1 + p z),  e = exp2(-z^2):    dQ / Q = L(t) d1 + d2,  L = t P'(t) / P(t).
    L is 1 for t -> 0, dips to 0.97 and reaches sum i a_i / sum a_i = 3.44 at t = 1 (u = 0); HW_L = 3.5 bounds it (test_act_sweep_cpu.py checks a grid).
    gelu = u Phi, Phi = 1 - Q or Q:   |d gelu|  <= |u| Q (HW_L + 1) 2^-23
    gelu' = Phi + px, px = c e u:     |d gelu'| <= Q (HW_L + 1) 2^-23 + |u| phi(u) 2^-23
(Q = erfc(|u| / sqrt 2) / 2 <= 1 / 2: at most 1.1 2^-22 |u|, and nothing in either tail.)
"""
import math

import numpy as np
import torch

from kernel_check import ulp

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
NAMES = {F32: "f32", BF16: "bf16", F16: "f16"}
SQRT1_2 = 1.0 / math.sqrt(2.0)
HW_L = 3.5                       # max of t P'(t) / P(t) on (0, 1] (3.444 at t = 1), see the docstring
HW_REL = 2.0 ** -23              # one ulp of v_rcp_f32 / v_exp_f32 as a relative error
# A&S 7.1.26 as common.h spells it
AS_P = 0.3275911
AS_A = (0.254829592, -0.284496736, 1.421413741, -1.453152027, 1.061405429)
HID = 768                        # hidden width of the block-level paths (4 E, E = 192)
_EXP = {BF16: 0x7F80, F16: 0x7C00}
_MINNORM = {BF16: 0x0080, F16: 0x0400}


# ------------------------------------------------------------------------------------------------------------------- patterns
def from_bits(bits, dt, device="cpu"):
    """int array / tensor of 16-bit patterns -> tensor of dt."""
    b = torch.as_tensor(np.asarray(bits.cpu() if torch.is_tensor(bits) else bits).astype(np.uint16).view(np.int16))
    return b.view(dt).to(device)


def to_bits(t):
    """16-bit float tensor -> int32 tensor of its patterns (0 .. 65535)."""
    assert t.dtype in (BF16, F16)
    return t.contiguous().view(torch.int16).to(torch.int32) & 0xFFFF


def bits32(t):
    assert t.dtype == F32
    return t.contiguous().view(torch.int32)


def all_patterns(dt, device="cpu"):
    return from_bits(np.arange(65536), dt, device)


def is_finite_bits(bits, dt):
    return (bits & _EXP[dt]) != _EXP[dt]


def is_subnormal_bits(bits, dt):
    """Non-zero magnitudes below the smallest normal."""
    mag = bits & 0x7FFF
    return (mag > 0) & (mag < _MINNORM[dt])


def s_f32(device="cpu"):
    """The finite values of S_bf16 and S_f16 as fp32, ascending, each once (+0 and -0 both kept)."""
    out = []
    for dt in (BF16, F16):
        b = torch.arange(65536, dtype=torch.int32)
        out.append(all_patterns(dt)[is_finite_bits(b, dt)].float())
    v = torch.cat(out)
    key = bits32(v).to(torch.int64)
    key = torch.where(key < 0, -(key & 0x7FFFFFFF) - 1, key)          # order of the values, -0 below +0
    key = torch.unique(key)                                            # sorted
    b = torch.where(key < 0, (-(key + 1)) | 0x80000000, key)
    b = torch.where(b >= 2 ** 31, b - 2 ** 32, b).to(torch.int32)
    return b.view(F32).to(device)


def s_tie(dt, device="cpu"):
    """(u fp32 [n], bits of rne_T(u) int32 [n]): for a = 0, 16, 32, ... (a + 1 finite) and both signs, mid(a, a + 1) - 1 fp32 ulp,
    the midpoint, + 1 fp32 ulp (ulps towards larger magnitude for '+').  a is even, so the three go to a, a, a + 1."""
    top = _EXP[dt] - 1                                                  # largest finite magnitude
    a = np.arange(0, top, 16)
    a = a[a + 1 <= top]
    lo, hi = from_bits(a, dt).float().double(), from_bits(a + 1, dt).float().double()
    mid = ((lo + hi) / 2).float()
    assert bool((mid.double() == (lo + hi) / 2).all())                  # exact in fp32
    inf = torch.full_like(mid, math.inf)
    below, above = torch.nextafter(mid, -inf), torch.nextafter(mid, inf)
    u = torch.stack([below, mid, above], 1).reshape(-1)
    want = torch.from_numpy(np.stack([a, a, a + 1], 1).reshape(-1).astype(np.int32))
    u = torch.cat([u, -u])
    want = torch.cat([want, want | 0x8000])
    return u.to(device), want.to(device)


# -------------------------------------------------------------------------------------------------------------------- layouts
def gemm_slots(nvals, N, K, pass_):
    """(k, n) of value j = 0 .. nvals - 1 in W[n, k] for pass 0 / 1."""
    cap = N * K
    assert nvals <= cap and N % 2 == 0
    s = torch.arange(nvals, dtype=torch.int64)
    return (s // N + pass_ * (K // 2)) % K, (s % N + pass_) % N


def gemm_operands(vals, M, N, K, pass_):
    """A [M, K] one-hot, W [N, K] of vals' dtype with the non-finite values replaced by 0, and the (k, n) slots."""
    k, n = gemm_slots(vals.numel(), N, K, pass_)
    k, n = k.to(vals.device), n.to(vals.device)
    W = torch.zeros(N, K, dtype=vals.dtype, device=vals.device)
    W[n, k] = torch.where(torch.isfinite(vals), vals, torch.zeros_like(vals))
    A = torch.zeros(M, K, dtype=vals.dtype, device=vals.device)
    m = torch.arange(M, device=vals.device)
    A[m, m % K] = 1
    return A, W, k, n


def bias_slots(nvals):
    """Two columns of different parity for value j of a bias-delivered set: j and off + j, off odd.  Returns (off, length)."""
    off = nvals | 1
    return off, off + nvals


def bias_vector(vals, N):
    """[N] vector of vals' dtype, zero but for value j at columns j and off + j (bias_slots).  Returns (vector, off)."""
    off, need = bias_slots(vals.numel())
    assert need <= N
    b = torch.zeros(N, dtype=vals.dtype, device=vals.device)
    b[:vals.numel()] = vals
    b[off:off + vals.numel()] = vals
    return b, off


def block_slots(nvals, pass_):
    """(block, column) of value j on the block-level paths: slices of HID values, the second pass one column on."""
    nblk = -(-(nvals + 1) // HID)
    s = (torch.arange(nvals, dtype=torch.int64) + pass_) % (nblk * HID)
    return s // HID, s % HID, nblk


def edge_slice(A0, P1, N1):
    """One 768-value slice of bf16 patterns that holds A0-1, A0, P1-1, P1, N1-1, N1 of both signs (path 5b), the rest spread over
    the finite range; every edge at an even and at an odd column."""
    edges = [A0 - 1, A0, P1 - 1, P1, N1 - 1, N1]
    e = [x | s for s in (0, 0x8000) for x in edges]
    seq = e + [0] + e                                  # second copy starts at an odd column (len(e) = 12, + 1)
    rest = np.linspace(0x0100, 0x7F7F, HID - len(seq)).astype(np.int64)
    rest[1::2] |= 0x8000
    return np.array(seq + list(rest), dtype=np.int64)


# ----------------------------------------------------------------------------------------------------------------- references
def gelu64(x):
    return 0.5 * x * torch.special.erfc(-x * SQRT1_2)


def dgelu64(x):
    return 0.5 * torch.special.erfc(-x * SQRT1_2) + x * torch.exp(-0.5 * x * x) / math.sqrt(2 * math.pi)


def _hw_q(u):
    return 0.5 * torch.special.erfc(u.abs() * SQRT1_2)


def e_gelu(u, ref):
    return 2.0 ** -22 * u.abs() + 2 * ulp(ref, F32) + u.abs() * _hw_q(u) * (HW_L + 1) * HW_REL


def e_dgelu(u, ref):
    phi = torch.exp(-0.5 * u * u) / math.sqrt(2 * math.pi)
    return 2.0 ** -21 + 2 * ulp(ref, F32) + _hw_q(u) * (HW_L + 1) * HW_REL + u.abs() * phi * HW_REL


def e_tanh(u, ref):
    return 2 * ulp(ref, F32)


KINDS = {"gelu": (gelu64, e_gelu), "dgelu": (dgelu64, e_dgelu), "tanh": (torch.tanh, e_tanh)}


def bound_ratio(kind, u, got, dt):
    """(|got - ref| / bound, ref) per element for finite u; u and got of any float dtype, dt the OUTPUT type."""
    f, e = KINDS[kind]
    u = u.double()
    ref = f(u)
    E = e(u, ref)
    bound = 0.5 * ulp(ref.abs() + E, dt) + E
    r = (got.double() - ref).abs() / bound
    return torch.where(torch.isnan(r), torch.full_like(r, math.inf), r), ref


def _show(u, got, ref, idx, n=6):
    return "; ".join(f"u={float(u[i]):.9g} got={float(got[i]):.9g} ref={float(ref[i]):.9g}" for i in idx[:n].tolist())


def assert_bound(where, kind, u, got, dt, sel=None):
    """Assertion 4 on the selected finite inputs.  Returns the worst ratio."""
    fin = torch.isfinite(u.double())
    sel = fin if sel is None else (sel & fin)
    r, ref = bound_ratio(kind, u, got, dt)
    r = torch.where(sel, r, torch.zeros_like(r))
    bad = (r > 1).nonzero().flatten()
    worst = float(r.max()) if r.numel() else 0.0
    assert bad.numel() == 0, (f"{where} {kind}: {bad.numel()} inputs beyond the fp64 bound, worst ratio {worst:.4g}: "
                              + _show(u.double(), got.double(), ref, bad))
    return worst


# ------------------------------------------------------------------------------------------------------ assertions on tables
def window_edges(A0, P1, N1):
    out = {}
    for s, sn in ((0, "+"), (0x8000, "-")):
        for nm, v in (("A0-1", A0 - 1), ("A0", A0), ("P1-1", P1 - 1), ("P1", P1), ("N1-1", N1 - 1), ("N1", N1)):
            out[sn + nm] = v | s
    return out


def assert_full_bits(where, g_bits, d_bits, full, win):
    """Assertion 1: for every finite bf16 input of bit magnitude >= 0x100, (gelu | gelu' << 16) equals full65536[u].
    g_bits, d_bits: int32 [65536] tables (index = bits of u); full: int64 / uint32 [65536]; win = (A0, P1, N1)."""
    full = torch.as_tensor(np.asarray(full).astype(np.int64), device=g_bits.device) if not torch.is_tensor(full) else full.to(g_bits.device)
    got = g_bits.to(torch.int64) | (d_bits.to(torch.int64) << 16)
    b = torch.arange(65536, device=g_bits.device, dtype=torch.int32)
    sel = is_finite_bits(b, BF16) & ((b & 0x7FFF) >= 0x100)
    diff = sel & (got != full)
    n = int(diff.sum())
    if n:
        edges = {k: v for k, v in window_edges(*win).items() if bool(diff[v])}
        idx = diff.nonzero().flatten()[:8].tolist()
        raise AssertionError(f"{where}: {n} inputs differ from full65536; window edges that differ: {sorted(edges) or 'none'}; first "
                             + ", ".join(f"u=0x{i:04X} got=0x{int(got[i]):08X} want=0x{int(full[i]):08X}" for i in idx))
    return n


def count_full_diffs(g_bits, d_bits, full):
    full = torch.as_tensor(np.asarray(full).astype(np.int64), device=g_bits.device) if not torch.is_tensor(full) else full.to(g_bits.device)
    got = g_bits.to(torch.int64) | (d_bits.to(torch.int64) << 16)
    b = torch.arange(65536, device=g_bits.device, dtype=torch.int32)
    sel = is_finite_bits(b, BF16) & ((b & 0x7FFF) >= 0x100)
    return (sel & (got != full)).nonzero().flatten()


def assert_below_window(where, g_bits, d_bits):
    """Assertion 2 (bf16, bit magnitude < 0x100, zeros included): gelu' = 0x3F00, gelu zero or of u's sign, |gelu| <= |u|."""
    b = torch.arange(65536, device=g_bits.device, dtype=torch.int32)
    sel = (b & 0x7FFF) < 0x100
    gm = g_bits & 0x7FFF
    bad = sel & ((d_bits != 0x3F00) | ((gm != 0) & ((g_bits & 0x8000) != (b & 0x8000))) | (gm > (b & 0x7FFF)))
    idx = bad.nonzero().flatten()
    assert idx.numel() == 0, (f"{where}: {idx.numel()} inputs below the window break (gelu' = 0.5, sign, |gelu| <= |u|): "
                              + ", ".join(f"u=0x{i:04X} gelu=0x{int(g_bits[i]):04X} gelu'=0x{int(d_bits[i]):04X}" for i in idx[:8].tolist()))


def nonfinite_summary(dt, g_bits, d_bits=None):
    """What a path gives for +inf, -inf and NaN inputs (the DESIGN record); assertion 3 is assert_nonfinite."""
    ex = _EXP[dt]
    qn = ex | ((ex & -ex) >> 1)                        # the quiet NaN without payload
    out = {}
    for nm, i in (("+inf", ex), ("-inf", 0x8000 | ex), ("+nan", qn), ("-nan", 0x8000 | qn)):
        out[nm] = f"0x{int(g_bits[i]):04X}" + (f"/0x{int(d_bits[i]):04X}" if d_bits is not None else "")
    return out


def assert_nonfinite(where, dt, g_bits):
    """Assertion 3: NaN -> gelu NaN (every NaN pattern, both signs), +inf -> +inf."""
    ex = _EXP[dt]
    b = torch.arange(65536, device=g_bits.device, dtype=torch.int32)
    nan_in = ((b & ex) == ex) & ((b & 0x7FFF) > ex)
    nan_out = ((g_bits & ex) == ex) & ((g_bits & 0x7FFF) > ex)
    bad = (nan_in & ~nan_out).nonzero().flatten()
    assert bad.numel() == 0, (f"{where}: {bad.numel()} NaN inputs give a gelu that is not NaN: "
                              + ", ".join(f"u=0x{i:04X} gelu=0x{int(g_bits[i]):04X}" for i in bad[:8].tolist()))
    assert int(g_bits[ex]) == ex, f"{where}: gelu(+inf) = 0x{int(g_bits[ex]):04X}"


def assert_gelu_properties(where, u, g, below=None, skip=None):
    """Assertion 5 for gelu on finite inputs given in ASCENDING order of u within each sign (any float dtype): sign(gelu) = sign(u)
    (where `below` is set: zero or u's sign), non-decreasing over ascending u >= 0, gelu(u) <= u for u > 0."""
    fin = torch.isfinite(u)
    if skip is not None:
        fin = fin & ~skip
    ud, gd = u.double(), g.double()
    su, sg = torch.signbit(u), torch.signbit(g)
    bad = fin & (su != sg)
    if below is not None:
        bad = bad & ~(below & (gd == 0))
    idx = bad.nonzero().flatten()
    assert idx.numel() == 0, f"{where}: sign(gelu) != sign(u) at {idx.numel()} inputs: " + _show(ud, gd, gd, idx)
    pos = (fin & ~su).nonzero().flatten()
    up, gp = ud[pos], gd[pos]
    assert bool((up[1:] >= up[:-1]).all()), "inputs not ascending"
    idx = (gp[1:] < gp[:-1]).nonzero().flatten()
    assert idx.numel() == 0, f"{where}: gelu decreases over ascending u >= 0 at {idx.numel()} inputs: " + _show(up[1:], gp[1:], gp[:-1], idx)
    idx = (gp > up).nonzero().flatten()
    assert idx.numel() == 0, f"{where}: gelu(u) > u at {idx.numel()} inputs: " + _show(up, gp, up, idx)


def assert_tanh_properties(where, u, h, neg_of, skip=None):
    """Assertion 5 for tanh: odd (h[neg_of] is the result for -u, bit-wise the sign flip), non-decreasing over ascending u >= 0,
    |tanh| <= 1; tanh(+-0) = +-0, tanh(+-big) = +-1 exactly (|u| >= 10: 1 - tanh(10) = 4e-9 is below half an fp32 ulp of 1),
    +-inf included.  NaN -> NaN."""
    ud, hd = u.double(), h.double()
    nan = torch.isnan(ud)
    assert bool(torch.isnan(hd[nan]).all()), f"{where}: tanh(NaN) is not NaN"
    ok = ~nan
    if skip is not None:
        ok = ok & ~skip & ~skip[neg_of]
    idx = (ok & ~((hd == -hd[neg_of]) & (torch.signbit(h) != torch.signbit(h[neg_of])))).nonzero().flatten()
    assert idx.numel() == 0, f"{where}: tanh not odd at {idx.numel()} inputs: " + _show(ud, hd, -hd[neg_of], idx)
    idx = (ok & (hd.abs() > 1)).nonzero().flatten()
    assert idx.numel() == 0, f"{where}: |tanh| > 1: " + _show(ud, hd, hd, idx)
    big = ok & (ud.abs() >= 10)
    idx = (big & (hd != torch.sign(ud))).nonzero().flatten()
    assert idx.numel() == 0, f"{where}: tanh(+-big) != +-1: " + _show(ud, hd, torch.sign(ud), idx)
    z = (ud == 0) & ok
    assert bool((hd[z] == 0).all()) and bool((torch.signbit(h[z]) == torch.signbit(u[z])).all()), f"{where}: tanh(+-0) != +-0"
    pos = (ok & ~torch.signbit(u)).nonzero().flatten()
    up, hp = ud[pos], hd[pos]
    assert bool((up[1:] >= up[:-1]).all()), "inputs not ascending"
    idx = (hp[1:] < hp[:-1]).nonzero().flatten()
    assert idx.numel() == 0, f"{where}: tanh decreases at {idx.numel()} inputs: " + _show(up[1:], hp[1:], hp[:-1], idx)


def assert_f16_finite(where, g_bits, d_bits=None):
    """Assertion 6: every finite fp16 input (up to 65504) gives finite results."""
    b = torch.arange(65536, device=g_bits.device, dtype=torch.int32)
    fin = is_finite_bits(b, F16)
    for nm, t in (("gelu", g_bits), ("gelu'", d_bits)):
        if t is None:
            continue
        bad = (fin & ~is_finite_bits(t, F16)).nonzero().flatten()
        assert bad.numel() == 0, f"{where}: {nm} not finite for finite inputs " + ", ".join(f"0x{i:04X}" for i in bad[:8].tolist())


def assert_ties(where, dt, want_bits, got, tab):
    """S_tie: the result for every fp32 u is the path's own result for rne_T(u).  got / tab: int32 bit tensors (tab indexed by bits)."""
    exp = tab[want_bits.long()]
    bad = (got != exp).nonzero().flatten()
    assert bad.numel() == 0, (f"{where}: {bad.numel()} of {got.numel()} tie inputs do not give the result of rne_{NAMES[dt]}(u): "
                              + ", ".join(f"#{i} (-> 0x{int(want_bits[i]):04X}) got=0x{int(got[i]):04X} want=0x{int(exp[i]):04X}"
                                          for i in bad[:8].tolist()))


def check_gelu_tables(where, dt, g_bits, d_bits, full=None, win=None, exact=True, nonfinite=True, neg_zero_lost=False):
    """Assertions 1 - 6 on one path's 16-bit tables.  Returns {output: worst bound ratio}.  neg_zero_lost: the delivery turned the
    input -0 into +0 (0 + -0 = +0 in a GEMM): the sign of that one result is not examined."""
    dev = g_bits.device
    b = torch.arange(65536, device=dev, dtype=torch.int32)
    u = all_patterns(dt, dev)
    g, d = from_bits(g_bits, dt, dev), from_bits(d_bits, dt, dev)
    fin = is_finite_bits(b, dt)
    below = ((b & 0x7FFF) < 0x100) if dt == BF16 else None
    if dt == BF16:
        if exact:
            assert_full_bits(where, g_bits, d_bits, full, win)
        assert_below_window(where, g_bits, d_bits)
    if nonfinite:
        assert_nonfinite(where, dt, g_bits)
    sel = fin if below is None else fin & ~below
    worst = {"gelu": assert_bound(where, "gelu", u, g, dt, sel), "gelu'": assert_bound(where, "dgelu", u, d, dt, sel)}
    # ascending order within each sign: positive patterns ascend with their bits; the negatives are not needed in order
    assert_gelu_properties(where, u, g, below, skip=(b == 0x8000) if neg_zero_lost else None)
    if dt == F16:
        assert_f16_finite(where, g_bits, d_bits)
    return worst


def check_tanh_table(where, dt, h_bits, neg_zero_lost=False):
    dev = h_bits.device
    u, h = all_patterns(dt, dev), from_bits(h_bits, dt, dev)
    neg_of = torch.arange(65536, device=dev) ^ 0x8000
    worst = assert_bound(where, "tanh", u, h, dt)
    assert_tanh_properties(where, u, h, neg_of, skip=(torch.arange(65536, device=dev) == 0x8000) if neg_zero_lost else None)
    return {"tanh": worst}


# ------------------------------------------------------------------------------------------- fp32 emulation of gelu_pair_fast
def _f(x):
    return np.asarray(x, dtype=np.float64).astype(np.float32)


def _fma(a, b, c):
    """fp32 fma through fp64: the product of two fp32 is exact there; the sum is rounded to fp64, then to fp32."""
    return _f(a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64))


def emu_gelu_pair(x):
    """common.h gelu_pair_fast on a float32 array with an exact reciprocal and exp2 (each rounded to fp32 once) and every
    `a * b + c` contracted, as -ffp-contract=fast compiles it.  Returns fp32 (gelu, gelu')."""
    with np.errstate(all="ignore"):
        x = _f(x)
        kz = np.float32(0.84932180028801904272)
        kp = np.float32(np.float32(np.float32(0.3275911) * np.float32(0.70710678118654752440)) / kz)
        z = _f(np.abs(x) * kz)
        d = _fma(z, np.full_like(z, kp), np.ones_like(z))
        t = _f(1.0 / d.astype(np.float64))
        w = _f(z * z)
        e = _f(np.exp2(-w.astype(np.float64)))
        h = np.float32(0.5)
        c = [np.float32(h * np.float32(a)) for a in AS_A]
        poly = _fma(t, np.full_like(t, c[4]), np.full_like(t, c[3]))
        for ci in (c[2], c[1], c[0]):
            poly = _fma(poly, t, np.full_like(t, ci))
        q = _f(_f(poly * t) * e)
        cdf = np.where(x >= 0, _f(np.float32(1.0) - q), q)
        px = _f(_f(e * np.float32(0.39894228040143267794)) * x)
        return _f(x * cdf), _f(cdf + px)


def emu_tables(dt, g32, d32):
    """fp32 results for all 65 536 patterns of dt -> int32 bit tables after the rounding to dt."""
    return to_bits(torch.from_numpy(g32).to(dt)), to_bits(torch.from_numpy(d32).to(dt))


def emu_full():
    """The emulation's full65536 (gelu | gelu' << 16 per bf16 input), as mlp_fused.hip gelu_full_kernel builds the device's."""
    u = all_patterns(BF16).float().numpy()
    g, d = emu_tables(BF16, *emu_gelu_pair(u))
    return (g.to(torch.int64) | (d.to(torch.int64) << 16)).numpy()


# --------------------------------------------------------------------- Python restatement of the table's window, image and keys
def scan_window(full):
    """mlp_fused.hip gelu_scan_kernel: (A0, P1, N1, gpn)."""
    full = np.asarray(full).astype(np.int64)
    gpn = int(full[0xFF7F] >> 16)
    a = np.arange(0x8000)
    ep, en = full[a], full[0x8000 | a]
    t_ok = (a < 0x80) | ((ep == ((a - 0x80) | (0x3F00 << 16))) & (en == ((0x8000 | (a - 0x80)) | (0x3F00 << 16))))
    p_ok = ep == (a | (0x3F80 << 16))
    n_ok = en == (0x8000 | (gpn << 16))
    rows = lambda m: m.reshape(256, 128).all(1)          # noqa: E731
    t_ok, p_ok, n_ok = rows(t_ok), rows(p_ok), rows(n_ok)
    e0 = 2
    while e0 < 255 and t_ok[e0]:
        e0 += 1
    ep_, en_ = 255, 255
    while ep_ > e0 and p_ok[ep_ - 1]:
        ep_ -= 1
    while en_ > e0 and n_ok[en_ - 1]:
        en_ -= 1
    return e0 * 128, ep_ * 128, en_ * 128, gpn


def build_image(full, A0, P1, N1, gpn):
    full = np.asarray(full).astype(np.int64)
    NP, NN = P1 - A0, N1 - A0
    img = np.zeros(NP + 2 + NN + 2, dtype=np.int64)
    img[0] = img[NP + 2] = 0x80 | (0x3F00 << 16)
    a = np.arange(A0, P1)
    f = full[a]
    img[1:NP + 1] = (a - (f & 0x7FFF)) | (f & 0xFFFF0000)
    img[NP + 1] = 0x3F80 << 16
    a = np.arange(A0, N1)
    f = full[0x8000 | a]
    img[NP + 3:NP + 3 + NN] = (a - (f & 0x7FFF)) | (f & 0xFFFF0000)
    img[NP + 3 + NN] = N1 | (gpn << 16)
    return img


def table_lookup(pb, img, A0, P1, N1, *, dklo=0, dkpos=0, dkneg=0, drop_sign_beyond_n1=False, nan_fix=True):
    """gelu_table.h gelu_table_pairs4's key arithmetic per 16-bit element (all operations modulo 2^16).  pb: int array of bf16
    patterns.  dklo / dkpos / dkneg shift ONE clamp constant of gelu_table_keys (the seeded off-by-one defects at A0, P1, N1); a
    key that leaves the image reads JUNK, as LDS past the image would give.  nan_fix=False: the lookup as it was before the sweep
    found that it turned NaNs with the sign bit set into -0."""
    JUNK = 0x7FC57FC5
    pb = np.asarray(pb).astype(np.int64) & 0xFFFF
    kneg, kpos, klo = (0x8000 | (N1 + dkneg)), P1 + dkpos, A0 - 1 + dklo
    koff = (0x10000 - 4 * (A0 - 1)) & 0xFFFF
    ksgn = (4 * (P1 - A0 + 2)) & 0xFFFF
    s16 = lambda v: np.where(v >= 0x8000, v - 0x10000, v)          # noqa: E731
    p1 = np.minimum(pb, kneg)                                        # v_pk_min_u16
    p2 = np.where(s16(p1) < s16(np.int64(kpos)), p1, kpos)           # v_pk_min_i16
    p1, p2 = p1 & 0x7FFF, p2 & 0x7FFF
    agv = np.maximum(p1, 0x80)
    if nan_fix:
        agv = (agv - np.maximum(pb - 0xFF80, 0)) & 0xFFFF             # v_pk_sub_u16 clamp, v_pk_sub_u16: a negative NaN stays a NaN
    ak = np.maximum(p2, klo)
    i4 = (ak * 4 + koff) & 0xFFFF
    sg = pb >> 15
    i4 = (i4 + sg * ksgn) & 0xFFFF
    assert (i4 % 4 == 0).all()
    idx = i4 // 4
    e = np.where(idx < len(img), np.asarray(img)[np.minimum(idx, len(img) - 1)], JUNK)
    gm = (agv - (e & 0xFFFF)) & 0xFFFF
    sign = pb & 0x8000
    if drop_sign_beyond_n1:
        sign = np.where((pb & 0x7FFF) >= N1, 0, sign)
    return sign | gm, e >> 16
