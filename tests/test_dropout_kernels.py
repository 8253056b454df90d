"""The dropout kernels (rgbnm.h, dropout mask contract) against the numpy restatement of tests/dropout_ref.py:
rgbnm_dropout_apply bit for bit (also past its grid cap: composite_ref.APPLY_BIG), rgbnm_gemm_nt_drop's RES / GELU epilogues
element-wise (tests/kernel_check.py bounds, guarded outputs) in the staged and the direct form, p = 0 against rgbnm_gemm_nt
bit for bit, and the statistics of the masks."""
import math

import numpy as np
import pytest
import torch

import composite_ref as CR
import dropout_ref as D
from kernel_check import U, guarded, nan_padded, check_bound, launched, ran, ulp
from rgb_no_more_amd import lib as L
from test_hip_kernels import option  # noqa: F401  (fixture: set a runtime switch for one test)
from test_kernel_edges import rnd, gelu64, dgelu64, u32

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
DTS3 = [F32, BF16, F16]
NAMES = {F32: "f32", BF16: "bf16", F16: "f16"}
SEEDS = [0, 0x0123456789ABCDEF, 2 ** 64 - 1, 987654321]


def seed_tensor(seed):
    s = int(seed) & (2 ** 64 - 1)
    return torch.tensor([s - 2 ** 64 if s >= 2 ** 63 else s], dtype=torch.int64, device=DEV)


def factor_t(seed, p, site, block, M, N):
    return torch.from_numpy(D.factor(seed, p, site, block, M, N)).to(DEV)


def apply(dt, st, p, site, block, x, ldx, y, ldy, M, N):
    L.check(L.lib().rgbnm_dropout_apply(L.dt_of(dt), st.data_ptr(), p, site, block, x.data_ptr(), ldx, y.data_ptr(), ldy, M, N,
                                        L.stream()), "dropout_apply")


@pytest.mark.parametrize("dt", DTS3, ids=lambda d: NAMES[d])
def test_apply_on_ones_is_keep_times_scale_bit_for_bit(dt):
    cases = [(1, 1, 0), (37, 13, 0), (300, 200, 8), (512, 192, 0), (129, 768, 16), (7, 4096, 0)]
    for i, (M, N, pad) in enumerate(cases):
        seed, site, block, p = SEEDS[i % 4], i % 3, 5 * i, (0.1, 0.5, 0.25)[i % 3]
        st = seed_tensor(seed)
        ld = N + pad
        x = nan_padded(torch.ones(M, N, device=DEV, dtype=dt), ld, 2)
        y = guarded(M, N, dt, ld)
        apply(dt, st, p, site, block, x, ld, y.t, ld, M, N)
        torch.cuda.synchronize()
        y.check(f"apply {NAMES[dt]} M={M} N={N}")
        ref = factor_t(seed, p, site, block, M, N).to(dt)
        assert torch.equal(y.t, ref), (M, N, site, block)
        # in place, on data: y = T(x * scale) or 0
        z = rnd((M, N), 40 + i, 1.0, dt)
        want = torch.where(ref != 0, (z.float() * float(D.threshold(p)[1])).to(dt), torch.zeros_like(z))
        apply(dt, st, p, site, block, z, N, z, N, M, N)
        assert torch.equal(z, want)


@pytest.mark.parametrize("dtn,M,N", CR.APPLY_BIG)
def test_apply_past_the_grid_cap_is_keep_times_scale_bit_for_bit(dtn, M, N):
    """launch_apply caps the grid at 8192 workgroups of 256 eight-column groups; JPEG-S's own [50176, 384] gradient is past it.
    These shapes turn dropout_apply_kernel's grid-stride loop twice, the second turn ragged, on the 16-byte path (16-bit and fp32)
    and on the element path (N % 8 != 0); tests/test_composite_edges_cpu.py asserts those regimes from launch_apply's arithmetic."""
    dt = CR.DT[dtn]
    i = [c[0] for c in CR.APPLY_BIG].index(dtn)
    seed, site, block, p = SEEDS[(i + 1) % 4], (2, 0, 1)[i], (0, 11, 5)[i], (0.1, 0.5, 0.25)[i]
    st = seed_tensor(seed)
    x = nan_padded(torch.ones(M, N, device=DEV, dtype=dt), N, 2)
    y = guarded(M, N, dt)
    _, names = launched(lambda: apply(dt, st, p, site, block, x, N, y.t, N, M, N))
    assert len(names) == 1 and "dropout_apply_kernel" in names[0], names
    y.check(f"apply {dtn} M={M} N={N}")
    ref = factor_t(seed, p, site, block, M, N).to(dt)
    assert torch.equal(y.t, ref), (M, N, site, block)
    del y, ref
    # on data, in place: y = T(x * scale) or 0
    z = rnd((M, N), 60 + i, 1.0, dt)
    want = CR.masked_copy(z, factor_t(seed, p, site, block, M, N), p)
    apply(dt, st, p, site, block, z, N, z, N, M, N)
    assert torch.equal(z, want)


def nt_drop_case(dt, epi, M, N, K, seed, p, site, block, *, c_f32=False, pad=False):
    """One rgbnm_gemm_nt_drop call, element-wise against the fp64 reference with the numpy masks (test_kernel_edges.nt_case's
    terms; the mask multiplies the T-rounded staged value and adds one fp32 rounding of the product)."""
    lda, ldw, ldc, ldr, ldc2 = (K + 16, K + 24, N + 8, N + 16, N + 24) if pad else (K, K, N, N, N)
    A = nan_padded(rnd((M, K), seed % 1000, 1.0, dt), lda, 3)
    W = nan_padded(rnd((N, K), seed % 1000 + 1, 0.1, dt), ldw, 3)
    bias = rnd((N,), seed % 1000 + 2, 0.5)
    R = nan_padded(rnd((M, N), seed % 1000 + 3, 1.0, dt), ldr, 3) if epi == L.EPI_RES_DROP else None
    odt = F32 if c_f32 else dt
    C = guarded(M, N, odt, ldc)
    C2 = guarded(M, N, dt, ldc2) if epi == L.EPI_GELU_DROP else None
    st = seed_tensor(seed)

    def call():
        L.check(L.lib().rgbnm_gemm_nt_drop(L.dt_of(dt), epi, A.data_ptr(), lda, W.data_ptr(), ldw, C.t.data_ptr(), ldc,
                                           bias.data_ptr(), L.ptr(R), ldr, C2.t.data_ptr() if C2 else None, ldc2, None, 0, M, N, K,
                                           int(c_f32), st.data_ptr(), p, site, block, L.stream()), "gemm_nt_drop")
    _, names = launched(call)
    where = f"gemm_nt_drop {NAMES[dt]} epi={epi} M={M} N={N} K={K} c_f32={int(c_f32)} p={p}"
    assert ran(names, "gemm_nt_kernel"), (where, sorted(set(names)))
    C.check(where)
    if C2:
        C2.check(where + " C2")
    f = factor_t(seed, p, site, block, M, N).double()
    A64, W64 = A.double(), W.double()
    pre = A64 @ W64.T + bias.double()
    mag = A64.abs() @ W64.abs().T + bias.double().abs()
    inter = ulp(pre, dt) if (dt != F32 and not c_f32) else 0.0     # staged epilogues round acc + bias to T first
    tile = (128, 192 if N % 192 == 0 else 128)
    if epi == L.EPI_RES_DROP:
        r = R.double()
        ref = r + f * pre
        return check_bound(C.t, ref, f * mag + r.abs(), odt, 1, K * U, where, extra=f * inter + u32(f * pre), tile=tile)
    ref, ref2 = f * gelu64(pre), f * dgelu64(pre)
    check_bound(C2.t, ref2, 0.8 * f * mag, dt, 1, K * U, where + " C2", extra=f * (0.8 * inter + 2.0 ** -21) + 2 * u32(ref2),
                tile=tile)
    return check_bound(C.t, ref, 1.13 * f * mag, odt, 1, K * U, where,
                       extra=f * (1.13 * inter + 2.0 ** -22 * pre.abs()) + 2 * u32(ref), tile=tile)


@pytest.mark.parametrize("staged", [0, 1])
@pytest.mark.parametrize("dt", DTS3, ids=lambda d: NAMES[d])
def test_gemm_nt_drop_epilogues_elementwise(option, dt, staged):
    option("nt_staged", staged)
    shapes = [(128, 192, 64), (300, 192, 192), (257, 384, 72), (129, 256, 128), (64, 40, 64), (1568, 768, 192)]
    for i, (M, N, K) in enumerate(shapes):
        for epi in (L.EPI_RES_DROP, L.EPI_GELU_DROP):
            nt_drop_case(dt, epi, M, N, K, SEEDS[i % 4] + epi, (0.1, 0.5)[i % 2], i % 3, i, pad=bool(i % 2))
    nt_drop_case(dt, L.EPI_RES_DROP, 200, 192, 64, 5, 0.1, 2, 11, c_f32=True)


@pytest.mark.parametrize("staged", [0, 1])
@pytest.mark.parametrize("dt", DTS3, ids=lambda d: NAMES[d])
def test_drop_epilogues_at_p0_give_the_bits_of_gemm_nt(option, dt, staged):
    option("nt_staged", staged)
    option("nt_kpipe", 0)        # rgbnm_gemm_nt on the generic kernel too (the drop entry never leaves it)
    option("nt_wres", 0)
    option("nt_small", 0)
    st = seed_tensor(SEEDS[1])
    for M, N, K in [(300, 192, 192), (129, 256, 64), (64, 40, 64)]:
        A, W = rnd((M, K), 1, 1.0, dt), rnd((N, K), 2, 0.1, dt)
        bias, R = rnd((N,), 3, 0.5), rnd((M, N), 4, 1.0, dt)
        for epi, base in ((L.EPI_RES_DROP, L.EPI_RES), (L.EPI_GELU_DROP, L.EPI_GELU)):
            outs = []
            for fn, e, extra in ((L.lib().rgbnm_gemm_nt, base, ()), (L.lib().rgbnm_gemm_nt_drop, epi, (st.data_ptr(), 0.0, 1, 2))):
                Cc, C2 = torch.empty(M, N, device=DEV, dtype=dt), torch.empty(M, N, device=DEV, dtype=dt)
                r = R if e in (L.EPI_RES, L.EPI_RES_DROP) else None
                c2 = C2 if e in (L.EPI_GELU, L.EPI_GELU_DROP) else None
                L.check(fn(L.dt_of(dt), e, A.data_ptr(), K, W.data_ptr(), K, Cc.data_ptr(), N, bias.data_ptr(), L.ptr(r), N,
                           L.ptr(c2), N, None, 0, M, N, K, 0, *extra, L.stream()))
                outs.append((Cc, c2))
            assert torch.equal(outs[0][0], outs[1][0]), (NAMES[dt], epi, M, N, K)
            if outs[0][1] is not None:
                assert torch.equal(outs[0][1], outs[1][1]), (NAMES[dt], epi, M, N, K)


def test_gemm_nt_drop_refuses_bad_arguments():
    st = seed_tensor(1)
    x = torch.zeros(64, 64, device=DEV, dtype=BF16)
    args = lambda epi, p, site: (L.DT_BF16, epi, x.data_ptr(), 64, x.data_ptr(), 64, x.data_ptr(), 64, None, x.data_ptr(), 64,  # noqa: E731
                                 x.data_ptr(), 64, None, 0, 64, 64, 64, 0, st.data_ptr(), p, site, 0, L.stream())
    assert L.lib().rgbnm_gemm_nt_drop(*args(L.EPI_RES, 0.1, 0)) != 0          # only the two dropout epilogues
    assert L.lib().rgbnm_gemm_nt_drop(*args(L.EPI_RES_DROP, 1.0, 0)) != 0     # p in [0, 1)
    assert L.lib().rgbnm_gemm_nt_drop(*args(L.EPI_RES_DROP, 0.1, 4)) != 0     # site 0 .. 3
    assert L.lib().rgbnm_gemm_nt(L.DT_BF16, L.EPI_RES_DROP, x.data_ptr(), 64, x.data_ptr(), 64, x.data_ptr(), 64, None,
                                 x.data_ptr(), 64, x.data_ptr(), 64, None, 0, 64, 64, 64, 0, L.stream()) != 0


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_keep_rates_are_binomial(p):
    M, N = 8192, 4096                                     # 3.4e7 elements
    st = seed_tensor(SEEDS[3])
    x = torch.ones(M, N, device=DEV, dtype=BF16)
    apply(BF16, st, p, 1, 7, x, N, x, N, M, N)
    k = (x != 0).double()
    q = 1.0 - p
    tot = k.mean().item()
    assert abs(tot - q) <= 6 * math.sqrt(p * q / (M * N)), tot
    rows, cols = k.mean(1), k.mean(0)
    assert (rows - q).abs().max().item() <= 6 * math.sqrt(p * q / N)
    assert (cols - q).abs().max().item() <= 6 * math.sqrt(p * q / M)
    # every column residue mod 4 (the counter word) and row parity keep at the same rate
    for w in range(4):
        assert abs(k[:, w::4].mean().item() - q) <= 6 * math.sqrt(p * q / (M * N / 4))


def test_sites_blocks_and_seeds_draw_different_masks():
    M, N = 256, 384
    outs = {}
    for key in [(SEEDS[1], 0, 0), (SEEDS[1], 1, 0), (SEEDS[1], 2, 0), (SEEDS[1], 0, 1), (SEEDS[1], 0, 11), (SEEDS[2], 0, 0),
                (SEEDS[1] ^ 1, 0, 0), (SEEDS[1] ^ (1 << 40), 0, 0)]:
        x = torch.ones(M, N, device=DEV, dtype=F32)
        apply(F32, seed_tensor(key[0]), 0.5, key[1], key[2], x, N, x, N, M, N)
        outs[key] = x != 0
        assert torch.equal(outs[key].cpu(), torch.from_numpy(D.keep(key[0], 0.5, key[1], key[2], M, N)))
    keys = list(outs)
    for i in range(len(keys)):
        for j in range(i + 1, len(keys)):
            agree = (outs[keys[i]] == outs[keys[j]]).double().mean().item()
            assert abs(agree - 0.5) < 0.02, (keys[i], keys[j], agree)     # independent masks agree half the time
