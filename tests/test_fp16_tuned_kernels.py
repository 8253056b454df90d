"""fp16 on the tuned GEMM kernels (option f16_tuned = 1): gemm_nt_small, gemm_nt_wres, gemm_nt_kpipe (kp7, kp8, persistent) and
gemm_tn_pipe (pipelined, wide, grouped), element-wise at their tile edges with the cases, guards and fp64 bounds of
tests/test_kernel_edges.py (nt_case / tn_case: ulp_T(ref) + K u mag plus the named epilogue terms; nothing fitted here).  Every
tuned case also asserts, through the profiler, that the named kernel ran in its fp16 instantiation and the generic kernel did not;
with the option off (the default) the same shapes must stay on the generic kernels.

Largest |got - ref| / bound per family measured on one MI355X (pytest -s prints them): small-M 0.50, weight-resident 0.59 (GELU;
0.49 the others), row-panel kp7 0.57 with and without the persistent kernel, kp8 0.57, weight gradient 0.025 pipelined / 0.0013
wide / 0.0004 grouped / 0.0023 three jobs in one launch without a token split (fp32 outputs against a bound that grows with the token count)."""
import pytest
import torch

import kernel_check as KC
import test_kernel_edges as TE
from test_kernel_edges import (nt_case, tn_case, nt_generic_opts, tn_operands, tn_outputs, tn_check, F16, BF16, F32, E_NONE, E_RES,
                               E_GELU, E_DGELU, E_TANH, E_DTANH, EPI_NAMES)
from kernel_check import guarded, ran
from rgb_no_more_amd import lib as L
from test_hip_kernels import option  # noqa: F401  (fixture: set a runtime switch for one test)

pytestmark = pytest.mark.gpu

# how the profiler spells the element type of a kernel instantiation (demangled, or the mangled name where it is not)
F16_MARKS = ("_Float16", "DF16_", "__half")
BF16_MARKS = ("__bf16", "DF16b", "bfloat16")
PLAIN4 = (E_NONE, E_RES, E_GELU, E_DGELU)


def is_f16(name):
    return any(m in name for m in F16_MARKS) and not any(m in name for m in BF16_MARKS)


@pytest.fixture
def launches(monkeypatch):
    """Records the kernel names of every launch nt_case / tn_case profile (they keep them to themselves)."""
    log = []
    real = KC.launched

    def rec(fn):
        res, names = real(fn)
        log.append(names)
        return res, names
    monkeypatch.setattr(TE, "launched", rec)
    return log


def assert_f16(log, *subs):
    """The last profiled call ran a kernel whose name holds every one of subs, and every such kernel in its fp16 instantiation."""
    hits = [n for n in log[-1] if all(s in n for s in subs)]
    assert hits, (subs, sorted(set(log[-1])))
    assert all(is_f16(n) for n in hits), hits


def tuned(option):
    nt_generic_opts(option, 1)
    option("f16_tuned", 1)


def test_small_m_fp16(option, launches):
    tuned(option)
    option("nt_small", 1)
    worst = KC.Worst()
    shapes = [(m, 1000, 72) for m in (1, 31, 32, 33, 511, 512)] + [(33, 4, 8), (77, 36, 1000), (32, 1000, 192)]
    for i, (M, N, K) in enumerate(shapes):
        for epi in (E_NONE, E_TANH, E_DTANH):
            for c_f32 in (False, True):
                nt_case(F16, epi, M, N, K, c_f32=c_f32, inter=True, seed=30 * i + epi, want=("gemm_nt_small_kernel",),
                        forbid=("gemm_nt_kernel",), worst=worst, key=f"{EPI_NAMES[epi]}-c_f32={int(c_f32)}")
                assert_f16(launches, "gemm_nt_small_kernel")
    for epi in (E_NONE, E_TANH, E_DTANH):
        nt_case(F16, epi, 33, 1000, 72, pad=True, inter=True, seed=900 + epi, want=("gemm_nt_small_kernel",),
                forbid=("gemm_nt_kernel",), worst=worst, key=EPI_NAMES[epi] + "-pad")
        assert_f16(launches, "gemm_nt_small_kernel")
    nt_case(F16, E_RES, 33, 192, 72, inter=True, seed=950, want=("gemm_nt_kernel",), forbid=("gemm_nt_small_kernel",))
    nt_case(F16, E_NONE, 513, 192, 72, inter=True, seed=951, want=("gemm_nt_kernel",), forbid=("gemm_nt_small_kernel",))
    worst.report("fp16 tuned: gemm_nt small-M")


def test_weight_resident_fp16(option, launches):
    tuned(option)
    option("nt_wres", 1)
    worst = KC.Worst()
    cases = [(4096, 576), (4128, 576), (4096, 192), (4096, 768), (6432, 192)]
    for i, (M, N) in enumerate(cases):
        for epi in PLAIN4:
            nt_case(F16, epi, M, N, 192, inter=True, seed=40 * i + epi, want=("gemm_nt_wres_kernel",),
                    forbid=("gemm_nt_kernel",), worst=worst, key=EPI_NAMES[epi])
            assert_f16(launches, "gemm_nt_wres_kernel")
    for epi in PLAIN4:
        nt_case(F16, epi, 4128, 576, 192, pad=True, inter=True, seed=990 + epi, want=("gemm_nt_wres_kernel",),
                forbid=("gemm_nt_kernel",), worst=worst, key=EPI_NAMES[epi] + "-pad")
        assert_f16(launches, "gemm_nt_wres_kernel")
    for M, N in [(4064, 576), (4100, 576), (4096, 6336)]:
        nt_case(F16, E_RES, M, N, 192, inter=True, seed=M + N, want=("gemm_nt_kernel",), forbid=("gemm_nt_wres_kernel",))
    worst.report("fp16 tuned: gemm_nt weight-resident")


@pytest.mark.parametrize("persist", [0, 1])
def test_row_panel_kp7_fp16(option, launches, persist):
    tuned(option)
    option("nt_kpipe", 1)
    option("kp_persist", persist)
    option("kp8", 0)
    worst = KC.Worst()
    k37 = 224 * 37                                           # 8288
    cases = [(k37 + r, 384, 256) for r in (0, 1, 17, 223)]
    cases += [(8305, 192, 320), (8305, 1152, 320), (8289, 192, 768)]
    for i, (M, N, K) in enumerate(cases):
        kern = "gemm_nt_kpipe_persist_kernel" if (persist and N > 192) else "gemm_nt_kpipe_kernel"
        for epi in PLAIN4:
            nt_case(F16, epi, M, N, K, inter=True, seed=50 * i + epi, want=(("kp7", kern),), forbid=("gemm_nt_kernel",),
                    worst=worst, key=EPI_NAMES[epi])
            assert_f16(launches, "kp7", kern)
    for epi in PLAIN4:
        nt_case(F16, epi, k37 + 223, 384, 256, pad=True, inter=True, seed=1100 + epi, want=("kp7",), forbid=("gemm_nt_kernel",),
                worst=worst, key=EPI_NAMES[epi] + "-pad")
        assert_f16(launches, "kp7", "gemm_nt_kpipe")
    nt_case(F16, E_RES, 8191, 384, 256, inter=True, seed=1200, want=("gemm_nt_kernel",), forbid=("gemm_nt_kpipe",))
    worst.report(f"fp16 tuned: gemm_nt row-panel kp7 persist={persist}")


def test_row_panel_kp8_fp16(option, launches):
    tuned(option)
    option("nt_kpipe", 1)
    option("kp8", 1)
    worst = KC.Worst()
    for epi in PLAIN4:
        nt_case(F16, epi, 16384, 768, 256, inter=True, seed=60 + epi, want=(("kp8", "gemm_nt_kpipe"),),
                forbid=("gemm_nt_kernel", "kp7"), worst=worst, key=EPI_NAMES[epi])
        assert_f16(launches, "kp8", "gemm_nt_kpipe")
    worst.report("fp16 tuned: gemm_nt row-panel kp8")


@pytest.mark.parametrize("wide", [0, 1])
def test_weight_gradient_fp16(option, launches, wide):
    option("f16_tuned", 1)
    option("tn_pipe", 1)
    option("tn_wide", wide)
    worst = KC.Worst()
    if wide:
        cases = [(3136, 1152, 384, 6), (576, 3072, 768, 0), (3136, 384, 1536, 0)]
        kern = "gemm_tn_wide_kernel"
    else:
        cases = [(64, 192, 192, 0), (448, 200, 384, 0), (3136, 576, 192, 3), (6400, 1152, 384, 6)]
        kern = "gemm_tn_pipe_kernel"
    for i, (M, No, Ki, heads) in enumerate(cases):
        for acc, with_db in ((0, True), (1, True), (0, False), (1, False)):
            tn_case(F16, M, No, Ki, heads, acc, with_db, pad=(i % 2 == 1), seed=30 * i + acc, want=(kern,),
                    forbid=("gemm_tn_kernel",), worst=worst, key=kern)
            assert_f16(launches, kern)
    tn_case(F16, 449, 192, 384, seed=999, want=("gemm_tn_kernel",), forbid=("gemm_tn_pipe_kernel", "gemm_tn_wide_kernel"),
            worst=worst, key="fallback")
    worst.report(f"fp16 tuned: gemm_tn pipelined wide={wide}")


def test_group_bracket_flushes_between_bf16_and_fp16(option):
    """One bracket, a bf16 job and then an fp16 job with the same row count: the fp16 job must not join the bf16 launch."""
    option("f16_tuned", 1)
    option("tn_pipe", 1)
    lib = L.lib()
    M, No, Ki = 1024, 384, 192
    state = []
    for i, dt in enumerate((BF16, F16)):
        dY, X, ldy, ldx = tn_operands(dt, M, No, Ki, 300 + 10 * i, pad=(i == 1))
        dW, db = tn_outputs(No, Ki, 0, True, 300 + 10 * i)
        wsb = lib.rgbnm_gemm_tn_workspace_splits(No, Ki, max(1, 256 // (-(-No // 128) * (Ki // 192))))
        ws = guarded(wsb // 4, None, F32)
        state.append((dt, dY, X, ldy, ldx, dW, db, ws, wsb))

    def bracket():
        lib.rgbnm_gemm_tn_group_begin_n(4)
        for (dt, dY, X, ldy, ldx, dW, db, ws, wsb) in state:
            L.check(lib.rgbnm_gemm_tn(L.dt_of(dt), dY.data_ptr(), ldy, X.data_ptr(), ldx, dW.t.data_ptr(), db.t.data_ptr(), M, No,
                                      Ki, 0, 0, ws.t.data_ptr(), wsb, L.stream()))
        L.check(lib.rgbnm_gemm_tn_group_end(L.stream()))
    _, names = KC.launched(bracket)
    grouped = [n for n in names if "gemm_tn_pipe_kernel" in n or "gemm_tn_wide_kernel" in n]
    assert len(grouped) == 2, (grouped, sorted(set(names)))
    assert sum(is_f16(n) for n in grouped) == 1, grouped
    assert not ran(names, "gemm_tn_kernel"), sorted(set(names))
    worst = KC.Worst()
    for (dt, dY, X, ldy, ldx, dW, db, ws, wsb) in state:
        where = f"group job {TE.NAMES[dt]}: M={M} No={No} Ki={Ki}"
        ws.check(where + " workspace", written=False)
        tn_check(dY, X, dW, db, 0, 0, None, where, worst, "group-" + TE.NAMES[dt])
    worst.report("fp16 tuned: gemm_tn group bracket bf16 + fp16")


@pytest.mark.parametrize("direct", [1, 0])
def test_group_bracket_three_fp16_jobs_in_one_launch_without_a_token_split(option, direct):
    """Three fp16 jobs of one row count in ONE grouped launch whose tiles (96 + 96 + 5 of 128 x 192) leave no token split
    (S = 256 / 197 = 1): with tn_direct the kernel writes dW / db itself, the qkv row permutation included; without it the partial
    sums go through the reduction.  A job that accumulates keeps the whole launch on the reduction path (its last case)."""
    option("f16_tuned", 1)
    option("tn_pipe", 1)
    option("tn_wide", 0)
    option("tn_direct", direct)
    lib = L.lib()
    M = 1024
    for accs in ((0, 0, 0), (0, 1, 0)):
        jobs = [(1536, 1536, 0, accs[0], True), (1536, 1536, 0, accs[1], False), (576, 192, 3, accs[2], True)]
        state = []
        for i, (No, Ki, heads, acc, with_db) in enumerate(jobs):
            dY, X, ldy, ldx = tn_operands(F16, M, No, Ki, 400 + 10 * i, pad=(i == 1))
            dW, db = tn_outputs(No, Ki, acc, with_db, 400 + 10 * i)
            init = (dW.t.double().clone(), db.t.double().clone() if db else None) if acc else None
            wsb = lib.rgbnm_gemm_tn_workspace_splits(No, Ki, max(1, 256 // (-(-No // 128) * (Ki // 192))))
            ws = guarded(wsb // 4, None, F32)
            state.append((dY, X, ldy, ldx, dW, db, init, ws, wsb, No, Ki, heads, acc))

        def bracket():
            lib.rgbnm_gemm_tn_group_begin_n(4)
            for (dY, X, ldy, ldx, dW, db, init, ws, wsb, No, Ki, heads, acc) in state:
                L.check(lib.rgbnm_gemm_tn(L.dt_of(F16), dY.data_ptr(), ldy, X.data_ptr(), ldx, dW.t.data_ptr(),
                                          db.t.data_ptr() if db else None, M, No, Ki, heads, acc, ws.t.data_ptr(), wsb, L.stream()))
            L.check(lib.rgbnm_gemm_tn_group_end(L.stream()))
        _, names = KC.launched(bracket)
        grouped = [n for n in names if "gemm_tn_pipe_kernel" in n or "gemm_tn_wide_kernel" in n]
        assert len(grouped) == 1 and is_f16(grouped[0]), (grouped, sorted(set(names)))
        assert not ran(names, "gemm_tn_kernel"), sorted(set(names))
        wrote_itself = bool(direct) and not any(accs)
        assert ran(names, "reduce_") != wrote_itself, (direct, accs, sorted(set(names)))
        worst = KC.Worst()
        for i, (dY, X, ldy, ldx, dW, db, init, ws, wsb, No, Ki, heads, acc) in enumerate(state):
            where = f"group job {i} tn_direct={direct}: M={M} No={No} Ki={Ki} heads={heads} acc={acc}"
            ws.check(where + " workspace", written=False)
            tn_check(dY, X, dW, db, heads, acc, init, where, worst, f"job{i}")
        worst.report(f"fp16 tuned: gemm_tn group of three, no token split, tn_direct={direct} acc={accs}")


def test_option_off_keeps_fp16_on_the_generic_kernels(launches):
    """The default: one shape of each family in fp16 launches gemm_nt_kernel / gemm_tn_kernel and nothing else of the GEMM files."""
    assert L.get_option("f16_tuned") == 0
    tuned_nt = ("gemm_nt_small_kernel", "gemm_nt_wres_kernel", "gemm_nt_kpipe")
    for (epi, M, N, K) in [(E_TANH, 33, 1000, 72), (E_GELU, 4096, 576, 192), (E_RES, 8305, 384, 256), (E_DGELU, 16384, 768, 256)]:
        nt_case(F16, epi, M, N, K, inter=True, seed=M + epi, want=("gemm_nt_kernel",), forbid=tuned_nt)
        assert_f16(launches, "gemm_nt_kernel")
    for (M, No, Ki, heads) in [(3136, 576, 192, 3), (3136, 1152, 384, 6)]:
        tn_case(F16, M, No, Ki, heads, seed=M + No, want=("gemm_tn_kernel",), forbid=("gemm_tn_pipe_kernel", "gemm_tn_wide_kernel"),
                worst=KC.Worst(), key="off")
        assert_f16(launches, "gemm_tn_kernel")
    lib = L.lib()
    lib.rgbnm_gemm_tn_group_begin_n(4)              # inside a bracket too: launched at once, never queued
    try:
        tn_case(F16, 1024, 384, 192, seed=77, want=("gemm_tn_kernel",), forbid=("gemm_tn_pipe_kernel", "gemm_tn_wide_kernel"),
                worst=KC.Worst(), key="off")
    finally:
        L.check(lib.rgbnm_gemm_tn_group_end(L.stream()))
