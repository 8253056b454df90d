"""The stand-alone attention and LayerNorm entries on hard value regimes, element-wise against fp64 (tests/regime_ref.py: the regimes,
the added bound terms and their derivation; tests/test_value_regimes_cpu.py: the same bounds on emulations and seeded defects).

The conventions are those of tests/test_kernel_edges.py, whose attn_case / ln_case make the launches: canary-guarded outputs, NaN rows
behind every input, workspaces of exactly the size their *_workspace() entry returns, the device kernel of every call asserted
through the profiler (fp16 instantiations included), every element of every output checked -- none excluded -- and the worst
|got - ref| / bound per (path, dtype, regime) printed (-s).  The tensors are the CPU file's (detfill), copied to the device.

Attention: every (path, dtype) of regime_ref.ATTN_PATHS at B = 2, H = 3 (six pairs: all five regimes in one call) for every N of
the path, one H = 1 and one H = 12 case, each at scale = 1 / sqrt(H 64) and 0.125; the persistent forward at 86 x 3 = 258 pairs.
N = 1 also asserts out == v bit for bit.  LayerNorm: 37 rows, row i in regime i % R, three dtypes, forward and backward with dres
and acc on and off: rgbnm_layernorm_* at E in {192, 384, 512, 768, 1024}, rgbnm_ln_generic_* at E in {4, 100, 768} (one wave per row)
and at 768 on the lanes-per-row kernels.

Worst |got - ref| / bound measured on one MI355X (this file's -s output; the largest over the paths of a dtype: first generation
with 7 and 10 tiles in three dtypes, attn2 and attn3 in bf16 and fp16), out / lse / dq / dk / dv:
    fp32  flat .02/.05/.28/.28/.03  peaked .03/.07/.17/.04/.07  offset+ .06/.11/.67/.22/.10  offset- .03/.06/.59/.30/.07  small-v .01/.05/.76/.15/.02
    bf16  flat .35/.05/.20/.11/.24  peaked .35/.04/.24/.23/.28  offset+ .33/.05/.15/.09/.24  offset- .32/.04/.16/.14/.22  small-v .36/.06/.17/.09/.25
    fp16  flat .32/.05/.19/.08/.24  peaked .29/.04/.25/.50/.24  offset+ .22/.06/.15/.09/.20  offset- .21/.06/.14/.11/.20  small-v .48/.05/.005/.004/.47
(fp16 small-v dq / dk: dS ~ 1e-10 rounds to zero in fp16 and the eta term is the whole bound, as the regime intends.)
LayerNorm, y / statistics / dx, the largest over the row regimes (none stands out; the 16-bit outputs sit at half an ulp):
    ln_fwd / ln_bwd_kernel        fp32 .010/.009/.010   bf16 .50/.007/.50   fp16 .49/.006/.49   dgamma, dbeta .014
    ln_generic_* / ln_rows_*      fp32 .28/.24/.21      bf16 .50/.14/.50    fp16 .50/.15/.50    dgamma, dbeta .03
Every kernel passed at the first run; no bound or constant was touched after a figure was seen ("Value regimes").
"""
import pytest

import regime_ref as G
import test_kernel_edges as TE
from kernel_check import nan_padded, ran
from regime_ref import BF16, F16, F32, NAMES
from rgb_no_more_amd import lib as L  # noqa: F401  (loads the library)
from test_fp16_tuned_kernels import is_f16, launches  # noqa: F401  (launches: fixture)
from test_hip_kernels import option  # noqa: F401  (fixture: set a runtime switch for one test)

pytestmark = pytest.mark.gpu
DEV = "cuda"
PATH_IDS = [f"{p[0]}-{NAMES[p[1]]}" for p in G.ATTN_PATHS]


def dev(t):
    """a CPU tensor on the device with three NaN rows behind it"""
    return nan_padded(t.to(DEV), None, 3)


@pytest.mark.parametrize("path", G.ATTN_PATHS, ids=PATH_IDS)
def test_attention_value_regimes(option, launches, path):
    name, dt, opts, ns, _ = path
    for k, v in opts.items():
        option(k, v)
    worst = G.Collect()
    v2 = name.startswith("attn")
    for i, (B, N, H) in enumerate(G.attn_shapes(name, ns)):
        for j, scale in enumerate(G.attn_scales(H)):
            qkv, dout = G.attn_inputs(dt, B, N, H, scale, 100 + 10 * i + j)
            wf, wb = G.attn_kernels(name, dt, B, N, H)

            def check(where, q, d, out, lse, dqkv, s):
                G.attn_check(worst, name, f"{where} scale={s:.4f}", dt, q, d, out, lse, dqkv, B, N, H, s, pshift=v2)
            TE.attn_case(dt, B, N, H, 0, wf, wb, worst, name, qkv=dev(qkv), dout=dev(dout), scale=scale, check=check)
            for names in (launches[-2], launches[-1]):
                hits = [n for n in names if "attn" in n]
                if v2:
                    assert not ran(names, "attn_fwd_kernel") and not ran(names, "attn_bwd_dq_kernel"), sorted(set(names))
                else:
                    assert not any("attn2_" in n or "attn3_" in n for n in names), sorted(set(names))
                if dt == F16:
                    assert hits and all(is_f16(n) for n in hits), hits
    worst.finish(f"value regimes: attention {name} {NAMES[dt]}")


class LnCheck:
    """ln_case's bounds per row regime (regime_ref.ln_check_fwd / ln_check_bwd: the same forms and constants)"""

    def __init__(self, worst, key, dt):
        self.worst, self.key, self.dt = worst, key, dt

    def fwd(self, where, x, gamma, beta, y, mean, rstd, eps, res, sc):
        G.ln_check_fwd(self.worst, self.key, where, self.dt, x, gamma, beta, y, mean, rstd, eps, res, sc)

    def bwd(self, where, x, gamma, dy, mean, rstd, dx, dg, dbt, dres, init, sc):
        G.ln_check_bwd(self.worst, self.key, where, self.dt, x, gamma, dy, mean, rstd, dx, dg, dbt, dres, init, sc)


def ln_rows(dt, E):
    x, dy = G.ln_inputs(dt, G.LN_M, E, 50 + E)
    return dev(x), dev(dy)


@pytest.mark.parametrize("dt", [F32, BF16, F16], ids=lambda d: NAMES[d])
@pytest.mark.parametrize("E", G.LN_E)
def test_layernorm_value_regimes(dt, E):
    """ln_fwd_kernel / ln_bwd_kernel at every width they dispatch: 16 / 8 / 4 rows per workgroup pass, each pass a mix of regimes."""
    worst = G.Collect()
    x, dy = ln_rows(dt, E)
    for dres_on, acc in ((0, 0), (1, 0), (0, 1), (1, 1)):
        TE.ln_case(dt, G.LN_M, E, dres_on, acc, 700 + 10 * dres_on + acc, worst, f"E={E}", want=("ln_fwd_kernel", "ln_bwd_kernel"),
                   x=x, dy=dy, check=LnCheck(worst, f"E={E}", dt))
    worst.finish(f"value regimes: layernorm {NAMES[dt]} E={E}")


@pytest.mark.parametrize("dt", [F32, BF16, F16], ids=lambda d: NAMES[d])
def test_layernorm_any_width_value_regimes(option, dt):
    """ln_generic_fwd / _bwd_kernel (one wave per row, four rows per pass) at E in {4, 100, 768}; ln_rows_* at E = 768; with and
    without the residual and the per-sample scale, accumulating and not."""
    worst = G.Collect()
    for rows, widths, want in ((0, G.LN_GENERIC_E, ("ln_generic_fwd_kernel", "ln_generic_bwd_kernel")),
                               (1, (768,), ("ln_rows_fwd_kernel", "ln_rows_bwd_kernel"))):
        option("ln_rows", rows)
        for E in widths:
            x, dy = ln_rows(dt, E)
            for acc in (0, 1):
                key = f"{'rows' if rows else 'generic'}-E={E}"
                TE.ln_case(dt, G.LN_M, E, False, acc, 800 + acc, worst, key, generic=True, res_on=bool(acc), ss_on=bool(acc),
                           want=want, x=x, dy=dy, check=LnCheck(worst, key, dt))
    worst.finish(f"value regimes: layernorm any-width {NAMES[dt]}")
