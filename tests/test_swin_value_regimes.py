"""The SwinV2 window attention (win_attn_fwd_kernel / win_attn_bwd_kernel) on hard value regimes, element-wise against fp64
(tests/swin_regime_ref.py: the regimes, the check and its fp16 range rule; tests/test_swin_value_regimes_cpu.py: the same check on
an emulation of a correct kernel and on seeded defects), and the continuous position bias at saturation.

The launches are win_case's of tests/test_swin_edges.py (caller inputs through its keywords): canary-guarded outputs, NaN rows behind
every input, a workspace of exactly rgbnm_window_attention_bwd_workspace bytes, both kernels asserted by name through the profiler,
every element of every output checked at weight c = 1 of the derived terms -- none excluded but the counted fp16 elements beyond
the type's range on exactly-zero rows -- and the worst |got - ref| / bound printed per (dtype, regime, output) (-s).  The tensors
are the CPU file's, copied to the device.
- B = 3, res 16, 5 heads (all five scales), shift 0 and 4: 12 windows, every regime in a masked window, the 4-region corner window
  in the signed regime on the s = 100 head (asserted from the mask).  fp32 reaches its two-wave backward, class (e).
- multi-window waves: the smallest (B, res, heads) at which, on the device's CU count, both directions walk >= 3 windows per wave
  with a ragged last range, shift 4, at win_xcd 1 and 0: the prefetch and the per-wave d(bias) accumulators carry across regime
  changes.
- position bias: W2 scaled so that every head's table spans +-120, one block with logit_scale = -20.

Worst |got - ref| / bound at c = 1 measured on one MI355X (256 CUs; this file's -s output), out / lse / dq / dk / dv / d(scale) partial,
12 windows | multi-window waves (fp32: B = 31, res 16, 24 heads; bf16 / fp16: B = 127, res 16, 12 heads):
    fp32  control    .05/.14/.06/.05/.11/.002 | .07/.16/.06/.07/.14/.004    aligned .05/.12/.06/.06/.12/.003 | .07/.15/.06/.07/.15/.004
          signed     .03/.12/.004/.009/.10/.001 | .04/.14/.004/.01/.11/.002   degenerate .06/.14/.06/.06/.14/.004 | .07/.15/.07/.08/.15/.006
          extremes   .04/.12/.04/.05/.10/.002 | .06/.16/.06/.06/.14/.004    small-v .04/.12/.06/.05/.11/.002 | .06/.15/.07/.08/.14/.004
          d(bias) .09 | .06   d(scale) .0007 | .0003
    bf16  control    .36/.26/.31/.27/.43/.02 | .43/.41/.46/.48/.51/.06    aligned .38/.28/.37/.31/.44/.01 | .44/.49/.46/.43/.53/.06
          signed     .31/.26/.003/.05/.44/.0001 | .36/.39/.007/.07/.49/.0002   degenerate .65/.25/.60/.47/.66/.02 | .73/.38/.70/.62/.81/.05
          extremes   .32/.32/.27/.28/.40/.02 | .44/.35/.40/.40/.53/.04    small-v .38/.27/.27/.35/.45/.02 | .49/.37/.39/.40/.53/.05
          d(bias) .35 | .29   d(scale) .002 | .0002
    fp16  control    .31/.24/.28/.31/.39/.03 | .41/.36/.41/.46/.50/.05    aligned .37/.26/.33/.34/.48/.03 | .43/.39/.38/.46/.55/.05
          signed     .27/.17/.0002/.05/.38/.00002 | .34/.42/.0009/.11/.47/.00005   degenerate .66/.31/.49/.49/.56/.04 | .67/.34/.49/.49/.68/.05
          extremes   .35/.27/.50/.50/.48/.02 | .41/.32/.50/.50/.51/.05    small-v .47/.24/.09/.06/.50/.02 | .49/.35/.15/.15/.50/.04
          d(bias) .31 | .29   d(scale) .002 | .0003
The largest is 0.81 (bf16 dv, degenerate rows, multi-window); on the 12 windows the bf16 and fp16 figures equal the CPU
emulation's to two digits.  fp16, own-row gradients of exactly-zero rows over both 12-window cases: dq 10211 elements beyond 65504 by
more than the bound, all +-inf of the reference's sign, and 29 straddling it; dk 8121 and 2119 (multi-window: 1036336 / 4048 and
877336 / 163048).  Every window-attention test passed at its first run on the device and no bound was touched after a figure was
seen.  The position-bias case found three things, fixed in csrc/swin.hip ("Value regimes of the SwinV2 window attention"):
bias 0 where 16 sigmoid(t) is still a number (expf(-t) = inf below t = -88.7), d(table) through 1 - s with a fifth of its value as
error for 8 < t < 17 (dW2 of hidden units that only saturated entries reach: 4.7 times the bound), and exp(logit_scale = -20) 3.3 ulp
off (1.03 times the bound).  Its worst ratios now: bias 0.99 (fp32 subnormals: one ulp), dW2 0.04, db1 / dW1 0.26, scale 0.24.
Run time on that machine: this file 6 s (3 s of it the first test's library start), test_window_attention_edges 0.3 s in the
same process.
"""
import pytest

import swin_ref as R
import swin_regime_ref as G
import test_swin_edges as E
from kernel_check import nan_padded
from oracle import swin_torch as ST
from swin_regime_ref import BF16, F16, F32, NAMES
from test_hip_kernels import option  # noqa: F401  (fixture: set a runtime switch for one test)

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTS = [F32, BF16, F16]


def run_case(option, dt, B, res, heads, shift, xcd, seed, worst, seen, counts):
    option("win_xcd", xcd)
    d = G.win_regime_inputs(dt, B, res, heads, shift, seed)
    qkv = nan_padded(d["qkv"].to(DEV), extra_rows=7)
    dout = nan_padded(d["dout"].to(DEV), extra_rows=5)
    bias = nan_padded(d["bias"].to(DEV).reshape(heads * 64, 64), extra_rows=64).view(heads, 64, 64)
    scale = nan_padded(d["scale"].to(DEV).view(heads, 1), extra_rows=3).view(heads)

    def check(dt_, B_, res_, heads_, shift_, qkv_, dout_, bias_, scale_, out, lse, dqkv, dbias, dsp, dsc, gb, fit, where):
        c = G.win_regime_check(worst, dt, B, res, heads, shift, qkv_, dout_, bias_, scale_, out.t, lse.t, dqkv.t, dbias.t, dsp.t,
                               dsc.t, gb, where, reg=d["reg"])
        for k, v in c.items():
            counts[k] = counts.get(k, 0) + v
    E.win_case(dt, B, res, heads, shift, seed, E.Fit(), seen, xcd, qkv=qkv, dout=dout, bias=bias, scale=scale, c=G.C1, check=check)


@pytest.mark.parametrize("dt", DTS, ids=lambda d: NAMES[d])
def test_window_attention_value_regimes(option, dt):
    worst, seen, counts = G.Collect(), set(), {}
    for B, res, heads, shift in G.CASES:
        if shift:                           # from the mask: the corner window (4 regions) is signed on the s = 100 head
            nW = (res // 8) ** 2
            nreg = [len(set(r.tolist())) for r in G.regions(res, shift)]
            assert bool((ST.shift_mask(res, 8, shift)[nreg.index(4)] != 0).any()) and nreg.count(4) == 1
            reg = G.pair_regimes(B * nW, heads)
            assert any(int(reg[w, 3]) == G.REGIMES.index("signed") for w in range(B * nW) if w % nW == nreg.index(4))
            assert float(G.head_scales(heads)[3]) == 100.0
        run_case(option, dt, B, res, heads, shift, 1, 31, worst, seen, counts)
    option("win_xcd", 1)
    print(f"\n[value regimes: window attention {NAMES[dt]}] launch classes {sorted(seen)}; counts {counts}")
    worst.finish(f"value regimes: window attention {NAMES[dt]}")
    assert max(worst.d.values()) <= 1.0
    assert dt != F32 or "e" in seen
    over = sum(v for k, v in counts.items() if k.endswith(("-dq", "-dk", "-edge")))
    assert (over > 0) == (dt == F16) and counts["zero"] > 0 and (counts["clamped"] > 0) == (dt != F16)


@pytest.mark.parametrize("dt", DTS, ids=lambda d: NAMES[d])
def test_window_attention_value_regimes_multi_window_waves(option, dt):
    worst, seen, counts = G.Collect(), set(), {}
    ncu = E.cus()
    case = G.multi_window_case(G.ESZ[dt], ncu)
    assert case is not None, ncu
    B, res, heads = case
    for xcd in (1, 0):
        for d in ("fwd", "bwd"):
            g = R.geometry(G.ESZ[dt], d, B, res, heads, ncu, xcd)
            assert g["wpw_min"] >= 3 and g["nwin"] % g["wph"], (d, xcd, g)
        run_case(option, dt, B, res, heads, 4, xcd, 47, worst, seen, counts)
    option("win_xcd", 1)
    print(f"\n[value regimes: multi-window waves {NAMES[dt]}] B={B} res={res} heads={heads}; launch classes {sorted(seen)}; counts {counts}")
    worst.finish(f"value regimes: multi-window waves {NAMES[dt]}")
    assert max(worst.d.values()) <= 1.0


def test_position_bias_at_saturation():
    """rgbnm_swin_cpb_fwd / _bwd with every head's table spanning +-120 (expf(-t) overflows below t = -88.7): bias exactly 0.0 and
    16.0 where the fp32 rounding of the fp64 value is, no NaN, d(table) exactly 0 where 16 s (1 - s) rounds to 0, every output
    inside the CPB bound form of tests/test_swin_edges.py; block 1 has logit_scale = -20."""
    fit = E.Fit()
    zeros, tops = E.cpb_case([3, 6, 12, 24], 4000, fit, span=120.0, ls_low=(1,))
    fit.report("position bias at saturation")
    print(f"[position bias at saturation] bias elements exactly 0: {zeros}, exactly 16: {tops}")
    assert zeros > 0 and tops > 0
