"""SwinV2's autograd nodes (rgb_no_more_amd/swinv2.py) checked stage by stage against fp64, on the model's own run.

The forward is a chain of torch.autograd.Function nodes, so the graph is the record: tests/swin_nodes_ref.py walks it from
logits.grad_fn (topology: the node sequence and every (node, output index) edge are asserted by construction -- the shortcut
forks, the one _CpbFn node feeding every block at outputs 2k / 2k + 1, the _QkvBiasFn inputs, shift per block parity), reads each
node's saved tensors and ctx attributes before backward() and hooks each node for the gradients it receives and returns.  Every
stored tensor and every returned gradient is then compared per element with the fp64 result of that ONE stage applied to the
tensors the same run stored upstream (bounds: the module docstring of tests/swin_nodes_ref.py; no constant is fitted here), every
parameter's .grad with what its node returned bit for bit, and the bias operands of the prep launch with their parameters bit for
bit (the qkv Linear's: q_bias | +0 | v_bias).

Cases (parameters: oracle.swin_torch.fill_params with one logit_scale on the clamp; inputs: detfill.normalish; the loss scaled by
2^16 in every dtype, as in tests/test_swin_fp16_model.py):
- small model: img 64, depths (2, 2), heads (3, 6), B = 2 -- stage 1 on a 16 x 16 grid with shift 4 on block 1, 512 rows, every
  Linear row-paired; stage 2 on the 8 x 8 grid (shift forced to 0), width 192, the reduction 192 x 384 unpaired.  bf16, fp16 with
  f16_tuned 0 and 1, fp32.
- four stages: img 256, depths (2, 2, 2, 2), heads (3, 6, 12, 24), widths 96 .. 768, B = 4 (NOT 2: gemm_nt_kpipe takes 8192 rows
  and more -- stage 1's paired fc2 runs on 16384 / 2 -- and gemm_nt_wres 4096 at K = 192; both are what the library's dispatch
  selects for SwinV2-T at B = 256).  bf16 and fp16 with f16_tuned 1; the tuned kernels are asserted by name on the bf16 run.
- DropPath: the small model in train mode, drop_path_rate 0.5, B = 8; the saved sscale vectors must hold a zero and a non-zero entry
  in some branch and all ones in block 0.
- bracket: the small model in bf16 with group_dw_backward, hold_reductions both ways: every node's dx / dqkv bit for bit the
  default run's, every final .grad within the fp64 bound computed from the default run's tensors (this reaches the deferred fold
  of the paired layers).

Worst |got - ref| / bound on one MI355X over all cases, bf16 | fp16 | fp32 ("SwinV2 nodes, element-wise"):
Linear outputs 0.500 | 0.499 | 0.158, g 0.497 | 0.612 | 0.043, g' 0.496 | 0.481 | 0.025, LayerNorm outputs 0.499 | 0.496 | 0.023
(statistics 0.018), pooled 0.312 | 0.296 | 0.004, embedding 0.500 | 0.499 | 0.301, attention out 0.200 | 0.193 | 0.147, lse 0.411 |
0.536 | 0.282, dq 0.295 | 0.334 | 0.164, dk 0.387 | 0.364 | 0.171, dv 0.339 | 0.401 | 0.151, d(bias) 0.337 | 0.210 | 0.024, d(scale)
0.475 | 0.507 | 0.663, position bias 0.482, scale 0.485, their gradients 0.049 - 0.469, Linear dx 0.499 | 0.494 | 0.051, _MlpFn dx
0.217 | 0.185 | 0.004, LayerNorm dx 0.499 | 0.495 | 0.017, mean backward 0 | 0.499 | 0, weight gradients <= 0.033 (head 0.311, fc1
0.209), biases <= 0.106, LayerNorm parameter sums <= 0.016; every bit-for-bit comparison holds.  The fp32 case holds the same
references to fp32 bounds (2^16 times tighter in their ulp term): it anchors them.  The ten tests take 7.5 s.
"""
import pytest
import torch

import kernel_check as KC
import swin_nodes_ref as SN
import rgb_no_more_amd as rg
from test_hip_kernels import option  # noqa: F401  (fixture: set a runtime switch for one test)

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
NAMES = {F32: "f32", BF16: "bf16", F16: "f16"}
LOSS_SCALE = 2.0 ** 16


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


_MODELS = {}


def model_of(case, drop=0.0):
    """One model per (shape, drop rate), shared by the tests of that shape (its parameters never change: no optimizer step)."""
    key = (case["img"], case["depths"], drop)
    if key not in _MODELS:
        m = rg.SwinTransformerV2(img_size=case["img"], patch_size=4, embed_dim=96, depths=case["depths"], num_heads=case["heads"],
                                 window_size=8, mlp_ratio=4.0, drop_rate=0.0, attn_drop_rate=0.0, drop_path_rate=drop,
                                 qkv_bias=True, ape=False, patch_norm=True, pretrained_window_sizes=[0] * len(case["depths"]),
                                 device=DEV, pixel_space="dct")
        missing = m.load_state_dict(SN.make_params(case["depths"], case["heads"]), strict=False)
        assert not missing.unexpected_keys and all("relative_" in k or "attn_mask" in k for k in missing.missing_keys), missing
        _MODELS[key] = m
    return _MODELS[key]


def run(case, dt, train=False, drop=0.0, bracket=False, hold=True):
    """One forward + backward, observed; returns (record, kernel names)."""
    m = model_of(case, drop)
    m.train(train)
    m.compute_dtype = dt
    m.group_dw_backward, m.hold_reductions = bracket, hold
    m.zero_grad(set_to_none=True)
    y, c, tgt = (t.to(DEV) for t in SN.make_inputs(case["img"], case["B"]))
    rec = dict(cfg=dict(case, dt=dt), y=y, c=c, params={n: p.detach() for n, p in m.named_parameters()})

    def step():
        logits = m(y, c)
        T = SN.topology(m, logits)
        rec["nodes"] = SN.observe(m, T, dt, bracket)
        rec["logits"] = logits.detach()
        loss = rg.cls_transforms.cross_entropy(logits, tgt, grad_dtype=dt)
        (loss * LOSS_SCALE).backward()
    _, names = KC.launched(step)
    rec["grads"] = {n: p.grad for n, p in m.named_parameters()}
    assert all(g is not None and bool(torch.isfinite(g).all()) for g in rec["grads"].values())
    m.group_dw_backward = False
    return rec, names


def verdict(w, title):
    w.report(title)
    assert not w.errors, f"{title}: {len(w.errors)} violations\n" + "\n".join(w.errors[:12])
    assert w.ok()


def check(rec, title):
    w = SN.Worst()
    SN.check_record(rec, w, cus())
    SN.check_grads(rec, w)
    verdict(w, title)
    return w


@pytest.mark.parametrize("dt,tuned", [(BF16, 0), (F16, 0), (F16, 1), (F32, 0)], ids=["bf16", "f16", "f16-tuned", "f32"])
def test_small_model_every_node_per_element(option, dt, tuned):
    option("f16_tuned", tuned)
    rec, names = run(SN.SMALL, dt)
    N = rec["nodes"]
    assert all(N[f"b{k}.{s}"]["pair"] for k in (0, 1) for s in ("qkv", "proj")) and N["b0.mlp"]["p1"] and N["b0.mlp"]["p2"]
    assert not any(N[f"b{k}.{s}"]["pair"] for k in (2, 3) for s in ("qkv", "proj")) and not N["m0.red"]["pair"]
    assert [N[f"b{k}.attn"]["geo"][4] for k in range(4)] == [0, 4, 0, 0]
    assert float(rec["params"]["layers.0.blocks.1.attn.logit_scale"].max()) > SN.LN100
    assert KC.ran(names, "win_attn_fwd_kernel") and KC.ran(names, "win_attn_bwd_kernel"), sorted(set(names))
    check(rec, f"swin nodes small {NAMES[dt]} f16_tuned={tuned}")


TUNED = ("gemm_nt_small", "gemm_nt_kpipe", "gemm_nt_wres", "gemm_tn_pipe", "gemm_tn_wide", "win_attn_fwd_kernel",
         "win_attn_bwd_kernel")


@pytest.mark.parametrize("dt,tuned", [(BF16, 0), (F16, 1)], ids=["bf16", "f16-tuned"])
def test_four_stages_every_node_per_element(option, dt, tuned):
    option("f16_tuned", tuned)
    rec, names = run(SN.FOUR, dt)
    assert [rec["nodes"][f"b{k}.attn"]["geo"][4] for k in range(8)] == [0, 4, 0, 4, 0, 4, 0, 0]
    for kern in TUNED:
        assert KC.ran(names, kern), f"{kern} did not run; ran {sorted(set(names))}"
    # rgbnm_ln_generic_*: its lanes-per-row kernels at the stage widths (option ln_rows, the default), one wave per row otherwise
    assert KC.ran(names, "ln_rows_fwd_kernel") or KC.ran(names, "ln_generic_fwd_kernel"), sorted(set(names))
    assert KC.ran(names, "ln_rows_bwd_kernel") or KC.ran(names, "ln_generic_bwd_kernel"), sorted(set(names))
    check(rec, f"swin nodes four stages {NAMES[dt]} f16_tuned={tuned}")


@pytest.mark.parametrize("dt", [BF16, F16], ids=["bf16", "f16"])
def test_drop_path_every_node_per_element(dt):
    torch.manual_seed(0)
    rec, _ = run(SN.DROP, dt, train=True, drop=0.5)
    N = rec["nodes"]
    ss = [N[f"b{k}.{s}"]["ss"] for k in range(4) for s in ("ln1", "ln2")]
    assert all(s is not None and s.numel() == SN.DROP["B"] for s in ss)
    assert bool((ss[0] == 1).all()) and bool((ss[1] == 1).all())                     # block 0: rate 0
    assert any(bool((s == 0).any()) and bool((s != 0).any()) for s in ss)
    check(rec, f"swin nodes DropPath {NAMES[dt]}")


@pytest.mark.parametrize("hold", [True, False], ids=["hold", "no-hold"])
def test_bracket_run_same_dx_bits_and_grads_in_bound(hold):
    rec0, _ = run(SN.SMALL, BF16)
    m = model_of(SN.SMALL)
    before = m.__dict__["_dw_bracket"].id if "_dw_bracket" in m.__dict__ else 0
    rec1, names = run(SN.SMALL, BF16, bracket=True, hold=hold)
    br = m.__dict__["_dw_bracket"]
    assert br.id > before and not br.active, "the weight-gradient bracket was not opened and closed by this pass"
    assert all(n["dW"] is None for n in rec1["nodes"].values() if isinstance(n, dict) and n["kind"] == "lin")
    w = SN.Worst()
    SN.same_dx(rec0, rec1, w)
    SN.check_record(SN.with_grads(rec0, rec1["grads"]), w, cus())
    verdict(w, f"swin nodes bracket hold={hold}")
    # the bracket was open: the unpaired Linears' weight gradients ran as grouped launches
    assert KC.ran(names, "gemm_tn_pipe") or KC.ran(names, "gemm_tn_wide"), sorted(set(names))
