"""CPU tests of the machinery behind tests/test_swin_nodes.py (no GPU, no rgb_no_more_amd kernel):
- swin_nodes_ref.Engine with T = float64 -- the fp64 stage references composed into the whole model, forward and hand-written
  backward, row-paired views and fold included -- reproduces oracle/swin_torch.swin_forward and its fp64 autograd gradients of
  every parameter to 1e-12: stage-local checks + this anchor = whole-model correctness;
- the Engine's emulation of the nodes' rounding points (fp32 / bf16 / fp16, with and without DropPath scales) goes through the very
  check functions the GPU test calls and passes EVERY stage: the bounds admit a correct implementation (measured on the reference
  side, never on a kernel);
- twelve defects of the Python layer are seeded into the emulation where they would arise in swinv2.py; each has to be rejected by
  the per-element checks.  For each the test also prints what the suite's whole-model 16-bit bars (tests/test_swin.py) make of it,
  measured on the emulated model in bf16, correct against defective: max |dlogit| <= 2.5e-2, the per-tensor gradient error
  <= 2.5e-2 (which the suite applies to twelve sliced tensors only, none of them a q_bias / v_bias) and the median over tensors of
  the gradient-norm error <= 1e-2.  Measured: the logit bar accepts the four backward-only defects (fold_off_diagonal,
  fork_grad_dropped, fork_grad_twice, qv_bias_grads_swapped: |dlogit| = 0); the median bar accepts fold_off_diagonal,
  qv_bias_grads_swapped (0: few tensors move) and nonzero_k_bias (7.9e-3); a per-tensor bar over ALL tensors would reject all
  twelve (0.88 .. 49.5), but over the sliced twelve qv_bias_grads_swapped passes every bar the suite had.  On this two-stage,
  four-block model a forward defect moves the logits by 0.05 (nonzero_k_bias) to 2.0; DESIGN.md section 2 has the table.
"""
import pytest
import torch

import swin_nodes_ref as SN
from oracle import swin_torch as ST

F32, BF16, F16, F64 = torch.float32, torch.bfloat16, torch.float16, torch.float64
CFG = dict(img=64, depths=(2, 2), heads=(3, 6), B=2)
NCLS = 40


def params():
    return SN.make_params(CFG["depths"], CFG["heads"], n_classes=NCLS)


def inputs():
    y, c, _ = SN.make_inputs(CFG["img"], CFG["B"])
    g = torch.Generator().manual_seed(3)
    tgt = torch.rand(CFG["B"], NCLS, generator=g, dtype=F64)
    return y, c, tgt / tgt.sum(1, keepdim=True)


def ce_grad(tgt, scale=1.0):
    """d(mean cross entropy) / d(logits), times the loss scale."""
    return lambda logits: (torch.softmax(logits.double(), 1) - tgt) / tgt.shape[0] * scale


def drops():
    """[blocks][2][B]: block 0 keeps everybody (rate 0), the others drop one sample of one branch."""
    d = torch.ones(4, 2, CFG["B"], dtype=F64)
    a, b = torch.tensor([2.0, 0.0], dtype=F64), torch.tensor([0.0, 2.0], dtype=F64)
    d[1, 0], d[1, 1], d[2, 0], d[3, 1] = a, b, b, a
    return d


# ================================================================================================================= anchor
def test_composed_stage_references_reproduce_the_oracle_model_and_its_gradients(monkeypatch):
    table = ST.coords_table
    monkeypatch.setattr(ST, "coords_table", lambda ws: table(ws).double())     # (the oracle's fp32 table, widened: an fp64 run)
    y, c, tgt = inputs()
    p = {k: v.double().requires_grad_(True) for k, v in params().items()}
    logits = ST.swin_forward(p, y.double(), c.double(), CFG["depths"], CFG["heads"])
    dl = torch.randn(logits.shape, generator=torch.Generator().manual_seed(5), dtype=F64)
    (logits * dl).sum().backward()
    rec = SN.Engine({k: v.detach() for k, v in p.items()}, CFG, F64).run(y.double(), c.double(), dl)

    def close(a, b, what):
        err, scale = float((a.double() - b).abs().max()), float(b.abs().max()) + 1e-300
        assert err <= 1e-12 * scale, f"{what}: max |diff| {err:.3g} at scale {scale:.3g}"
    close(rec["logits"], logits.detach(), "logits")
    assert sorted(rec["grads"]) == sorted(p)
    for k, v in p.items():
        assert float(v.grad.abs().max()) > 0 or "logit_scale" in k, k
        close(rec["grads"][k].reshape(v.shape), v.grad, k)
    # the clamped head's logit_scale gradient is exactly 0, the others are not
    g = rec["grads"]["layers.0.blocks.1.attn.logit_scale"].reshape(-1)
    assert float(g[1]) == 0.0 and float(g[0]) != 0.0


# ============================================================================================================== emulation
_CACHE = {}


def emulated(dt, defect=None, drop=False):
    key = (dt, defect, drop)
    if key not in _CACHE:
        y, c, tgt = inputs()
        scale = 2.0 ** 16 if dt == F16 else 1.0
        _CACHE[key] = SN.Engine(params(), CFG, dt, defect, drops() if drop else None).run(y, c, ce_grad(tgt, scale))
    return _CACHE[key]


def checked(rec):
    w = SN.Worst()
    SN.check_record(rec, w)
    SN.check_grads(rec, w)
    return w


@pytest.mark.parametrize("drop", [False, True], ids=["eval", "droppath"])
@pytest.mark.parametrize("dt", [BF16, F16, F32], ids=["bf16", "f16", "f32"])
def test_emulation_passes_every_stage(dt, drop):
    w = checked(emulated(dt, drop=drop))
    w.report(f"swin nodes emulation {dt} drop={drop}")
    assert not w.errors, "\n".join(w.errors[:10])
    assert w.ok()
    if dt != F32:                  # the 16-bit outputs sit at half an ulp: round-to-nearest of a nearly exact value
        for k in ("qkv", "proj", "fc2", "ln1", "ln2"):       # (g and gp round twice: the pre-activation, then the result)
            assert 0.3 <= w.d[k] <= 0.51, (k, w.d[k])


def old_bars(good, bad):
    """(max |dlogit|, worst per-tensor gradient relative error, median over tensors of the gradient-NORM relative error) of the
    defective emulated model against the correct one: the figures tests/test_swin.py holds to 2.5e-2, 2.5e-2 (on the tensors whose
    slices the golden carries) and 1e-2."""
    dl = float((bad["logits"].double() - good["logits"].double()).abs().max())
    worst, norms = 0.0, []
    for k, g in good["grads"].items():
        b = bad["grads"][k].double().reshape(-1)
        g = g.double().reshape(-1)
        worst = max(worst, float((b - g).norm() / (g.norm() + 1e-30)))
        norms.append(abs(float(b.norm()) - float(g.norm())) / (float(g.norm()) + 1e-30))
    return dl, worst, float(torch.tensor(norms).median())


NEEDS_DROP = ("drop_scale_on_residual", "drop_scale_row_mod_B")


@pytest.mark.parametrize("defect", SN.DEFECTS)
def test_seeded_defect_is_rejected_per_element(defect):
    drop = defect in NEEDS_DROP
    bad = emulated(BF16, defect, drop)
    w = checked(bad)
    failing = sorted(k for k, v in w.d.items() if v > 1.0)
    dl, gr, med = old_bars(emulated(BF16, drop=drop), bad)
    print(f"\n[defect {defect}] rejected at {failing}; old bars: max |dlogit| {dl:.3g} ({'accepts' if dl <= 2.5e-2 else 'rejects'}), "
          f"worst per-tensor gradient error {gr:.3g} ({'accepts' if gr <= 2.5e-2 else 'rejects'}), median gradient-norm error "
          f"{med:.3g} ({'accepts' if med <= 1e-2 else 'rejects'})")
    assert failing and not w.ok(), defect
