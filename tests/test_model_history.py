"""The models' host-side state across mode switches, bit for bit (case data: tests/history_cases.py).

plainvit.py and swinv2.py keep state from one step to the next -- operand shadows and chain images, cached parameter structs, the
skip decision of ViT._prep, an arena pool keyed by (B, dtype, need_grad) whose arenas carry lazily built tables and workspaces, the
flat gradient buffer and its side buffers, SwinV2's brackets.  The kernel tests run one configuration at a time on a freshly built
model; here the configuration changes from step to step:

  history independence   one model H lives through a walk over the modes in which every ordered pair of distinct modes is taken as
                         consecutive steps (an optimizer step after each, so no buffer has seen the next step's weights).  Each step
                         is repeated on a FRESH model F loaded with H's weights of that moment, same mode, inputs and .grad starting
                         condition: logits and every gradient must be the same bits.  Every third step, and after every step whose
                         gradients were attached, F also takes the optimizer step from H's optimizer state: the weights must be the
                         same bits (flat_grad_base against the gather path of FusedClipAdamWWD._flat_grads).
  control                the premise of that comparison: for every mode two fresh models with the same weights agree bit for bit.
                         A mode that does not is a kernel whose result depends on buffer addresses: ADDRESS_DEPENDENT (empty).
  mode relations         what a mode's result owes the default mode's at the same weights (history_cases.RELATION), at three weight
                         states (initial, after 3 and after 6 optimizer steps), each on a fresh model.
  teeth                  defects seeded into the Python layer (monkeypatch) that the checks above must report: a ViT._prep that does
                         nothing for one step after an optimizer step (stale operands), an _acquire_arena that hands a step tables
                         built for another arena's buffers, the held-reduction bracket re-opened for a backward whose gradients are
                         attached; SwinV2: the no-op _prep.

What the suite found when it was written (both fixed in plainvit.py; the teeth keep them found):
  * held reductions with attached gradients (test_teeth_held_bracket_with_attached_gradients).  Before the fix, at the initial
    weights: "held_attached against default: classhead.ch_linear1.weight.grad breaks 'bits'" and so for all 30 gradients of the
    blocks and the head (the patch embedding's two, reduced at once, were right), the same for held_attached_own, 'twice' for
    held_accumulate; in the pairs history first "step 39 (default -> held_attached_own): encoder.0.0.fn.eb_lrnorm1.weight.grad
    differs from a fresh model's" -- 660 reports, all in held_attached and held_attached_own;
  * block shadows skipped by the forward's prep and bwd_chain switched off before the backward
    (test_teeth_skipped_shadows_and_a_late_option_change).  Before the fix: "bwd_off_late against default:
    encoder.0.0.fn.eb_mha.qkv.weight.grad breaks 'regroup' (ratio 1e+05)", i.e. wrong by the tensor's own size, every gradient below
    the head; in the pairs history first "step 7 (default -> bwd_off_late): patchembed.projection.0.weight.grad differs from a fresh
    model's" -- 408 reports, all in bwd_off_late.

Measured on one MI355X (pytest -s), worst ratio to the bar per mode/against over the three weight states; the control passes for
every mode of both models (ADDRESS_DEPENDENT is empty):
  ViT     bits / twice relations 0 (equal): accumulate, attached_zero, held, held_accumulate, held_attached, held_attached_own,
          no_table, tn_direct_off /default; bwd_off_late/bwd_off; held_perop/both_off; no_table_perop/both_off;
          regroup: bwd_off 0.0621, bwd_off_late 0.0621, per_block_nodes 0 (its gradients come out equal);
          rounding: fwd_off, both_off, held_perop, no_table_perop 0.33
  SwinV2  accumulate, attached_zero 0; bracket: grouped 0.0106, grouped_held 0.0106
The 24 tests take 19 s (the longest, the first ViT chunk with its set-up, 2.8 s).
"""
import copy

import numpy as np
import pytest
import torch

import rgb_no_more_amd as rg
from rgb_no_more_amd import detfill, plainvit as P, swinv2 as SW
import history_cases as HC
from kernel_check import Worst
from test_hip_kernels import option  # noqa: F401  (fixture: set a runtime switch for one test)

pytestmark = pytest.mark.gpu
DEV = "cuda"
DT = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
OPT = dict(lr=1e-3, eps=1e-8, weight_decay=1e-4, max_norm=1.0)

# (mode, cause) of the ViT modes whose CONTROL failed (two fresh models, same weights, different bits): the history check holds them to
# their relation's bar instead of bits.  Expected to be empty; it is.
ADDRESS_DEPENDENT = ()


# ------------------------------------------------------------------------------------------------ the two model families
class _Vit:
    name = "vit"
    modes = HC.by_name(HC.VIT_MODES)
    relation = HC.VIT_RELATION
    attr_defaults = HC.VIT_ATTR_DEFAULTS
    _data, _init = {}, {}

    @staticmethod
    def build(ncls=1000):
        c = HC.VIT_MODEL
        return rg.ViT(3, 16, c["emb_size"], depth=c["depth"], n_classes=ncls, drop_p=0.0, device=DEV, num_heads=c["num_heads"],
                      head_size=64, pixel_space="DCT", ver=c["ver"], use_subblock=True)

    @classmethod
    def initial(cls, ncls=1000):
        if ncls not in cls._init:
            shapes = {k: tuple(v.shape) for k, v in cls.build(ncls).state_dict().items()}
            sd = detfill.fill_state_dict(shapes, base_seed=1)
            cls._init[ncls] = {k: torch.from_numpy(v).to(DEV) for k, v in sd.items()}
        return cls._init[ncls]

    @classmethod
    def data(cls, B, ncls=1000):
        if (B, ncls) not in cls._data:
            y = torch.from_numpy(detfill.normalish((B, 1, 28, 28, 8, 8), 71)).to(DEV)
            c = torch.from_numpy(detfill.normalish((B, 2, 14, 14, 8, 8), 72)).to(DEV)
            tgt = torch.from_numpy(detfill.integers((B,), 74, 0, 998, np.int64) % ncls).to(DEV)
            cls._data[(B, ncls)] = (y, c, tgt)
        return cls._data[(B, ncls)]

    @staticmethod
    def set_attrs(m, attrs):
        for k, v in attrs.items():
            setattr(m, k, v)


class _Swin:
    name = "swin"
    modes = HC.by_name(HC.SWIN_MODES)
    relation = HC.SWIN_RELATION
    attr_defaults = HC.SWIN_ATTR_DEFAULTS
    _data, _init = {}, {}

    @staticmethod
    def build(ncls=1000):
        import test_swin as TS
        return TS._model(HC.SWIN_MODEL, DEV)[0]

    @classmethod
    def initial(cls, ncls=1000):
        if not cls._init:
            import test_swin as TS
            from conftest import load_golden
            m = cls.build()
            TS._load(m, HC.SWIN_MODEL, load_golden("g15_swin.npz"))
            cls._init[ncls] = {k: v.detach().clone() for k, v in m.state_dict().items()}
        return cls._init[ncls]

    @classmethod
    def data(cls, B, ncls=1000):
        if B not in cls._data:
            import test_swin as TS
            nb = TS.CASES[HC.SWIN_MODEL][0] // 8
            y = torch.from_numpy(detfill.normalish((B, 1, nb, nb, 8, 8), 171)).to(DEV)
            c = torch.from_numpy(detfill.normalish((B, 2, nb // 2, nb // 2, 8, 8), 172)).to(DEV)
            tgt = detfill.uniform((B, 1000), 173, 0.0, 1.0)
            cls._data[B] = (y, c, torch.from_numpy(tgt / tgt.sum(1, keepdims=True)).to(DEV))
        return cls._data[B]

    @staticmethod
    def set_attrs(m, attrs):
        for k, v in attrs.items():
            if k == "drop_path_p":
                for ly in m.layers:
                    for blk in ly.blocks:
                        blk.drop_path_p = v
            else:
                setattr(m, k, v)


# ------------------------------------------------------------------------------------------------ one step in one mode
def start_grads(m, kind):
    """The .grad starting condition of a training step (history_cases: grads)."""
    if kind == "none":
        m.zero_grad(set_to_none=True)
    elif kind == "flat":
        # what zero_grad(set_to_none=False) leaves after an ordinary step: zeros in the views of the flat gradient buffer that
        # autograd adopted.  A model that has no gradients yet gets exactly those views.
        m._ensure_flat()
        for n, p in m._named.items():
            if p.grad is None:
                p.grad = m._gview(m._gflat, n)
            p.grad.zero_()
    else:
        for p in m.parameters():
            p.grad = torch.zeros_like(p)


def run_step(fam, m, mode, option, ncls=1000):
    """One step of `m` in `mode`: (logits, {name: gradient} or None for eval), as clones."""
    for k, v in HC.OPTION_DEFAULTS.items():
        option(k, mode.options.get(k, v))
    fam.set_attrs(m, {**fam.attr_defaults, **mode.attrs})
    cdt = DT[mode.dtype]
    m.compute_dtype = cdt
    y, c, tgt = fam.data(mode.B, ncls)
    if mode.kind == "eval":
        m.eval()
        with torch.no_grad():
            logits = m(y, c).detach().clone()
        torch.cuda.synchronize()
        return logits, None
    m.train()
    start_grads(m, mode.grads)
    for _ in range(2 if mode.kind == "accumulate" else 1):
        if mode.seed is not None:
            torch.manual_seed(mode.seed)
        logits = m(y, c)
        loss = rg.cls_transforms.cross_entropy(logits, tgt, grad_dtype=cdt)
        if mode.loss_scale != 1.0:
            loss = loss * mode.loss_scale
        for k, v in mode.late.items():
            option(k, v)
        try:
            loss.backward()
        finally:
            for k in mode.late:
                option(k, mode.options.get(k, HC.OPTION_DEFAULTS[k]))
    torch.cuda.synchronize()
    return logits.detach().clone(), {n: p.grad.detach().clone() for n, p in m.named_parameters()}


def fresh(fam, weights, ncls=1000):
    m = fam.build(ncls)
    m.load_state_dict(weights)
    return m


def snapshot(m):
    return {k: v.detach().clone() for k, v in m.state_dict().items()}


# ------------------------------------------------------------------------------------------------ comparing two results
def ratio(kind, got, ref, what):
    """|difference| over the bar of relation `kind` (<= 1 passes); bits / twice: 0 or inf."""
    if kind == "bits":
        return 0.0 if torch.equal(got, ref) else float("inf")
    if kind == "twice":
        return 0.0 if torch.equal(got, 2 * ref) else float("inf")
    g, r = got.double(), ref.double()
    if not torch.isfinite(g).all():
        return float("inf")
    if kind in ("regroup", "bracket"):                        # max |d| against the tensor's scale
        return float((g - r).abs().max() / (r.abs().max() + 1e-30)) / HC.BARS[kind]
    assert kind == "rounding"
    if what == "logits":
        return float((g - r).abs().max()) / HC.BARS["rounding_logits"]
    return float((g - r).norm() / max(float(r.norm()), 1e-30)) / HC.BARS["rounding_grads"]


def differences(rel, got, ref):
    """[(tensor name, ratio)] of what breaks relation `rel` between two results of run_step, and the worst ratio seen."""
    bad, worst = [], 0.0
    if rel.logits != "none":
        x = ratio(rel.logits, got[0], ref[0], "logits")
        worst = max(worst, x)
        if not x <= 1.0:
            bad.append(("logits", x))
    if rel.grads != "none" and got[1] is not None:
        for n in ref[1]:
            x = ratio(rel.grads, got[1][n], ref[1][n], "grads")
            worst = max(worst, x)
            if not x <= 1.0:
                bad.append((n + ".grad", x))
    return bad, worst


BITS = HC.Relation("bits", "bits", None, "history independence")


# ------------------------------------------------------------------------------------------------ history independence
def run_history(fam, history, option, ncls=1000, before_step=None):
    """Walk `history` on one model H, repeating every step on a fresh model; returns the mismatches as strings."""
    H = fresh(fam, fam.initial(ncls), ncls)
    opt = rg.custom_optims.FusedClipAdamWWD(H, **OPT)
    bad, prev = [], None
    for i, name in enumerate(history):
        mode = fam.modes[name]
        where = f"step {i} ({prev} -> {name})"
        weights = snapshot(H)
        if before_step is not None:
            before_step(i, H)
        got = run_step(fam, H, mode, option, ncls)
        F = fresh(fam, weights, ncls)
        want = run_step(fam, F, mode, option, ncls)
        rel = fam.relation[name][0] if name in [x[0] for x in ADDRESS_DEPENDENT] else BITS
        diff, _ = differences(rel, got, want)
        bad += [f"{where}: {t} differs from a fresh model's (ratio {x:.3g})" for t, x in diff]
        if got[1] is not None:
            nonfinite = [n for n, g in got[1].items() if not torch.isfinite(g).all()]
            bad += [f"{where}: {n}.grad is not finite" for n in nonfinite]
            if i % 3 == 0 or mode.grads != "none" or mode.kind == "accumulate":
                opt_f = rg.custom_optims.FusedClipAdamWWD(F, **OPT)
                opt_f.load_state_dict(copy.deepcopy(opt.state_dict()))
                opt.step()
                opt_f.step()
                torch.cuda.synchronize()
                if not diff:
                    wf = F.state_dict()
                    bad += [f"{where}: weight {k} differs after the optimizer step" for k, v in H.state_dict().items()
                            if not torch.equal(v, wf[k])]
            else:
                opt.step()
        prev = name
        del F, want
    return bad


def report(bad):
    assert not bad, f"{len(bad)} mismatches, first: " + " | ".join(bad[:8])


VIT_PARTS = HC.chunks(HC.vit_pairs_history(), HC.VIT_CHUNK)
SWIN_PARTS = HC.chunks(HC.swin_pairs_history(), HC.SWIN_CHUNK)


@pytest.mark.parametrize("part", range(len(VIT_PARTS)))
def test_vit_history_independence(option, part):  # noqa: F811
    report(run_history(_Vit, VIT_PARTS[part], option))


def test_vit_history_independence_with_a_padded_head(option):  # noqa: F811
    """n_classes = 10: the padded head (_b2pad, the padded gradient buffers of _HeadFn.backward)."""
    report(run_history(_Vit, HC.vit_classcount_history(), option, ncls=10))


@pytest.mark.parametrize("part", range(len(SWIN_PARTS)))
def test_swin_history_independence(option, part):  # noqa: F811
    report(run_history(_Swin, SWIN_PARTS[part], option))


# ------------------------------------------------------------------------------------------------ control
def control(fam, option, ncls=1000):
    bad = []
    for name, mode in fam.modes.items():
        a = run_step(fam, fresh(fam, fam.initial(ncls), ncls), mode, option, ncls)
        b = run_step(fam, fresh(fam, fam.initial(ncls), ncls), mode, option, ncls)
        diff, _ = differences(BITS, a, b)
        bad += [f"{name}: {t}" for t, _ in diff]
    return bad


def test_vit_control_two_fresh_models_agree(option):  # noqa: F811
    bad = control(_Vit, option)
    assert sorted({b.split(":")[0] for b in bad}) == sorted(x[0] for x in ADDRESS_DEPENDENT), bad[:8]


def test_swin_control_two_fresh_models_agree(option):  # noqa: F811
    bad = control(_Swin, option)
    assert not bad, bad[:8]


# ------------------------------------------------------------------------------------------------ mode relations
def weight_states(fam, option, steps=(0, 3, 6)):
    """The weights after 0, 3 and 6 optimizer steps of default-mode training."""
    m = fresh(fam, fam.initial())
    opt = rg.custom_optims.FusedClipAdamWWD(m, **OPT)
    out = []
    for k in range(max(steps) + 1):
        if k in steps:
            out.append(snapshot(m))
        if k < max(steps):
            run_step(fam, m, fam.modes["default"], option)
            opt.step()
    return out


def relation_failures(fam, weights, option, names=None, worst=None):
    """Every mode (or `names`) on a fresh model against the mode its relations name, at `weights`."""
    cache, bad = {}, []

    def result(name):
        if name not in cache:
            cache[name] = run_step(fam, fresh(fam, weights), fam.modes[name], option)
        return cache[name]

    for name in (names or list(fam.modes)):
        if name == "default":
            continue
        for rel in fam.relation[name]:
            if rel.logits == "none" and rel.grads == "none":
                continue
            diff, w = differences(rel, result(name), result(rel.against))
            if worst is not None:
                worst(f"{name}/{rel.against}", w)
            bad += [f"{name} against {rel.against}: {t} breaks '{rel.logits if t == 'logits' else rel.grads}' (ratio {x:.3g})"
                    for t, x in diff]
    return bad


@pytest.mark.parametrize("fam", [_Vit, _Swin], ids=["vit", "swin"])
def test_mode_relations(option, fam):  # noqa: F811
    worst, bad = Worst(), []
    for k, weights in zip((0, 3, 6), weight_states(fam, option)):
        bad += [f"after {k} optimizer steps: {b}" for b in relation_failures(fam, weights, option, worst=worst)]
    worst.report(f"{fam.name} mode relations, mode/against")
    report(bad)


# ------------------------------------------------------------------------------------------------ teeth
def test_teeth_stale_operands_after_an_optimizer_step(option, monkeypatch):  # noqa: F811
    """ViT._prep does nothing for the one step that follows an optimizer step: H computes with the operands of the step before."""
    orig, armed = P.ViT._prep, {}

    def prep(self, cdtype, chains=True, shadows=False):
        if armed.get("model") is self:
            armed["model"] = None
            self._prep_gen += 1
            return None
        return orig(self, cdtype, chains, shadows)

    monkeypatch.setattr(P.ViT, "_prep", prep)
    bad = run_history(_Vit, ["default", "held", "default", "default"], option,
                      before_step=lambda i, H: armed.update(model=H) if i == 2 else None)
    assert bad and all(b.startswith("step 2 (held -> default)") for b in bad), bad[:4]
    assert any("logits" in b for b in bad)


def test_teeth_an_arena_with_another_arenas_tables(option, monkeypatch):  # noqa: F811
    """_acquire_arena hands a need_grad step a new arena that carries the lazily built members of the pooled one: chain tables whose
    pointers are the OTHER arena's buffers (all of the same size and alive: the pooled arena stays in the pool)."""
    orig, armed = P.ViT._acquire_arena, {}
    lazy = ("chain_table", "chain_bwd_table", "du_blk", "dxmid_blk", "dqkv_blk", "dx_blk", "dattn_chain", "lnpart", "ws_chain")

    def acquire(self, B, cdtype, need_grad):
        pool = self._arenas.get((B, cdtype, need_grad))
        if armed.get("model") is self and need_grad and pool and pool[-1].chain_bwd_table is not None:
            armed["model"] = None
            old = pool[-1]
            new = P._Arena(self, B, cdtype, need_grad)
            for k in lazy:
                setattr(new, k, getattr(old, k))
            new.chain_bwd_dy = new.dx[0].data_ptr()           # "nothing to rebuild"
            new.donor = old
            return new
        return orig(self, B, cdtype, need_grad)

    monkeypatch.setattr(P.ViT, "_acquire_arena", acquire)
    bad = run_history(_Vit, ["default", "default", "default"], option, before_step=lambda i, H: armed.update(model=H) if i == 2 else None)
    assert armed.get("model") is None
    assert bad and all(b.startswith("step 2 (default -> default)") for b in bad), bad[:4]


def test_teeth_held_bracket_with_attached_gradients(option, monkeypatch):  # noqa: F811
    """Before the fix _FwdState.begin_hold opened the held-reduction bracket also for a backward whose gradients autograd adds to
    attached .grad tensors: the sums were added before they existed.  With the guard taken out again the relations of the three
    held + attached modes must fail (the history check alone would not notice: a fresh model is wrong in the same way)."""
    weights = _Vit.initial()
    names = ["held_attached", "held_accumulate", "held_attached_own"]
    assert not relation_failures(_Vit, weights, option, names)
    monkeypatch.setattr(P._FwdState, "grads_attached", lambda self: False)
    bad = relation_failures(_Vit, weights, option, names)
    for n in names:
        assert any(b.startswith(n + " against default") for b in bad), (n, bad[:4])


def test_teeth_skipped_shadows_and_a_late_option_change(option, monkeypatch):  # noqa: F811
    """Before the fix a backward that found bwd_chain switched off after its forward ran rgbnm_vit_block_bwd on block shadows the
    forward's prep had skipped: zeros on a fresh model, the weights of some earlier per-operation step on a used one.  With
    ViT._ensure_block_shadows taken out again both checks must report mode bwd_off_late."""
    weights = _Vit.initial()
    history = ["default", "both_off", "bwd_off_late", "default"]
    assert not relation_failures(_Vit, weights, option, ["bwd_off_late"])
    monkeypatch.setattr(P.ViT, "_ensure_block_shadows", lambda self, st: None)
    bad = relation_failures(_Vit, weights, option, ["bwd_off_late"])
    assert any(b.startswith("bwd_off_late against default") for b in bad) and any(b.startswith("bwd_off_late against bwd_off") for b in bad)
    bad = run_history(_Vit, history, option)
    assert bad and all(b.startswith("step 2 (both_off -> bwd_off_late)") for b in bad), bad[:4]


def test_teeth_swin_stale_operands(option, monkeypatch):  # noqa: F811
    orig, armed = SW.SwinTransformerV2._prep, {}

    def prep(self, cdtype):
        if armed.get("model") is self:
            armed["model"] = None
            return self._sh_views[cdtype]
        return orig(self, cdtype)

    monkeypatch.setattr(SW.SwinTransformerV2, "_prep", prep)
    bad = run_history(_Swin, ["default", "grouped_held", "default"], option,
                      before_step=lambda i, H: armed.update(model=H) if i == 2 else None)
    assert bad and all(b.startswith("step 2 (grouped_held -> default)") for b in bad), bad[:4]
