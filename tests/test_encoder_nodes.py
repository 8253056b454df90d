"""The encoder's autograd node(s) (plainvit._BlocksFn) on two paths no other test takes, for both node layouts (all blocks in one
node, one node per block).  Model: E = 192, 3 heads, bf16, depth 3, B = 4 (the builder of tests/test_chain_fwd.py).

  several launches per direction   plainvit.CHAIN_MAX_DEPTH patched to 2: the one-launch forward runs as 2 + 1 blocks, the backward as
                                   1 + 2, and a grouped weight-gradient launch takes at most 2 blocks -- the `s0` loops of
                                   ViT._chain_forward / _chain_backward, otherwise reached only by a 13-block model.  Against the
                                   unpatched step of a fresh model with the same weights: logits the same bits (the same per-block
                                   arithmetic, the residual handed over through the same buffer), gradients within 1e-5 of each tensor's
                                   largest magnitude (fp32 sums in another grouping: tests/test_chain_bwd.py::test_other_batches).
  gradient exchange hand-offs      model._grad_sync is a recorder (no process group) whose bucket is too small for the held bracket:
                                   what it is told (`ready`) is model.grad_ready_order(), a gradient announced as ready is final (a
                                   stream-ordered clone taken at the announcement equals the .grad the step ends with), and the
                                   gradients are those of the step without an exchange up to the regrouping -- the same bits where the
                                   group covers every block of the one-node layout (the same launch).
  re-flatten                       the parameter lists the model caches by identity follow `_named` through a `_flatten()`.

Measured on one MI355X (pytest -s), with the two node classes this file was first run on and with the merged one alike: the logits
relation holds as torch.equal, and the worst gradient ratio is 0 in all six cases (the gradients come out equal, as per_block_nodes
does in tests/test_model_history.py).  The re-flatten test failed before `_flatten` dropped `_pe_params`.  The 7 tests take 3 s.
"""
import pytest
import torch
from torch import nn

import rgb_no_more_amd as rg
from rgb_no_more_amd import plainvit as P
from test_chain_fwd import build

pytestmark = pytest.mark.gpu
DEPTH, B = 3, 4
REGROUP = 1e-5          # tests/test_chain_bwd.py::test_other_batches
LAYOUTS = pytest.mark.parametrize("single", [True, False], ids=["one_node", "per_block_nodes"])


def train_step(m, y, c, tgt):
    m.train()
    m.zero_grad(set_to_none=True)
    logits = m(y, c)
    rg.cls_transforms.cross_entropy(logits, tgt, grad_dtype=torch.bfloat16).backward()
    torch.cuda.synchronize()
    return logits.detach().clone(), {n: p.grad.detach().clone() for n, p in m.named_parameters()}


def model(single):
    m, y, c, tgt = build(DEPTH, B)
    m.single_encoder_node = single
    return m, (y, c, tgt)


_PLAIN = {}


def plain_step(single):
    """The ordinary step of this layout on a fresh model (no exchange, CHAIN_MAX_DEPTH as shipped): computed once, never changed."""
    if single not in _PLAIN:
        m, data = model(single)
        _PLAIN[single] = train_step(m, *data)
    return _PLAIN[single]


def worst_regroup(got, ref):
    return max(float((got[n].double() - ref[n].double()).abs().max() / (ref[n].double().abs().max() + 1e-30)) for n in ref)


@LAYOUTS
def test_several_launches_per_direction(monkeypatch, single):
    ref_logits, ref_grads = plain_step(single)
    monkeypatch.setattr(P, "CHAIN_MAX_DEPTH", 2)
    m, data = model(single)
    logits, grads = train_step(m, *data)
    w = worst_regroup(grads, ref_grads)
    print(f"CHAIN_MAX_DEPTH 2, single={single}: logits equal {torch.equal(logits, ref_logits)}, "
          f"max|dlogits| {float((logits - ref_logits).abs().max()):.3e}, worst gradient ratio {w:.3e}")
    assert torch.equal(logits, ref_logits)
    assert w <= REGROUP, w


class Recorder:
    """What parallel.FlatGradSync is to the model, without a process group: bucket_elems = 1 keeps the held bracket off."""
    bucket_elems = 1

    def __init__(self, m):
        self.m, self.calls, self.clones = m, [], []

    def begin_step(self):
        pass

    def ready(self, gbuf, names, last=False):
        self.calls.append((tuple(names), last))
        self.clones += [(n, self.m._gview(gbuf, n).clone()) for n in names]


@LAYOUTS
@pytest.mark.parametrize("group", [1, 4])
def test_gradient_exchange_hand_offs(single, group):
    _, ref_grads = plain_step(single)
    m, data = model(single)
    m.dw_group_overlapped = group
    rec = Recorder(m)
    m._grad_sync = rec
    try:
        _, grads = train_step(m, *data)
    finally:
        m._grad_sync = None
    assert rec.calls == [(tuple(names), last) for names, last in m.grad_ready_order()]
    changed = [n for n, t in rec.clones if not torch.equal(t, grads[n])]
    assert not changed, changed[:4]
    w = worst_regroup(grads, ref_grads)
    print(f"exchange, single={single}, dw_group_overlapped={group}: worst gradient ratio {w:.3e}")
    assert w <= REGROUP, w
    if single and group >= DEPTH:          # one group of all blocks: the launch of the step without an exchange
        assert all(torch.equal(grads[n], ref_grads[n]) for n in ref_grads)


def test_reflatten_rebuilds_the_cached_parameter_lists():
    """_pe_params and the block-parameter list hold Parameter objects; _flatten() rebuilds `_named`, so it has to drop them too.
    (_ensure_flat re-flattens when the SAME Parameter objects have moved, which leaves such lists valid; the lists must not rely on it.)"""
    m, data = model(True)
    m.defer_grad_reduction = True          # begin_hold asks for the patch embedding's parameters
    train_step(m, *data)
    lin = m.patchembed.projection[0]
    lin.weight = nn.Parameter(lin.weight.detach().clone(), requires_grad=False)
    lin.bias = nn.Parameter(lin.bias.detach().clone(), requires_grad=False)
    m._flatten()
    pe = m._pe_params_list()
    assert [id(p) for p in pe] == [id(m._named[n]) for n in m._pe_names]
    assert not any(p.requires_grad for p in pe)
    want = [m._named[n] for i in range(m.depth) for n in m._block_param_order[i]]
    assert [id(p) for p in m._all_block_params()] == [id(p) for p in want]
