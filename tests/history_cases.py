"""Case data of tests/test_model_history.py: the modes a training loop can switch between from one step to the next, the
histories (lists of modes) one model lives through, and what each mode's result owes the `default` mode's.  Pure data: importing
this module needs no GPU (tests/test_model_history_cpu.py checks its coverage claims).

A MODE fully determines one step: the library options that hold while it runs (every option in OPTION_DEFAULTS is set for every
step: the mode's value or the default), model attributes, compute dtype, batch size, what the step does (`kind`) and what the
.grad tensors are when it starts (`grads`).

  kind   "train"       one forward + backward
         "accumulate"  two forward + backward passes, no zeroing in between
         "eval"        model.eval() under no_grad: logits only (the need_grad=False arena)
  grads  "none"        zero_grad(set_to_none=True): autograd adopts the views the backward kernels wrote
         "flat"        attached zeros that alias the model's flat gradient buffer -- the state zero_grad(set_to_none=False)
                       leaves after an ordinary step: the backward writes a side buffer (FlatParamModule._grad_buffer)
         "own"         attached zeros in tensors of their own (p.grad = zeros_like(p)): the backward writes the flat buffer and
                       autograd adds it to them
  late   options set AFTER the forward and put back after the backward
  seed   torch.manual_seed(seed) immediately before every forward (dropout / drop-path draws)
  loss_scale  the loss is multiplied by it before backward() (a power of two; fp16: without one the gradients underflow)

A RELATION says what a mode's logits and gradients owe the mode `against` (default: "default") at the same weights and inputs:

  bits      torch.equal
  twice     exactly 2 x (g + g is exact in fp32)
  regroup   max|d| <= 1e-5 max|ref| per parameter: fp32 sums taken in another grouping
  rounding  logits within 2e-2 absolute, gradients within 5e-2 relative L2 per parameter: another kernel path, bf16 rounding
  none      nothing beyond history independence (values pinned by the model tests of that dtype / batch / feature)

Every relation names the test or header its bar comes from (`source`); no tolerance is new.
"""
from collections import namedtuple

Mode = namedtuple("Mode", "name options late attrs dtype B kind grads seed loss_scale")
Relation = namedtuple("Relation", "logits grads against source")

# ------------------------------------------------------------------------------------------------ ViT
VIT_MODEL = dict(emb_size=192, num_heads=3, depth=2, ver=1)          # as tests/test_chain_fwd.py::build
OPTION_DEFAULTS = {"fwd_chain": 1, "bwd_chain": 1, "tn_direct": 1, "gelu_table": 1, "f16_tuned": 0}      # csrc/vit.hip g_opts
VIT_ATTR_DEFAULTS = {"single_encoder_node": True, "defer_grad_reduction": False, "drop_p": 0.0, "train_dropout": False}
HELD = {"defer_grad_reduction": True}
BOTH_OFF = {"fwd_chain": 0, "bwd_chain": 0}


def _mode(name, options=None, late=None, attrs=None, dtype="bf16", B=4, kind="train", grads="none", seed=None, loss_scale=1.0):
    return Mode(name, dict(options or {}), dict(late or {}), dict(attrs or {}), dtype, B, kind, grads, seed, loss_scale)


VIT_MODES = [
    _mode("default"),
    _mode("fwd_off", {"fwd_chain": 0}),
    _mode("bwd_off", {"bwd_chain": 0}),
    _mode("both_off", BOTH_OFF),
    _mode("bwd_off_late", late={"bwd_chain": 0}),
    _mode("per_block_nodes", attrs={"single_encoder_node": False}),
    _mode("held", attrs=HELD),
    _mode("held_perop", BOTH_OFF, attrs=HELD),
    _mode("tn_direct_off", {"tn_direct": 0}),
    _mode("B3", B=3),                       # generic weight-gradient kernel
    _mode("B16", B=16),                     # B * 196 divisible by 64: the grouped pipelined launch
    _mode("fp32", dtype="fp32"),
    _mode("fp16", dtype="fp16", loss_scale=256.0),
    _mode("fp16_tuned", {"f16_tuned": 1}, dtype="fp16", loss_scale=256.0),
    _mode("dropout", attrs={"drop_p": 0.1, "train_dropout": True}, seed=1234),
    _mode("eval", kind="eval"),
    _mode("attached_zero", grads="flat"),
    _mode("accumulate", kind="accumulate"),
    _mode("held_attached", attrs=HELD, grads="flat"),
    _mode("held_accumulate", attrs=HELD, kind="accumulate"),
    # the held bracket with gradients attached by hand: the backward writes the flat buffer itself, not a side buffer
    _mode("held_attached_own", attrs=HELD, grads="own"),
    # gelu_table = 0 for the step.  The chain kernels carry their own copy of the table and do not read the option (csrc/vit_chain.hip
    # refuses only when rgbnm_gelu_table_init found no usable table, which no option reaches: _chain_refused stays False), and no other
    # kernel of the default step has a GELU: the step is the default step
    _mode("no_table", {"gelu_table": 0}),
    # ... so the option is also crossed with the per-operation kernels, whose GELU epilogues do read it
    _mode("no_table_perop", {"gelu_table": 0, "fwd_chain": 0, "bwd_chain": 0}),
]
VIT_CLASSCOUNT_MODES = ("default", "both_off", "held", "attached_zero", "accumulate", "eval", "fp32")      # n_classes = 10: padded head

_HELD_SRC = "include/rgbnm.h rgbnm_reduce_hold_*: held reductions keep the summation order (tests/test_held_reductions.py)"
_ZERO_SRC = "0 + g is exact in fp32; tests/test_vit_model.py::test_vit_step_is_bit_reproducible"
_TWICE_SRC = "g + g is exact in fp32; tests/test_vit_model.py::test_vit_step_is_bit_reproducible"
_REGROUP_SRC = "tests/test_chain_bwd.py::test_other_batches (1e-5 of the tensor's scale: fp32 sums in another grouping)"
_ROUND_SRC = "tests/test_chain_fwd.py::test_saved_tensors_match_the_per_operation_path (logits 2e-2, gradients 5e-2 rel L2)"
_SAME_SRC = "tests/test_vit_model.py::test_vit_step_is_bit_reproducible: the same kernels on the same operands"
_TABLE_SRC = "tests/test_gelu_table.py: the table holds the library's own GELU arithmetic for every bf16 input (same bits)"


def _rel(logits, grads, source, against="default"):
    return Relation(logits, grads, against, source)


_NONE = _rel("none", "none", "values pinned by the model tests of this dtype / batch / feature "
             "(tests/test_vit_model.py, test_fp16_model.py, test_fp16_tuned_model.py, test_dropout_model.py)")

VIT_RELATION = {
    "default": (_rel("bits", "bits", "tests/test_vit_model.py::test_vit_step_is_bit_reproducible"),),
    "fwd_off": (_rel("rounding", "rounding", _ROUND_SRC),),
    "bwd_off": (_rel("bits", "regroup", _REGROUP_SRC),),
    "both_off": (_rel("rounding", "rounding", _ROUND_SRC),),
    "bwd_off_late": (_rel("bits", "regroup", _REGROUP_SRC), _rel("bits", "bits", _SAME_SRC, "bwd_off")),
    "per_block_nodes": (_rel("bits", "regroup", _REGROUP_SRC),),
    "held": (_rel("bits", "bits", _HELD_SRC),),
    "held_perop": (_rel("rounding", "rounding", _ROUND_SRC), _rel("bits", "bits", _HELD_SRC, "both_off")),
    "tn_direct_off": (_rel("bits", "bits", "tests/test_chain_bwd.py::test_direct_weight_gradient_writes_equal_the_reduced_ones"),),
    "B3": (_NONE,), "B16": (_NONE,), "fp32": (_NONE,), "fp16": (_NONE,), "fp16_tuned": (_NONE,), "dropout": (_NONE,), "eval": (_NONE,),
    "attached_zero": (_rel("bits", "bits", _ZERO_SRC),),
    "accumulate": (_rel("bits", "twice", _TWICE_SRC),),
    "held_attached": (_rel("bits", "bits", _HELD_SRC + "; " + _ZERO_SRC),),
    "held_accumulate": (_rel("bits", "twice", _HELD_SRC + "; " + _TWICE_SRC),),
    "held_attached_own": (_rel("bits", "bits", _HELD_SRC + "; " + _ZERO_SRC),),
    "no_table": (_rel("bits", "bits", _TABLE_SRC),),
    "no_table_perop": (_rel("rounding", "rounding", _ROUND_SRC), _rel("bits", "bits", _TABLE_SRC, "both_off")),
}

# ------------------------------------------------------------------------------------------------ SwinV2
SWIN_MODEL = "sw3"          # tests/test_swin.py CASES: img 128, depths (2, 2, 2), heads (3, 6, 12) -- the smallest it builds
SWIN_ATTR_DEFAULTS = {"group_dw_backward": False, "hold_reductions": True, "drop_path_p": 0.0}
SWIN_MODES = [
    _mode("default", B=2),
    _mode("grouped_held", attrs={"group_dw_backward": True, "hold_reductions": True}, B=2),
    _mode("grouped", attrs={"group_dw_backward": True, "hold_reductions": False}, B=2),
    _mode("fp16", dtype="fp16", B=2, loss_scale=256.0),
    _mode("fp16_tuned", {"f16_tuned": 1}, dtype="fp16", B=2, loss_scale=256.0),
    _mode("fp32", dtype="fp32", B=2),
    _mode("eval", kind="eval", B=2),
    _mode("attached_zero", grads="own", B=2),          # (SwinV2's gradients are ordinary tensors: there is no flat buffer to alias)
    _mode("accumulate", kind="accumulate", B=2),
    _mode("drop_path", attrs={"drop_path_p": 0.2}, B=2, seed=4321),
    _mode("B3", B=3),
]
_BRACKET_SRC = ("tests/test_swin.py::test_backward_wide_weight_gradient_bracket_equals_per_linear_launches "
                "(logits the same bits, gradients 2e-5 of the tensor's scale)")
_SWIN_NONE = _rel("none", "none", "values pinned by tests/test_swin.py, test_swin_fp16_model.py")
SWIN_RELATION = {
    "default": (_rel("bits", "bits", "tests/test_swin.py::test_swin_step_is_bit_reproducible"),),
    "grouped_held": (_rel("bits", "bracket", _BRACKET_SRC),),
    "grouped": (_rel("bits", "bracket", _BRACKET_SRC),),
    "fp16": (_SWIN_NONE,), "fp16_tuned": (_SWIN_NONE,), "fp32": (_SWIN_NONE,), "eval": (_SWIN_NONE,), "drop_path": (_SWIN_NONE,),
    "B3": (_SWIN_NONE,),
    "attached_zero": (_rel("bits", "bits", "0 + g is exact in fp32; tests/test_swin.py::test_swin_step_is_bit_reproducible"),),
    "accumulate": (_rel("bits", "twice", "g + g is exact in fp32; tests/test_swin.py::test_swin_step_is_bit_reproducible"),),
}

# bars of the relation kinds: (absolute logits bar | None, gradient bar, how the gradient difference is measured)
BARS = {"regroup": 1e-5, "bracket": 2e-5, "rounding_logits": 2e-2, "rounding_grads": 5e-2}


# ------------------------------------------------------------------------------------------------ histories
def pairs_walk(names):
    """A closed walk over `names` in which every ordered pair of distinct names occurs as consecutive steps exactly once: an
    Euler circuit of the complete directed graph (every vertex has n - 1 edges in and out), by Hierholzer's algorithm with the
    edges of each vertex taken in list order.  n (n - 1) + 1 steps, the same list on every call."""
    names = list(names)
    nxt = {a: [b for b in names if b != a] for a in names}
    stack, walk = [names[0]], []
    while stack:
        v = stack[-1]
        if nxt[v]:
            stack.append(nxt[v].pop(0))
        else:
            walk.append(stack.pop())
    return walk[::-1]


def chunks(history, size):
    """The history cut into pieces of at most `size` steps; each piece starts with the last step of the one before it, so no
    consecutive pair is lost at a cut."""
    out, i = [], 0
    while i < len(history) - 1:
        out.append(history[i:i + size])
        i += size - 1
    return out


def by_name(modes):
    return {m.name: m for m in modes}


def vit_pairs_history():
    return pairs_walk([m.name for m in VIT_MODES])


def vit_classcount_history():
    return pairs_walk(list(VIT_CLASSCOUNT_MODES))


def swin_pairs_history():
    return pairs_walk([m.name for m in SWIN_MODES])


VIT_CHUNK = 64
SWIN_CHUNK = 28
