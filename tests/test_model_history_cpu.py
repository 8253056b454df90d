"""The case data of tests/test_model_history.py (tests/history_cases.py) keeps its coverage promises: every ordered pair of distinct
modes is taken as two consecutive steps, also after the history is cut into chunks; every mode has a relation that names where its
bar comes from; the histories are the same list on every call.  No GPU."""
import os
import re

import pytest

import history_cases as HC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {"vit": (HC.VIT_MODES, HC.vit_pairs_history, HC.VIT_RELATION, HC.VIT_CHUNK),
         "swin": (HC.SWIN_MODES, HC.swin_pairs_history, HC.SWIN_RELATION, HC.SWIN_CHUNK)}
KINDS = {"bits", "twice", "regroup", "bracket", "rounding", "none"}


def _pairs(seq):
    return set(zip(seq[:-1], seq[1:]))


@pytest.mark.parametrize("model", list(CASES))
def test_every_ordered_pair_of_modes_is_taken_consecutively(model):
    modes, history, _, chunk = CASES[model]
    names = [m.name for m in modes]
    assert len(set(names)) == len(names)
    want = {(a, b) for a in names for b in names if a != b}
    walk = history()
    assert set(walk) == set(names)
    assert want <= _pairs(walk)
    assert len(walk) == len(names) * (len(names) - 1) + 1            # an Euler circuit: no pair twice
    # ... and no pair is lost where the walk is cut into the chunks the GPU test runs (each on a fresh model)
    parts = HC.chunks(walk, chunk)
    assert all(2 <= len(p) <= chunk for p in parts)
    got = set()
    for p in parts:
        got |= _pairs(p)
    assert want <= got
    assert sum(len(p) - 1 for p in parts) == len(walk) - 1


def test_classcount_history_covers_its_modes():
    names = list(HC.VIT_CLASSCOUNT_MODES)
    assert set(names) <= {m.name for m in HC.VIT_MODES}
    assert names == ["default", "both_off", "held", "attached_zero", "accumulate", "eval", "fp32"]
    walk = HC.vit_classcount_history()
    assert {(a, b) for a in names for b in names if a != b} <= _pairs(walk)


def test_the_modes_the_issue_names_are_there():
    vit = {m.name for m in HC.VIT_MODES}
    assert {"default", "fwd_off", "bwd_off", "both_off", "bwd_off_late", "per_block_nodes", "held", "held_perop", "tn_direct_off", "B3",
            "B16", "fp32", "fp16", "fp16_tuned", "dropout", "eval", "attached_zero", "accumulate", "held_attached", "held_accumulate",
            "no_table"} <= vit
    m = HC.by_name(HC.VIT_MODES)
    assert m["default"].dtype == "bf16" and m["default"].B == 4 and not m["default"].options and not m["default"].attrs
    assert m["bwd_off_late"].late == {"bwd_chain": 0} and not m["bwd_off_late"].options
    assert m["B3"].B == 3 and m["B16"].B == 16 and (16 * 196) % 64 == 0 and (3 * 196) % 64 != 0
    assert m["dropout"].seed is not None and m["dropout"].attrs == {"drop_p": 0.1, "train_dropout": True}
    assert m["held_attached"].grads == "flat" and m["held_attached"].attrs == {"defer_grad_reduction": True}
    assert m["held_accumulate"].kind == "accumulate" and m["held_perop"].options == {"fwd_chain": 0, "bwd_chain": 0}
    assert m["fp16_tuned"].options == {"f16_tuned": 1} and m["fp16_tuned"].dtype == "fp16" and m["no_table"].options == {"gelu_table": 0}
    sw = HC.by_name(HC.SWIN_MODES)
    assert sw["grouped_held"].attrs == {"group_dw_backward": True, "hold_reductions": True}
    assert sw["grouped"].attrs == {"group_dw_backward": True, "hold_reductions": False}
    assert {"default", "fp16", "fp16_tuned", "fp32", "eval", "attached_zero", "accumulate", "drop_path"} <= set(sw)
    assert sw["drop_path"].seed is not None and len({x.B for x in HC.SWIN_MODES}) == 2
    for x in HC.VIT_MODES + HC.SWIN_MODES:
        assert set(x.options) | set(x.late) <= set(HC.OPTION_DEFAULTS), x.name
        assert x.kind in ("train", "accumulate", "eval") and x.grads in ("none", "flat", "own") and x.dtype in ("bf16", "fp16", "fp32")
    assert all(set(x.attrs) <= set(HC.VIT_ATTR_DEFAULTS) for x in HC.VIT_MODES)
    assert all(set(x.attrs) <= set(HC.SWIN_ATTR_DEFAULTS) for x in HC.SWIN_MODES)


def test_option_defaults_are_the_librarys():
    """OPTION_DEFAULTS is what every step puts back: it must be the option table of the library source."""
    src = open(os.path.join(ROOT, "rgb-no-more_amd", "csrc", "vit.hip")).read()
    table = dict((k, int(v)) for k, v in re.findall(r'\{"(\w+)", (\d+)\}', src[src.index("Opt g_opts[]"):].split(";")[0]))
    for k, v in HC.OPTION_DEFAULTS.items():
        assert table[k] == v, k


@pytest.mark.parametrize("model", list(CASES))
def test_every_mode_has_a_relation_with_a_source(model):
    modes, _, relation, _ = CASES[model]
    names = {m.name for m in modes}
    assert set(relation) == names
    for name, rels in relation.items():
        assert rels and rels[0].against == "default", name
        for r in rels:
            assert r.logits in KINDS and r.grads in KINDS and r.against in names and (r.against != name or name == "default")
            # the bar's origin: an existing test file or header of this repository, named in a plain string
            files = re.findall(r"(tests/\w+\.py|include/\w+\.h)", r.source)
            assert files, (name, r.source)
            for f in files:
                assert os.path.exists(os.path.join(ROOT, f)), (name, f)
            for f, t in re.findall(r"(tests/\w+\.py)::(\w+)", r.source):
                assert re.search(rf"^def {t}\(", open(os.path.join(ROOT, f)).read(), re.M), (name, f, t)
    # the relations the issue fixes
    if model == "vit":
        for n in ("held", "attached_zero", "held_attached", "tn_direct_off"):
            assert (relation[n][0].logits, relation[n][0].grads) == ("bits", "bits"), n
        for n in ("accumulate", "held_accumulate"):
            assert relation[n][0].grads == "twice", n
        for n in ("bwd_off", "bwd_off_late", "per_block_nodes"):
            assert relation[n][0].grads == "regroup", n
        assert relation["per_block_nodes"][0].logits == "bits"
        for n in ("fwd_off", "both_off", "held_perop"):
            assert (relation[n][0].logits, relation[n][0].grads) == ("rounding", "rounding"), n
        for n in ("B3", "B16", "fp32", "fp16", "fp16_tuned", "dropout", "eval"):
            assert relation[n][0].grads == "none", n
    else:
        assert relation["attached_zero"][0].grads == "bits" and relation["accumulate"][0].grads == "twice"
        assert relation["grouped"][0].logits == "bits" and relation["grouped"][0].grads == "bracket"
    assert HC.BARS == {"regroup": 1e-5, "bracket": 2e-5, "rounding_logits": 2e-2, "rounding_grads": 5e-2}


def test_histories_are_deterministic():
    for f in (HC.vit_pairs_history, HC.vit_classcount_history, HC.swin_pairs_history):
        assert f() == f()
    assert HC.pairs_walk(["a", "b", "c"]) == HC.pairs_walk(["a", "b", "c"])
    assert _pairs(HC.pairs_walk(["a", "b", "c"])) == {(a, b) for a in "abc" for b in "abc" if a != b}
