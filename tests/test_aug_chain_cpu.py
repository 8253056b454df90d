"""CPU-only checks around rgbnm_dct_augment_chain and rgbnm_mixup_any: header, library and binding agree; the chain sampler
keeps the reference's cumulative exclusion rule; sample() still makes the draws it made before the chain sampler existed;
pack_chain round-trips."""
import ctypes
import hashlib
import os
import re

import numpy as np
import pytest

from rgb_no_more_amd import custom_transforms as CT
from rgb_no_more_amd import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_vp = ctypes.c_void_p
CTYPE = {"const int16_t*": _vp, "const long long*": _vp, "const rgbnm_aug_params*": _vp, "const rgbnm_aug_op*": _vp,
         "const float*": _vp, "const void*": _vp, "void*": _vp, "int": ctypes.c_int, "size_t": ctypes.c_size_t,
         "long long": ctypes.c_longlong}


def header():
    txt = open(os.path.join(ROOT, "include", "rgbnm.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def header_args(name):
    m = re.search(r"\b(\w[\w ]*?)\s+" + name + r"\s*\(([^)]*)\)\s*;", header())
    assert m, name
    args = [re.sub(r"\s*\b\w+$", "", " ".join(a.split())).replace(" *", "*") for a in m.group(2).split(",")]
    return m.group(1).strip(), args


def test_header_library_and_binding_agree():
    dll = ctypes.CDLL(L.LIB_PATH)
    for name in ("rgbnm_dct_augment_chain", "rgbnm_mixup_any"):
        assert hasattr(dll, name), name
        ret, args = header_args(name)
        res, argtypes = L.PROTOTYPES[name]
        assert res is CTYPE[ret], (name, ret)
        assert [CTYPE[a] for a in args] == argtypes, (name, args)
    _, chain = header_args("rgbnm_dct_augment_chain")
    _, packed = header_args("rgbnm_dct_augment_packed")
    # the packed entry's arguments with the two ops arrays behind the parameters
    assert chain == packed[:7] + ["const rgbnm_aug_op*"] * 2 + packed[7:]
    assert header_args("rgbnm_mixup_any") == header_args("rgbnm_mixup")
    h = header()
    assert re.search(r"#define RGBNM_ABI_VERSION 3\b", h) and L.lib().rgbnm_abi_version() == L.ABI_VERSION == 3
    for name, val in (("RGBNM_AUG_MAX_OPS", 8), ("RGBNM_AUG_OUT_F32", 0), ("RGBNM_AUG_OUT_BF16", 1), ("RGBNM_AUG_OUT_I16", 2),
                      ("RGBNM_AUG_OUT_F16", 3), ("RGBNM_DT_F16", 2), ("RGBNM_DT_I16", 2)):
        assert re.search(r"#define %s %d\b" % (name, val), h), name
    assert (L.AUG_OUT_F32, L.AUG_OUT_BF16, L.AUG_OUT_I16, L.AUG_OUT_F16, L.AUG_MAX_OPS, CT.AUG_MAX_OPS) == (0, 1, 2, 3, 8, 8)
    m = re.search(r"typedef struct rgbnm_aug_op \{(.*?)\} rgbnm_aug_op;", h, flags=re.S)
    assert " ".join(m.group(1).split()) == "int op; float fmag; int iarg0, iarg1, iarg2;"
    assert CT.AUG_OP_DTYPE.itemsize == 20 == ctypes.sizeof(CT.AugOp)
    assert [CT.AUG_OP_DTYPE.fields[n][1] for n in CT.AUG_OP_DTYPE.names] == [getattr(CT.AugOp, n).offset for n, _ in CT.AugOp._fields_]
    assert CT.AUG_DTYPE.itemsize == ctypes.sizeof(CT.AugParams) == 60


def test_refusals_that_need_no_device():
    """Arguments the entries turn down before they look at the device (the rest: tests/test_augment_chain.py)."""
    lib = L.lib()
    P = 0x1000

    def chain(**kw):
        a = dict(Y=P, y_off=None, c_off=None, ops_dev=None, ops_host=None, out=3, size=28, B=1, nops=0)
        a.update(kw)
        return lib.rgbnm_dct_augment_chain(a["Y"], P, a["y_off"], a["c_off"], P, P, P, a["ops_dev"], a["ops_host"], P, None, P, P,
                                           a["out"], a["size"], a["B"], 28, 28, 14, 14, 1, a["nops"], P, 1 << 20, None)
    for kw in (dict(Y=None), dict(B=0), dict(size=30), dict(out=4), dict(out=-1), dict(nops=-1), dict(nops=3),
               dict(nops=9, ops_dev=P, ops_host=P), dict(ops_dev=P), dict(ops_host=P), dict(y_off=P), dict(c_off=P)):
        assert chain(**kw) == -1, kw
    for i, o in ((1, 0), (2, 0), (2, 1), (1, 2), (3, 2), (0, 3)):
        assert lib.rgbnm_mixup_any(i, o, P, P, P, 2, 8, None) == -1, (i, o)
    for i, o in ((0, 2), (2, 2), (0, 0)):
        assert lib.rgbnm_mixup_any(i, o, P, P, P, 2, 6, None) == -1 and lib.rgbnm_mixup_any(i, o, None, P, P, 2, 8, None) == -1


# digests of FastParamSampler.sample() taken on the commit before sample_chain() was written (num_ops = 2): sha256 over the bytes
# of sample(256, 60, 64) and sample(37, 28, 28) of one sampler, each followed by its nops
SAMPLE_DIGESTS = {0: "6997d9b561bafd4a8ebdec33821a309afc7dea2263665a4328921c93b2d2eaa6",
                  1: "3338e200bf27235f249af01c7c9ffab91b5f9037198606097cccc0e17d42b94d",
                  7: "9eb5738d2105855200b8a6ffa97f9b4a8766690ce42e732737ed46718264e492"}
SWIN_DIGEST = "6edf7fb2f2c1f9ac25b6b273b50d0f1300ef398241463086892e6ce84b8dc185"      # size 32, DEFAULT_OPS, magnitude 5, seed 3: sample(64, 64, 64)


def test_sample_makes_the_same_draws_for_two_ops():
    for seed, want in SAMPLE_DIGESTS.items():
        s = CT.FastParamSampler(CT.TrainTransform_DCT(size=28, num_ops=2, magnitude=3), seed=seed)
        h = hashlib.sha256()
        for B, H, W in ((256, 60, 64), (37, 28, 28)):
            out, nops = s.sample(B, H, W)
            assert out.dtype == CT.AUG_DTYPE and nops == 2
            h.update(out.tobytes())
            h.update(bytes([nops]))
        assert h.hexdigest() == want, seed
    t = CT.TrainTransform_DCT(size=32, num_ops=2, magnitude=5, ops_list=CT.DEFAULT_OPS)
    out, nops = CT.FastParamSampler(t, seed=3).sample(64, 64, 64)
    assert nops == 2 and hashlib.sha256(out.tobytes()).hexdigest() == SWIN_DIGEST


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_sample_chain_keeps_the_cumulative_exclusion_rule(seed):
    t = CT.TrainTransform_DCT(size=28, num_ops=5, magnitude=3)           # VITTI_OPS: all four chroma ops, Cutout, signed ops
    s = CT.FastParamSampler(t, seed=seed)
    packed, ops, nops = s.sample_chain(4096, 60, 64)
    assert nops == 5 and ops.shape == (4096, 5) and ops.dtype == CT.AUG_OP_DTYPE and packed.dtype == CT.AUG_DTYPE
    assert not packed["op"].any() and set(np.unique(packed["crop"][:, 2])) <= {14, 28, 56}
    ids = ops["op"]
    gray = CT.OPS["Grayscale"]
    chroma = np.isin(ids, [CT.OPS[n] for n in CT.CHROMA_OPS])
    is_gray = ids == gray
    seen_gray = np.cumsum(is_gray, axis=1) - is_gray > 0                 # Grayscale in an EARLIER slot
    other = chroma & ~is_gray
    seen_other = np.cumsum(other, axis=1) - other > 0                    # another chroma op in an earlier slot
    assert seen_gray.any() and seen_other.any()                          # the rule had something to exclude
    assert not (chroma & seen_gray).any(), "a CHROMA_OPS member after Grayscale"
    assert not (is_gray & seen_other).any(), "Grayscale after another chroma op"
    assert (other & seen_other).any()                                    # chroma ops other than Grayscale may repeat
    assert set(np.unique(ids)) == {CT.OPS[n] for n in CT.VITTI_OPS}      # every op of the list is drawn
    for k in range(nops):                                                # ... in every slot the rule leaves it
        assert len(np.unique(ids[:, k])) == len(CT.VITTI_OPS)
    # every signed op shows both signs, in the field its magnitude lives in
    meta = CT.magnitude_table(11, (28, 28))
    for name in CT.VITTI_OPS:
        if not meta[name][1]:
            continue
        m = ids == CT.OPS[name]
        if name in ("TranslateX", "TranslateY", "Rotate90"):
            assert (ops["iarg0"][m] > 0).any() and (ops["iarg0"][m] < 0).any(), name
        elif name == "MidfreqAug":
            assert len(np.unique(ops["iarg0"][m])) == 2, name            # two tables of the bank: +mag and -mag
        elif name == "Brightness":
            assert (ops["fmag"][m] > 0).any() and (ops["fmag"][m] < 0).any(), name
        else:                                                            # Color, Contrast: factor 1 + mag / 1 - mag
            assert (ops["fmag"][m] > 1).any() and (ops["fmag"][m] < 1).any(), name
    cut = ids == CT.OPS["Cutout"]
    for f in ("iarg1", "iarg2"):
        c = ops[f][cut]
        assert (c % 2 == 0).all() and c.min() >= 0 and c.max() < 28 and len(np.unique(c)) == 14
    drop = ids == CT.OPS["ChromaDrop"]
    assert set(np.unique(ops["iarg0"][drop])) == {0, 1}
    # an empty op list: no ops
    _, ops0, n0 = CT.FastParamSampler(CT.TrainTransform_DCT(num_ops=5, ops_list=[]), seed=seed).sample_chain(4, 60, 64)
    assert n0 == 0 and ops0.shape == (4, 0)


def test_pack_chain_round_trips_and_pack_still_refuses():
    t = CT.TrainTransform_DCT(size=28, num_ops=4)
    four = [("Posterize", 2.0, None), ("TranslateX", -3.75, None), ("Cutout", 1.8, (4, 6)), ("MidfreqAug", 0.27, None)]
    params = [dict(box=(2, 4, 56, 56), flip=True, ops=four), dict(box=(0, 6, 14, 14), flip=False, ops=four[2:3])]
    arr, ops, nops = t.pack_chain(params)
    assert nops == 4 and ops.shape == (2, 4) and ops.dtype == CT.AUG_OP_DTYPE and len(arr) == 2
    assert [(a.crop_i, a.crop_j, a.crop_h, a.crop_w, a.flip) for a in arr] == [(2, 4, 56, 56, 1), (0, 6, 14, 14, 0)]
    assert all(a.op[0] == a.op[1] == 0 for a in arr)
    f0 = t.bank.index("MidfreqAug", 0.27)
    assert [tuple(r) for r in ops[0].tolist()] == [(2, 0.0, 2, 511, 0), (9, 0.0, -4, 0, 0), (8, 0.0, 2, 4, 6), (7, 0.0, f0, 0, 0)]
    assert [tuple(r) for r in ops[1].tolist()] == [(8, 0.0, 2, 4, 6)] + [(0, 0.0, 0, 0, 0)] * 3         # padded with Identity
    # the records are what pack() writes into the parameters' two slots
    two, n2 = t.pack([dict(p, ops=p["ops"][:2]) for p in params])
    assert n2 == 2 and [(two[0].op[s], two[0].fmag[s], two[0].iarg0[s], two[0].iarg1[s], two[0].iarg2[s]) for s in (0, 1)] == \
        [tuple(r) for r in ops[0, :2].tolist()]
    with pytest.raises(ValueError):
        t.pack(params)
    with pytest.raises(ValueError):
        t.pack_chain([dict(box=(0, 0, 28, 28), flip=False, ops=four * 2 + four[:1])])
    assert t.pack_chain([dict(box=(0, 0, 28, 28), flip=False, ops=four * 2)])[2] == 8
