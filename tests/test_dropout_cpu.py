"""CPU checks of the dropout feature (rgbnm.h, dropout mask contract): the numpy Philox of tests/dropout_ref.py against the
Random123 known-answer vectors, the header and binding surface, and the ViT switch's default."""
import os
import re

import numpy as np

import dropout_ref as D
import rgb_no_more_amd as rg
from rgb_no_more_amd import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _hex(ws):
    return " ".join(f"{int(np.asarray(w).reshape(-1)[0]):08x}" for w in ws)


def test_philox_known_answer_vectors():
    # Random123 kat_vectors, philox4x32 with 10 rounds: (counter, key) -> output
    assert _hex(D.philox4x32_10(0, 0, 0, 0, 0, 0)) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"
    f = 0xFFFFFFFF
    assert _hex(D.philox4x32_10(f, f, f, f, f, f)) == "408f276d 41c83b0e a20bc7c6 6d5451fd"
    assert _hex(D.philox4x32_10(0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344, 0xA4093822, 0x299F31D0)) == \
        "d16cfe09 94fdcceb 5001e420 24126ea1"


def test_mask_layout_and_threshold():
    # word (col & 3) of counter (col >> 2, row, 4 block + site, 0); key = the seed's low / high halves
    seed = 0x0123456789ABCDEF
    w = D.words(seed, 1, 3, 5, 11)
    for r in (0, 4):
        for c in (0, 5, 10):
            ref = D.philox4x32_10(c >> 2, r, 4 * 3 + 1, 0, 0x89ABCDEF, 0x01234567)
            assert w[r, c] == ref[c & 3]
    assert D.threshold(0.0) == (0, np.float32(1.0))
    thr, scale = D.threshold(0.1)
    assert thr == round(float(np.float32(0.1)) * 2 ** 32) and scale == np.float32(1) / np.float32(0.9)
    k = D.keep(seed, 0.5, 0, 0, 256, 256)
    assert abs(k.mean() - 0.5) < 0.01


def test_header_declares_dropout_entries():
    h = open(os.path.join(ROOT, "include", "rgbnm.h")).read()
    assert "#define RGBNM_EPI_RES_DROP 7" in h and "#define RGBNM_EPI_GELU_DROP 8" in h
    for name in ("rgbnm_gemm_nt_drop", "rgbnm_dropout_apply", "rgbnm_vit_block_fwd_drop", "rgbnm_vit_block_bwd_drop"):
        assert re.search(r"\b" + name + r"\s*\(", h), name
        assert name in L.PROTOTYPES
    assert "typedef struct rgbnm_dropout" in h
    assert [f for f, _ in L.Dropout._fields_] == ["seed", "p", "block", "dy_m", "dxmid_m"]
    assert (L.EPI_RES_DROP, L.EPI_GELU_DROP) == (7, 8)
    assert L.ABI_VERSION == 3


def test_train_dropout_defaults_off():
    assert rg.ViT.train_dropout is False
    m = rg.ViT(3, 16, 192, depth=1, n_classes=16, num_heads=3, head_size=64, pixel_space="DCT", ver=1)
    assert m.drop_p == 0.1 and m.train_dropout is False and m.last_dropout_seed is None
