"""CPU checks of the fp16 compute mode's boundary: the header and the binding agree on the dtype code, the binding maps
torch.float16 to it, and the gfx950 code of the GEMM file really issues the fp16 MFMA."""
import os
import re
import shutil
import subprocess

import pytest
import torch

from rgb_no_more_amd import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rgb-no-more_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_header_dtype_code_matches_binding():
    txt = open(os.path.join(ROOT, "include", "rgbnm.h")).read()
    m = re.search(r"#define\s+RGBNM_DT_F16\s+(\d+)", txt)
    assert m, "include/rgbnm.h does not define RGBNM_DT_F16"
    assert int(m.group(1)) == L.DT_F16 == 2
    assert (L.DT_F32, L.DT_BF16) == (0, 1)
    assert re.search(r"#define\s+RGBNM_ABI_VERSION\s+3\b", txt)


def test_dt_of_float16():
    assert L.dt_of(torch.float16) == L.DT_F16
    assert L.dt_of(torch.bfloat16) == L.DT_BF16 and L.dt_of(torch.float32) == L.DT_F32
    with pytest.raises(TypeError):
        L.dt_of(torch.float64)


@pytest.mark.skipif(not os.path.exists(HIPCC) and shutil.which("hipcc") is None, reason="needs hipcc (cross-compiles, no GPU)")
def test_gemm_code_object_issues_the_fp16_mfma(tmp_path):
    hipcc = HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")
    out = str(tmp_path / "gemm.s")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=fast", "-S", "--cuda-device-only",
                    os.path.join(CSRC, "gemm.hip"), "-o", out], check=True, capture_output=True)
    s = open(out).read()
    assert "v_mfma_f32_32x32x16_f16" in s
    assert "v_mfma_f32_32x32x16_bf16" in s
    # round to nearest even (no round-toward-zero packing) and fp16 subnormals kept in every kernel
    assert "v_cvt_pkrtz" not in s
    modes = re.findall(r"\.amdhsa_float_denorm_mode_16_64\s+(\d+)", s)
    assert modes and set(modes) == {"3"}
    rounds = re.findall(r"\.amdhsa_float_round_mode_16_64\s+(\d+)", s)
    assert rounds and set(rounds) == {"0"}
