"""CPU checks of the fp16 route through the tuned GEMM kernels (option f16_tuned): each of the four kernel files carries both the
fp16 and the bf16 MFMA in its gfx950 code, converts with round-to-nearest-even and keeps fp16 subnormals in every kernel, and the
library has the option, off by default."""
import os
import re
import shutil
import subprocess

import pytest

from rgb_no_more_amd import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rgb-no-more_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FILES = ["gemm_nt_small.hip", "gemm_nt_wres.hip", "gemm_nt_kpipe.hip", "gemm_tn_pipe.hip"]


@pytest.mark.skipif(not os.path.exists(HIPCC) and shutil.which("hipcc") is None, reason="needs hipcc (cross-compiles, no GPU)")
@pytest.mark.parametrize("fname", FILES)
def test_tuned_gemm_code_objects_issue_both_mfmas(tmp_path, fname):
    hipcc = HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")
    out = str(tmp_path / (fname + ".s"))
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=fast", "-S", "--cuda-device-only",
                    os.path.join(CSRC, fname), "-o", out], check=True, capture_output=True)
    s = open(out).read()
    assert "v_mfma_f32_32x32x16_f16" in s
    assert "v_mfma_f32_32x32x16_bf16" in s
    # round to nearest even (no round-toward-zero packing) and fp16 subnormals kept in every kernel
    assert "v_cvt_pkrtz" not in s
    nkern = len(re.findall(r"^\s*\.amdhsa_kernel\s", s, re.M))
    modes = re.findall(r"\.amdhsa_float_denorm_mode_16_64\s+(\d+)", s)
    assert nkern and len(modes) == nkern and set(modes) == {"3"}
    rounds = re.findall(r"\.amdhsa_float_round_mode_16_64\s+(\d+)", s)
    assert len(rounds) == nkern and set(rounds) == {"0"}
    rounds32 = re.findall(r"\.amdhsa_float_round_mode_32\s+(\d+)", s)
    assert len(rounds32) == nkern and set(rounds32) == {"0"}


def test_f16_tuned_option_exists_and_is_off_by_default():
    """(every test that sets the option restores it: what this process's library holds is the library's default)"""
    lib = L.lib()
    assert lib.rgbnm_get_option(b"f16_tuned") == 0
    try:
        assert lib.rgbnm_set_option(b"f16_tuned", 1) == 0
        assert lib.rgbnm_get_option(b"f16_tuned") == 1
        L.set_option("f16_tuned", 0)
        assert L.get_option("f16_tuned") == 0
        L.set_option("f16_tuned", 1)
        assert L.get_option("f16_tuned") == 1
    finally:
        lib.rgbnm_set_option(b"f16_tuned", 0)
    assert L.get_option("no_such_option") == -1
    with pytest.raises(L.RgbnmError):
        L.set_option("no_such_option", 1)
