"""CPU checks of SwinV2's fp16 compute mode: the gfx950 code of the window-attention file really issues the fp16 MFMA next to the
bf16 one, and no Swin kernel rounds toward zero or flushes fp16 subnormals."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rgb-no-more_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC) and shutil.which("hipcc") is None,
                                reason="needs hipcc (cross-compiles, no GPU)")


def _isa(tmp_path, name):
    hipcc = HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")
    out = str(tmp_path / (name + ".s"))
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=fast", "-S", "--cuda-device-only",
                    os.path.join(CSRC, name + ".hip"), "-o", out], check=True, capture_output=True)
    return open(out).read()


def _modes(s):
    modes = re.findall(r"\.amdhsa_float_denorm_mode_16_64\s+(\d+)", s)
    assert modes and set(modes) == {"3"}                  # fp16 subnormals kept in every kernel
    rounds = re.findall(r"\.amdhsa_float_round_mode_16_64\s+(\d+)", s)
    assert rounds and set(rounds) == {"0"}                # round to nearest even
    assert "v_cvt_pkrtz" not in s                         # no round-toward-zero packing


def test_window_attention_issues_the_fp16_mfma(tmp_path):
    s = _isa(tmp_path, "swin_attn")
    assert "v_mfma_f32_32x32x16_f16" in s
    assert "v_mfma_f32_32x32x16_bf16" in s
    kernels = re.findall(r"\.amdhsa_kernel (\S+)", s)
    assert any("win_attn_fwd_kernelIDF16_" in k for k in kernels) and any("win_attn_bwd_kernelIDF16_" in k for k in kernels)
    _modes(s)


def test_swin_kernels_have_fp16_instances(tmp_path):
    s = _isa(tmp_path, "swin")
    kernels = re.findall(r"\.amdhsa_kernel (\S+)", s)
    for stem in ("swin_embed_kernelIDF16_", "swin_embed_kernelIfDF16_", "ln_rows_fwd_kernelIDF16_", "ln_rows_bwd_kernelIDF16_",
                 "ln_generic_fwd_kernelIDF16_", "ln_generic_bwd_kernelIDF16_", "merge_gather_kernelIDF16_",
                 "token_mean_fwd_kernelIDF16_", "token_mean_bwd_kernelIDF16_", "token_mean_fwd_scalar_kernelIDF16_",
                 "token_mean_bwd_scalar_kernelIDF16_"):
        assert any(stem in k for k in kernels), stem
    _modes(s)
