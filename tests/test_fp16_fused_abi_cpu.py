"""CPU checks of fp16 on the per-block fused kernels (option f16_tuned = 2): attention v2, the fused MLP and the row-panel GEMM with
its LayerNorm epilogues each carry both the fp16 and the bf16 MFMA in their gfx950 code, convert with round-to-nearest-even and keep
fp16 subnormals in every kernel; the fused MLP forward has an fp16 twin of the arithmetic kernel only (the GELU table is a bf16
image); the option takes level 2 and is off by default.  The assertions of tests/test_fp16_tuned_abi_cpu.py on three more files."""
import os
import re
import shutil
import subprocess

import pytest

from rgb_no_more_amd import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rgb-no-more_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FILES = ["attention_v2.hip", "mlp_fused.hip", "gemm_nt_kpipe.hip"]
# element type inside a mangled kernel name: _Float16 is DF16_, __bf16 is DF16b
F16_ARG, BF16_ARG = "DF16_", "DF16b"


def kernel_names(s):
    return re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", s, re.M)


@pytest.mark.skipif(not os.path.exists(HIPCC) and shutil.which("hipcc") is None, reason="needs hipcc (cross-compiles, no GPU)")
@pytest.mark.parametrize("fname", FILES)
def test_fused_code_objects_issue_both_mfmas(tmp_path, fname):
    hipcc = HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")
    out = str(tmp_path / (fname + ".s"))
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=fast", "-S", "--cuda-device-only",
                    os.path.join(CSRC, fname), "-o", out], check=True, capture_output=True)
    s = open(out).read()
    assert "v_mfma_f32_32x32x16_f16" in s
    assert "v_mfma_f32_32x32x16_bf16" in s
    # round to nearest even (no round-toward-zero packing) and fp16 subnormals kept in every kernel
    assert "v_cvt_pkrtz" not in s
    names = kernel_names(s)
    nkern = len(names)
    modes = re.findall(r"\.amdhsa_float_denorm_mode_16_64\s+(\d+)", s)
    assert nkern and len(modes) == nkern and set(modes) == {"3"}
    rounds = re.findall(r"\.amdhsa_float_round_mode_16_64\s+(\d+)", s)
    assert len(rounds) == nkern and set(rounds) == {"0"}
    rounds32 = re.findall(r"\.amdhsa_float_round_mode_32\s+(\d+)", s)
    assert len(rounds32) == nkern and set(rounds32) == {"0"}
    if fname == "attention_v2.hip":
        # every kernel of the file has its fp16 twin
        for k in ("attn2_fwd_kernel", "attn2_bwd_kernel", "attn3_fwd_kernel", "attn3_bwd_kernel"):
            mine = [n for n in names if k in n]
            assert mine and sum(F16_ARG in n for n in mine) == sum(BF16_ARG in n for n in mine), mine
    if fname == "gemm_nt_kpipe.hip":
        # the LayerNorm epilogues included: as many fp16 as bf16 instantiations of the 7-wave kernel
        kp7 = [n for n in names if "kp7" in n and "gemm_nt_kpipe_kernel" in n]
        assert kp7 and sum(F16_ARG in n for n in kp7) == sum(BF16_ARG in n for n in kp7), kp7
    if fname == "mlp_fused.hip":
        fwd = [n for n in names if "mlp_fwd_kernel" in n]
        arith = [n for n in fwd if "ILb0E" in n]          # mlp_fwd_kernel<false, T>: the arithmetic GELU
        table = [n for n in fwd if "ILb1E" in n]          # mlp_fwd_kernel<true, T>: the GELU table
        assert len(arith) + len(table) == len(fwd) and arith and table, fwd
        # (the bf16 kernels name no element type: mlp_fwd_kernel<false> / <true>; the fp16 twin is mlp_fwd_kernel<false, _Float16>)
        assert sum(F16_ARG in n for n in arith) == sum(F16_ARG not in n for n in arith) >= 1, arith
        assert not any(F16_ARG in n for n in table), table          # there is no fp16 table kernel
        bwd = [n for n in names if "mlp_bwd_kernel" in n]
        assert sum(F16_ARG in n for n in bwd) == sum(BF16_ARG in n for n in bwd) >= 1, bwd


def test_f16_tuned_takes_level_2_and_is_off_by_default():
    """(every test that sets the option restores it: what this process's library holds is the library's default)"""
    lib = L.lib()
    assert lib.rgbnm_get_option(b"f16_tuned") == 0
    try:
        assert lib.rgbnm_set_option(b"f16_tuned", 2) == 0
        assert lib.rgbnm_get_option(b"f16_tuned") == 2
        L.set_option("f16_tuned", 1)
        assert L.get_option("f16_tuned") == 1
        L.set_option("f16_tuned", 2)
        assert L.get_option("f16_tuned") == 2
    finally:
        lib.rgbnm_set_option(b"f16_tuned", 0)
    assert L.get_option("f16_tuned") == 0
    assert "level" in (L.set_option.__doc__ or "") or "levels" in (L.set_option.__doc__ or "")
