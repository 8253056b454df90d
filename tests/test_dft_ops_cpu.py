"""CPU-only checks of the batched DFT-plane path (csrc/dft_ops.hip): the composed gather map that the kernels resample with, the
C ABI's declarations, and that the fused transform still refuses the three ops without its opt-in."""
import os
import re

import numpy as np
import pytest
import torch

import rgb_no_more_amd as rg
from rgb_no_more_amd import custom_transforms as CT
from rgb_no_more_amd import dct_ops as DO
from rgb_no_more_amd import lib as L
from oracle import dft_np as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MATRICES = [("rotate 9", DO.rotate_plan(9.0)[1], D.tv_inverse_affine_matrix([0.0, 0.0], 9.0, [0.0, 0.0], 1.0, [0.0, 0.0])),
            ("rotate -27", DO.rotate_plan(-27.0)[1], D.tv_inverse_affine_matrix([0.0, 0.0], -27.0, [0.0, 0.0], 1.0, [0.0, 0.0])),
            ("shear-x 5.1", DO.shear_plan(deg_x=5.1)[1], D.tv_inverse_affine_matrix([0.0, 0.0], 0.0, [0.0, 0.0], 1.0, [5.1, 0.0])),
            ("shear-y -17", DO.shear_plan(deg_y=-17.0)[1], D.tv_inverse_affine_matrix([0.0, 0.0], 0.0, [0.0, 0.0], 1.0, [0.0, -17.0]))]


@pytest.mark.parametrize("N", [16, 40, 312])
@pytest.mark.parametrize("case", MATRICES, ids=[m[0] for m in MATRICES])
def test_gather_map_is_shift_sample_unshift_of_the_oracle(case, N):
    """G = F.flat[map] (0 where map == -1) equals ifftshift(tv_grid_sample_nearest(fftshift(F))) of oracle/dft_np.py, exactly: it is
    a gather.  (rotate_plan's matrix is the oracle's: rotate_block hands tv_rotate -left, which negates it again.)"""
    _, matrix, oracle_matrix = case
    assert list(matrix) == list(oracle_matrix)
    rng = np.random.default_rng(N)
    F = (rng.standard_normal((1, N, N)) + 1j * rng.standard_normal((1, N, N))).astype(np.complex64)
    m = DO.dft_gather_map(matrix, N, "cpu")
    assert m.dtype == torch.int32 and tuple(m.shape) == (N, N) and int(m.min()) >= -1 and int(m.max()) < N * N
    m = m.numpy().reshape(-1)
    got = np.where(m >= 0, F.reshape(-1)[np.clip(m, 0, None)], 0).reshape(1, N, N)
    sh = np.fft.fftshift(F, axes=(-2, -1))
    grid = D.tv_affine_grid(oracle_matrix, N, N)
    res = D.tv_grid_sample_nearest(sh.real.astype(np.float32), grid) + 1j * D.tv_grid_sample_nearest(sh.imag.astype(np.float32), grid)
    ref = np.fft.ifftshift(res.astype(np.complex64), axes=(-2, -1))
    assert np.array_equal(got, ref)
    assert (m < 0).any() or "rotate" not in case[0]            # a rotation leaves corners empty: the zero mask is exercised


def test_gather_map_cache_is_bounded_and_keyed():
    a = DO.dft_gather_map(DO.rotate_plan(9.0)[1], 16, "cpu")
    assert DO.dft_gather_map(DO.rotate_plan(9.0)[1], 16, "cpu") is a
    assert DO.dft_gather_map(DO.rotate_plan(9.0)[1], 24, "cpu") is not a
    for k in range(40):
        DO.dft_gather_map(DO.rotate_plan(1.0 + 0.5 * k)[1], 8, "cpu")
    assert len(DO._GATHER_MAPS) <= DO._GATHER_MAPS_MAX == 32
    assert torch.equal(DO.dft_gather_map(DO.rotate_plan(9.0)[1], 16, "cpu"), a)         # rebuilt after eviction: the same map


def test_identity_map_and_plans():
    m = DO.dft_gather_map(DO.shear_plan(0.0, 0.0)[1], 24, "cpu")
    assert torch.equal(m.reshape(-1), torch.arange(24 * 24, dtype=torch.int32))
    assert [DO.rotate_plan(d)[0] for d in (0.0, 90.0, -90.0, 180.0, 270.0, 9.0, 30.0, -100.0)] == [0, 1, 3, 2, 3, 0, 0, 3]
    assert DO.padded_blocks(28, 2 ** 0.5) == 39 and DO.padded_blocks(14, 2 ** 0.5) == 19 and DO.padded_blocks(10, False) == 10


def test_tensor_path_keeps_its_bits_on_the_cpu():
    """_dft_plane_op's resampling now shares its index math with the map: the map applied by hand gives the tensor path's bits."""
    rng = np.random.default_rng(3)
    x = torch.from_numpy(rng.integers(-300, 300, size=(2, 5, 5, 8, 8)).astype(np.int16))
    for deg in (9.0, -100.0):
        rot, matrix = DO.rotate_plan(deg)
        ref = DO.rotate_block(x, deg, pad=2 ** 0.5)
        Hp = DO.padded_blocks(5, 2 ** 0.5)
        pad = torch.zeros(2, Hp, Hp, 8, 8, dtype=torch.int16)
        pad[:, 1:6, 1:6] = x
        comp, Lm, Mm = DO.combine_blocks_dft(DO.blockshift(DO.rotate_dct_90deg(pad, rot)))
        m = DO.dft_gather_map(matrix, 8 * Hp, "cpu").reshape(-1).long()
        G = torch.where(m >= 0, comp.reshape(2, -1)[:, m.clamp(min=0)], torch.zeros((), dtype=comp.dtype)).reshape(comp.shape)
        dec = DO.iblockshift(DO.decompose_block_dft(G, Hp, Hp, 8, 8, Lm, Mm))[:, 1:6, 1:6]
        assert torch.equal(torch.round(dec).to(torch.int16), ref)


def test_header_declares_the_entries_and_abi_stays_3():
    txt = open(os.path.join(ROOT, "include", "rgbnm.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert re.search(r"#define\s+RGBNM_ABI_VERSION\s+3\b", code)
    assert re.search(r"typedef\s+struct\s+rgbnm_dft_job\s*\{\s*int\s+sample;\s*int\s+rot90s;\s*int\s+map_y;\s*int\s+map_c;\s*\}\s*rgbnm_dft_job;",
                     code)
    assert re.search(r"size_t\s+rgbnm_dct_dft_workspace\s*\(\s*int\s+njobs,\s*int\s+Hp_y,\s*int\s+Hp_c\s*\)", code)
    assert re.search(r"int\s+rgbnm_dct_dft_ops\s*\(\s*int16_t\*\s*Y,\s*int16_t\*\s*C,", code)
    assert "rgbnm_dct_dft_workspace" in L.PROTOTYPES and "rgbnm_dct_dft_ops" in L.PROTOTYPES
    assert len(L.PROTOTYPES["rgbnm_dct_dft_ops"][1]) == 18
    assert L.ABI_VERSION == 3 and L.lib().rgbnm_abi_version() == 3
    import ctypes
    assert ctypes.sizeof(L.DftJob) == 16
    # the workspace query: two complex N x N buffers per plane
    assert L.lib().rgbnm_dct_dft_workspace(3, 39, 19) == 3 * 4 * (312 * 312 + 2 * 152 * 152) * 4
    assert L.lib().rgbnm_dct_dft_workspace(0, 39, 19) == 0


def test_host_side_refusals_need_no_device():
    """Everything the entry refuses is decided on the host before a launch: with null buffers the refused calls return RGBNM_EINVAL
    (-1) and njobs == 0 returns 0, on a machine without a GPU."""
    f = L.lib().rgbnm_dct_dft_ops
    jobs = (L.DftJob * 1)()
    assert f(None, None, 4, 28, 39, 19, None, None, 0, None, None, None, None, 1, 0, None, 0, None) == 0
    assert f(None, None, 4, 27, 39, 19, None, None, 0, None, None, None, None, 1, 0, None, 0, None) == -1       # odd S
    assert f(None, None, 4, 34, 48, 24, None, None, 0, None, None, None, None, 1, 0, None, 0, None) == -1       # S out of range
    assert f(None, None, 4, 28, 27, 19, None, None, 0, None, None, None, None, 1, 0, None, 0, None) == -1       # Hp < Hb
    assert f(None, None, 4, 28, 49, 19, None, None, 0, None, None, None, None, 1, 0, None, 0, None) == -1       # Hp > 48
    assert f(None, None, 4, 28, 39, 19, None, None, -1, None, None, None, None, 1, 0, None, 0, None) == -1      # njobs < 0
    assert f(None, None, 4, 28, 39, 19, None, None, 0, None, None, None, None, 1, 2, None, 0, None) == -1       # clamp
    assert f(None, None, 4, 28, 39, 19, None, jobs, 0, None, None, None, None, 1, 0, None, 0, None) == -1       # one of the job arrays


def test_fused_transform_refuses_without_the_opt_in_and_accepts_with_it():
    with pytest.raises(NotImplementedError):
        CT.TrainTransform_DCT(size=28, ops_list=["Rotate"])
    with pytest.raises(NotImplementedError):
        CT.TrainTransform_DCT(size=28, ops_list=["Rotate"], dft_ops=False)
    t = CT.TrainTransform_DCT(size=28, ops_list=["Rotate", "ShearX", "ShearY", "Color"], dft_ops=True)
    torch.manual_seed(0)
    ps = t.sample_params(16, 64, 64)
    assert any(o[0] in CT.DFT_OPS for p in ps for o in p["ops"])
    with pytest.raises(NotImplementedError):
        CT.TrainTransform_DCT(size=28, ops_list=["Warp"], dft_ops=True)
    with pytest.raises(NotImplementedError, match="sample_params"):
        CT.FastParamSampler(t)
    assert CT.RandAugment_dct().dft_kernel is False and CT.RandAugment_dct(dft_kernel=True).dft_kernel is True
    assert rg.custom_transforms.REFERENCE_DEFAULT_OPS[3] == "Rotate"
