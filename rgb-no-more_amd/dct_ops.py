"""Host-side mirror of the reference's `utils/dct_ops.py` surface for the north-star path.

Constant-table generators (DCT basis / conversion matrices / Gaussian windows) are tiny host
computations done once and handed to the HIP kernels; the per-coefficient work is in csrc/*.hip
(see custom_transforms.py for the batched device transforms).
"""
import math

import torch


def generate_basis_matrix(length=8, scale=True, dtype=torch.float32, device="cpu"):
    """Orthonormal DCT-II basis D[u, x] = c(u) sqrt(2/L) cos(pi/L * u * (x + 1/2)).
    Reference: utils/dct_ops.py:150-169 (same evaluation order, in `dtype`)."""
    u = torch.arange(length, dtype=dtype, device=device).unsqueeze(1)
    x = torch.arange(length, dtype=dtype, device=device).unsqueeze(0) + 0.5
    basis = (u.mm(x) * torch.pi / length).cos()
    if scale:
        basis[0] *= 1 / (2 ** 0.5)
        basis *= (2 / length) ** 0.5
    return basis


def generate_conversion_matrix(length_small=2, mult=2, scale=True, dtype=torch.float32, device="cpu"):
    """A = D_{small*mult} . blockdiag(D_small, ..., D_small)^T  (orthonormal).
    Reference: utils/dct_ops.py:180-208.  A.X.A^T merges mult x mult small DCT blocks into one large one."""
    if mult == 1:
        return torch.eye(length_small, dtype=dtype, device=device)
    big = generate_basis_matrix(length_small * mult, scale=scale, dtype=dtype, device=device)
    small = generate_basis_matrix(length_small, scale=scale, dtype=dtype, device=device)
    blocks = torch.block_diag(*([small] * mult))
    inv = blocks.T if scale else torch.linalg.inv(blocks)
    return big.mm(inv)


_CONV = {}


def _conv(length_small, mult, device):
    key = (length_small, mult, str(device))
    if key not in _CONV:          # built on the host like the reference builds it (same evaluation order), then moved
        _CONV[key] = generate_conversion_matrix(length_small, mult, scale=True, dtype=torch.float32).to(device)
    return _CONV[key]


def upsample_dct(coeff, L=1, M=1):
    """utils/dct_ops.py:436-482 on (..., H, W, KH, KW), fp32: every block zero-padded to (L KH) x (M KW) and scaled by sqrt(L M),
    A_L^T . P . A_M, split into L x M blocks.  Device tensor ops (two batched matrix products)."""
    if L == 1 and M == 1:
        return coeff.to(torch.float32)
    *lead, H, W, KH, KW = coeff.shape
    AL = _conv(KH, L, coeff.device)
    AM = AL if (L == M and KH == KW) else _conv(KW, M, coeff.device)
    P = torch.zeros(*lead, H, W, L * KH, M * KW, dtype=torch.float32, device=coeff.device)
    P[..., :KH, :KW] = coeff.to(torch.float32) * (L * M) ** 0.5
    t = torch.matmul(torch.matmul(AL.T, P), AM)
    t = t.reshape(*lead, H, W, L, KH, M, KW)
    n = len(lead)
    t = t.permute(*range(n), n, n + 2, n + 1, n + 4, n + 3, n + 5)            # ... h l w m kh kw
    return t.reshape(*lead, H * L, W * M, KH, KW)


def downsample_dct(coeff, L=1, M=1):
    """utils/dct_ops.py:484-527: L x M neighbouring blocks gathered into one (L KH) x (M KW) block, A_L . X . A_M^T, top-left KH x KW
    kept, / sqrt(L M)."""
    if L == 1 and M == 1:
        return coeff.to(torch.float32)
    *lead, H, W, KH, KW = coeff.shape
    if H % L or W % M:
        raise ValueError(f"downsample_dct: a {H} x {W} grid is not a multiple of {L} x {M}")
    AL = _conv(KH, L, coeff.device)
    AM = AL if (L == M and KH == KW) else _conv(KW, M, coeff.device)
    n = len(lead)
    x = coeff.to(torch.float32).reshape(*lead, H // L, L, W // M, M, KH, KW)
    x = x.permute(*range(n), n, n + 2, n + 1, n + 4, n + 3, n + 5).reshape(*lead, H // L, W // M, L * KH, M * KW)
    t = torch.matmul(torch.matmul(AL, x), AM.T)
    return t[..., :KH, :KW] / (L * M) ** 0.5


def resize_dct(coeff, size, dtype_out="keep"):
    """utils/dct_ops.py:529-580 for ANY block grid: up by size / gcd(H, size), down by H / gcd (both axes on their own), fp32, then
    torch.round and back to the input dtype ('keep') or cast to dtype_out.  This is the general path of Resize_DCT -- the HIP augment
    kernels cover the factors 1/2, 1 and 2 of the training / eval pipelines (custom_transforms.Resize_DCT picks); here the work is
    two library batched matrix products per direction, like the DFT-plane ops below (no kernel of this repo).
    Parity: golden g23 (tests/golden/make_golden_r5_resize.py), <= 1 LSB and exact off .5 ties."""
    *_, H, W, KH, KW = coeff.shape
    hg, wg = math.gcd(H, size), math.gcd(W, size)
    up = upsample_dct(coeff, size // hg, size // wg)
    out = downsample_dct(up, H // hg, W // wg)
    if dtype_out == "keep":
        return torch.round(out).to(coeff.dtype)
    return out.to(dtype_out)


def gaussian_window(n, std, dtype=torch.float64):
    """scipy.signal.windows.gaussian(n, std) in closed form (used by midfreqaug_dct, dct_ops.py:732-733)."""
    k = torch.arange(n, dtype=dtype) - (n - 1.0) / 2.0
    return torch.exp(-0.5 * (k / std) ** 2)


def midfreq_filter(intensity, KH=8, KW=8):
    """8x8 multiplier of midfreqaug_dct (dct_ops.py:710-746) in un-shifted coordinates, fp32."""
    hi = KH // 2 - (KH // 8 * 2.2) * abs(intensity)
    wi = KW // 2 - (KW // 8 * 2.2) * abs(intensity)
    fh = gaussian_window(KH, hi).to(torch.float32).unsqueeze(1)
    fw = gaussian_window(KW, wi).to(torch.float32).unsqueeze(0)
    F = fh.mm(fw)
    if intensity >= 0:
        F = 1 / F
    return torch.roll(F, shifts=(-(KH // 2), -(KW // 2)), dims=(0, 1)).contiguous()


# ----------------------------------------------------------------------------------------------------------------
# DFT-plane Rotate / ShearX / ShearY of RandAugment_dct (utils/dct_ops.py:210-232, 303-434, 957-1013,
# utils/dct_torch_utils.py:232-321).  In no DCT op list of utils/configs.py, so not on the timed path.  Below: the device TENSOR path
# (complex matrix products through the library, index arithmetic for the nearest-neighbour resampling) and the operands of the
# batched kernels that compute the same thing (csrc/dft_ops.hip: conversion matrix, dft_gather_map, rotate_plan / shear_plan).  The
# reference resamples with torchvision's rotate / affine; torchvision is not installed here, so the sampling below restates its
# published tensor path (affine grid in fp32 + grid_sample nearest / zeros / align_corners=False) and the row is PARITY UNPINNED
# (oracle/dft_np.py says the same; tests compare the two restatements and pin what can be pinned structurally).
# ----------------------------------------------------------------------------------------------------------------
_DFT_CONV = {}


def generate_fourier_basis(length=8, scale=True, device="cpu"):
    """utils/dct_ops.py:135-146."""
    t = torch.arange(length, device=device, dtype=torch.float32)
    basis = (t.unsqueeze(1).mm(t.unsqueeze(0)) * (-1j * 2 * torch.pi / length)).exp()
    return basis / (length ** 0.5) if scale else basis


def generate_conversion_matrix_dft(length_small=2, mult=2, device="cpu"):
    """utils/dct_ops.py:210-232 (scale=True): small DCT blocks -> one large DFT; cached per (size, device)."""
    key = (length_small, mult, str(device))
    if key not in _DFT_CONV:
        small = generate_basis_matrix(length_small, device=device)
        blocks = torch.block_diag(*([small] * mult))
        _DFT_CONV[key] = generate_fourier_basis(length_small * mult, device=device).mm(blocks.T.to(torch.complex64))
    return _DFT_CONV[key]


def combine_blocks_dft(coeff):
    """utils/dct_ops.py:303-332 on (C,H,W,KH,KW)."""
    C, H, W, KH, KW = coeff.shape
    Lm = generate_conversion_matrix_dft(KH, H, coeff.device)
    Mm = Lm if (H == W and KH == KW) else generate_conversion_matrix_dft(KW, W, coeff.device)
    x = coeff.to(torch.complex64).permute(0, 1, 3, 2, 4).reshape(C, H * KH, W * KW)
    y = torch.einsum("ho,cow->chw", Lm, x) * ((KH * H) ** 0.5)
    y = torch.einsum("cho,ow->chw", y, torch.conj(Mm.T)) / ((KW * W) ** 0.5)
    return y, Lm, Mm


def decompose_block_dft(coeff, H, W, KH, KW, Lm, Mm):
    """utils/dct_ops.py:334-364."""
    y = torch.einsum("ho,cow->chw", torch.conj(Lm.T), coeff.to(torch.complex64)) / ((KH * H) ** 0.5)
    y = torch.einsum("cho,ow->chw", y, Mm) * ((KW * W) ** 0.5)
    return y.reshape(y.shape[0], H, KH, W, KW).permute(0, 1, 3, 2, 4).real


def blockshift(x, dim=(1, 2)):
    return torch.roll(torch.roll(x, x.shape[dim[0]] // 2, dim[0]), x.shape[dim[1]] // 2, dim[1])


def iblockshift(x, dim=(1, 2)):
    h, w = x.shape[dim[0]], x.shape[dim[1]]
    return torch.roll(torch.roll(x, h - h // 2, dim[0]), w - w // 2, dim[1])


def rotate_dct_90deg(coeff, rotate=0):
    """utils/dct_ops.py:99-130: exact quarter turns (counter-clockwise count) of (C,H,W,KH,KW) by index and sign work."""
    rotate = int(rotate)
    sign = (rotate / abs(rotate)) if rotate != 0 else 1
    r = abs(rotate) % 4
    out = coeff.clone()
    if r == 0:
        return out
    if sign * r == 3 or sign * r == -1:          # clockwise
        out = torch.rot90(out, k=-1, dims=(1, 2)).transpose(-2, -1).contiguous()
        out[..., 1::2] *= -1
        return out
    if r == 2:
        out = torch.flip(out, dims=(1, 2)).contiguous()
        out[..., 1::2, :] *= -1
        out[..., 1::2] *= -1
        return out
    out = torch.rot90(out, k=1, dims=(1, 2)).transpose(-2, -1).contiguous()
    out[..., 1::2, :] *= -1
    return out


def _inverse_affine_matrix(angle, shear):
    """torchvision.transforms.functional._get_inverse_affine_matrix(center=[0,0], angle, translate=[0,0], scale=1, shear)."""
    rot, sx, sy = math.radians(angle), math.radians(shear[0]), math.radians(shear[1])
    a = math.cos(rot - sy) / math.cos(sy)
    b = -math.cos(rot - sy) * math.tan(sx) / math.cos(sy) - math.sin(rot)
    c = math.sin(rot - sy) / math.cos(sy)
    d = -math.sin(rot - sy) * math.tan(sx) / math.cos(sy) + math.cos(rot)
    return [d, -b, 0.0, -c, a, 0.0]


def _nearest_source(H, W, matrix, dev):
    """The index math of torchvision's tensor path for rotate / affine with NEAREST, expand=False on an H x W plane: affine grid in
    fp32 (_gen_affine_grid), then grid_sample(mode='nearest', padding_mode='zeros', align_corners=False) as explicit index math
    (source index = round-half-even(((g + 1) * size - 1) / 2)).  Returns (iy, ix, ok): source row / column per output position
    (int64, unclamped) and whether it lies inside the plane."""
    theta = torch.tensor(matrix, dtype=torch.float32, device=dev).reshape(2, 3)
    base = torch.empty(H, W, 3, dtype=torch.float32, device=dev)
    base[..., 0] = torch.linspace(-W * 0.5 + 0.5, W * 0.5 + 0.5 - 1, steps=W, device=dev)
    base[..., 1] = torch.linspace(-H * 0.5 + 0.5, H * 0.5 + 0.5 - 1, steps=H, device=dev).unsqueeze(-1)
    base[..., 2] = 1
    rescaled = theta.T / torch.tensor([0.5 * W, 0.5 * H], dtype=torch.float32, device=dev)
    grid = base.view(-1, 3).mm(rescaled).view(H, W, 2)
    ix = torch.round(((grid[..., 0] + 1) * W - 1) / 2).long()
    iy = torch.round(((grid[..., 1] + 1) * H - 1) / 2).long()
    ok = (ix >= 0) & (ix < W) & (iy >= 0) & (iy < H)
    return iy, ix, ok


def _resample_nearest(plane, matrix):
    """torchvision's tensor path for rotate / affine with NEAREST, expand=False, fill 0 on a (C,H,W) fp32 plane (_nearest_source)."""
    C, H, W = plane.shape
    iy, ix, ok = _nearest_source(H, W, matrix, plane.device)
    src = (iy.clamp(0, H - 1) * W + ix.clamp(0, W - 1)).view(-1)
    out = plane.reshape(C, -1)[:, src].view(C, H, W)
    return out * ok.to(plane.dtype)


_GATHER_MAPS = {}            # (matrix, N, device) -> int32 (N, N); insertion ordered, at most _GATHER_MAPS_MAX entries
_GATHER_MAPS_MAX = 32        # training uses at most six matrices per grid (Rotate +-, ShearX +-, ShearY +- at one magnitude)


def dft_gather_map(matrix, N, device="cpu"):
    """fftshift, _resample_nearest and ifftshift of an N x N DFT plane composed into ONE gather: G.view(-1)[p] = F.view(-1)[map[p]],
    or 0 where map[p] == -1 (the sample falls outside the plane).  int32 (N, N), built on `device` from the fp32 tensor expressions
    of _nearest_source, so its source indices are those of the tensor path there; cached per (matrix, N, device).  The operand of
    rgbnm_dct_dft_ops (csrc/dft_ops.hip)."""
    key = (tuple(float(v) for v in matrix), int(N), str(device))
    m = _GATHER_MAPS.get(key)
    if m is None:
        iy, ix, ok = _nearest_source(N, N, matrix, device)
        h = N // 2
        # the sampler works on the fftshift-ed plane sh[a, b] = F[(a + h) % N, (b + h) % N] (N is even: 8 Hp)
        src = ((iy + h) % N) * N + (ix + h) % N
        src = torch.where(ok, src, torch.full_like(src, -1))
        m = torch.fft.ifftshift(src, dim=(-2, -1)).to(torch.int32).contiguous()
        while len(_GATHER_MAPS) >= _GATHER_MAPS_MAX:
            _GATHER_MAPS.pop(next(iter(_GATHER_MAPS)))
        _GATHER_MAPS[key] = m
    return m


def _dft_plane_op(coeff, matrix, pad, rot90s=0):
    """The common part of rotate_block / shear_block (window=False): pad, [exact quarter turns of the PADDED grid -- its margins
    differ by one block when the padded size is odd --], block shift, combine, fftshift, resample real and imaginary parts, inverse
    shifts, decompose, crop, round for integer dtypes."""
    C, H, W, KH, KW = coeff.shape
    dt = coeff.dtype
    x, hm, wm = coeff, 0, 0
    if pad:
        assert pad >= 1, "Padding should be larger than 1"
        Hp, Wp = int(H * pad // 1), int(W * pad // 1)
        hm, wm = (Hp - H) // 2, (Wp - W) // 2
        x = torch.zeros(C, Hp, Wp, KH, KW, dtype=dt, device=coeff.device)
        x[:, hm:hm + H, wm:wm + W] = coeff
    if rot90s:
        x = rotate_dct_90deg(x, rotate=rot90s)
    Hp, Wp = x.shape[1], x.shape[2]
    comp, Lm, Mm = combine_blocks_dft(blockshift(x))
    sh = torch.fft.fftshift(comp, dim=(-2, -1))
    res = torch.complex(_resample_nearest(sh.real.contiguous(), matrix), _resample_nearest(sh.imag.contiguous(), matrix))
    dec = iblockshift(decompose_block_dft(torch.fft.ifftshift(res, dim=(-2, -1)), Hp, Wp, KH, KW, Lm, Mm))
    if pad:
        dec = dec[:, hm:hm + H, wm:wm + W]
    if not dt.is_floating_point:
        dec = torch.round(dec)
    return dec.to(dt)


def rotate_plan(degrees):
    """rotate_block's split of an angle (utils/dct_ops.py:367-434): (exact quarter turns 0..3, inverse affine matrix of the
    remainder in (-45, 45])."""
    sign = degrees / abs(degrees) if degrees != 0 else 1
    rem = sign * (abs(degrees) % 360)
    shifted = (rem + 360 + 45) % 360
    rot90s = shifted // 90
    left = -((rot90s * 90) - (shifted - 45))
    # dct_torch_utils.py:247 negates the angle, torchvision's rotate negates it again for its inverse matrix: +left here
    return int(rot90s), _inverse_affine_matrix(left, [0.0, 0.0])


def shear_plan(deg_x=0, deg_y=0):
    """shear_block's (quarter turns, inverse affine matrix)."""
    return 0, _inverse_affine_matrix(0.0, [deg_x, deg_y])


def padded_blocks(H, pad):
    """Block count of the padded grid _dft_plane_op works on."""
    return int(H * pad // 1) if pad else H


def rotate_block(coeff, degrees=45, pad=False):
    """utils/dct_ops.py:367-434 on a device tensor (C,H,W,KH,KW): counter-clockwise; quarter turns exactly, the remainder in
    (-45, 45] on the DFT plane."""
    rot90s, matrix = rotate_plan(degrees)
    return _dft_plane_op(coeff, matrix, pad, rot90s=rot90s)


def shear_block(coeff, deg_x=0, deg_y=0, pad=False):
    """utils/dct_ops.py:957-1013 on a device tensor."""
    return _dft_plane_op(coeff, shear_plan(deg_x, deg_y)[1], pad)
