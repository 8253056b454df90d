"""Host restatement of what rgbnm_clip_adamw_wd_step_scaled does to its state block (include/rgbnm.h,
rgbnm_loss_scale_state), and the allowance its device-side bias corrections add to the AdamW bounds of step_ends_ref.  A plain
module: tests/test_loss_scale_cpu.py anchors update_scale() bit for bit to torch._amp_update_scale_ on CPU tensors (and shows
that an fp32 product fails there), tests/test_loss_scale_kernels.py compares the kernel's state with it after every call.

The scale update (torch._amp_update_scale_, then pipeline_utils.clip_gradscaler):
    found_inf : scale = fp32(fp64(scale) * backoff), tracker = 0
    otherwise : tracker += 1; at tracker == growth_interval: scale = fp32(fp64(scale) * growth) if finite, tracker = 0
    then      : scale > scale_max -> scale_max; scale < scale_min -> scale_min          (a NaN scale stays NaN)

Bias corrections.  The kernel takes bc1 = fp32(1 - beta1^t) and bc2_sqrt = fp32(sqrt(1 - beta2^t)) from an fp64 pow on the device,
step_ends_ref.adamw_ref from Python's.  Two fp64 results a few fp64 ulps apart round to the same fp32 number except next to a
rounding tie, where they land one fp32 ulp apart: at most 2^-23 relative on bc1 and on bc2_sqrt.  To first order the update
lr / bc1 * m / (sqrt(v) / bc2_sqrt + eps) then moves by at most 2^-23 |update| for each: BC_EXTRA = 2 * 2^-23 times |update| is
added to the bound of p (times 1 + wd_factor on a decayed chunk); m, v and the norm do not see the bias corrections.
"""
import math

import numpy as np
import torch

F32 = np.float32
BC_EXTRA = 2 * 2.0 ** -23


def update_scale(scale, tracker, found_inf, growth, backoff, interval, scale_min=None, scale_max=None, product="fp64"):
    """(scale, tracker) after one call; scale an fp32 value held in a Python float.  product="fp32" is the seeded defect: the
    product taken in fp32 instead of fp64."""
    s = F32(scale)

    def mul(a, f):
        with np.errstate(over="ignore"):
            return F32(np.float64(a) * np.float64(f)) if product == "fp64" else F32(a * F32(f))
    if found_inf:
        s, tracker = mul(s, backoff), 0
    else:
        tracker += 1
        if tracker == interval:
            grown = mul(s, growth)
            if np.isfinite(grown):
                s = grown
            tracker = 0
    if scale_max is not None and s > F32(scale_max):
        s = F32(scale_max)
    if scale_min is not None and s < F32(scale_min):
        s = F32(scale_min)
    return float(s), tracker


def torch_update_scale(scale, tracker, found_inf, growth, backoff, interval):
    """The same call through torch._amp_update_scale_ on CPU tensors (no clamp: GradScaler has none)."""
    s = torch.tensor([scale], dtype=torch.float32)
    t = torch.tensor([tracker], dtype=torch.int32)
    torch._amp_update_scale_(s, t, torch.tensor([1.0 if found_inf else 0.0]), float(growth), float(backoff), int(interval))
    return float(s), int(t)


def run_sequence(scale, found, growth, backoff, interval, scale_min=None, scale_max=None, product="fp64"):
    """[(scale, tracker)] after each entry of `found` (1 = a non-finite step)."""
    out, tracker = [], 0
    for f in found:
        scale, tracker = update_scale(scale, tracker, bool(f), growth, backoff, interval, scale_min, scale_max, product)
        out.append((scale, tracker))
    return out


def inv_of(scale):
    """fp32(1.0 / fp64(scale)): GradScaler.unscale_'s reciprocal, the kernel's `inv`."""
    return float(F32(1.0 / np.float64(F32(scale))))


def bias_correction_extra(r, p_before, flags, step, lr, beta1, beta2, eps, wd_factor):
    """BC_EXTRA |update| (1 + wd_factor on decayed chunks) for a result dict of step_ends_ref.adamw_ref: fp64 tensor to add to
    r["dp"]."""
    f = lambda x: float(torch.tensor(float(x), dtype=torch.float32))
    bc1 = f(1.0 - f(beta1) ** step)
    bc2s = f(math.sqrt(1.0 - f(beta2) ** step))
    upd = (f(lr) / bc1) * r["m"] / (torch.sqrt(r["v"]) / bc2s + f(eps))
    dec = flags.to(upd.device).bool().repeat_interleave(256)
    return BC_EXTRA * upd.abs() * torch.where(dec, 1.0 + f(wd_factor), 1.0)
