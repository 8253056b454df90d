#!/usr/bin/env python
"""Time the pixel <-> DCT kernels (csrc/pixel_dct.hip) on one GPU: dct_manip.quantize_at_quality(., 100) and dct_manip.decode_coeff
on a batch of 256 RGB images at 224 x 224 and at 256 x 256, the four configurations interleaved.

Every configuration runs WARMUP calls, then ROUNDS interleaved blocks of ITERS timed calls (order reversed every other round), device
events around each block after a synchronise (tools/aug_chain_step.py: timed / summary / compare).  Reported per configuration:
median / min / max over the blocks' per-call times (they include the host side of a call: the table, the output allocation, the
launch), the bytes a call has to move (pixels once, coefficients once: 6 H W per image) and the rate the median implies, next to the
device's copy rate measured the same way (a device-to-device copy of the same byte count: the floor a memory-bound kernel can reach).
For scale, the reference's own quantize_at_quality / decode_coeff (libjpeg, one image per call on one host core) where the compiled
reference module is present.  Writes profiles/pixel_dct.json and prints it.
usage: python tools/pixel_dct_step.py [--iters 200] [--warmup 5] [--rounds 6] [--batch 256]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from rgb_no_more_amd import dct_manip as DM, lib as L  # noqa: E402
from tools.aug_chain_step import timed, summary, compare  # noqa: E402


def host_reference(img, reps=5):
    """ms per image of the reference's two functions on the host, or None where oracle/_ref is not built."""
    try:
        from oracle import build_ref
        dm = build_ref.load_ref()
    except Exception:
        dm = None
    if dm is None:
        return None
    t = torch.from_numpy(img.copy())
    dim, quant, Y, C = dm.quantize_at_quality(t, 100)
    enc, dec = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        dim, quant, Y, C = dm.quantize_at_quality(t, 100)
        t1 = time.perf_counter()
        dm.decode_coeff(dim, quant, Y, C)
        t2 = time.perf_counter()
        enc.append((t1 - t0) * 1e3)
        dec.append((t2 - t1) * 1e3)
    return {"encode_ms_per_image": float(np.median(enc)), "decode_ms_per_image": float(np.median(dec)), "reps": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200, help="calls per timed block")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pixel_dct.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    B = a.batch
    res = {"batch": B, "quality": 100, "iters": a.iters, "warmup": a.warmup, "rounds": a.rounds,
           "device": torch.cuda.get_device_name(0), "source_hash": L.source_hash(), "sizes": {}}
    r = np.random.RandomState(1234)
    fns, nbytes, imgs = {}, {}, {}
    for side in (224, 256):
        yy, xx = np.mgrid[0:side, 0:side]
        base = np.stack([128 + 90 * np.sin(xx / (17.0 + 5 * c)) * np.cos(yy / (23.0 - 4 * c)) for c in range(3)])
        img = np.clip(np.rint(base[None] + r.randint(-20, 21, (B, 3, side, side))), 0, 255).astype(np.uint8)
        imgs[side] = img[0]
        px = torch.from_numpy(img).to(dev)
        dim, quant, Y, C = DM.quantize_at_quality(px, 100)
        back = DM.decode_coeff(dim, quant, Y, C)
        res["sizes"][str(side)] = {"round_trip_max_abs_diff": int((back.int() - px.int()).abs().max())}
        n = 6 * side * side * B
        src, dst = torch.empty(n // 2, dtype=torch.uint8, device=dev), torch.empty(n // 2, dtype=torch.uint8, device=dev)
        fns[f"encode_{side}"] = lambda px=px: DM.quantize_at_quality(px, 100)
        fns[f"decode_{side}"] = lambda dim=dim, quant=quant, Y=Y, C=C: DM.decode_coeff(dim, quant, Y, C)
        fns[f"copy_{side}"] = lambda src=src, dst=dst: dst.copy_(src)          # reads n / 2, writes n / 2: the same traffic
        for k in ("encode", "decode", "copy"):
            nbytes[f"{k}_{side}"] = n
    out = summary(timed(list(fns), fns, a.warmup, a.rounds, a.iters))
    for k, v in out.items():
        v["bytes"] = nbytes[k]
        v["GB_per_s"] = nbytes[k] / (v["ms_median"] * 1e-3) / 1e9
    for side in (224, 256):
        s = res["sizes"][str(side)]
        for k in ("encode", "decode", "copy"):
            s[k] = out[f"{k}_{side}"]
        s["encode_vs_copy"] = compare(out, f"copy_{side}", f"encode_{side}")
        s["decode_vs_copy"] = compare(out, f"copy_{side}", f"decode_{side}")
        s["host_reference"] = host_reference(imgs[side])
        print(f"{side}: encode {s['encode']['ms_median']:.3f} ms ({s['encode']['GB_per_s']:.0f} GB/s), decode "
              f"{s['decode']['ms_median']:.3f} ms ({s['decode']['GB_per_s']:.0f} GB/s), copy {s['copy']['ms_median']:.3f} ms "
              f"({s['copy']['GB_per_s']:.0f} GB/s), host reference {s['host_reference']}", file=sys.stderr)
    line = json.dumps(res)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
