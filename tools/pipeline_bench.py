#!/usr/bin/env python
"""JPEG-fed end-to-end figure (SURVEY 8d "report the JPEG-fed pipeline figure separately", 8f f2): real baseline
JPEG files -> librgbnm_reader.so (pthread pool, libjpeg coefficient read, no IDCT) into pinned int16 batches -> one H2D
copy -> HIP dequant/crop/resize/RandAugment/ToRange -> mixup -> HIP ViT train step.  The decoder thread runs ahead of
the GPU by a two-deep queue.  Prints one JSON line; never part of bench.py's `value` (that one starts from HBM-resident
coefficients).  --decode device: the loader ships the compressed bytes instead and the GPU walks the files' restart runs
(csrc/jpeg_decode.hip; whole grids, no crop on the host); --restart-rows N writes the files with a restart marker per N MCU rows.
S-jpeg set: 64 files, 512x512, 4:2:0, q90 (32x32 uniform RGB upsampled bicubic + N(0,8) noise)."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rgb_no_more_amd as rg  # noqa: E402
from rgb_no_more_amd import custom_transforms as CT  # noqa: E402
from rgb_no_more_amd import dct_manip as dm  # noqa: E402


def write_sjpeg(d, n=64, restart_rows=0, quality=90):
    from PIL import Image
    rng = np.random.default_rng(0)
    paths = []
    for i in range(n):
        small = rng.integers(0, 256, (32, 32, 3), dtype=np.uint8)
        img = np.asarray(Image.fromarray(small).resize((512, 512), Image.BICUBIC), dtype=np.float32)
        img = np.clip(img + rng.normal(0, 8, img.shape), 0, 255).astype(np.uint8)
        p = os.path.join(d, f"s{i:03d}.jpg")
        kw = {"restart_marker_rows": restart_rows} if restart_rows else {}      # one restart marker per so many MCU rows
        Image.fromarray(img).save(p, quality=quality, subsampling="4:2:0", **kw)
        paths.append(p)
    return paths


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--threads", type=int, default=dm.default_threads())
    ap.add_argument("--crop-on-host", type=int, default=1, help="1: only the crop boxes cross PCIe (loader crop_on_host)")
    ap.add_argument("--decode", choices=("host", "device"), default="host",
                    help="device: the loader ships the compressed bytes and the GPU walks the restart runs (no crop on the host then)")
    ap.add_argument("--restart-rows", type=int, default=0, help="synthetic files carry a restart marker every N MCU rows (0: none)")
    ap.add_argument("--prefetch", type=int, default=2, help="batches the loader keeps ahead of the step")
    ap.add_argument("--jpeg-split", action="store_true",
                    help="with --decode device: long runs are cut into bit segments, one lane each (loader jpeg_split)")
    ap.add_argument("--crop-on-device", nargs="?", const=True, default=False, choices=("split",),
                    help="with --decode device: the decode walks and stores only each image's crop box (loader crop_on_device); "
                         "`--crop-on-device split`: through the split decode, for files without restart markers")
    a = ap.parse_args()
    if a.decode == "device":
        a.crop_on_host = 0
    if a.crop_on_device and a.decode != "device":
        ap.error("--crop-on-device needs --decode device")
    fused = bool(a.crop_on_host or a.crop_on_device)         # the loader draws the parameters and applies the transform itself
    dev = "cuda:0"
    torch.cuda.set_device(0)
    tmp = tempfile.mkdtemp(prefix="sjpeg_")
    paths = write_sjpeg(tmp, restart_rows=a.restart_rows)
    fsize = sum(os.path.getsize(p) for p in paths) / len(paths)
    B = a.batch
    batch_paths = [paths[i % len(paths)] for i in range(B)]

    # ---- host decode alone
    ring = [dm.alloc_batch(B) for _ in range(4)]          # pinned staging buffers, re-used
    for _ in range(2):
        dm.read_coefficients_batch(batch_paths, threads=a.threads, out=ring[0])
    t0 = time.perf_counter()
    nrep = 8
    for i in range(nrep):
        dm.read_coefficients_batch(batch_paths, threads=a.threads, out=ring[i % 4])
    dec = nrep * B / (time.perf_counter() - t0)

    model = rg.ViT(3, 16, 192, depth=12, n_classes=1000, drop_p=0.0, device=dev, num_heads=3, head_size=64,
                   pixel_space="DCT", ver=1, use_subblock=True)
    model.compute_dtype = torch.bfloat16
    opt = rg.custom_optims.FusedClipAdamWWD(model, lr=1e-3, eps=1e-8, weight_decay=1e-4, max_norm=1.0)
    mix = rg.cls_transforms.RandomMixup_DCT(1000, alpha=0.2)
    mix.out_dtype = torch.bfloat16
    mix.lazy = True             # the ViT mixes while its sub-block kernel loads (cls_transforms.LazyMixed), as in bench.py
    aug = CT.TrainTransform_DCT(out_dtype=torch.bfloat16)
    sampler = CT.FastParamSampler(aug, seed=1234)
    lab = torch.randint(0, 999, (B,), device=dev)

    # the product loader (rgb_no_more_amd/loader.py): decoder thread + pinned ring + one H2D copy per tensor; the fused
    # HIP transform is applied here with FastParamSampler so that the step is the one bench.py times
    from rgb_no_more_amd.loader import DCTBatchLoader
    nb = a.warmup + a.steps + 4
    loader = DCTBatchLoader([batch_paths[i % B] for i in range(nb * B)], [int(v) for v in torch.randint(0, 999, (nb * B,))], B,
                            device=dev, threads=a.threads, prefetch=a.prefetch, shuffle=False,
                            transform=aug if fused else None, crop_on_host=bool(a.crop_on_host), decode=a.decode,
                            jpeg_split=a.jpeg_split, crop_on_device=a.crop_on_device)
    it = iter(loader)

    def step():
        opt.zero_grad(set_to_none=True)
        if fused:
            (y, c), labd = next(it)
        else:
            (Yd, Cd, Qd), labd = next(it)
            packed, nops = sampler.sample(B, 64, 64)
            y, c = CT.apply_packed(aug, Yd, Cd, Qd, packed, nops)
        (my, mc), mt = mix((y, c), labd)
        loss = rg.cls_transforms.cross_entropy(model(my, mc), mt, grad_dtype=torch.bfloat16)
        loss.backward()
        opt.step()
        return loss

    for _ in range(a.warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        loss = step()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    it.close()
    h2d = loader.h2d_bytes / B if (a.crop_on_host or a.decode == "device") else 64 * 64 * 64 * 2 + 2 * 32 * 32 * 64 * 2 + 3 * 64 * 2
    out = {"metric": f"images/sec JPEG-Ti DCT train step fed from JPEG files ({a.decode} entropy decode + H2D inside)",
           "decode": a.decode, "jpeg_split": bool(a.jpeg_split),
           "jpeg_split_seg_bits": dm.JPEG_SPLIT_SEG_BITS if a.jpeg_split else None,      # what the loader's split launch uses
           "jpeg_split_rounds": dm.JPEG_SPLIT_ROUNDS if a.jpeg_split else None, "restart_rows": a.restart_rows, "prefetch": a.prefetch,
           "value": round(B * a.steps / dt, 1), "unit": "images/sec", "n_gpus": 1, "steps": a.steps,
           "ms_per_step": round(1e3 * dt / a.steps, 3), "per_gpu_batch": B, "host_threads": a.threads,
           "host_decode_only_images_per_sec": round(dec, 1), "avg_jpeg_bytes": round(fsize),
           "h2d_bytes_per_image": round(h2d),
           "crop_on_host": bool(a.crop_on_host), "crop_on_device": bool(a.crop_on_device), "crop_split": a.crop_on_device == "split",
           "loss": round(float(loss.item()), 4),
           "note": "one process; decoder thread (pthread pool inside librgbnm_reader.so, GIL released) runs two batches "
                   "ahead; bounded by the host Huffman decode when value ~ host_decode_only"}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
