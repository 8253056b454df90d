#!/usr/bin/env python
"""Measure the device JPEG entropy decode (csrc/jpeg_scan.h, jpeg_decode.hip) on one GPU.  B = 256 files of 512 x 512, 4:2:0, made as
tests/test_loader_gpu.py makes them (16 x 16 random colours upsampled bicubic, plus N(0, 8) noise; 64 distinct files, repeated).

  (a) dct_manip.prepare_jpeg_batch alone, on the host, ms per batch with 1 and with 16 threads (file bytes already in memory).
  (b) the decode launch alone (plan already on the device: dct_manip.launch_jpeg_decode) for four file sets -- quality 75 and 90
      without restart markers, quality 90 with one restart per MCU row and with one per 4 MCUs -- with the bytes a batch ships
      beside the 201 MB of coefficients the host path ships.
  (c) tools/pipeline_bench.py images/s: --decode host (the loader's existing path, 16 threads, measured again here) and --decode
      device on the same files without restart markers and with one per MCU row; each a process of its own.

  (s) the SPLIT decode launch (dct_manip.launch_jpeg_decode(split=True): long runs cut into bit segments, one lane each) beside the
      plain launch of (b) -- the same code as before, so the yardstick -- on the same four file sets, in the same interleaved rounds:
      seg_bits in 512 / 1024 / 2048 / 4096 and a few values of rounds, with the share of images per `path` value (0 not split,
      1 split, 2 split and then decoded by the one-lane walk).
  (p) tools/pipeline_bench.py images/s with --decode device --jpeg-split on the marker-less files and on those with a marker per
      MCU row, beside --decode host at 16 threads and plain --decode device; each a process of its own per round.
  (s) and (p) go to profiles/jpeg_split.json, (a) - (c) to profiles/jpeg_decode.json.

  (x) the CROP decode launch (dct_manip.launch_jpeg_decode(boxes=...): runs outside an image's crop box are skipped, the others stop
      after the last MCU the box needs, only the boxes are stored) beside the plain whole-grid launch on the same plans in the same
      interleaved rounds: no restart markers, one per MCU row, one per 4 MCUs.  The boxes are FastParamSampler's at the defaults of
      TrainTransform_DCT; reported with the time: the mean share of MCUs walked (from the launch's `walked` array), the share of runs
      skipped, the bytes written, and the crop launch with one run per wave ("jpeg_lanes" = 1).
  (y) tools/pipeline_bench.py images/s with --decode device --crop-on-device beside plain --decode device, on the marker-less files
      and on those with a marker per MCU row; each a process of its own per round.
  (x) and (y) go to profiles/jpeg_crop.json.

  (z) the SPLIT decode launch FOR CROP BOXES (dct_manip.launch_jpeg_split_crop: scout, sync and verify over the whole runs, the write
      pass only over the segments that hold a block of an image's box, compacted into dense waves, only the boxes stored) beside the
      whole-grid split launch -- the yardstick, measured again here -- and the plain crop launch, on the marker-less q90 files, with
      (x)'s boxes and the split decode's defaults: bytes written, the live share of the segments (from the launch's `seg_live`
      array) and the share of images per `path` value.
  (w) tools/pipeline_bench.py images/s with --decode device --crop-on-device split beside --decode device --jpeg-split (the
      yardstick) and plain --decode device, on the marker-less files; each a process of its own per round.
  (z) and (w) go to profiles/jpeg_split_crop.json.

Protocol of the other step tools: warm-up, then ROUNDS interleaved rounds (order reversed every other round); median and min - max.
Writes profiles/jpeg_decode.json, or profiles/jpeg_split.json for parts s / p, or profiles/jpeg_crop.json for parts x / y, or
profiles/jpeg_split_crop.json for parts z / w (parts given with --parts are replaced, the others kept), and prints it.
usage: python tools/jpeg_decode_step.py [--parts a,b,c | s,p | x,y | z,w] [--rounds 6] [--batch 256]"""
import argparse
import io
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from rgb_no_more_amd import dct_manip as DM, lib as L  # noqa: E402
from tools.aug_chain_step import timed, summary  # noqa: E402

SETS = {"q75": dict(quality=75), "q90": dict(quality=90), "q90_rst_row": dict(quality=90, restart_marker_rows=1),
        "q90_rst_4mcu": dict(quality=90, restart_marker_blocks=4)}
COEF_BYTES = (64 * 64 + 2 * 32 * 32) * 128 + 3 * 128


def synth(n, **kw):
    from PIL import Image
    rng = np.random.default_rng(0)
    out = []
    for _ in range(n):
        small = rng.integers(0, 256, (16, 16, 3), dtype=np.uint8)
        img = np.asarray(Image.fromarray(small).resize((512, 512), Image.BICUBIC), dtype=np.float32)
        img = np.clip(img + rng.normal(0, 8, img.shape), 0, 255).astype(np.uint8)
        buf = io.BytesIO()
        Image.fromarray(img).save(buf, format="JPEG", subsampling="4:2:0", **kw)
        out.append(buf.getvalue())
    return out


def spread(v):
    return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v)), "rounds": [float(x) for x in v]}


def part_a(B, rounds, reps=4):
    res = {}
    for name in ("q90", "q90_rst_row"):
        files = synth(64, **SETS[name])
        batch = [files[i % 64] for i in range(B)]
        plan = DM.JpegBatchPlan(B, (64, 64), pin_memory=True)
        ms = {1: [], 16: []}
        for th in (1, 16):
            DM.prepare_jpeg_batch(batch, out=plan, threads=th)
        assert plan.nbad == 0
        for r in range(rounds):
            for th in ((1, 16) if r % 2 == 0 else (16, 1)):
                t0 = time.perf_counter()
                for _ in range(reps):
                    DM.prepare_jpeg_batch(batch, out=plan, threads=th)
                ms[th].append((time.perf_counter() - t0) * 1e3 / reps)
        res[name] = {"file_bytes_per_batch": sum(len(b) for b in batch), "runs": plan.nruns,
                     "ms_per_batch_1_thread": spread(ms[1]), "ms_per_batch_16_threads": spread(ms[16]),
                     "images_per_s_1_thread": B / np.median(ms[1]) * 1e3, "images_per_s_16_threads": B / np.median(ms[16]) * 1e3}
        print(f"(a) {name}: 1 thread {np.median(ms[1]):.2f} ms, 16 threads {np.median(ms[16]):.2f} ms per batch", file=sys.stderr)
    return res


def part_b(B, rounds, iters, warmup):
    dev = torch.device("cuda", 0)
    fns, meta, keep = {}, {}, []
    for name, kw in SETS.items():
        files = synth(64, **kw)
        batch = [files[i % 64] for i in range(B)]
        plan = DM.prepare_jpeg_batch(batch, grid=(64, 64))
        assert plan.nbad == 0
        up = DM.upload_jpeg_plan(plan, dev)
        out = DM.alloc_jpeg_out(B, (64, 64), dev)
        out[2].copy_(up[4])
        out[3].copy_(up[5])
        DM.launch_jpeg_decode(plan, up, out)
        torch.cuda.synchronize()
        ref = DM.read_coefficients_bytes(batch[5])                        # same bits as the host reader, at the size that is timed
        assert torch.equal(out[0][5].cpu(), ref[2]) and torch.equal(out[1][5].cpu(), ref[3]) and int(out[3].min()) == 0
        keep.append((plan, up, out))
        fns[name] = lambda plan=plan, up=up, out=out: DM.launch_jpeg_decode(plan, up, out)
        meta[name] = {"runs": plan.nruns, "tables": plan.ntables, "h2d_bytes_per_batch": plan.h2d_bytes(),
                      "h2d_bytes_host_path": COEF_BYTES * B, "file_bytes_per_batch": sum(len(b) for b in batch),
                      "runs_per_wave": max(1, min(64, -(-plan.nruns // 2048)))}
        # the same launch with every wave full (option "jpeg_lanes" = 64): what spreading the runs over more waves is worth
        fns[name + "_64_per_wave"] = fns[name]
        meta[name + "_64_per_wave"] = dict(meta[name], runs_per_wave=64)
    out = summary(timed(list(fns), fns, warmup, rounds, iters,
                        before=lambda cfg: L.set_option("jpeg_lanes", 64 if cfg.endswith("_64_per_wave") else 0)))
    L.set_option("jpeg_lanes", 0)
    for k, v in out.items():
        v.update(meta[k])
        v["images_per_s"] = B / v["ms_median"] * 1e3
        print(f"(b) {k}: {v['ms_median']:.3f} ms ({v['ms_min']:.3f} - {v['ms_max']:.3f}) per batch, {v['runs']} runs, "
              f"{v['h2d_bytes_per_batch'] / 1e6:.1f} MB shipped", file=sys.stderr)
    return out


SPLIT_SEG_BITS = (512, 1024, 2048, 4096)
SPLIT_ROUNDS = (2, 6, 16)


def part_s(B, rounds, iters, warmup, sets):
    dev = torch.device("cuda", 0)
    fns, meta, keep = {}, {}, []
    for name in sets:
        files = synth(64, **SETS[name])
        batch = [files[i % 64] for i in range(B)]
        plan = DM.prepare_jpeg_batch(batch, grid=(64, 64))
        assert plan.nbad == 0
        up = DM.upload_jpeg_plan(plan, dev)
        out = DM.alloc_jpeg_out(B, (64, 64), dev)
        out[2].copy_(up[4])
        out[3].copy_(up[5])
        DM.launch_jpeg_decode(plan, up, out)
        torch.cuda.synchronize()
        want = [t.clone() for t in out]
        keep.append((plan, up, out))
        fns[name] = lambda plan=plan, up=up, out=out: DM.launch_jpeg_decode(plan, up, out)
        meta[name] = {"runs": plan.nruns, "file_bytes_per_batch": sum(len(b) for b in batch), "stream_bytes": plan.stream_bytes}
        for sb in SPLIT_SEG_BITS:
            scratch = DM.jpeg_split_scratch(plan, sb, dev)
            for r in SPLIT_ROUNDS:
                path = torch.empty(B, dtype=torch.int32, device=dev)
                for t in out[:2]:
                    t.fill_(0x5555)
                DM.launch_jpeg_decode(plan, up, out, split=True, seg_bits=sb, rounds=r, path=path, scratch=scratch)
                torch.cuda.synchronize()
                assert all(torch.equal(x, y) for x, y in zip(out, want)), (name, sb, r)       # the bits of the plain launch
                share = [float((path == v).sum()) / B for v in (0, 1, 2)]
                cfg = f"{name}_split_sb{sb}_r{r}"
                fns[cfg] = lambda plan=plan, up=up, out=out, sb=sb, r=r, path=path, scratch=scratch: DM.launch_jpeg_decode(
                    plan, up, out, split=True, seg_bits=sb, rounds=r, path=path, scratch=scratch)
                meta[cfg] = dict(meta[name], seg_bits=sb, sync_rounds=r, scratch_bytes=scratch.numel(), path_share=share)
    out = summary(timed(list(fns), fns, warmup, rounds, iters))
    for k, v in out.items():
        v.update(meta[k])
        v["images_per_s"] = B / v["ms_median"] * 1e3
        print(f"(s) {k}: {v['ms_median']:.3f} ms ({v['ms_min']:.3f} - {v['ms_max']:.3f}) per batch, path share {v.get('path_share')}",
              file=sys.stderr)
    return out


CROP_SETS = ("q90", "q90_rst_row", "q90_rst_4mcu")


def part_x(B, rounds, iters, warmup):
    from rgb_no_more_amd import custom_transforms as CT
    dev = torch.device("cuda", 0)
    packed, _ = CT.FastParamSampler(CT.TrainTransform_DCT(out_dtype=torch.bfloat16), seed=1234).sample(B, 64, 64)
    boxes = torch.from_numpy(packed["crop"].astype("int32"))
    y_off, c_off, ny, ncc = DM.packed_offsets(boxes)
    bdev, yo, co = boxes.to(dev), y_off.to(dev), c_off.to(dev)
    fns, meta, keep = {}, {}, []
    for name in CROP_SETS:
        files = synth(64, **SETS[name])
        batch = [files[i % 64] for i in range(B)]
        plan = DM.prepare_jpeg_batch(batch, grid=(64, 64))
        assert plan.nbad == 0
        up = DM.upload_jpeg_plan(plan, dev)
        out = DM.alloc_jpeg_out(B, (64, 64), dev)
        out[2].copy_(up[4])
        out[3].copy_(up[5])
        DM.launch_jpeg_decode(plan, up, out)
        pk = (torch.full((ny,), 0x5555, dtype=torch.int16, device=dev), torch.full((ncc,), 0x5555, dtype=torch.int16, device=dev),
              out[2].clone(), up[5].clone())
        walked = torch.full((plan.nruns,), -1, dtype=torch.int32, device=dev)
        DM.launch_jpeg_decode(plan, up, pk, boxes=bdev, packed_out=(yo, co, ny, ncc), walked=walked)
        torch.cuda.synchronize()
        # the bits that are timed: the boxes cut out of the whole-grid launch's output
        for i in range(B):
            t, l, h, w = boxes[i].tolist()
            assert torch.equal(pk[0][int(y_off[i]):int(y_off[i]) + h * w * 64], out[0][i, 0, t:t + h, l:l + w].reshape(-1)), (name, i)
            assert torch.equal(pk[1][int(c_off[i]):int(c_off[i]) + h * w * 32],
                               out[1][i, :, t // 2:(t + h) // 2, l // 2:(l + w) // 2].reshape(-1)), (name, i)
        assert int(pk[3].min()) == 0 and int(out[3].min()) == 0
        nmcu = plan.runs[:plan.nruns, 4].to(torch.int64)
        wk = walked.cpu().to(torch.int64)
        assert bool((wk >= 0).all()) and bool((wk <= nmcu).all())
        keep.append((plan, up, out, pk, walked))
        fns[name] = lambda plan=plan, up=up, out=out: DM.launch_jpeg_decode(plan, up, out)
        meta[name] = {"runs": plan.nruns, "bytes_written": 2 * (out[0].numel() + out[1].numel())}
        crop = lambda plan=plan, up=up, pk=pk: DM.launch_jpeg_decode(plan, up, pk, boxes=bdev, packed_out=(yo, co, ny, ncc))  # noqa: E731
        cm = {"runs": plan.nruns, "bytes_written": 2 * (ny + ncc), "walked_share_of_mcus": float(wk.sum()) / float(nmcu.sum()),
              "runs_skipped_share": float((wk == 0).sum()) / plan.nruns,
              "runs_stopped_early_share": float(((wk > 0) & (wk < nmcu)).sum()) / plan.nruns,
              "box_share_of_grid": ny / (B * 64 * 64 * 64)}
        fns[name + "_crop"] = crop
        meta[name + "_crop"] = cm
        fns[name + "_crop_1_per_wave"] = crop
        meta[name + "_crop_1_per_wave"] = dict(cm, runs_per_wave=1)
    out = summary(timed(list(fns), fns, warmup, rounds, iters,
                        before=lambda cfg: L.set_option("jpeg_lanes", 1 if cfg.endswith("_1_per_wave") else 0)))
    L.set_option("jpeg_lanes", 0)
    for k, v in out.items():
        v.update(meta[k])
        v["images_per_s"] = B / v["ms_median"] * 1e3
        print(f"(x) {k}: {v['ms_median']:.3f} ms ({v['ms_min']:.3f} - {v['ms_max']:.3f}) per batch, {v['bytes_written'] / 1e6:.1f} MB written, "
              f"walked share {v.get('walked_share_of_mcus')}", file=sys.stderr)
    return out


def part_z(B, rounds, iters, warmup):
    from rgb_no_more_amd import custom_transforms as CT
    dev = torch.device("cuda", 0)
    packed, _ = CT.FastParamSampler(CT.TrainTransform_DCT(out_dtype=torch.bfloat16), seed=1234).sample(B, 64, 64)
    boxes = torch.from_numpy(packed["crop"].astype("int32"))
    y_off, c_off, ny, ncc = DM.packed_offsets(boxes)
    bdev, yo, co = boxes.to(dev), y_off.to(dev), c_off.to(dev)
    sb, nr = DM.JPEG_SPLIT_SEG_BITS, DM.JPEG_SPLIT_ROUNDS
    files = synth(64, **SETS["q90"])
    batch = [files[i % 64] for i in range(B)]
    plan = DM.prepare_jpeg_batch(batch, grid=(64, 64))
    assert plan.nbad == 0
    up = DM.upload_jpeg_plan(plan, dev)
    out = DM.alloc_jpeg_out(B, (64, 64), dev)
    out[2].copy_(up[4])
    out[3].copy_(up[5])
    path = torch.empty(B, dtype=torch.int32, device=dev)
    scratch = DM.jpeg_split_scratch(plan, sb, dev)
    DM.launch_jpeg_decode(plan, up, out, split=True, path=path, scratch=scratch)
    pk = (torch.full((ny,), 0x5555, dtype=torch.int16, device=dev), torch.full((ncc,), 0x5555, dtype=torch.int16, device=dev),
          out[2].clone(), up[5].clone())
    pk2 = tuple(t.clone() for t in pk)
    xpath = torch.empty(B, dtype=torch.int32, device=dev)
    xscratch = DM.jpeg_split_crop_scratch(plan, sb, dev)
    seg_live = torch.full((plan.nruns,), -1, dtype=torch.int32, device=dev)
    DM.launch_jpeg_split_crop(plan, up, pk, bdev, (yo, co, ny, ncc), path=xpath, scratch=xscratch, seg_live=seg_live)
    DM.launch_jpeg_decode(plan, up, pk2, boxes=bdev, packed_out=(yo, co, ny, ncc))
    torch.cuda.synchronize()
    # the bits that are timed: the boxes cut out of the whole-grid split launch's output, and the plain crop launch's
    for i in range(B):
        t, l, h, w = boxes[i].tolist()
        assert torch.equal(pk[0][int(y_off[i]):int(y_off[i]) + h * w * 64], out[0][i, 0, t:t + h, l:l + w].reshape(-1)), i
        assert torch.equal(pk[1][int(c_off[i]):int(c_off[i]) + h * w * 32], out[1][i, :, t // 2:(t + h) // 2, l // 2:(l + w) // 2].reshape(-1)), i
    assert torch.equal(pk[0], pk2[0]) and torch.equal(pk[1], pk2[1]) and torch.equal(path, xpath)
    assert int(pk[3].min()) == 0 and int(out[3].min()) == 0
    nbytes = plan.runs[:plan.nruns, 1].to(torch.int64) & 0xFFFFFFFF
    nseg = (nbytes * 8 + sb - 1) // sb
    written = (xpath.cpu() == 1)[plan.runs[:plan.nruns, 2].to(torch.int64)] & (nseg >= 16)
    share = [float((path == v).sum()) / B for v in (0, 1, 2)]
    base = {"runs": plan.nruns, "seg_bits": sb, "sync_rounds": nr, "path_share": share, "stream_bytes": plan.stream_bytes}
    meta = {"q90_split": dict(base, bytes_written=2 * (out[0].numel() + out[1].numel()), scratch_bytes=scratch.numel()),
            "q90_split_crop": dict(base, bytes_written=2 * (ny + ncc), scratch_bytes=xscratch.numel(), box_share_of_grid=ny / (B * 64 * 64 * 64),
                                   segments=int(nseg[written].sum()), segments_live=int(seg_live.cpu()[written].sum()),
                                   live_share_of_segments=float(seg_live.cpu()[written].sum()) / max(1, int(nseg[written].sum()))),
            "q90_crop": {"runs": plan.nruns, "bytes_written": 2 * (ny + ncc)}}
    fns = {"q90_split": lambda: DM.launch_jpeg_decode(plan, up, out, split=True, path=path, scratch=scratch),
           "q90_split_crop": lambda: DM.launch_jpeg_split_crop(plan, up, pk, bdev, (yo, co, ny, ncc), path=xpath, scratch=xscratch),
           "q90_crop": lambda: DM.launch_jpeg_decode(plan, up, pk2, boxes=bdev, packed_out=(yo, co, ny, ncc))}
    res = summary(timed(list(fns), fns, warmup, rounds, iters))
    for k, v in res.items():
        v.update(meta[k])
        v["images_per_s"] = B / v["ms_median"] * 1e3
        print(f"(z) {k}: {v['ms_median']:.3f} ms ({v['ms_min']:.3f} - {v['ms_max']:.3f}) per batch, {v['bytes_written'] / 1e6:.1f} MB written, "
              f"live share {v.get('live_share_of_segments')}", file=sys.stderr)
    return res


PIPELINE = {"host_16_threads": ["--decode", "host", "--threads", "16"],
            "device": ["--decode", "device", "--threads", "16", "--prefetch", "4"],
            "device_rst_row": ["--decode", "device", "--threads", "16", "--prefetch", "4", "--restart-rows", "1"]}
PIPELINE_SPLIT = {"host_16_threads": PIPELINE["host_16_threads"], "device": PIPELINE["device"],
                  "device_split": PIPELINE["device"] + ["--jpeg-split"], "device_rst_row": PIPELINE["device_rst_row"],
                  "device_rst_row_split": PIPELINE["device_rst_row"] + ["--jpeg-split"]}


PIPELINE_CROP = {"device": PIPELINE["device"], "device_crop": PIPELINE["device"] + ["--crop-on-device"],
                 "device_rst_row": PIPELINE["device_rst_row"], "device_rst_row_crop": PIPELINE["device_rst_row"] + ["--crop-on-device"]}


PIPELINE_SPLIT_CROP = {"device": PIPELINE["device"], "device_split": PIPELINE["device"] + ["--jpeg-split"],
                       "device_crop_split": PIPELINE["device"] + ["--crop-on-device", "split"]}


def part_c(B, rounds, steps, warmup, cfgs=PIPELINE):
    val = {k: [] for k in cfgs}
    last = {}
    for r in range(rounds):
        for k in (list(cfgs) if r % 2 == 0 else list(cfgs)[::-1]):
            cmd = [sys.executable, os.path.join(ROOT, "tools", "pipeline_bench.py"), "--steps", str(steps), "--warmup", str(warmup),
                   "--batch", str(B)] + cfgs[k]
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
            if p.returncode != 0:
                raise RuntimeError(f"{' '.join(cmd)} failed:\n{p.stderr[-2000:]}")
            last[k] = json.loads(p.stdout.strip().splitlines()[-1])
            val[k].append(last[k]["value"])
            print(f"(c) round {r} {k}: {last[k]['value']} images/s", file=sys.stderr, flush=True)
    return {k: {"images_per_s": spread(val[k]), "ms_per_step": last[k]["ms_per_step"], "h2d_bytes_per_image": last[k]["h2d_bytes_per_image"],
                "host_decode_only_images_per_sec": last[k]["host_decode_only_images_per_sec"], "steps": steps, "args": cfgs[k],
                "jpeg_split_seg_bits": last[k].get("jpeg_split_seg_bits"), "jpeg_split_rounds": last[k].get("jpeg_split_rounds")}
            for k in cfgs}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="a,b,c")
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--iters", type=int, default=5, help="(b) launches per timed block")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=40, help="(c) timed steps per process")
    ap.add_argument("--sets", default=",".join(SETS), help="(s) file sets")
    ap.add_argument("--out", default=None, help="default: profiles/jpeg_split.json for parts s / p, else profiles/jpeg_decode.json")
    a = ap.parse_args()
    parts = a.parts.split(",")
    groups = [g for g in ({"a", "b", "c"}, {"s", "p"}, {"x", "y"}, {"z", "w"}) if set(parts) & g]
    if len(groups) != 1:
        raise SystemExit("parts a / b / c, s / p, x / y and z / w write different files: run them separately")
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", {"a": "jpeg_decode.json", "p": "jpeg_split.json", "x": "jpeg_crop.json",
                                                "w": "jpeg_split_crop.json"}[min(groups[0])])
    assert torch.cuda.is_available(), "needs the GPU"
    torch.cuda.set_device(0)
    res = {}
    if os.path.exists(a.out):
        with open(a.out) as fh:
            res = json.loads(fh.read())
    res.update({"batch": a.batch, "rounds": a.rounds, "device": torch.cuda.get_device_name(0), "source_hash": L.source_hash(),
                "host_cpus": DM.default_threads()})
    if "a" in parts:
        res["a_prepare_host"] = part_a(a.batch, a.rounds)
    if "b" in parts:
        res["b_decode_launch"] = part_b(a.batch, a.rounds, a.iters, a.warmup)
    if "c" in parts:
        res["c_pipeline"] = part_c(a.batch, a.rounds, a.steps, 8)
    if "s" in parts:
        res["s_split_launch"] = part_s(a.batch, a.rounds, a.iters, a.warmup, a.sets.split(","))
        res["split_defaults"] = {"seg_bits": DM.JPEG_SPLIT_SEG_BITS, "rounds": DM.JPEG_SPLIT_ROUNDS, "min_seg": 16}
    if "p" in parts:
        res["p_pipeline"] = part_c(a.batch, a.rounds, a.steps, 8, PIPELINE_SPLIT)
        res["split_defaults"] = {"seg_bits": DM.JPEG_SPLIT_SEG_BITS, "rounds": DM.JPEG_SPLIT_ROUNDS, "min_seg": 16}
    if "x" in parts:
        res["x_crop_launch"] = part_x(a.batch, a.rounds, a.iters, a.warmup)
    if "y" in parts:
        res["y_pipeline"] = part_c(a.batch, a.rounds, a.steps, 8, PIPELINE_CROP)
    if "z" in parts:
        res["z_split_crop_launch"] = part_z(a.batch, a.rounds, a.iters, a.warmup)
    if "w" in parts:
        res["w_pipeline"] = part_c(a.batch, a.rounds, a.steps, 8, PIPELINE_SPLIT_CROP)
    line = json.dumps(res)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
