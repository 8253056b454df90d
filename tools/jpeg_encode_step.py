#!/usr/bin/env python
"""Measure the device JPEG entropy ENCODE (csrc/jpeg_emit.h, jpeg_encode.hip) on one GPU, by the protocol of tools/jpeg_decode_step.py:
B = 256 files of 512 x 512, 4:2:0, quality 90, the same synthetic files, decoded once on the device to get the coefficients.

  (e) dct_manip.encode_jpeg_batch alone (outputs and scratch allocated before) with restart 0, "row" (one interval per MCU row) and 4
      MCUs, at the default stride; beside them a device copy of the coefficient bytes (the floor: the encode has to read them once)
      and, for each of the three, the plain decode launch (dct_manip.launch_jpeg_decode) of the files the encode just wrote.
  (t) the transcode end to end per batch, plan already on the device: split decode of the marker-less files -> encode with "row" ->
      copy of the files to pinned host memory, at a stride of 1.25 x the longest source file.

Warm-up, then ROUNDS interleaved rounds (order reversed every other round); median and min - max.  Writes profiles/jpeg_encode.json
and prints it.
usage: python tools/jpeg_encode_step.py [--rounds 6] [--batch 256] [--iters 5]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from rgb_no_more_amd import dct_manip as DM, lib as L  # noqa: E402
from tools.aug_chain_step import timed, summary  # noqa: E402
from tools.jpeg_decode_step import synth, SETS  # noqa: E402

RESTARTS = {"restart_0": 0, "restart_row": "row", "restart_4mcu": 4}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--iters", type=int, default=5, help="calls per timed block")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg_encode.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    B, grid = a.batch, (64, 64)
    files = synth(64, **SETS["q90"])
    batch = [files[i % 64] for i in range(B)]
    plan = DM.prepare_jpeg_batch(batch, grid=grid)
    assert plan.nbad == 0
    up = DM.upload_jpeg_plan(plan, dev)
    src = DM.alloc_jpeg_out(B, grid, dev)
    src[2].copy_(up[4])
    src[3].copy_(up[5])
    DM.launch_jpeg_decode(plan, up, src)
    torch.cuda.synchronize()
    Y, C, Q, st = src
    assert int(st.min()) == 0
    dims = torch.tensor([[512, 512]] * B, dtype=torch.int32, device=dev)
    coef_bytes = Y.numel() * 2 + C.numel() * 2

    fns, meta, keep = {}, {}, []
    Y2, C2 = torch.empty_like(Y), torch.empty_like(C)

    def copy():
        Y2.copy_(Y)
        C2.copy_(C)

    fns["copy_of_the_coefficients"] = copy
    meta["copy_of_the_coefficients"] = {"bytes_read": coef_bytes}
    stride = DM.jpeg_encode_header_bytes(3, 1) + 64 * (64 * 64 + 2 * 32 * 32)
    for name, restart in RESTARTS.items():
        out = (torch.empty((B, stride), dtype=torch.uint8, device=dev), torch.empty(B, dtype=torch.int32, device=dev),
               torch.empty(B, dtype=torch.int32, device=dev))
        scratch = DM.jpeg_encode_scratch(B, grid, 3, restart, stride, dev)
        DM.encode_jpeg_batch(Y, C, Q, dims, restart, stride, out, scratch)
        torch.cuda.synchronize()
        assert out[2].tolist() == [0] * B
        nb = out[1].tolist()
        host = out[0].cpu()
        written = [host[i, :nb[i]].numpy().tobytes() for i in range(B)]
        back = DM.read_coefficients_bytes(written[5])                     # the host reader gets the coefficients back
        assert torch.equal(back[2], Y[5].cpu()) and torch.equal(back[3], C[5].cpu())
        fns[f"encode_{name}"] = lambda restart=restart, out=out, scratch=scratch: DM.encode_jpeg_batch(Y, C, Q, dims, restart, stride, out, scratch)
        meta[f"encode_{name}"] = {"file_bytes_per_batch": sum(nb), "stride": stride, "scratch_bytes": scratch.numel(), "coefficient_bytes": coef_bytes}
        p2 = DM.prepare_jpeg_batch(written, grid=grid)
        assert p2.nbad == 0
        up2 = DM.upload_jpeg_plan(p2, dev)
        o2 = DM.alloc_jpeg_out(B, grid, dev)
        o2[2].copy_(up2[4])
        o2[3].copy_(up2[5])
        DM.launch_jpeg_decode(p2, up2, o2)
        torch.cuda.synchronize()
        assert torch.equal(o2[0], Y) and torch.equal(o2[1], C) and int(o2[3].min()) == 0      # lossless
        keep.append((p2, up2, o2))
        fns[f"decode_of_{name}"] = lambda p2=p2, up2=up2, o2=o2: DM.launch_jpeg_decode(p2, up2, o2)
        meta[f"decode_of_{name}"] = {"runs": p2.nruns, "file_bytes_per_batch": sum(nb)}

    # (t) the transcode: split decode -> encode "row" -> D2H
    tight = (int(max(len(f) for f in batch) * 1.25) + 1023) // 1024 * 1024
    t_out = (torch.empty((B, tight), dtype=torch.uint8, device=dev), torch.empty(B, dtype=torch.int32, device=dev),
             torch.empty(B, dtype=torch.int32, device=dev))
    t_scratch = DM.jpeg_encode_scratch(B, grid, 3, "row", tight, dev)
    t_dst = DM.alloc_jpeg_out(B, grid, dev)
    t_dst[2].copy_(up[4])
    t_dst[3].copy_(up[5])
    path = torch.empty(B, dtype=torch.int32, device=dev)
    s_scratch = DM.jpeg_split_scratch(plan, None, dev)
    pinned = (torch.empty((B, tight), dtype=torch.uint8, pin_memory=True), torch.empty(B, dtype=torch.int32, pin_memory=True),
              torch.empty(B, dtype=torch.int32, pin_memory=True))

    def transcode():
        DM.launch_jpeg_decode(plan, up, t_dst, split=True, path=path, scratch=s_scratch)
        DM.encode_jpeg_batch(t_dst[0], t_dst[1], t_dst[2], dims, "row", tight, t_out, t_scratch)
        for h, d in zip(pinned, t_out):
            h.copy_(d, non_blocking=True)

    transcode()
    torch.cuda.synchronize()
    assert pinned[2].tolist() == [0] * B and torch.equal(t_dst[0], Y)
    fns["transcode_split_decode_encode_row_d2h"] = transcode
    meta["transcode_split_decode_encode_row_d2h"] = {"stride": tight, "d2h_bytes": B * tight, "source_file_bytes": sum(len(f) for f in batch),
                                                     "file_bytes_per_batch": int(pinned[1].sum())}

    out = summary(timed(list(fns), fns, a.warmup, a.rounds, a.iters))
    for k, v in out.items():
        v.update(meta[k])
        v["images_per_s"] = B / v["ms_median"] * 1e3
        print(f"{k}: {v['ms_median']:.3f} ms ({v['ms_min']:.3f} - {v['ms_max']:.3f}) per batch", file=sys.stderr)
    res = {"batch": B, "rounds": a.rounds, "iters": a.iters, "device": torch.cuda.get_device_name(0), "source_hash": L.source_hash(),
           "size": "512x512 4:2:0 quality 90", "results": out}
    line = json.dumps(res)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
