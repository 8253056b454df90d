#!/usr/bin/env python
"""Time the batched DFT-plane kernels (csrc/dft_ops.hip) against the per-sample tensor path, on one GPU, configurations interleaved.
B = 256, S = 28, the reference's default op list (REFERENCE_DEFAULT_OPS: Rotate / ShearX / ShearY are 3 of its 16), num_ops = 2,
magnitude 3, one fixed draw of every sample's ops for all configurations:

  (a) randaugment  RandAugment_dct on int16 28-block grids, dft_kernel=True against dft_kernel=False (the tensor path), the same
                   per-sample op lists
  (b) fused        TrainTransform_DCT(dft_ops=True) on the reference's default list against the same transform on DEFAULT_OPS (the
                   list without the three ops: what the fused transform cost before), explicit parameters drawn once each
  (c) gemm         the four GEMM launches of the calls of (a), bracketed with device events by the library (trace tag 10):
                   achieved f32 FLOP/s over 12 real N^3 products per plane

Every configuration runs WARMUP calls, then ROUNDS interleaved blocks of ITERS timed calls (order reversed every other round),
device events around each block after a synchronise.  Reported per configuration: median / min / max over the blocks' per-call
times, and per comparison the difference of the medians next to the spread (the largest max - min of the two).  The times include
the host work of a call (packing the parameters; for the tensor path its few dozen launches per plane): that is what a training
step waits for.  Writes profiles/dft_ops.json and prints it.
usage: python tools/dft_ops_step.py [--iters 5] [--warmup 3] [--rounds 6] [--batch 256]
"""
import argparse
import ctypes
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from rgb_no_more_amd import custom_transforms as CT, lib as L  # noqa: E402
from bench import synth_coefficients  # noqa: E402
from tools.aug_chain_step import timed, summary, compare  # noqa: E402

TR_DFT = 10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5, help="calls per timed block")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dft_ops.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    B, S = a.batch, 28
    res = {"batch": B, "size": S, "num_ops": 2, "magnitude": 3, "ops_list": list(CT.REFERENCE_DEFAULT_OPS), "iters": a.iters,
           "warmup": a.warmup, "rounds": a.rounds, "device": torch.cuda.get_device_name(0), "source_hash": L.source_hash()}
    Yq, Cq, quant = synth_coefficients(B, dev, 1234)

    # ---- int16 28-block grids for (a): the crop / resize / flip stage of the default transform, no ops
    torch.manual_seed(1234)
    first = CT.TrainTransform_DCT(size=S, out_dtype=torch.int16)
    Y28, C28 = first(Yq, Cq, quant, params=[dict(p, ops=[]) for p in first.sample_params(B, 64, 64)])
    meta = CT.magnitude_table(11, (S, S))
    chosen = [CT.sample_ops(CT.REFERENCE_DEFAULT_OPS, 2, 3, meta, S) for _ in range(B)]
    res["samples_with_a_dft_op"] = sum(any(o[0] in CT.DFT_OPS for o in c) for c in chosen)
    res["dft_jobs_per_pass"] = [sum(len(c) > k and c[k][0] in CT.DFT_OPS for c in chosen) for k in range(2)]
    ra = {"kernel": CT.RandAugment_dct(num_ops=2, magnitude=3, dft_kernel=True), "tensor": CT.RandAugment_dct(num_ops=2, magnitude=3)}
    fns = {k: (lambda m=m: m((Y28, C28), per_sample_ops=chosen)) for k, m in ra.items()}
    (ky, kc), (ty, tc) = fns["kernel"](), fns["tensor"]()
    dy, dc = (ky.int() - ty.int()).abs(), (kc.int() - tc.int()).abs()
    res["kernel_vs_tensor"] = {"max_abs_diff": int(max(dy.max(), dc.max())), "share_differing_Y": float((dy > 0).float().mean()),
                               "share_differing_C": float((dc > 0).float().mean())}
    out = summary(timed(list(fns), fns, a.warmup, a.rounds, a.iters))
    out["kernel_vs_tensor"] = compare(out, "tensor", "kernel")
    res["randaugment"] = out
    print("randaugment: " + ", ".join(f"{k} {out[k]['ms_median']:.3f} ms" for k in fns), file=sys.stderr)

    # ---- (c) the GEMM launches alone
    lib = L.lib()
    L.check(lib.rgbnm_trace_reserve(64), "trace_reserve")
    L.set_option("trace", 1 << TR_DFT)
    for _ in range(4):
        fns["kernel"]()
    torch.cuda.synchronize()
    L.set_option("trace", 0)
    ms, fl, by, n = ctypes.c_double(), ctypes.c_double(), ctypes.c_double(), ctypes.c_int()
    L.check(lib.rgbnm_trace_collect(TR_DFT, ctypes.byref(ms), ctypes.byref(fl), ctypes.byref(by), ctypes.byref(n)), "trace_collect")
    res["gemm"] = {"calls": n.value, "ms_total": ms.value, "flops_total": fl.value,
                   "tflops_f32": fl.value / (ms.value * 1e-3) / 1e12 if ms.value > 0 else None,
                   "ms_per_randaugment_call": ms.value / 4}
    print(f"gemm: {res['gemm']['tflops_f32']} TFLOP/s f32 over {n.value} calls", file=sys.stderr)

    # ---- (b) the fused transform with and without the three ops in its list
    fused = {"with_dft_ops": CT.TrainTransform_DCT(size=S, num_ops=2, magnitude=3, ops_list=CT.REFERENCE_DEFAULT_OPS, dft_ops=True),
             "default_ops": CT.TrainTransform_DCT(size=S, num_ops=2, magnitude=3, ops_list=CT.DEFAULT_OPS)}
    params = {}
    for k, t in fused.items():
        torch.manual_seed(1234)
        params[k] = t.sample_params(B, 64, 64)
    res["fused_samples_with_a_dft_op"] = sum(any(o[0] in CT.DFT_OPS for o in p["ops"]) for p in params["with_dft_ops"])
    fns = {k: (lambda k=k: fused[k](Yq, Cq, quant, params=params[k])) for k in fused}
    out = summary(timed(list(fns), fns, a.warmup, a.rounds, a.iters))
    out["with_vs_without"] = compare(out, "default_ops", "with_dft_ops")
    res["fused"] = out
    print("fused: " + ", ".join(f"{k} {out[k]['ms_median']:.3f} ms" for k in fns), file=sys.stderr)

    line = json.dumps(res)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
