#!/usr/bin/env python
"""Write the JPEG files of the device-decode tests (tests/jpeg_cases.py: the golden g1 files, the Pillow-made ones and the synthetic
ones of tests/jpeg_writer.py) into a directory, as input of the stand-alone sanitizer check tools/jpeg_scan_check.cpp.  A file whose
name ends in _refused is one the parser must refuse.    python tools/jpeg_scan_files.py DIR"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import jpeg_cases as JC  # noqa: E402


def main():
    out = sys.argv[1]
    os.makedirs(out, exist_ok=True)
    files = {**JC.pillow_files(), **JC.g1_files()}
    files.update({f"batch{i}": b for i, b in enumerate(JC.small_batch())})
    files.update({k: s.data for k, s in JC.synthetic().items()})
    keep = ("many_gray0", "many_gray1", "many_420_1", "many_420_2")               # gray and colour, both table families
    files.update({s.name: s.data for s in JC.many_runs() if s.name in keep})
    files["three_scans_refused"] = JC.three_scans().data
    files["over_subscribed_refused"] = JC.over_subscribed()
    # rst_blocks2 and g40x56 sort first: the two files whose every truncation length is tried (restart markers; one component)
    order = ["rst_blocks2", "g40x56"] + sorted(k for k in files if k not in ("rst_blocks2", "g40x56"))
    for j, k in enumerate(order):
        with open(os.path.join(out, f"{j:02d}_{k}.jpg"), "wb") as fh:
            fh.write(files[k])
    print(f"{len(order)} files in {out}")


if __name__ == "__main__":
    main()
