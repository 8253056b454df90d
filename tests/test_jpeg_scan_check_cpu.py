"""The stand-alone sanitizer build of the marker parser and the one-lane walk (tools/jpeg_scan_check.cpp: csrc/jpeg_scan.h and
jpeg_walk.h compiled for the CPU) on the suite's files, their truncations and mutations.  It is the walk that tools/jpeg_split_check.cpp
and tools/jpeg_crop_check.cpp measure against."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def scan_check(tmp_path_factory):
    """tools/jpeg_scan_check.cpp under the host sanitizers, as a program of its own; skipped where the compiler has no runtime for them."""
    d = tmp_path_factory.mktemp("scan_check")
    exe = str(d / "jpeg_scan_check")
    probe = d / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    flags = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-pthread"]
    r = subprocess.run(["g++"] + flags + [str(probe), "-o", str(d / "probe")], capture_output=True, text=True)
    if r.returncode != 0 or subprocess.run([str(d / "probe")], capture_output=True).returncode != 0:
        pytest.skip("g++ has no address / undefined-behaviour sanitizer runtime here")
    r = subprocess.run(["g++"] + flags + [os.path.join(ROOT, "tools", "jpeg_scan_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    files = d / "files"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "jpeg_scan_files.py"), str(files)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe, sorted(str(f) for f in files.iterdir())


def test_parser_and_walk_under_the_host_sanitizers(scan_check):
    """Every file as given, every truncation of the first two, all 6000 mutations: each is decoded or refused with a status, and the
    sanitizers stay silent."""
    exe, files = scan_check
    r = subprocess.run([exe] + files, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    tally = {}
    for name in ("as given", "truncations", "mutations"):
        m = re.search(name + r":\s+(\d+) decoded, (\d+) refused by the parser, (\d+) by the walk", r.stdout)
        assert m, r.stdout[-2000:]
        tally[name] = tuple(int(v) for v in m.groups())
    wanted = [f for f in files if not f.endswith("_refused.jpg")]
    assert len(wanted) >= 35 and tally["as given"] == (len(wanted), len(files) - len(wanted), 0)
    cut = sum(os.path.getsize(f) for f in files[:2])              # one input per length below the file's own
    assert tally["truncations"] == (0, cut, 0)
    assert min(tally["mutations"]) > 0 and sum(tally["mutations"]) == 6000
    assert re.search(r"checksum [0-9a-f]{16}", r.stdout)
