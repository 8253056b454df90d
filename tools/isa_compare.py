#!/usr/bin/env python3
"""Compare the gfx950 kernels of two assembly listings (hipcc -S --cuda-device-only) body by body, ignoring symbol names, label
numbers and comments, and list VGPRs / scratch / spills per kernel from the listing's own metadata.

    tools/isa_compare.py before/attention_v2.s after/attention_v2.s

A kernel of the first file counts as kept when some kernel of the second file has the same instruction stream.  Needs no GPU."""
import re
import subprocess
import sys


def kernels(path):
    text = open(path).read()
    names = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M)
    out = {}
    for n in names:
        m = re.search(r"^%s:[^\n]*\n(.*?)^\.Lfunc_end\d+:" % re.escape(n), text, re.M | re.S)
        body = []
        for line in m.group(1).splitlines():
            line = line.split(";")[0].rstrip()
            if not line.strip():
                continue
            line = re.sub(r"\.LBB\d+_", ".LBB_", line)
            line = re.sub(r"_Z[\w$.]+", "SYM", line)
            body.append(line)
        tail = text[m.end():m.end() + 4000]
        meta = {k: int(re.search(r"; %s: (\d+)" % k, tail).group(1)) for k in ("NumVgprs", "NumAgprs", "ScratchSize")}
        meta["spill"] = int(re.search(r"\.vgpr_spill_count:\s+(\d+)", text[text.index(".name:           " + n):]).group(1))
        out[n] = ("\n".join(body), meta)
    return out


def demangle(names):
    for tool in ("llvm-cxxfilt", "c++filt"):
        try:
            r = subprocess.run([tool] + names, capture_output=True, text=True, check=True)
            return [re.sub(r"\(anonymous namespace\)::", "", s[5:].rsplit("(", 1)[0] if s.startswith("void ") else s)
                    for s in r.stdout.splitlines()]
        except Exception:
            continue
    return names


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    bodies_b = {}
    for n, (body, _) in b.items():
        bodies_b.setdefault(body, []).append(n)
    same = 0
    for n, (body, meta) in a.items():
        if body in bodies_b:
            same += 1
        else:
            print("DIFFERENT:", demangle([n])[0])
    print(f"{sys.argv[1]}: {len(a)} kernels, {same} with an identical instruction stream in {sys.argv[2]} ({len(b)} kernels)")
    nb = list(b)
    for n, d in sorted(zip(nb, demangle(nb)), key=lambda t: t[1]):
        m = b[n][1]
        print(f"  {d:100s} vgpr {m['NumVgprs']:3d} agpr {m['NumAgprs']:3d} scratch {m['ScratchSize']:4d} spills {m['spill']}")
    return 0 if same == len(a) else 1


if __name__ == "__main__":
    sys.exit(main())
