#!/usr/bin/env python
"""Prove that a source-only refactor left the machine code alone: per csrc/*.hip, compile the file as of REV and as of the working
tree to gfx950 device assembly with build.py's flags (RGBNM_HIPCC_FLAGS included) plus the file's own `// hipcc-flags:` line, and
compare the two after dropping what depends on the text and not on the code (.file, .ident, comments, and every line naming
__hip_cuid_, a hash of the translation unit's text).  Prints `identical` or the first differing lines per file; exits 1 on any
difference.  usage: python tools/isa_diff.py [REV] [file.hip ...]   (REV defaults to HEAD~1; no file names = every file)
With --kernels PATTERN (a regular expression over the mangled names) only the bodies of the matching functions are compared, each from
its label to its end, with the function numbers in local labels dropped: for a change that ADDS kernels to a file and must leave
the existing ones what they were."""
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rgb-no-more_amd"))
from build import FLAGS, HIPCC  # noqa: E402

CSRC = os.path.join("rgb-no-more_amd", "csrc")


def asm(tree, name):
    """Normalised device assembly of tree/CSRC/name as a list of lines, or None where the file does not exist in that tree."""
    src = os.path.join(tree, CSRC, name)
    if not os.path.exists(src):
        return None
    with open(src) as fh:
        extra = [w for _, line in zip(range(40), fh) if line.startswith("// hipcc-flags:") for w in line.split(":", 1)[1].split()]
    r = subprocess.run([HIPCC] + FLAGS + extra + ["-S", "--cuda-device-only", src, "-o", "-"], capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"hipcc failed for {src}:\n{r.stderr}")
    out = []
    for line in r.stdout.split("\n"):
        t = re.sub(r"\s*;.*$", "", line).rstrip()
        if t and "__hip_cuid_" not in t and not re.match(r"\s*\.(file|ident)\b", t):
            out.append(t)
    return out


def bodies(lines, pattern):
    """name -> instruction lines of every function whose mangled name matches; local labels lose their function number."""
    out, name = {}, None
    for t in lines or []:
        m = re.match(r"(\w+):$", t)
        if name is None and m and re.search(pattern, m.group(1)) and not m.group(1).startswith("."):
            name = m.group(1)
            out[name] = []
        elif name is not None:
            if re.match(r"\.Lfunc_end\d+:$", t):
                name = None
            else:
                out[name].append(re.sub(r"\.L(BB|tmp|func_begin)\d+_?", r".L\1_", t))
    return out


def main():
    args = sys.argv[1:]
    pattern = None
    if "--kernels" in args:
        k = args.index("--kernels")
        pattern = args[k + 1]
        del args[k:k + 2]
    rev = args.pop(0) if args and not args[0].endswith(".hip") else "HEAD~1"
    names = [os.path.basename(a) for a in args] or sorted(f for f in os.listdir(os.path.join(ROOT, CSRC)) if f.endswith(".hip"))
    bad = 0
    with tempfile.TemporaryDirectory() as old:
        ar = subprocess.run(["git", "-C", ROOT, "archive", rev, CSRC, "include"], check=True, capture_output=True).stdout
        subprocess.run(["tar", "-x", "-C", old], input=ar, check=True)
        with ThreadPoolExecutor(max_workers=4) as ex:
            pairs = ex.map(lambda n: (n, asm(old, n), asm(ROOT, n)), names)
            for n, a, b in pairs:
                if pattern is not None:
                    ka, kb = bodies(a, pattern), bodies(b, pattern)
                    for name in sorted(set(ka) | set(kb)):
                        same, only = ka.get(name) == kb.get(name), name not in ka or name not in kb
                        bad += not same and not only
                        verdict = "identical" if same else f"only in {'the working tree' if name not in ka else rev}" if only else "DIFFERS"
                        print(f"{n:24s} {name:72s} {verdict}  ({len(ka.get(name, []))} -> {len(kb.get(name, []))} lines)")
                    continue
                if a == b:
                    print(f"{n:24s} identical  ({len(b)} lines)")
                    continue
                bad += 1
                if a is None or b is None:
                    print(f"{n:24s} DIFFERS: only in {'the working tree' if a is None else rev}")
                    continue
                i = next((k for k, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
                print(f"{n:24s} DIFFERS from line {i + 1}: {len(a)} -> {len(b)} lines")
                for tag, t in (("-", a), ("+", b)):
                    print("".join(f"    {tag} {l}\n" for l in t[i:i + 6]), end="")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
