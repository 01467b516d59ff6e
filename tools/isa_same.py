#!/usr/bin/env python3
"""Is the device code of every csrc/*.hip the same as at a git revision?

    python tools/isa_same.py REV [--cache DIR] [FILE.hip ...]

`git archive REV` goes into a temporary directory; every csrc/*.hip of that tree and of the working tree is compiled to gfx950
assembly with the product flags of rlt_hip/build.py (`-S --cuda-device-only`), and once more per stamps macro that a committed tool
documents, at most 6 compilations at a time.  One line per file and configuration: `same` means the two .s files are equal byte
for byte once the name of the `__hip_cuid_<hash>` symbol is masked.  (hipcc hashes the PATH of the source file into it: four lines
at the end of the file that differ between any two directories.)  The exit status is 0 only when every line says so.

Both sides are compiled with the WORKING TREE's FLAGS / FILE_FLAGS: a change to the flags in rlt_hip/build.py goes unnoticed here.

With --cache DIR the assembly is kept there, and the revision's files found there are not compiled again."""
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "ranked-list-truncation_amd"
sys.path.insert(0, os.path.join(REPO, PKG))
from rlt_hip import build as B  # noqa: E402

# the diagnostic builds that tools/bench_kernels.py and tools/pp_stamps.py ask for
STAMPS = {"gemm.hip": ["RLT_STAMPS"], "attention3.hip": ["RLT_STAMPS"], "attention6.hip": ["RLT_PP_STAMPS", "RLT_DKV1_STAMPS"],
          "attention6n.hip": ["RLT_A6N_STAMPS"], "attention6h.hip": ["RLT_A6H_STAMPS"]}


def compile_s(src, macro, out):
    cmd = [B.HIPCC] + B.FLAGS + B.FILE_FLAGS.get(os.path.basename(src), []) + (["-D" + macro] if macro else []) + \
        ["-S", "--cuda-device-only", src, "-o", out]
    res = subprocess.run(cmd, capture_output=True, text=True)
    if res.returncode:
        sys.stderr.write(f"{' '.join(cmd)}\n{res.stderr}\n")
    return res.returncode == 0


def main():
    args = sys.argv[1:]
    cache = None
    if "--cache" in args:
        i = args.index("--cache")
        cache = os.path.abspath(args[i + 1])
        del args[i:i + 2]
    rev, only = args[0], args[1:]
    sha = subprocess.run(["git", "rev-parse", "--short=12", rev], cwd=REPO, check=True, capture_output=True, text=True).stdout.strip()
    with tempfile.TemporaryDirectory() as tmp:
        out_dir = cache or os.path.join(tmp, "s")
        os.makedirs(out_dir, exist_ok=True)
        old = os.path.join(tmp, "old")
        os.makedirs(old)
        tar = subprocess.Popen(["git", "archive", rev, PKG + "/csrc", "include"], cwd=REPO, stdout=subprocess.PIPE)
        subprocess.run(["tar", "-x", "-C", old], stdin=tar.stdout, check=True)
        assert tar.wait() == 0
        old_csrc = os.path.join(old, PKG, "csrc")
        files = only or sorted(set(f for d in (B.CSRC, old_csrc) for f in os.listdir(d) if f.endswith(".hip")))
        configs = [(f, m) for f in files for m in [None] + STAMPS.get(f, [])]
        jobs = []
        for f, m in configs:
            stem = f[:-4] + ("." + m if m else "")
            a, b = os.path.join(out_dir, f"{stem}.{sha}.s"), os.path.join(out_dir, f"{stem}.tree.s")
            if not os.path.exists(a):
                jobs.append((os.path.join(old_csrc, f), m, a))
            jobs.append((os.path.join(B.CSRC, f), m, b))
        with ThreadPoolExecutor(max_workers=6) as ex:
            ok = dict(zip((j[2] for j in jobs), ex.map(lambda j: os.path.exists(j[0]) and compile_s(*j), jobs)))
        bad = 0
        print(f"| file | build | lines of assembly | against {sha} |\n|---|---|---|---|")
        for f, m in configs:
            stem = f[:-4] + ("." + m if m else "")
            a, b = os.path.join(out_dir, f"{stem}.{sha}.s"), os.path.join(out_dir, f"{stem}.tree.s")
            if not ok.get(a, True) or not ok[b]:
                verdict, n = "DOES NOT COMPILE", 0
            else:
                ta, tb = (re.sub(rb"__hip_cuid_[0-9a-f]+", b"__hip_cuid_", open(x, "rb").read()) for x in (a, b))
                verdict, n = ("same" if ta == tb else "DIFFERENT"), tb.count(b"\n")
            bad += verdict != "same"
            print(f"| {f} | {'-D' + m if m else 'product'} | {n} | {verdict} |", flush=True)
        print(f"\n{len(configs) - bad} of {len(configs)} the same")
        return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
