#!/usr/bin/env python3
"""Is the device code of every csrc/*.hip the same as at a git revision?

    python tools/isa_same.py [--by-kernel] REV [--cache DIR] [FILE.hip ...]

`git archive REV` goes into a temporary directory; every csrc/*.hip of that tree and of the working tree is compiled to gfx950
assembly with the product flags of rlt_hip/build.py (`-S --cuda-device-only`), and once more per stamps macro that a committed tool
documents, at most 6 compilations at a time.  One line per file and configuration: `same` means the two .s files are equal byte
for byte once the name of the `__hip_cuid_<hash>` symbol is masked.  (hipcc hashes the PATH of the source file into it: four lines
at the end of the file that differ between any two directories.)  A file that only one side has is `not in <side>`.  The exit
status is 0 only when every line says `same`.

--by-kernel is for a change that moves kernels between files: the files named (all, if none is named; each on the sides that have
it) are cut into one record per kernel, and the revision's SET of records is compared with the working tree's, whichever file a
record sits in.  One line per kernel and build: `same`, `DIFFERENT`, `missing` (the tree has lost it) or `new`.  A kernel that
several files of a side emit (a `static` kernel of a shared header) counts once when all its copies are equal - the line says how
many there are - and is DIFFERENT when they are not.  A stamps build of a side holds every named file: compiled with the macro if
its text names the macro, as in the product build if not.

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
STAMPS = {"gemm3.hip": ["RLT_STAMPS"], "gemm6c.hip": ["RLT_STAMPS"], "attention3.hip": ["RLT_STAMPS"],
          "attention6.hip": ["RLT_PP_STAMPS", "RLT_DKV1_STAMPS"], "attention6n.hip": ["RLT_A6N_STAMPS"], "attention6h.hip": ["RLT_A6H_STAMPS"]}


def mask_cuid(text):
    return re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid_", text)


def kernel_records(text):
    """{kernel symbol: its code} of one assembly file - a pure function of the text.  A kernel is a symbol with an `.amdhsa_kernel`
    block; its record runs from the symbol's label to its `.Lfunc_end<n>:` (the block lies in between).  Masked: what tells where
    in its file a function stands and not what it does - the function's ordinal in the local labels (.LBB<n>_<m>, .LJTI<n>_<m>,
    .LCPI<n>_<m>, .Lfunc_begin<n>, .Lfunc_end<n>, and BB<n>_<m> where a comment names a loop header) - and the __hip_cuid_<hash>
    name."""
    kernels = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, flags=re.M))
    records, name, lines = {}, None, []
    for line in text.split("\n"):
        if name is None:
            m = re.match(r"([^\s:]+):", line)
            if m and m.group(1) in kernels:
                name, lines = m.group(1), []
        if name is not None:
            lines.append(line)
            if re.match(r"\.Lfunc_end\d+:", line):
                body = re.sub(r"\.L(BB|JTI|CPI)\d+_", r".L\1#_", "\n".join(lines))
                body = re.sub(r"(?<![\w.])BB\d+_(?=\d)", "BB#_", body)          # `in Loop: Header=BB<n>_<m>` comments
                body = re.sub(r"[ \t]+;", " ;", body)                           # (padded to a column: the ordinal's digits shift them)
                records[name] = mask_cuid(re.sub(r"\.Lfunc_(begin|end)\d+", r".Lfunc_\1#", body))
                name = None
    return records


def compare_records(old, new):
    """[(kernel, verdict, copies in new)] for two lists of kernel_records() dicts, one dict per file of a side"""
    def merged(dicts):
        out = {}
        for d in dicts:
            for k, v in d.items():
                out.setdefault(k, []).append(v)
        return out
    a, b = merged(old), merged(new)
    rows = []
    for k in sorted(set(a) | set(b)):
        if k not in b:
            verdict = "missing"
        elif k not in a:
            verdict = "new"
        else:
            verdict = "same" if len(set(a[k] + b[k])) == 1 else "DIFFERENT"
        rows.append((k, verdict, len(b.get(k, []))))
    return rows


def compile_s(src, macro, out):
    cmd = [B.HIPCC] + B.FLAGS + B.FILE_FLAGS.get(os.path.basename(src), []) + (["-D" + macro] if macro else []) + \
        ["-S", "--cuda-device-only", src, "-o", out]
    res = subprocess.run(cmd, capture_output=True, text=True)
    if res.returncode:
        sys.stderr.write(f"{' '.join(cmd)}\n{res.stderr}\n")
    return res.returncode == 0


def compile_all(jobs):
    """jobs: (source, macro, output); compiles those whose output is not there yet.  {output: compiled or found}"""
    todo = [j for j in jobs if not os.path.exists(j[2])]
    with ThreadPoolExecutor(max_workers=6) as ex:
        ok = dict(zip((j[2] for j in todo), ex.map(lambda j: compile_s(*j), todo)))
    return {j[2]: ok.get(j[2], True) for j in jobs}


def by_file(files, dirs, out_dir, sha):
    configs = [(f, m) for f in files for m in [None] + STAMPS.get(f, [])]

    def path(f, m, side):
        return os.path.join(out_dir, f"{f[:-4]}{'.' + m if m else ''}.{side}.s")
    for f, m in configs:          # the working tree's assembly is never taken from the cache
        if os.path.exists(path(f, m, "tree")):
            os.remove(path(f, m, "tree"))
    ok = compile_all([(os.path.join(dirs[side], f), m, path(f, m, side)) for f, m in configs for side in (sha, "tree")
                      if os.path.exists(os.path.join(dirs[side], f))])
    bad = 0
    print(f"| file | build | lines of assembly | against {sha} |\n|---|---|---|---|")
    for f, m in configs:
        a, b = path(f, m, sha), path(f, m, "tree")
        n = 0
        if a not in ok or b not in ok:
            verdict = f"not in {sha if a not in ok else 'tree'}"
        elif not ok[a] or not ok[b]:
            verdict = "DOES NOT COMPILE"
        else:
            ta, tb = (mask_cuid(open(x).read()) for x in (a, b))
            verdict, n = ("same" if ta == tb else "DIFFERENT"), tb.count("\n")
        bad += verdict != "same"
        print(f"| {f} | {'-D' + m if m else 'product'} | {n} | {verdict} |", flush=True)
    print(f"\n{len(configs) - bad} of {len(configs)} the same")
    return 1 if bad else 0


def by_kernel(files, dirs, out_dir, sha):
    sides = {side: [f for f in files if os.path.exists(os.path.join(d, f))] for side, d in dirs.items()}
    texts = {(side, f): open(os.path.join(dirs[side], f)).read() for side in sides for f in sides[side]}
    macros = [m for m in sorted({m for ms in STAMPS.values() for m in ms}) if any(m in t for t in texts.values())]

    def path(side, f, m):          # a file that does not name the macro: its product build
        m = m if m and m in texts[side, f] else None
        return os.path.join(out_dir, f"{f[:-4]}{'.' + m if m else ''}.{side}.s"), m
    jobs = {}
    for side in sides:
        for f in sides[side]:
            for m in [None] + macros:
                out, m_ = path(side, f, m)
                if side == "tree" and out not in jobs and os.path.exists(out):
                    os.remove(out)
                jobs[out] = (os.path.join(dirs[side], f), m_, out)
    ok = compile_all(list(jobs.values()))
    failed = sorted(o for o, good in ok.items() if not good)
    if failed:
        print("DOES NOT COMPILE: " + ", ".join(os.path.basename(o) for o in failed))
        return 1
    bad = total = 0
    print(f"| kernel | build | in the tree's | against {sha} |\n|---|---|---|---|")
    for m in [None] + macros:
        recs = {side: {f: kernel_records(open(path(side, f, m)[0]).read()) for f in sides[side]} for side in sides}
        where = {}
        for f, d in recs["tree"].items():
            for k in d:
                where.setdefault(k, []).append(f)
        for k, verdict, copies in compare_records(list(recs[sha].values()), list(recs["tree"].values())):
            total += 1
            bad += verdict != "same"
            place = ", ".join(where.get(k, [])) or "-"
            print(f"| `{k}` | {'-D' + m if m else 'product'} | {place} | {verdict} |", flush=True)
    print(f"\n{total - bad} of {total} the same")
    return 1 if bad else 0


def main():
    args = sys.argv[1:]
    cache = None
    if "--cache" in args:
        i = args.index("--cache")
        cache = os.path.abspath(args[i + 1])
        del args[i:i + 2]
    kernels = "--by-kernel" in args
    if kernels:
        args.remove("--by-kernel")
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
        dirs = {sha: os.path.join(old, PKG, "csrc"), "tree": B.CSRC}
        files = only or sorted(set(f for d in dirs.values() for f in os.listdir(d) if f.endswith(".hip")))
        return (by_kernel if kernels else by_file)(files, dirs, out_dir, sha)


if __name__ == "__main__":
    sys.exit(main())
