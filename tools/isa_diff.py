#!/usr/bin/env python3
"""usage: tools/isa_diff.py OLD_CSRC NEW_CSRC [--debug] [-D NAME ...] [--only REGEX] [--rename REGEX=REPL ...]
Is the device code of two csrc trees the same?  Every .hip of both directories is compiled with the build's flags plus
-S --cuda-device-only; lines naming __hip_cuid_ (a hash of the translation unit) are dropped.  --debug adds -DRDST_DEBUG,
-D further switches (LB3_STAMPS, ...), --only keeps the file names that match.  Per file: `identical`, or the kernels whose
text differs, each with the kernel-resource-usage numbers of both sides (dynamic LDS is not in `LDS Size`).  Exit status 1 if
anything differs or fails to compile.
--rename REGEX=REPL (repeatable) rewrites the OLD side's text before the comparison: a kernel whose symbol changed (a new template
argument, another argument type) is paired with its successor.  Mangled names carry length prefixes: match the mangled text.
OLD_CSRC is a directory: take the parent's from `git worktree add` or `git archive` (it needs ../../include next to it)."""
import argparse, os, re, subprocess, sys, tempfile
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rdst_amd.build import FLAGS, HIPCC

RES = ["VGPRs", "AGPRs", "VGPRs Spill", "SGPRs Spill", "ScratchSize [bytes/lane]", "LDS Size [bytes/block]"]


def compile_one(src, out, extra):
    cmd = [HIPCC, *FLAGS, *extra, "-S", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", src, "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        return None, r.stderr[-2000:]
    res, cur = {}, None
    for l in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", l)
        if m:
            cur = res.setdefault(m.group(1), {})
        for k in RES:
            m = re.search(r"    " + re.escape(k) + r": (\d+)", l)
            if m and cur is not None:
                cur[k] = int(m.group(1))
    return res, ""


def renamed(text, renames):
    for rx, repl in renames:
        text = rx.sub(repl, text)
    return text


def sections(path, renames=()):
    """{function symbol: its lines (body and kernel descriptor)}; everything outside a function under ''"""
    sec, cur = {"": []}, ""
    for l in open(path):
        if "__hip_cuid_" in l:
            continue
        l = renamed(l, renames)
        m = re.match(r"\s*\.type\s+(\S+),@function", l) or re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l)
        if m:
            cur = m.group(1)
        sec.setdefault(cur, []).append(l)
        if re.match(r"\s*(\.size\s|\.end_amdhsa_kernel)", l):
            cur = ""
    return sec


def demangle(names):
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    except OSError:
        out = names
    return {n: re.sub(r"\(.*", "", d.replace("(anonymous namespace)::", "").replace("void ", "")) for n, d in zip(names, out)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--debug", action="store_true")
    ap.add_argument("-D", dest="defs", action="append", default=[])
    ap.add_argument("--only", default=".")
    ap.add_argument("--rename", action="append", default=[], metavar="REGEX=REPL")
    a = ap.parse_args()
    renames = [(re.compile(rx), repl) for rx, _, repl in (r.partition("=") for r in a.rename)]
    extra = (["-DRDST_DEBUG"] if a.debug else []) + ["-D" + d for d in a.defs]
    files = sorted({f for d in (a.old, a.new) for f in os.listdir(d) if f.endswith(".hip") and re.search(a.only, f)})
    bad = 0
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(max_workers=16) as ex:
        jobs = {}
        for f in files:
            for side, d in (("old", a.old), ("new", a.new)):
                src = os.path.join(d, f)
                if os.path.exists(src):
                    jobs[f, side] = ex.submit(compile_one, src, os.path.join(tmp, f"{side}_{f}.s"), extra)
        print(f"# {' '.join([*FLAGS, *extra])}: {a.old} -> {a.new}")
        for f in files:
            if (f, "old") not in jobs or (f, "new") not in jobs:
                print(f"{f}: only in {'new' if (f, 'new') in jobs else 'old'}")
                bad += 1
                continue
            (ro, eo), (rn, en) = jobs[f, "old"].result(), jobs[f, "new"].result()
            if ro is None or rn is None:
                print(f"{f}: does not compile ({'old' if ro is None else 'new'})\n{eo or en}")
                bad += 1
                continue
            ro = {renamed(k, renames): v for k, v in ro.items()}
            so, sn = sections(os.path.join(tmp, f"old_{f}.s"), renames), sections(os.path.join(tmp, f"new_{f}.s"))
            diff = [k for k in sorted(set(so) | set(sn)) if so.get(k) != sn.get(k)]
            if not diff:
                print(f"{f}: identical")
                continue
            bad += 1
            names = demangle(diff)
            print(f"{f}: {len(diff)} of {len(set(so) | set(sn))} sections differ")
            for k in diff:
                print(f"  {names[k] or '(outside any function)'}")
                for side, r in (("old", ro), ("new", rn)):
                    if k in r:
                        print(f"    {side}: " + "  ".join(f"{q.split(' [')[0]}={r[k].get(q)}" for q in RES))
                if k in ro and k in rn:
                    print("    resources " + ("equal" if ro[k] == rn[k] else "DIFFER"))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
