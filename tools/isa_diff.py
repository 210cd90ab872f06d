#!/usr/bin/env python3
"""usage: tools/isa_diff.py OLD_CSRC NEW_CSRC [--debug] [-D NAME ...] [--only REGEX] [--rename REGEX=REPL ...] [--by-symbol]
Is the device code of two csrc trees the same?  Every .hip of both directories is compiled with the build's flags plus
-S --cuda-device-only; lines naming __hip_cuid_ (a hash of the translation unit) are dropped.  --debug adds -DRDST_DEBUG,
-D further switches (LB3_STAMPS, ...), --only keeps the file names that match.  Per file: `identical`, or the kernels whose
text differs, each with the kernel-resource-usage numbers of both sides (dynamic LDS is not in `LDS Size`).  Exit status 1 if
anything differs or fails to compile.
--rename REGEX=REPL (repeatable) rewrites the OLD side's text before the comparison: a kernel whose symbol changed (a new template
argument, another argument type) is paired with its successor.  Mangled names carry length prefixes: match the mangled text.
--by-symbol pairs the function sections (body and kernel descriptor) and the kernels' metadata entries by symbol over the WHOLE
tree instead of file by file, so code that moved to another file is compared with itself; what lies outside them is not compared.
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


def sections(path, renames=(), local_labels=True):
    """{function symbol: its lines (body and kernel descriptor)}; everything outside a function under ''.
    local_labels=False drops the function's number within its file from the local labels (.LBB7_3 -> .LBB_3)."""
    sec, cur = {"": []}, ""
    for l in open(path):
        if "__hip_cuid_" in l:
            continue
        l = renamed(l, renames)
        if not local_labels:
            l = re.sub(r"(\.L|\b)(BB|JTI|CPI)\d+_", r"\1\2_",re.sub(r"\.Lfunc_(begin|end)\d+", r".Lfunc_\1", l))   # (in comments as well,
            l = re.sub(r"[ \t]+;", " ;", l)                                                                  # and their padding)
        m = re.match(r"\s*\.type\s+(\S+),@function", l) or re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l)
        if m:
            cur = m.group(1)
        sec.setdefault(cur, []).append(l)
        if re.match(r"\s*(\.size\s|\.end_amdhsa_kernel)", l):
            cur = ""
    return sec


def metadata(lines):
    """{'meta ' + kernel symbol: its entry of .amdgpu_metadata} from the lines outside any function"""
    out, cur = {}, None
    for l in lines:
        if re.match(r"  - \.", l):
            cur = []
        elif not l.startswith("    ") or cur is None:
            cur = None
            continue
        cur.append(l)
        m = re.match(r"    \.name:\s+(\S+)", l)
        if m:
            out["meta " + m.group(1)] = cur
    return out


def by_symbol(jobs, tmp, renames):
    """Pool the sections of every file per side and pair them by symbol: a kernel that moved to another file is compared with
    itself.  A symbol emitted by several files (an inline function) is compared as the sorted list of its copies."""
    pool, res, bad = {"old": {}, "new": {}}, {"old": {}, "new": {}}, 0
    for (f, side), job in sorted(jobs.items()):
        r, err = job.result()
        if r is None:
            print(f"{f}: does not compile ({side})\n{err}")
            bad += 1
            continue
        rn = renames if side == "old" else ()
        res[side].update({renamed(k, rn): v for k, v in r.items()})
        sec = sections(os.path.join(tmp, f"{side}_{f}.s"), rn, local_labels=False)
        sec.update(metadata(sec.pop("")))
        for k, v in sec.items():
            pool[side].setdefault(k, []).append((v, f))
    keys = sorted(set(pool["old"]) | set(pool["new"]))
    names = demangle([k.replace("meta ", "") for k in keys])
    moved = 0
    for k in keys:
        o, n = sorted(pool["old"].get(k, [])), sorted(pool["new"].get(k, []))
        name = ("metadata of " if k.startswith("meta ") else "") + names[k.replace("meta ", "")]
        if [t for t, _ in o] == [t for t, _ in n]:
            if [f for _, f in o] != [f for _, f in n] and not k.startswith("meta "):
                moved += 1
                print(f"  moved, identical: {name}: {','.join(f for _, f in o)} -> {','.join(f for _, f in n)}")
            continue
        bad += 1
        print(f"  DIFFERS: {name} ({','.join(f for _, f in o) or 'absent'} -> {','.join(f for _, f in n) or 'absent'})")
        for side in ("old", "new"):
            if k in res[side]:
                print(f"    {side}: " + "  ".join(f"{q.split(' [')[0]}={res[side][k].get(q)}" for q in RES))
    nk = sum(1 for k in keys if k.startswith("meta "))
    print(f"{len(keys) - nk} function sections and {nk} kernel metadata entries paired by symbol over {len({f for f, _ in jobs})} files: "
          f"{bad} differ, {moved} moved between files and are identical")
    return bad


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
    ap.add_argument("--by-symbol", action="store_true")
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
        print(f"# {' '.join([*FLAGS, *extra])}: {a.old} -> {a.new}" + (" (by symbol)" if a.by_symbol else ""))
        if a.by_symbol:
            return 1 if by_symbol(jobs, tmp, renames) else 0
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
