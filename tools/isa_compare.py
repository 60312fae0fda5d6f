#!/usr/bin/env python3
"""Device assembly of two source trees, function by function: did a change move a kernel?

    tools/isa_compare.py <old tree> <new tree> [--work DIR] [--gone NAME ...] unit [unit ...]

e.g.  git worktree add /tmp/parent HEAD^ && tools/isa_compare.py /tmp/parent . wh_d4c wh_cheaptrick wh_synthesis wh_timebase

Each named unit that exists in a tree (python-world_amd/csrc/<unit>.hip) is compiled with that tree's own build.py FLAGS
and TU_FLAGS plus -save-temps=obj; the gfx950 .s is split into functions (every __global__ symbol and every device function
that was not inlined), and what depends only on a function's position in its file is normalised away: the numbers of the
.LBB / .Ltmp / .Lfunc labels, `;` comments, blank and debug lines.  Functions are matched across units by demangled name
(without namespaces: a kernel may have changed files, a type its namespace).  The kernel descriptor is part of a kernel's
text.  Per function: identical, or the first differing line and both sides' registers, LDS, scratch and instruction count.
--gone NAME (repeatable) declares a function of the old tree — its short demangled name as this tool prints it — as removed
on purpose: it is listed under a heading of its own and does not count against the run.
Needs hipcc, no GPU.  Exit status 1 if any function differs, exists on one side only without having been declared gone, or
was declared gone and is not (or was never there)."""
import importlib.util
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

DEBUG = re.compile(r"^\s*\.(loc|file|cfi_\w+|ident|addrsig\w*)\b")
DESCR = ("next_free_vgpr", "next_free_sgpr", "group_segment_fixed_size", "private_segment_fixed_size")


def compile_units(tree, units, work):
    spec = importlib.util.spec_from_file_location("_b" + str(abs(hash(work))), os.path.join(tree, "python-world_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    os.makedirs(work, exist_ok=True)

    def one(u):
        src = os.path.join(tree, "python-world_amd", "csrc", u + ".hip")
        if not os.path.exists(src):
            return None
        cmd = [b._hipcc()] + b.FLAGS + b.TU_FLAGS.get(u + ".hip", []) + ["-save-temps=obj", "-c", src, "-o", os.path.join(work, u + ".o")]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            sys.exit("hipcc failed on %s\n%s" % (src, r.stderr[-3000:]))
        return os.path.join(work, "%s-hip-amdgcn-amd-amdhsa-%s.s" % (u, b.ARCH))

    with ThreadPoolExecutor(max_workers=4) as ex:
        return [s for s in ex.map(one, units) if s]


def demangle(symbols):
    symbols = sorted(symbols)
    if not symbols:
        return {}
    out = subprocess.run(["c++filt"], input="\n".join(symbols) + "\n", capture_output=True, text=True).stdout.splitlines()
    short = lambda d: re.sub(r"\(anonymous namespace\)::|\bwh::", "", d).replace("void ", "")
    return {s: short(d) for s, d in zip(symbols, out)}


def functions(path):
    """{short demangled name: {"text": [normalised lines], descriptor fields, "insts": n}} of one device .s"""
    lines = open(path).read().splitlines()
    names = demangle(set(re.findall(r"_Z\w+", "\n".join(lines))))
    funcs, cur, body = {}, None, []
    for ln in lines:
        m = re.match(r"\s*\.type\s+(\S+),@function", ln)
        if m and cur is None:
            cur, body = m.group(1), []
            continue
        if cur is None:
            continue
        if re.match(r"\s*\.size\s+" + re.escape(cur) + ",", ln):
            funcs[names.get(cur, cur)] = body
            cur = None
            continue
        ln = ln.split(";")[0].rstrip()
        if not ln.strip() or DEBUG.match(ln):
            continue
        ln = re.sub(r"\.LBB\d+_", ".LBB_", ln)
        ln = re.sub(r"\.Lfunc_(begin|end)\d+", r".Lfunc_\1", ln)
        ln = re.sub(r"_Z\w+", lambda s: names.get(s.group(0), s.group(0)), ln)
        body.append(ln)
    out = {}
    for name, body in funcs.items():
        tmp = {}  # .Ltmp numbers run through the file: renumber in order of appearance
        text = [re.sub(r"\.Ltmp\d+", lambda s: tmp.setdefault(s.group(0), ".Ltmp%d" % len(tmp)), ln) for ln in body]
        rec = {"text": text, "insts": sum(1 for ln in text if re.match(r"^\t[a-z]\w*(\s|$)", ln))}
        for ln in text:
            m = re.match(r"\s*\.amdhsa_(\w+)\s+(\S+)", ln)
            if m and m.group(1) in DESCR:
                rec[m.group(1)] = m.group(2)
        out[name] = rec
    return out


def describe(rec):
    if "next_free_vgpr" not in rec:
        return "device function, %d instructions" % rec["insts"]
    return "vgpr %s sgpr %s lds %s scratch %s, %d instructions" % tuple([rec[k] for k in DESCR] + [rec["insts"]])


def main():
    args = sys.argv[1:]
    work = None
    if "--work" in args:
        i = args.index("--work")
        work = args[i + 1]
        del args[i:i + 2]
    gone = []
    while "--gone" in args:
        i = args.index("--gone")
        gone.append(args[i + 1])
        del args[i:i + 2]
    if len(args) < 3:
        sys.exit(__doc__)
    old, new, units = os.path.abspath(args[0]), os.path.abspath(args[1]), args[2:]
    work = work or tempfile.mkdtemp(prefix="isa_compare_")
    sides = []
    for tag, tree in (("old", old), ("new", new)):
        fs = {}
        for s in compile_units(tree, units, os.path.join(work, tag)):
            for name, rec in functions(s).items():
                rec["unit"] = os.path.basename(s).split("-hip-")[0]
                fs[name] = rec
        sides.append(fs)
    a, b = sides
    bad = 0
    print("units: %s" % " ".join(units))
    removed = [n for n in gone if n in a and n not in b]
    if gone:
        print("declared removed (%d):" % len(gone))
        for n in gone:
            if n in removed:
                print("gone       %s  (%s; %s)" % (n, a[n]["unit"], describe(a[n])))
            else:
                bad += 1
                print("NOT GONE   %s  (%s)" % (n, "still in the new tree" if n in b else "not in the old tree"))
    for name in sorted(set(a) | set(b)):
        if name in removed:
            continue
        if name not in a or name not in b:
            bad += 1
            print("ONLY %s  %s  (%s)" % ("old" if name in a else "new", name, (a.get(name) or b.get(name))["unit"]))
            continue
        ra, rb = a[name], b[name]
        where = ra["unit"] if ra["unit"] == rb["unit"] else "%s -> %s" % (ra["unit"], rb["unit"])
        if ra["text"] == rb["text"]:
            print("identical  %s  (%s; %s)" % (name, where, describe(ra)))
            continue
        bad += 1
        i = next((i for i, (x, y) in enumerate(zip(ra["text"], rb["text"])) if x != y), min(len(ra["text"]), len(rb["text"])))
        print("DIFFERS    %s  (%s)" % (name, where))
        print("    old: %s\n    new: %s" % (describe(ra), describe(rb)))
        print("    first difference at normalised line %d:\n      old: %s\n      new: %s" % (
            i, ra["text"][i].strip() if i < len(ra["text"]) else "<end>", rb["text"][i].strip() if i < len(rb["text"]) else "<end>"))
    total = len((set(a) | set(b)) - set(removed))
    print("%d functions, %d identical, %d not; %d removed as declared" % (total, total - bad, bad, len(removed)))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
