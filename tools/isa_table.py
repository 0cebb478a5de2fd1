#!/usr/bin/env python3
"""Per-kernel table of a gfx950 device assembly file (hipcc <the Makefile's HIPFLAGS> --cuda-device-only -S x.hip -o x.s).

  isa_table.py x.s        one line per kernel: LDS bytes, VGPRs, SGPRs, scratch bytes, VGPR / SGPR spills, instruction
                          count, a short hash of the instruction text, the demangled name
  isa_table.py a.s b.s    the kernels that disappear, appear or differ from a to b; a differing kernel whose LDS size
                          changed or whose VGPRs, scratch or spills went up is marked WORSE (exit status 1 if any is)

The hash covers the instructions only: comments and directives are stripped, block labels renumbered in order of
appearance.  Figures come from the compiler's own metadata note.  The tool counts and hashes; it knows no instruction.
"""
import hashlib
import re
import shutil
import subprocess
import sys

META = {"group_segment_fixed_size": "lds", "vgpr_count": "vgpr", "sgpr_count": "sgpr", "private_segment_fixed_size": "scratch",
        "vgpr_spill_count": "vspill", "sgpr_spill_count": "sspill"}
COLS = ["lds", "vgpr", "sgpr", "scratch", "vspill", "sspill", "insts", "hash"]


def parse(path):
    text = open(path).read().splitlines()
    kernels, cur = {}, None
    for ln in text:  # metadata: keys of a kernel sit at indent 4 ("  - " opens one), those of its arguments deeper
        m = re.match(r"^(  - |    )\.(\w+):\s*(.*)$", ln)
        if not m:
            continue
        if m.group(1) == "  - ":
            cur = {}
        if cur is None:
            continue
        key, val = m.group(2), m.group(3).strip("'\" ")
        if key == "name":
            kernels[val] = cur
        elif key in META:
            cur[META[key]] = int(val)
    body = None
    for ln in text:
        m = re.match(r"^([A-Za-z_][\w$.]*):", ln)
        if m and m.group(1) in kernels:
            name, body, labels = m.group(1), [], {}
            continue
        if body is None:
            continue
        s = ln.split(";")[0].strip()
        if s.startswith(".Lfunc_end"):
            kernels[name]["insts"] = sum(1 for b in body if not b.endswith(":"))
            kernels[name]["hash"] = hashlib.sha1("\n".join(body).encode()).hexdigest()[:12]
            body = None
        elif s and (not s.startswith(".") or s.startswith(".LBB")):
            body.append(re.sub(r"\.LBB\d+_\d+", lambda b: labels.setdefault(b.group(0), ".L%d" % len(labels)), s))
    return kernels


def demangle(names):
    tool = shutil.which("llvm-cxxfilt") or shutil.which("c++filt") or shutil.which("llvm-cxxfilt", path="/opt/rocm/llvm/bin")
    if not tool:
        return dict(zip(names, names))
    out = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()
    short = [re.sub(r"\(.*$", "", d.replace("(anonymous namespace)::", "").replace("void ", "", 1)) for d in out]  # no argument list
    return dict(zip(names, short))


def row(k):
    return " ".join(f"{k.get(c, '?'):>{12 if c == 'hash' else 7}}" for c in COLS)


def main(argv):
    if len(argv) not in (2, 3):
        sys.exit(__doc__)
    tabs = [parse(p) for p in argv[1:]]
    nice = demangle(sorted(set().union(*tabs)))
    head = " ".join(f"{c:>{12 if c == 'hash' else 7}}" for c in COLS)
    if len(tabs) == 1:
        print(head + "  kernel")
        for n in sorted(tabs[0], key=nice.get):
            print(row(tabs[0][n]) + "  " + nice[n])
        print(f"{len(tabs[0])} kernels")
        return 0
    a, b = tabs
    worse = 0
    for n in sorted(set(a) - set(b), key=nice.get):
        print("GONE    " + nice[n])
    for n in sorted(set(b) - set(a), key=nice.get):
        print("NEW     " + nice[n])
    differ = [n for n in sorted(set(a) & set(b), key=nice.get) if row(a[n]) != row(b[n])]
    for n in differ:
        bad = a[n]["lds"] != b[n]["lds"] or any(b[n][c] > a[n][c] for c in ("vgpr", "scratch", "vspill", "sspill"))
        worse += bad
        print(("WORSE   " if bad else "DIFFERS ") + nice[n] + "\n        " + head + "\n        " + row(a[n]) + "\n        " + row(b[n]))
    print(f"{len(a)} -> {len(b)} kernels: {len(set(a) - set(b))} gone, {len(set(b) - set(a))} new, {len(differ)} differ, {worse} worse")
    return 1 if worse else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
