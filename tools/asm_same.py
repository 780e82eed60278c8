#!/usr/bin/env python3
"""Are two `make -C contractn_amd/csrc asm` listings the same code, kernel by kernel?

    tools/asm_same.py OLD.s NEW.s [--remarks OLD.txt NEW.txt] [--map NEW_SYMBOL=OLD_SYMBOL ...]

For a refactor that must not change what the compiler emits.  Of every kernel (.amdhsa_kernel <symbol>) it compares the
text from the symbol's label to its .Lfunc_end, and the .amdhsa_kernel block: comments after ';' dropped, the function
index taken out of the .LBB<n>_<k> / .Lfunc_end<n> labels, symbols renamed by --map (a kernel that became a template
instantiation has another mangled name).  With --remarks (the stderr of the two builds) the kernel-resource-usage remark
lines are compared per kernel as well, without their file:line:col prefix.  A template's code goes into a section of its
own: the `.section ...,comdat` directive in its body, and the plain `.text` it stands for, are not counted.  Exit status 1
when anything differs.
"""
import argparse
import re
import sys


def normalise(line, rename):
    line = line.split(";", 1)[0].rstrip()
    line = re.sub(r"\.LBB\d+_", ".LBB_", line)
    line = re.sub(r"\.Lfunc_(begin|end)\d+", r".Lfunc_\1", line)
    for new, old in rename.items():
        line = line.replace(new, old)
    return line


def kernels(path, rename):
    """symbol -> (body lines, .amdhsa_kernel block lines), both normalised, under the OLD names"""
    lines = open(path).read().split("\n")
    desc = {m.group(1): i for i, l in enumerate(lines) if (m := re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l))}
    label = {}
    for i, l in enumerate(lines):
        l = l.split(";", 1)[0].rstrip()
        if l.endswith(":") and l[:-1] in desc:
            label[l[:-1]] = i
    out = {}
    for name, k0 in desc.items():
        start = label[name]
        end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
        body = [n for l in lines[start:end + 1] if (n := normalise(l, rename)).strip() and not re.search(r"\.section\s.*comdat|^\s*\.text$", n)]
        k1 = next(i for i in range(k0, len(lines)) if ".end_amdhsa_kernel" in lines[i])
        out[rename.get(name, name)] = (body, [normalise(l, rename) for l in lines[k0:k1 + 1]])
    return out


def remarks(path, rename):
    """symbol -> its remark lines, without position, under the OLD names"""
    out, cur = {}, None
    for l in open(path):
        m = re.search(r"remark: (.*) \[-Rpass-analysis=kernel-resource-usage\]", l)
        if not m:
            continue
        text = m.group(1)
        for new, old in rename.items():
            text = text.replace(new, old)
        f = re.match(r"Function Name: (\S+)", text)
        if f:
            cur = f.group(1)
            out[cur] = []
        elif cur is not None:
            out[cur].append(text.strip())
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--remarks", nargs=2, metavar=("OLD", "NEW"))
    ap.add_argument("--map", action="append", default=[], metavar="NEW=OLD")
    a = ap.parse_args()
    rename = dict(m.split("=", 1) for m in a.map)

    old, new = kernels(a.old, {}), kernels(a.new, rename)
    bad = sorted(set(old) ^ set(new))
    for name in bad:
        print("only in %s: %s" % ("old" if name in old else "new", name))
    for name in sorted(set(old) & set(new)):
        for what, o, n in (("code", old[name][0], new[name][0]), ("kernel descriptor", old[name][1], new[name][1])):
            if o != n:
                bad.append(name)
                first = next((i for i, (x, y) in enumerate(zip(o, n)) if x != y), min(len(o), len(n)))
                print("%s differs: %s (%d / %d lines, first at %d)" % (what, name, len(o), len(n), first))
                print("   old: %s\n   new: %s" % (o[first] if first < len(o) else "<end>", n[first] if first < len(n) else "<end>"))
    print("kernels: %d old, %d new" % (len(old), len(new)))
    if a.remarks:
        ro, rn = remarks(a.remarks[0], {}), remarks(a.remarks[1], rename)
        for name in sorted(set(ro) | set(rn)):
            if ro.get(name) != rn.get(name):
                bad.append(name)
                print("remarks differ: %s\n   old: %s\n   new: %s" % (name, ro.get(name), rn.get(name)))
        print("remarks: %d old, %d new functions" % (len(ro), len(rn)))
        for name in rename.values():
            print("%s: %s" % (name, "; ".join(rn.get(name, ["<none>"]))))
    print("DIFFERENT" if bad else "SAME")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
