#!/usr/bin/env python3
"""Are the device functions of one compilation unit the same instructions after it was split?

    hipcc <the Makefile's HIPFLAGS> --cuda-device-only -S X.hip -o X.s     (parent and new units)
    tools/isa_identity.py PARENT.s NEW_1.s [NEW_2.s ...]

Every function (`.type NAME,@function`) and every kernel descriptor (`.amdhsa_kernel NAME` to
`.end_amdhsa_kernel`) of PARENT.s must appear in the union of the NEW files under the same name
with the same text, and the union must hold nothing else. A function that is no kernel (a helper
the compiler kept out of line) may appear in several NEW files, each copy equal to the parent's.
Before comparing, what depends on a function's position in its unit or on the unit itself is
taken out: comments, the function index of block labels (.LBB<n>_<k> -> .LBB_<k>), temporary
labels (.Ltmp<n>, renumbered per function by first appearance), .Lfunc_begin / .Lfunc_end, and
the compilation-unit id (__hip_cuid_<id> and every other occurrence of <id>).
Prints the counts and every difference; exit status 0 only if there is none.

    tools/isa_identity.py --counts A.s [B.s]

For each kernel of each file: the number of instructions and the count of every FP64 vector
mnemonic (v_*_f64). With two files, the differences of B from A as well; exit status 0 only if
every kernel of A has the same FP64 counts in B. A register renumbering or another schedule keeps
these counts; another contraction or another order of the arithmetic does not.
"""
import collections
import re
import sys


def parse(path):
    text = open(path).read()
    for cuid in set(re.findall(r"__hip_cuid_([0-9a-f]+)", text)):
        text = text.replace(cuid, "")
    lines = [ln.split(";", 1)[0].rstrip() for ln in text.splitlines()]
    names = set(re.findall(r"^\s*\.type\s+([^\s,]+),@function", text, re.M))
    funcs, descs = {}, {}
    cur = body = desc = None  # the function, its lines, and the descriptor being read
    for ln in lines:
        if not ln.strip():
            continue
        if desc is not None:  # (a kernel's descriptor sits between its code and its .Lfunc_end)
            if ln.strip() == ".end_amdhsa_kernel":
                desc = None
            else:
                desc.append(ln.strip())
            continue
        m = re.match(r"^\s*\.amdhsa_kernel\s+(\S+)$", ln)
        if m:
            desc = descs[m.group(1)] = []
            continue
        m = re.match(r"^([^\s:]+):$", ln)
        if cur is None and m and m.group(1) in names:
            cur, body = m.group(1), []
        elif cur is not None and re.match(r"^\.Lfunc_end\d+:$", ln):
            funcs[cur] = normalise(body)
            cur = body = None
        elif cur is not None:
            body.append(ln)
    return funcs, descs


def normalise(body):
    tmp = {}

    def renumber(m):
        return ".Ltmp_%d" % tmp.setdefault(m.group(0), len(tmp))

    out = []
    for ln in body:
        if re.match(r"^\.Lfunc_begin\d+:$", ln):
            continue
        ln = re.sub(r"\.LBB\d+_(\d+)", r".LBB_\1", ln)
        ln = re.sub(r"\.Ltmp\d+", renumber, ln)
        out.append(ln.strip())
    return out


def counts(paths):
    per_file = []
    for path in paths:
        funcs, descs = parse(path)
        table = {}
        for name in sorted(descs):
            ops = [ln.split()[0] for ln in funcs[name] if not re.match(r"^[.\w$]+:$|^\.", ln)]
            table[name] = (len(ops), collections.Counter(
                op for op in ops if op.startswith("v_") and op.endswith("_f64")))
            print("%s %s: %d instructions" % (path, name, len(ops)))
            for op, n in sorted(table[name][1].items()):
                print("  %-24s %5d" % (op, n))
        per_file.append(table)
    if len(per_file) < 2:
        return 0
    a, b = per_file
    bad = 0
    for name in sorted(set(a) | set(b)):
        (ta, ca), (tb, cb) = a.get(name, (0, {})), b.get(name, (0, {}))
        diff = {op: cb.get(op, 0) - ca.get(op, 0) for op in set(ca) | set(cb)
                if ca.get(op, 0) != cb.get(op, 0)}
        print("%s: instructions %d -> %d (%+d), FP64 counts %s" %
              (name, ta, tb, tb - ta, "EQUAL" if not diff else "DIFFER %s" % sorted(diff.items())))
        bad += bool(diff)
    return 1 if bad else 0


def main():
    if len(sys.argv) in (3, 4) and sys.argv[1] == "--counts":
        return counts(sys.argv[2:])
    if len(sys.argv) < 3:
        sys.exit(__doc__)
    pf, pd = parse(sys.argv[1])
    nf, nd, bad = {}, {}, 0
    for path in sys.argv[2:]:
        f, d = parse(path)
        print("%-28s %4d functions, %4d kernel descriptors" % (path, len(f), len(d)))
        for name, body in f.items():
            if name in nf and (name in d or nf[name] != body):
                print("DUPLICATE that is a kernel or differs between units: " + name)
                bad += 1
            nf[name] = body
        nd.update(d)
    print("%-28s %4d functions, %4d kernel descriptors" % (sys.argv[1], len(pf), len(pd)))
    print("%-28s %4d functions, %4d kernel descriptors" % ("union of the new units", len(nf), len(nd)))
    for what, p, n in (("function", pf, nf), ("descriptor", pd, nd)):
        missing, extra = sorted(set(p) - set(n)), sorted(set(n) - set(p))
        differ = sorted(k for k in set(p) & set(n) if p[k] != n[k])
        same = len(set(p) & set(n)) - len(differ)
        print("%ss: %d identical, %d differ, %d missing, %d extra" %
              (what, same, len(differ), len(missing), len(extra)))
        for tag, ks in (("DIFFERS", differ), ("MISSING", missing), ("EXTRA", extra)):
            for k in ks:
                print("  %s %s %s" % (tag, what, k))
        bad += len(differ) + len(missing) + len(extra)
    print("IDENTICAL" if bad == 0 else "NOT IDENTICAL")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
