#!/usr/bin/env python3
"""Do two builds of a HIP source compile to the same kernels?  For a change that must not touch the machine code (a file split,
a pruned template list, a resolved #if).

    hipcc <the Makefile's HIPFLAGS> -S --cuda-device-only old/gacq_ldsfft.hip -o old.s      (the same for the new tree)
    tools/isa_diff.py old.s new.s [--rename 'lds_correlate_kernel<2,1,1,0,0,1>=lds_correlate_kernel<1,1>' ...]

Kernels are matched by base name and template-argument values (`name<v0,v1,...>`, read from the mangled symbol); --rename gives
a kernel of the first listing the name it has in the second when the template list itself changed.  Per matched kernel the tool
prints the instruction count and one of three verdicts:
    same        body and .amdhsa_kernel block are the same text
    reordered   the .amdhsa_kernel block is the same and so is the multiset of opcodes: the same instruction mix and resources in
                another order or with other operands (what moving code into a shared device function typically does to the scheduler)
    differs     anything else; its diff is printed
and exits non-zero on any `differs` (or when nothing matched).  Kernels in only one listing are named and otherwise ignored: a file
split is checked with one run per new file.

What is compared, as text: the kernel's body from its label to its end label, and its .amdhsa_kernel block (register counts, LDS
bytes, scratch).  Comments are dropped; the kernel's own mangled name, the enclosing function in the name of a function-local LDS
variable (the kernel itself or a device function it shares with others: `_ZZ<function>E6s_peak` -> `@L@s_peak`) and the function
number in local labels are normalised away."""
import argparse
import collections
import difflib
import re
import sys


def kernel_key(sym):
    """`name<v0,v1,...>` from an Itanium-mangled function symbol with literal template arguments; the symbol itself otherwise."""
    m = re.match(r"_ZN?", sym)
    if not m:
        return sym
    pos, name = m.end(), None
    while True:
        m = re.compile(r"(\d+)").match(sym, pos)
        if not m:
            break
        n = int(m.group(1))
        name = sym[m.end():m.end() + n]
        pos = m.end() + n
    if name is None:
        return sym
    if pos >= len(sym) or sym[pos] != "I":
        return name
    pos += 1
    args = []
    while pos < len(sym) and sym[pos] != "E":
        m = re.compile(r"L[a-z](n?)(\d+)E").match(sym, pos)
        if not m:
            return sym                      # a type or pack argument: leave the kernel under its mangled name
        args.append(("-" if m.group(1) else "") + m.group(2))
        pos = m.end()
    return "%s<%s>" % (name, ",".join(args))


def local_static(m):
    """`@L@name` for the mangled name of a function-local static (`_ZZ<function encoding>E<len><name>[_<n>]`), whatever the function."""
    tok = m.group(0)
    for e in reversed(list(re.finditer(r"E(\d+)", tok))):
        n = int(e.group(1))
        name, rest = tok[e.end():e.end() + n], tok[e.end() + n:]
        if len(name) == n and re.fullmatch(r"[A-Za-z_]\w*", name) and re.fullmatch(r"(_\d*)?", rest):
            return "@L@" + name
    return tok


def opcodes(body):
    return collections.Counter(ln.split()[0] for ln in body if not ln.startswith(".") and not ln.endswith(":"))


def kernels(path):
    """{key: (body lines, descriptor lines)} of every kernel (a function with an .amdhsa_kernel block) in a -S listing."""
    lines = open(path).read().split("\n")
    out = {}
    i = 0
    while i < len(lines):
        m = re.match(r"(_Z\w+):", lines[i])
        if not m:
            i += 1
            continue
        sym = m.group(1)
        end = i + 1
        while end < len(lines) and not re.match(r"\.Lfunc_end\d+:", lines[end]):
            end += 1
        body, desc, where = [], [], 0       # where: 0 = code, 1 = inside the .amdhsa_kernel block, 2 = behind it
        for ln in lines[i + 1:end]:
            ln = re.sub(r"\s*;.*$", "", ln).strip()
            if not ln:
                continue
            ln = re.sub(r"\s+", " ", re.sub(r"_ZZ\w+", local_static, ln).replace(sym[2:], "@K@"))
            ln = re.sub(r"\.L([A-Za-z_]+)\d+_(\d+)", r".L\1_\2", ln)
            if ln.startswith(".amdhsa_kernel"):
                where = 1
            if where == 1:
                desc.append(ln)
            elif where == 0 and not ln.startswith(".section"):
                body.append(ln)
            if ln.startswith(".end_amdhsa_kernel"):
                where = 2
        if desc:
            out[kernel_key(sym)] = (body, desc)
        i = end + 1
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("first")
    ap.add_argument("second")
    ap.add_argument("--rename", action="append", default=[], metavar="FIRST=SECOND")
    ap.add_argument("--show", type=int, default=40, help="lines of unified diff printed per differing kernel")
    a = ap.parse_args()
    ka, kb = kernels(a.first), kernels(a.second)
    for r in a.rename:
        old, new = r.split("=", 1)
        if old not in ka:
            sys.exit("--rename: no kernel %s in %s (it has: %s)" % (old, a.first, ", ".join(sorted(ka))))
        ka[new] = ka.pop(old)
    bad = matched = moved = 0
    for k in sorted(set(ka) | set(kb)):
        if k not in ka or k not in kb:
            print("%-52s only in %s" % (k, a.second if k in kb else a.first))
            continue
        matched += 1
        (ba, da), (bb, db) = ka[k], kb[k]
        count = sum(1 for ln in bb if not ln.startswith(".") and not ln.endswith(":"))
        verdict = "same" if ba == bb and da == db else "reordered" if da == db and opcodes(ba) == opcodes(bb) else "differs"
        print("%-52s %6d instructions  %s" % (k, count, verdict))
        moved += verdict == "reordered"
        if verdict == "differs":
            bad += 1
            diff = list(difflib.unified_diff(ba + da, bb + db, a.first, a.second, lineterm="", n=2))
            print("\n".join(diff[:a.show]))
            if len(diff) > a.show:
                print("... (%d more lines)" % (len(diff) - a.show))
    print("%d kernels compared, %d reordered, %d differ" % (matched, moved, bad))
    sys.exit(1 if bad or not matched else 0)


if __name__ == "__main__":
    main()
