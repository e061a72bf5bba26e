#!/usr/bin/env python3
"""Did a host-only change leave the device code alone?  Compares two `hipcc --offload-device-only -S` listings of one source
file kernel by kernel: the same set of kernels, identical bodies, identical `.amdhsa_kernel` descriptor blocks.

    python tools/asm_kernel_diff.py before.s after.s

Whole-file equality is not the criterion: kernels are emitted in order of first use, so a launcher edit moves them and renumbers
the local labels that carry the function's number (.LBB<n>_, BB<n>_, .Lfunc_end<n>) or a file-wide counter (.Ltmp<n>).  Those
numbers are normalised per body and runs of blanks collapsed (a longer label shifts the padding of its comment); everything else
is compared as text (by hash).  Exit status 1 if anything differs."""
import hashlib
import re
import sys

FUNC_NO = re.compile(r"(\.LBB|\bBB|\.Lfunc_end)\d+")
TMP = re.compile(r"\.Ltmp\d+")
TOP_LABEL = re.compile(r"^([A-Za-z_$][\w$.]*):")


def normalise(lines):
    tmp = {}
    out = []
    for ln in lines:
        ln = FUNC_NO.sub(r"\1#", ln)
        ln = TMP.sub(lambda m: tmp.setdefault(m.group(0), ".Ltmp%d" % len(tmp)), ln)
        out.append(" ".join(ln.split()))  # (a label one digit longer shifts the padding in front of its comment)
    return hashlib.sha256("\n".join(out).encode()).hexdigest()


def kernels(path):
    """{kernel: (hash of its body, hash of its descriptor block)}"""
    bodies, descs, funcs = {}, {}, set()
    name, cur, dname, dcur = None, None, None, None
    with open(path) as f:
        for ln in f:
            s = ln.strip()
            if s.startswith(".amdhsa_kernel "):
                dname, dcur = s.split()[1], []
            if dname is not None:
                dcur.append(s + "\n")
                if s == ".end_amdhsa_kernel":
                    descs[dname] = hashlib.sha256("".join(dcur).encode()).hexdigest()
                    dname = None
                continue
            if name is None:
                m = TOP_LABEL.match(ln)
                if m and m.group(1) in funcs:
                    name, cur = m.group(1), []
                elif s.startswith(".type") and s.endswith(",@function"):
                    funcs.add(s.split()[1].split(",")[0])
            elif s.startswith(".Lfunc_end"):
                bodies[name] = normalise(cur)
                name = None
            else:
                cur.append(ln)
    missing = sorted(set(descs) - set(bodies))
    if missing:
        sys.exit(f"{path}: no body found for {missing}")
    return {k: (bodies[k], descs[k]) for k in descs}


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    only_a, only_b = sorted(set(a) - set(b)), sorted(set(b) - set(a))
    body = sorted(k for k in a if k in b and a[k][0] != b[k][0])
    desc = sorted(k for k in a if k in b and a[k][1] != b[k][1])
    print(f"{len(a)} kernels before, {len(b)} after: {len(only_a)} only before, {len(only_b)} only after, "
          f"{len(body)} bodies differ, {len(desc)} descriptors differ")
    for title, names in (("only before", only_a), ("only after", only_b), ("body differs", body), ("descriptor differs", desc)):
        for k in names:
            print(f"  {title}: {k}")
    sys.exit(1 if only_a or only_b or body or desc else 0)


if __name__ == "__main__":
    main()
