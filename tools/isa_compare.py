"""Compare the gfx950 instruction streams of every kernel in two builds (objects
or libraries), with addresses, encodings and comments stripped -- a refactor's
check that no surviving kernel changed, without a GPU.
Usage: python tools/isa_compare.py --a FILE [FILE ...] --b FILE [FILE ...]
Prints the kernels only in one side, the kernels whose streams differ (with
both instruction counts; "operand order only": every differing line is the
same instruction with its source operands in another order), and the count of
identical ones; exit status 1 when any kernel differs."""
import argparse
import re
import subprocess
import sys
import tempfile

from kernel_resources import LLVM, code_objects


def kernels(paths, tmp):
    """demangled kernel name -> list of instruction lines"""
    out = {}
    for n, path in enumerate(paths):
        sub = tempfile.mkdtemp(dir=tmp, prefix=f"f{n}_")
        for dev in code_objects(path, sub):
            kd = subprocess.run([f"{LLVM}/llvm-readelf", "-s", "--wide", dev], capture_output=True,
                                text=True).stdout
            entry = {f[7][:-3] for f in (l.split() for l in kd.splitlines())
                     if len(f) >= 8 and f[3] == "OBJECT" and f[7].endswith(".kd")}
            dis = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", "--no-leading-addr",
                                  dev], capture_output=True, text=True, check=True).stdout
            cur = None
            for line in dis.splitlines():
                m = re.match(r"^[0-9a-f]* ?<(.+)>:$", line)
                if m:
                    name = m.group(1)
                    if name not in entry:   # a basic-block label inside a kernel, or a device function
                        cur = cur if name.startswith((".L", "L")) else None
                        continue
                    while name in out:   # the same internal name in two units
                        name += " "
                    cur = out.setdefault(name, [])
                    continue
                ins = line.split("//")[0].strip()
                if cur is not None and ins and ins != "...":   # "...": padding between kernels
                    cur.append(ins)
    names = list(out)
    dm = subprocess.run(["c++filt"], input="\n".join(n.rstrip() for n in names), capture_output=True, text=True).stdout.splitlines()
    short = lambda s: re.sub(r"\(.*", "", s.replace("(anonymous namespace)", "anon"))
    return {short(d) + "'" * (len(n) - len(n.rstrip())): out[n] for n, d in zip(names, dm)}


def commuted(x, y):
    """the streams differ only in the order of some instructions' source operands"""
    ops = lambda l: (l.split(None, 1)[0], l.split(None, 1)[1].split(", ") if " " in l else [])
    if len(x) != len(y):
        return False
    for l, r in zip(x, y):
        if l != r:
            (ml, ol), (mr, orr) = ops(l), ops(r)
            if ml != mr or ol[:1] != orr[:1] or sorted(ol[1:]) != sorted(orr[1:]):
                return False
    return True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--a", nargs="+", required=True)
    ap.add_argument("--b", nargs="+", required=True)
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        a, b = kernels(args.a, tmp), kernels(args.b, tmp)
    for k in sorted(set(a) - set(b)):
        print(f"only in a: {k}")
    for k in sorted(set(b) - set(a)):
        print(f"only in b: {k}")
    both = sorted(set(a) & set(b))
    diff = [k for k in both if a[k] != b[k]]
    for k in diff:
        note = "  operand order only" if commuted(a[k], b[k]) else ""
        print(f"differs: {k}  ({len(a[k])} / {len(b[k])} instructions){note}")
    print(f"{len(both) - len(diff)} of {len(both)} common kernels identical, {len(diff)} differ")
    return 1 if diff else 0


if __name__ == "__main__":
    sys.exit(main())
