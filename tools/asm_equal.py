#!/usr/bin/env python3
"""Per-kernel comparison of two builds' device assembly.

    make -C fem-libraries_amd/csrc asm        # at each of the two commits -> femasm-gfx950.s
    python tools/asm_equal.py old.s new.s

A host-side change can reorder the functions of the device assembly (templates are emitted in
instantiation order), so the two files differ as wholes while every kernel is the same. This compares
per symbol: the text of every function from its label to its .Lfunc_end, and every kernel's
.amdhsa_kernel descriptor block, with the function's ordinal in local labels (.LBB<n>_, .LJTI<n>_,
.Lfunc_end<n>, .Ltmp<k>) normalised away and comments dropped. It compares text only; it knows no
instruction.

Prints the symbols only in one file and the symbols whose text or descriptor differs; exit status 1 if
there are any, else 0.
"""
import hashlib
import re
import sys

TYPE = re.compile(r"^\s*\.type\s+([^,\s]+),@function")
FUNC_END = re.compile(r"^\.Lfunc_end\d+:")
KD_BEGIN = re.compile(r"^\s*\.amdhsa_kernel\s+(\S+)")
KD_END = re.compile(r"^\s*\.end_amdhsa_kernel")
ORDINAL = re.compile(r"\.L(BB|JTI|CPI|func_begin|func_end)\d+")
TMP = re.compile(r"\.Ltmp\d+")


def normalise(lines):
    tmp = {}
    out = []
    for ln in lines:
        if '"' not in ln:  # comments name blocks by ordinal too (BB<n>_<m>) and are aligned to the label's width
            ln = ln.split(";", 1)[0]
        ln = ORDINAL.sub(lambda m: ".L" + m.group(1), ln)
        ln = TMP.sub(lambda m: ".Ltmp%d" % tmp.setdefault(m.group(0), len(tmp)), ln)
        out.append(ln.rstrip())
    return hashlib.sha256("\n".join(out).encode()).hexdigest()


def parse(path):
    """-> ({function: hash of its text}, {kernel: hash of its descriptor block})"""
    funcs, descs = {}, {}
    name = body = desc = None  # the function / descriptor being read
    pending = None             # a .type ...,@function whose label has not come yet
    with open(path) as f:
        for ln in f:
            m = TYPE.match(ln)
            if m:
                pending = m.group(1)
                continue
            if pending is not None and ln.startswith(pending + ":"):
                name, body, pending = pending, [], None
                continue
            if name is None:
                continue
            m = KD_BEGIN.match(ln)
            if m:
                desc = (m.group(1), [])
                continue
            if desc is not None:
                if KD_END.match(ln):
                    descs[desc[0]] = normalise(desc[1])
                    desc = None
                else:
                    desc[1].append(ln)
                continue
            if FUNC_END.match(ln):
                funcs[name] = normalise(body)
                name = body = None
                continue
            body.append(ln)
    return funcs, descs


def report(title, names):
    print("%s: %d" % (title, len(names)))
    for n in names:
        print("  " + n)


def main(argv):
    if len(argv) != 3:
        sys.exit(__doc__)
    fa, da = parse(argv[1])
    fb, db = parse(argv[2])
    print("functions: %d / %d, kernel descriptors: %d / %d" % (len(fa), len(fb), len(da), len(db)))
    only_a = sorted((set(fa) - set(fb)) | (set(da) - set(db)))
    only_b = sorted((set(fb) - set(fa)) | (set(db) - set(da)))
    text = sorted(n for n in set(fa) & set(fb) if fa[n] != fb[n])
    kd = sorted(n for n in set(da) & set(db) if da[n] != db[n])
    report("only in " + argv[1], only_a)
    report("only in " + argv[2], only_b)
    report("function text differs", text)
    report("kernel descriptor differs", kd)
    return 1 if only_a or only_b or text or kd else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
