"""Compares the kernels of two device assembly listings written by `make -C plaid_amd/csrc asm`, symbol by symbol:
    python3 tools/kernel_isa_diff.py OLD NEW        (each a .s file or a directory of them)
For every kernel on both sides: the instruction stream (comments, .loc / .file / .cfi lines and the numbering of .LBB,
.Ltmp and .Lfunc labels removed) and the resource figures of its .amdhsa_kernel block.  One line per kernel, `same` or
the first pair that differs; then the kernels on one side only.  Exit status 1 when a kernel on both sides differs."""
import glob
import os
import re
import shutil
import subprocess
import sys

FIGURES = ("next_free_vgpr", "next_free_sgpr", "accum_offset", "private_segment_fixed_size", "group_segment_fixed_size")
LABEL = re.compile(r"\.L(BB|JTI)\d+_|\.L(tmp|func_begin|func_end)\d+")


def kernels(path):
    """{symbol: (instruction lines, {figure: value})} of one file or of every .s file in a directory"""
    out = {}
    for name in sorted(glob.glob(os.path.join(path, "*.s"))) if os.path.isdir(path) else [path]:
        lines = open(name).read().split("\n")
        start = {l.split(":")[0]: i for i, l in enumerate(lines) if re.match(r"[A-Za-z_$][\w$.]*:", l)}
        for i, l in enumerate(lines):
            if not l.strip().startswith(".amdhsa_kernel "):
                continue
            sym = l.split()[1]
            end = next(j for j in range(i, len(lines)) if lines[j].strip() == ".end_amdhsa_kernel")
            fig = {w[0][len(".amdhsa_"):]: w[1] for w in (x.split() for x in lines[i + 1:end]) if w[0][len(".amdhsa_"):] in FIGURES}
            body = []
            for x in lines[start[sym] + 1:i]:
                x = x.split(";")[0].strip()
                if x and not re.match(r"\.(loc|file|cfi_\w+|section|p2align)\b", x):
                    body.append(LABEL.sub(lambda m: ".L" + (m.group(1) or m.group(2)) + "_", x))
            out[sym] = (body, fig)
    return out


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    names = sorted(set(a) | set(b))
    filt = shutil.which("c++filt") or shutil.which("llvm-cxxfilt")
    plain = subprocess.run([filt], input="\n".join(names), capture_output=True, text=True).stdout.split("\n") if filt else names
    plain = dict(zip(names, plain))
    differ = 0
    for s in names:
        if s not in a or s not in b:
            continue
        (ia, fa), (ib, fb) = a[s], b[s]
        what = "same"
        if fa != fb:
            what = "figures differ: " + ", ".join(f"{k} {fa.get(k)} -> {fb.get(k)}" for k in FIGURES if fa.get(k) != fb.get(k))
        elif ia != ib:
            at = next((i for i, (x, y) in enumerate(zip(ia, ib)) if x != y), min(len(ia), len(ib)))
            what = f"differs at instruction {at}: {ia[at] if at < len(ia) else '<end>'!r} -> {ib[at] if at < len(ib) else '<end>'!r}"
        differ += what != "same"
        print(f"{plain[s]}: {what} ({len(ib)} lines, " + ", ".join(f"{k} {fb.get(k)}" for k in FIGURES) + ")")
    for side, x, y in (("only in " + sys.argv[1], a, b), ("only in " + sys.argv[2], b, a)):
        for s in names:
            if s in x and s not in y:
                print(f"{side}: {plain[s]}")
    print(f"{sum(s in a and s in b for s in names)} kernels on both sides, {differ} differ; "
          f"{sum(s not in b for s in names)} only in the first, {sum(s not in a for s in names)} only in the second")
    sys.exit(1 if differ else 0)


if __name__ == "__main__":
    main()
