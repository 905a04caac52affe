"""Per-kernel comparison of two `hipcc -S --cuda-device-only` listings of one source (e.g. csrc/maxsim_fwd16.hip at two commits).

For every kernel symbol of listing A the instruction stream (labels, directives and comments dropped; mangled symbol names and the
per-translation-unit __hip_cuid_* name replaced by placeholders) must be identical in listing B; kernels only B has are listed.
usage: python scratch/compare_listings.py A.s B.s      exit 0 = every kernel of A is unchanged in B
"""
import re
import subprocess
import sys


def kernels(path):
    lines = open(path).read().splitlines()
    out, i = {}, 0
    while i < len(lines):
        m = re.match(r"^(_Z\w+):", lines[i])
        if m:
            j = i + 1
            while not lines[j].startswith(".Lfunc_end"):
                j += 1
            body = []
            for ln in lines[i + 1:j]:
                t = ln.split(";")[0].strip() if not ln.strip().startswith(";;#") else ln.strip()
                if not t or t.startswith(".") or t.endswith(":"):
                    continue
                t = re.sub(r"_Z\w+", "SYM", t)
                t = re.sub(r"__hip_cuid_\w+", "CUID", t)
                t = re.sub(r"\.LBB\d+_", ".LBB_", t)
                body.append(t)
            name = subprocess.run(["c++filt", m.group(1)], capture_output=True, text=True).stdout.strip()
            out[name] = body
            i = j
        i += 1
    return out


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    bad = 0
    for name, body in a.items():
        if name not in b:
            print("MISSING  ", name)
            bad += 1
        elif b[name] != body:
            print(f"DIFFERENT {name}  ({len(body)} vs {len(b[name])} instructions)")
            bad += 1
        else:
            print(f"same      {name}  ({len(body)} instructions)")
    for name in b:
        if name not in a:
            print(f"new       {name}  ({len(b[name])} instructions)")
    print(f"{len(a)} kernels compared, {bad} changed")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
