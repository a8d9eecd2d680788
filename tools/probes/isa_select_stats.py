"""Static select statistics of the kernels of a .hip file of geoflowslam_amd/csrc: compiles it with the Makefile's own compile line
plus `--cuda-device-only -S` (nothing is linked, no GPU is needed) and prints, per kernel, the VALU instructions, the v_cndmask_*
among them, the v_cmp_eq_u32 / v_cmp_eq_i32 (VOPC, VOP3 and SDWA forms) and the share of the two in the VALU count.  A private array
indexed at run time that the compiler keeps in registers shows as a high share: every read is a compare-and-select chain over all
of its elements.  Counts only; nothing is asserted.  The counts are static: a loop body counts once.

    python tools/probes/isa_select_stats.py gicp.hip orb.hip gms.hip [--min-valu 200] [--keep DIR]
"""
import argparse
import os
import re
import shlex
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
CSRC = os.path.join(ROOT, "geoflowslam_amd", "csrc")


def compile_line(name):
    """The Makefile's command for <name>.o as an argument list, without -c, -o and the dependency-file flags."""
    obj = os.path.splitext(name)[0] + ".o"
    out = subprocess.run(["make", "-n", "-B", obj], cwd=CSRC, check=True, capture_output=True, text=True).stdout
    line = next(ln for ln in out.splitlines() if " -c " in ln and name in ln)
    args, skip = [], False
    for a in shlex.split(line):
        if skip:
            skip = False
        elif a == "-o":
            skip = True
        elif a not in ("-c", "-MMD", "-MP"):
            args.append(a)
    return args


def demangle(names):
    for tool in ("llvm-cxxfilt", "/opt/rocm/llvm/bin/llvm-cxxfilt", "c++filt"):
        try:
            out = subprocess.run([tool], input="\n".join(names), check=True, capture_output=True, text=True).stdout.splitlines()
            return dict(zip(names, out))
        except (OSError, subprocess.CalledProcessError):
            continue
    return {n: n for n in names}


def short(name):
    """`(anonymous namespace)::k_x<unsigned int>(args...)` -> `k_x<unsigned int>`"""
    depth, cut = 0, len(name)
    for i, ch in enumerate(name):
        if ch == "<":
            depth += 1
        elif ch == ">":
            depth -= 1
        elif ch == "(" and depth == 0 and not name.startswith("(anonymous namespace)", i):
            cut = i
            break
    name = name[:cut].replace("(anonymous namespace)::", "")
    return name.split(" ", 1)[1] if name.startswith("void ") else name


def kernel_stats(asm):
    """{symbol: (valu, cndmask, cmp_eq)} for every symbol that has an .amdhsa_kernel block."""
    kernels = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm, re.M))
    stats, cur = {}, None
    for ln in asm.splitlines():
        m = re.match(r"^([A-Za-z_$][\w$.]*):", ln)
        if m:
            if m.group(1) in kernels:
                cur = m.group(1)
                stats[cur] = [0, 0, 0]
            continue
        if cur is None:
            continue
        t = ln.strip()
        if t.startswith(".Lfunc_end"):
            cur = None
        elif t.startswith("v_"):
            op = t.split(None, 1)[0]
            stats[cur][0] += 1
            stats[cur][1] += op.startswith("v_cndmask")
            stats[cur][2] += re.match(r"v_cmpx?_eq_[ui]32(_e32|_e64|_sdwa)?$", op) is not None
    return stats


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("files", nargs="+", help="names of .hip files in geoflowslam_amd/csrc")
    ap.add_argument("--min-valu", type=int, default=0, help="leave out kernels with fewer VALU instructions")
    ap.add_argument("--keep", help="keep the assembly in this directory")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        out_dir = a.keep or tmp
        os.makedirs(out_dir, exist_ok=True)
        print(f"{'file':<12} {'kernel':<44} {'VALU':>6} {'cndmask':>8} {'cmp_eq':>7} {'share':>6}")
        for f in a.files:
            f = os.path.basename(f)
            s = os.path.join(out_dir, os.path.splitext(f)[0] + ".s")
            subprocess.run(compile_line(f) + ["--cuda-device-only", "-S", "-o", s], cwd=CSRC, check=True)
            st = kernel_stats(open(s).read())
            names = demangle(list(st))
            for sym, (valu, cnd, cmp_eq) in sorted(st.items(), key=lambda kv: -(kv[1][1] + kv[1][2]) / max(kv[1][0], 1)):
                if valu >= max(a.min_valu, 1):
                    print(f"{f:<12} {short(names[sym]):<44} {valu:>6} {cnd:>8} {cmp_eq:>7} {(cnd + cmp_eq) / valu:>6.2f}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
