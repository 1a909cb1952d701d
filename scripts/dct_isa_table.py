#!/usr/bin/env python3
"""Static ISA table of the fused transform kernels (dct_fast.hip: dct_fused_kernel).

Compiles dct_fast.hip for gfx950 with the Makefile's flags (--cuda-device-only -S) and counts, per instantiation, the static
VALU instructions (loop bodies once, both sides of every branch), the f64 ones among them, v_rcp_f64, VGPRs, scratch and occupancy.
Every compile-time-length instantiation (CN = 512) is listed next to its runtime-length fallback (CN = 0), with the f64 opcode mix
of both.  Static f64 counts of a pair need not be equal: the fallback also carries the radix-4 / radix-2 stage code and the stage
loop of other lengths, which is dead at N = 512, and a two-trip work-item loop may be laid out differently.  Same results bit for bit is
what tests/test_gpu_dct_const_len.py checks on the device.

    python scripts/dct_isa_table.py [--asm FILE.s] [--check]

--check exits non-zero when a CN = 512 kernel uses scratch or runs fewer waves per SIMD than its fallback.
"""
import argparse
import collections
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bifurcationkit.jl_amd", "csrc")
FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wall", "-Wno-unused-function", "-ffp-contract=off"]
PARAMS = ["NT", "MODE", "AX0", "NTM", "DOT", "FZ", "SLAB", "FZS", "TURN", "CN", "NRM", "SRC"]
CN = PARAMS.index("CN")


def compile_asm(out):
    hipcc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    subprocess.run([hipcc, *FLAGS, "--cuda-device-only", "-S", "dct_fast.hip", "-o", out], cwd=CSRC, check=True)


def parse(asm):
    """{template args tuple: stats} for every dct_fused_kernel in the listing."""
    kernels = {}
    cur, body = None, False
    for line in open(asm):
        m = re.match(r"^(_Z\S*):", line)
        if m:
            cur, body = None, False
            if "dct_fused_kernel" in m.group(1):
                name = m.group(1)
                args = tuple(int(v) for _, v in re.findall(r"L([ib])(\d+)E", name.split("dct_fused_kernel", 1)[1]))
                cur = args + (0,) * (len(PARAMS) - len(args))
                kernels[cur] = {"ops": collections.Counter(), "meta": {}, "name": name}
                body = True
            continue
        if cur is None:
            continue
        s = line.strip()
        if line.startswith(".Lfunc_end"):
            body = False
        elif body and s.startswith("v_"):
            kernels[cur]["ops"][s.split()[0]] += 1
        elif not body:
            for key in ("NumVgprs", "ScratchSize", "Occupancy"):
                mm = re.match(r";\s*%s:\s*(\d+)" % key, s)
                if mm and key not in kernels[cur]["meta"]:
                    kernels[cur]["meta"][key] = int(mm.group(1))
    return kernels


def stats(k):
    ops = k["ops"]
    valu = sum(ops.values())
    f64 = sum(n for op, n in ops.items() if "_f64" in op)
    return {"valu": valu, "f64": f64, "other": valu - f64, "rcp": ops.get("v_rcp_f64", 0),
            "vgpr": k["meta"].get("NumVgprs", -1), "scratch": k["meta"].get("ScratchSize", -1),
            "occ": k["meta"].get("Occupancy", -1)}


def label(args):
    a = dict(zip(PARAMS, args))
    s = "<%d,%d,%s" % (a["NT"], a["MODE"], "AX0" if a["AX0"] else ("z" if a["MODE"] == 2 else "y"))
    for f in ("NTM", "DOT", "FZ", "FZS", "TURN", "NRM", "SRC"):
        if a[f]:
            s += "," + f
    if a["SLAB"]:
        s += ",SLAB%d" % a["SLAB"]
    return s + ">"


def top_int_ops(k, n=8):
    c = collections.Counter({op: v for op, v in k["ops"].items() if "_f64" not in op})
    return " ".join("%s %d" % (op[2:], v) for op, v in c.most_common(n))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--asm", help="existing listing (default: compile dct_fast.hip into a temporary directory)")
    ap.add_argument("--check", action="store_true")
    a = ap.parse_args()
    if a.asm:
        kernels = parse(a.asm)
    else:
        with tempfile.TemporaryDirectory() as d:
            out = os.path.join(d, "dct_fast.s")
            compile_asm(out)
            kernels = parse(out)
    bad = []
    hdr = "%-28s %5s %5s %5s %4s %4s %4s %3s" % ("instantiation", "VALU", "f64", "int", "rcp", "VGPR", "scr", "occ")
    print("All fused-kernel instantiations (runtime length, CN = 0)")
    print(hdr)
    for args in sorted(k for k in kernels if k[CN] == 0):
        s = stats(kernels[args])
        print("%-28s %5d %5d %5d %4d %4d %4d %3d" % (label(args), s["valu"], s["f64"], s["other"], s["rcp"], s["vgpr"],
                                                   s["scratch"], s["occ"]))
    print()
    print("Compile-time length (CN = 512) against the runtime-length fallback (CN = 0); int = VALU - f64")
    print("%-28s %11s %11s %11s %9s %7s %3s  %s" % ("instantiation", "VALU 0/512", "f64 0/512", "int 0/512", "int cut", "VGPR",
                                                   "scr", "largest non-f64 VALU ops at CN = 512"))
    diff = []
    for args in sorted(k for k in kernels if k[CN] == 512):
        fb = args[:CN] + (0,) + args[CN + 1:]
        s1 = stats(kernels[args])
        if fb not in kernels:
            bad.append("%s: no fallback" % label(args))
            continue
        s0 = stats(kernels[fb])
        print("%-28s %5d/%-5d %5d/%-5d %5d/%-5d %8.0f%% %3d/%-3d %3d  %s" % (
            label(args), s0["valu"], s1["valu"], s0["f64"], s1["f64"], s0["other"], s1["other"],
            100.0 * (1 - s1["other"] / s0["other"]), s0["vgpr"], s1["vgpr"], s1["scratch"], top_int_ops(kernels[args])))
        mix = lambda k: collections.Counter({op.replace("_e32", ""): n for op, n in k["ops"].items() if "_f64" in op})
        m0, m1 = mix(kernels[fb]), mix(kernels[args])
        diff.append("%-28s %s" % (label(args), " ".join("%s %d/%d" % (op[2:], m0[op], m1[op])
                                                          for op in sorted(set(m0) | set(m1)) if m0[op] != m1[op])))
        if s1["scratch"] != 0:
            bad.append("%s: scratch %d" % (label(args), s1["scratch"]))
        if s1["occ"] < s0["occ"]:
            bad.append("%s: occupancy %d vs fallback %d" % (label(args), s1["occ"], s0["occ"]))
    print()
    print("f64 opcodes that differ, fallback / CN = 512")
    print("\n".join(diff))
    if bad:
        print()
        print("CHECK:\n  " + "\n  ".join(bad))
    return 1 if (a.check and bad) else 0


if __name__ == "__main__":
    sys.exit(main())
