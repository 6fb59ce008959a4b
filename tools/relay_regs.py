#!/usr/bin/env python3
"""Registers, scratch and occupancy of the relayed dataflow kernels that fold the order changes in (gs_relay.hpp, template
flags PB / PX), each beside the kernel it was derived from (the same instantiation with both flags off).

Compiles tools/flow_inst.hip (the parents) and tools/flow_inst_perm.hip (the new kernels) to gfx950 assembly with
--save-temps-style metadata (the .amdhsa_* directives and the `; Occupancy:` remark of every kernel) and prints one line per
new kernel.  Exit code 1 if a new kernel spills, uses AGPRs its parent does not, or loses a wave of occupancy.
usage: python tools/relay_regs.py [parents.s new.s]      (assembly files already made: skips the compilation)"""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
NAME = re.compile(r"gs_bw_relay_kernelI([df])Lb([01])ELb([01])ELi(\d+)ELi(\d+)ELb([01])ELb([01])ELb([01])ELb([01])E")


def compile_s(src, out):
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "--cuda-device-only", "-S", "-o", out, src]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    if r.returncode != 0:
        raise SystemExit(r.stdout.decode(errors="replace")[-2000:])


def figures(path):
    """{instantiation key: [vgprs, agprs, scratch bytes, occupancy]}; key = (type, SOR, BWD, MAXK, W, DICT, LATE, PB, PX)"""
    text = open(path).read()
    out = {}
    # behind every kernel: ".size <name>, ..." and the compiler's remarks "; NumVgprs", "; NumAgprs", "; ScratchSize", "; Occupancy"
    for m in re.finditer(r"\n\t\.size\t(\S+), \.Lfunc_end\d+-.*?\n; NumVgprs: (\d+)\n; NumAgprs: (\d+)\n.*?\n; ScratchSize: (\d+)\n.*?\n; Occupancy: (\d+)\n", text, re.S):
        k = NAME.search(m.group(1))
        if k:
            out[k.groups()] = [int(m.group(2)), int(m.group(3)), int(m.group(4)), int(m.group(5))]
    return out


def main():
    with tempfile.TemporaryDirectory() as tmp:
        if len(sys.argv) > 2:
            ps, ns = sys.argv[1], sys.argv[2]
        else:
            ps, ns = os.path.join(tmp, "parents.s"), os.path.join(tmp, "new.s")
            compile_s(os.path.join(ROOT, "tools", "flow_inst.hip"), ps)
            compile_s(os.path.join(ROOT, "tools", "flow_inst_perm.hip"), ns)
        par, new = figures(ps), figures(ns)
    rc = 0
    print("type SOR BWD MAXK W DICT LATE PB PX |  VGPRs AGPRs scratch occupancy | parent: VGPRs AGPRs scratch occupancy")
    for key in sorted(new, key=lambda k: (k[0], int(k[3]), k[5], k[6], k[1], k[2], k[7], k[8])):
        if key[7] == "0" and key[8] == "0":
            continue
        p = par.get(key[:7] + ("0", "0"))
        v = new[key]
        bad = p is None or v[2] != 0 or v[1] > p[1] or v[3] < p[3]
        rc |= 1 if bad else 0
        print("%s    %s   %s   %3s  %s  %s    %s    %s  %s  | %5d %5d %7d %9s | %13s %5s %7s %9s%s" % (
            key + (v[0], v[1], v[2], v[3]) + (tuple(p) if p else ("-", "-", "-", "-")) + ("   <-- FAIL" if bad else "",)))
    n = sum(1 for k in new if k[7] == "1" or k[8] == "1")
    print("%d new instantiations; %s" % (n, "all within their parents' scratch, AGPRs and occupancy" if rc == 0 and n else "FAIL"))
    return rc if n else 2


if __name__ == "__main__":
    sys.exit(main())
