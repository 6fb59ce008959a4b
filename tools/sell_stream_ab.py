#!/usr/bin/env python3
"""A/B of the sliced-ELL launches (sell_stream_kernel) against csr_stream_kernel on the operators of the N^3 hierarchy, in the
level order the cycle uses: residual / prolongation / restriction of levels 0-2 through amgh_bench_op (which = 5 / 6 / 7: the
level-ordered copies as the cycle launches them), the switch amgh_debug_set_sell_stream flipped between timings of the same
handle.  The cap is lifted for the build and the row threshold set one below its default (which leaves the choice to the rule alone:
amgh_finalize's own timings would drop the copies that do not win), so every operator has the padded copy and the table shows where
it stops paying.

    python tools/sell_stream_ab.py [N=256] [coded=1|0] [rounds=3]

(amgh_bench_op's restriction is the round-robin launch: the XCD-contiguous mapping amgh_finalize may pick for a restriction is
only in the cycle's own launch, see the kernel trace of bench.py for that one.)
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    N = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    coded = int(sys.argv[2]) if len(sys.argv) > 2 else 1
    rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    import amg_amd as AMG
    lib = AMG.hip_lib()
    assert lib.amgh_debug_set_tunable(b"stream_code", coded) == 0
    assert lib.amgh_debug_set_sell_stream(1, (1 << 18) - 1, 100000) == 0
    A = AMG.poisson((N, N, N))
    ml = AMG.ruge_stuben(A, setup="gpu")
    dev = ml.device()
    print(f"N={N} {'value-coded' if coded else 'plain'} form; device bytes {dev.device_bytes()}", flush=True)
    print(f"{'level':>5} {'operator':>12} {'rows':>9} {'entries/row':>11} {'padded/nnz':>10} {'csr ms':>8} {'sell ms':>8} {'ratio':>6}")
    for level in range(min(3, len(ml.levels))):
        lv = ml.levels[level]
        for name, which, op, M in (("residual", 5, 0, lv.A), ("prolongation", 6, 1, lv.P), ("restriction", 7, 2, lv.R)):
            padded = lib.amgh_debug_sell_stream_padded(dev.h, level, op)
            if padded <= 0:
                print(f"{level:5d} {name:>12} {M.m:9d} {M.nnz / M.m:11.2f} {'-':>10} (no sliced-ELL copy)")
                continue
            t = {0: [], 1: []}
            for _ in range(rounds):
                for on in (0, 1):
                    assert lib.amgh_debug_set_sell_stream(on, (1 << 18) - 1, 100000) == 0
                    before = lib.amgh_debug_sell_stream_launches(dev.h, level, op)
                    t[on].append(dev.bench_op(level, which, reps=20, warmup=3))
                    assert (lib.amgh_debug_sell_stream_launches(dev.h, level, op) - before == 23) == bool(on)
            csr, sell = sorted(t[0])[rounds // 2], sorted(t[1])[rounds // 2]
            print(f"{level:5d} {name:>12} {M.m:9d} {M.nnz / M.m:11.2f} {padded / M.nnz:10.3f} {csr:8.4f} {sell:8.4f} {sell / csr:6.2f}", flush=True)
    lib.amgh_debug_set_sell_stream(1, 0, 0)
    lib.amgh_debug_set_tunable(b"stream_code", 1)


if __name__ == "__main__":
    main()
