"""bench.py at N = 1 on a small grid: a plain run reports the headline figure and nothing that takes runs of its own; --full
adds the roofline, time to solution, the block of right-hand sides, the uncompressed layouts, the CPU baseline and the parity
of the timed V-cycle against the oracle.  Both runs time the same steps: the dumped solutions agree."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("roofline", "sweep_roofline", "pcg_to_solution", "block_of_right_hand_sides", "vcycle_uncompressed", "cpu_baseline",
             "parity")


def _bench(outdir, *extra):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--size", "32", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", outdir, *extra], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    lines = [ln for ln in r.stdout.decode().splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    return json.loads(lines[0])


def test_bench_plain_and_full(tmp_path):
    plain = _bench(str(tmp_path / "plain"))
    full = _bench(str(tmp_path / "full"), "--full", "--no-pmc", "--no-secondary-configs", "--cpu-budget", "0.5")
    for d in (plain, full):
        assert all(k in d for k in HEADLINE)
        assert d["metric"] == "V-cycle unknowns/sec + fine-level SpMV GB/s (% HBM peak), 3-D Poisson 32^3"
        assert d["unit"] == "unknowns/s" and d["higher_is_better"] is True and d["dtype"] == "f64"
        assert d["steps"] == 3 and d["warmup"] == 1 and d["config"]["unknowns"] == 32 ** 3
        assert d["value"] == pytest.approx(32 ** 3 / (d["ms_per_step"] * 1e-3), rel=1e-9)
    assert not [k for k in FULL_ONLY if k in plain]
    assert plain["vcycle"]["fine_symmetric_gs_ms"] is None
    assert all(k in full for k in FULL_ONLY)
    assert full["roofline"]["achieved"] > 0 and full["vcycle"]["fine_symmetric_gs_ms"] > 0
    assert full["parity"]["rel_err_vs_oracle"] <= 1e-10
    assert full["pcg_to_solution"]["true_rel_residual"] <= 1e-7
    assert full["block_of_right_hand_sides"]["first_column_rel_diff_vs_single_column_cycle"] <= 1e-10
    assert full["vcycle_uncompressed"]["rel_diff_vs_compressed_cycle"] <= 1e-10
    zp, zf = np.load(tmp_path / "plain" / "z.npy"), np.load(tmp_path / "full" / "z.npy")
    assert zp.shape == (32 ** 3,) and np.linalg.norm(zp - zf) <= 1e-13 * np.linalg.norm(zf)
