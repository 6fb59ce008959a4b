"""The relayed kernels that fold the fine level's order changes in (csrc/hip/gs_relay.hpp, template flags PB / PX; instantiated
by tools/flow_inst_perm.hip, 256 of them) count their memory pipeline by hand like their parents: the linear audit
(tools/flow_asm_linear.py) must find no hand-issued load touched in flight in any of them, and tools/relay_regs.py no spill, no
AGPR and no wave of occupancy lost against the same instantiation with both flags off (tests/test_flow_asm.py audits those)."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_HIPCC = shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc")


TOOLS = os.path.join(ROOT, "tools")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def new_s(tmp_path_factory):
    """the new kernels' assembly, made once for both audits (the command of tools/relay_regs.py and tools/flow_asm_linear.py)"""
    out = str(tmp_path_factory.mktemp("perm_io") / "new.s")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "--cuda-device-only", "-S", "-o", out,
                        os.path.join(TOOLS, "flow_inst_perm.hip")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=1200)
    assert r.returncode == 0, r.stdout.decode(errors="replace")[-2000:]
    return out


@pytest.mark.skipif(NO_HIPCC, reason="hipcc not available")
def test_no_set_in_flight_is_touched_in_the_kernels_that_fold_the_order_changes_in(new_s):
    r = subprocess.run([sys.executable, os.path.join(TOOLS, "flow_asm_linear.py"), new_s], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=1200)
    out = r.stdout.decode(errors="replace")
    lines = [l for l in out.splitlines() if l.startswith(("ok", "FAIL"))]
    assert r.returncode == 0 and len(lines) == 256 and all(l.startswith("ok") and "relay" in l for l in lines), out


@pytest.mark.skipif(NO_HIPCC, reason="hipcc not available")
def test_they_neither_spill_nor_lose_a_wave_of_occupancy(new_s, tmp_path):
    par = str(tmp_path / "parents.s")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "--cuda-device-only", "-S", "-o", par,
                        os.path.join(TOOLS, "flow_inst.hip")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=1200)
    assert r.returncode == 0, r.stdout.decode(errors="replace")[-2000:]
    r = subprocess.run([sys.executable, os.path.join(TOOLS, "relay_regs.py"), par, new_s], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    out = r.stdout.decode(errors="replace")
    assert r.returncode == 0 and "256 new instantiations; all within" in out, out[-4000:]
