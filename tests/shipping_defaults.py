"""The library's shipping configuration for a test module of its own.

tests/conftest.py pins three of the library's defaults off for the whole session so that most of the suite can compare bits
(gs_bw_inorder = 1, gs_wave_quad = 0, tail_dense_rows = 0).  `shipping_defaults()` undoes that for the duration of a with
block — and only for it:

1. it reads the COMPILED-IN value of every tunable, for both instances of the library, in a fresh child process that sets
   none (no GPU work: the values are host globals);
2. it saves the values this process holds now (amgh_debug_get_tunable);
3. it applies the compiled-in values and yields;
4. it puts the saved values back in a `finally` and asserts that they read back.

Some tunables take effect only when a hierarchy is built (gs_wave_quad, tail_dense_rows, gs_bw*): handles meant to run the
shipping configuration must be created inside the block.  `pinned()` sets a few tunables for a nested block and restores
exactly what it found (unlike test_gpu_flow.tunables, which restores the suite's pins)."""
import contextlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = ("float64", "float32")

# every name amgh_debug_set_tunable accepts (tests/test_tunable_names_host.py holds this list equal to the source's)
TUNABLES = (
    "gs_block_inverse", "gs_lpr", "gs_il", "trim_coded", "gs_wave_quad", "pcg_fused", "tail_dense_rows", "tail_dense",
    "gs_lean", "gs_sell", "gs_tiny", "gs_bw", "gs_bw_rows", "gs_bw_chain", "gs_bw_flow", "gs_bw_spin", "gs_bw_nc",
    "gs_bw_nrhs", "gs_bw_skip_pub", "gs_bw_two_min_rows", "gs_flow_xzero", "gs_bw_dict", "gs_bw_inorder", "stream_code",
    "gs_bw_relay", "rhs_il", "jacobi_zero", "gs_ept", "gs_merge", "gs_coarse_lo", "gs_dense_tri", "gs_dense_blk",
    "gs_bigslot", "gs_super", "gs_block_pipe",
)

_CHILD = r"""
import ctypes, json, sys
sys.path.insert(0, sys.argv[1])
import amg_amd as AMG
names = json.loads(sys.argv[2])
out = {}
for dt in ("float64", "float32"):
    lib = AMG.hip_lib(dt)
    vals = {}
    for n in names:
        v = ctypes.c_int(0)
        rc = lib.amgh_debug_get_tunable(n.encode(), ctypes.byref(v))
        if rc != 0:
            raise SystemExit("amgh_debug_get_tunable(%r) = %d in the %s library" % (n, rc, dt))
        vals[n] = v.value
    out[dt] = vals
print(json.dumps(out))
"""

_compiled = None


def compiled_defaults():
    """{dtype: {name: value}} as a process that never set a tunable holds them (computed once per session)."""
    global _compiled
    if _compiled is None:
        env = {k: v for k, v in os.environ.items() if not k.startswith("AMGH_")}   # (AMGH_LEAN etc. are read at build, not here)
        r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, json.dumps(list(TUNABLES))], stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE, env=env, timeout=300)
        if r.returncode != 0:
            raise RuntimeError("reading the compiled-in tunables failed:\n" + r.stderr.decode(errors="replace")[-2000:])
        _compiled = json.loads(r.stdout.decode().strip().splitlines()[-1])
    return _compiled


def get_tunable(lib, name):
    import ctypes
    v = ctypes.c_int(0)
    rc = lib.amgh_debug_get_tunable(name.encode(), ctypes.byref(v))
    assert rc == 0, (name, rc)
    return v.value


def set_tunable(lib, name, value):
    rc = lib.amgh_debug_set_tunable(name.encode(), int(value))
    assert rc == 0, (name, value, rc)


def _libs():
    import amg_amd as AMG
    return {dt: AMG.hip_lib(dt) for dt in DTYPES}


def _snapshot(libs):
    return {dt: {n: get_tunable(lib, n) for n in TUNABLES} for dt, lib in libs.items()}


def _apply(libs, values):
    for dt, lib in libs.items():
        for n in TUNABLES:
            set_tunable(lib, n, values[dt][n])


@contextlib.contextmanager
def shipping_defaults():
    """Both libraries at their compiled-in tunables inside the block; the caller's values restored (and checked) after it."""
    want = compiled_defaults()
    libs = _libs()
    saved = _snapshot(libs)
    try:
        _apply(libs, want)
        assert _snapshot(libs) == want
        yield want
    finally:
        _apply(libs, saved)
        assert _snapshot(libs) == saved


@contextlib.contextmanager
def pinned(lib, **kw):
    """Set tunables of one library for a nested block; put back exactly the values found."""
    saved = {k: get_tunable(lib, k) for k in kw}
    try:
        for k, v in kw.items():
            set_tunable(lib, k, v)
        yield
    finally:
        for k, v in saved.items():
            set_tunable(lib, k, v)
