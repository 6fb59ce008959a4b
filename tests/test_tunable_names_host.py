"""The tunable names tests/shipping_defaults.py saves and restores are exactly the names the library accepts (no GPU needed):
read from the source of amgh_debug_set_tunable and amgh_debug_get_tunable, and from the compiled libraries themselves."""
import os
import re

import amg_amd as AMG
from conftest import ROOT
from shipping_defaults import TUNABLES, compiled_defaults, get_tunable

SRC = os.path.join(ROOT, "algebraicmultigrid.jl_amd", "csrc", "hip", "amghip.hip")


def _names_in(fn):
    txt = open(SRC).read()
    m = re.search(r"\nint " + fn + r"\(const char\* name, [^)]*\) \{\n(.*?)\n\}\n", txt, flags=re.S)
    assert m, fn
    return re.findall(r'strcmp\(name, "([^"]*)"\)', m.group(1))


def test_helper_list_is_the_setters_names():
    names = _names_in("amgh_debug_set_tunable")
    assert len(names) == len(set(names))
    assert set(names) == set(TUNABLES) and len(TUNABLES) == len(set(TUNABLES))


def test_getter_accepts_the_same_names_as_the_setter():
    assert _names_in("amgh_debug_get_tunable") == _names_in("amgh_debug_set_tunable")


def test_compiled_in_values_are_the_shipping_defaults():
    """A fresh process reads every tunable of both libraries; the three defaults the suite's conftest pins off are on there,
    and this process (pinned) differs from it in exactly those three."""
    d = compiled_defaults()
    for dt in ("float64", "float32"):
        assert set(d[dt]) == set(TUNABLES)
        assert d[dt]["gs_bw_inorder"] == 0 and d[dt]["gs_wave_quad"] == 1 and d[dt]["tail_dense_rows"] == 6144
        assert d[dt]["tail_dense"] == 1
        here = {n: get_tunable(AMG.hip_lib(dt), n) for n in TUNABLES}
        assert {n for n in TUNABLES if here[n] != d[dt][n]} == {"gs_bw_inorder", "gs_wave_quad", "tail_dense_rows"}
