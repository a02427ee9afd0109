"""CPU suite: sph_slab_set_state (start a sharded run from any state) is declared by the header, exported by the built library and listed by the binding."""
import os
import re

from cfd_taichi_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_slab_set_state_is_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "sph_mi355x.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\bint\s+sph_slab_set_state\s*\(([^)]*)\)\s*;", text)
    assert m, "include/sph_mi355x.h does not declare sph_slab_set_state"
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert args == ["SphHandle *h", "const float *pos", "const float *vel", "const float *scalar", "size_t n_fluid", "double delta_time"], args
    assert re.search(r"#define\s+SPH_ABI_VERSION\s+5\b", text)          # additive: the version stays
    lib = _native.load()
    assert hasattr(lib, "sph_slab_set_state")
    assert "sph_slab_set_state" in _native.EXPORTS and "sph_slab_set_state" in _native.OPTIONAL_EXPORTS
    assert hasattr(_native.Simulation, "slab_set_state")
