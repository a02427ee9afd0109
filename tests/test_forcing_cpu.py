"""CPU suite: gravity as a vector, constant or harmonic -- the test helper (tests/forcing.py) against the untouched second restatement, and the
pure-Python config reading (scene.gravity as a number or a list of three, scene.forcing)."""
import copy

import numpy as np
import pytest

from cfd_taichi_amd import _native as nat
from cfd_taichi_amd import scenes
import coupled_scenes as cs
import forcing as fo
import restatement_compare as rc
from harness import same_bits
from second_restatement import Scene, Solver
from second_restatement_pbf import PbfSolver


@pytest.mark.parametrize("scene", ["wcsph_tiny_wall", "dfsph_tiny_wall", "pbf_tiny_wall"])
def test_helper_fed_the_default_vector_is_the_untouched_restatement(scene):
    """[0, -G, 0] through the helper, 5 steps: every field of the solver bit for bit"""
    cfg = scenes.get(scene)
    solver = cfg["solver"]["name"]
    G = cfg["scene"]["gravity"]
    mine = fo.run_restatement(cfg, [[0.0, -G, 0.0]] * 5)
    ref = PbfSolver(cfg) if solver == "pbf" else Solver(cfg)
    if solver == "dfsph":
        ref.max_dens = 100
    with np.errstate(all="ignore"):
        for _ in range(5):
            ref.step()
    for attr in rc.FIELDS[solver]:
        same_bits(getattr(ref, attr), getattr(mine, attr), "%s: %s" % (scene, attr))
    assert fo.stats_of(ref) == fo.stats_of(mine)


def test_forced_body_fed_the_default_vector_is_the_untouched_body():
    """the coupled tiny scene (wcsph), 3 steps with the body step behind each: ForcedBody hands kinematic the same three floats"""
    cfg = cs.coupled("wcsph")
    G = cfg["scene"]["gravity"]
    mine = fo.run_restatement(cfg, [[0.0, -G, 0.0]] * 3, rg=cs.rigid(cfg))
    ref = Solver(cfg, cs.rigid(cfg))
    with np.errstate(all="ignore"):
        for _ in range(3):
            ref.step()
            ref.rigid_step()
    assert isinstance(mine.body, fo.ForcedBody) and not isinstance(ref.body, fo.ForcedBody)
    for what in ("pos", "vel"):
        same_bits(getattr(ref, what), getattr(mine, what), "fluid " + what)
    for what in ("pos", "centroid", "vel", "omega", "acc"):
        same_bits(getattr(ref.body, what), getattr(mine.body, what), "body " + what)


def test_forced_body_reads_the_vector():
    cfg = cs.coupled("wcsph")
    a = fo.run_restatement(cfg, [fo.TILT], rg=cs.rigid(cfg))
    b = fo.run_restatement(cfg, [fo.default_vector(cfg)], rg=cs.rigid(cfg))
    d = a.body.acc.astype(np.float64) - b.body.acc.astype(np.float64)
    assert np.allclose(d, np.array(fo.TILT) - fo.default_vector(cfg).astype(np.float64), atol=1e-4), d


def test_accel_formula_and_ulp_distance():
    a = fo.accel_formula(fo.TILT, fo.AMP, fo.OMEGA, fo.PHASE, 0.0)
    assert a[0] == np.float32(-4.9) and a[1] == np.float32(-8.6)                  # sin(0) = 0; no amplitude on y
    assert a[2] == np.float32(np.float64(np.float32(2.0)) + 2.0 * np.sin(1.0))
    z = fo.accel_formula([-0.0, -9.8, 0.0], [0.0, 0.0, 1.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0], 3.0)
    assert np.signbit(z[0]) and not np.signbit(z[2])                             # an axis without amplitude keeps g's bits
    x = np.float32(1.5)
    assert fo.ulp_distance([x], [np.nextafter(x, np.float32(2))])[0] == 1 and fo.ulp_distance([np.float32(-0.0)], [np.float32(0.0)])[0] == 0


# ---- config reading -------------------------------------------------------------------------------------------------------------------------

def test_gravity_calls_number_list_and_block():
    cfg = scenes.get("dfsph_tiny_wall")
    assert nat.gravity_calls(cfg) == []                                             # a number: the handle keeps gravity * (0, -1, 0)
    assert nat.config_from_dict(cfg).gravity == 9.8
    vec = copy.deepcopy(cfg)
    vec["scene"]["gravity"] = [-4.9, -8.6, 2]
    assert nat.gravity_calls(vec) == [("set_gravity", [-4.9, -8.6, 2.0])]
    assert nat.config_from_dict(vec).gravity == 8.6
    same = copy.deepcopy(cfg)
    same["scene"]["gravity"] = [0, -9.8, 0]
    assert nat.config_from_dict(same).gravity == 9.8 and nat.gravity_calls(same) == [("set_gravity", [0.0, -9.8, 0.0])]
    both = copy.deepcopy(vec)
    both["scene"]["forcing"] = {"amplitude": [3, 0, 2], "omega": [40, 0, 25], "phase": [0, 0, 1]}
    assert nat.gravity_calls(both) == [("set_gravity", [-4.9, -8.6, 2.0]), ("set_forcing", [3.0, 0.0, 2.0], [40.0, 0.0, 25.0], [0.0, 0.0, 1.0])]
    only_amp = copy.deepcopy(cfg)
    only_amp["scene"]["forcing"] = {"amplitude": [0, 0, 1]}
    assert nat.gravity_calls(only_amp) == [("set_forcing", [0.0, 0.0, 1.0], None, None)]


def test_gravity_calls_reach_the_target_in_order():
    class Target:
        def __init__(self):
            self.calls = []

        def set_gravity(self, vec):
            self.calls.append(("g", vec))

        def set_forcing(self, amp, omega=None, phase=None):
            self.calls.append(("f", amp, omega, phase))

    cfg = scenes.get("sloshing_dfsph")
    t = Target()
    nat.apply_gravity_calls(t, cfg)
    assert t.calls == [("f", [3.0, 0.0, 0.0], [6.0, 0.0, 0.0], [0.0, 0.0, 0.0])]


def test_a_library_without_the_calls_raises_state():
    """the new entry points are optional exports: on an implementation of the ABI that lacks them the calls raise SphError(SPH_E_STATE)"""
    assert {"sph_set_gravity", "sph_set_forcing"} <= set(nat.OPTIONAL_EXPORTS) and not {"sph_set_gravity", "sph_set_forcing"} & set(nat.CORE_EXPORTS)

    class OldLibrary:
        _name = "an older library"

    sim = nat.Simulation.__new__(nat.Simulation)
    sim._lib, sim._h = OldLibrary(), None
    for call in (lambda: sim.set_gravity([0.0, -9.8, 0.0]), lambda: sim.set_forcing([1.0, 0.0, 0.0])):
        with pytest.raises(nat.SphError) as e:
            call()
        assert e.value.code == nat.SPH_E_STATE


@pytest.mark.parametrize("bad", [[0, -9.8], [0, -9.8, 0, 0], [0, "down", 0], [0, float("nan"), 0], [0, float("inf"), 0], "0,-9.8,0", [0, [1], 0], [0, True, 0]])
def test_malformed_gravity_list_is_refused(bad):
    cfg = scenes.get("dfsph_tiny_wall")
    cfg["scene"]["gravity"] = bad
    with pytest.raises(ValueError):
        nat.gravity_calls(cfg)
    with pytest.raises(ValueError):
        nat.config_from_dict(cfg)


@pytest.mark.parametrize("bad", [{"omega": [1, 2, 3]}, {"amplitude": [1, 2]}, {"amplitude": [1, 2, 3], "frequency": [1, 2, 3]}, [1, 2, 3],
                                 {"amplitude": [1, 2, 3], "omega": [1, float("nan"), 3]}])
def test_malformed_forcing_block_is_refused(bad):
    cfg = scenes.get("dfsph_tiny_wall")
    cfg["scene"]["forcing"] = bad
    with pytest.raises(ValueError):
        nat.gravity_calls(cfg)


def test_sloshing_scene_is_small_and_matches_its_file():
    """config/sloshing_dfsph.json: a few thousand particles (the runner test steps it on the GPU), the tank about half full, forced along x only"""
    import json
    import os
    cfg = scenes.get("sloshing_dfsph")
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "config", "sloshing_dfsph.json")) as f:
        assert json.load(f) == cfg
    sc = Scene(cfg)
    assert 2000 <= sc.N <= 4000, sc.N
    top = float(sc.pos[:, 1].max()) + cfg["scene"]["particle_radius"]
    assert 0.4 <= top / cfg["scene"]["box_max"][1] <= 0.6, top
    (name, amp, omega, phase), = nat.gravity_calls(cfg)
    assert name == "set_forcing" and amp[0] != 0 and amp[1] == amp[2] == 0 and omega[0] > 0
