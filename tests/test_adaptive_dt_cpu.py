"""The adaptive time step of wcsph / pcisph / iisph / pbf without a GPU (tests/adaptive_dt.py): the rule restated in numpy f32, the inputs of the
GPU suite shown fair on the oracle alone, the config keys and the mirrors' defaults.

Bounds used here and why: a time step "inside the bounds" is compared with `<` on f32 values, no tolerance.  dt_1 is compared with the value the
rule gives for the seed's maximum (a property of the generator: 2.451e-4 at amplitude 10, 9.802e-4 at 2.5, four digits): rel 1e-3."""
import json
import os

import numpy as np
import pytest

import adaptive_dt as ad
import harness as h
import particle_flow as pf
from cfd_taichi_amd import _native as nat
from cfd_taichi_amd import scenes
from oracle import oracle as orc

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the rule ------------------------------------------------------------------------------------------------------------------------------
def test_rule_at_rest_takes_max_dt_through_infinity():
    assert ad.rule(np.zeros((5, 3), np.float32), 5e-4, 1e-5) == F(5e-4)
    assert ad.rule(np.zeros((0, 3), np.float32), 5e-4, 1e-5) == F(5e-4)


def test_rule_clamps_and_passes():
    v = np.float32([[3, 4, 0], [0, 0, 1]])                       # vmax = 5: m = f32(0.02) / 5 * 0.2 = 8e-4
    m = F(F(F(0.4 * 0.025 * 2) / F(5)) * F(0.2))
    assert abs(float(m) - 8e-4) < 1e-9
    assert ad.rule(v, 1e-3, 1e-5) == m
    assert ad.rule(v, 5e-4, 1e-5) == F(5e-4)
    assert ad.rule(v, 1e-2, 1e-3) == F(1e-3)
    assert ad.rule(v, 1e-3, 1e-5, rigid=F(5)) == F(F(F(0.02) / F(10)) * F(0.2))


def test_rule_is_rounded_per_operation():
    """products and sums round separately (no contraction): a case where (x x + y y) + z z differs from the f64 norm rounded once"""
    rng = np.random.default_rng(3)
    v = rng.uniform(-1, 1, (4096, 3)).astype(np.float32)
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    per_op = np.sqrt((x * x + y * y) + z * z)
    once = np.sqrt((v.astype(np.float64) ** 2).sum(axis=1)).astype(np.float32)
    assert (per_op != once).any() and ad.vmax_of(v) == per_op.max()


def test_rigid_term():
    pos = np.float32([[1, 0, 0], [0, 2, 0]])
    t = ad.rigid_term(pos, [0, 0, 0], [0, 3, 4], [0, 0, 1])      # |vel| = 5, |omega x r| = 1 and 2
    assert t == F(7)
    assert ad.rigid_term(pos, [np.nan] * 3, [0, 0, 0], [0, 0, 0]) == F(0)


def test_pcisph_delta_follows_the_oracle_of_that_step():
    """a fresh oracle constructed with delta_time = dt gives the delta that the neighbourhood sums S of construction give under dt:
    delta = fl(1 / fl(S * fl(beta(dt)))), so against the oracle of the configured step delta / delta_0 = beta_0 / beta to within the four
    roundings involved (2 per delta, each 2^-24 relative: bound 4 * 2^-23).  The GPU suite compares the handle's delta with such an oracle's,
    bit for bit."""
    cfg = pf.config("pcisph", "wall", 640)
    o = h.make_oracle(cfg)
    d0 = F(o.pcisph_delta)
    o.close()
    m = 1000 * (0.025 ** 3) * 8
    for dt in (F(9.802e-4), F(5.1e-4), F(1.2345e-3)):
        o = h.make_oracle(ad.with_dt(cfg, dt))
        d = F(o.pcisph_delta)
        o.close()
        # delta scales with 1 / (float)beta: the ratio of the two deltas is the ratio of the betas to within three roundings
        b0, b = F(1e-3 * 1e-3 * m * m * 2 / 1e6), F(float(dt) * float(dt) * m * m * 2 / 1e6)
        assert abs(float(d) / float(d0) - float(b0) / float(b)) < 4 * 2.0 ** -23 * float(b0) / float(b)
        assert np.isfinite(d) and d > 0


# ---- the inputs of the GPU suite are fair ----------------------------------------------------------------------------------------------------
DT_1 = {"wcsph": 2.451e-4, "pbf": 2.451e-4, "iisph": 9.802e-4, "pcisph": 9.802e-4}


@pytest.mark.parametrize("walls", ["wall", "clamp"])
@pytest.mark.parametrize("solver", ad.SOLVERS)
def test_lockstep_inputs_stay_strictly_inside_the_bounds(solver, walls):
    """8 steps on the oracle alone: every dt_k strictly between min_dt and max_dt (the GPU suite never compares a clamped value by accident),
    the state finite, no particle lost"""
    dts, o = ad.oracle_run(solver, walls)
    max_dt, min_dt = ad.bounds(solver)
    print(solver, walls, [float(d) for d in dts])
    assert abs(float(dts[0]) / DT_1[solver] - 1) < 1e-3
    assert len(dts) == ad.STEPS and all(F(min_dt) < d < F(max_dt) for d in dts), dts
    assert np.isfinite(o.get(orc.F_POS)).all() and np.isfinite(o.get(orc.F_VEL)).all() and o.lost == 0
    o.close()


def test_set_dt_writes_all_three_for_every_solver():
    """Oracle.set_dt is what the GPU suite drives the oracle with: delta_time reads back, for every solver"""
    for solver in ad.SOLVERS:
        o = h.make_oracle(pf.config(solver, "wall", 640))
        o.set_dt(float(F(3.21e-4)))
        assert F(o.dt) == F(3.21e-4)
        o.close()


# ---- config and mirrors ----------------------------------------------------------------------------------------------------------------------
def cfg_with(**solver_keys):
    cfg = scenes.get("breaking_dam_30k_iisph")
    cfg["solver"].update(solver_keys)
    return cfg


def test_config_keys_are_optional_and_ordered():
    assert nat.adaptive_dt_calls(cfg_with()) == []
    assert nat.adaptive_dt_calls(cfg_with(adaptive_dt=False, max_dt=1e-3)) == [("step_max_dt", 1e-3)]
    assert nat.adaptive_dt_calls(cfg_with(adaptive_dt=True)) == [("step_adaptive_dt", 1.0)]
    assert nat.adaptive_dt_calls(cfg_with(adaptive_dt=True, min_dt=1e-4, max_dt=2e-3)) == [("step_max_dt", 2e-3), ("step_min_dt", 1e-4), ("step_adaptive_dt", 1.0)]


def test_config_keys_under_dfsph_are_the_references_own():
    cfg = cfg_with(adaptive_dt=True, max_dt=2e-3)
    cfg["solver"]["name"] = "dfsph"
    assert nat.adaptive_dt_calls(cfg) == []
    assert nat.adaptive_dt_calls(cfg_with(adaptive_dt=True), solver_name="dfsph") == []
    assert nat.adaptive_dt_calls(cfg, solver_name="iisph") == [("step_max_dt", 2e-3), ("step_adaptive_dt", 1.0)]


@pytest.mark.parametrize("key,value", [("max_dt", 0.0), ("max_dt", -1e-3), ("min_dt", float("nan")), ("min_dt", float("inf")), ("max_dt", "1e-3"),
                                       ("max_dt", True), ("adaptive_dt", "yes"), ("adaptive_dt", 2)])
def test_config_refuses_what_the_library_would(key, value):
    with pytest.raises(ValueError):
        nat.adaptive_dt_calls(cfg_with(**{key: value}))


def test_parameter_table_names_the_three_ids():
    assert [nat.SOLVER_PARAMS[k] for k in ("step_adaptive_dt", "step_max_dt", "step_min_dt")] == [ad.P_ADAPTIVE, ad.P_MAX_DT, ad.P_MIN_DT] == [77, 78, 79]
    with open(os.path.join(ROOT, "include", "sph_mi355x.h")) as f:
        header = f.read()
    for name, num in (("SPH_P_STEP_ADAPTIVE_DT", 77), ("SPH_P_STEP_MAX_DT", 78), ("SPH_P_STEP_MIN_DT", 79)):
        assert "#define %s %d " % (name, num) in header


def test_shipped_scene():
    cfg = scenes.get("dam_adaptive_iisph")
    base = scenes.get("breaking_dam_30k_iisph")
    assert cfg["solver"]["adaptive_dt"] is True and cfg["solver"]["max_dt"] == 2e-3 and "min_dt" not in cfg["solver"]
    for k in ("adaptive_dt", "max_dt"):
        del cfg["solver"][k]
    assert cfg == base
    with open(os.path.join(ROOT, "config", "dam_adaptive_iisph.json")) as f:
        assert json.load(f) == scenes.get("dam_adaptive_iisph")


class FakeHandle:
    """what solver_base._forward_attributes needs of a Simulation"""

    def __init__(self, delta_time):
        self.values = {"step_adaptive_dt": 0.0, "step_max_dt": delta_time, "step_min_dt": 1e-5}
        self.calls = []

    def param(self, name):
        return self.values[name]

    def set_param(self, name, value):
        self.calls.append((name, value))
        self.values[name] = value


def mirror(cls, config):
    """a mirror's attribute handling without a handle: the class's tables and solver_base's methods on a bare object"""
    from cfd_taichi_amd.solver_base import solver_base
    m = object.__new__(cls)
    solver_base._adaptive_dt_attributes(m, config)
    m._sim = FakeHandle(config["solver"]["delta_time"])
    return m


def test_mirror_defaults_and_live_forwarding():
    from cfd_taichi_amd.iisph_solver import iisph_solver
    from cfd_taichi_amd.pbf_solver import pbf_solver
    from cfd_taichi_amd.pcisph_solver import pcisph_solver
    from cfd_taichi_amd.wcsph_solver import wcsph_solver
    from cfd_taichi_amd.dfsph_solver import dfsph_solver
    assert "adaptive_dt" not in dfsph_solver._LIVE and "adaptive_dt" in dfsph_solver._BAKED          # dfsph keeps the reference's, baked ...
    d = object.__new__(dfsph_solver)                                                               # ... and sends them under their own names (70-72)
    for name in dfsph_solver._BAKED + dfsph_solver._LIVE:
        setattr(d, name, 1.0)

    class Dfsph(FakeHandle):
        def param(self, name):
            return 5e-4 if name == "max_dt" else 1.0
    d._sim = Dfsph(1e-3)
    d.max_dt = 2e-4
    d._forward_attributes()
    assert d._sim.calls == [("max_dt", 2e-4)]
    for cls in (wcsph_solver, pcisph_solver, iisph_solver, pbf_solver):
        assert cls._LIVE == ("max_dt", "min_dt", "adaptive_dt")
        m = mirror(cls, cfg_with())
        assert (m.adaptive_dt, m.max_dt, m.min_dt) == (False, 2.5e-4, 1e-5)
        m._BAKED = ()
        m._forward_attributes()
        assert m._sim.calls == []                                                                   # the defaults are the library's: nothing sent
        m.adaptive_dt, m.max_dt = True, 1e-3
        m._forward_attributes()
        assert m._sim.calls == [("step_max_dt", 1e-3), ("step_adaptive_dt", 1.0)]                   # the bounds before the switch
        m._forward_attributes()
        assert len(m._sim.calls) == 2
        m.adaptive_dt = False                                                                       # live: a later edit is forwarded too
        m._forward_attributes()
        assert m._sim.calls[-1] == ("step_adaptive_dt", 0.0)
    m = mirror(iisph_solver, cfg_with(adaptive_dt=True, max_dt=2e-3, min_dt=1e-4))
    assert (m.adaptive_dt, m.max_dt, m.min_dt) == (True, 2e-3, 1e-4)
