"""GPU suite of the adaptive time step of wcsph / pcisph / iisph / pbf handles (SPH_P_STEP_ADAPTIVE_DT / _MAX_DT / _MIN_DT; DESIGN.md section 6h;
tests/adaptive_dt.py restates the rule, test_adaptive_dt_cpu.py shows the inputs fair on the oracle alone).

Every comparison is bit for bit (harness.same_bits: np.array_equal on the u32 views; scalars through np.float32 views); no tolerance is
involved.  Exact handles are held to the oracle driven with set_dt(dt_k) -- pcisph to a fresh oracle constructed with delta_time = dt_k --,
relaxed and Morton handles to a fixed-step twin that gets set_dt(dt_k) between steps."""
import os

import numpy as np
import pytest

import adaptive_dt as ad
import harness as h
import particle_flow as pf
from cfd_taichi_amd import _native as nat
from cfd_taichi_amd import run, scenes
from oracle import oracle as orc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def switch_on(sim, max_dt=None, min_dt=None):
    if max_dt is not None:
        sim.set_param("step_max_dt", max_dt)
    if min_dt is not None:
        sim.set_param("step_min_dt", min_dt)
    sim.set_param("step_adaptive_dt", 1)
    assert sim.param("step_adaptive_dt") == 1.0
    return sim


def same_scalar(a, b, what):
    assert h.bits(F(a)) == h.bits(F(b)), "%s: %r vs %r" % (what, float(a), float(b))


def reported_dt(sim, dt, when):
    """the three places a handle reports the step's dt"""
    same_scalar(sim.scalar(nat.S_DELTA_TIME), dt, when + ": SPH_S_DELTA_TIME")
    same_scalar(sim.scalar(nat.S_PS_DELTA_TIME), dt, when + ": SPH_S_PS_DELTA_TIME")
    if sim.cfg.solver in (nat.SOLVER_PCISPH, nat.SOLVER_IISPH):
        same_scalar(sim.last_stats.dt, dt, when + ": SphStepStats.dt")


def same_fields(a, b, when, fields=(nat.F_POS, nat.F_VEL, nat.F_RHO)):
    for f in fields:
        h.same_bits(a.download(f), b.download(f), "%s: field %d" % (when, f))


# ---- 1: lockstep against the oracle ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("walls", ["wall", "clamp"])
@pytest.mark.parametrize("solver", ad.SOLVERS)
def test_lockstep_against_the_oracle(solver, walls, monkeypatch):
    cfg = pf.config(solver, walls, 640)
    max_dt, min_dt = ad.bounds(solver)
    sim, o = h.make_handle(cfg, monkeypatch), h.make_oracle(cfg)
    vel = ad.velocities(sim.n_fluid, ad.AMPLITUDE[solver])
    sim.upload(nat.F_VEL, vel); o.set(orc.F_VEL, vel)
    switch_on(sim, max_dt, min_dt)
    clock = 0.0
    for k in range(ad.STEPS):
        when = "%s %s step %d" % (solver, walls, k + 1)
        dt = ad.rule(sim.download(nat.F_VEL), max_dt, min_dt)
        assert F(min_dt) < dt < F(max_dt), (when, dt)                       # (test_adaptive_dt_cpu.py: never a clamped value)
        st = sim.step(1)
        o, ot = ad.oracle_step_dt(o, cfg, solver, dt)
        reported_dt(sim, dt, when)
        if solver == "pcisph":
            same_scalar(sim.scalar(nat.S_PCISPH_DELTA), o.pcisph_delta, when + ": SPH_S_PCISPH_DELTA")
        h.same_stats(st, ot, solver, when + ": statistics")
        pf.same_state(sim, o, solver, when)
        clock += float(dt)
        assert sim.time() == clock, (when, sim.time(), clock)
    sim.close(); o.close()


# ---- 2: the clamps -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", ad.SOLVERS)
def test_clamps(solver, monkeypatch):
    cfg = pf.config(solver, "wall", 640)
    max_dt, min_dt = ad.bounds(solver)
    sim = switch_on(h.make_handle(cfg, monkeypatch), max_dt, min_dt)
    sim.step(1)                                                             # from rest: vmax = 0, m = +inf
    reported_dt(sim, F(max_dt), solver + " from rest")
    vel = ad.velocities(sim.n_fluid, ad.AMPLITUDE[solver]) * F(8)           # dt_1 / 8 lies below min_dt = DT / 4 for every solver (dt_1 < DT)
    sim.upload(nat.F_VEL, vel)
    assert ad.rule(vel, max_dt, 1e-9) < F(min_dt) and ad.rule(vel, max_dt, min_dt) == F(min_dt)
    sim.step(1)
    reported_dt(sim, F(min_dt), solver + " fast")
    sim.close()
    # max_dt left at its default: never above the configured step
    sim = h.make_handle(cfg, monkeypatch)
    sim.set_param("step_adaptive_dt", 1)
    assert sim.param("step_max_dt") == pf.DT[solver] and sim.param("step_min_dt") == 1e-5
    for k in range(3):                                                      # from rest: the configured step, until the rule asks for less
        dt = ad.rule(sim.download(nat.F_VEL), pf.DT[solver], 1e-5)
        sim.step(1)
        assert dt <= F(pf.DT[solver]) and (k > 0 or dt == F(pf.DT[solver]))
        reported_dt(sim, dt, "%s default max_dt, step %d" % (solver, k + 1))
    sim.upload(nat.F_VEL, ad.velocities(sim.n_fluid, ad.AMPLITUDE[solver]))
    v = sim.download(nat.F_VEL)
    sim.step(1)
    dt = ad.rule(v, pf.DT[solver], 1e-5)
    assert dt < F(pf.DT[solver])
    reported_dt(sim, dt, solver + " default max_dt, moving")
    sim.close()


# ---- 3: other sweep modes, against a host-driven twin -------------------------------------------------------------------------------------------
# (iisph's relaxed sweeps are the staged ones: they exist on Morton cells only)
TWINS = [("wcsph", h.MORTON, "exact"), ("wcsph", None, "relaxed"), ("wcsph", h.MORTON, "relaxed"), ("iisph", h.MORTON, "exact"), ("iisph", h.MORTON, "relaxed")]


@pytest.mark.parametrize("solver,env,arith", TWINS, ids=["%s-%s%s" % (s, "morton-" if e else "", a) for s, e, a in TWINS])
def test_equals_a_host_driven_twin(solver, env, arith, monkeypatch):
    cfg = pf.config(solver, "wall", 640)
    max_dt, min_dt = ad.bounds(solver)
    a, b = h.make_handle(cfg, monkeypatch, env, arith), h.make_handle(cfg, monkeypatch, env, arith)
    if arith == "relaxed":
        assert a.scalar(nat.S_ARITH_RELAXED) == 1.0
    vel = ad.velocities(a.n_fluid, ad.AMPLITUDE[solver])
    a.upload(nat.F_VEL, vel); b.upload(nat.F_VEL, vel)
    switch_on(a, max_dt, min_dt)
    dts = []
    for k in range(ad.STEPS):
        when = "%s step %d" % (solver, k + 1)
        dt = ad.rule(a.download(nat.F_VEL), max_dt, min_dt)
        sa = a.step(1)
        reported_dt(a, dt, when)
        b.set_dt(float(dt))
        sb = b.step(1)
        h.same_stats(sa, sb, solver, when + ": statistics")
        same_fields(a, b, when)
        dts.append(dt)
    assert len(set(float(d) for d in dts)) > 1
    assert a.time() == b.time()
    if solver == "wcsph" and arith == "relaxed":
        assert a.scalar(nat.S_VERLET_BUILDS) == b.scalar(nat.S_VERLET_BUILDS) > 0
    a.close(); b.close()


# ---- 4: asynchrony -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", ad.SOLVERS)
def test_one_call_of_six_steps_equals_six_calls(solver, monkeypatch):
    cfg = pf.config(solver, "wall", 640)
    max_dt, min_dt = ad.bounds(solver)
    a, b = h.make_handle(cfg, monkeypatch), h.make_handle(cfg, monkeypatch)
    vel = ad.velocities(a.n_fluid, ad.AMPLITUDE[solver])
    for s in (a, b):
        s.upload(nat.F_VEL, vel)
        switch_on(s, max_dt, min_dt)
    a.step(6)
    for _ in range(6):
        b.step(1)
    same_fields(a, b, solver + " step(6) against 6 x step(1)")
    for which in (nat.S_DELTA_TIME, nat.S_PS_DELTA_TIME, nat.S_PCISPH_DELTA):
        same_scalar(a.scalar(which), b.scalar(which), "scalar %d" % which)
    assert a.time() == b.time() and a.time() > 0
    if solver == "wcsph":
        assert a.scalar(nat.S_GRAPH_LAUNCHES) > 0 and b.scalar(nat.S_GRAPH_LAUNCHES) == 0
        a.set_param("step_adaptive_dt", 0)                                  # the captured pairs hold the two nodes: dropped with the switch
        before = a.scalar(nat.S_GRAPH_LAUNCHES)
        dt = a.scalar(nat.S_DELTA_TIME)
        a.step(2)
        b.set_param("step_adaptive_dt", 0)
        b.step(1); b.step(1)
        assert a.scalar(nat.S_GRAPH_LAUNCHES) == before + 1 and a.scalar(nat.S_DELTA_TIME) == dt == b.scalar(nat.S_DELTA_TIME)
        same_fields(a, b, "wcsph, switched off: the last dt stays")
    a.close(); b.close()


# ---- 5: with inlets ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", ["wcsph", "iisph", "pbf"])
def test_added_particles_set_the_next_step(solver, monkeypatch):
    """(not pcisph: the oracle of the 704 lattice has that lattice's delta, the handle keeps the 640 lattice's -- test_particle_flow_gpu.py's subject,
    and recomputing the sums after the count changes is not this feature's)"""
    cfg = pf.config(solver, "wall", 640, capacity=704)
    max_dt = 2 * pf.DT[solver]
    sim = switch_on(h.make_handle(cfg, monkeypatch), max_dt)
    sim.step(3)
    before = h.fluid_state(sim, solver)
    new = pf.layer_above(cfg, 640, 64)
    fast = np.tile(F([0, -20, 0]), (64, 1))
    assert sim.add_particles(new, fast) == 640 and sim.n_fluid == 704
    st = {"pos": np.concatenate([before["pos"], new]), "vel": np.concatenate([before["vel"], fast])}
    if solver == "iisph":
        st["p_past"] = np.concatenate([before["p_past"], np.zeros(64, np.float32)])
    dt = ad.rule(st["vel"], max_dt, 1e-5)
    same_scalar(dt, F(F(F(0.4 * 0.025 * 2) / F(20)) * F(0.2)), "the rule's value for 20 m/s")
    assert F(1e-5) < dt < F(max_dt) and dt != F(before["dt"])
    cfg704 = pf.config(solver, "wall", 704)
    o = h.give(h.make_oracle(cfg704), st, solver)
    stats = sim.step(1)
    o, ot = ad.oracle_step_dt(o, cfg704, solver, dt)
    reported_dt(sim, dt, solver + " after add_particles")
    h.same_stats(stats, ot, solver, "statistics")
    pf.same_state(sim, o, solver, solver + " after add_particles")
    sim.close(); o.close()


# ---- 6: with a body --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", ["wcsph", "iisph"])
def test_with_a_body(solver):
    import rigid_release as rr
    from test_rigid_modes_gpu import check_rigid
    cfg = rr.scene(solver, active=True)
    radius = cfg["scene"]["particle_radius"]
    max_dt, min_dt = 2 * rr.DT[solver], rr.DT[solver] / 64                 # (the amplitudes of the lockstep cases: dt_1 just under DT)
    sim = nat.Simulation(nat.config_from_dict(cfg), rigid=rr.rigid(cfg))
    o = rr.body_oracle(cfg, solver)
    vel = ad.velocities(sim.n_fluid, ad.AMPLITUDE[solver])
    sim.upload(nat.F_VEL, vel); o.set(orc.F_VEL, vel)
    switch_on(sim, max_dt, min_dt)
    terms = []
    for k in range(10):
        when = "%s coupled step %d" % (solver, k + 1)
        sc = sim.rigid_scalars()
        term = ad.rigid_term(sim.download(nat.F_RIGID_POS, nat.SPECIES_RIGID), sc["centroid"], sc["vel"], sc["omega"])
        dt = ad.rule(sim.download(nat.F_VEL), max_dt, min_dt, radius=radius, rigid=term)
        assert F(min_dt) < dt < F(max_dt), (when, dt)
        terms.append(float(term))
        st = sim.step(1)
        o.set_dt(float(dt))
        ot = h.oracle_step(o, solver)
        reported_dt(sim, dt, when)
        if h.stats_tuple(ot, solver):
            assert h.stats_tuple(st, solver) == h.stats_tuple(ot, solver), when
        h.same_bits(sim.download(nat.F_RIGID_FORCE, nat.SPECIES_RIGID), o.get(orc.F_RIGID_FORCE), when + ": force on the body")
        sim.rigid_step(); o.rigid_step()                                   # both take ps.delta_time = dt_k
        check_rigid(sim, o, "after rigid " + when, nan_aware=False)
        pf.same_state(sim, o, solver, when)
    assert terms[0] == 0.0 and terms[-1] > 0.0                              # the body started at rest and moves by the end: its term took part
    sim.close(); o.close()


# ---- 7: refusals leave the handle unchanged ----------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_unchanged(monkeypatch):
    # a dfsph handle has 70-72
    cfg = pf.config("dfsph", "wall", 640)
    a, b = h.make_handle(cfg, monkeypatch), h.make_handle(cfg, monkeypatch)
    for name, value in (("step_adaptive_dt", 1), ("step_max_dt", 5e-4), ("step_min_dt", 1e-4)):
        h.refused(nat.SPH_E_STATE, lambda: a.set_param(name, value))
    for s in range(3):
        sa, sb = a.step(1), b.step(1)
        h.same_stats(sa, sb, "dfsph", "dfsph step %d: statistics" % (s + 1))
    same_fields(a, b, "dfsph after refused calls", (nat.F_POS, nat.F_VEL, nat.F_RHO, nat.F_WARM_K))
    a.close(); b.close()
    # a slab handle (its ranks would need a max all-reduce)
    cfg = pf.config("wcsph", "wall", 640)
    for k in h.KNOBS:
        monkeypatch.delenv(k, raising=False)
    slab = nat.Simulation(nat.config_from_dict(cfg, slab_rank=0, slab_count=2))
    for name, value in (("step_adaptive_dt", 1), ("step_max_dt", 5e-4), ("step_min_dt", 1e-4)):
        h.refused(nat.SPH_E_STATE, lambda: slab.set_param(name, value))
    assert (slab.param("step_adaptive_dt"), slab.param("step_max_dt"), slab.param("step_min_dt")) == (0.0, pf.DT["wcsph"], 1e-5)
    slab.close()
    # bounds that are not finite or not positive, a flag that is neither 0 nor 1
    for solver in ("wcsph", "pcisph"):
        cfg = pf.config(solver, "wall", 640)
        a, b = h.make_handle(cfg, monkeypatch), h.make_handle(cfg, monkeypatch)
        vel = ad.velocities(a.n_fluid, ad.AMPLITUDE[solver])
        max_dt, min_dt = ad.bounds(solver)
        for s in (a, b):
            s.upload(nat.F_VEL, vel)
            switch_on(s, max_dt, min_dt)
        for name in ("step_max_dt", "step_min_dt"):
            for value in (0.0, -1e-3, float("nan"), float("inf"), -float("inf")):
                h.refused(nat.SPH_E_INVALID, lambda: a.set_param(name, value))
        for value in (2.0, -1.0, 0.5, float("nan")):
            h.refused(nat.SPH_E_INVALID, lambda: a.set_param("step_adaptive_dt", value))
        assert (a.param("step_adaptive_dt"), a.param("step_max_dt"), a.param("step_min_dt")) == (1.0, max_dt, min_dt)
        a.step(4); b.step(4)
        same_fields(a, b, solver + " after refused calls")
        same_scalar(a.scalar(nat.S_DELTA_TIME), b.scalar(nat.S_DELTA_TIME), "dt")
        assert a.time() == b.time()
        a.close(); b.close()


# ---- 8: off is invisible ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", ad.SOLVERS)
def test_on_and_off_again_before_the_first_step_is_invisible(solver, monkeypatch):
    cfg = pf.config(solver, "wall", 640)
    a, b = h.make_handle(cfg, monkeypatch), h.make_handle(cfg, monkeypatch)
    vel = ad.velocities(a.n_fluid, ad.AMPLITUDE[solver])
    a.upload(nat.F_VEL, vel); b.upload(nat.F_VEL, vel)
    delta = a.scalar(nat.S_PCISPH_DELTA)
    switch_on(a, *ad.bounds(solver))
    a.set_param("step_adaptive_dt", 0)
    assert a.param("step_adaptive_dt") == 0.0 and a.scalar(nat.S_PCISPH_DELTA) == delta
    for s in range(5):
        sa, sb = a.step(1), b.step(1)
        h.same_stats(sa, sb, solver, "step %d: statistics" % (s + 1))
        same_fields(a, b, "%s step %d" % (solver, s + 1))
        assert a.scalar(nat.S_DELTA_TIME) == b.scalar(nat.S_DELTA_TIME) == float(F(pf.DT[solver]))
    assert a.time() == b.time() and a.scalar(nat.S_PS_DELTA_TIME) == b.scalar(nat.S_PS_DELTA_TIME)
    a.close(); b.close()


@pytest.mark.parametrize("solver", ["iisph", "pcisph"])
def test_switching_off_keeps_the_last_step(solver, monkeypatch):
    """dt -- and pcisph's delta -- stay where the last adaptive step left them: the handle goes on as a fixed handle given that dt (pcisph: as the
    oracle constructed with it)"""
    cfg = pf.config(solver, "wall", 640)
    max_dt, min_dt = ad.bounds(solver)
    sim, o = h.make_handle(cfg, monkeypatch), h.make_oracle(cfg)
    vel = ad.velocities(sim.n_fluid, ad.AMPLITUDE[solver])
    sim.upload(nat.F_VEL, vel); o.set(orc.F_VEL, vel)
    switch_on(sim, max_dt, min_dt)
    dt = None
    for k in range(3):
        dt = ad.rule(sim.download(nat.F_VEL), max_dt, min_dt)
        sim.step(1)
        o, _ = ad.oracle_step_dt(o, cfg, solver, dt)
    delta = sim.scalar(nat.S_PCISPH_DELTA)
    sim.set_param("step_adaptive_dt", 0)
    same_scalar(sim.scalar(nat.S_DELTA_TIME), dt, "dt after the switch")
    assert sim.scalar(nat.S_PCISPH_DELTA) == delta
    for k in range(3):
        st = sim.step(1)
        ot = h.oracle_step(o, solver)                                      # the oracle keeps dt (pcisph: and the delta of its construction with dt)
        h.same_stats(st, ot, solver, "fixed step %d: statistics" % (k + 1))
        same_scalar(st.dt, dt, "SphStepStats.dt")
    pf.same_state(sim, o, solver, solver + " three fixed steps after the switch")
    sim.close(); o.close()


# ---- 9: the shipped scene ----------------------------------------------------------------------------------------------------------------------------
def test_shipped_scene_through_the_runner(monkeypatch, capsys):
    for k in h.KNOBS:
        monkeypatch.delenv(k, raising=False)
    frames, t, _ = run.main(["--config", os.path.join(ROOT, "config", "dam_adaptive_iisph.json"), "--steps", "150"])
    capsys.readouterr()
    ps, solver, dts = run.LAST["ps"], run.LAST["solver"], run.LAST["frame_dt"]
    sim = ps._sim
    assert frames == 150 and len(dts) == 150 and solver.adaptive_dt is True and sim.param("step_adaptive_dt") == 1.0 and sim.param("step_max_dt") == 2e-3
    assert np.isfinite(sim.download(nat.F_POS)).all() and np.isfinite(sim.download(nat.F_VEL)).all() and sim.last_stats.lost == 0
    assert len(set(dts)) >= 2 and all(F(1e-5) <= F(d) <= F(2e-3) for d in dts), sorted(set(dts))[:5]
    clock = 0.0
    for d in dts:
        clock += d
    assert sim.time() == clock == t
    print("dam_adaptive_iisph: 150 steps to t = %.6f s, dt from %.3e to %.3e" % (t, min(dts), max(dts)))
    sim.close()
