"""GPU suite of the inlets and sinks: sph_add_particles / sph_remove_in_box and SphConfig.fluid_capacity on single-GPU handles
(tests/particle_flow.py; test_particle_flow_cpu.py checks the lattice counts and pcisph's delta on the oracle alone).

Every comparison is bit for bit (particle_flow.same: np.array_equal on the u32 views); no tolerance is involved.  Exact handles are held to the
oracle, relaxed handles to a fresh relaxed handle given the same state (rigid_release.give_sim) -- not iisph there: its last pressure, which a
step reads, cannot be uploaded into a handle."""
import os

import numpy as np
import pytest

import harness as h
import particle_flow as pf
from cfd_taichi_amd import _native as nat
from cfd_taichi_amd import mesh, run, scenes
from oracle import oracle as orc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def append_top(sim, top, calls=pf.ADD_CALLS):
    at, n0 = 0, sim.n_fluid
    for m in calls:
        assert sim.add_particles(top[at:at + m]) == n0 + at            # at rest
        at += m
        assert sim.n_fluid == n0 + at
    assert at == len(top)


# ---- 1: append at step 0 -------------------------------------------------------------------------------------------------------------------
def run_append(solver, walls, monkeypatch, env=None, n0=640, calls=pf.ADD_CALLS):
    o = h.make_oracle(pf.config(solver, walls, 832))
    sim = h.make_handle(pf.config(solver, walls, n0, capacity=832), monkeypatch, env)
    assert sim.n_fluid == n0 and sim.capacity == 832
    append_top(sim, o.get(orc.F_POS)[n0:], calls)
    assert sim.n_fluid == 832 and sim._shape(nat.SPECIES_FLUID, nat.F_POS) == (832, 3)
    h.same_bits(sim.download(nat.F_POS), o.get(orc.F_POS), "the appended lattice")
    assert not sim.download(nat.F_VEL).any() and not sim.download(nat.F_RHO)[n0:].any()
    pf.lockstep(sim, o, solver, 20, "%s %s append" % (solver, walls))
    sim.close(); o.close()


@pytest.mark.parametrize("walls", ["wall", "clamp"])
@pytest.mark.parametrize("solver", pf.SOLVERS)
def test_append_at_step_0(solver, walls, monkeypatch):
    run_append(solver, walls, monkeypatch)


@pytest.mark.parametrize("solver", pf.SOLVERS)
def test_append_at_step_0_morton(solver, monkeypatch):
    """Morton cells, and with them the staged sweeps of dfsph / pcisph / iisph"""
    run_append(solver, "wall", monkeypatch, env=h.MORTON)


def test_append_pcisph_from_704(monkeypatch):
    """the lattice pair on which max_index agrees too (test_particle_flow_cpu.py)"""
    run_append("pcisph", "wall", monkeypatch, n0=704, calls=(37, 27, 64))


# ---- 2 / 4: recycle mid-run ----------------------------------------------------------------------------------------------------------------------
def recycle(sim, solver, cfg):
    """remove the inner box, check the survivors against numpy, add as many on a layer above the surface falling at 1 m/s.  Returns the state
    the handle now holds, as rigid_release.give / give_sim take it."""
    before = h.fluid_state(sim, solver)
    lo, hi = pf.inner_box(cfg)
    gone = pf.in_box(before["pos"], lo, hi)
    r = sim.remove_in_box(lo, hi)
    assert 0 < r <= 64 and r == gone.sum() and sim.n_fluid == 640 - r
    h.same_bits(sim.download(nat.F_POS), before["pos"][~gone], "survivors: pos")
    h.same_bits(sim.download(nat.F_VEL), before["vel"][~gone], "survivors: vel")
    if solver == "dfsph":
        h.same_bits(sim.download(nat.F_WARM_K), before["warm_k"][~gone], "survivors: warm_start_k")
    new = pf.layer_above(cfg, 640, r)
    vel = np.tile(np.float32([0, -1, 0]), (r, 1))
    assert sim.add_particles(new, vel) == 640 - r and sim.n_fluid == 640
    st = {"pos": np.concatenate([before["pos"][~gone], new]), "vel": np.concatenate([before["vel"][~gone], vel]), "dt": sim.scalar(nat.S_DELTA_TIME)}
    h.same_bits(sim.download(nat.F_POS), st["pos"], "recycled: pos")
    h.same_bits(sim.download(nat.F_VEL), st["vel"], "recycled: vel")
    assert st["dt"] == before["dt"]
    if solver == "dfsph":
        st["warm_k"] = sim.download(nat.F_WARM_K)
        h.same_bits(st["warm_k"], np.concatenate([before["warm_k"][~gone], np.zeros(r, np.float32)]), "recycled: warm_start_k")
    if solver == "iisph":          # (the carried pressure has no download of its own between steps: what the call promises, checked by the lock step that follows)
        st["p_past"] = np.concatenate([before["p_past"][~gone], np.zeros(r, np.float32)])
    return st


@pytest.mark.parametrize("walls", ["wall", "clamp"])
@pytest.mark.parametrize("solver", pf.SOLVERS)
def test_recycle_mid_run(solver, walls, monkeypatch):
    cfg = pf.config(solver, walls, 640, capacity=704)
    sim, o = h.make_handle(cfg, monkeypatch), h.make_oracle(pf.config(solver, walls, 640))
    pf.lockstep(sim, o, solver, 10, "%s %s history" % (solver, walls), count=False)
    st = recycle(sim, solver, cfg)
    o.close()
    o = h.give(h.make_oracle(pf.config(solver, walls, 640)), st, solver)
    pf.lockstep(sim, o, solver, 30, "%s %s after the recycle" % (solver, walls))
    sim.close(); o.close()


@pytest.mark.parametrize("solver,env", [("wcsph", None), ("dfsph", None), ("pcisph", h.MORTON)])
def test_recycle_mid_run_relaxed(solver, env, monkeypatch):
    """wcsph (Verlet lists), dfsph and pcisph (staged sweeps) under the relaxed arithmetic, against a fresh relaxed handle given the same state"""
    cfg = pf.config(solver, "wall", 640, capacity=704)
    sim = h.make_handle(cfg, monkeypatch, env, arith="relaxed")
    assert sim.scalar(nat.S_ARITH_RELAXED) == 1.0
    sim.step(10)
    st = recycle(sim, solver, cfg)
    fresh = h.give_sim(h.make_handle(pf.config(solver, "wall", 640), monkeypatch, env, arith="relaxed"), st, solver)
    for s in range(30):
        a, b = sim.step(1), fresh.step(1)
        h.same_stats(a, b, solver, "step %d: statistics" % (s + 1))
        if (s + 1) % 5 == 0:
            for f in (nat.F_POS, nat.F_VEL, nat.F_RHO) + ((nat.F_WARM_K,) if solver == "dfsph" else ()):
                h.same_bits(sim.download(f), fresh.download(f), "step %d: field %d" % (s + 1, f))
    sim.build_neighbors(); fresh.build_neighbors()
    h.same_bits(sim.download(nat.F_NBR_COUNT), fresh.download(nat.F_NBR_COUNT), "neighbour count")
    sim.close(); fresh.close()


# ---- 3: remove at step 0 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", pf.SOLVERS)
def test_remove_at_step_0(solver, monkeypatch):
    """the 832 lattice without its top three layers is the 640 lattice (a handle without capacity: a sink needs none)"""
    cfg = pf.config(solver, "wall", 832)
    sim, o = h.make_handle(cfg, monkeypatch), h.make_oracle(pf.config(solver, "wall", 640))
    top = o.get(orc.F_POS)[:, 1].max()
    assert sim.remove_in_box([0, top + 0.5 * pf.D, 0], [1, 1, 1]) == 192 and sim.n_fluid == 640 and sim.capacity == 832
    h.same_bits(sim.download(nat.F_POS), o.get(orc.F_POS), "the cut lattice")
    pf.lockstep(sim, o, solver, 20, "%s remove" % solver)
    sim.close(); o.close()


# ---- 5: the thresholds of the live count -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", ["dfsph", "wcsph"])
def test_growing_past_65536(solver, monkeypatch):
    """64 512 particles (quad sweeps, nine-wave list build) grown by two lattice layers to 66 560 (plain sweeps, three-wave list build; dfsph: the
    wall cache comes into use) equal a fresh handle of the tall lattice"""
    tall = h.make_handle(pf.threshold_config(solver, 66560), monkeypatch)
    sim = h.make_handle(pf.threshold_config(solver, 64512, capacity=66560), monkeypatch)
    assert (sim.n_fluid, sim.capacity, tall.n_fluid, tall.capacity) == (64512, 66560, 66560, 66560)
    pos = tall.download(nat.F_POS)
    h.same_bits(sim.download(nat.F_POS), pos[:64512], "the short lattice")
    assert sim.add_particles(pos[64512:]) == 64512
    for s in range(3):
        a, b = sim.step(1), tall.step(1)
        if solver == "dfsph":
            h.same_stats(a, b, solver, "step %d: statistics" % (s + 1))
    for f in (nat.F_POS, nat.F_VEL, nat.F_RHO, nat.F_NBR_COUNT) + ((nat.F_WARM_K, nat.F_ALPHA) if solver == "dfsph" else (nat.F_PRESSURE,)):
        h.same_bits(sim.download(f), tall.download(f), "field %d" % f)
    sim.close(); tall.close()


# ---- 6: refusals and no-ops ------------------------------------------------------------------------------------------------------------------
def twins_agree(a, b, solver, steps=5):
    for s in range(steps):
        sa, sb = a.step(1), b.step(1)
        h.same_stats(sa, sb, solver, "step %d: statistics" % (s + 1))
    for f in (nat.F_POS, nat.F_VEL, nat.F_RHO, nat.F_NBR_COUNT):
        h.same_bits(a.download(f), b.download(f), "field %d" % f)


@pytest.mark.parametrize("solver", ["dfsph", "wcsph", "pbf"])
def test_refusals_and_noops(solver, monkeypatch):
    cfg = pf.config(solver, "wall", 640, capacity=704)
    a, b = h.make_handle(cfg, monkeypatch), h.make_handle(cfg, monkeypatch)
    a.step(3); b.step(3)
    ok = pf.layer_above(cfg, 640, 64)
    state = [a.download(f) for f in (nat.F_POS, nat.F_VEL, nat.F_RHO, nat.F_NBR_COUNT)]
    h.refused(nat.SPH_E_INVALID, lambda: a.add_particles(np.concatenate([ok, ok[:1] + np.float32([0, pf.D, 0])])))      # 65 > 704 - 640
    bad = ok[:3].copy(); bad[1, 2] = np.nan
    h.refused(nat.SPH_E_INVALID, lambda: a.add_particles(bad))
    bad = ok[:3].copy(); bad[2, 0] = np.inf
    h.refused(nat.SPH_E_INVALID, lambda: a.add_particles(bad))
    for axis, value in ((0, 1.0), (1, 0.0), (2, 1.5), (1, -0.25)):                                                      # on a face, beyond one
        bad = ok[:3].copy(); bad[0, axis] = value
        h.refused(nat.SPH_E_INVALID, lambda: a.add_particles(bad))
    h.refused(nat.SPH_E_INVALID, lambda: a.add_particles(ok[:2], np.float32([[0, 0, 0], [0, np.nan, 0]])))
    h.refused(nat.SPH_E_INVALID, lambda: a.remove_in_box([0, 0, 0], [1, 1, 1]))                                           # every particle
    assert a.add_particles(np.zeros((0, 3), np.float32)) == 640                                                         # n == 0
    assert a.remove_in_box([0.8, 0.8, 0.8], [0.9, 0.9, 0.9]) == 0 and a.remove_in_box([0.3, 0.3, 0.3], [0.2, 0.9, 0.9]) == 0   # nobody there; lo > hi
    assert a.n_fluid == 640 and a.capacity == 704
    for f, was in zip((nat.F_POS, nat.F_VEL, nat.F_RHO, nat.F_NBR_COUNT), state):      # not even what is valid changed: last step's rho and counts still read
        h.same_bits(a.download(f), was, "field %d after the refused calls" % f)
    twins_agree(a, b, solver)
    a.close(); b.close()


def test_capacity_zero_refuses_any_add(monkeypatch):
    cfg = pf.config("dfsph", "wall", 640)
    a, b = h.make_handle(cfg, monkeypatch), h.make_handle(cfg, monkeypatch)
    assert a.capacity == 640
    h.refused(nat.SPH_E_INVALID, lambda: a.add_particles(pf.layer_above(cfg, 640, 1)))
    twins_agree(a, b, "dfsph")
    a.close(); b.close()


def test_capacity_is_refused_where_it_is_out_of_scope(monkeypatch):
    cfg = pf.config("dfsph", "wall", 640, capacity=704)
    h.refused(nat.SPH_E_INVALID, lambda: h.make_handle(cfg, monkeypatch, slab_count=2, slab_rank=0))
    h.refused(nat.SPH_E_INVALID, lambda: h.make_handle(pf.config("dfsph", "wall", 640, capacity=639), monkeypatch))
    h.refused(nat.SPH_E_INVALID, lambda: h.make_handle(pf.config("dfsph", "wall", 640, capacity=1 << 28), monkeypatch))
    body = scenes.get("dfsph_rigid_small")
    rigid = mesh.rigid_from_config(body)
    body["fluid"]["capacity"] = 8192
    h.refused(nat.SPH_E_INVALID, lambda: nat.Simulation(nat.config_from_dict(body), rigid=rigid))
    # a handle with a body and no capacity: both calls are refused, and it steps on like its twin
    body = scenes.get("dfsph_rigid_small")
    a, b = (nat.Simulation(nat.config_from_dict(body), rigid=rigid) for _ in range(2))
    a.step(2); b.step(2)
    h.refused(nat.SPH_E_STATE, lambda: a.add_particles(np.float32([[1.5, 1.0, 0.7]])))
    h.refused(nat.SPH_E_STATE, lambda: a.remove_in_box([0, 0, 0], [0.3, 0.3, 0.3]))
    for s in range(5):
        sa, sb = a.step(1), b.step(1)
        h.same_stats(sa, sb, "dfsph", "step %d" % (s + 1))
        a.rigid_step(); b.rigid_step()
    for f in (nat.F_POS, nat.F_VEL):
        h.same_bits(a.download(f), b.download(f), "field %d" % f)
    a.close(); b.close()


# ---- 7: capacity alone is invisible ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", ["dfsph", "wcsph"])
def test_capacity_alone_is_invisible(solver, monkeypatch):
    a, b = h.make_handle(pf.config(solver, "wall", 640, capacity=4096), monkeypatch), h.make_handle(pf.config(solver, "wall", 640), monkeypatch)
    assert (a.n_fluid, a.capacity, b.capacity) == (640, 4096, 640)
    if solver == "wcsph":            # one call: captured step pairs are replayed
        a.step(20); b.step(20)
        assert a.scalar(nat.S_GRAPH_LAUNCHES) == b.scalar(nat.S_GRAPH_LAUNCHES) > 0
    else:
        for s in range(20):
            h.same_bits(np.float32(h.stats_tuple(a.step(1), solver)), np.float32(h.stats_tuple(b.step(1), solver)), "step %d" % (s + 1))
    for f in (nat.F_POS, nat.F_VEL, nat.F_RHO, nat.F_NBR_COUNT) + ((nat.F_WARM_K, nat.F_ALPHA) if solver == "dfsph" else (nat.F_PRESSURE, nat.F_ACC)):
        h.same_bits(a.download(f), b.download(f), "field %d" % f)
    a.close(); b.close()


def test_wcsph_graphs_follow_the_count(monkeypatch):
    """captured step pairs are dropped when the count changes: multi-step calls before and after an append equal the oracle"""
    o = h.make_oracle(pf.config("wcsph", "wall", 832))
    sim = h.make_handle(pf.config("wcsph", "wall", 640, capacity=832), monkeypatch)
    sim.step(4)                                         # pairs captured at 640 particles
    st = {"pos": np.concatenate([sim.download(nat.F_POS), o.get(orc.F_POS)[640:]]), "vel": np.concatenate([sim.download(nat.F_VEL), np.zeros((192, 3), np.float32)])}
    append_top(sim, o.get(orc.F_POS)[640:])
    h.give(o, st, "wcsph")
    sim.step(6); o.step_wcsph(6)
    assert sim.scalar(nat.S_GRAPH_LAUNCHES) >= 4
    pf.same_state(sim, o, "wcsph", "after the append")
    sim.close(); o.close()


# ---- 8: the shipped scenes ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,frames", [("filling_tank_dfsph", 700), ("channel_wcsph", 400)])
def test_shipped_scenes(name, frames, monkeypatch, tmp_path):
    for k in h.KNOBS:
        monkeypatch.delenv(k, raising=False)
    cfg = scenes.get(name)
    d = 2 * cfg["scene"]["particle_radius"]
    n0 = int(cfg["fluid"]["water_size"][0] / d * cfg["fluid"]["water_size"][1] / d * cfg["fluid"]["water_size"][2] / d)
    run.main(["--config", os.path.join(ROOT, "config", name + ".json"), "--steps", str(frames), "--ply-dir", str(tmp_path)])      # (SPH_E_OVERFLOW would raise)
    ps, (em,), sinks = run.LAST["ps"], run.LAST["emitters"], run.LAST["sinks"]
    sim = ps._sim
    due = em.layers_due(sim.time())
    print("%s: %d frames, t = %.6f, %d layers due, %d emitted, %d removed, %d particles" % (name, frames, sim.time(), due, em.emitted, sum(s.removed for s in sinks), sim.n_fluid))
    assert due >= 3 and not em.exhausted and em.layers_emitted == due and em.emitted == due * em.layer_size       # the emitter's own schedule
    assert sim.n_fluid == ps.particle_num == n0 + em.emitted - sum(s.removed for s in sinks) <= sim.capacity
    pos = ps.fluid_particles.pos.to_numpy()
    assert pos.shape == (sim.n_fluid, 3) and ps.rgba.to_numpy().shape == (sim.n_fluid, 4) and np.isfinite(pos).all()
    assert (pos >= np.float32(cfg["scene"]["box_min"])).all() and (pos <= np.float32(cfg["scene"]["box_max"])).all()
    if name == "filling_tank_dfsph":
        assert sim.last_stats.lost == 0
    last = sorted(p for p in os.listdir(tmp_path) if p.endswith(".ply"))[-1]
    header = open(os.path.join(tmp_path, last)).read(200)
    assert "element vertex" in header and n0 < int(header.split("element vertex ")[1].split()[0]) <= sim.n_fluid       # the PLY frames hold the live count
