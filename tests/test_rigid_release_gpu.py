"""GPU suite: `ps.active_rigid` as a runtime value -- sph_rigid_set_active / sph_rigid_init_data (main.py:100-106: let the fluid settle, then
release the body into it) and the way back, freezing a moving body.  Scenes and the hand-over: tests/rigid_release.py;
test_rigid_release_cpu.py proves on the oracle alone that the placements exercise what is asserted here and that pcisph's delta is the same
with the body in the grid or not at the two-way placement (so the pcisph cases are held to the oracle too).

The oracle has no setter for the flag.  An inactive body never moves, so "created inactive, K steps, release" must equal "a fresh oracle
created with `active: true` and given the fluid state of step K", bit for bit, at every step after the release.

  1. release at step 0: body data bit-equal to a handle (and an oracle) created active -- the factored init routine;
  2. release at step K, two-way, four solvers, against the transplanted oracle;
  3. release at step K, one-way: dfsph in rigid_modes' corner placement (pcisph's delta sees the body there: no pcisph case);
  4. freeze: the fluid goes on as if there were no body (oracle without a solid block), the body stays where it was; the second release needs
     no init_data.  A body's pose, velocity and omega cannot be uploaded through the ABI, so no second handle can be given the frozen
     body's state: the steps after the second release are checked to be finite and to move the body on, not against a twin;
  5. the same release under the relaxed arithmetic, GPU against GPU;
  6. refusals (no body, one-way under the relaxed arithmetic, a slab handle) and the guard: stepping a released body whose data are those of
     an unbinned body is SPH_E_STATE until sph_rigid_init_data has run;
  7. the mirror API: main.py:101-106 verbatim, and `run.py --release-rigid-at`.

The neighbour count is compared after every step for dfsph, the solver that computes it (as test_rigid_modes_gpu.py does: the oracle's count
belongs to the grid of the step).  For the other solvers both sides build the grid of the current positions before every step and the counts of
that grid are compared."""
import json

import numpy as np
import pytest

from cfd_taichi_amd import _native as nat
from oracle import oracle as orc
from harness import fluid_state, give, give_sim, oracle_step, same_nan_mask, same_values, stats_tuple
from rigid_release import AFTER, K, SOLVERS, body_oracle, rigid, scene
from test_rigid_modes_gpu import check_rigid

pytestmark = pytest.mark.gpu


def make_sim(cfg, **kw):
    return nat.Simulation(nat.config_from_dict(cfg, **kw), rigid=rigid(cfg))


def stepper(sim, solver):
    return {"dfsph": sim.step_dfsph, "wcsph": sim.step_wcsph, "pcisph": sim.step_pcisph, "iisph": sim.step_iisph}[solver]


def release(sim):
    """main.py:101-106"""
    sim.rigid_set_active(1)          # ps.active_rigid[None] = 1
    sim.build_neighbors()            # ps.reset_grid(); ps.update_grid()
    sim.rigid_init_data()            # ps.init_rigid_particles_data()


def body(sim):
    return (sim.rigid_scalars(), sim.download(nat.F_RIGID_POS, nat.SPECIES_RIGID), sim.download(nat.F_RIGID_VERT, nat.SPECIES_RIGID))


def same_body(a, b, what, nan_aware=False):
    for k in ("centroid", "omega", "vel", "inertia_inv", "mass"):
        (same_nan_mask if nan_aware else same_values)(np.float32(a[0][k]), np.float32(b[0][k]), "%s: %s" % (what, k))
    same_values(a[1], b[1], what + ": sample positions")
    same_values(a[2], b[2], what + ": mesh vertices")


def count_before_step(sim, o, solver, when):
    """dfsph compares the count of the step itself (after it); the others compare the count of the grid both sides build from the current positions"""
    if solver == "dfsph":
        return
    sim.build_neighbors()
    o.build_grid(); o.compute_nbr_count()
    same_values(sim.download(nat.F_NBR_COUNT), o.get(orc.F_NBR_COUNT), "neighbour count before " + when)


def lockstep(sim, o, solver, nsteps, active, one_way=False):
    """`nsteps` steps on both sides, everything the issue lists compared at every step; returns the body's vertical velocities"""
    g_step, vy = stepper(sim, solver), []
    for s in range(nsteps):
        when = "step +%d" % (s + 1)
        count_before_step(sim, o, solver, when)
        st = g_step(1)
        so = oracle_step(o, solver)
        assert np.float32(sim.scalar(nat.S_DELTA_TIME)) == np.float32(o.dt), (when, sim.scalar(nat.S_DELTA_TIME), o.dt)
        if solver != "wcsph":
            assert stats_tuple(st, solver) == stats_tuple(so, solver), (when, stats_tuple(st, solver), stats_tuple(so, solver))
        if solver == "dfsph":
            same_values(sim.download(nat.F_NBR_COUNT), o.get(orc.F_NBR_COUNT), "neighbour count of " + when)
        if active:
            if s % 10 == 0:
                fg, fo = sim.download(nat.F_RIGID_FORCE, nat.SPECIES_RIGID), o.get(orc.F_RIGID_FORCE)
                same_values(fg, fo, "force on the body, " + when)
                if one_way:
                    assert not fg.any(), "%s: a force on a body the fluid does not couple to" % when
            sim.rigid_step()
            o.rigid_step()
            vy.append(check_rigid(sim, o, "after rigid " + when, nan_aware=False)["vel"][1])
    same_values(sim.download(nat.F_POS), o.get(orc.F_POS), "fluid positions")
    same_values(sim.download(nat.F_VEL), o.get(orc.F_VEL), "fluid velocities")
    same_values(sim.download(nat.F_RHO), o.get(orc.F_RHO), "rho")
    return vy


# ---- 1 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", SOLVERS)
def test_release_at_step_0_equals_created_active(solver):
    cfg_off, cfg_on = scene(solver, False), scene(solver, True)
    a, b, o = make_sim(cfg_off), make_sim(cfg_on), body_oracle(cfg_on, solver)
    assert a.scalar(nat.S_RIGID_ACTIVE) == 0.0 and b.scalar(nat.S_RIGID_ACTIVE) == 1.0
    assert not a.download(nat.F_RIGID_VOL, nat.SPECIES_RIGID).any() and np.isnan(np.float32(a.rigid_scalars()["centroid"])).all()
    release(a)
    assert a.scalar(nat.S_RIGID_ACTIVE) == 1.0
    same_body(body(a), body(b), "released at step 0 vs created active")
    for f, name in ((nat.F_RIGID_VOL, "volumes"), (nat.F_RIGID_MASS, "masses")):
        same_values(a.download(f, nat.SPECIES_RIGID), b.download(f, nat.SPECIES_RIGID), "sample " + name)
        same_values(a.download(f, nat.SPECIES_RIGID), o.get({nat.F_RIGID_VOL: orc.F_RIGID_VOL, nat.F_RIGID_MASS: orc.F_RIGID_MASS}[f]), "sample %s vs the oracle" % name)
    assert a.download(nat.F_RIGID_VOL, nat.SPECIES_RIGID).all()
    check_rigid(a, o, "released at step 0 vs the oracle created active", nan_aware=False)
    if solver == "pcisph":      # the delta of construction stays (semantics 3); at this placement it is the active handle's and the oracle's too
        for s in (nat.S_PCISPH_DELTA, nat.S_PCISPH_BETA, nat.S_PCISPH_MAX_INDEX, nat.S_PCISPH_MAX_COUNT):
            assert np.float32(a.scalar(s)) == np.float32(b.scalar(s)), (s, a.scalar(s), b.scalar(s))
        assert np.float32(a.scalar(nat.S_PCISPH_DELTA)) == np.float32(o.pcisph_delta)
        assert (int(a.scalar(nat.S_PCISPH_MAX_INDEX)), int(a.scalar(nat.S_PCISPH_MAX_COUNT))) == o.pcisph_max_index
    # ... and the two go on alike: one coupled step and one body step
    for sim in (a, b):
        stepper(sim, solver)(1)
        sim.rigid_step()
    same_body(body(a), body(b), "one step after the release")
    same_values(a.download(nat.F_POS), b.download(nat.F_POS), "fluid positions one step after the release")
    a.close(); b.close(); o.close()


# ---- 2, 3 ------------------------------------------------------------------------------------------------------------------------------
def release_at_step_k(solver, fs_couple):
    sim = make_sim(scene(solver, False, fs_couple))
    g_step = stepper(sim, solver)
    for _ in range(K):
        g_step(1)
    at_k = body(sim)
    state = fluid_state(sim, solver)
    release(sim)
    o = give(body_oracle(scene(solver, True, fs_couple), solver), state, solver)
    same_values(at_k[1], o.get(orc.F_RIGID_POS), "the inactive body did not move")
    check_rigid(sim, o, "at the release", nan_aware=False)
    vy = lockstep(sim, o, solver, AFTER, active=True, one_way=not fs_couple)
    assert vy[0] < 0, "the released body did not fall"
    sim.close(); o.close()


@pytest.mark.parametrize("solver", SOLVERS)
def test_release_at_step_k_two_way(solver):
    release_at_step_k(solver, True)


def test_release_at_step_k_one_way():
    release_at_step_k("dfsph", False)


# ---- 4 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", SOLVERS)
def test_freeze_then_release_again(solver):
    sim = make_sim(scene(solver, True))
    g_step = stepper(sim, solver)
    for _ in range(10):
        g_step(1)
        sim.rigid_step()
    at_10 = body(sim)
    assert at_10[0]["vel"][1] < 0
    state = fluid_state(sim, solver)
    sim.rigid_set_active(0)
    assert sim.scalar(nat.S_RIGID_ACTIVE) == 0.0
    o = give(body_oracle(scene(solver, None), solver), state, solver)
    o.build_grid(); o.compute_nbr_count()
    same_values(sim.download(nat.F_NBR_COUNT), o.get(orc.F_NBR_COUNT), "neighbour count right after the freeze: the fluid-only count")
    lockstep(sim, o, solver, 20, active=False)
    same_body(body(sim), at_10, "the frozen body after 20 fluid steps")
    if solver != "dfsph":
        count_before_step(sim, o, solver, "the second release")
    # release again: the data are those of a binned body, no init_data, no guard
    sim.rigid_set_active(1)
    assert sim.scalar(nat.S_RIGID_ACTIVE) == 1.0
    for _ in range(5):
        g_step(1)
        sim.rigid_step()
    after = body(sim)
    for k in ("centroid", "omega", "vel", "inertia_inv", "mass"):
        assert np.isfinite(np.float32(after[0][k])).all(), k
    assert np.isfinite(sim.download(nat.F_POS)).all() and np.isfinite(after[1]).all()
    assert after[0]["centroid"][1] < at_10[0]["centroid"][1] and after[0]["vel"][1] < at_10[0]["vel"][1], "the body did not go on falling"
    assert np.float32(after[0]["mass"]) == np.float32(at_10[0]["mass"])             # rigid_solver.mass is taken once (run_once_flag)
    sim.close(); o.close()


# ---- 5 ---------------------------------------------------------------------------------------------------------------------------------
def test_release_under_the_relaxed_arithmetic(monkeypatch):
    """dfsph_rigid_small's geometry on the Morton curve: the smallest dfsph scene on which S_ARITH_RELAXED reads 1 next to a coupled body
    (tests/test_relaxed_gpu.py::test_relaxed_next_to_a_rigid_body).  No oracle: the relaxed sweeps are held to it by tolerance elsewhere; a
    release must be the same bits as the handle created active."""
    monkeypatch.setenv("SPH_CELL_ORDER", "morton")
    a = make_sim(scene("dfsph", False), arith=nat.ARITH_RELAXED)
    for _ in range(5):
        a.step_dfsph(1)
    assert a.scalar(nat.S_ARITH_RELAXED) == 1.0
    state = fluid_state(a, "dfsph")
    release(a)
    b = give_sim(make_sim(scene("dfsph", True), arith=nat.ARITH_RELAXED), state, "dfsph")
    for s in range(5):
        sa, sb = a.step_dfsph(1), b.step_dfsph(1)
        assert a.scalar(nat.S_ARITH_RELAXED) == 1.0 and b.scalar(nat.S_ARITH_RELAXED) == 1.0
        assert stats_tuple(sa, "dfsph") == stats_tuple(sb, "dfsph"), (s, stats_tuple(sa, "dfsph"), stats_tuple(sb, "dfsph"))
        same_values(a.download(nat.F_RIGID_FORCE, nat.SPECIES_RIGID), b.download(nat.F_RIGID_FORCE, nat.SPECIES_RIGID), "force on the body, step +%d" % (s + 1))
        a.rigid_step(); b.rigid_step()
        same_body(body(a), body(b), "step +%d" % (s + 1))
    for f, name in ((nat.F_POS, "positions"), (nat.F_VEL, "velocities"), (nat.F_RHO, "rho"), (nat.F_WARM_K, "warm_start_k")):
        same_values(a.download(f), b.download(f), "fluid " + name)
    assert b.rigid_scalars()["vel"][1] < 0
    a.close(); b.close()


# ---- 6 ---------------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    sim = make_sim(scene("dfsph", None))
    for call in (lambda: sim.rigid_set_active(1), sim.rigid_init_data):
        with pytest.raises(nat.SphError, match="no rigid body") as e:
            call()
        assert e.value.code == nat.SPH_E_STATE
    assert sim.scalar(nat.S_RIGID_ACTIVE) == 0.0
    sim.close()
    # a one-way body under the relaxed arithmetic: refused as sph_create_rigid refuses it, and the handle stays as it was
    sim = make_sim(scene("dfsph", False, fs_couple=False), arith=nat.ARITH_RELAXED)
    with pytest.raises(nat.SphError, match="exact arithmetic") as e:
        sim.rigid_set_active(1)
    assert e.value.code == nat.SPH_E_STATE and sim.scalar(nat.S_RIGID_ACTIVE) == 0.0
    sim.rigid_set_active(0)
    sim.step_dfsph(1)
    sim.close()
    # slab handles (the body replicated on every rank) are out of scope: rank 0 of 2, planning only -- no transport is attached, no step taken
    cfg = scene("dfsph", True)
    sim = make_sim(cfg, slab_rank=0, slab_count=2, slab_ghost_layers=2)
    for call in (lambda: sim.rigid_set_active(0), sim.rigid_init_data):
        with pytest.raises(nat.SphError, match="slab handles") as e:
            call()
        assert e.value.code == nat.SPH_E_STATE
    assert sim.scalar(nat.S_RIGID_ACTIVE) == 1.0
    sim.close()


@pytest.mark.parametrize("solver", SOLVERS)
def test_stepping_a_released_body_needs_init_data(solver):
    sim = make_sim(scene(solver, False))
    g_step = stepper(sim, solver)
    g_step(1)
    sim.rigid_set_active(1)
    before = fluid_state(sim, solver)
    for call in (lambda: g_step(1), sim.rigid_step):
        with pytest.raises(nat.SphError, match="call sph_rigid_init_data after releasing the body") as e:
            call()
        assert e.value.code == nat.SPH_E_STATE
    same_values(sim.download(nat.F_POS), before["pos"], "a refused step moved the fluid")
    sim.rigid_init_data()
    g_step(1)
    sim.rigid_step()
    sc = sim.rigid_scalars()
    assert all(np.isfinite(np.float32(sc[k])).all() for k in sc) and sc["vel"][1] < 0 and np.isfinite(sim.download(nat.F_POS)).all()
    sim.close()


# ---- 7 ---------------------------------------------------------------------------------------------------------------------------------
def test_mirror_api_runs_the_reference_sequence():
    from cfd_taichi_amd import ParticleSystem, dfsph_solver, rigid_solver
    cfg = scene("dfsph", False)
    ps = ParticleSystem(cfg)
    solver = dfsph_solver(ps, cfg, verbose=False)
    rs = rigid_solver(ps, cfg)
    assert ps.exist_rigid[None] == 1 and ps.active_rigid[None] == 0
    for _ in range(3):
        solver.step()
    resting = ps.rigid_vertices.to_numpy()
    # main.py:101-106
    ps.active_rigid[None] = 1
    ps.reset_grid()
    ps.update_grid()
    ps.init_rigid_particles_data()
    assert ps.active_rigid[None] == 1
    assert ps.rigid_particles.volume.to_numpy().all() and np.isfinite(ps.rigid_centriod[None]).all()
    solver.step()
    rs.step()
    assert ps._sim.rigid_scalars()["vel"][1] < 0 and rs.mass[None] > 0
    assert (ps.rigid_vertices.to_numpy()[:, 1] < resting[:, 1]).all()
    ps.active_rigid[None] = 0
    assert ps.active_rigid[None] == 0


def test_headless_runner_releases_the_body(tmp_path):
    from cfd_taichi_amd import run
    cfg = scene("dfsph", False)
    cfg["scene"]["output_fps"] = 2000          # a frame (one step of 1e-3) is two output intervals: every frame writes its OBJ
    path = tmp_path / "scene.json"
    path.write_text(json.dumps(cfg))
    frames, t, plys = run.main(["--config", str(path), "--steps", "6", "--release-rigid-at", "3", "--ply-dir", str(tmp_path / "out")])
    assert frames == 6 and plys == 6

    def vertices(k):
        lines = (tmp_path / "out" / ("obj_%06d.obj" % k)).read_text().splitlines()
        return np.array([[float(x) for x in l.split()[1:]] for l in lines if l.startswith("v ")])

    v = [vertices(k) for k in range(6)]
    assert v[0].shape == (8, 3)
    assert np.array_equal(v[0], v[1]) and np.array_equal(v[1], v[2]), "the body moved before it was released"
    for k in (3, 4, 5):
        assert (v[k][:, 1] < v[k - 1][:, 1]).all(), "OBJ frame %d: the released body does not fall" % k
