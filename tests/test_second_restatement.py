"""CPU suite: the oracle against a SECOND, independently written restatement of the reference (tests/second_restatement.py: numpy f32,
brute-force O(N^2) neighbour search, written from the reference's text with no code shared with oracle/ or the library).

What it is for (VERDICT r5 missing #5): the oracle and the HIP kernels come from one reading of the reference by one hand, and the GPU suite
proves that they agree with each other.  A transcription error common to both would pass every one of those tests.  Two restatements that
differ in algorithm (27-cell walk over per-cell lists there, all-pairs test + sort by (cell offset, index) here) and in language, and still
agree bit for bit over ten steps of a wall-bounded scene -- state, densities, alpha, iteration counts, residuals, dt -- make such an error
much less likely.  It does NOT pin the oracle to the reference: both restatements rest on the same assumptions about Taichi's arithmetic
(SURVEY.md Appendix A), and `parity` stays "unpinned"."""
import numpy as np
import pytest

import coupled_scenes as cs
import restatement_compare as rc
from cfd_taichi_amd import scenes
from oracle import oracle as orc
from second_restatement import Scene, Solver


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same(a, b, what):
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    assert a.shape == b.shape, what
    if not np.array_equal(bits(a), bits(b)):
        bad = np.argwhere(bits(a) != bits(b))
        i = tuple(bad[0])
        raise AssertionError("%s: %d of %d values differ, first at %s: %r (second restatement) vs %r (oracle)" % (what, len(bad), a.size, i, a[i], b[i]))


@pytest.mark.parametrize("scene", ["wcsph_tiny_wall", "dfsph_tiny_wall", "wcsph_tiny_clamp", "dfsph_tiny_clamp"])
def test_scene_construction(scene):
    """ParticleSystem.__init__: counts, grid, lattice, wall particles, wall volumes (ParticleSystem.py:78-195, 309-320)"""
    cfg = scenes.get(scene)
    o = orc.Oracle(cfg)
    sc = Scene(cfg)
    assert (sc.N, sc.Nb, tuple(sc.grid), sc.C) == (o.N, o.Nb, tuple(o.grid), o.C)
    same(sc.pos, o.get(orc.F_POS), "lattice")
    same(sc.wall_pos, o.get(orc.F_WALL_POS), "wall positions")
    if cfg["solver"]["boundary_handle"]:
        same(sc.wall_vol, o.get(orc.F_WALL_VOL), "wall volumes")
    o.close()


@pytest.mark.parametrize("scene,steps", [("wcsph_tiny_wall", 10), ("wcsph_tiny_clamp", 10)])
def test_wcsph_ten_steps(scene, steps):
    """wcsph_solver.step (wcsph_solver.py:25-129, solver_base.py:41-72, 170-217), every step compared"""
    cfg = scenes.get(scene)
    o = orc.Oracle(cfg)
    s = Solver(cfg)
    assert s.N <= 700
    with np.errstate(all="ignore"):
        for k in range(steps):
            s.step()
            o.step_wcsph(1)
            same(s.rho, o.get(orc.F_RHO), "rho, step %d" % (k + 1))
            same(s.pressure, o.get(orc.F_PRESSURE), "pressure, step %d" % (k + 1))
            same(s.viscosity, o.get(orc.F_VISCOSITY), "viscosity, step %d" % (k + 1))
            same(s.tension, o.get(orc.F_TENSION), "tension, step %d" % (k + 1))
            same(s.acc, o.get(orc.F_ACC), "acc, step %d" % (k + 1))
            same(s.vel, o.get(orc.F_VEL), "vel, step %d" % (k + 1))
            same(s.pos, o.get(orc.F_POS), "pos, step %d" % (k + 1))
    o.close()


@pytest.mark.parametrize("scene,steps", [("dfsph_tiny_wall", 10), ("dfsph_tiny_clamp", 10)])
def test_dfsph_ten_steps(scene, steps):
    """dfsph_solver.step (dfsph_solver.py:32-445): state, per-particle solver fields, iteration counts, residuals and dt, every step"""
    cfg = scenes.get(scene)
    o = orc.Oracle(cfg)
    s = Solver(cfg)
    assert s.N <= 700
    iterated = 0
    with np.errstate(all="ignore"):
        for k in range(steps):
            s.step()
            o.step_dfsph(1)
            st = o.last_stats
            assert (s.n_div, s.n_dens) == (st.n_div, st.n_dens), "iteration counts, step %d" % (k + 1)
            assert np.float32(s.div_first) == np.float32(st.div_first_err) and np.float32(s.div_err) == np.float32(st.div_err), "divergence residuals, step %d" % (k + 1)
            assert np.float32(s.dens_err) == np.float32(st.dens_err), "density residual, step %d" % (k + 1)
            assert np.float32(s.dt) == np.float32(st.dt), "dt, step %d" % (k + 1)
            same(s.rho, o.get(orc.F_RHO), "rho, step %d" % (k + 1))
            same(s.alpha, o.get(orc.F_ALPHA), "alpha, step %d" % (k + 1))
            same(s.rho_derivative, o.get(orc.F_RHO_DER), "rho_derivative, step %d" % (k + 1))
            same(s.warm, o.get(orc.F_WARM_K), "warm_start_k, step %d" % (k + 1))
            same(s.rho_adv, o.get(orc.F_RHO_ADV), "rho_adv, step %d" % (k + 1))
            same(s.vel_adv, o.get(orc.F_VEL_ADV), "vel_adv, step %d" % (k + 1))
            same(s.vel, o.get(orc.F_VEL), "vel, step %d" % (k + 1))
            same(s.pos, o.get(orc.F_POS), "pos, step %d" % (k + 1))
            iterated += (s.n_div > 1) + (s.n_dens > 2)
    assert iterated > 0, "neither solver loop ever ran past its minimum: the loops were not exercised"
    o.close()


@pytest.mark.parametrize("scene,steps", [("wcsph_tiny_wall", 5), ("dfsph_tiny_wall", 5)])
def test_jittered_state_five_steps(scene, steps):
    """The same from a ragged state: every particle displaced by up to 0.3 d and given a random velocity of up to 0.5 m/s (seeded), so that
    cells are unevenly filled, pairs approach each other (the viscosity's `shear < 0` branch) and the walls are pressed from the first step"""
    cfg = scenes.get(scene)
    o = orc.Oracle(cfg)
    s = Solver(cfg)
    rng = np.random.default_rng(20261005)
    d = np.float32(2 * cfg["scene"]["particle_radius"])
    pos = (s.pos + rng.uniform(-0.3, 0.3, s.pos.shape).astype(np.float32) * d).astype(np.float32)
    vel = rng.uniform(-0.5, 0.5, s.vel.shape).astype(np.float32)
    s.pos, s.vel = pos.copy(), vel.copy()
    o.set(orc.F_POS, pos)
    o.set(orc.F_VEL, vel)
    with np.errstate(all="ignore"):
        for k in range(steps):
            s.step()
            if cfg["solver"]["name"] == "wcsph":
                o.step_wcsph(1)
            else:
                o.step_dfsph(1)
                assert (s.n_div, s.n_dens) == (o.last_stats.n_div, o.last_stats.n_dens), "iteration counts, step %d" % (k + 1)
                same(s.alpha, o.get(orc.F_ALPHA), "alpha, step %d" % (k + 1))
            same(s.rho, o.get(orc.F_RHO), "rho, step %d" % (k + 1))
            same(s.vel, o.get(orc.F_VEL), "vel, step %d" % (k + 1))
            same(s.pos, o.get(orc.F_POS), "pos, step %d" % (k + 1))
    o.close()


# ---- PCISPH, IISPH and the rigid body: the oracle against the second restatement (tests/coupled_scenes.py has the scenes and the loop) ----


def _past_minimum(solver, iters):
    if solver == "dfsph":
        return any(nd > 1 or ns > 2 for nd, ns in iters)
    return any(n > 1 for n in iters)


KINDS = ["wall", "clamp_rest", "clamp", "jitter"]


def uncoupled_case(solver, kind):
    """(config, steps, state): dfsph_tiny_wall_<solver> for 10 steps; its clamp twin from rest for 10 steps (free fall: the block starts
    0.075 above the clamp plane); the clamp twin thrown at the floor and the x = 0 plane (cs.clamp_thrown) for cs.CLAMP_THROWN_STEPS; the
    seeded ragged state of the wall scene for 5 steps"""
    if kind in ("clamp", "clamp_rest"):
        cfg = cs.clamp_twin(solver)
        return (cfg, cs.CLAMP_THROWN_STEPS, cs.clamp_thrown(cfg)) if kind == "clamp" else (cfg, 10, None)
    cfg = scenes.get("dfsph_tiny_wall_" + solver)
    return (cfg, 5, cs.jitter(cfg)) if kind == "jitter" else (cfg, 10, None)


def check_uncoupled(solver, kind, ev):
    """each case exercised what it claims"""
    print("%s %s: pressure iterations per step %s; particle coordinates on a clamp plane %d; press_force of -0: %d" % (
        solver, kind, ev["iters"], ev["on_plane"], ev["minus_zero"]))
    if kind == "clamp_rest":    # what it claims is free fall without walls: nothing touches a plane, no pressure builds up
        assert ev["on_plane"] == 0 and all(n == 1 for n in ev["iters"])
    else:
        assert _past_minimum(solver, ev["iters"]), "the pressure loop never ran past its minimum"
    if kind == "clamp":
        assert ev["on_plane"] > 0, "no particle ever sat on a clamp plane: the clamp branch did nothing"
    if solver == "pcisph" and kind in ("clamp", "clamp_rest"):
        assert ev["minus_zero"] > 0, "`- press_force` of an empty sum (pcisph_solver.py:119) never occurred"


@pytest.mark.parametrize("solver", ["pcisph", "iisph"])
@pytest.mark.parametrize("kind", KINDS)
def test_pcisph_iisph_steps(solver, kind):
    """pcisph_solver.py:28-240 / iisph_solver.py:35-349 on the cases of uncoupled_case: pos, vel, rho, pressure, predicted position,
    pressure force, d_ii, a_ii, sum d_ij, the PCISPH delta and fullest neighbourhood, iteration counts and residuals, every step"""
    cfg, steps, state = uncoupled_case(solver, kind)
    check_uncoupled(solver, kind, rc.compare_run(cfg, steps, [rc.OracleSide], state=state))


@pytest.mark.parametrize("solver", ["dfsph", "pcisph", "iisph", "wcsph"])
@pytest.mark.parametrize("tilted", [False, True], ids=["upright", "tilted"])
def test_coupled_scene(solver, tilted):
    """Two-way coupling: the rigid samples as a third species in every sum of the solver, the force each one deposits, and
    rigid_solver.step after every fluid step (cs.STEPS steps; the upright body's first wall impulse lies inside the window)."""
    cfg = cs.coupled(solver, tilted=tilted)
    rg = cs.rigid(cfg)
    ev = rc.compare_run(cfg, cs.TILTED_STEPS[solver] if tilted else cs.STEPS[solver], [rc.OracleSide], rg=rg)
    b = ev["solver"].body
    print("%s %s: iterations %s; impulse steps %s; largest per-sample force %.4g; vy %s" % (solver, "tilted" if tilted else "upright", ev["iters"],
                                                                                           ev["hit_steps"], max(ev["force"]), ev["vy"][-3:]))
    assert b.Nr == 168 and b.pos[:, 1].min() >= np.float32(0.05), "a sample starts below box_min + diameter"
    assert max(ev["force"]) > 0, "the fluid never pushed the body"
    if tilted and solver == "wcsph":    # a particle that slipped through a wall pushes the body from outside the grid (listed under a wrapped index)
        assert ev["outside_deposits"] > 0, "no fluid particle outside the grid deposited a force"
    if solver != "wcsph":
        assert _past_minimum(solver, ev["iters"]), "the pressure loop never ran past its minimum"
    if not tilted:
        assert ev["hit_steps"], "no step took the wall-impulse branch (collision_point_cnt > 0)"


@pytest.mark.parametrize("solver", ["dfsph", "pcisph"])
def test_one_way_body(solver):
    """fs_couple false, active body: binned (get_neighbour_count's rigid branch, quirk included), ignored by the sums, falling and bouncing"""
    cfg = cs.coupled(solver, fs_couple=False)
    ev = rc.compare_run(cfg, cs.ONEWAY_STEPS, [rc.OracleSide], rg=cs.rigid(cfg))
    print("%s one-way: iterations %s; impulse steps %s; quirk count differs for %d particle-steps" % (solver, ev["iters"], ev["hit_steps"], ev["quirk"]))
    assert max(ev["force"]) == 0, "a force on a body the fluid does not couple to"
    assert ev["hit_steps"], "the body never reached the floor impulse"
    assert ev["quirk"] > 0, "the quirk count never differed from the plain fluid count"   # (ncount itself is compared every step, both solvers)


def test_inactive_body_equals_no_body():
    """active false: never binned, never stepped -- the fluid of the run with the body equals the run without a solid block, on both readings"""
    with_body, without = cs.coupled("pcisph", active=False), cs.coupled("pcisph", solid=False)
    a = rc.compare_run(with_body, 5, [rc.OracleSide], rg=cs.rigid(with_body))["solver"]
    b = rc.compare_run(without, 5, [rc.OracleSide])["solver"]
    same(a.pos, b.pos, "positions with an inactive body and with none")
    same(a.vel, b.vel, "velocities with an inactive body and with none")
    assert (a.delta, a.max_index) == (b.delta, b.max_index)
    assert not a.body.vol.any() and not a.body.force.any()
