"""CPU suite: the oracle against a SECOND, independently written restatement of the reference (tests/second_restatement.py: numpy f32,
brute-force O(N^2) neighbour search, written from the reference's text with no code shared with oracle/ or the library).

What it is for (VERDICT r5 missing #5): the oracle and the HIP kernels come from one reading of the reference by one hand, and the GPU suite
proves that they agree with each other.  A transcription error common to both would pass every one of those tests.  Two restatements that
differ in algorithm (27-cell walk over per-cell lists there, all-pairs test + sort by (cell offset, index) here) and in language, and still
agree bit for bit over ten steps of a wall-bounded scene -- state, densities, alpha, iteration counts, residuals, dt -- make such an error
much less likely.  It does NOT pin the oracle to the reference: both restatements rest on the same assumptions about Taichi's arithmetic
(SURVEY.md Appendix A), and `parity` stays "unpinned".

PBF (tests/second_restatement_pbf.py, the last section below) is held the same way: rho, pbf_lambda, delta_pos, pos and vel after every step of
four cases, compute_all_rho alone, and two f64 checks of the restatement's own poly6 / spiky kernel functions that rest on no reading at all.
Disagreements found between the PBF restatement and the oracle: none, on any case, field or step."""
import math

import numpy as np
import pytest

import coupled_scenes as cs
import restatement_compare as rc
from harness import same_bits, squeezed
from cfd_taichi_amd import scenes
from oracle import oracle as orc
from second_restatement import Scene, Solver


@pytest.mark.parametrize("scene", ["wcsph_tiny_wall", "dfsph_tiny_wall", "wcsph_tiny_clamp", "dfsph_tiny_clamp"])
def test_scene_construction(scene):
    """ParticleSystem.__init__: counts, grid, lattice, wall particles, wall volumes (ParticleSystem.py:78-195, 309-320)"""
    cfg = scenes.get(scene)
    o = orc.Oracle(cfg)
    sc = Scene(cfg)
    assert (sc.N, sc.Nb, tuple(sc.grid), sc.C) == (o.N, o.Nb, tuple(o.grid), o.C)
    same_bits(sc.pos, o.get(orc.F_POS), "lattice")
    same_bits(sc.wall_pos, o.get(orc.F_WALL_POS), "wall positions")
    if cfg["solver"]["boundary_handle"]:
        same_bits(sc.wall_vol, o.get(orc.F_WALL_VOL), "wall volumes")
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
            same_bits(s.rho, o.get(orc.F_RHO), "rho, step %d" % (k + 1))
            same_bits(s.pressure, o.get(orc.F_PRESSURE), "pressure, step %d" % (k + 1))
            same_bits(s.viscosity, o.get(orc.F_VISCOSITY), "viscosity, step %d" % (k + 1))
            same_bits(s.tension, o.get(orc.F_TENSION), "tension, step %d" % (k + 1))
            same_bits(s.acc, o.get(orc.F_ACC), "acc, step %d" % (k + 1))
            same_bits(s.vel, o.get(orc.F_VEL), "vel, step %d" % (k + 1))
            same_bits(s.pos, o.get(orc.F_POS), "pos, step %d" % (k + 1))
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
            same_bits(s.rho, o.get(orc.F_RHO), "rho, step %d" % (k + 1))
            same_bits(s.alpha, o.get(orc.F_ALPHA), "alpha, step %d" % (k + 1))
            same_bits(s.rho_derivative, o.get(orc.F_RHO_DER), "rho_derivative, step %d" % (k + 1))
            same_bits(s.warm, o.get(orc.F_WARM_K), "warm_start_k, step %d" % (k + 1))
            same_bits(s.rho_adv, o.get(orc.F_RHO_ADV), "rho_adv, step %d" % (k + 1))
            same_bits(s.vel_adv, o.get(orc.F_VEL_ADV), "vel_adv, step %d" % (k + 1))
            same_bits(s.vel, o.get(orc.F_VEL), "vel, step %d" % (k + 1))
            same_bits(s.pos, o.get(orc.F_POS), "pos, step %d" % (k + 1))
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
                same_bits(s.alpha, o.get(orc.F_ALPHA), "alpha, step %d" % (k + 1))
            same_bits(s.rho, o.get(orc.F_RHO), "rho, step %d" % (k + 1))
            same_bits(s.vel, o.get(orc.F_VEL), "vel, step %d" % (k + 1))
            same_bits(s.pos, o.get(orc.F_POS), "pos, step %d" % (k + 1))
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
    same_bits(a.pos, b.pos, "positions with an inactive body and with none")
    same_bits(a.vel, b.vel, "velocities with an inactive body and with none")
    assert (a.delta, a.max_index) == (b.delta, b.max_index)
    assert not a.body.vol.any() and not a.body.force.any()


# ---- PBF: the oracle against tests/second_restatement_pbf.py (its numbered conventions say how pbf_solver.py is read) ----------------------

PBF_KINDS = ["wall_squeezed", "clamp_squeezed", "clamp_thrown", "wall_jitter"]
PBF_THROWN_SHIFT = (-0.05, -0.05, 0.0)


def pbf_squeezed(cfg, factor=0.9):
    """test_pbf_gpu.squeeze as a state: the rest lattice scaled about its minimum corner, at rest -- lambda and delta_pos act from step 1"""
    pos = Scene(cfg).pos
    return squeezed(pos, factor), np.zeros_like(pos)


def pbf_case(kind):
    """(config, steps, state) on pbf_tiny_wall / pbf_tiny_clamp (640 fluid, 2 402 wall particles, dt 2.5e-4).
    clamp_thrown: cs.clamp_thrown (the ragged state plus (-4, -4, 0) m/s) covers 1e-3 per step, and the block starts 0.06 above the planes
    box_min + radius: 60 steps away.  The choice made here is to MOVE THE START, by PBF_THROWN_SHIFT = 0.05 towards the x = 0 and y = 0
    planes (the lowest coordinate is then 0.035, 0.01 above the planes), and keep the 4 m/s: the planes are reached from step 10 of 30."""
    if kind == "clamp_thrown":
        cfg = scenes.get("pbf_tiny_clamp")
        pos, vel = cs.clamp_thrown(cfg)
        return cfg, 30, ((pos + np.array(PBF_THROWN_SHIFT, dtype=np.float32)).astype(np.float32), vel)
    cfg = scenes.get("pbf_tiny_clamp" if kind == "clamp_squeezed" else "pbf_tiny_wall")
    return (cfg, 5, cs.jitter(cfg)) if kind == "wall_jitter" else (cfg, 10, pbf_squeezed(cfg))


def check_pbf(kind, ev):
    """each case exercised what it claims"""
    print("pbf %s: particles with lambda != 0 per step %s; particle coordinates on a clamp plane %d; max |v| of phase 2 per step %s; particles "
          "whose cell changed inside a step %s" % (kind, ev["lambda_active"], ev["on_plane"], ["%.3g" % v for v in ev["xsph_max"]], ev["cell_changes"]))
    if kind.endswith("squeezed"):
        assert ev["lambda_active"][0] > 0, "the density constraint is not active at step 1: lambda / delta_pos not exercised"
    if kind == "clamp_thrown":
        assert ev["on_plane"] > 0, "no particle ever sat on a clamp plane: the clamp branch did nothing"
    if kind == "wall_jitter":
        assert max(ev["xsph_max"]) > 0, "the viscosity sum of update_all_pos was zero throughout"
    # "old cells, new distances" (convention 3) is observable only where a particle leaves its cell inside a step: every case has some
    assert sum(ev["cell_changes"]) > 0, "no particle changed its cell inside a step"


@pytest.mark.parametrize("kind", PBF_KINDS)
def test_pbf_steps(kind):
    """pbf_solver.step (pbf_solver.py:26-187): rho, pbf_lambda, delta_pos, pos, vel on raw bits after every step"""
    cfg, steps, state = pbf_case(kind)
    check_pbf(kind, rc.compare_run(cfg, steps, [rc.OracleSide], state=state))


def test_pbf_compute_all_rho_alone():
    """solver_base.compute_all_rho with PBF's poly6 callbacks (solver_base.py:41-51, pbf_solver.py:166-174) after 3 squeezed steps: rho equal,
    pbf_lambda, delta_pos, pos and vel untouched on both sides"""
    cfg = scenes.get("pbf_tiny_wall")
    ev = rc.compare_run(cfg, 3, [rc.OracleSide], state=pbf_squeezed(cfg), density_after=True)
    assert ev["lambda_active"][-1] > 0, "pbf_lambda is all zero: 'untouched' would prove nothing"


# ---- two checks of the PBF restatement's kernel functions that depend on no reading of pbf_solver.py (f64) ---------------------------------


def test_poly_kernel_integrates_to_one():
    """the poly6 kernel is normalised: 4 pi int_0^h W(r) r^2 dr = 1 (composite Simpson, 2000 intervals: the integrand is a polynomial of degree
    8, the quadrature error ~1e-13; the f32 constants 315 and 64 pi inside poly_kernel are good to 6e-8)"""
    from second_restatement_pbf import poly_kernel
    h = np.float64(0.1)
    n = 2000
    r = np.linspace(0.0, float(h), n + 1)
    w = poly_kernel(r, h)
    assert w.dtype == np.float64
    f = 4 * math.pi * w * r * r
    simpson = np.ones(n + 1)
    simpson[1:-1:2], simpson[2:-1:2] = 4, 2
    total = float((f * simpson).sum() * (float(h) / n) / 3)
    print("integral of poly_kernel over the ball: 1 + %.3e" % (total - 1))
    assert abs(total - 1) <= 1e-6
    assert poly_kernel(np.float64(0.1000001), h) == 0 and poly_kernel(np.float32(0.2), np.float32(0.1)) == 0


def test_spiky_kernel_derivative_is_the_gradient_of_the_spiky_kernel():
    """d/dr of 15 (1 - q)^3 / (pi h^3) (solver_base.py:105-111) by central differences, at ten radii inside (0, h), along three directions;
    exactly zero at r = 0 and for q > 1"""
    from second_restatement_pbf import spiky_kernel_derivative
    h = np.float64(0.1)

    def spiky(r):
        return 15 * (1 - r / h) ** 3 / (math.pi * h ** 3)

    eps = 1e-6 * float(h)        # truncation eps^2 / 6 times the third derivative: relative 1e-9 or less at these radii; rounding ~1e-16 / 1e-6
    worst = 0.0
    for direction in ([1.0, 0.0, 0.0], [0.0, -1.0, 0.0], [0.6, 0.0, 0.8]):
        n = np.array(direction)
        for r in np.linspace(0.05, 0.95, 10) * float(h):
            g = spiky_kernel_derivative((n * r)[None, :], h)[0]
            assert g.dtype == np.float64
            fd = (spiky(r + eps) - spiky(r - eps)) / (2 * eps)
            rel = float(np.abs(g - fd * n).max() / abs(fd))
            worst = max(worst, rel)
            assert rel <= 1e-6, (direction, r, g, fd)
    print("spiky_kernel_derivative against the central difference: worst relative error %.3e" % worst)
    zero = spiky_kernel_derivative(np.array([[0.0, 0.0, 0.0], [0.1000001, 0.0, 0.0], [0.08, 0.08, 0.0]]), h)
    assert np.array_equal(zero, np.zeros((3, 3)))
    zero32 = spiky_kernel_derivative(np.array([[0.0, 0.0, 0.0], [0.0, 0.11, 0.0]], dtype=np.float32), np.float32(0.1))
    assert zero32.dtype == np.float32 and np.array_equal(zero32, np.zeros((2, 3), dtype=np.float32))


def pbf_rho_f64(cfg, pos, wall_pos, wall_vol):
    """rho of compute_all_rho with the poly6 callbacks as a plain f64 all-pairs sum (no cells, no order): (rho, K, sum |t_j|) per particle,
    K = the number of nonzero terms of the particle's two sums, t_j = the f64 terms m W(r_ij) and rho_0 V_b W(r_ib)"""
    r = cfg["scene"]["particle_radius"]
    h, m = 4 * r, 1000 * r ** 3 * 8
    k = 315 / (64 * math.pi * h ** 3)
    p, w = np.asarray(pos, dtype=np.float64), np.asarray(wall_pos, dtype=np.float64)

    def kernel(a, b):
        q = np.sqrt(((a[:, None, :] - b[None, :, :]) ** 2).sum(-1)) / h
        return np.where(q <= 1, k * (1 - q * q) ** 3, 0.0)

    tf = m * kernel(p, p)
    np.fill_diagonal(tf, 0.0)
    tw = 1000.0 * np.asarray(wall_vol, dtype=np.float64)[None, :] * kernel(p, w)
    return 0.001 + tf.sum(1) + tw.sum(1), (tf != 0).sum(1) + (tw != 0).sum(1), np.abs(tf).sum(1) + np.abs(tw).sum(1)


PBF_RHO_ROUNDINGS = 10


def check_pbf_rho_bound(cfg, pos, wall_pos, wall_vol, rho32, who):
    """|rho32 - rho64| <= (K + 10) 2^-24 sum |t_j| per particle: an f32 sum of K terms in any order is within (K - 1) u sum |t_j| of the exact
    sum of its terms (u = 2^-24), and each f32 term carries about ten roundings (the norm's subtractions, squares, additions and square
    root; r / h; q * q; 1 - q2; the two products of the cube; the products with the constant, with m or V_b and rho_0) -- a derived bound, not
    a measured one.  The second restatement's own rho uses 0.2 of it at worst on the jittered wall state, so the constant 10 stands."""
    rho64, K, tot = pbf_rho_f64(cfg, pos, wall_pos, wall_vol)
    err = np.abs(np.asarray(rho32, dtype=np.float64) - rho64)
    bound = (K + PBF_RHO_ROUNDINGS) * 2.0 ** -24 * tot
    print("%s: rho against the f64 all-pairs poly6 sum: terms per particle %d..%d, worst error / bound %.3f" % (who, K.min(), K.max(), float((err / bound).max())))
    assert K.min() > 0
    bad = np.flatnonzero(err > bound)
    assert len(bad) == 0, (who, len(bad), int(bad[0]), float(err[bad[0]]), float(bound[bad[0]]))


def test_pbf_rho_of_the_restatement_within_the_f64_bound():
    """before the library is held to check_pbf_rho_bound (test_second_restatement_gpu.py): the second restatement's f32 rho, bit-equal to what
    the GPU must produce, satisfies it for every particle of the jittered wall state"""
    from second_restatement_pbf import PbfSolver
    cfg = scenes.get("pbf_tiny_wall")
    s = PbfSolver(cfg)
    s.pos, s.vel = cs.jitter(cfg)
    s.density_only()
    check_pbf_rho_bound(cfg, s.pos, s.sc.wall_pos, s.sc.wall_vol, s.rho, "second restatement")
