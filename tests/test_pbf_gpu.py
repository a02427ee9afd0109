"""GPU suite, SURVEY.md 8f.4: the PBF step (pbf_solver.py:176-187) against the oracle, bit for bit.

The reference file is stale at the surveyed commit (fluid callbacks written for particle indices, for_all_neighbor passes structs) and
its update_all_pos races on pos / vel; library and oracle read it the same documented way (csrc/sph_pbf_kernels.h): callbacks on the
structs' fields, update_all_pos under the barrier-synchronised schedule.  Parity is therefore "equal to the restatement under that
reading", unpinned like the rest.  The reading itself is checked by a second, independently written restatement
(tests/second_restatement_pbf.py; tests/test_second_restatement.py for the oracle, tests/test_second_restatement_gpu.py for the library).

The cases of the lower half run what the upper half never reaches: the plain (one lane per particle) instantiations and the Morton cell
order that a default handle takes above 65 536 and from 131 072 particles, and a particle count that fills no workgroup."""
import numpy as np
import pytest

from cfd_taichi_amd import _native as nat
from cfd_taichi_amd import scenes
from harness import same_values, squeeze
from oracle import oracle as orc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("scene,steps,squeezed", [("pbf_tiny_wall", 150, True), ("pbf_tiny_clamp", 150, True), ("pbf_small", 60, False),
                                                  ("pbf_tiny_wall", 400, False)])
def test_pbf_steps(scene, steps, squeezed):
    cfg = scenes.get(scene)
    sim = nat.Simulation(nat.config_from_dict(cfg))
    o = orc.Oracle(cfg, num_threads=8)
    assert (sim.n_fluid, sim.n_wall) == (o.N, o.Nb)
    if squeezed:
        squeeze(sim, o)
    active = False
    for s in range(steps):
        sim.step_pbf(1)
        o.step_pbf(1)
        if s % 25 == 0 or s == steps - 1:
            lam = o.get(orc.F_PBF_LAMBDA)
            same_values(sim.download(nat.F_RHO), o.get(orc.F_RHO), "rho, step %d" % s)
            same_values(sim.download(nat.F_PBF_LAMBDA), lam, "pbf_lambda, step %d" % s)
            same_values(sim.download(nat.F_PBF_DELTA_POS), o.get(orc.F_PBF_DELTA_POS), "delta_pos, step %d" % s)
            same_values(sim.download(nat.F_POS), o.get(orc.F_POS), "pos, step %d" % s)
            same_values(sim.download(nat.F_VEL), o.get(orc.F_VEL), "vel, step %d" % s)
            active = active or bool((lam != 0).any())
    pos = sim.download(nat.F_POS)
    assert np.isfinite(pos).all()
    if squeezed or steps >= 400:
        assert active, "the density constraint never became active: lambda / delta_pos not exercised"
    sim.close(); o.close()


def test_pbf_mirror_api_and_30k():
    """main.py:65-68 discovery for `pbf`, and the 30 k dam break: the first steps against the oracle, then a longer run stays finite."""
    import importlib
    from cfd_taichi_amd import ParticleSystem
    cfg = scenes.get("breaking_dam_30k_pbf")
    ps = ParticleSystem(cfg)
    solver = getattr(importlib.import_module("cfd_taichi_amd.pbf_solver"), "pbf_solver")(ps, cfg)
    o = orc.Oracle(cfg, num_threads=8)
    for _ in range(5):
        solver.step(); o.step_pbf(1)
    same_values(ps.fluid_particles.pos.to_numpy(), o.get(orc.F_POS), "pos")
    same_values(ps.fluid_particles.vel.to_numpy(), o.get(orc.F_VEL), "vel")
    same_values(solver.pbf_lambda.to_numpy(), o.get(orc.F_PBF_LAMBDA), "lambda")
    same_values(solver.pos_predict.to_numpy(), o.get(orc.F_POS), "pos_predict == pos after a step (pbf_solver.py:84)")
    solver.step(400)
    pos = ps.fluid_particles.pos.to_numpy()
    assert np.isfinite(pos).all() and solver.delta_time[None] == np.float32(2.5e-4) and solver.simulate_cnt[None] == 405
    o.close()


def test_pbf_rejects_a_rigid_body():
    from cfd_taichi_amd import mesh
    cfg = scenes.get("dfsph_rigid_small")
    cfg["solver"]["name"] = "pbf"
    with pytest.raises(nat.SphError):
        nat.Simulation(nat.config_from_dict(cfg), rigid=mesh.rigid_from_config(cfg))


@pytest.mark.parametrize("scene", ["pbf_tiny_wall", "pbf_tiny_clamp"])
def test_pbf_compute_density_is_poly6_and_leaves_lambda_alone(scene):
    """solver_base.compute_all_rho() on a pbf solver: pbf_solver.py:166-174 overrides the rho callbacks with the poly6 kernel, and
    nothing but rho[] is written -- pbf_lambda keeps the values of the last step, positions and velocities keep their roles."""
    cfg = scenes.get(scene)
    sim = nat.Simulation(nat.config_from_dict(cfg))
    o = orc.Oracle(cfg, num_threads=8)
    squeeze(sim, o)
    for _ in range(3):
        sim.step_pbf(1); o.step_pbf(1)
    lam = o.get(orc.F_PBF_LAMBDA).copy()
    assert (lam != 0).any()
    pos, vel, dpos = sim.download(nat.F_POS), sim.download(nat.F_VEL), sim.download(nat.F_PBF_DELTA_POS)
    same_values(dpos, o.get(orc.F_PBF_DELTA_POS), "delta_pos before compute_density")
    sim.compute_density()
    o.build_grid(); o.compute_rho()
    same_values(sim.download(nat.F_RHO), o.get(orc.F_RHO), "rho after compute_density")
    same_values(sim.download(nat.F_PBF_LAMBDA), lam, "pbf_lambda after compute_density")
    same_values(sim.download(nat.F_PBF_DELTA_POS), dpos, "delta_pos after compute_density (carried through the re-sort like pbf_lambda)")
    same_values(sim.download(nat.F_POS), pos, "pos after compute_density")
    same_values(sim.download(nat.F_VEL), vel, "vel after compute_density")
    # rho is the poly6 sum, not the cubic spline one: the two differ on a squeezed lattice
    sim.step_pbf(1); o.step_pbf(1)
    same_values(sim.download(nat.F_POS), o.get(orc.F_POS), "pos, the step after")
    same_values(sim.download(nat.F_PBF_LAMBDA), o.get(orc.F_PBF_LAMBDA), "pbf_lambda, the step after")
    sim.close(); o.close()


# ---- the kernels and cell order a large handle really runs (the cases above all stay below 65 536 particles: k_pbf_*<true>, linear cells) ----

FIELDS = (("rho", nat.F_RHO, orc.F_RHO), ("pbf_lambda", nat.F_PBF_LAMBDA, orc.F_PBF_LAMBDA), ("delta_pos", nat.F_PBF_DELTA_POS, orc.F_PBF_DELTA_POS),
          ("pos", nat.F_POS, orc.F_POS), ("vel", nat.F_VEL, orc.F_VEL))


def water_block(nx, ny, nz, margin=0.5):
    """pbf_tiny_wall's scene (r = 0.025, Akinci walls) with a block of nx x ny x nz particles at (0.1, 0.1, 0.1) in a box `margin` larger than it"""
    cfg = scenes.get("pbf_tiny_wall")
    d = 2 * cfg["scene"]["particle_radius"]
    ws = [round(n * d, 6) for n in (nx, ny, nz)]
    cfg["scene"]["box_max"] = [round(w + margin, 6) for w in ws]
    cfg["fluid"].update(start_pos=[0.1, 0.1, 0.1], water_size=ws)
    return cfg


def lockstep(sim, o, steps):
    active = 0
    for s in range(steps):
        sim.step_pbf(1); o.step_pbf(1)
        for name, f, of in FIELDS:
            same_values(sim.download(f), o.get(of), "%s, step %d" % (name, s + 1))
        active = max(active, int((o.get(orc.F_PBF_LAMBDA) != 0).sum()))
    return active


@pytest.mark.parametrize("block,lo,hi", [((42, 40, 40), 65536, 131072), ((52, 52, 50), 131072, 1 << 18)],
                         ids=["linear_cells_plain_sweeps", "morton_cells_plain_sweeps"])
def test_pbf_beyond_the_thresholds_without_overrides(block, lo, hi):
    """The two thresholds of a default handle, with no development override in force: above quad_below = 65 536 particles step_pbf_once
    launches k_pbf_{lambda,delta,xsph}<false>, from 1 << 17 particles on the cells are stored along the Morton curve and k_pbf_xsph reaches them
    through cell_slot_xyz.  67 200 and 135 200 particles clear the thresholds by 2.5 % and 3.1 %; three squeezed steps, every field, every step."""
    cfg = water_block(*block)
    sim = nat.Simulation(nat.config_from_dict(cfg))
    o = orc.Oracle(cfg, num_threads=16)
    try:
        assert sim.overrides() == [], sim.overrides()
        assert lo < sim.n_fluid < min(hi, int(lo * 1.05)) and sim.n_fluid == block[0] * block[1] * block[2], sim.n_fluid
        assert (sim.n_fluid, sim.n_wall, tuple(sim.grid)) == (o.N, o.Nb, tuple(o.grid))
        squeeze(sim, o)
        active = lockstep(sim, o, 3)
        print("%d particles: up to %d with lambda != 0" % (sim.n_fluid, active))
        assert active > 0, "the density constraint never became active"
    finally:
        sim.close(); o.close()


@pytest.mark.parametrize("quad", ["1", "0"], ids=["quad", "plain"])
def test_pbf_ragged_last_workgroup(quad, monkeypatch):
    """A 9 x 10 x 7 block -- 629 particles by the reference's truncating count (ParticleSystem.py:85-86: 0.35 / 0.05 < 7), an incomplete top
    layer, neither a multiple of 64 (a quad workgroup's particles) nor of 256 (a plain one's): the last workgroup of both grids is partly empty -- `if (i >= c.n) return` with "a quad leaves together" in k_pbf_xsph, the prologue's guard in the list sweeps."""
    cfg = water_block(9, 10, 7)
    if quad == "0":
        monkeypatch.setenv("SPH_QUAD", "0")
    else:
        monkeypatch.delenv("SPH_QUAD", raising=False)
    sim = nat.Simulation(nat.config_from_dict(cfg))
    o = orc.Oracle(cfg, num_threads=4)
    try:
        assert sim.overrides() == (["SPH_QUAD=0"] if quad == "0" else []), sim.overrides()
        assert sim.n_fluid == o.N == 629 and sim.n_fluid % 64 and sim.n_fluid % 256
        squeeze(sim, o)
        active = lockstep(sim, o, 12)
        assert active > 0, "the density constraint never became active"
    finally:
        sim.close(); o.close()
