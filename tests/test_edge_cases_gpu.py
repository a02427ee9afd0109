"""GPU suite, edge cases (the reference has no tests; these are the degenerate inputs its code paths imply):
ragged particle counts far below one wave / one workgroup, a single particle, coincident particles (r = 0 takes the q <= 1e-5
branch of the kernel derivative, solver_base.py:96), and particles resting exactly on a cell face.  All four solvers, against
the oracle, bit for bit -- on the default handle and, for the ragged counts and the coincident particles, on the plain sweeps (SPH_QUAD=0) and
on Morton cells in tiles of 4^3 as well.  PBF, the fifth solver, has its own file: tests/test_pbf_edges_gpu.py."""
import numpy as np
import pytest

from cfd_taichi_amd import _native as nat
from cfd_taichi_amd import scenes
from oracle import oracle as orc

pytestmark = pytest.mark.gpu
SOLVERS = ["wcsph", "dfsph", "pcisph", "iisph"]


def tiny_scene(solver, water, start=(0.1, 0.1, 0.1), walls=True):
    cfg = scenes.get("dfsph_tiny_wall" if walls else "dfsph_tiny_clamp")
    cfg["solver"]["name"] = solver
    cfg["solver"]["delta_time"] = 2.5e-4 if solver == "wcsph" else 1e-3
    cfg["fluid"]["water_size"] = list(water)
    cfg["fluid"]["start_pos"] = list(start)
    return cfg


def step_both(sim, o, solver, n):
    for _ in range(n):
        if solver == "wcsph":
            sim.step_wcsph(1); o.step_wcsph(1)
        elif solver == "dfsph":
            st = sim.step_dfsph(1); o.step_dfsph(1, 100)
            assert (st.n_div, st.n_dens) == (o.last_stats.n_div, o.last_stats.n_dens)
        else:
            st = sim.step(1)
            (o.step_pcisph if solver == "pcisph" else o.step_iisph)(1)
            assert st.n_dens == o.last_stats.n_dens
    for f, of in ((nat.F_POS, orc.F_POS), (nat.F_VEL, orc.F_VEL), (nat.F_RHO, orc.F_RHO)):
        a, b = sim.download(f), o.get(of)
        assert np.array_equal(a, b, equal_nan=True), (solver, f, a[:4], b[:4])


WATERS = [(0.05, 0.05, 0.05), (0.35, 0.05, 0.05), (0.36, 0.16, 0.16), (0.26, 0.66, 0.06)]
# the other families of handle: the sweeps with one lane per particle instead of four, and cells along the Morton curve in tiles of 4^3
KIND_KNOBS = ("SPH_QUAD", "SPH_CELL_ORDER", "SPH_CELL_TILE")
KINDS = {"plain": {"SPH_QUAD": "0"}, "morton": {"SPH_CELL_ORDER": "morton", "SPH_CELL_TILE": "4"}}


def handle_of_kind(cfg, kind, monkeypatch):
    """kind None: the default handle, no knob in force.  Every knob that was set must be named by sim.overrides(), and no other of the three."""
    knobs = KINDS[kind] if kind else {}
    for name in KIND_KNOBS:
        monkeypatch.delenv(name, raising=False)
    for name, value in knobs.items():
        monkeypatch.setenv(name, value)
    sim = nat.Simulation(nat.config_from_dict(cfg))
    for name in KIND_KNOBS:
        monkeypatch.delenv(name, raising=False)
    named = sim.overrides()
    for name in KIND_KNOBS:
        assert [t for t in named if t.startswith(name + "=")] == (["%s=%s" % (name, knobs[name])] if name in knobs else []), (kind, named)
    return sim


def ragged_particle_counts(solver, water, sim_of):
    cfg = tiny_scene(solver, water, start=(0.05, 0.05, 0.05))
    sim = sim_of(cfg)
    o = orc.Oracle(cfg, solver=solver, num_threads=2)
    assert sim.n_fluid == o.N and 1 <= o.N < 128
    step_both(sim, o, solver, 25)
    sim.close(); o.close()


def coincident_particles_and_cell_faces(solver, sim_of):
    cfg = tiny_scene(solver, (0.3, 0.3, 0.3), start=(0.3, 0.3, 0.3), walls=False)
    sim = sim_of(cfg)
    o = orc.Oracle(cfg, solver=solver, num_threads=2)
    pos = o.get(orc.F_POS)
    pos[5] = pos[4]                                     # two particles in the same place: |x_ij| = 0
    pos[17] = pos[16] + np.float32(1e-7)                # q just above the 1e-5 gate's lower end
    pos[40] = np.float32([0.4, 0.5, 0.6])               # exactly on cell faces (h = 0.1)
    o.set(orc.F_POS, pos)
    sim.upload(nat.F_POS, pos)
    step_both(sim, o, solver, 15)
    sim.close(); o.close()


@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("water", WATERS)
def test_ragged_particle_counts(solver, water):
    """N = int(wx/d * wy/d * wz/d) (ParticleSystem.py:85-86): 1, 6, 73 and 82 particles -- below one wave, just above one wave."""
    ragged_particle_counts(solver, water, lambda cfg: nat.Simulation(nat.config_from_dict(cfg)))


@pytest.mark.parametrize("solver", SOLVERS)
def test_coincident_particles_and_cell_faces(solver):
    coincident_particles_and_cell_faces(solver, lambda cfg: nat.Simulation(nat.config_from_dict(cfg)))


@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("water", WATERS)
@pytest.mark.parametrize("kind", KINDS)
def test_ragged_particle_counts_on_the_other_handles(kind, solver, water, monkeypatch):
    """the same 1, 6, 73 and 82 particles on the plain sweeps and on Morton cells (the cases above keep their ids and run the default handle)"""
    ragged_particle_counts(solver, water, lambda cfg: handle_of_kind(cfg, kind, monkeypatch))


@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("kind", KINDS)
def test_coincident_particles_and_cell_faces_on_the_other_handles(kind, solver, monkeypatch):
    coincident_particles_and_cell_faces(solver, lambda cfg: handle_of_kind(cfg, kind, monkeypatch))


@pytest.mark.parametrize("scene,solver,steps", [("dfsph_dam_x", "dfsph", 700), ("wcsph_dam_x", "wcsph", 5000), ("dfsph_tiny_wall_iisph", "iisph", 800),
                                                ("dfsph_tiny_wall_pcisph", "pcisph", 500)])
def test_long_runs_with_wall_leaks_match_oracle(scene, solver, steps):
    """Hundreds to thousands of steps on small scenes whose single-layer walls leak: particles whose 1-D cell index wraps into a far cell
    or falls out of range (ParticleSystem.py:393).  The GPU path must stay on the oracle's trajectory bit for bit through all of it."""
    cfg = scenes.get(scene)
    sim = nat.Simulation(nat.config_from_dict(cfg))
    o = orc.Oracle(cfg, solver=solver, num_threads=8)
    chunk = 100
    for s0 in range(0, steps, chunk):
        if solver == "wcsph":
            sim.step_wcsph(chunk); o.step_wcsph(chunk)
        else:
            for _ in range(chunk):
                st = sim.step(1)
                if solver == "dfsph":
                    o.step_dfsph(1, 100)
                    assert (st.n_div, st.n_dens) == (o.last_stats.n_div, o.last_stats.n_dens), s0
                else:
                    (o.step_pcisph if solver == "pcisph" else o.step_iisph)(1)
                    assert st.n_dens == o.last_stats.n_dens, s0
        a, b = sim.download(nat.F_POS), o.get(orc.F_POS)
        assert np.array_equal(a, b, equal_nan=True), (scene, s0 + chunk, int((a != b).sum()))
    pos = o.get(orc.F_POS)
    box = np.asarray(cfg["scene"]["box_max"], dtype=np.float32)
    leaked = int(((pos < 0) | (pos > box)).any(axis=1).sum())
    print(scene, "particles outside the box at the end:", leaked)
    sim.close(); o.close()


@pytest.mark.parametrize("solver", ["wcsph", "dfsph"])
@pytest.mark.parametrize("morton", [False, True])
def test_spray_and_clump(solver, morton, monkeypatch):
    """The two ends of the cell occupancy the list build sees: spray -- every particle alone in its cell, so a wave holds 64 runs of
    equal cell (more than its per-wave table of cell entries takes: the per-lane path) -- and a clump of 40 particles inside one
    cell (more candidates than one 32-bit accept mask holds).  Both against the oracle, on the reference's cell order and on the curve."""
    if morton:
        monkeypatch.setenv("SPH_CELL_ORDER", "morton")
        monkeypatch.setenv("SPH_STAGE", "1")              # dfsph: staged workgroups (16-bit local lists) next to unstaged ones
    cfg = scenes.get("dfsph_tiny_clamp")
    cfg["solver"]["name"] = solver
    cfg["solver"]["delta_time"] = 2.5e-4 if solver == "wcsph" else 1e-3
    cfg["scene"]["box_max"] = [2.0, 2.0, 2.0]
    sim = nat.Simulation(nat.config_from_dict(cfg))
    o = orc.Oracle(cfg, solver=solver, num_threads=2)
    n = o.N
    rng = np.random.default_rng(5)
    pos = np.empty((n, 3), dtype=np.float32)
    # spray: one particle per cell on a jittered lattice of pitch 0.1 = h (neighbours in adjacent cells, 0.06 .. 0.14 apart)
    side = int(np.ceil((n - 40) ** (1.0 / 3.0)))
    g = np.stack(np.meshgrid(np.arange(side), np.arange(side), np.arange(side), indexing="ij"), -1).reshape(-1, 3)[: n - 40]
    pos[: n - 40] = (0.15 + 0.1 * g + rng.uniform(-0.02, 0.02, (n - 40, 3))).astype(np.float32)
    # clump: 40 particles inside the cell (15, 15, 15), 0.012 apart on average
    pos[n - 40:] = (1.5 + rng.uniform(0.02, 0.08, (40, 3))).astype(np.float32)
    pos = pos[rng.permutation(n)]
    o.set(orc.F_POS, pos)
    sim.upload(nat.F_POS, pos)
    sim.build_neighbors()
    assert sim.download(nat.F_NBR_COUNT).max() >= 39      # the clump is there
    step_both(sim, o, solver, 6)
    sim.close(); o.close()


def test_environment_knobs_are_development_overrides(monkeypatch, capfd):
    """Without SPH_DEV=1 a set SPH_* knob is ignored (one line on stderr), with it the handle reports it through sph_overrides."""
    cfg = nat.config_from_dict(scenes.get("dfsph_small"))
    monkeypatch.setenv("SPH_CELL_ORDER", "morton")
    monkeypatch.setenv("SPH_ARITH", "relaxed")
    monkeypatch.delenv("SPH_DEV", raising=False)
    sim = nat.Simulation(cfg)
    assert sim.overrides() == [] and sim.scalar(nat.S_ARITH_RELAXED) == 0.0
    sim.close()
    assert "SPH_CELL_ORDER is set but ignored" in capfd.readouterr().err
    monkeypatch.setenv("SPH_DEV", "1")
    sim = nat.Simulation(cfg)
    assert "SPH_CELL_ORDER=morton" in sim.overrides() and "SPH_ARITH=relaxed" in sim.overrides()
    sim.step_dfsph(1)
    assert sim.scalar(nat.S_ARITH_RELAXED) == 1.0
    sim.close()


def test_slab_protocol_switch_refuses_what_the_handle_cannot_do():
    """sph_slab_set_overlap: only slab handles have a protocol, and one created without the overlapped form (slab_overlap = 1, or the one-column
    protocol of the other solvers) cannot be switched to it; switching it OFF is always allowed."""
    one = nat.Simulation(nat.config_from_dict(scenes.get("dfsph_small")))
    with pytest.raises(nat.SphError):
        one.set_slab_overlap(False)
    one.close()
    cfg = scenes.get("dfsph_small")
    plain = nat.Simulation(nat.config_from_dict(cfg, slab_rank=0, slab_count=2, slab_overlap=1))
    with pytest.raises(nat.SphError):
        plain.set_slab_overlap(True)
    plain.set_slab_overlap(False)
    plain.close()
    able = nat.Simulation(nat.config_from_dict(cfg, slab_rank=1, slab_count=2))
    able.set_slab_overlap(False)
    able.set_slab_overlap(True)
    able.close()
    w = nat.Simulation(nat.config_from_dict(scenes.get("wcsph_small"), slab_rank=0, slab_count=2))
    with pytest.raises(nat.SphError):
        w.set_slab_overlap(True)
    w.close()
