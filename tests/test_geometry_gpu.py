"""GPU suite of static geometry (sph_geometry_add / _remove / _info / _carve, Simulation.add_geometry / remove_geometry / geometry / carve,
`scene.geometry`).

The yardstick is tests/geometry_ref.py (shown to be felt by test_geometry_cpu.py): the second restatement with the same groups appended to its
wall arrays and its volumes recomputed.  Every comparison with it is bit for bit (harness.same_bits) after every step; handles are compared
among themselves bit for bit as well.  The one tolerance is the project's parity bar for the relaxed arithmetic, 1e-5 on positions.  Every test
here fails without the entry points.

Scenes: the tiny wall scenes (640 particles, d = 0.05, h = 0.1, 2 402 box samples) with geometry_ref.PLATE (108 samples) and BLOCK (26)."""
import copy
import os

import numpy as np
import pytest

import geometry_ref as gr
import harness as h
import restatement_compare as rc
from cfd_taichi_amd import _native as nat
from cfd_taichi_amd import geometry, mesh, run, scenes

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
PLAIN = dict(h.LINEAR, SPH_QUAD="0")
WALL, VOL = (nat.F_WALL_POS, nat.SPECIES_WALL), (nat.F_WALL_VOL, nat.SPECIES_WALL)


def side(solver, monkeypatch, env=None, label="library", cfg=None, **config_kw):
    """a restatement_compare.NativeSide of the solver's tiny wall scene, created under `env` alone"""
    for k in h.KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    s = rc.NativeSide(cfg or scenes.get(gr.SCENES[solver]), None, solver, label)
    for k in (env or {}):
        assert any(t.startswith(k + "=") for t in s.sim.overrides()), (k, s.sim.overrides())
    return s


def same_walls(sim, walls, when):
    sc = walls.sc
    assert sim.n_wall == sc.Nb, (when, sim.n_wall, sc.Nb)
    h.same_bits(sim.download(*WALL), sc.wall_pos, "%s: SPH_F_WALL_POS" % when)
    h.same_bits(sim.download(*VOL), sc.wall_vol, "%s: SPH_F_WALL_VOL" % when)
    assert sim.geometry() == walls.info(), (when, sim.geometry(), walls.info())


def both(sides, walls, call, *args):
    """the same edit on the restatement's walls and on every side; the group ids must agree"""
    want = getattr(walls, call)(*args)
    for sd in sides:
        got = getattr(sd.sim, call + "_geometry")(*args)
        assert got == want, (call, got, want)
    return want


def twins_agree(a, b, solver, steps=3):
    for s in range(steps):
        h.same_stats(a.step(1), b.step(1), solver, "step %d: statistics" % (s + 1))
    for f in (nat.F_POS, nat.F_VEL, nat.F_RHO, nat.F_NBR_COUNT):
        h.same_bits(a.download(f), b.download(f), "field %d" % f)


# ---- 1: the wall tables ------------------------------------------------------------------------------------------------------------------------
def test_wall_tables_after_every_edit(monkeypatch):
    s, walls = gr.make_solver(scenes.get("dfsph_tiny_wall"))
    sd = side("dfsph", monkeypatch)
    try:
        same_walls(sd.sim, walls, "at creation")
        vol0 = walls.sc.wall_vol.copy()
        p = both([sd], walls, "add", gr.PLATE)
        same_walls(sd.sim, walls, "plate added")
        b = both([sd], walls, "add", gr.BLOCK)
        assert (p, b) == (1, 2)
        same_walls(sd.sim, walls, "block added")
        assert (sd.sim.download(*VOL)[:2402] != vol0).sum() == 116
        both([sd], walls, "remove", p)                          # the first: the block moves down and keeps its id
        same_walls(sd.sim, walls, "plate removed")
        assert sd.sim.geometry() == [(2, 2402, 26)]
        both([sd], walls, "remove", b)                          # the last: the box alone, with the volumes of creation
        same_walls(sd.sim, walls, "block removed")
        h.same_bits(sd.sim.download(*VOL), vol0, "the box's volumes after the last removal")
        assert both([sd], walls, "add", gr.BLOCK) == 3          # ids are never reused
        same_walls(sd.sim, walls, "block added again")
    finally:
        sd.close()


# ---- 2: steps with geometry from the start ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", ["wcsph", "dfsph", "pcisph", "iisph", "pbf"])
def test_five_steps_with_plate_and_block(solver, monkeypatch):
    s, walls = gr.make_solver(scenes.get(gr.SCENES[solver]))
    sd = side(solver, monkeypatch)
    try:
        both([sd], walls, "add", gr.PLATE)
        both([sd], walls, "add", gr.BLOCK)
        fullest = 0
        for k in range(1, 6):
            gr.step_and_compare(s, [sd], k, solver)
            per, row = gr.wall_evidence(s, walls)
            if solver == "pbf":                                 # (its lists are built at the predicted positions: a 19th particle reaches the block)
                assert per[1] == 80 and per[2] >= 18, per
            else:
                assert per == {1: 80, 2: 18}, per
            fullest = max(fullest, row)
            if solver == "dfsph":                               # the fullest wall row the handle has built so far
                assert sd.sim.last_stats.max_wall_nbrs == fullest == 19, (sd.sim.last_stats.max_wall_nbrs, fullest)
        same_walls(sd.sim, walls, "after the steps")
    finally:
        sd.close()


# ---- 3: edits mid-run --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", ["wcsph", "dfsph", "pcisph", "iisph", "pbf"])
def test_plate_added_after_five_steps(solver, monkeypatch):
    s, walls = gr.make_solver(scenes.get(gr.SCENES[solver]))
    sd = side(solver, monkeypatch)
    try:
        for k in range(1, 6):
            gr.step_and_compare(s, [sd], k, solver)
        both([sd], walls, "add", gr.PLATE)
        for k in range(6, 9):
            gr.step_and_compare(s, [sd], k, solver)
        assert gr.wall_evidence(s, walls)[0][1] > 0
    finally:
        sd.close()


@pytest.mark.parametrize("solver", ["wcsph", "dfsph", "pcisph", "iisph", "pbf"])
def test_plate_removed_after_five_steps(solver, monkeypatch):
    s, walls = gr.make_solver(scenes.get(gr.SCENES[solver]))
    sd = side(solver, monkeypatch)
    try:
        p = both([sd], walls, "add", gr.PLATE)
        b = both([sd], walls, "add", gr.BLOCK)
        for k in range(1, 6):
            gr.step_and_compare(s, [sd], k, solver)
        both([sd], walls, "remove", p)
        if solver == "dfsph":                                   # ... ending with no group left
            both([sd], walls, "remove", b)
            assert sd.sim.geometry() == [] and sd.sim.n_wall == 2402
        for k in range(6, 9):
            gr.step_and_compare(s, [sd], k, solver)
    finally:
        sd.close()


# ---- 4: the sweep modes --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", ["wcsph", "dfsph", "pcisph", "iisph", "pbf"])
def test_sweep_modes_agree_with_the_restatement(solver, monkeypatch):
    """plain, quad and Morton (staged where the solver stages) handles, dfsph also without its wall cache: each bit-equal to the restatement after
    every step, hence among themselves"""
    s, walls = gr.make_solver(scenes.get(gr.SCENES[solver]))
    modes = {"plain": PLAIN, "quad": None, "morton": h.MORTON, "morton plain": dict(h.MORTON, SPH_QUAD="0")}
    if solver == "dfsph":
        modes["plain, no wall cache"] = dict(PLAIN, SPH_WALL_CACHE="0")
        modes["morton, no wall cache"] = dict(h.MORTON, SPH_QUAD="0", SPH_WALL_CACHE="0")
    sides = [side(solver, monkeypatch, env, "library (%s)" % name) for name, env in modes.items()]
    try:
        both(sides, walls, "add", gr.PLATE)
        both(sides, walls, "add", gr.BLOCK)
        for k in range(1, 4):
            gr.step_and_compare(s, sides, k, solver)
        both(sides, walls, "remove", 1)
        gr.step_and_compare(s, sides, 4, solver)
    finally:
        for sd in sides:
            sd.close()


# ---- 5: captured graphs ----------------------------------------------------------------------------------------------------------------------------------
def test_wcsph_graphs_follow_the_walls(monkeypatch):
    cfg = scenes.get("wcsph_tiny_wall")
    a, b = h.make_handle(cfg, monkeypatch), h.make_handle(cfg, monkeypatch)
    a.step(4)
    for _ in range(4):
        b.step(1)
    assert a.scalar(nat.S_GRAPH_LAUNCHES) > 0
    assert a.add_geometry(gr.PLATE) == b.add_geometry(gr.PLATE) == 1
    a.step(4)
    for _ in range(4):
        b.step(1)
    for f in (nat.F_POS, nat.F_VEL, nat.F_RHO, nat.F_PRESSURE, nat.F_ACC):
        h.same_bits(a.download(f), b.download(f), "field %d across the edit" % f)
    a.remove_geometry(1); b.remove_geometry(1)
    a.step(4)
    for _ in range(4):
        b.step(1)
    for f in (nat.F_POS, nat.F_VEL, nat.F_RHO):
        h.same_bits(a.download(f), b.download(f), "field %d across the removal" % f)
    plain = h.make_handle(cfg, monkeypatch)
    plain.step(12)
    assert (plain.download(nat.F_POS) != a.download(nat.F_POS)).any(), "the plate was not felt"
    a.close(); b.close(); plain.close()


# ---- 6: relaxed handles --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", ["dfsph", "wcsph", "pbf"])
def test_relaxed_handles_take_geometry(solver, monkeypatch):
    """one step from the shared initial state: the wall neighbours of every particle are the exact handle's (a Verlet handle: those and the ones
    within its skin), every position within 1e-5 of the exact handle's (README, "Parity status")"""
    cfg = scenes.get(gr.SCENES[solver])
    exact, relaxed = h.make_handle(cfg, monkeypatch), h.make_handle(cfg, monkeypatch, arith="relaxed")
    assert relaxed.scalar(nat.S_ARITH_RELAXED) == 1.0
    for sim in (exact, relaxed):
        assert sim.add_geometry(gr.PLATE) == 1 and sim.add_geometry(gr.BLOCK) == 2
    if solver != "wcsph":              # (a Verlet handle bins its walls in cells of h + skin: the same sums in another order, at creation already)
        h.same_bits(relaxed.download(*VOL), exact.download(*VOL), "volumes")
    assert np.isfinite(relaxed.download(*VOL)).all() and relaxed.n_wall == exact.n_wall == 2536
    se, sr = exact.step(1), relaxed.step(1)
    if solver == "dfsph":
        assert se.max_wall_nbrs == sr.max_wall_nbrs == 19, (se.max_wall_nbrs, sr.max_wall_nbrs)
    we, wr = exact.wall_neighbor_counts(), relaxed.wall_neighbor_counts()
    assert we.max() == 19 and (we > 0).sum() >= 98                  # (80 list the plate and 18 the block: test_geometry_cpu.py)
    if solver != "wcsph":
        h.same_values(wr, we, "wall neighbours per particle")
        h.same_bits(relaxed.download(nat.F_NBR_COUNT), exact.download(nat.F_NBR_COUNT), "neighbour count")
    else:              # a Verlet handle lists the pairs within h + skin: every wall entry of the exact handle and, for some particles, more
        assert (wr >= we).all() and (wr > we).any() and wr.max() <= relaxed.max_wall_neighbors
    worst = float(np.abs(relaxed.download(nat.F_POS).astype(np.float64) - exact.download(nat.F_POS)).max())
    print("relaxed %s with geometry: worst position difference after one step %.3e" % (solver, worst))
    assert worst <= 1e-5
    exact.close(); relaxed.close()


# ---- 6b: a coupled body ---------------------------------------------------------------------------------------------------------------------------
def test_coupled_body_beside_a_plate(monkeypatch):
    """The restatement's own coupled scene (coupled_scenes.coupled: the tiny wall scene with a box of 168 samples in the water's support radius)
    with a plate 0.075 beside the column, three solver and body steps against second_restatement_rigid.  dfsph_rigid_small itself (5 760 fluid,
    9 000 wall particles) is beyond the all-pairs arrays of the restatement; this is the scene the restatement's coupled tests run on."""
    import coupled_scenes as cs
    from second_restatement import Solver
    cfg = cs.coupled("dfsph")
    rg = cs.rigid(cfg)
    s = Solver(cfg, rg)
    s.max_dens = 100
    walls = gr.Walls(s)
    for k in h.KNOBS:
        monkeypatch.delenv(k, raising=False)
    sd = rc.NativeSide(cfg, rg, "dfsph")
    plate = np.array([[gr.D * i, gr.D * j, 0.475] for i in range(1, 10) for j in range(1, 13)], dtype=F)      # clear of the body (x >= 0.47)
    try:
        both([sd], walls, "add", plate)
        force = 0.0
        for k in range(1, 4):
            gr.step_and_compare(s, [sd], k, "dfsph")
            h.same_bits(s.body.force, sd.get("rigid_force"), "step %d: per-sample force" % k)
            force = max(force, float(np.abs(s.body.force).max()))
            assert gr.wall_evidence(s, walls)[0][1] > 50
            with np.errstate(all="ignore"):
                s.rigid_step()
            sd.rigid_step()
            rc._same_body(s.body, sd, "after rigid step %d" % k, True)
        assert force > 0, "the fluid never pushed the body"
    finally:
        sd.close()


# ---- 7: carving --------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", ["dfsph", "wcsph"])
def test_carve_removes_the_helpers_set(solver, monkeypatch):
    s, walls = gr.make_solver(scenes.get(gr.SCENES[solver]))
    sd = side(solver, monkeypatch)
    sim = sd.sim
    try:
        for k in range(1, 4):
            gr.step_and_compare(s, [sd], k, solver)
        sim.enable_scalar(0.0, 0.0, 0.0, values=np.arange(640, dtype=F))
        far = both([sd], walls, "add", gr.PLATE)                # 0.075 from the column: nobody within d
        before = {f: sim.download(f) for f in (nat.F_POS, nat.F_VEL, nat.F_RHO, nat.F_NBR_COUNT)}
        assert not walls.carve_mask(s.pos, far).any() and sim.carve(far) == 0 and sim.n_fluid == 640
        for f, was in before.items():                           # not even what is valid changed
            h.same_bits(sim.download(f), was, "field %d after a carve that removed nobody" % f)
        g = both([sd], walls, "add", gr.CARVE_PLATE)
        gone = walls.carve_mask(s.pos, g)
        assert 100 < gone.sum() < 640
        assert sim.carve(g) == gone.sum() and sim.n_fluid == 640 - gone.sum()
        h.same_bits(sim.download(nat.F_POS), before[nat.F_POS][~gone], "survivors: pos")
        h.same_bits(sim.download(nat.F_VEL), before[nat.F_VEL][~gone], "survivors: vel")
        h.same_bits(sim.scalar(), np.arange(640, dtype=F)[~gone], "survivors: the carried scalar")
        sim.disable_scalar()
        gr.keep_rows(s, ~gone)
        for k in range(4, 6):
            gr.step_and_compare(s, [sd], k, solver)
    finally:
        sd.close()


def test_carve_at_rest_default_clearance_and_every_group(monkeypatch):
    """the lattice at rest: the plate at x = 0.225 takes 160 of the 640 at the default clearance d; group -1 is every added group"""
    cfg = scenes.get("dfsph_tiny_wall")
    s, walls = gr.make_solver(cfg)
    a, b = h.make_handle(cfg, monkeypatch), h.make_handle(cfg, monkeypatch, h.MORTON)
    for sim in (a, b):
        assert sim.add_geometry(gr.PLATE) == 1 and sim.add_geometry(gr.CARVE_PLATE) == 2
    walls.add(gr.PLATE); walls.add(gr.CARVE_PLATE)
    gone = walls.carve_mask(s.pos, 2)
    assert gone.sum() == 160 and (walls.carve_mask(s.pos, -1) == gone).all()
    assert a.carve(2) == 160 and b.carve() == 160
    h.same_bits(a.download(nat.F_POS), s.pos[~gone], "survivors")
    h.same_bits(b.download(nat.F_POS), s.pos[~gone], "survivors (group -1, Morton cells)")
    twins_agree(a, b, "dfsph")
    a.close(); b.close()


# ---- 8: invisibility -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", ["dfsph", "wcsph", "pbf"])
def test_a_group_added_and_removed_is_invisible(solver, monkeypatch):
    cfg = scenes.get(gr.SCENES[solver])
    a, b = h.make_handle(cfg, monkeypatch), h.make_handle(cfg, monkeypatch)
    g = a.add_geometry(gr.PLATE)
    a.remove_geometry(g)
    assert a.n_wall == b.n_wall and a.geometry() == []
    h.same_bits(a.download(*WALL), b.download(*WALL), "wall positions")
    h.same_bits(a.download(*VOL), b.download(*VOL), "wall volumes")
    twins_agree(a, b, solver, steps=5)
    a.step(2); b.step(2)                                            # (wcsph: captured pairs)
    h.same_bits(a.download(nat.F_POS), b.download(nat.F_POS), "positions after a multi-step call")
    a.close(); b.close()


# ---- 9: refusals ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", ["dfsph", "wcsph", "pbf"])
def test_refusals_leave_the_handle_unchanged(solver, monkeypatch):
    cfg = scenes.get(gr.SCENES[solver])
    a, b = h.make_handle(cfg, monkeypatch), h.make_handle(cfg, monkeypatch)
    a.step(2); b.step(2)
    for sim in (a, b):
        assert sim.add_geometry(gr.PLATE) == 1
    state = [a.download(f) for f in (nat.F_POS, nat.F_VEL, nat.F_RHO, nat.F_NBR_COUNT)] + [a.download(*WALL), a.download(*VOL)]
    inv = nat.SPH_E_INVALID
    h.refused(inv, lambda: a.add_geometry(np.zeros((0, 3), F)))                                                    # n == 0 (and a null pointer)
    add = a._lib.sph_geometry_add
    assert add(a._h, None, 5, None) == inv                                                                         # null positions
    assert add(a._h, gr.BLOCK.ctypes.data, 1 << 28, None) == inv                                                   # refused before a byte is read
    for bad in (np.nan, np.inf, -0.06, 1.35):                                                                      # not finite; a cell outside the grid
        pts = gr.BLOCK.copy(); pts[7, 1] = bad
        h.refused(inv, lambda: a.add_geometry(pts))
    h.refused(inv, lambda: a.add_geometry(F([[0.7, 0.5, 0.7]])))                                                   # an isolated sample: infinite volume
    h.refused(inv, lambda: a.add_geometry(F([[0.7, 0.5, 0.7], [0.7, 0.5, 0.85]])))                                 # ... two of them, 1.5 h apart
    h.refused(inv, lambda: a.remove_geometry(2))
    h.refused(inv, lambda: a.remove_geometry(0))                                                                   # the box is no group to remove
    h.refused(inv, lambda: a.carve(2))
    h.refused(inv, lambda: a.carve(0))
    for clearance in (0.0, -0.05, float(np.nextafter(F(0.1), F(1))), np.nan):
        h.refused(inv, lambda: a.carve(1, clearance))
    counts = a._lib.sph_geometry_wall_counts
    room = np.zeros(641, dtype=np.int32)
    assert counts(a._h, None, 640) == inv and counts(a._h, room.ctypes.data, 641) == inv and counts(a._h, room.ctypes.data, 639) == inv
    info = a._lib.sph_geometry_info
    assert info(a._h, None, None, None, 1, None) == inv
    assert a.n_wall == 2402 + 108 and a.geometry() == [(1, 2402, 108)] and a.n_fluid == 640
    for f, was in zip([(nat.F_POS,), (nat.F_VEL,), (nat.F_RHO,), (nat.F_NBR_COUNT,), WALL, VOL], state):
        h.same_bits(a.download(*f), was, "field %d after the refused calls" % f[0])
    assert a.add_geometry(F([[0.7, 0.5, 0.7], [0.7, 0.5, 0.7]])) == 2                                               # coincident samples are allowed: W(0) each
    a.remove_geometry(2)
    twins_agree(a, b, solver)
    a.close(); b.close()


def test_a_carve_that_would_take_every_particle_is_refused(monkeypatch):
    cfg = scenes.get("dfsph_tiny_wall")
    a, b = h.make_handle(cfg, monkeypatch), h.make_handle(cfg, monkeypatch)
    pos = a.download(nat.F_POS)
    for sim in (a, b):
        assert sim.add_geometry(pos) == 1                                                                          # a sample on every particle
    h.refused(nat.SPH_E_INVALID, lambda: a.carve(1))
    assert a.n_fluid == 640
    a.remove_geometry(1); b.remove_geometry(1)
    twins_agree(a, b, "dfsph")
    a.close(); b.close()


def test_clamp_walls_and_bodies_refuse(monkeypatch):
    a, b = h.make_handle(scenes.get("dfsph_tiny_clamp"), monkeypatch), h.make_handle(scenes.get("dfsph_tiny_clamp"), monkeypatch)
    h.refused(nat.SPH_E_INVALID, lambda: a.add_geometry(gr.PLATE))
    h.refused(nat.SPH_E_INVALID, lambda: a.carve())
    twins_agree(a, b, "dfsph")
    a.close(); b.close()
    body = scenes.get("dfsph_rigid_small")
    rigid = mesh.rigid_from_config(body)
    a, b = (nat.Simulation(nat.config_from_dict(body), rigid=rigid) for _ in range(2))
    lo = a.download(nat.F_POS).min(0)
    shelf = geometry.plate(lo - F([0.0, 0.075, 0.0]), [0.3, 0, 0], [0, 0, 0.3], 0.05)                                # under the column's corner
    for sim in (a, b):
        assert sim.add_geometry(shelf) == 1                                                                        # geometry next to a body is fine ...
    h.refused(nat.SPH_E_STATE, lambda: a.carve(1))                                                                 # ... carving is what sph_remove_in_box refuses
    for s in range(3):
        h.same_stats(a.step(1), b.step(1), "dfsph", "step %d" % (s + 1))
        a.rigid_step(); b.rigid_step()
    h.same_bits(a.download(nat.F_POS), b.download(nat.F_POS), "positions")
    a.close(); b.close()


# ---- 10: overflow ----------------------------------------------------------------------------------------------------------------------------------------
def test_geometry_reaches_the_wall_row_overflow(monkeypatch):
    """max_wall_neighbors 8 with the plate: SPH_E_OVERFLOW from the step.  And at the capacity that holds the fullest row of the box alone (what
    the restatement counts), the plate added three times over overflows it while the untouched twin steps on"""
    cfg = scenes.get("dfsph_tiny_wall")
    sim = h.make_handle(cfg, monkeypatch, max_wall_neighbors=8)
    sim.add_geometry(gr.PLATE)
    msg = h.refused(nat.SPH_E_OVERFLOW, lambda: sim.step(1))
    assert "19 wall neighbours, capacity 64 / 8" in msg, msg
    sim.close()
    s, walls = gr.make_solver(cfg)
    s.prologue()
    alone = int(s.nw.count.max())
    for _ in range(3):                                              # coincident samples are allowed: the plate three times over
        walls.add(gr.PLATE)
    s.prologue()
    full = int(s.nw.count.max())
    assert alone == 19 and full == 24
    a, b = h.make_handle(cfg, monkeypatch, max_wall_neighbors=alone), h.make_handle(cfg, monkeypatch, max_wall_neighbors=alone)
    assert alone <= a.max_wall_neighbors < full                     # (the library rounds a row's capacity up to whole groups of four entries)
    for _ in range(3):
        a.add_geometry(gr.PLATE)
    h.refused(nat.SPH_E_OVERFLOW, lambda: a.step(1))
    b.step(1)
    a.close(); b.close()


# ---- 11: config, runner, scenes ----------------------------------------------------------------------------------------------------------------------
def test_scene_geometry_of_a_config(monkeypatch):
    cfg = copy.deepcopy(scenes.get("dfsph_tiny_wall"))
    cfg["scene"]["geometry"] = [{"name": "far", "type": "points", "points": gr.PLATE.tolist()},
                                {"name": "cut", "type": "plate", "origin": [0.225, 0.05, 0.05], "u": [0, 0.55, 0], "v": [0, 0, 0.4], "carve": True}]
    for k in h.KNOBS:
        monkeypatch.delenv(k, raising=False)
    sim = nat.Simulation(nat.config_from_dict(cfg), config=cfg)
    assert sim.geometry_groups == {"far": 1, "cut": 2} and sim.geometry() == [(1, 2402, 108), (2, 2510, 108)]
    assert sim.n_fluid == 640 - 160
    sim.step(2)
    assert np.isfinite(sim.download(nat.F_POS)).all()
    sim.close()


def test_runner_pulls_the_gate(monkeypatch, tmp_path):
    for k in h.KNOBS:
        monkeypatch.delenv(k, raising=False)
    run.main(["--config", os.path.join(ROOT, "config", "dam_gate_wcsph.json"), "--steps", "3", "--remove-geometry", "gate@2", "--geometry-ply", str(tmp_path)])
    sim = run.LAST["ps"]._sim
    assert run.LAST["geometry_frames"] == 2 and sorted(os.listdir(tmp_path)) == ["geometry_000000.ply", "geometry_000002.ply"]
    rows = [open(os.path.join(tmp_path, p)).read().split("end_header\n")[1].splitlines() for p in sorted(os.listdir(tmp_path))]
    assert len(rows[1]) == sim.n_wall and len(rows[0]) == sim.n_wall + 1711 and sim.geometry() == []
    assert {r.split()[3] for r in rows[0]} == {"0", "1"} and {r.split()[3] for r in rows[1]} == {"0"}
    assert np.isfinite(sim.download(nat.F_POS)).all()


@pytest.mark.parametrize("name,samples", [("dam_pillars_dfsph", 3 * 498), ("dam_gate_wcsph", 1711), ("pbf_step_pbf", 322)])
def test_shipped_scenes_take_three_steps(name, samples, monkeypatch):
    for k in h.KNOBS:
        monkeypatch.delenv(k, raising=False)
    cfg = scenes.get(name)
    sim = nat.Simulation(nat.config_from_dict(cfg), config=cfg)
    twin = nat.Simulation(nat.config_from_dict(cfg))
    assert sim.n_wall == twin.n_wall + samples and sorted(sim.geometry_groups) == [e["name"] for e in cfg["scene"]["geometry"]]
    assert np.isfinite(sim.download(*VOL)).all()
    sim.step(3); twin.step(3)
    pos, rho = sim.download(nat.F_POS), sim.download(nat.F_RHO)
    assert np.isfinite(pos).all() and np.isfinite(rho).all()
    if name == "dam_gate_wcsph":                                    # the gate stands a spacing and a half from the column: in its density sums from the first step
        assert (rho != twin.download(nat.F_RHO)).sum() > 1000
    sim.close(); twin.close()
