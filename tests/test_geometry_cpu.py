"""CPU suite of static geometry (no library is loaded): the samplers of cfd_taichi_amd/geometry.py, the facts that make
tests/geometry_ref.py a yardstick a geometry nobody feels cannot pass, `scene.geometry` parsing, the shipped scenes' blocks, the runner's flags
and PLY writer on a fake simulation, and the new names against the header.

The facts, measured on the second restatement (tiny wall scenes: 640 particles, d = 0.05, h = 0.1, 2 402 box samples; PLATE 108 samples, BLOCK 26):
80 particles list a plate sample and 18 a block sample in each of the first ten steps; every volume is finite; after ten steps the positions differ
from the run without geometry in 61 rows for wcsph, 520 for iisph, 554 for pcisph and all 640 for dfsph, by up to 2.0e-3 (dfsph); the fullest wall
row of the ten steps holds 19 entries, 20 on pcisph (at its tenth step); the plate at x = 0.225 carves 160 particles at clearance d; 116 box volumes
change (the feature's issue quotes 115: the tests hold the restatement's own figure)."""
import copy
import json
import os
import re

import numpy as np
import pytest

import geometry_ref as gr
from cfd_taichi_amd import _native, geometry, run, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


# ---- the samplers --------------------------------------------------------------------------------------------------------------------------------
def test_plate_counts_order_and_spacing():
    p = geometry.plate([0.475, 0.05, 0.05], [0, 0.55, 0], [0, 0, 0.40], 0.05)
    assert p.dtype == np.float32 and p.shape == (108, 3)
    assert np.abs(p - gr.PLATE).max() < 1e-7                         # u outermost, on the d lattice: the test plate
    assert p.tobytes() == geometry.plate([0.475, 0.05, 0.05], [0, 0.55, 0], [0, 0, 0.40], 0.05).tobytes()
    ramp = geometry.plate([1.0, 0.05, 0.05], [0.8, 0.6, 0.0], [0, 0, 0.5], 0.05)          # |u| = 1: 20 intervals; 10 along v
    assert ramp.shape == (21 * 11, 3)
    step = np.linalg.norm(ramp[11] - ramp[0])
    assert abs(step - 0.05) < 1e-6 and abs(np.linalg.norm(ramp[1] - ramp[0]) - 0.05) < 1e-6
    assert np.allclose(ramp[-1], [1.8, 0.65, 0.55], atol=1e-6)
    assert geometry.plate([0, 0, 0], [0, 0, 0], [0, 0, 0.1], 0.05).shape == (3, 3)       # a degenerate edge: a line of samples


def test_box_shell_counts_and_order():
    b = geometry.box_shell([0.10, 0.05, 0.475], [0.20, 0.15, 0.575], 0.05)
    assert b.dtype == np.float32 and b.shape == (26, 3)
    assert np.abs(b - gr.BLOCK).max() < 1e-7                         # C order of (i, j, k), the centre left out: the test block
    big = geometry.box_shell([0, 0, 0], [0.5, 0.3, 0.2], 0.1)
    assert len(big) == 6 * 4 * 3 - 4 * 2 * 1 and len(np.unique(big, axis=0)) == len(big)
    on_face = np.zeros(len(big), dtype=bool)
    for a, hi in enumerate((0.5, 0.3, 0.2)):
        on_face |= np.isclose(big[:, a], 0) | np.isclose(big[:, a], hi)
    assert on_face.all()
    with pytest.raises(ValueError):
        geometry.box_shell([0, 0, 0], [1, -1, 1], 0.1)
    with pytest.raises(ValueError):
        geometry.box_shell([0, 0, 0], [1, 1, 1], 0.0)


def test_sphere_shell():
    s = geometry.sphere_shell([0.5, 0.5, 0.5], 0.2, 0.05)
    assert s.dtype == np.float32 and len(s) == int(round(4 * np.pi * 0.04 / 0.0025)) == 201
    r = np.linalg.norm(s.astype(np.float64) - 0.5, axis=1)
    assert np.abs(r - 0.2).max() < 1e-6
    assert (np.diff(s[:, 2]) < 0).all()                              # top to bottom
    d = np.linalg.norm(s[:, None, :].astype(np.float64) - s[None, :, :], axis=2) + np.eye(len(s))
    assert 0.5 * 0.05 < d.min(axis=1).min() and d.min(axis=1).max() < 1.5 * 0.05          # about one sample per spacing^2
    assert s.tobytes() == geometry.sphere_shell([0.5, 0.5, 0.5], 0.2, 0.05).tobytes()


def test_mesh_samples_of_the_cube():
    """assets/cube1.stl is the box 0.8 x 0.5 x 1.0 (mesh.py): at pitch 0.05 a 17 x 11 x 21 block of voxels"""
    shell = geometry.mesh_samples("assets/cube1.stl", 0.05)
    solid = geometry.mesh_samples("assets/cube1.stl", 0.05, fill=True)
    assert solid.shape == (17 * 11 * 21, 3) and shell.shape == (17 * 11 * 21 - 15 * 9 * 19, 3) and shell.dtype == np.float32
    moved = geometry.mesh_samples("assets/cube1.stl", 0.05, scale=0.5, translate=(1.0, 0.2, 0.3))
    assert np.allclose(moved.min(0), [1.0, 0.2, 0.3], atol=1e-6) and np.allclose(moved.max(0), [1.4, 0.45, 0.8], atol=1e-6)
    assert shell.tobytes() == geometry.mesh_samples("assets/cube1.stl", 0.05).tobytes()


# ---- the helper's facts ----------------------------------------------------------------------------------------------------------------------------
def test_walls_helper_bookkeeping():
    s, walls = gr.make_solver(scenes.get("dfsph_tiny_wall"))
    assert s.sc.Nb == 2402 and gr.PLATE.shape == (108, 3) and gr.BLOCK.shape == (26, 3)
    vol0 = s.sc.wall_vol.copy()
    assert np.array_equal(gr.volumes(s.sc, s.sc.wall_pos), vol0)      # the helper's loop is Scene.__init__'s
    p, b = walls.add(gr.PLATE), walls.add(gr.BLOCK)
    assert (p, b) == (1, 2) and walls.info() == [(1, 2402, 108), (2, 2510, 26)] and s.sc.Nb == 2536
    assert np.isfinite(s.sc.wall_vol).all() and (s.sc.wall_vol > 0).all()
    changed = s.sc.wall_vol[:2402] != vol0
    assert changed.sum() == 116 and (s.sc.wall_vol[:2402][changed] < vol0[changed]).all()      # a box sample next to geometry gets a smaller volume
    cells = s.sc.cell(s.sc.wall_pos)
    assert (cells >= 0).all() and (cells < np.array(s.sc.grid)).all()
    walls.remove(p)
    assert walls.info() == [(2, 2402, 26)] and s.sc.Nb == 2428
    walls.remove(b)
    assert walls.info() == [] and np.array_equal(s.sc.wall_vol, vol0)
    assert walls.add(gr.BLOCK) == 3
    one = F([[0.7, 0.5, 0.7]])
    walls.add(one)
    assert np.isinf(s.sc.wall_vol[-1])                               # an isolated sample: what the library refuses
    walls.remove(4)
    g = walls.add(gr.CARVE_PLATE)
    gone = walls.carve_mask(s.pos, g)
    assert gone.sum() == 160 and not walls.carve_mask(s.pos, 3).any() and (walls.carve_mask(s.pos, -1) == gone).all()
    assert (np.abs(s.pos[gone][:, 0] - 0.225) < 0.05).all() and (np.abs(s.pos[~gone][:, 0] - 0.225) >= 0.05 - 1e-6).all()


@pytest.mark.parametrize("solver,rows,fullest_row", [("wcsph", 61, 19), ("iisph", 520, 19), ("pcisph", 554, 20), ("dfsph", 640, 19)])
def test_the_geometry_is_felt(solver, rows, fullest_row):
    cfg = scenes.get(gr.SCENES[solver])
    s, walls = gr.make_solver(cfg)
    plain, _ = gr.make_solver(cfg)
    walls.add(gr.PLATE); walls.add(gr.BLOCK)
    fullest = 0
    with np.errstate(all="ignore"):
        for k in range(10):
            s.step(); plain.step()
            per, row = gr.wall_evidence(s, walls)
            assert per == {1: 80, 2: 18}, (k, per)
            fullest = max(fullest, row)
    assert fullest == fullest_row
    differ = (s.pos != plain.pos).any(axis=1)
    worst = float(np.abs(s.pos - plain.pos).max())
    print("%s: %d rows differ after ten steps, by up to %.3e" % (solver, differ.sum(), worst))
    assert differ.sum() == rows and np.isfinite(s.pos).all()
    if solver == "dfsph":
        assert 1.9e-3 < worst < 2.1e-3


# ---- config parsing ------------------------------------------------------------------------------------------------------------------------------------
class FakeSim:
    """what apply_config, the runner's removals and the PLY writer need of a Simulation"""

    def __init__(self, n_box=4):
        self.box = np.zeros((n_box, 3), dtype=F)
        self.groups, self.next_id, self.carved = [], 1, []

    def add_geometry(self, pts):
        self.groups.append((self.next_id, np.asarray(pts, dtype=F)))
        self.next_id += 1
        return self.next_id - 1

    def remove_geometry(self, g):
        assert g in [k for k, _ in self.groups]
        self.groups = [(k, p) for k, p in self.groups if k != g]

    def carve(self, group=-1, clearance=None):
        self.carved.append((group, clearance))
        return 0

    def geometry(self):
        out, at = [], len(self.box)
        for g, p in self.groups:
            out.append((g, at, len(p)))
            at += len(p)
        return out

    def download(self, field, species):
        assert (field, species) == (_native.F_WALL_POS, _native.SPECIES_WALL)
        return np.concatenate([self.box] + [p for _, p in self.groups])


def test_scene_geometry_block():
    cfg = copy.deepcopy(scenes.get("dfsph_tiny_wall"))
    assert geometry.config_groups(cfg) == [] and geometry.apply_config(FakeSim(), cfg) == {}
    cfg["scene"]["geometry"] = [
        {"name": "plate", "type": "plate", "origin": [0.475, 0.05, 0.05], "u": [0, 0.55, 0], "v": [0, 0, 0.40]},
        {"name": "block", "type": "box", "min": [0.10, 0.05, 0.475], "max": [0.20, 0.15, 0.575], "carve": True},
        {"name": "ball", "type": "sphere", "centre": [0.7, 0.3, 0.7], "radius": 0.1, "spacing": 0.025, "carve": 0.08},
        {"name": "cube", "type": "mesh", "mesh": "assets/cube1.stl", "scale": 0.25, "translate": [0.6, 0.05, 0.1]},
        {"name": "dots", "type": "points", "points": [[0.5, 0.5, 0.5], [0.5, 0.55, 0.5]]}]
    got = geometry.config_groups(cfg)
    assert [(n, len(p), c) for n, p, c in got] == [("plate", 108, False), ("block", 26, True), ("ball", 201, 0.08), ("cube", len(got[3][1]), False), ("dots", 2, False)]
    assert all(p.dtype == np.float32 and p.ndim == 2 for _, p, _ in got)          # the default spacing is the particle diameter
    sim = FakeSim()
    assert geometry.apply_config(sim, cfg) == {"plate": 1, "block": 2, "ball": 3, "cube": 4, "dots": 5}
    assert sim.carved == [(2, None), (3, 0.08)]
    for bad in ({"type": "plate", "origin": [0, 0, 0], "u": [1, 0, 0], "v": [0, 1, 0]},                              # no name
                {"name": "plate", "type": "points", "points": [[0, 0, 0]]},                                      # a name twice
                {"name": "x", "type": "cone"}, {"name": "x", "type": "box", "min": [0, 0, 0]},                  # unknown type; a key missing
                {"name": "x", "type": "box", "min": [0, 0, 0], "max": [1, 1, 1], "colour": 3},                   # an unknown key
                {"name": "x", "type": "box", "min": [0, 0, 0], "max": [1, 1, 1], "fill": True},                  # a mesh's key on a box
                {"name": "x", "type": "plate", "origin": [0, 0, 0], "u": [1, 0, 0], "v": [0, 1, 0], "scale": 2},
                {"name": "x", "type": "points", "points": [[0, 0, 0]], "spacing": 0.1},                          # points are taken as given
                {"name": "x", "type": "points", "points": []}, {"name": "x", "type": "points", "points": [[0, 0, 0]], "carve": -1}):
        c2 = copy.deepcopy(cfg)
        c2["scene"]["geometry"].append(bad)
        with pytest.raises(ValueError):
            geometry.config_groups(c2)
    cfg["scene"]["geometry"] = {"name": "x"}
    with pytest.raises(ValueError):
        geometry.config_groups(cfg)


@pytest.mark.parametrize("name,counts", [("dam_pillars_dfsph", {"pillar_0": 498, "pillar_1": 498, "pillar_2": 498}), ("dam_gate_wcsph", {"gate": 1711}),
                                         ("pbf_step_pbf", {"step": 322})])
def test_shipped_scenes_blocks(name, counts):
    cfg = scenes.get(name)
    assert json.load(open(os.path.join(ROOT, "config", name + ".json"))) == cfg
    groups = geometry.config_groups(cfg)
    assert {n: len(p) for n, p, _ in groups} == counts
    h, box = 4 * cfg["scene"]["particle_radius"], np.array(cfg["scene"]["box_max"])
    lo, size = np.array(cfg["fluid"]["start_pos"]), np.array(cfg["fluid"]["water_size"])
    for n, p, carve in groups:
        assert carve is False
        assert (p > 0).all() and (p < box).all(), n                        # inside the tank, hence inside the grid
        d = np.linalg.norm(p[:, None, :].astype(np.float64) - p[None, :, :], axis=2) + 10 * np.eye(len(p))
        assert d.min(axis=1).max() <= 1.01 * 0.05, n                       # no sample is isolated: every one has a neighbour at the spacing
        inside = ((p > lo - 0.049) & (p < lo + size + 0.049 - 0.05)).all(axis=1)
        assert not inside.any(), "%s stands in the lattice: it would need carving" % n


# ---- the runner ------------------------------------------------------------------------------------------------------------------------------------------
def test_remove_geometry_flag_parsing():
    assert run.parse_remove_geometry(None) == {} and run.parse_remove_geometry([]) == {}
    assert run.parse_remove_geometry(["gate@40", "a@b@7", "lid@40"], known=["gate", "lid", "a@b"]) == {40: ["gate", "lid"], 7: ["a@b"]}
    for bad in (["gate"], ["gate@"], ["@3"], ["gate@-1"], ["gate@x"], ["gate@1", "gate@2"]):
        with pytest.raises(SystemExit):
            run.parse_remove_geometry(bad, known=["gate"])
    with pytest.raises(SystemExit):
        run.parse_remove_geometry(["door@1"], known=["gate"])
    cfg = copy.deepcopy(scenes.get("dam_gate_wcsph"))
    cfg["scene"]["geometry"].append({"name": "cube", "type": "mesh", "mesh": "no/such/file.stl"})
    assert run.geometry_names(cfg) == ["gate", "cube"] and run.geometry_names(scenes.get("dfsph_tiny_wall")) == []      # names alone: nothing is sampled
    assert run.unreached_removals({40: ["gate", "lid"], 7: ["a"]}, 40) == ["gate@40", "lid@40"] and run.unreached_removals({7: ["a"]}, 8) == []


def test_geometry_ply_writer(tmp_path):
    sim = FakeSim(n_box=3)
    sim.add_geometry(gr.BLOCK[:2]); sim.add_geometry(gr.PLATE[:3])
    sim.remove_geometry(1)
    sim.add_geometry(gr.BLOCK[:1])
    path = str(tmp_path / "g.ply")
    run.write_geometry_ply(path, sim)
    head, body = open(path).read().split("end_header\n")
    assert "element vertex 7\n" in head and head.count("property float") == 3 and "property int group\n" in head
    rows = [r.split() for r in body.splitlines()]
    assert [r[3] for r in rows] == ["0", "0", "0", "2", "2", "2", "3"]
    assert np.allclose(np.array([[float(v) for v in r[:3]] for r in rows[3:6]]), gr.PLATE[:3], atol=1e-6)


# ---- names ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_new_names_against_the_header():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sph_mi355x.h")).read(), flags=re.S)
    names = ["sph_geometry_add", "sph_geometry_remove", "sph_geometry_info", "sph_geometry_carve", "sph_geometry_wall_counts"]
    for name in names:
        assert re.search(r"\bint %s\s*\(SphHandle \*h" % name, text), name
        assert name in _native.EXPORTS and name in _native.OPTIONAL_EXPORTS and name not in _native.CORE_EXPORTS
    assert _native.ABI_VERSION == int(re.search(r"#define SPH_ABI_VERSION (\d+)", text).group(1)) == 5      # no struct grew: the version stays
    for method in ("add_geometry", "remove_geometry", "geometry", "carve", "wall_neighbor_counts"):
        assert callable(getattr(_native.Simulation, method))
    from cfd_taichi_amd import slab
    assert callable(slab.SlabSimulation.add_geometry) and callable(slab.SlabSimulation.remove_geometry) and not hasattr(slab.SlabSimulation, "carve")
