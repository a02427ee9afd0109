"""Static geometry on slab handles: the walls are replicated, sph_geometry_add / sph_geometry_remove are plain local calls
every rank makes alike between the same steps, and the sharded run is bit-identical to the one-GPU handle with the same geometry -- gathered pos,
vel and rho and every rank's statistics after every step (tests/slab_geometry_worker.py, over the loopback stand-in for librccl).  Carving is
refused with SPH_E_STATE on every rank.

Scene: the long tank of the sharded-PBF tests (1 151 particles in 15 of 21 cell columns, so two and three slabs all hold fluid) with a plate
beside the whole column and a block above it; the worker also steps a handle without geometry, so that a geometry nobody feels cannot pass."""
import copy
import json
import os

import pytest

import slab_pbf_states as sp
from cfd_taichi_amd import _native as nat
from harness import run_ranks

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "slab_geometry_worker.py")
DT = {"dfsph": 1e-3, "pbf": 2.5e-4}


def long_tank(solver):
    cfg = copy.deepcopy(sp.config("long_wall"))
    cfg["solver"]["name"] = solver
    cfg["solver"]["delta_time"] = DT[solver]
    return cfg


def run_worker(tmp_path, cfg, world, steps, remove_after=0):
    scene = tmp_path / "scene.json"
    scene.write_text(json.dumps(cfg))
    out = tmp_path / "out.json"
    return run_ranks(WORKER, ["--scene", scene, "--world", world, "--steps", steps, "--remove-after", remove_after, "--out", out], world, "loopback", out)


def check(r, world, removed):
    assert r["world"] == world and r["n"] == sp.N_LONG and r["finite"]
    assert r["groups"] == [[1, 2]] * (world + 1) and r["walls_equal"]
    assert r["carve_codes"] == [nat.SPH_E_STATE] * world and r["count_codes"] == [nat.SPH_E_STATE] * world, (r["carve_codes"], r["count_codes"])
    assert r["first_difference"] is None, r["first_difference"]
    assert r["stats_equal"]
    assert r["rows_felt"] > 100, r["rows_felt"]
    assert len(set(r["n_wall"])) == 1 and all(g == r["geometry"][-1] for g in r["geometry"])
    assert [g[0] for g in r["geometry"][-1]] == ([2] if removed else [1, 2])
    assert sum(s["owned"] for s in r["slabs"]) == r["n"] and all(s["owned"] > 0 for s in r["slabs"]), r["slabs"]
    assert all(any(o.startswith("SPH_RCCL_LIB=") for o in ov) for ov in r["overrides"])


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("solver", ["dfsph", "pbf"])
def test_plate_and_block_on_slabs(tmp_path, solver, world):
    check(run_worker(tmp_path, long_tank(solver), world, 5), world, removed=False)


def test_plate_removed_after_step_3_on_slabs(tmp_path):
    check(run_worker(tmp_path, long_tank("dfsph"), 2, 5, remove_after=3), 2, removed=True)
