"""Gravity as a vector under harmonic forcing on slab handles: the set calls are plain local calls every rank makes alike, every rank forms the
vector itself (the same kernel on the same clock), and the sharded run is bit-identical to the one-GPU handle -- gathered pos and vel, and
SPH_S_TIME and SPH_S_ACCEL on every rank, after every step (tests/slab_forcing_worker.py, over the loopback stand-in for librccl).

Scenes: the long tank of the sharded-PBF tests (1 151 particles in 15 of 21 cell columns, so two and three slabs all hold fluid) with the solver
switched; the coupled case is the body over the water of tests/test_slab_scripted_gpu.py on dfsph, a DYNAMIC body that reads the vector."""
import copy
import json
import os

import pytest

from cfd_taichi_amd import scenes
import slab_pbf_states as sp
from harness import run_ranks

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "slab_forcing_worker.py")
DT = {"dfsph": 1e-3, "wcsph": 2.5e-4, "pbf": 2.5e-4}


def long_tank(solver):
    cfg = copy.deepcopy(sp.config("long_wall"))
    cfg["solver"]["name"] = solver
    cfg["solver"]["delta_time"] = DT[solver]
    return cfg


def body_over_water():
    """dfsph_rigid_small with the body 0.03 above the water, coupled from step 1 (the dfsph scene of tests/test_slab_scripted_gpu.py)"""
    cfg = copy.deepcopy(scenes.get("dfsph_rigid_small"))
    cfg["solid"]["pos_offset"] = [0.2, 1.08, 0.5]
    return cfg


def run_worker(tmp_path, cfg, world, steps, body=False):
    scene = tmp_path / "scene.json"
    scene.write_text(json.dumps(cfg))
    out = tmp_path / "out.json"
    args = ["--scene", scene, "--world", world, "--steps", steps, "--out", out] + (["--body"] if body else [])
    return run_ranks(WORKER, args, world, "loopback", out)


def check(r, world):
    assert r["world"] == world and r["finite"] and r["clock_start_equal"]
    assert r["first_difference"] is None, r["first_difference"]
    assert r["stats_equal"]
    assert r["time"] > 0.0
    assert len({tuple(v) for v in r["vectors"]}) == len(r["vectors"]), "the vector did not change from step to step"
    assert sum(s["owned"] for s in r["slabs"]) == r["n"] and all(s["owned"] > 0 for s in r["slabs"]), r["slabs"]
    assert all(any(o.startswith("SPH_RCCL_LIB=") for o in ov) for ov in r["overrides"])


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("solver", ["dfsph", "wcsph", "pbf"])
def test_harmonic_forcing_on_slabs(tmp_path, solver, world):
    r = run_worker(tmp_path, long_tank(solver), world, 10)
    assert r["n"] == sp.N_LONG
    check(r, world)


def test_dynamic_body_under_forcing_on_slabs(tmp_path):
    r = run_worker(tmp_path, body_over_water(), 2, 10, body=True)
    check(r, 2)
    assert abs(r["body_vel"][0]) > 0 and abs(r["body_vel"][2]) > 0, r["body_vel"]
