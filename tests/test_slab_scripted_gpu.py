"""A scripted or fixed rigid body on slab handles: bit-identical to the one-GPU handle in the same mode.  The body is replicated; the mode and the
motion are plain local calls every rank makes alike, sph_rigid_step keeps its all-reduce of the per-sample forces in every mode, so the load
(sph_rigid_get_load) is the whole body's on every rank.

Scene: the geometry of tests/test_slab_rigid_gpu.py (dfsph_rigid_small with the body 0.03 above the water, coupled from step 1).  The scripted body
starts at x = 0.245 -- its sample planes at 0.245, 0.295, ..., 0.645, the plane at 0.395 just left of the cut between cell columns 3 and 4 that 2 and
3 ranks make at t = 0 (x = 0.4) -- and moves in +x at 1.5 m/s: that plane changes its owning rank after 0.005 of travel, within every window here
(0.01 s of wcsph, 0.012 s of the others).  The worker reports the owned sample counts at the first and at the last step; they must differ."""
import copy
import json
import os

import pytest

from harness import run_ranks
from test_slab_rigid_gpu import scene_config

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "slab_scripted_worker.py")
VEL = [1.5, 0.0, 0.0]


def scripted_scene(solver, mode):
    if solver == "dfsph":
        from cfd_taichi_amd import scenes
        cfg = copy.deepcopy(scenes.get("dfsph_rigid_small"))
        cfg["solid"]["pos_offset"] = [0.2, 1.08, 0.5]
    else:
        cfg = scene_config(solver)
    if mode == "scripted":
        cfg["solid"]["pos_offset"] = [0.245, 1.08, 0.5]
    return cfg


def run_worker(tmp_path, transport, solver, mode, world, steps, rebalance):
    scene = tmp_path / ("%s_%s_body.json" % (solver, mode))
    scene.write_text(json.dumps(scripted_scene(solver, mode)))
    out = tmp_path / ("scripted_%s_%s_%d.json" % (transport, solver, world))
    args = ["--scene", scene, "--transport", transport, "--world", world, "--steps", steps, "--rebalance", rebalance, "--mode", mode, "--vel"] + VEL + ["--out", out]
    return run_ranks(WORKER, args, world, transport, out)


def check(r, world, mode):
    print({k: r[k] for k in ("cols_first", "cols_last", "owned_samples_first", "owned_samples_last", "load_first_max", "load_max", "body_moved",
                             "body_centroid", "stats_last", "ref_stats_last")})
    assert r["mode"] == {"scripted": 1, "fixed": 2}[mode] and r["finite"]
    assert r["samples_equal_first"] and r["samples_equal_last"]
    assert sum(r["owned_samples_first"]) == r["n_samples"] == sum(r["owned_samples_last"]), r
    assert sum(1 for k in r["owned_samples_first"] if k > 0) >= 2, (r["cols_first"], r["owned_samples_first"])
    assert r["load_first_max"] > 0.0 and r["load_max"] > 0.0, "the fluid never pushed the body"
    assert r["pos_equal"] and r["vel_equal"] and r["rho_equal"], r
    assert len(r["stats_equal"]) == world and all(r["stats_equal"]), (r["stats_last"], r["ref_stats_last"])
    assert len(r["body_equal"]) == world and all(r["body_equal"]), r["body_equal"]
    assert len(r["loads_equal"]) == world and all(r["loads_equal"]), r["loads_equal"]
    assert sum(s["owned"] for s in r["slabs"]) == r["n"]
    if mode == "scripted":
        assert r["owned_samples_first"] != r["owned_samples_last"], "no sample changed its owning rank: %s" % r["owned_samples_first"]
        assert r["body_moved"] > 0.005
    else:
        assert r["body_moved"] == 0.0


@pytest.mark.parametrize("transport,solver,world,steps,rebalance", [("gloo", "wcsph", 2, 40, 0), ("gloo", "dfsph", 3, 12, 5), ("loopback", "pcisph", 2, 12, 0)])
def test_scripted_body_on_slabs(tmp_path, transport, solver, world, steps, rebalance):
    """wcsph on 2 ranks over gloo; dfsph on 3 ranks with its two ghost columns and re-cuts every 5 steps; pcisph on 2 ranks on the native transport
    (the loopback stand-in): fluid fields, step stats on every rank, the body on every rank, the load after every body step on every rank"""
    r = run_worker(tmp_path, transport, solver, "scripted", world, steps, rebalance)
    check(r, world, "scripted")
    if solver == "dfsph":
        assert all(s["ghost_columns"] == 2 and s["rebalance_every"] == rebalance for s in r["slabs"]), r["slabs"]
    if transport == "loopback":
        assert all(any(o.startswith("SPH_RCCL_LIB=") for o in ov) for ov in r["overrides"])


def test_fixed_obstacle_on_slabs(tmp_path):
    """iisph on 3 ranks: the obstacle across the cuts never moves, and every rank reads the whole body's load"""
    r = run_worker(tmp_path, "gloo", "iisph", "fixed", 3, 12, 0)
    check(r, 3, "fixed")
