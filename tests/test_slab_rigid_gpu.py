"""A two-way coupled rigid body on slab handles of wcsph, pcisph and iisph (one ghost column): bit-identical to the one-GPU run, as dfsph's is
(tests/test_slab_gpu.py::test_rigid_body_on_slabs).  The body is replicated on every rank; a sample's force is summed whole by the rank that owns the
sample's cell column, from fluid operands that are the owners' values on the ghost column too; the fluid positions and densities the reference's
index quirks read and the per-sample forces go through the transport's reduce buffer.

Scene: the geometry of dfsph_rigid_small (5 760 fluid particles in cell columns 1-6, a body of 594 samples, 0.4 x 0.25 x 0.5) with the body moved
over the water: across the cuts of 2 and 3 ranks and 0.03 above the top fluid layer (y = 1.05), so that it is coupled from step 1.  The fluid at
rest has rho < rho_0 (the reference's density has no self term: 680-890 here) and every solver clamps such a pressure to zero, so a body 0.07 above
the water feels no force in the first step (the CPU oracle says so for all three solvers); at 0.03 the samples' own density terms lift the top layer
above rho_0.  A tilted, lighter twin (its lowest edge 0.03 above the water, samples in columns 1-7) rotates.
Every comparison is bit for bit against the one-GPU handle, which tests/test_rigid_gpu.py holds to the oracle for these solvers."""
import copy
import json
import os

import pytest

from cfd_taichi_amd import _native as nat
from cfd_taichi_amd import scenes
from harness import run_ranks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "slab_rigid_worker.py")
DT = {"wcsph": 2.5e-4, "pcisph": 1e-3, "iisph": 1e-3}


def scene_config(solver, tilted=False):
    cfg = copy.deepcopy(scenes.get("dfsph_rigid_small"))
    cfg["solver"]["name"] = solver
    cfg["solver"]["delta_time"] = DT[solver]
    cfg["solid"]["pos_offset"] = [0.2, 1.08, 0.5]
    if tilted:
        cfg["solid"]["pos_offset"] = [0.45, 1.08, 0.5]
        cfg["solid"]["attitude_offset"] = [20.0, 0.0, 35.0]
        cfg["solid"]["rho_0"] = 500
    return cfg


def write_scene(tmp_path, solver, tilted):
    path = tmp_path / ("%s_rigid_over_water%s.json" % (solver, "_tilted" if tilted else ""))
    path.write_text(json.dumps(scene_config(solver, tilted)))
    return str(path)


def run_worker(tmp_path, transport, solver, tilted, world, steps, rebalance, env_extra=None):
    out = tmp_path / ("rigid_%s_%s_%d_%d.json" % (transport, solver, world, rebalance))
    args = ["--scene", write_scene(tmp_path, solver, tilted), "--transport", transport, "--world", world, "--steps", steps, "--rebalance", rebalance, "--out", out]
    return run_ranks(WORKER, args, world, transport, out, env_extra)


def check(r, world, solver, rebalance, tilted=False):
    print({k: r[k] for k in ("cols_first", "cols_last", "owned_samples_first", "owned_samples_last", "force_first_max", "force_first_ranks", "stats_last",
                             "ref_stats_last", "body_centroid", "body_omega", "delta", "ref_delta")})
    # the scene's conditions: the body lies across a cut at the first and at the last step, and is coupled before its first step
    assert r["samples_equal_first"] and r["samples_equal_last"]
    assert sum(r["owned_samples_first"]) == r["n_samples"] == sum(r["owned_samples_last"]), r
    assert sum(1 for k in r["owned_samples_first"] if k > 0) >= 2, (r["cols_first"], r["owned_samples_first"])
    assert sum(1 for k in r["owned_samples_last"] if k > 0) >= 2, (r["cols_last"], r["owned_samples_last"])
    assert r["force_first_max"] > 0.0
    # ... and what every rank summed for its own samples is the one-GPU force (x + 0 = x); the level body's underside spans the cuts, so more than
    # one rank contributes (the tilted one touches the water with one edge)
    assert r["force_first_equal"] and sum(1 for k in r["force_first_ranks"] if k > 0) >= (1 if tilted else 2), r["force_first_ranks"]
    assert r["pos_equal"] and r["vel_equal"] and r["rho_equal"], r
    assert r["stats_equal"] and r["stats_same_on_all_ranks"], (r["stats_last"], r["ref_stats_last"])
    assert len(r["body_equal"]) == world and all(r["body_equal"]), (r["body_equal"], r["body_centroid"], r["body_omega"])
    assert sum(s["owned"] for s in r["slabs"]) == r["n"]
    assert all(s["ghost_columns"] == 1 for s in r["slabs"])
    if rebalance:
        assert all(s["rebalance_every"] == rebalance for s in r["slabs"])
    if solver == "pcisph":
        assert r["delta"] == [r["ref_delta"]] * world and r["ref_delta"] > 0.0, (r["delta"], r["ref_delta"])


@pytest.mark.gpu
@pytest.mark.parametrize("solver,tilted,world,steps,rebalance,order", [
    ("wcsph", False, 2, 40, 0, None), ("pcisph", False, 2, 12, 0, None), ("iisph", False, 3, 12, 5, None),
    ("pcisph", True, 3, 12, 5, "morton"), ("wcsph", True, 3, 40, 9, None)])
def test_rigid_body_on_slabs_of_the_other_solvers(tmp_path, solver, tilted, world, steps, rebalance, order):
    """Ranks sharing one GPU over gloo, through SlabSimulation.step (which follows every solver step with one body step, for wcsph too): fluid positions,
    velocities and densities, iteration counts / residuals / dt, the body's centroid, omega, velocity, inertia and every sample position on every
    rank, the owned counts; with re-cuts, and on the Morton curve (a slab handle's own cell slots, staged sweeps)."""
    r = run_worker(tmp_path, "gloo", solver, tilted, world, steps, rebalance, env_extra={"SPH_CELL_ORDER": order} if order else None)
    check(r, world, solver, rebalance, tilted)
    if tilted:
        assert any(abs(v) > 1e-4 for v in r["body_omega"]), r["body_omega"]


@pytest.mark.gpu
@pytest.mark.parametrize("solver,world,steps,rebalance", [("pcisph", 2, 12, 0), ("iisph", 3, 12, 0), ("wcsph", 3, 40, 9)])
def test_rigid_body_on_the_native_transport(tmp_path, solver, world, steps, rebalance):
    """The library's native transport on the loopback stand-in (tests/test_slab_gpu.py::run_loopback's pattern): no host wait between the sweeps, the
    pressure loop's (sum, count, flags) gathered in the refresh's own group of transfers -- a force kernel that read a ghost's pressure before its
    refresh would show here."""
    r = run_worker(tmp_path, "loopback", solver, False, world, steps, rebalance)
    check(r, world, solver, rebalance)
    assert all(any(o.startswith("SPH_RCCL_LIB=") for o in ov) for ov in r["overrides"])


def rigid_struct(active=1):
    import ctypes
    import numpy as np
    pts = np.zeros((4, 3), dtype=np.float32)
    rg = nat.SphRigid()
    rg.n_particles, rg.n_vertices = len(pts), 0
    rg.points, rg.vertices = pts.ctypes.data, None
    rg.rho_0 = 1000.0
    rg.active = active
    return rg, pts, ctypes


@pytest.mark.parametrize("solver,layers,fs_couple,message", [
    ("pbf", 0, 1, "pbf has no rigid coupling"),
    ("wcsph", 0, 0, "a one-way rigid body (active, fs_couple 0) is not supported on slab handles"),
    ("pcisph", 0, 0, "a one-way rigid body (active, fs_couple 0) is not supported on slab handles"),
    ("dfsph", 1, 1, "a rigid body on slab handles needs dfsph with two ghost columns")])
def test_refusals_that_remain(solver, layers, fs_couple, message):
    """sph_create_rigid on a slab handle still refuses pbf, a one-way body and dfsph with one ghost column: SPH_E_INVALID with the message, before
    any device call (so this runs without a GPU)."""
    lib = nat.load()
    cfg = nat.config_from_dict(scene_config("wcsph"), solver_name=solver, slab_rank=0, slab_count=2, slab_ghost_layers=layers)
    cfg.fs_couple = fs_couple
    rg, pts, ctypes = rigid_struct()
    handle = ctypes.c_void_p()
    rc = lib.sph_create_rigid(ctypes.byref(cfg), ctypes.byref(rg), ctypes.byref(handle))
    assert rc == nat.SPH_E_INVALID and not handle.value
    assert message in (lib.sph_last_error(None) or b"").decode()
