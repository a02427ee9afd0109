"""GPU suite: sph_slab_set_state -- a slab handle's owned set replaced from a full state, so that a sharded run can start from (or be moved to)
any state: a fluid settled on one GPU, a user-made initial condition, a run re-started on another number of ranks.

The yardstick (tests/slab_state_worker.py): A = a fresh one-GPU handle given the state with sph_upload + sph_set_scalar(SPH_S_DELTA_TIME),
B = fresh slab handles given the same state with sph_slab_set_state; positions, velocities, densities and the step statistics of B equal A's
bit for bit after every following step.  No tolerance anywhere.  The ranks are handles of one process on the loopback stand-in for the native
transport (one gloo case covers the callback transport), with SPH_SLAB_CHECK=1."""
import os

import pytest

from harness import run_ranks

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_worker(tmp_path, *opts, env_extra=None, timeout=300):
    out = tmp_path / "state.json"
    return run_ranks(os.path.join(ROOT, "tests", "slab_state_worker.py"), ("--out", out) + opts, None, "loopback", out, env_extra, timeout)


def assert_equal_to_one_gpu(r):
    assert r["partition"] and sum(r["owned"]) == r["n"], r
    assert r["roundtrip"] and r["dt_set"], r                                   # what went in is what the handles hold, before any step
    assert r["ghosts_after_set"] == [0] * len(r["owned"]), r
    assert r["first_difference"] is None, r["first_difference"]
    assert r["stats_difference"] is None, r["stats_difference"]


@pytest.mark.parametrize("overlap", [0, 2])
def test_dam_state_recut_every_7_steps(tmp_path, overlap):
    """Case 1: dfsph_dam_x on 3 ranks, state of step 60, 30 steps compared; Morton cells, two ghost columns, re-cuts every 7 steps; in order (0) and
    overlapped (2).  The dam has moved mass along x by step 60: the cuts planned from the state are not the cuts of creation.  (Chunks of 256
    particles: the state goes through the device buffer in four pieces, the last one partly filled.)"""
    r = run_worker(tmp_path, "--scene", "dfsph_dam_x", "--world", 3, "--k", 60, "--m", 30, "--rebalance", 7, "--overlap", overlap,
                   env_extra={"SPH_CELL_ORDER": "morton", "SPH_STATE_CHUNK": "256"})
    assert_equal_to_one_gpu(r)
    assert r["cuts_set"] != r["cuts_created"], r
    assert "SPH_STATE_CHUNK=256" in r["overrides"] and "SPH_CELL_ORDER=morton" in r["overrides"]


@pytest.mark.parametrize("scene,world,k,m,layers", [
    ("dfsph_small", 2, 20, 15, 1),                  # case 2: one ghost column, linear cells
    ("wcsph_small", 2, 40, 20, 0),                  # case 3
    ("dfsph_tiny_wall_pcisph", 2, 15, 10, 0),       # case 4
    ("breaking_dam_30k_iisph", 3, 6, 6, 0)])        # case 5
def test_state_handover_equals_one_gpu(tmp_path, scene, world, k, m, layers):
    assert_equal_to_one_gpu(run_worker(tmp_path, "--scene", scene, "--world", world, "--k", k, "--m", m, "--layers", layers))


def test_replace_mid_run(tmp_path):
    """Case 6: the slab handles have stepped 10 times from rest -- ghosts resident, stamps set, cuts moved -- when they get the state of step 60."""
    r = run_worker(tmp_path, "--scene", "dfsph_dam_x", "--world", 3, "--k", 60, "--m", 20, "--rebalance", 7, "--prestep", 10,
                   env_extra={"SPH_CELL_ORDER": "morton"})
    assert sum(r["ghosts_before"]) > 0, r
    assert_equal_to_one_gpu(r)


def test_state_far_from_the_lattice(tmp_path):
    """Case 7: every x mirrored (x' = box_min.x + box_max.x - x): all fluid sits where the cuts of creation put nearly nothing."""
    r = run_worker(tmp_path, "--scene", "dfsph_small", "--world", 3, "--k", 20, "--m", 10, "--mirror")
    assert_equal_to_one_gpu(r)
    assert r["cuts_set"] != r["cuts_created"], r


def test_round_trip(tmp_path):
    """Case 8: set_state, then the state read back before any step, is the input bit for bit (random velocities and scalars; chunks of 1000 -> 1024
    particles, five full ones and a remainder); NULL velocities / scalars are zeros."""
    r = run_worker(tmp_path, "--mode", "roundtrip", "--scene", "dfsph_small", "--world", 3, "--k", 20, env_extra={"SPH_STATE_CHUNK": "1000"})
    assert r["partition"] and r["equal"] == [True, True, True] and r["null_is_zero"] and sum(r["owned"]) == r["n"], r
    assert "SPH_STATE_CHUNK=1000" in r["overrides"]


def test_refusals_leave_every_handle_untouched(tmp_path):
    """Case 9: a NaN position, a position outside the box, a wrong n_fluid, a scalar on a wcsph handle, a handle with a body, one rank without the
    capacity: every rank returns the same code at the same call (none hangs: the timeout), the handles are exactly what they were, and five more
    steps equal a twin run that was never asked."""
    r = run_worker(tmp_path, "--mode", "refuse", timeout=300)
    assert sorted(r) == ["capacity:one_rank", "dfsph:nan", "dfsph:outside", "dfsph:wrong_n", "rigid:body", "wcsph:scalar"], sorted(r)
    for name, v in r.items():
        assert v["codes"] == v["want"] and v["untouched"] and v["steps_equal_twin"], (name, v)


def test_set_state_over_torch_distributed(tmp_path):
    """Case 10: SlabSimulation.set_state(..., src=0) -- rank 0's arrays broadcast through torch.distributed (gloo), the callback transport."""
    out = tmp_path / "gloo.json"
    r = run_ranks(os.path.join(ROOT, "tests", "slab_state_gloo_worker.py"), ("--scene", "dfsph_small", "--state-steps", 20, "--steps", 10, "--out", out), 2, "gloo", out)
    assert r["roundtrip"] and r["first_difference"] is None and r["stats_difference"] is None and r["state_dt"], r
