"""GPU suite: pbf_solver on x-slab handles -- a PBF run sharded over 2-4 slabs gives, bit for bit, what the one-GPU handle gives (and therefore what
the oracle gives): pos, vel, rho, pbf_lambda and delta_pos of the owned particles, gathered by particle id, as raw f32; no tolerance anywhere.

Per step a slab handle refreshes lambda of its ghosts after the lambda sweep and their new position / phase-1 velocity (one message) after the
delta_pos sweep; k_pbf_xsph_slab keeps the ghosts out of the 27-cell walk (csrc/sph_host_pressure.h: step_pbf_once).  The inputs load that path:
tests/slab_pbf_states.py, shown fair on the oracle alone by tests/test_slab_pbf_cpu.py -- ~20 particles cross every column boundary in the 60
steps and lambda is nonzero on ~40 % of the particles.  The ranks are processes over gloo (the callback transport) or slab handles of one process on
the loopback stand-in for the native transport (tests/slab_pbf_worker.py), every subprocess under its own timeout, at most 4 ranks, no retries.

On the comm identities of case 2 / 3: an ordinary step exchanges particles in one round and a re-cut step in two -- and so does the first step
after sph_slab_set_state (include/sph_mi355x.h), which is how the state gets in and is no re-cut.  The identities the issue states per step
(count_exchanges == steps + recuts, p2p_groups - recuts == 3 steps) are therefore asserted over steps 2 .. 60, and over the whole run with that
one extra round named."""
import os

import numpy as np
import pytest

import slab_pbf_states as sp
from harness import run_ranks

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "slab_pbf_worker.py")
E_INVALID, E_OVERFLOW, E_STATE = -1, -4, -5


def state_file(tmp_path, scene, seed):
    pos, vel = sp.state(scene, seed)
    path = tmp_path / ("state_%s_%d.npz" % (scene, seed))
    np.savez(path, pos=pos, vel=vel)
    return str(path)


def run_loopback(tmp_path, *opts, env_extra=None, timeout=240):
    out = tmp_path / "pbf.json"
    return run_ranks(WORKER, ("--transport", "loopback", "--out", out) + opts, None, "loopback", out, env_extra, timeout)


def run_gloo(tmp_path, world, *opts, timeout=300):
    out = tmp_path / "pbf_gloo.json"
    return run_ranks(WORKER, ("--transport", "gloo", "--out", out) + opts, world, "gloo", out, timeout=timeout)


def assert_comm_identities(r, steps):
    assert max(s["recuts"] for s in r["slabs"]) >= 1, r["slabs"]
    for w in r["comm_after_step_1"]:                           # steps 2 .. steps: ordinary and re-cut steps
        assert w["steps"] == steps - 1, w
        assert w["count_exchanges"] == w["steps"] + w["recuts"], w
        assert w["p2p_groups"] - w["recuts"] == 3 * w["steps"], w
        assert w["allreduce_stream"] == 0, w
    for w in r["comm_whole_run"]:                              # ... and with the two-round first step after sph_slab_set_state
        assert w["steps"] == steps, w
        assert w["count_exchanges"] == w["steps"] + w["recuts"] + 1, w
        assert w["p2p_groups"] - w["recuts"] - 1 == 3 * w["steps"], w
        assert w["allreduce_stream"] == 0, w


def test_two_slabs_over_gloo_equal_one_gpu_and_the_oracle(tmp_path):
    """Case 1: long_wall, seed 1, 2 ranks over gloo, static cuts, linear cells, 60 steps.  Sharded == one GPU after every step; == the f32 oracle
    after the last; the owned counts sum to N at every step; >= 15 particles changed owner; both slabs hold ghosts; SlabSimulation.step returns
    None and state() round-trips with scalar None."""
    dump = tmp_path / "sharded.npz"
    r = run_gloo(tmp_path, 2, "--scene", "long_wall", "--state", state_file(tmp_path, "long_wall", 1), "--steps", sp.STEPS, "--dump", dump)
    assert r["first_difference"] is None, r["first_difference"]
    assert r["n"] == sp.N_LONG and r["owned_sums"] == [sp.N_LONG] * sp.STEPS, r["owned_sums"]
    assert r["owner_changes"] >= 15, r["owner_changes"]
    assert min(r["ghosts_max"]) > 0, r["ghosts_max"]
    assert r["step_returns_none"] and r["state_round_trip"], r
    assert [s["ghost_columns"] for s in r["slabs"]] == [1, 1], r["slabs"]
    assert all(w["allreduce_stream"] == 0 and w["p2p_groups"] == 3 * sp.STEPS + 1 for w in r["comm_whole_run"]), r["comm_whole_run"]
    want = sp.oracle_run("long_wall", 1)[sp.STEPS]
    got = np.load(dump)
    for name, _ in sp.FIELDS:
        assert np.array_equal(got[name], want[name]), (name, int((got[name] != want[name]).sum()))


def test_four_slabs_native_transport_recuts_morton(tmp_path):
    """Case 2: long_clamp, seed 3, 4 ranks on the loopback native transport, re-cuts every 7 steps, cells on the Morton curve."""
    r = run_loopback(tmp_path, "--scene", "long_clamp", "--state", state_file(tmp_path, "long_clamp", 3), "--world", 4, "--steps", sp.STEPS,
                     "--rebalance", 7, env_extra={"SPH_CELL_ORDER": "morton"})
    assert r["first_difference"] is None, r["first_difference"]
    assert r["owned_sums"] == [sp.N_LONG] * sp.STEPS, r["owned_sums"]
    assert "SPH_CELL_ORDER=morton" in r["overrides"], r["overrides"]
    assert r["relaxed"] == [0.0] * 5, r["relaxed"]
    assert_comm_identities(r, sp.STEPS)


def test_three_slabs_relaxed_arithmetic(tmp_path):
    """Case 3: the same with arith = relaxed on 3 ranks: the sharded relaxed run equals the one-GPU relaxed run bit for bit.  (At 1151 particles
    the one-GPU handle walks its lists quad-wide, which under the relaxed bodies' fma accumulation rounds differently from a plain one-lane walk --
    19 positions were one ulp off at the first compared step that differed, before the slab handles took the quad walk's additions, csrc/sph_pbf_kernels.h: QSUM.)"""
    r = run_loopback(tmp_path, "--scene", "long_clamp", "--state", state_file(tmp_path, "long_clamp", 3), "--world", 3, "--steps", sp.STEPS,
                     "--rebalance", 7, "--arith", 1, env_extra={"SPH_CELL_ORDER": "morton"})
    assert r["first_difference"] is None, r["first_difference"]
    assert r["owned_sums"] == [sp.N_LONG] * sp.STEPS, r["owned_sums"]
    assert r["relaxed"] == [1.0] * 4, r["relaxed"]
    assert_comm_identities(r, sp.STEPS)


def test_the_30k_dam_from_rest_over_gloo(tmp_path):
    """Case 4: breaking_dam_30k_pbf from rest, 4 ranks over gloo, 10 steps -- the size the reference ships; an unloaded halo."""
    r = run_gloo(tmp_path, 4, "--scene", "breaking_dam_30k_pbf", "--steps", 10, "--final-only")
    assert r["first_difference"] is None, r["first_difference"]
    assert r["owned_sums"] == [r["n"]] * 10 and r["n"] > 25000, r
    assert all(w["p2p_groups"] == 30 and w["allreduce_stream"] == 0 for w in r["comm_whole_run"]), r["comm_whole_run"]


def test_state_of_three_slabs_into_two(tmp_path):
    """Case 5: long_wall on 3 ranks, 20 steps, state() into set_state() of a fresh group of 2 ranks, 20 more: 40 uninterrupted one-GPU steps.  A scalar
    is refused with SPH_E_INVALID on every rank and leaves the handles usable; pbf_lambda is "before the first step" after every set_state."""
    r = run_loopback(tmp_path, "--mode", "roundtrip", "--scene", "long_wall", "--state", state_file(tmp_path, "long_wall", 1), "--world", 3, "--steps", 20)
    assert r["state_equal_one_gpu"], r
    assert r["scalar_refused"] == [E_INVALID] * 3, r
    assert r["first_difference"] is None, r["first_difference"]
    assert r["refused_group_runs_on"] is None, r["refused_group_runs_on"]
    assert sum(r["owned_after_set"]) == sp.N_LONG, r
    assert r["lambda_before_first_step"] == [E_STATE] * 3 and r["lambda_after_set_state"] == [E_STATE] * 2 and r["lambda_after_set_state_mid_run"] == [E_STATE] * 3, r


def test_density_and_list_builds_between_steps(tmp_path):
    """Case 6: long_wall on 2 ranks; between steps 10 and 11 every rank calls sph_compute_density, then sph_build_neighbors twice.  rho of the owned
    particles is the one-GPU handle's; the trajectory through step 30 is unchanged; pbf_lambda / delta_pos are not carried through a slab handle's
    re-sort (their device order is gone and the resident set has changed): SPH_E_STATE until step 11 has run."""
    r = run_loopback(tmp_path, "--mode", "midrun", "--scene", "long_wall", "--state", state_file(tmp_path, "long_wall", 1), "--world", 2, "--steps", 30,
                     "--at", 10)
    assert r["first_difference"] is None, r["first_difference"]
    assert r["rho_after_compute_density"] and r["state_after_build"] and r["owned_after_build"] == sp.N_LONG, r
    assert r["lambda_after_compute_density"] == [E_STATE] * 2 and r["lambda_after_build"] == [E_STATE] * 2 and r["delta_pos_after_build"] == [E_STATE] * 2, r
    assert r["lambda_after_next_step"] == [0, 0], r


def test_a_list_overflow_on_one_slab_fails_every_slab(tmp_path):
    """Case 7: rank 1 of 3 gets neighbour lists of 12 rows: every rank's sph_step_pbf returns SPH_E_OVERFLOW, none hangs (the timeout)."""
    r = run_loopback(tmp_path, "--mode", "overflow", "--scene", "long_wall", "--state", state_file(tmp_path, "long_wall", 1), "--world", 3,
                     "--overflow-rank", 1, "--max-neighbors", 12, timeout=120)
    assert r["codes"] == [E_OVERFLOW] * 3, r
