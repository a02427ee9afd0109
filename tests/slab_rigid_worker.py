"""Worker of tests/test_slab_rigid_gpu.py: a two-way coupled rigid body on slab handles of wcsph / pcisph / iisph against the same steps on a one-GPU
handle, bit for bit.  Two transports (tests/slab_ranks.py: body_ranks runs this worker's run_rank and compare on either):

  --transport gloo      one process per rank under torch.distributed.run, all on GPU 0, SlabSimulation + TorchComm (as tests/slab_worker.py)
  --transport loopback  the library's native transport on tests/loopback_rccl.hip, one thread per rank in this process (as tests/loopback_worker.py)

Beyond what those two workers report: the force on the body BEFORE the first body step (every rank's own array -- a sample's force is summed whole
by the rank that owns its cell column, the others leave zeros -- added up and compared with the one-GPU force), the x coordinates of the samples and
every slab's owned columns at the first and at the last solver step, and pcisph's delta on every handle."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from slab_ranks import body_ranks, owned_samples, stat_row  # noqa: E402


def body_of(sim, nat):
    return {"scalars": sim.rigid_scalars(), "pos": sim.download(nat.F_RIGID_POS, nat.SPECIES_RIGID).tolist()}


def run_rank(nat, native, steps, step_rest):
    """One rank's (or the one-GPU handle's) run.  native: its nat.Simulation; step_rest(): one solver step + one body step after the first."""
    rep = {"delta": native.scalar(nat.S_PCISPH_DELTA), "stats": []}
    for k in range(steps):
        if k in (0, steps - 1):       # the solver step and the body step apart: what the force kernels saw, what they left
            sample_x = native.download(nat.F_RIGID_POS, nat.SPECIES_RIGID)[:, 0].copy()
            st = native.step(1)
            info = native.slab_info()
            tag = "first" if k == 0 else "last"
            rep["sample_x_" + tag] = sample_x
            rep["cols_" + tag] = [info["x_lo"], info["x_hi"]]
            if k == 0:
                rep["force_first"] = native.download(nat.F_RIGID_FORCE, nat.SPECIES_RIGID)
            native.rigid_step()
        else:
            st = step_rest()
        row = stat_row(st)
        if row is not None:
            rep["stats"].append(row)
    rep["info"] = native.slab_info()
    rep["body"] = body_of(native, nat)
    return rep


def compare(nat, cfg, rigid, steps, reps, fields):
    """reps: every rank's report; fields: the gathered (pos, vel, rho).  Runs the one-GPU twin and returns the result dictionary."""
    ref = nat.Simulation(nat.config_from_dict(cfg), rigid=rigid)
    h = np.float32(ref.scalar(nat.S_SUPPORT_RADIUS))

    def ref_rest():
        st = ref.step(1)
        ref.rigid_step()
        return st
    rr = run_rank(nat, ref, steps, ref_rest)
    rp, rv, rrho = ref.download(nat.F_POS), ref.download(nat.F_VEL), ref.download(nat.F_RHO)
    ref.close()
    pos, vel, rho = fields
    force_sum = np.zeros_like(rr["force_first"], dtype=np.float64)
    for r in reps:
        force_sum += r["force_first"]

    def owners(tag):       # how many samples lie in each rank's owned columns, from the samples' x, the cell edge and the slabs' x_lo / x_hi
        return [owned_samples(r["sample_x_" + tag], h, r["cols_" + tag]) for r in reps]
    return {
        "n": int(len(rp)), "steps": steps, "slabs": [r["info"] for r in reps],
        "pos_equal": bool(np.array_equal(pos, rp)), "vel_equal": bool(np.array_equal(vel, rv)), "rho_equal": bool(np.array_equal(rho, rrho)),
        "stats_equal": reps[0]["stats"] == rr["stats"], "stats_same_on_all_ranks": all(r["stats"] == reps[0]["stats"] for r in reps),
        "stats_last": reps[0]["stats"][-1] if reps[0]["stats"] else None, "ref_stats_last": rr["stats"][-1] if rr["stats"] else None,
        "body_equal": [r["body"] == rr["body"] for r in reps], "body_centroid": rr["body"]["scalars"]["centroid"], "body_omega": rr["body"]["scalars"]["omega"],
        "samples_equal_first": all(np.array_equal(r["sample_x_first"], rr["sample_x_first"]) for r in reps),
        "samples_equal_last": all(np.array_equal(r["sample_x_last"], rr["sample_x_last"]) for r in reps),
        "owned_samples_first": owners("first"), "owned_samples_last": owners("last"), "n_samples": int(len(rr["sample_x_first"])),
        "cols_first": [r["cols_first"] for r in reps], "cols_last": [r["cols_last"] for r in reps],
        "force_first_max": float(np.abs(rr["force_first"]).max()), "force_first_equal": bool(np.array_equal(force_sum.astype(np.float32), rr["force_first"])),
        "force_first_ranks": [int(np.count_nonzero(np.abs(r["force_first"]).sum(axis=1))) for r in reps],
        "delta": [r["delta"] for r in reps], "ref_delta": rr["delta"],
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", required=True, help="path to a config JSON with a `solid` block")
    ap.add_argument("--transport", choices=("gloo", "loopback"), required=True)
    ap.add_argument("--world", type=int, default=2, help="loopback: the number of ranks (gloo: WORLD_SIZE)")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rebalance", type=int, default=0)
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    assert args.steps >= 2
    cfg = json.load(open(args.scene))
    from cfd_taichi_amd import mesh
    rigid = mesh.rigid_from_config(cfg)
    body_ranks(args, cfg, rigid, lambda nat, native, full_step: run_rank(nat, native, args.steps, full_step),
               lambda nat, reps, fields: compare(nat, cfg, rigid, args.steps, reps, fields))


if __name__ == "__main__":
    main()
