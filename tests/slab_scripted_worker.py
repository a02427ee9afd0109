"""Worker of tests/test_slab_scripted_gpu.py: a scripted or fixed rigid body (sph_rigid_set_mode / sph_rigid_set_motion) on slab handles against
the same calls on a one-GPU handle, bit for bit.  Transports and layout as tests/slab_rigid_worker.py (gloo: one process per rank under
torch.distributed.run, SlabSimulation + TorchComm; loopback: the native transport on tests/loopback_rccl.hip, one thread per rank).

Every rank makes the same mode / motion calls before its first step.  Reported beyond slab_rigid_worker: the load (sph_rigid_get_load) after every
body step on every rank, as the bytes of its six doubles, and the owned sample counts at the first and at the last step."""
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
    return {"scalars": sim.rigid_scalars(motion=True), "pos": sim.download(nat.F_RIGID_POS, nat.SPECIES_RIGID).tolist()}


def prepare(native, args):
    native.rigid_set_mode(args.mode)
    if args.mode == "scripted":
        native.rigid_set_motion(args.vel, args.omega)


def run_rank(nat, native, steps, full_step, load):
    """full_step(): one solver step and the body step after it (SlabSimulation.step); load(): (force, torque) of this rank's handle"""
    rep = {"stats": [], "loads": []}
    for k in range(steps):
        sample_x = native.download(nat.F_RIGID_POS, nat.SPECIES_RIGID)[:, 0].copy()
        st = full_step()
        if k in (0, steps - 1):
            info = native.slab_info()
            tag = "first" if k == 0 else "last"
            rep["sample_x_" + tag] = sample_x
            rep["cols_" + tag] = [info["x_lo"], info["x_hi"]]
        force, torque = load()
        rep["loads"].append(force.tobytes().hex() + torque.tobytes().hex())
        rep["load_first_max"] = rep.get("load_first_max", float(np.abs(force).max()))
        rep["load_max"] = max(rep.get("load_max", 0.0), float(np.abs(force).max()), float(np.abs(torque).max()))
        row = stat_row(st)
        if row is not None:
            rep["stats"].append(row)
    rep["info"] = native.slab_info()
    rep["body"] = body_of(native, nat)
    rep["vert"] = native.download(nat.F_RIGID_VERT, nat.SPECIES_RIGID).tolist()
    return rep


def compare(nat, cfg, rigid, args, reps, fields):
    ref = nat.Simulation(nat.config_from_dict(cfg), rigid=rigid)
    h = np.float32(ref.scalar(nat.S_SUPPORT_RADIUS))
    start = ref.download(nat.F_RIGID_POS, nat.SPECIES_RIGID).copy()
    prepare(ref, args)
    def ref_step():
        st = ref.step(1)
        ref.rigid_step()
        return st
    rr = run_rank(nat, ref, args.steps, ref_step, ref.rigid_load)
    rp, rv, rrho = ref.download(nat.F_POS), ref.download(nat.F_VEL), ref.download(nat.F_RHO)
    end = ref.download(nat.F_RIGID_POS, nat.SPECIES_RIGID)
    ref.close()
    pos, vel, rho = fields

    def owners(tag):
        return [owned_samples(r["sample_x_" + tag], h, r["cols_" + tag]) for r in reps]
    return {
        "n": int(len(rp)), "steps": args.steps, "slabs": [r["info"] for r in reps], "mode": rr["body"]["scalars"]["mode"],
        "pos_equal": bool(np.array_equal(pos, rp)), "vel_equal": bool(np.array_equal(vel, rv)), "rho_equal": bool(np.array_equal(rho, rrho)),
        "finite": bool(np.isfinite(rp).all() and np.isfinite(rv).all()),
        "stats_equal": [r["stats"] == rr["stats"] for r in reps],
        "stats_last": reps[0]["stats"][-1] if reps[0]["stats"] else None, "ref_stats_last": rr["stats"][-1] if rr["stats"] else None,
        "body_equal": [r["body"] == rr["body"] and r["vert"] == rr["vert"] for r in reps],
        "loads_equal": [r["loads"] == rr["loads"] for r in reps], "load_max": rr["load_max"], "load_first_max": rr["load_first_max"],
        "samples_equal_first": all(np.array_equal(r["sample_x_first"], rr["sample_x_first"]) for r in reps),
        "samples_equal_last": all(np.array_equal(r["sample_x_last"], rr["sample_x_last"]) for r in reps),
        "owned_samples_first": owners("first"), "owned_samples_last": owners("last"), "n_samples": int(len(rr["sample_x_first"])),
        "cols_first": [r["cols_first"] for r in reps], "cols_last": [r["cols_last"] for r in reps],
        "body_moved": float(np.abs(end - start).max()), "body_centroid": rr["body"]["scalars"]["centroid"],
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", required=True, help="path to a config JSON with a `solid` block")
    ap.add_argument("--transport", choices=("gloo", "loopback"), required=True)
    ap.add_argument("--world", type=int, default=2, help="loopback: the number of ranks (gloo: WORLD_SIZE)")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rebalance", type=int, default=0)
    ap.add_argument("--mode", choices=("scripted", "fixed"), required=True)
    ap.add_argument("--vel", type=float, nargs=3, default=[0.0, 0.0, 0.0])
    ap.add_argument("--omega", type=float, nargs=3, default=[0.0, 0.0, 0.0])
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    assert args.steps >= 2
    cfg = json.load(open(args.scene))
    from cfd_taichi_amd import mesh
    rigid = mesh.rigid_from_config(cfg)

    def per_rank(nat, native, full_step):
        prepare(native, args)
        return run_rank(nat, native, args.steps, full_step, native.rigid_load)
    body_ranks(args, cfg, rigid, per_rank, lambda nat, reps, fields: compare(nat, cfg, rigid, args, reps, fields))


if __name__ == "__main__":
    main()
