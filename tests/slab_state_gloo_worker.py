"""Worker of tests/test_slab_state_gpu.py::test_set_state_over_torch_distributed (launched by torch.distributed.run like tests/slab_worker.py):
SlabSimulation.set_state(..., src=0) over the callback transport (gloo).  Rank 0 makes the state (a one-GPU run of K steps), every rank gets it through
the broadcast; after every following step the gathered particles equal a one-GPU handle given the same state with sph_upload + sph_set_scalar."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", required=True)
    ap.add_argument("--state-steps", type=int, default=20)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    import torch.distributed as dist
    from harness import bits_equal
    from slab_ranks import process_group, stat_row
    from slab_state_worker import one_gpu_state
    with process_group() as (rank, world, device):
        from cfd_taichi_amd import _native as nat
        from cfd_taichi_amd import scenes
        from cfd_taichi_amd.slab import SlabSimulation
        cfg = scenes.get(args.scene)
        sim = SlabSimulation(cfg, rank, world, device=device)
        state = one_gpu_state(nat, cfg, args.state_steps) if rank == 0 else (None, None, None, None)
        sim.set_state(*state, src=0)
        back = sim.state()                                   # rank 0: (pos, vel, scalar, delta_time) in original order
        a = None
        res = {}
        if rank == 0:
            pos, vel, warm, dt = state
            res["roundtrip"] = bits_equal(back[0], pos) and bits_equal(back[1], vel) and bits_equal(back[2], warm)
            res["state_dt"] = np.float32(back[3]) == np.float32(dt)
            a = nat.Simulation(nat.config_from_dict(cfg, device=device))
            a.upload(nat.F_POS, pos); a.upload(nat.F_VEL, vel); a.upload(nat.F_WARM_K, warm)
            a.set_dt(dt)
        first_bad, stats_bad = None, None
        for k in range(args.steps):
            sb = stat_row(sim.step(1))
            rows = [None] * world if rank == 0 else None
            dist.gather_object(sb, rows, dst=0)
            got = [sim.gather(f) for f in (nat.F_POS, nat.F_VEL, nat.F_RHO)]
            if rank == 0:
                sa = stat_row(a.step(1))
                if stats_bad is None and any(row != sa for row in rows):
                    stats_bad = {"step": k + 1, "one_gpu": sa, "ranks": rows}
                for name, field, g in zip(("pos", "vel", "rho"), (nat.F_POS, nat.F_VEL, nat.F_RHO), got):
                    if first_bad is None and not bits_equal(g, a.download(field)):
                        first_bad = {"step": k + 1, "field": name}
        if rank == 0:
            res.update({"first_difference": first_bad, "stats_difference": stats_bad, "world": world, "n": int(sim.n_fluid)})
            res["roundtrip"], res["state_dt"] = bool(res["roundtrip"]), bool(res["state_dt"])
            with open(args.out, "w") as f:
                json.dump(res, f)
            a.close()
        sim.close()


if __name__ == "__main__":
    main()
