"""Worker of tests/test_slab_pbf_gpu.py: pbf_solver on x-slab handles against the one-GPU handle, bit for bit.

Two ways to run `world` ranks on one GPU:
  --transport gloo       launched by torch.distributed.run, one process per rank, SlabSimulation over the callback transport (mode equal only);
  --transport loopback   `world` slab handles of this one process, one thread each per collective call, on the library's NATIVE transport with
                         tests/loopback_rccl.hip standing in for librccl (tests/slab_ranks.py holds the rank group and describes the stand-in; SPH_DEV=1 is set here).
(tests/slab_worker.py and tests/loopback_worker.py read step statistics, which PBF has none of.)

The yardstick of every comparison: a one-GPU handle given the same state with sph_upload (pos, vel) and stepped the same number of steps; the
owned particles of the slab handles, gathered by particle id, must equal its pos, vel, rho, pbf_lambda and delta_pos as raw f32 -- after EVERY
step, so that a failure names the first step and field.  The state comes from the caller as an .npz (pos, vel; tests/slab_pbf_states.py) and
enters the slab handles through sph_slab_set_state; without --state both sides run from rest.

modes: equal (steps from a state or from rest; comm statistics; --dump writes the sharded run's final fields), roundtrip (state() of one group
into set_state() of another; the scalar refusal), midrun (sph_compute_density / sph_build_neighbors between steps), overflow (one rank's lists
overflow: every rank fails together)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import slab_pbf_states as sp  # noqa: E402
from harness import bits_equal  # noqa: E402
from slab_ranks import Ranks, loopback_env, process_group  # noqa: E402


def first_difference(step, got, ref):
    """None, or where the sharded fields leave the one-GPU handle's"""
    for name, _ in sp.FIELDS:
        if not bits_equal(got[name], ref[name]):
            bad = np.flatnonzero((got[name].view(np.uint32) != ref[name].view(np.uint32)).reshape(len(ref[name]), -1).any(1))
            return {"step": step, "field": name, "particles": int(len(bad)), "first_ids": [int(i) for i in bad[:8]],
                    "max_abs": float(np.nanmax(np.abs(got[name].astype(np.float64) - ref[name])))}
    return None


def one_gpu(nat, cfg, state, arith=0, device=0):
    a = nat.Simulation(nat.config_from_dict(cfg, arith=arith, device=device))
    if state is not None:
        a.upload(nat.F_POS, state[0]); a.upload(nat.F_VEL, state[1])
    return a


def fields_of(nat, download):
    return {name: download(f) for name, f in sp.FIELDS}


def set_state(group, pos, vel, scalar=None, dt=0.0):
    group.each(lambda r, s: s.slab_set_state(pos, vel, scalar, dt))


def load_state(path):
    if not path:
        return None
    z = np.load(path)
    return np.ascontiguousarray(z["pos"], dtype=np.float32), np.ascontiguousarray(z["vel"], dtype=np.float32)


def window(stats0, stats1, recuts0, recuts1):
    d = {k: stats1[k] - stats0[k] for k in stats1}
    d["recuts"] = recuts1 - recuts0
    return d


def mode_equal_loopback(nat, cfg, args):
    state = load_state(args.state)
    b = Ranks(nat, cfg, args.world, slab_rebalance_every=args.rebalance, arith=args.arith)
    a = one_gpu(nat, cfg, state, arith=args.arith)
    if state is not None:
        set_state(b, state[0], state[1])
    own0 = b.owners()
    for s in b.sims:
        s.comm_stats(reset=True)
    res = {"n": int(b.sims[0].n_fluid), "world": args.world, "cuts_start": [i["x_lo"] for i in b.infos()], "owned_sums": [], "ghosts_max": [0] * args.world,
           "first_difference": None}
    after_first = None
    for k in range(1, args.steps + 1):
        b.step(); a.step_pbf(1)
        infos = b.infos()
        res["owned_sums"].append(sum(i["owned"] for i in infos))
        res["ghosts_max"] = [max(g, i["ghosts"]) for g, i in zip(res["ghosts_max"], infos)]
        if k == 1:
            after_first = ([s.comm_stats() for s in b.sims], [i["recuts"] for i in infos])
        if res["first_difference"] is None and (args.every_step or k == args.steps):
            res["first_difference"] = first_difference(k, fields_of(nat, b.gather), fields_of(nat, a.download))
    infos = b.infos()
    total = [s.comm_stats() for s in b.sims]
    res["comm_whole_run"] = [dict(t, recuts=i["recuts"]) for t, i in zip(total, infos)]
    # an ordinary step exchanges particles in one round, a step that moved the cuts in two; so does the first step after sph_slab_set_state, which
    # is not a re-cut: the per-step identities are taken over steps 2 .. steps
    res["comm_after_step_1"] = [window(s0, s1, r0, i["recuts"]) for s0, s1, r0, i in zip(after_first[0], total, after_first[1], infos)]
    res["slabs"] = infos
    res["owner_changes"] = int((b.owners() != own0).sum())
    res["relaxed"] = [s.scalar(nat.S_ARITH_RELAXED) for s in b.sims] + [a.scalar(nat.S_ARITH_RELAXED)]
    res["overrides"] = b.sims[0].overrides()
    if args.dump:
        np.savez(args.dump, **fields_of(nat, b.gather))
    a.close(); b.close()
    return res


def mode_roundtrip(nat, cfg, args):
    """world ranks run `steps` steps, their state() goes into set_state() of a fresh group of 2 ranks, which runs `steps` more: 2 x steps uninterrupted
    steps of one GPU.  In between, the first group is offered a scalar (refused everywhere, handles untouched: it runs on and must agree as well)."""
    state = load_state(args.state)
    a = one_gpu(nat, cfg, state)
    b = Ranks(nat, cfg, args.world)
    set_state(b, state[0], state[1])
    res = {"n": int(b.sims[0].n_fluid)}
    res["lambda_before_first_step"] = b.codes(lambda r, s: s.download_local(nat.F_PBF_LAMBDA))
    for _ in range(args.steps):
        b.step()
    a.step_pbf(args.steps)
    pos, vel, dt = b.gather(nat.F_POS), b.gather(nat.F_VEL), b.sims[0].scalar(nat.S_DELTA_TIME)
    res["state_equal_one_gpu"] = bits_equal(pos, a.download(nat.F_POS)) and bits_equal(vel, a.download(nat.F_VEL))
    res["scalar_refused"] = b.codes(lambda r, s: s.slab_set_state(pos, vel, np.zeros(len(pos), dtype=np.float32), dt))
    c = Ranks(nat, cfg, 2)
    set_state(c, pos, vel, None, dt)
    res["owned_after_set"] = [i["owned"] for i in c.infos()]
    res["lambda_after_set_state"] = c.codes(lambda r, s: s.download_local(nat.F_PBF_LAMBDA))
    for _ in range(args.steps):
        b.step(); c.step()
    a.step_pbf(args.steps)
    ref = fields_of(nat, a.download)
    res["first_difference"] = first_difference(2 * args.steps, fields_of(nat, c.gather), ref)
    res["refused_group_runs_on"] = first_difference(2 * args.steps, fields_of(nat, b.gather), ref)
    # set_state on handles that have stepped: pbf_lambda / delta_pos are "before the first step" again
    set_state(b, pos, vel, None, dt)
    res["lambda_after_set_state_mid_run"] = b.codes(lambda r, s: s.download_local(nat.F_PBF_LAMBDA))
    a.close(); b.close(); c.close()
    return res


def mode_midrun(nat, cfg, args):
    """between steps `at` and `at` + 1 every rank calls sph_compute_density, then sph_build_neighbors twice"""
    state = load_state(args.state)
    a = one_gpu(nat, cfg, state)
    b = Ranks(nat, cfg, args.world)
    set_state(b, state[0], state[1])
    res = {"n": int(b.sims[0].n_fluid), "first_difference": None}
    for k in range(1, args.steps + 1):
        b.step(); a.step_pbf(1)
        if res["first_difference"] is None:
            res["first_difference"] = first_difference(k, fields_of(nat, b.gather), fields_of(nat, a.download))
        if k == args.at:
            b.each(lambda r, s: s.compute_density())
            a2 = one_gpu(nat, cfg, state)
            a2.step_pbf(args.at); a2.compute_density()
            res["rho_after_compute_density"] = bits_equal(b.gather(nat.F_RHO), a2.download(nat.F_RHO))
            res["lambda_after_compute_density"] = b.codes(lambda r, s: s.download_local(nat.F_PBF_LAMBDA))
            a2.close()
            b.each(lambda r, s: (s.build_neighbors(), s.build_neighbors()))
            res["lambda_after_build"] = b.codes(lambda r, s: s.download_local(nat.F_PBF_LAMBDA))
            res["delta_pos_after_build"] = b.codes(lambda r, s: s.download_local(nat.F_PBF_DELTA_POS))
            res["state_after_build"] = bits_equal(b.gather(nat.F_POS), a.download(nat.F_POS)) and bits_equal(b.gather(nat.F_VEL), a.download(nat.F_VEL))
            res["owned_after_build"] = sum(i["owned"] for i in b.infos())
        if k == args.at + 1:
            res["lambda_after_next_step"] = b.codes(lambda r, s: s.download_local(nat.F_PBF_LAMBDA))
    a.close(); b.close()
    return res


def mode_overflow(nat, cfg, args):
    state = load_state(args.state)
    b = Ranks(nat, cfg, args.world, per_rank={args.overflow_rank: {"max_neighbors": args.max_neighbors}})
    set_state(b, state[0], state[1])
    res = {"codes": b.codes(lambda r, s: s.step_pbf(1)), "errors": [None if e is None else str(e) for e in b.errors]}
    b.close()
    return res


def mode_equal_gloo(args, rank, world, device):
    import torch
    import torch.distributed as dist
    from cfd_taichi_amd import _native as nat
    from cfd_taichi_amd.slab import SlabSimulation
    cfg = sp.config(args.scene)
    state = load_state(args.state) if rank == 0 else None
    sim = SlabSimulation(cfg, rank, world, device=device, rebalance_every=args.rebalance, arith=args.arith)
    if args.state:
        sim.set_state(*(state or (None, None)), src=0)          # rank 0's arrays, broadcast; scalar None: pbf carries none

    def owners():
        parts = [None] * world if rank == 0 else None
        dist.gather_object(sim.owned(nat.F_POS)[0], parts, dst=0)
        if rank != 0:
            return None
        own = np.full(sim.n_fluid, -1, dtype=np.int32)
        for r, ids in enumerate(parts):
            own[ids] = r
        return own

    def total(v):
        t = torch.tensor([int(v)], dtype=torch.int64)
        dist.all_reduce(t)
        return int(t[0])
    own0 = owners()
    a = one_gpu(nat, cfg, state, arith=args.arith, device=device) if rank == 0 else None
    res = {"n": int(sim.n_fluid), "world": world, "owned_sums": [], "first_difference": None}
    ghosts_max = 0
    ret = "unset"
    for k in range(1, args.steps + 1):
        ret = sim.step(1)
        info = sim.sim.slab_info()
        ghosts_max = max(ghosts_max, info["ghosts"])
        res["owned_sums"].append(total(info["owned"]))
        if args.every_step or k == args.steps:
            got = {name: sim.gather(f) for name, f in sp.FIELDS}
            if rank == 0:
                a.step_pbf(1 if args.every_step else args.steps)
                if res["first_difference"] is None:
                    res["first_difference"] = first_difference(k, got, fields_of(nat, a.download))
    back = sim.state()
    own1 = owners()
    parts = [None] * world if rank == 0 else None
    dist.gather_object((ghosts_max, sim.sim.slab_info(), sim.sim.comm_stats(), sim.comm.stats, sim.sim.scalar(nat.S_ARITH_RELAXED)), parts, dst=0)
    if rank == 0:
        res["step_returns_none"] = ret is None
        res["state_round_trip"] = bool(bits_equal(back[0], got["pos"]) and bits_equal(back[1], got["vel"]) and back[2] is None and
                                       np.float32(back[3]) == np.float32(cfg["solver"]["delta_time"]))
        res["ghosts_max"] = [p[0] for p in parts]
        res["slabs"] = [p[1] for p in parts]
        res["comm_whole_run"] = [p[2] for p in parts]
        res["callbacks"] = [p[3] for p in parts]
        res["relaxed"] = [p[4] for p in parts] + [a.scalar(nat.S_ARITH_RELAXED)]
        res["owner_changes"] = int((own1 != own0).sum())
        if args.dump:
            np.savez(args.dump, **got)
        with open(args.out, "w") as f:
            json.dump(res, f)
        a.close()
    sim.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--transport", default="loopback", choices=["loopback", "gloo"])
    ap.add_argument("--mode", default="equal", choices=["equal", "roundtrip", "midrun", "overflow"])
    ap.add_argument("--scene", required=True, help="long_wall, long_clamp or a scene of cfd_taichi_amd.scenes")
    ap.add_argument("--state", default="", help=".npz with pos and vel in original particle order; without it the runs start from rest")
    ap.add_argument("--world", type=int, default=2, help="loopback: the number of ranks (gloo: torch.distributed.run sets it)")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rebalance", type=int, default=0)
    ap.add_argument("--arith", type=int, default=0)
    ap.add_argument("--at", type=int, default=10, help="midrun: the calls come after this step")
    ap.add_argument("--overflow-rank", type=int, default=1)
    ap.add_argument("--max-neighbors", type=int, default=12)
    ap.add_argument("--final-only", dest="every_step", action="store_false", help="compare after the last step only (large scenes)")
    ap.add_argument("--dump", default="", help="equal: write the sharded run's final fields (gathered by id) to this .npz")
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    os.environ.setdefault("SPH_SLAB_CHECK", "1")
    if args.transport == "gloo":
        assert args.mode == "equal", "the gloo worker runs mode equal"
        with process_group() as (rank, world, device):
            mode_equal_gloo(args, rank, world, device)
        return
    loopback_env()
    from cfd_taichi_amd import _native as nat
    cfg = sp.config(args.scene)
    res = {"equal": mode_equal_loopback, "roundtrip": mode_roundtrip, "midrun": mode_midrun, "overflow": mode_overflow}[args.mode](nat, cfg, args)
    with open(args.out, "w") as f:
        json.dump(res, f)


if __name__ == "__main__":
    main()
