"""Worker of tests/test_slab_state_gpu.py: sph_slab_set_state on the loopback stand-in for the native transport (the ranks are slab handles of
this one process, one thread each per collective call -- tests/slab_ranks.py holds the rank group and describes the stand-in).

The yardstick of every comparison: A = a fresh one-GPU handle given a state with sph_upload (pos, vel, warm_start_k) + sph_set_scalar(delta_time),
B = `world` slab handles given the same state with sph_slab_set_state.  After EVERY following step the owned particles of B, gathered by id, must
equal A bit for bit (positions, velocities, densities), and so must the step statistics, on every rank.  The state comes from a one-GPU run of K steps.

modes: equal (cases 1-7: options for re-cuts, ghost columns, steps from rest before the hand-over, a mirrored state), roundtrip (case 8),
refuse (case 9: every refusal on every rank alike, the handles untouched), time (the cost of the call, for BASELINE.md)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from harness import bits_equal  # noqa: E402
from slab_ranks import Ranks, gather_by_id, loopback_env, stat_row  # noqa: E402


def gather_ok(b, field):
    """(the owned particles by id, whether the ownership is a partition): the flag goes into the report instead of an assertion"""
    out, seen = gather_by_id(b.sims, field)
    return out, bool(np.all(seen == 1))


def one_gpu_state(nat, cfg, steps, rigid=None):
    """(pos, vel, warm_start_k or None, delta_time) after `steps` steps from rest on one GPU"""
    sim = nat.Simulation(nat.config_from_dict(cfg), rigid=rigid)
    if steps:
        sim.step(steps)
    dfsph = sim.cfg.solver == nat.SOLVER_DFSPH
    st = (sim.download(nat.F_POS), sim.download(nat.F_VEL), sim.download(nat.F_WARM_K) if dfsph else None, sim.scalar(nat.S_DELTA_TIME))
    sim.close()
    return st


def mode_equal(nat, cfg, args):
    pos, vel, warm, dt = one_gpu_state(nat, cfg, args.k)
    if args.mirror:           # x' = box_min.x + box_max.x - x, in the arithmetic of the arrays
        pos = pos.copy()
        pos[:, 0] = np.float32(cfg["scene"]["box_min"][0]) + np.float32(cfg["scene"]["box_max"][0]) - pos[:, 0]
    a = nat.Simulation(nat.config_from_dict(cfg))
    a.upload(nat.F_POS, pos); a.upload(nat.F_VEL, vel)
    if warm is not None:
        a.upload(nat.F_WARM_K, warm)
    a.set_dt(dt)
    b = Ranks(nat, cfg, args.world, slab_rebalance_every=args.rebalance, slab_ghost_layers=args.layers, slab_overlap=args.overlap)
    for _ in range(args.prestep):
        b.step()
    res = {"cuts_created": b.cuts(), "ghosts_before": [s.slab_info()["ghosts"] for s in b.sims]}
    b.each(lambda r, s: s.slab_set_state(pos, vel, warm, dt))
    res["cuts_set"] = b.cuts()
    res["owned"] = [s.slab_info()["owned"] for s in b.sims]
    res["ghosts_after_set"] = [s.slab_info()["ghosts"] for s in b.sims]
    res["n"] = int(a.n_fluid)
    back = [gather_ok(b, f) for f in (nat.F_POS, nat.F_VEL)] + ([gather_ok(b, nat.F_WARM_K)] if warm is not None else [])
    res["partition"] = all(ok for _, ok in back)
    res["roundtrip"] = all(bits_equal(got, want) for (got, _), want in zip(back, (pos, vel, warm)))
    res["dt_set"] = [s.scalar(nat.S_DELTA_TIME) for s in b.sims] == [a.scalar(nat.S_DELTA_TIME)] * args.world
    first_bad, stats_bad = None, None
    for k in range(args.m):
        sa = stat_row(a.step(1))
        sb = b.step()
        if stats_bad is None and any(row != sa for row in sb):
            stats_bad = {"step": k + 1, "one_gpu": sa, "ranks": sb}
        for name, field in (("pos", nat.F_POS), ("vel", nat.F_VEL), ("rho", nat.F_RHO)):
            got, ok = gather_ok(b, field)
            if first_bad is None and not (ok and bits_equal(got, a.download(field))):
                first_bad = {"step": k + 1, "field": name, "partition": ok}
    res.update({"steps_compared": args.m, "first_difference": first_bad, "stats_difference": stats_bad, "stats_last": sa,
                "cuts_end": b.cuts(), "recuts": [s.slab_info()["recuts"] for s in b.sims], "overrides": b.sims[0].overrides()})
    a.close(); b.close()
    return res


def mode_roundtrip(nat, cfg, args):
    pos = one_gpu_state(nat, cfg, args.k)[0]
    rng = np.random.default_rng(7)
    vel = rng.standard_normal(pos.shape).astype(np.float32)
    warm = rng.standard_normal(len(pos)).astype(np.float32)
    b = Ranks(nat, cfg, args.world)
    b.each(lambda r, s: s.slab_set_state(pos, vel, warm, 0.0))
    back = [gather_ok(b, f) for f in (nat.F_POS, nat.F_VEL, nat.F_WARM_K)]
    res = {"partition": all(ok for _, ok in back), "equal": [bits_equal(got, want) for (got, _), want in zip(back, (pos, vel, warm))],
           "owned": [s.slab_info()["owned"] for s in b.sims], "n": len(pos), "overrides": b.sims[0].overrides()}
    # vel / scalar NULL: zeros
    b.each(lambda r, s: s.slab_set_state(pos))
    back = [gather_ok(b, f) for f in (nat.F_VEL, nat.F_WARM_K)]
    res["null_is_zero"] = all(ok and not got.view(np.uint32).any() for got, ok in back)
    b.close()
    return res


def mode_refuse(nat, scenes, args):
    """Every refusal: the same code on every rank, and the handles go on for 5 steps exactly like a twin that was never asked."""
    E_INVALID, E_OVERFLOW, E_STATE = nat.SPH_E_INVALID, nat.SPH_E_OVERFLOW, nat.SPH_E_STATE
    res = {}

    def group(name, scene, world, calls, per_rank=None):
        cfg = scenes.get(scene)
        rigid = None
        if cfg.get("solid"):
            from cfd_taichi_amd import mesh
            rigid = mesh.rigid_from_config(cfg)
        pos, vel, warm, dt = one_gpu_state(nat, cfg, 0)        # the lattice at rest: valid where a call does not spoil it
        n = len(pos)
        twin = Ranks(nat, cfg, world, rigid=rigid, per_rank=per_rank)
        want = []
        for _ in range(3):
            twin.step()
        for _ in calls:
            for _ in range(5):
                twin.step()
            want.append(twin.digest())
        twin.close()
        b = Ranks(nat, cfg, world, rigid=rigid, per_rank=per_rank)
        for _ in range(3):
            b.step()
        for (label, make, code), digest in zip(calls, want):
            state = make(pos.copy(), vel, warm, n, cfg)
            before = b.digest()
            codes = b.codes(lambda r, s: s.slab_set_state(*state))
            untouched = b.digest() == before
            for _ in range(5):
                b.step()
            res[name + ":" + label] = {"codes": codes, "want": [code] * world, "untouched": untouched, "steps_equal_twin": b.digest() == digest}
        b.close()

    def nan_pos(p, v, w, n, cfg):
        p[n // 3, 1] = np.nan
        return p, v, w, 0.0

    def outside(p, v, w, n, cfg):
        p[n - 1, 0] = np.float32(cfg["scene"]["box_max"][0]) + np.float32(1.0)
        return p, v, w, 0.0

    def wrong_n(p, v, w, n, cfg):
        return p[:-1], v[:-1], None if w is None else w[:-1], 0.0

    def plain(p, v, w, n, cfg):
        return p, v, w, 0.0

    def scalar_where_none(p, v, w, n, cfg):
        return p, v, np.zeros(n, dtype=np.float32), 0.0

    def mirrored(p, v, w, n, cfg):
        p[:, 0] = np.float32(cfg["scene"]["box_min"][0]) + np.float32(cfg["scene"]["box_max"][0]) - p[:, 0]
        return p, v, w, 0.0
    group("dfsph", "dfsph_small", 2, [("nan", nan_pos, E_INVALID), ("outside", outside, E_INVALID), ("wrong_n", wrong_n, E_INVALID)])
    group("wcsph", "wcsph_small", 2, [("scalar", scalar_where_none, E_INVALID)])
    group("rigid", "dfsph_rigid_small", 2, [("body", plain, E_STATE)])
    # rank 2 of 3 owns nothing of the lattice at rest (it lies beyond the fluid) and gets room for 600 particles; the mirrored lattice gives it thousands
    group("capacity", "dfsph_small", 3, [("one_rank", mirrored, E_OVERFLOW)], per_rank={2: {"slab_capacity": 600}})
    return res


def mode_time(nat, cfg, args):
    pos, vel, warm, dt = one_gpu_state(nat, cfg, args.k)
    b = Ranks(nat, cfg, args.world)
    ms = []
    for _ in range(3):
        for s in b.sims:
            s.synchronize()
        t0 = time.perf_counter()
        b.each(lambda r, s: s.slab_set_state(pos, vel, warm, dt))
        ms.append((time.perf_counter() - t0) * 1e3)
    res = {"n": len(pos), "world": args.world, "ms_per_call": ms, "owned": [s.slab_info()["owned"] for s in b.sims]}
    b.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="equal", choices=["equal", "roundtrip", "refuse", "time"])
    ap.add_argument("--scene", default="dfsph_small")
    ap.add_argument("--world", type=int, default=2)
    ap.add_argument("--k", type=int, default=20, help="steps of the one-GPU run the state comes from")
    ap.add_argument("--m", type=int, default=10, help="steps compared after the hand-over")
    ap.add_argument("--rebalance", type=int, default=0)
    ap.add_argument("--layers", type=int, default=0)
    ap.add_argument("--overlap", type=int, default=0)
    ap.add_argument("--prestep", type=int, default=0, help="steps the slab handles run from rest before they are given the state")
    ap.add_argument("--mirror", action="store_true")
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    loopback_env()
    from cfd_taichi_amd import _native as nat
    from cfd_taichi_amd import scenes
    if args.mode == "refuse":
        res = mode_refuse(nat, scenes, args)
    else:
        cfg = scenes.get(args.scene)
        res = {"equal": mode_equal, "roundtrip": mode_roundtrip, "time": mode_time}[args.mode](nat, cfg, args)
    with open(args.out, "w") as f:
        json.dump(res, f)


if __name__ == "__main__":
    main()
