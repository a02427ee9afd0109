"""Worker of tests/test_slab_forcing_gpu.py: gravity as a vector under harmonic forcing (sph_set_gravity / sph_set_forcing) on x-slab handles
against the same calls on a one-GPU handle, bit for bit.  `world` slab handles of this one process, one thread each per collective call, on the
library's native transport with tests/loopback_rccl.hip standing in for librccl (tests/slab_ranks.py holds the rank group and describes the stand-in).

Every rank makes the same set calls before its first step.  After every step: the gathered pos and vel against the one-GPU handle's, and
SPH_S_TIME and SPH_S_ACCEL of every rank against its (the clock's eight bytes, the vector's twelve).  With --body (a scene with a `solid` block)
every solver step is followed by a body step, and the body's samples and scalars are compared on every rank as well."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import forcing as fo  # noqa: E402
from harness import bits_equal  # noqa: E402
from slab_ranks import Ranks, loopback_env  # noqa: E402


def clock_and_vector(sim):
    return np.float64(sim.time()).tobytes().hex() + sim.accel().tobytes().hex()


def body_of(nat, sim):
    sc = sim.rigid_scalars()
    return [sim.download(nat.F_RIGID_POS, nat.SPECIES_RIGID).tobytes().hex(), sc["centroid"], sc["vel"], sc["omega"]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", required=True, help="path to a config JSON")
    ap.add_argument("--world", type=int, default=2)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--body", action="store_true")
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    loopback_env()
    from cfd_taichi_amd import _native as nat
    cfg = json.load(open(args.scene))
    rigid = None
    if args.body:
        from cfd_taichi_amd import mesh
        rigid = mesh.rigid_from_config(cfg)
    world = args.world
    group = Ranks(nat, cfg, world, rigid=rigid)
    sims = group.sims
    ref = nat.Simulation(nat.config_from_dict(cfg), rigid=rigid)

    def prepare(s):
        s.set_gravity(fo.TILT)
        s.set_forcing(fo.AMP, fo.OMEGA, fo.PHASE)

    def full_step(s):
        st = s.step(1)
        if args.body:
            s.rigid_step()
        return None if st is None else [st.n_div, st.n_dens, st.lost]

    group.each(lambda r, s: prepare(s))
    prepare(ref)
    res = {"n": int(ref.n_fluid), "world": world, "first_difference": None, "vectors": [], "stats_equal": True,
           "clock_start_equal": all(clock_and_vector(s) == clock_and_vector(ref) for s in sims)}
    for k in range(1, args.steps + 1):
        stats = group.each(lambda r, s: full_step(s))
        want = full_step(ref)
        res["stats_equal"] = res["stats_equal"] and all(st == want for st in stats)
        res["vectors"].append(ref.accel().tolist())
        if res["first_difference"] is None:
            for name, f in (("pos", nat.F_POS), ("vel", nat.F_VEL)):
                if not bits_equal(group.gather(f), ref.download(f)):
                    res["first_difference"] = {"step": k, "what": name}
                    break
        if res["first_difference"] is None:
            for r, s in enumerate(sims):
                if clock_and_vector(s) != clock_and_vector(ref):
                    res["first_difference"] = {"step": k, "what": "time / accel on rank %d" % r, "rank": [s.time(), s.accel().tolist()],
                                               "one_gpu": [ref.time(), ref.accel().tolist()]}
                    break
                if args.body and body_of(nat, s) != body_of(nat, ref):
                    res["first_difference"] = {"step": k, "what": "the body on rank %d" % r}
                    break
    res["time"] = ref.time()
    res["finite"] = bool(np.isfinite(ref.download(nat.F_POS)).all())
    res["slabs"] = [s.slab_info() for s in sims]
    res["overrides"] = [s.overrides() for s in sims]
    if args.body:
        res["body_vel"] = ref.rigid_scalars()["vel"]
    with open(args.out, "w") as f:
        json.dump(res, f)
    group.close()
    ref.close()


if __name__ == "__main__":
    main()
