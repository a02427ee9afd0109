"""Worker of tests/test_slab_geometry_gpu.py: static geometry (sph_geometry_add / sph_geometry_remove) on x-slab handles
against the same calls on a one-GPU handle, bit for bit.  `world` slab handles of this one process on the library's native transport with
tests/loopback_rccl.hip standing in for librccl (tests/slab_ranks.py).

Every rank makes the same calls between the same steps (the walls are replicated).  After every step: the gathered pos, vel and rho against the
one-GPU handle's and every rank's statistics against its.  --remove-after K: the plate is taken out after step K.  Carving is refused on every rank."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from harness import bits_equal  # noqa: E402
from slab_ranks import Ranks, loopback_env, stat_row  # noqa: E402

D = 0.05
# the long tank (box 2.0 x 0.6 x 0.6, fluid x 0.1 .. 1.65, y and z 0.1 .. 0.35): a plate along the whole column 0.075 beside it, in every slab, and
# the shell of a 3 x 3 x 3 block 0.075 above it
PLATE = np.array([[D * i, D * j, 0.425] for i in range(1, 37) for j in range(1, 9)], dtype=np.float32)
BLOCK = np.array([[0.5 + D * i, 0.425 + D * j, 0.15 + D * k] for i in range(3) for j in range(3) for k in range(3) if (i, j, k) != (1, 1, 1)], dtype=np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", required=True, help="path to a config JSON")
    ap.add_argument("--world", type=int, default=2)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--remove-after", type=int, default=0)
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    loopback_env()
    from cfd_taichi_amd import _native as nat
    cfg = json.load(open(args.scene))
    group = Ranks(nat, cfg, args.world)
    ref, plain = nat.Simulation(nat.config_from_dict(cfg)), nat.Simulation(nat.config_from_dict(cfg))

    def prepare(s):
        return [s.add_geometry(PLATE), s.add_geometry(BLOCK)]

    ids = group.each(lambda r, s: prepare(s)) + [prepare(ref)]
    res = {"n": int(ref.n_fluid), "world": args.world, "groups": ids, "first_difference": None, "stats_equal": True,
           "carve_codes": group.codes(lambda r, s: s.carve(1)), "count_codes": group.codes(lambda r, s: s.wall_neighbor_counts()),
           "walls_equal": all(bits_equal(s.download(f, nat.SPECIES_WALL), ref.download(f, nat.SPECIES_WALL)) and s.geometry() == ref.geometry()
                              for s in group.sims for f in (nat.F_WALL_POS, nat.F_WALL_VOL))}
    for k in range(1, args.steps + 1):
        stats = group.step()
        want = stat_row(ref.step(1))
        plain.step(1)
        res["stats_equal"] = res["stats_equal"] and all(st == want for st in stats)
        if res["first_difference"] is None:
            for name, f in (("pos", nat.F_POS), ("vel", nat.F_VEL), ("rho", nat.F_RHO)):
                if not bits_equal(group.gather(f), ref.download(f)):
                    res["first_difference"] = {"step": k, "what": name}
                    break
        if k == args.remove_after:
            group.each(lambda r, s: s.remove_geometry(1))
            ref.remove_geometry(1)
    res["n_wall"] = [int(s.n_wall) for s in group.sims] + [int(ref.n_wall)]
    res["geometry"] = [s.geometry() for s in group.sims] + [ref.geometry()]
    # (pbf's lattice at rest is under-dense: its constraint stays at zero, the geometry shows in rho alone)
    res["rows_felt"] = int(((ref.download(nat.F_POS) != plain.download(nat.F_POS)).any(axis=1) | (ref.download(nat.F_RHO) != plain.download(nat.F_RHO))).sum())
    res["finite"] = bool(np.isfinite(ref.download(nat.F_POS)).all())
    res["slabs"] = [s.slab_info() for s in group.sims]
    res["overrides"] = [s.overrides() for s in group.sims]
    with open(args.out, "w") as f:
        json.dump(res, f)
    group.close()
    ref.close(); plain.close()


if __name__ == "__main__":
    main()
