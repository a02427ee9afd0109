"""Worker of tests/test_scalar_gpu.py: the carried scalar is refused on x-slab handles.  `world` slab handles of this one process on the library's
native transport with tests/loopback_rccl.hip standing in for librccl (tests/slab_ranks.py).  Every rank makes every sph_scalar_* call and reports
its code; then the ranks and a one-GPU handle take the same steps, and the gathered positions and velocities are compared bit for bit (a refused
call left nothing behind)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from harness import bits_equal  # noqa: E402
from slab_ranks import Ranks, loopback_env  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", required=True, help="path to a config JSON")
    ap.add_argument("--world", type=int, default=2)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    loopback_env()
    from cfd_taichi_amd import _native as nat
    cfg = json.load(open(args.scene))
    group = Ranks(nat, cfg, args.world)
    ref = nat.Simulation(nat.config_from_dict(cfg))
    buf = np.zeros(ref.n_fluid, dtype=np.float32)
    calls = {
        "enable": lambda r, s: s.enable_scalar(1e-3, 0.1, 0.5),
        "disable": lambda r, s: s.disable_scalar(),
        "download": lambda r, s: s._check(s._lib.sph_scalar_download(s._h, buf.ctypes.data, buf.size)),
        "upload": lambda r, s: s._check(s._lib.sph_scalar_upload(s._h, buf.ctypes.data, buf.size)),
        "rate": lambda r, s: s._check(s._lib.sph_scalar_rate(s._h, buf.ctypes.data, buf.size)),
        "set_inflow": lambda r, s: s.set_scalar_inflow(1.0),
    }
    res = {"world": args.world, "n": int(ref.n_fluid), "codes": {}, "messages": {}, "first_difference": None}
    for name, fn in calls.items():
        res["codes"][name] = group.codes(fn)
        res["messages"][name] = [str(e) for e in group.errors]
    for k in range(1, args.steps + 1):
        group.step()
        ref.step(1)
        for name, f in (("pos", nat.F_POS), ("vel", nat.F_VEL)):
            if res["first_difference"] is None and not bits_equal(group.gather(f), ref.download(f)):
                res["first_difference"] = {"step": k, "what": name}
    res["state_code"] = nat.SPH_E_STATE
    with open(args.out, "w") as f:
        json.dump(res, f)
    group.close()
    ref.close()


if __name__ == "__main__":
    main()
