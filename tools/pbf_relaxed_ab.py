"""PBF under the exact and the relaxed arithmetic (csrc/sph_pbf_kernels.h, RX), interleaved inside one process (one clock state):
    tools/pbf_relaxed_ab.py [--scene 30k|1m|both] [--repeats R] [--window SECONDS] [--warm STEPS]
Three handles on the same start state -- exact, exact again (`exact'`: the spread of the same arithmetic against itself) and relaxed -- advance in
lock step; per repeat each gets one window of at least `--window` seconds of steps, in random order, fenced by a device synchronise on both sides.
A separate pass with the handle's own profile on gives the mean time of the three sweeps per launch.
  30k   breaking_dam_30k_pbf (quad sweeps, the reference's cell order)
  1m    dfsph_1m's geometry with solver.name = "pbf" and PBF's delta_time (plain sweeps, Morton cells); built here, no scene file"""
import argparse
import os
os.environ.setdefault("SPH_DEV", "1")     # tools run with development overrides enabled (sph_overrides reports them)
import random
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cfd_taichi_amd import _native as nat, scenes  # noqa: E402

KERNELS = ("pbf_lambda", "pbf_delta_pos", "pbf_xsph")


def config(which):
    if which == "30k":
        return "breaking_dam_30k_pbf", scenes.get("breaking_dam_30k_pbf")
    cfg = scenes.get("dfsph_1m")
    cfg["solver"]["name"] = "pbf"
    cfg["solver"]["delta_time"] = 2.5e-4
    return "dfsph_1m geometry, solver pbf, dt 2.5e-4", cfg


def window(sim, steps):
    sim.synchronize()
    t0 = time.perf_counter()
    sim.step_pbf(steps)
    sim.synchronize()
    return time.perf_counter() - t0


def run(which, args):
    label, cfg = config(which)
    sims = {"exact": nat.Simulation(nat.config_from_dict(cfg)), "exact'": nat.Simulation(nat.config_from_dict(cfg)),
            "relaxed": nat.Simulation(nat.config_from_dict(cfg, arith=nat.ARITH_RELAXED))}
    n = sims["exact"].n_fluid
    print("== %s: %d fluid particles, overrides %s, SPH_S_ARITH_RELAXED %s" % (
        label, n, sims["exact"].overrides(), {k: int(s.scalar(nat.S_ARITH_RELAXED)) for k, s in sims.items()}))
    for s in sims.values():
        s.step_pbf(args.warm)
    steps = 16                                  # steps per window: doubled until a window of the exact handle lasts long enough
    while window(sims["exact"], steps) < args.window:
        for k in ("exact'", "relaxed"):
            sims[k].step_pbf(steps)             # lock step
        steps *= 2
    for k in ("exact'", "relaxed"):
        sims[k].step_pbf(steps)
    print("window: %d steps" % steps)
    ms = {k: [] for k in sims}
    order = list(sims)
    for r in range(args.repeats):
        random.shuffle(order)
        for k in order:
            ms[k].append(window(sims[k], steps) / steps * 1e3)
        print("repeat %d  " % (r + 1) + "  ".join("%s %.4f ms/step" % (k, ms[k][-1]) for k in sims))
    med = {k: statistics.median(v) for k, v in ms.items()}
    for k in sims:
        print("%-8s ms/step min %.4f median %.4f max %.4f -> %.1f Mparticle-steps/s (median)" % (k, min(ms[k]), med[k], max(ms[k]), n / med[k] / 1e3))
    spread = max(abs(a / b - 1.0) for a, b in zip(ms["exact'"], ms["exact"]))
    print("spread of the exact arithmetic against itself: median ratio exact'/exact %.4f, largest |ratio - 1| of a repeat %.4f" % (
        med["exact'"] / med["exact"], spread))
    print("relaxed/exact: median ratio %.4f (per repeat %s)" % (med["relaxed"] / med["exact"],
                                                                " ".join("%.4f" % (a / b) for a, b in zip(ms["relaxed"], ms["exact"]))))
    # per-kernel means from the handle's own profile, in a pass of its own
    psteps = max(steps // 4, 16)
    prof = {}
    for k in ("exact", "relaxed"):
        sims[k].profile_enable(True); sims[k].profile_reset()
        sims[k].step_pbf(psteps); sims[k].synchronize()
        prof[k] = sims[k].profile()
        sims[k].profile_enable(False)
    sims["exact'"].step_pbf(psteps)
    print("per-kernel mean over %d launches, us:  %-14s %10s %10s %8s" % (psteps, "kernel", "exact", "relaxed", "ratio"))
    for name in KERNELS:
        e, x = (prof[k][name][0] / prof[k][name][1] * 1e3 for k in ("exact", "relaxed"))
        print("%38s %-14s %10.2f %10.2f %8.3f" % ("", name, e, x, x / e))
    for s in sims.values():
        s.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scene", default="both", choices=["30k", "1m", "both"])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--warm", type=int, default=50)
    args = ap.parse_args()
    for which in (("30k", "1m") if args.scene == "both" else (args.scene,)):
        run(which, args)


if __name__ == "__main__":
    main()
