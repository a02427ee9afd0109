"""What measuring loads on walls costs:
    tools/wall_load_cost.py [steps] [rounds] [warm]
On dam_pillars_dfsph three handles advance in lock step behind `warm` steps -- nothing measured, the three pillars measured, the pillars and the box
measured -- and rounds of `steps` steps are timed alternately (host clock around step + synchronize).  Then dfsph_1m with nothing measured and
with the box measured: the worst case, one force launch over every box sample per density iteration.  Last the fixed costs on both scenes: one
measure_loads call (the measured set is built on the host and uploaded) and one wall_load read (the reduction pair and a blocking copy).
Measuring is invisible to the fluid, so the handles of a scene hold the same state throughout; the tool checks that at the end."""
import os
os.environ.setdefault("SPH_DEV", "1")
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cfd_taichi_amd import _native as nat, scenes  # noqa: E402

steps, rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 20, int(sys.argv[2]) if len(sys.argv) > 2 else 10
warm = int(sys.argv[3]) if len(sys.argv) > 3 else 2400


def timed(fn, repeat=5):
    out = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return min(out), statistics.median(out)


def compare(scene, variants, warm_steps):
    cfg = scenes.get(scene)
    cfg["scene"].pop("loads", None)
    sims = {}
    for name, groups in variants:
        sims[name] = nat.Simulation(nat.config_from_dict(cfg), config=cfg)
        if groups:
            sims[name].measure_loads(groups)
        sims[name].step(warm_steps)
        sims[name].synchronize()
    res = {n: [] for n in sims}
    for _ in range(rounds):
        for n, s in sims.items():
            t0 = time.perf_counter()
            s.step(steps)
            s.synchronize()
            res[n].append((time.perf_counter() - t0) / steps * 1e3)
    first = next(iter(sims.values()))
    pos = first.download(nat.F_POS)
    for n, t in res.items():
        s = sims[n]
        assert np.array_equal(s.download(nat.F_POS).view(np.uint32), pos.view(np.uint32)), "measuring changed the fluid"
        measured = sum(len(s.wall_forces(g)) for g in s.measured_groups)
        line = "%-20s %-14s %7d particles %7d wall samples %7d measured  ms/step min %.3f median %.3f  (last step: %d density iterations)" % (
            scene, n, s.n_fluid, s.n_wall, measured, min(t), statistics.median(t), s.last_stats.n_dens)
        if s.measured_groups:
            f = s.wall_load(None)[0]
            line += "  |F| of the measured groups %.6g N" % float(np.sqrt((f * f).sum()))
        print(line, flush=True)
    for n, s in sims.items():
        if s.measured_groups:
            groups = list(s.measured_groups)
            print("%-20s %-14s one wall_load read: min %.3f median %.3f ms;  one measure_loads call: min %.1f median %.1f ms" % (
                (scene, n) + timed(lambda: s.wall_load(None)) + timed(lambda: s.measure_loads(groups), 3)), flush=True)
        s.close()


compare("dam_pillars_dfsph", [("off", None), ("pillars", ["pillar_0", "pillar_1", "pillar_2"]), ("pillars+box", ["pillar_0", "pillar_1", "pillar_2", "box"])], warm)
compare("dfsph_1m", [("off", None), ("box", ["box"])], min(warm, 100))
