"""Host cost of editing a handle's wall set and the step time of a scene with geometry beside the same scene without:
    tools/geometry_cost.py [steps] [rounds] [warm]
On breaking_dam_30k_dfsph: one add_geometry of a box shell of about 10 k samples, one remove_geometry of it, one carve of a plate standing in the
column (wall clock around the call, which ends with the stream drained).  Then dam_pillars_dfsph and breaking_dam_30k_dfsph in lock step, rounds
of `steps` steps timed alternately (host clock around step + synchronize), behind `warm` steps of warm-up: 40 times the run is still a column at
rest, after 2 400 steps (0.6 s) the front has passed the pillars and their samples stand in the particles' lists -- the tool prints how many particles
are within h of the pillars' slice of the tank and how many list a wall sample at all."""
import os
os.environ.setdefault("SPH_DEV", "1")
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cfd_taichi_amd import _native as nat, geometry, scenes  # noqa: E402

steps, rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 20, int(sys.argv[2]) if len(sys.argv) > 2 else 10
warm = int(sys.argv[3]) if len(sys.argv) > 3 else 2400


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, (time.perf_counter() - t0) * 1e3


cfg = scenes.get("breaking_dam_30k_dfsph")
sim = nat.Simulation(nat.config_from_dict(cfg))
sim.step(5)
sim.synchronize()
shell = geometry.box_shell([1.5, 0.05, 0.05], [4.5, 2.0, 1.45], 0.05)
for k in range(3):
    g, t_add = timed(lambda: sim.add_geometry(shell))
    print("add_geometry of %d samples onto %d wall samples: %.2f ms" % (len(shell), sim.n_wall - len(shell), t_add))
    _, t_rm = timed(lambda: sim.remove_geometry(g))
    print("remove_geometry of them: %.2f ms" % t_rm)
plate = geometry.plate([0.6, 0.05, 0.05], [0, 2.9, 0], [0, 0, 1.4], 0.05)
g = sim.add_geometry(plate)
n0 = sim.n_fluid
r, t_carve = timed(lambda: sim.carve(g))
print("carve of a plate of %d samples: %d of %d particles removed, %.2f ms" % (len(plate), r, n0, t_carve))
sim.step(2)
assert np.isfinite(sim.download(nat.F_POS)).all()
sim.close()

sims = {}
for name in ("dam_pillars_dfsph", "breaking_dam_30k_dfsph"):
    c = scenes.get(name)
    c["scene"].pop("loads", None)             # the cost of the geometry alone (what measuring loads adds: tools/wall_load_cost.py)
    sims[name] = nat.Simulation(nat.config_from_dict(c), config=c)
    sims[name].step(warm)
    sims[name].synchronize()
res = {n: [] for n in sims}
for _ in range(rounds):
    for n, s in sims.items():
        t0 = time.perf_counter()
        s.step(steps)
        s.synchronize()
        res[n].append((time.perf_counter() - t0) / steps * 1e3)
for n, t in res.items():
    x = sims[n].download(nat.F_POS)[:, 0]
    print("%-24s %6d wall samples  ms/step min %.3f median %.3f  (after %d steps: %d particles with 1.9 < x < 2.3, %d list a wall sample)"
          % (n, sims[n].n_wall, min(t), statistics.median(t), warm + steps * rounds, int(((x > 1.9) & (x < 2.3)).sum()), int((sims[n].wall_neighbor_counts() > 0).sum())))
