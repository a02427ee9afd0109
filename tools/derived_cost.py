"""What one sph_derived call costs:
    tools/derived_cost.py scene [warm_steps] [calls]
Per call, after one solver step (so that the call has to re-sort, rebuild the lists and recompute the densities): the host clock around
Simulation.derived("vorticity"), min / median over `calls`; then the same calls with HIP-event profiling on, split into the sort + list build, the
density sweep (the same run's k_density), the new sweep (profile id `derived`: pack + k_derived) and the transfer (un-sort); and the host clock of a
second call on the unchanged state (the un-sort and the copy alone)."""
import os
os.environ.setdefault("SPH_DEV", "1")
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cfd_taichi_amd import _native as nat, scenes  # noqa: E402

scene = sys.argv[1]
warm = int(sys.argv[2]) if len(sys.argv) > 2 else 20
calls = int(sys.argv[3]) if len(sys.argv) > 3 else 10
sim = nat.Simulation(nat.config_from_dict(scenes.get(scene)))
sim.step(warm)
sim.derived("vorticity")               # the feature's memory, outside the timed region
sim.synchronize()

first, again = [], []
for _ in range(calls):
    sim.step(1)
    sim.synchronize()
    t0 = time.perf_counter()
    sim.derived("vorticity")
    first.append((time.perf_counter() - t0) * 1e3)
    t0 = time.perf_counter()
    sim.derived("cover")
    again.append((time.perf_counter() - t0) * 1e3)

LISTS = ("hash_count", "scan", "scatter", "order_gather", "build_nl", "rigid")
DENSITY = ("wcsph_density", "dfsph_density_alpha", "pbf_lambda")
sim.profile_enable(True)
split = {"lists": [], "density": [], "derived": [], "transfer": [], "other": []}
for _ in range(calls):
    sim.step(1)
    sim.synchronize()
    sim.profile_reset()
    sim.derived("vorticity")
    sim.synchronize()
    prof = sim.profile()
    row = {k: 0.0 for k in split}
    for name, (ms, _n) in prof.items():
        key = "lists" if name in LISTS else "density" if name in DENSITY else name if name in ("derived", "transfer") else "other"
        row[key] += ms
    for k in split:
        split[k].append(row[k])
sim.profile_enable(False)

print("%s: %d particles, %d calls after one step each" % (scene, sim.n_fluid, calls))
print("  host clock, first call of a state   min %.3f ms  median %.3f ms" % (min(first), statistics.median(first)))
print("  host clock, second call (cached)    min %.3f ms  median %.3f ms" % (min(again), statistics.median(again)))
for k in ("lists", "density", "derived", "transfer", "other"):
    print("  device, %-9s min %.3f ms  median %.3f ms" % (k, min(split[k]), statistics.median(split[k])))
sim.close()
