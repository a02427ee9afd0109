"""What the carried scalar costs per step:
    tools/scalar_cost.py scene [warm_steps] [rounds] [chunk]
Two handles of one build on the same scene, one with the scalar enabled (D > 0, beta > 0, a two-valued T), one without; rounds of `chunk` steps are
timed on the host clock in alternation (min / median per step).  Then `rounds` single steps of the enabled handle with HIP-event profiling on: the
profile id `scalar` (pack + k_scalar_rate) against the same run's density sweep, and `finalize` (which holds k_scalar_advance) on both handles."""
import os
os.environ.setdefault("SPH_DEV", "1")
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cfd_taichi_amd import _native as nat, scenes  # noqa: E402

scene = sys.argv[1]
warm = int(sys.argv[2]) if len(sys.argv) > 2 else 20
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 10
chunk = int(sys.argv[4]) if len(sys.argv) > 4 else 20
sims = {name: nat.Simulation(nat.config_from_dict(scenes.get(scene))) for name in ("off", "on")}
x = sims["on"].download(nat.F_POS)[:, 0]
sims["on"].enable_scalar(1e-4, 0.05, 0.5, values=(x > np.median(x)).astype(np.float32))
for s in sims.values():
    s.step(warm)
    s.synchronize()

host = {name: [] for name in sims}
for r in range(rounds):
    for name in (("off", "on") if r % 2 == 0 else ("on", "off")):
        t0 = time.perf_counter()
        sims[name].step(chunk)
        sims[name].synchronize()
        host[name].append((time.perf_counter() - t0) / chunk * 1e3)

DENSITY = ("wcsph_density", "dfsph_density_alpha", "pbf_lambda")
split = {name: {"scalar": [], "density": [], "finalize": [], "all": []} for name in sims}
for name, s in sims.items():
    s.profile_enable(True)
    for _ in range(rounds):
        s.profile_reset()
        s.step(1)
        s.synchronize()
        prof = s.profile()
        split[name]["scalar"].append(prof.get("scalar", (0.0, 0))[0])            # (profile() lists what ran: nothing on the handle that is off)
        split[name]["finalize"].append(prof.get("finalize", (0.0, 0))[0])
        split[name]["density"].append(sum(prof[k][0] / prof[k][1] for k in DENSITY if k in prof))      # ONE density sweep (a solver may run it more than once)
        split[name]["all"].append(sum(ms for ms, _n in prof.values()))
    s.profile_enable(False)

n = sims["on"].n_fluid
print("%s: %d particles, %d rounds of %d steps" % (scene, n, rounds, chunk))
for name in ("off", "on"):
    print("  host clock, scalar %-3s  ms/step min %.4f  median %.4f" % (name, min(host[name]), statistics.median(host[name])))
print("  host clock, on - off    ms/step min %+.4f  median %+.4f" % (min(host["on"]) - min(host["off"]), statistics.median(host["on"]) - statistics.median(host["off"])))
for name in ("off", "on"):
    for k in ("scalar", "density", "finalize", "all"):
        print("  device (events, single steps), scalar %-3s %-9s min %.4f ms  median %.4f ms" % (name, k, min(split[name][k]), statistics.median(split[name][k])))
dens = statistics.median(split["on"]["density"])
print("  the `scalar` sweep = %.2f x one density sweep of the same run (medians)" % (statistics.median(split["on"]["scalar"]) / dens if dens else float("nan")))
for s in sims.values():
    s.close()
