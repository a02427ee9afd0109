"""What the adaptive time step of wcsph / pcisph / iisph / pbf costs and buys:
    tools/adaptive_dt_cost.py launches SCENE WARM_STEPS   the two launches per step: two handles of one build on SCENE, one with the rule on and both
                                                          bounds at the configured step (dt is then the configured step bit for bit, both handles do the
                                                          same work), rounds of AB_CHUNK steps timed in random order, AB_ROUNDS of them
    tools/adaptive_dt_cost.py dam                         dam_adaptive_iisph to t = 1.0 s against breaking_dam_30k_iisph at its fixed 2.5e-4: steps,
                                                          pressure iterations, wall time"""
import os
import random
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cfd_taichi_amd import _native as nat, scenes  # noqa: E402


def launches(scene, warm):
    chunk, rounds = int(os.environ.get("AB_CHUNK", "20")), int(os.environ.get("AB_ROUNDS", "10"))
    cfg = scenes.get(scene)
    dt = cfg["solver"]["delta_time"]
    sims = {"off": nat.Simulation(nat.config_from_dict(cfg)), "on": nat.Simulation(nat.config_from_dict(cfg))}
    for name, value in (("step_max_dt", dt), ("step_min_dt", dt), ("step_adaptive_dt", 1)):
        sims["on"].set_param(name, value)
    for s in sims.values():
        s.step(warm)
        s.synchronize()
    res = {n: [] for n in sims}
    order = list(sims)
    for _ in range(rounds):
        random.shuffle(order)
        for n in order:
            t0 = time.perf_counter()
            sims[n].step(chunk)
            sims[n].synchronize()
            res[n].append((time.perf_counter() - t0) / chunk * 1e3)
    assert sims["on"].time() == sims["off"].time() and (sims["on"].download(nat.F_POS) == sims["off"].download(nat.F_POS)).all()
    for n, t in res.items():
        print("%-24s %-4s ms/step min %.4f median %.4f" % (scene, n, min(t), statistics.median(t)))
    print("%-24s on - off: min %+.2f us, median %+.2f us per step (n = %d)" % (
        scene, (min(res["on"]) - min(res["off"])) * 1e3, (statistics.median(res["on"]) - statistics.median(res["off"])) * 1e3, sims["on"].n_fluid))


def dam():
    for name in ("dam_adaptive_iisph", "breaking_dam_30k_iisph"):
        cfg = scenes.get(name)
        sim = nat.Simulation(nat.config_from_dict(cfg), config=cfg)
        steps, iters, dts = 0, 0, set()
        t0 = time.perf_counter()
        try:
            while sim.time() <= 1.0 and steps < 20000:
                for _ in range(10):
                    st = sim.step(1)
                    iters += st.n_dens
                    dts.add(float(st.dt))
                steps += 10
            sim.synchronize()
            wall = time.perf_counter() - t0
            ok = bool(np.isfinite(sim.download(nat.F_POS)).all()) and sim.last_stats.lost == 0
            print("%-24s t = %.6f s after %d steps, %d pressure iterations, wall %.2f s, dt %.3e .. %.3e, finite and none lost: %s" % (
                name, sim.time(), steps, iters, wall, min(dts), max(dts), ok))
        except nat.SphError as e:
            print("%-24s stopped after %d steps at t = %.6f s: %s" % (name, steps, sim.time(), e))
        sim.close()


if __name__ == "__main__":
    if sys.argv[1] == "launches":
        launches(sys.argv[2], int(sys.argv[3]))
    else:
        dam()
