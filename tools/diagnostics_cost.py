"""What the run diagnostics cost:
    tools/diagnostics_cost.py record SCENE WARM_STEPS   recording on minus off on one build: three handles on SCENE -- off, every = 1, every = 10 --
                                                        advance in lock step (recording changes no bits, so the state they time is the same), rounds of
                                                        AB_CHUNK steps timed in random order, AB_ROUNDS of them
    tools/diagnostics_cost.py call SCENE WARM_STEPS     one sph_diagnostics call between steps, host clock around the call, AB_ROUNDS of them"""
import os
import random
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cfd_taichi_amd import _native as nat, scenes  # noqa: E402


def record(scene, warm):
    chunk, rounds = int(os.environ.get("AB_CHUNK", "20")), int(os.environ.get("AB_ROUNDS", "10"))
    cfg = scenes.get(scene)
    sims = {name: nat.Simulation(nat.config_from_dict(cfg)) for name in ("off", "every1", "every10")}
    sims["every1"].record_diagnostics(1)
    sims["every10"].record_diagnostics(10)
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
    assert all((s.download(nat.F_POS) == sims["off"].download(nat.F_POS)).all() for s in sims.values())
    rows, lost = sims["every1"].diagnostics_log()
    assert len(rows) + lost == warm + chunk * rounds and rows["step"][-1] == warm + chunk * rounds
    for n, t in res.items():
        print("%-24s %-8s ms/step min %.4f median %.4f" % (scene, n, min(t), statistics.median(t)))
    for n in ("every1", "every10"):
        print("%-24s %-8s - off: min %+.2f us, median %+.2f us per step (n = %d)" % (
            scene, n, (min(res[n]) - min(res["off"])) * 1e3, (statistics.median(res[n]) - statistics.median(res["off"])) * 1e3, sims[n].n_fluid))


def call(scene, warm):
    rounds = int(os.environ.get("AB_ROUNDS", "10"))
    sim = nat.Simulation(nat.config_from_dict(scenes.get(scene)))
    sim.step(warm)
    sim.synchronize()
    sim.diagnostics()                     # (the first call allocates the scratch rows)
    t = []
    for _ in range(rounds):
        sim.step(1)
        sim.synchronize()
        t0 = time.perf_counter()
        row = sim.diagnostics()
        t.append((time.perf_counter() - t0) * 1e6)
    print("%-24s one sph_diagnostics call: min %.1f us, median %.1f us (n = %d, kinetic energy %.6g J)" % (scene, min(t), statistics.median(t), sim.n_fluid, row["kinetic"]))


if __name__ == "__main__":
    {"record": record, "call": call}[sys.argv[1]](sys.argv[2], int(sys.argv[3]))
