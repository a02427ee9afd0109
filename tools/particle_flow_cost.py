"""What SphConfig.fluid_capacity and the two calls on top of it cost, on the GPU:

    python tools/particle_flow_cost.py pitch     # dfsph_1m with capacity 0 and 1.25 M alternating (100 steps after 50), then five
                                                 # add_particles of 1 000 particles and five remove_in_box at 1 M (host clock around each call)
    python tools/particle_flow_cost.py scenes    # config/filling_tank_dfsph.json for 2 400 steps and config/channel_wcsph.json for 12 000:
                                                 # count, emitted, removed, lost, the largest list, every twelfth of the run
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cfd_taichi_amd import _native as nat, scenes  # noqa: E402


def timed_steps(cap, warm=50, steps=100):
    cfg = scenes.get("dfsph_1m")
    if cap:
        cfg["fluid"]["capacity"] = cap
    sim = nat.Simulation(nat.config_from_dict(cfg))
    sim.step(warm); sim.synchronize()
    t0 = time.perf_counter()
    sim.step(steps); sim.synchronize()
    dt = time.perf_counter() - t0
    n = sim.n_fluid
    print("dfsph_1m capacity %d: n %d cap %d, %d steps %.4f s, %.3f ms/step, %.1f Mparticle-steps/s, overrides %s" % (cap, n, sim.capacity, steps, dt, 1e3 * dt / steps, n * steps / dt / 1e6, sim.overrides()), flush=True)
    return sim


if sys.argv[1] == "pitch":
    keep = None
    for rnd in range(3):
        for cap in (0, 1250000):
            s = timed_steps(cap)
            if cap and rnd == 2:
                keep = s
            else:
                s.close()
    sim = keep
    ix, iz = np.meshgrid(np.arange(32), np.arange(32))
    for k in range(5):
        pos = np.stack([6.0 + 0.05 * ix.reshape(-1), np.full(1024, 5.6 + 0.05 * k), 0.5 + 0.05 * iz.reshape(-1)], 1)[:1000].astype(np.float32)
        vel = np.zeros_like(pos)
        sim.synchronize(); t0 = time.perf_counter(); sim.add_particles(pos, vel); t1 = time.perf_counter()
        print("add_particles(1000) at n %d: %.1f us" % (sim.n_fluid, 1e6 * (t1 - t0)), flush=True)
    for k in range(5):
        lo, hi = [6.0, 5.59 + 0.05 * k, 0.0], [8.0, 5.61 + 0.05 * k, 5.2]
        sim.synchronize(); t0 = time.perf_counter(); r = sim.remove_in_box(lo, hi); t1 = time.perf_counter()
        print("remove_in_box at n %d removed %d: %.1f us" % (sim.n_fluid + r, r, 1e6 * (t1 - t0)), flush=True)
    t0 = time.perf_counter(); r = sim.remove_in_box([15.5, 6.5, 5.0], [15.6, 6.6, 5.1]); t1 = time.perf_counter()
    print("remove_in_box at n %d removed %d (nothing in the box): %.1f us" % (sim.n_fluid, r, 1e6 * (t1 - t0)), flush=True)
    st = sim.step(5)
    print("5 steps after: n_dens %d lost %d n %d" % (st.n_dens, st.lost, sim.n_fluid), flush=True)
else:
    from cfd_taichi_amd import emitter, ParticleSystem
    import importlib
    for name, frames in (("filling_tank_dfsph", 2400), ("channel_wcsph", 12000)):
        cfg = scenes.get(name)
        ps = ParticleSystem(cfg)
        solver = getattr(importlib.import_module("cfd_taichi_amd.%s_solver" % cfg["solver"]["name"]), cfg["solver"]["name"] + "_solver")(ps, cfg)
        ems, sinks = emitter.from_config(cfg)
        t0 = time.perf_counter()
        try:
            for f in range(frames):
                solver.step()
                emitter.apply(ps._sim, ems, sinks)
                if (f + 1) % (frames // 12) == 0:
                    pos = ps.fluid_particles.pos.to_numpy()
                    st = ps._sim.last_stats
                    print("%s frame %d t %.4f n %d emitted %d removed %d exhausted %s lost %d max_nbrs %d n_dens %d ymax %.3f finite %s inside %s" % (
                        name, f + 1, ps._sim.time(), ps.particle_num, ems[0].emitted, sum(s.removed for s in sinks), ems[0].exhausted, st.lost, st.max_nbrs, st.n_dens,
                        float(pos[:, 1].max()), bool(np.isfinite(pos).all()), bool(((pos >= 0) & (pos <= np.float32(cfg["scene"]["box_max"]))).all())), flush=True)
        except nat.SphError as e:
            print("%s: SphError at frame %d: %s" % (name, f + 1, e), flush=True)
        print("%s: %d frames in %.2f s" % (name, f + 1, time.perf_counter() - t0), flush=True)
