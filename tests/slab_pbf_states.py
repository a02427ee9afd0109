"""Scenes and input states of the sharded-PBF tests (tests/test_slab_pbf_cpu.py, tests/test_slab_pbf_gpu.py, tests/slab_pbf_worker.py).

From rest a PBF column barely moves in 60 steps: nothing migrates between slabs and the lambda halo carries zeros.  So the sharded runs start
from a state that loads every part of the slab path --

  scene "long"   solver pbf, delta_time 2.5e-4, particle_radius 0.025, box [0, 0, 0] - [2.0, 0.6, 0.6], water_size [1.6, 0.3, 0.3] at
                 start_pos [0.1, 0.1, 0.1]: N = 1151 particles in 15 fluid cell columns of a 21-column grid, so four slabs all hold fluid;
                 "long_wall" with wall particles, "long_clamp" with boundary_handle false (the clamp planes of pbf_solver.py:73-81)
  state(seed)    the oracle's lattice scaled by 0.92 about its centroid, plus uniform(-0.15 d, 0.15 d) per coordinate (d = 0.05), velocities
                 uniform(-0.5, 0.5) per component drawn after the positions, plus 6 m/s on x; in f64, rounded to f32 once -- the same bits for
                 every participant.  The drift carries ~20 particles across every column boundary in 60 steps; the compression switches the
                 density constraint on for ~40 % of the particles from the first step.

tests/test_slab_pbf_cpu.py shows on the f32 oracle alone that these inputs are fair.  The recipe is narrow: a compression of 0.90 sends seed 3
out of the box on long_wall, a drift of -4 m/s sends seed 1 out, +4 m/s crosses some boundaries with 2-8 particles only.

TEST INFRASTRUCTURE ONLY: nothing here imports the HIP library."""
import copy
import functools

import numpy as np

from cfd_taichi_amd import scenes

from oracle.oracle import F_PBF_DELTA_POS, F_PBF_LAMBDA, F_POS, F_RHO, F_VEL  # noqa: E402,F401  (the library shares the ids)
FIELDS = (("pos", F_POS), ("vel", F_VEL), ("rho", F_RHO), ("pbf_lambda", F_PBF_LAMBDA), ("delta_pos", F_PBF_DELTA_POS))
SEEDS = (1, 3)
STEPS = 60
N_LONG = 1151
COMPRESSION, JITTER, DRIFT_X = 0.92, 0.15, 6.0


def config(name):
    """long_wall / long_clamp, or any scene of cfd_taichi_amd.scenes"""
    if name not in ("long_wall", "long_clamp"):
        return scenes.get(name)
    c = copy.deepcopy(scenes.get("pbf_tiny_wall"))
    c["solver"]["name"] = "pbf"
    c["solver"]["delta_time"] = 2.5e-4
    c["solver"]["boundary_handle"] = name == "long_wall"
    c["scene"]["particle_radius"] = 0.025
    c["scene"]["box_min"] = [0.0, 0.0, 0.0]
    c["scene"]["box_max"] = [2.0, 0.6, 0.6]
    c["fluid"]["water_size"] = [1.6, 0.3, 0.3]
    c["fluid"]["start_pos"] = [0.1, 0.1, 0.1]
    return c


def support_radius(cfg):
    return 4.0 * float(cfg["scene"]["particle_radius"])


@functools.lru_cache(maxsize=None)
def state(name, seed):
    """(pos, vel) as read-only f32 arrays"""
    from oracle import oracle as orc
    cfg = config(name)
    o = orc.Oracle(cfg, num_threads=1)
    lat = o.get(orc.F_POS).astype(np.float64)
    o.close()
    d = 2.0 * float(cfg["scene"]["particle_radius"])
    rng = np.random.default_rng(seed)
    c = lat.mean(0)
    pos = c + (lat - c) * COMPRESSION + rng.uniform(-JITTER * d, JITTER * d, lat.shape)
    vel = rng.uniform(-0.5, 0.5, lat.shape)
    vel[:, 0] += DRIFT_X
    pos, vel = np.ascontiguousarray(pos, dtype=np.float32), np.ascontiguousarray(vel, dtype=np.float32)
    pos.setflags(write=False); vel.setflags(write=False)
    return pos, vel


def snapshot(get):
    res = {name: np.array(get(f)) for name, f in FIELDS}
    for a in res.values():
        a.setflags(write=False)
    return res


@functools.lru_cache(maxsize=None)
def oracle_run(name, seed, steps=STEPS, keep=(1, STEPS)):
    """The f32 oracle from state(name, seed): {step: fields} for the steps in `keep`, plus "pos_path" = the positions after every step
    (steps + 1 entries, the input first).  Computed once, shared, never written to."""
    from oracle import oracle as orc
    cfg = config(name)
    pos, vel = state(name, seed)
    o = orc.Oracle(cfg, num_threads=8, precision="f32")
    o.set(orc.F_POS, pos); o.set(orc.F_VEL, vel)
    out, path, speed = {}, [np.array(pos)], 0.0
    for s in range(1, steps + 1):
        o.step_pbf(1)
        path.append(np.array(o.get(orc.F_POS)))
        speed = max(speed, float(np.sqrt((o.get(orc.F_VEL).astype(np.float64) ** 2).sum(1)).max()))
        if s in keep:
            out[s] = snapshot(o.get)
    o.close()
    out["pos_path"] = path
    out["max_speed"] = speed
    return out


def columns(cfg, pos):
    """cell column of every particle (the reference's floor(x / h))"""
    return np.floor(np.asarray(pos, dtype=np.float32) / np.float32(support_radius(cfg))).astype(np.int64)[:, 0]


def clamp_plane_hits(cfg, pos):
    """coordinates sitting exactly on a clamp plane box_min + r / box_max - r (as the f32 participants form it)"""
    sc = cfg["scene"]
    r = np.float32(sc["particle_radius"])
    pos = np.asarray(pos, dtype=np.float32)
    n = 0
    for a in range(3):
        n += int((pos[:, a] == np.float32(np.float32(sc["box_min"][a]) + r)).sum()) + int((pos[:, a] == np.float32(np.float32(sc["box_max"][a]) - r)).sum())
    return n
