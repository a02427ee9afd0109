"""Scenes and helpers of the inlet / sink suites (TEST INFRASTRUCTURE: test_particle_flow_cpu.py and test_particle_flow_gpu.py; nothing here
loads the HIP library; the generic helpers are tests/harness.py's).

The yardstick is the equivalence that sph_add_particles / sph_remove_in_box promise: a handle whose particles arrived
or left between steps computes, bit for bit, what a fresh oracle (or, under the relaxed arithmetic, a fresh handle) holding the same particles
under the same ids computes.  The lattice index of the reference runs x, then z, then y (ParticleSystem.py:142-151), so a column of more layers
begins with the particles of the shorter column and continues with whole layers of 8 x 8 = 64: "the short lattice plus the top layers of the
tall one, appended" IS the tall lattice, id for id.

Shapes: the tiny wall / clamp scenes (particle_radius 0.025, lattice 8 x ny x 8) with water_size[1] 0.5, 0.55, 0.65 -> 640, 704, 832
particles (0.6 and 0.7 give 767 and 895 through the f64 rounding of ParticleSystem.py:85-86).  640 -> 832 crosses a wave boundary (704), a
256-block boundary (768) and odd counts on the way (the calls add 37, 27, 64, 64).
"""
import copy

import numpy as np

from cfd_taichi_amd import _native as nat
from cfd_taichi_amd import scenes
from harness import fluid_state, oracle_step, same_bits, same_stats
from oracle import oracle as orc

SOLVERS = ("wcsph", "dfsph", "pcisph", "iisph", "pbf")
DT = {"dfsph": 1e-3, "wcsph": 2.5e-4, "pcisph": 1e-3, "iisph": 1e-3, "pbf": 2.5e-4}       # as the tiny scenes of scenes.SCENES set it
HEIGHTS = {640: 0.5, 704: 0.55, 832: 0.65}
ADD_CALLS = (37, 27, 64, 64)                  # 640 -> 677 -> 704 -> 768 -> 832
D = 0.05                                      # particle diameter of the tiny scenes


def config(solver, walls, n, capacity=0):
    """the tiny wall ("wall") or clamp ("clamp") scene with `solver` and the column of `n` particles; capacity > 0: fluid.capacity"""
    cfg = copy.deepcopy(scenes.get("dfsph_tiny_wall" if walls == "wall" else "dfsph_tiny_clamp"))
    cfg["solver"]["name"] = solver
    cfg["solver"]["delta_time"] = DT[solver]
    cfg["fluid"]["water_size"][1] = HEIGHTS[n]
    if capacity:
        cfg["fluid"]["capacity"] = int(capacity)
    return cfg


# the threshold pair: a lattice of 32 x ny x 32 at radius 0.01 just under 65 536 particles (quad sweeps, nine-wave list build) and two layers
# taller (plain sweeps, three-wave list build)
THRESHOLD = {64512: 1.26, 66560: 1.30}


def threshold_config(solver, n, capacity=0):
    cfg = copy.deepcopy(scenes.get("dfsph_tiny_wall"))
    cfg["scene"]["particle_radius"] = 0.01
    cfg["scene"]["box_max"] = [0.8, 1.6, 0.8]
    cfg["solver"]["name"] = solver
    cfg["solver"]["delta_time"] = DT[solver]
    cfg["fluid"]["start_pos"] = [0.08, 0.08, 0.08]
    cfg["fluid"]["water_size"] = [0.64, THRESHOLD[n], 0.64]
    if capacity:
        cfg["fluid"]["capacity"] = int(capacity)
    return cfg


def same_state(sim, o, solver, when):
    """every field fluid_state names, plus rho (harness.same_bits)"""
    a, b = fluid_state(sim, solver), fluid_state(o, solver)
    for k in a:
        same_bits(np.float32(a[k]), np.float32(b[k]), "%s: %s" % (when, k))
    same_bits(sim.download(nat.F_RHO), o.get(orc.F_RHO), "%s: rho" % when)


def same_nbr_count(sim, o, when):
    """SPH_F_NBR_COUNT of the positions both sides hold now (re-sorts the handle: the last comparison of a run)"""
    sim.build_neighbors()
    o.build_grid(); o.compute_nbr_count()
    same_bits(sim.download(nat.F_NBR_COUNT), o.get(orc.F_NBR_COUNT), "%s: neighbour count" % when)


def lockstep(sim, o, solver, steps, when, every=5, count=True):
    """`steps` steps of the handle and the oracle: the statistics of every step, the state every few steps and at the end; count: then the
    neighbour count (it re-sorts the handle, after which the last step's pressures -- iisph's carried scalar as fluid_state reads it -- are no
    longer downloadable: not where the state is taken afterwards)"""
    for s in range(steps):
        st = sim.step(1)
        ot = oracle_step(o, solver)
        same_stats(st, ot, solver, "%s, step %d: statistics" % (when, s + 1))
        if (s + 1) % every == 0 or s + 1 == steps:
            same_state(sim, o, solver, "%s, step %d" % (when, s + 1))
    if count:
        same_nbr_count(sim, o, when + ", the end")


def inner_box(cfg):
    """a box inside the column of the 640 lattice: 4 x 4 columns of the 8 x 8, the two layers that start 0.2 above the column's foot"""
    sx, sy, sz = (np.float32(v) for v in cfg["fluid"]["start_pos"])
    lo = np.float32([sx + 0.075, sy + 0.175, sz + 0.075])
    hi = np.float32([sx + 0.275, sy + 0.275, sz + 0.275])
    return lo, hi


def in_box(pos, lo, hi):
    """the sink's test, in f32 like the device's"""
    pos = np.asarray(pos, dtype=np.float32)
    return ((pos >= np.float32(lo)) & (pos < np.float32(hi))).all(axis=1)


def layer_above(cfg, n, r):
    """r positions of the 8 x 8 lattice one diameter of clearance above the top layer of the column of n particles"""
    sx, sy, sz = cfg["fluid"]["start_pos"]
    layers = n // 64
    ix, iz = np.meshgrid(np.arange(8), np.arange(8), indexing="xy")
    pos = np.stack([sx + D * ix.reshape(-1), np.full(64, sy + D * (layers + 1)), sz + D * iz.reshape(-1)], axis=1)
    return pos[:r].astype(np.float32)


class FakeSim:
    """what cfd_taichi_amd.emitter needs of a simulation, with a scripted clock"""

    def __init__(self, n_fluid, capacity):
        self.n_fluid, self.capacity, self.t = n_fluid, capacity, 0.0
        self.added, self.boxes, self.clock_reads = [], [], 0
        self.in_box = 0

    def time(self):
        self.clock_reads += 1
        return self.t

    def add_particles(self, pos, vel=None):
        assert pos.dtype == np.float32 and pos.ndim == 2 and pos.shape[1] == 3 and self.n_fluid + len(pos) <= self.capacity
        first = self.n_fluid
        self.added.append((self.t, pos.copy(), None if vel is None else np.asarray(vel).copy()))
        self.n_fluid += len(pos)
        return first

    def remove_in_box(self, lo, hi):
        self.boxes.append((np.asarray(lo).copy(), np.asarray(hi).copy()))
        self.n_fluid -= self.in_box
        return self.in_box
