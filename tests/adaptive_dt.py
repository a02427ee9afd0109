"""The adaptive time step of wcsph / pcisph / iisph / pbf, restated (TEST INFRASTRUCTURE: test_adaptive_dt_cpu.py and test_adaptive_dt_gpu.py;
nothing here imports the HIP library).

The rule is dfsph's (dfsph_solver.py:104-119), applied at the head of a step to the velocities the step starts with, in f32 without contraction:

    vmax = max_i sqrtf((vx vx + vy vy) + vz vz)  [+ the body's term, :104-110, if a body is binned]
    m    = f32(0.4 * particle_radius * 2) / vmax * 0.2f           (vmax = 0: +inf)
    dt   = max_dt if m > max_dt else max(m, min_dt)

The oracle has no such rule outside dfsph; it is driven with Oracle.set_dt(dt_k), which writes delta_time, delta_time_2 and ps.delta_time for every
solver.  pcisph's delta belongs to the time step of construction (pcisph_solver.py:23, :47), so a pcisph step under dt_k is taken by a FRESH oracle
constructed with solver.delta_time = float(dt_k) and handed the positions and velocities.

Scenes: the 640-particle tiny wall / clamp scenes of tests/particle_flow.py, its DT table, velocities rng(7).uniform(-1, 1, (N, 3)) * A."""
import copy

import numpy as np

import harness as h
import particle_flow as pf
from oracle import oracle as orc

F = np.float32
SOLVERS = ("wcsph", "pbf", "iisph", "pcisph")
AMPLITUDE = {"wcsph": 10.0, "pbf": 10.0, "iisph": 2.5, "pcisph": 2.5}
STEPS = 8
RADIUS = 0.025
P_ADAPTIVE, P_MAX_DT, P_MIN_DT = 77, 78, 79          # SPH_P_STEP_ADAPTIVE_DT, SPH_P_STEP_MAX_DT, SPH_P_STEP_MIN_DT


def bounds(solver):
    """(max_dt, min_dt) of the lockstep cases: twice and a quarter of the configured step"""
    return 2 * pf.DT[solver], pf.DT[solver] / 4


def velocities(n, amplitude, seed=7):
    return (np.random.default_rng(seed).uniform(-1, 1, (n, 3)) * amplitude).astype(np.float32)


def vmax_of(vel):
    v = np.asarray(vel, dtype=np.float32)
    if len(v) == 0:
        return F(0)
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    return F(np.sqrt((x * x + y * y) + z * z).max())           # f32 products and sums, each rounded; sqrt correctly rounded


def rigid_term(rigid_pos, centroid, vel, omega):
    """max over the body's samples of |vel| + |omega x (x - centroid)|          dfsph_solver.py:104-110.  A NaN term (an unbinned body's centroid)
    never exceeds the running maximum, which starts at 0"""
    p, c, v, w = (np.asarray(a, dtype=np.float32) for a in (rigid_pos, centroid, vel, omega))
    vn = F(np.sqrt(F(F(v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])))
    rx, ry, rz = p[:, 0] - c[0], p[:, 1] - c[1], p[:, 2] - c[2]
    cx, cy, cz = w[1] * rz - w[2] * ry, w[2] * rx - w[0] * rz, w[0] * ry - w[1] * rx
    t = vn + np.sqrt((cx * cx + cy * cy) + cz * cz)
    t = t[~np.isnan(t)]
    return F(max(F(0), t.max())) if len(t) else F(0)


def rule(vel, max_dt, min_dt, radius=RADIUS, rigid=F(0)):
    """dt_k of a step that starts with the velocities `vel`, as an f32"""
    vmax = F(vmax_of(vel) + F(rigid))
    with np.errstate(divide="ignore"):
        m = F(F(F(0.4 * radius * 2) / vmax) * F(0.2))
    if m > F(max_dt):
        return F(max_dt)
    return max(m, F(min_dt))


def pcisph_delta(s_sum, dt, radius=RADIUS):
    """delta = 1 / (S * (float)beta(dt)), beta folded in f64 from (double)dt             pcisph_solver.py:23, :47"""
    m = 1000 * (radius * radius * radius) * 8
    dtf = float(F(dt))
    beta = dtf * dtf * m * m * 2 / float(1000 * 1000)
    return F(1.0) / F(F(s_sum) * F(beta))


def with_dt(cfg, dt):
    c = copy.deepcopy(cfg)
    c["solver"]["delta_time"] = float(dt)
    return c


def oracle_step_dt(o, cfg, solver, dt):
    """one oracle step under the time step dt.  Returns (the oracle to go on with, the step's statistics): pcisph moves to a fresh oracle
    constructed with delta_time = dt, every other solver keeps its oracle and gets set_dt(dt)"""
    if solver == "pcisph":
        st = h.fluid_state(o, solver)
        o.close()
        o = h.give(h.make_oracle(with_dt(cfg, dt)), st, solver)
        assert F(o.dt) == F(dt)
    else:
        o.set_dt(float(dt))
    return o, h.oracle_step(o, solver)


def oracle_run(solver, walls, steps=STEPS):
    """the lockstep case on the oracle alone.  Returns (dt_1 .. dt_steps, the final oracle)"""
    cfg = pf.config(solver, walls, 640)
    o = h.make_oracle(cfg)
    o.set(orc.F_VEL, velocities(o.N, AMPLITUDE[solver]))
    max_dt, min_dt = bounds(solver)
    dts = []
    for _ in range(steps):
        dt = rule(o.get(orc.F_VEL), max_dt, min_dt)
        o, _ = oracle_step_dt(o, cfg, solver, dt)
        dts.append(dt)
    return dts, o
