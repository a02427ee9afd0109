"""The yardstick of the wall-load suites (TEST INFRASTRUCTURE: test_wall_load_cpu.py, test_wall_load_gpu.py; numpy f32, nothing here loads the
HIP library).

DESIGN.md section 6m: during a step every wall sample b collects f_b, the reaction to what the fluid feels from it.  Pair by pair that is the
expression the reference deposits on a rigid body's sample with V_b in place of the sample's volume, written here from the reference's lines:

  wcsph   once per step     ret = - V_b p_i / rho_i^2 gradW rho_0,  f += - ret m                        wcsph_solver.py:124-126
  dfsph   once per executed density iteration (iter_all_vel_adv)
                            k_i = (rho_adv_i - rho_0) alpha_i / dt^2, ret = V_b rho_0 k_i / rho_i gradW,  f += ret m       dfsph_solver.py:208-212
  pcisph  once, behind the loop, from the press_iter the last update_press_force read
                            ret = V_b rho_0 press_iter_i gradW / rho_i^2,  f += ret m                   pcisph_solver.py:185-186
  iisph   once, behind the loop, from the final p_iter
                            force = V_b rho_0 / rho_i^2 gradW p_iter_i,  f += force m                   iisph_solver.py:158-159

gradW = cubic_kernel_derivative(x_i - x_b).  The pairs (i, b) are those in which fluid particle i lists b; a sample's sum starts at zero per
event, runs in f32 in the order of the sample's own cell walk -- Neighbours(sc, wall_pos, pos, same=False): dx outermost, ascending particle
index inside a cell -- and is then added to the sample's f32 total of the step (`force[3 o] += fx`).  The divergence loop's wall impulses are not
counted, as the reference does not count them for a body.  pcisph deviates from the body's rule on purpose: the reference deposits on a body in
EVERY iteration from a pressure that accumulates, several times the force the fluid receives; a measurement counts the pressure behind the
press_force the integration applies, once (test_wall_load_cpu.py shows by action and reaction that this is the right one).

LoadSolver wraps the second restatement's Solver, imported unchanged, and measures EVERY wall sample: a test takes the rows of the groups it
selected.  Beside f_b every step records the fluid's side -- the wall force the restatement itself applies to the particles, from its own
_wall_sum -- for the action-and-reaction test, and sum |pair terms| for the bounds.

The test state (`pressed`): from rest almost no wall sample sees pressure (the reference's density has no self term and p clamps at zero), so the
tiny wall scenes get geometry_ref.CARVE_PLATE, are carved at clearance d (480 of 640 particles remain), squeezed in x towards the plate, jittered
by up to 0.1 d per coordinate and given velocities within 0.2 m/s per component, all from default_rng(7)."""
import functools
from fractions import Fraction

import numpy as np

import geometry_ref as gr
from second_restatement import F, Neighbours, Solver, _ipow, cubic_kernel_derivative

D = gr.D
PLATE_X = 0.225
PLATE_CENTRE = (0.225, 0.325, 0.25)        # of CARVE_PLATE: y = 0.05 .. 0.60, z = 0.05 .. 0.45


class LoadSolver(Solver):
    def prologue(self):
        """the grid of the step, and on it the samples' own walk over the fluid"""
        super().prologue()
        wp = self.sc.wall_pos
        self.pos_step = self.pos.copy()
        self.ns = Neighbours(self.sc, wp, self.pos, same=False) if self.walls else None
        self.f_b = np.zeros((len(wp), 3), dtype=F)                  # the step's totals start at zero
        self.abs_terms = 0.0                                        # sum over pairs and components of |term|, all events of the step
        self.fluid_force = np.zeros((self.N, 3), dtype=np.float64)  # what the restatement's own wall sums apply to the particles, as a force
        self.events = 0

    # ---- one event: every sample's sum over its fluid neighbours in walk order, then `force += sum` ----
    def _deposit(self, term):
        """term(i) -> (Nb, 3) f32: the pair term of every sample b with fluid particle i[b]"""
        acc = np.zeros_like(self.f_b)
        for k in range(self.ns.kmax):
            live = k < self.ns.count
            t = term(self.ns.index[:, k]).astype(F)
            acc = np.where(live[:, None], acc + t, acc)
            self.abs_terms += float(np.abs(t[live].astype(np.float64)).sum())
        self.f_b = self.f_b + acc
        self.events += 1

    def _grad(self, i):
        return cubic_kernel_derivative(self.pos_step[i] - self.sc.wall_pos, self.h)          # q = x_i - x_b

    def _fluid_side(self, wall_term, scale):
        """the restatement's own sum over a particle's wall neighbours (its _wall_sum, at the positions of the step), times `scale`: the force on
        every particle from the walls in this event"""
        keep, self.pos = self.pos, self.pos_step
        try:
            self.fluid_force += (scale(self._wall_sum((3,), wall_term))).astype(np.float64)
        finally:
            self.pos = keep

    def _correct(self, k, vel, gate, force=False):
        """dfsph: iter_all_vel_adv is the one correction that deposits (force=True), once per executed density iteration"""
        if force and self.walls:
            V, rho = self.sc.wall_vol, self.rho
            self._deposit(lambda i: ((V * self.rho_0 * k[i] / rho[i])[:, None] * self._grad(i)) * self.m)                      # :211-212
            # the fluid's side: v -= (a + b rho_0) dt with b = sum_w V_w k / rho gradW  (second_restatement._correct)
            self._fluid_side(lambda w: (V[w] * k / rho)[:, None] * self.grad_w(w), lambda b: (F(0.0) - b * self.rho_0) * self.m)
        return super()._correct(k, vel, gate, force)

    def step(self):
        super().step()
        if not self.walls or self.name == "dfsph":
            return
        V, rho = self.sc.wall_vol, self.rho
        rho_2 = _ipow(rho, 2)
        if self.name == "wcsph":
            p = self.pressure
            self._deposit(lambda i: (-((((-V) * p[i] / rho_2[i])[:, None] * self._grad(i)) * self.rho_0)) * self.m)            # :124, :126
            self._fluid_side(lambda b: F(0.0) - (V[b] * p / rho_2)[:, None] * self.grad_w(b), lambda s: (s * self.rho_0) * self.m)      # bacc, as an m a
        elif self.name == "pcisph":
            p = self.press_iter                                                                                                 # the last iter_press
            self._deposit(lambda i: ((V * self.rho_0 * p[i])[:, None] * self._grad(i) / rho_2[i][:, None]) * self.m)           # :185-186
            self._fluid_side(lambda b: F(0.0) - (V[b] * p / rho_2)[:, None] * self.grad_w(b), lambda s: s * self.rho_0 * self.m)      # update_press_force's ba
        else:
            p = self.p_iter
            self._deposit(lambda i: ((V * self.rho_0 / rho_2[i])[:, None] * self._grad(i) * p[i][:, None]) * self.m)           # :158-159
            # f_press = (d_ij + d_ii p) m / dt^2, the walls' part of d_ii = db rho_0 dt^2 with db = sum_w - V_w / rho^2 gradW
            self._fluid_side(lambda w: ((-V[w]) / (rho * rho))[:, None] * self.grad_w(w), lambda db: (db * self.rho_0) * p[:, None] * self.m)


# ---- the pressed state ------------------------------------------------------------------------------------------------------------------
def pressed_solver(solver, cls=LoadSolver):
    """steps 1-5 of the state on the restatement: (solver object, Walls, plate group id)"""
    from cfd_taichi_amd import scenes
    cfg = scenes.get(gr.SCENES[solver])
    s = cls(cfg)
    walls = gr.Walls(s)
    gid = walls.add(gr.CARVE_PLATE)
    keep = ~walls.carve_mask(s.pos, gid, F(D))
    gr.keep_rows(s, keep)
    rng = np.random.default_rng(7)
    pos = s.pos.copy()
    pos[:, 0] = F(PLATE_X) + F(0.9) * (pos[:, 0] - F(PLATE_X))
    pos = (pos + rng.uniform(-0.1 * D, 0.1 * D, size=pos.shape).astype(F)).astype(F)
    s.pos = pos
    s.vel = rng.uniform(-0.2, 0.2, size=pos.shape).astype(F)
    return cfg, s, walls, gid


def pressed_state(solver):
    """(cfg, the state as harness.give_sim takes it, n) without stepping anything"""
    cfg, s, _, _ = pressed_solver(solver)
    return cfg, {"pos": s.pos.copy(), "vel": s.vel.copy(), "warm_k": s.warm.copy(), "dt": float(s.dt)}


@functools.lru_cache(maxsize=None)
def run(solver, steps=6, dt0=None):
    """The pressed state stepped `steps` times, once per process (dt0: delta_time as set before the first step, where it is not the scene's -- dfsph
    then takes its first divergence loop under it and moves to its own): a list of per-step records
    {f: (Nb, 3) f32 per-sample forces, dt: the dt the step used, pos / vel: the fluid after the step, fluid: (N, 3) f64, abs, events, kf, ks}
    and the wall set (pos, rows of the plate).  Treat as read-only."""
    cfg, s, walls, gid = pressed_solver(solver)
    if dt0 is not None:
        s.dt = F(dt0)
        s.dt2 = s.dt * s.dt
    state = {"pos": s.pos.copy(), "vel": s.vel.copy(), "warm_k": s.warm.copy(), "dt": float(s.dt)}
    (g, first, count), = walls.info()
    out = []
    with np.errstate(all="ignore"):
        for _ in range(steps):
            s.step()
            out.append({"f": s.f_b.copy(), "dt": float(F(s.dt)), "pos": s.pos.copy(), "vel": s.vel.copy(), "fluid": s.fluid_force.copy(), "abs": s.abs_terms,
                        "events": s.events, "kf": int(s.nw.count.max()), "ks": int(s.ns.count.max()), "n_dens": s.n_dens})
    return {"cfg": cfg, "state": state, "wall_pos": s.sc.wall_pos.copy(), "plate": (first, count), "box": (0, first), "steps": out}


# ---- group sums: exact, and the bound of the device's f64 reduction -------------------------------------------------------------------------
def exact_load(x, f, about=(0.0, 0.0, 0.0)):
    """F = sum f_b and torque = sum (x_b - c) x f_b as exact rationals (x, f: f32 rows; c: doubles), rounded once: (force (3,), torque (3,)) f64"""
    c = [Fraction(float(v)) for v in about]
    Fs, Ts = [Fraction(0)] * 3, [Fraction(0)] * 3
    for xb, fb in zip(np.asarray(x, dtype=np.float64), np.asarray(f, dtype=np.float64)):
        r = [Fraction(float(xb[a])) - c[a] for a in range(3)]
        q = [Fraction(float(v)) for v in fb]
        Fs = [Fs[a] + q[a] for a in range(3)]
        Ts = [Ts[0] + r[1] * q[2] - r[2] * q[1], Ts[1] + r[2] * q[0] - r[0] * q[2], Ts[2] + r[0] * q[1] - r[1] * q[0]]
    return np.array([float(v) for v in Fs]), np.array([float(v) for v in Ts])


def load_terms(x, f, about=(0.0, 0.0, 0.0)):
    """the device's f64 terms, per sample: (n, 3) force terms and the two products of every torque component, (n, 3, 2)"""
    x, f = np.asarray(x, dtype=np.float64), np.asarray(f, dtype=np.float64)
    r = x - np.asarray(about, dtype=np.float64)[None, :]
    t = np.stack([np.stack([r[:, 1] * f[:, 2], -(r[:, 2] * f[:, 1])], axis=1), np.stack([r[:, 2] * f[:, 0], -(r[:, 0] * f[:, 2])], axis=1),
                  np.stack([r[:, 0] * f[:, 1], -(r[:, 1] * f[:, 0])], axis=1)], axis=1)
    return f, t


def load_bound(x, f, about=(0.0, 0.0, 0.0)):
    """(n + 8) 2^-53 sum |t_i| per component: n - 1 additions of the fixed-order f64 sum, each within 2^-53 of the running sum's magnitude
    <= sum |t_i|, and at most 8 roundings inside a term (x - c, two products, their difference) -- (force bound (3,), torque bound (3,))"""
    ft, tt = load_terms(x, f, about)
    n = len(ft)
    return (n + 8) * 2.0 ** -53 * np.abs(ft).sum(axis=0), (n + 8) * 2.0 ** -53 * np.abs(tt).sum(axis=(0, 2))


# ---- the other runs the GPU suite compares against: each once per process, each held to the fairness condition by test_wall_load_cpu.py ----------
def fair_counts(f):
    """(plate samples, box samples) with a nonzero f_b: the plate is group 1, rows 2402 .. 2509 of every wall set here, the box the rows before"""
    nz = (np.asarray(f) != 0).any(axis=1)
    return int(nz[2402:2510].sum()), int(nz[:2402].sum())


def _state_of(s):
    return {"pos": s.pos.copy(), "vel": s.vel.copy(), "warm_k": s.warm.copy(), "dt": float(s.dt)}


def _record(s):
    with np.errstate(all="ignore"):
        s.step()
    return {"f": s.f_b.copy(), "pos": s.pos.copy(), "dt": float(F(s.dt)), "wall_pos": s.sc.wall_pos.copy()}


EDGE = {                 # short rows of points on the d lattice half a spacing inside a box face, beside the column: 1, 63, 64 and 65 samples
    1: F([[0.025, 0.3, 0.025]]),
    63: F([[0.075 + D * i, 0.025, 0.075 + D * k] for i in range(9) for k in range(7)]),
    64: F([[0.075 + D * i, 0.05 + D * j, 0.025] for i in range(7) for j in range(10)])[:64],
    65: F([[0.025, 0.05 + D * j, 0.075 + D * k] for k in range(7) for j in range(10)])[:65],
}


@functools.lru_cache(maxsize=None)
def edge_run():
    """the pressed wcsph state with the four edge groups behind the plate (ids 2 .. 5), two steps"""
    _, s, walls, _ = pressed_solver("wcsph")
    state = _state_of(s)
    ids = [walls.add(EDGE[n]) for n in (1, 63, 64, 65)]
    assert ids == [2, 3, 4, 5] and np.isfinite(s.sc.wall_vol).all()
    steps = [_record(s) for _ in range(2)]
    return {"state": state, "steps": steps, "wall_pos": s.sc.wall_pos.copy(), "info": {g: (a, n) for g, a, n in walls.info()}, "box": (0, 2402)}


@functools.lru_cache(maxsize=None)
def edit_run(solver):
    """two steps; EDGE[65] added as group 2; two steps; group 2 removed; two steps"""
    _, s, walls, _ = pressed_solver(solver)
    state = _state_of(s)
    steps = [_record(s) for _ in range(2)]
    assert walls.add(EDGE[65]) == 2
    steps += [_record(s) for _ in range(2)]
    walls.remove(2)
    steps += [_record(s) for _ in range(2)]
    return {"state": state, "steps": steps}


REMOVE_BOX = (F([0.0, 0.3, 0.0]), F([1.0, 1.0, 1.0]))                                   # the column's top
ADDED = F([[0.1 + D * i, 0.4, 0.1 + D * k] for i in range(3) for k in range(3)])        # nine particles dropped back in


@functools.lru_cache(maxsize=None)
def particles_run(solver):
    """two steps; remove_in_box(REMOVE_BOX); two steps; add_particles(ADDED) at rest; two steps"""
    _, s, _, _ = pressed_solver(solver)
    state = _state_of(s)
    steps = [_record(s) for _ in range(2)]
    gone = ((s.pos >= REMOVE_BOX[0]) & (s.pos < REMOVE_BOX[1])).all(axis=1)
    gr.keep_rows(s, ~gone)
    steps += [_record(s) for _ in range(2)]
    s.pos, s.vel, s.warm = np.concatenate([s.pos, ADDED]), np.concatenate([s.vel, np.zeros_like(ADDED)]), np.concatenate([s.warm, np.zeros(len(ADDED), dtype=F)])
    s.N = len(s.pos)
    steps += [_record(s) for _ in range(2)]
    return {"state": state, "steps": steps, "gone": int(gone.sum())}


def compared_runs():
    """every restatement run a GPU test compares against, as (name, [f_b of every compared step])"""
    out = [("%s, %d steps" % (sv, 6), [st["f"] for st in run(sv, 6)["steps"]]) for sv in ("wcsph", "dfsph", "pcisph", "iisph")]
    out.append(("dfsph from delta_time 5e-4", [st["f"] for st in run("dfsph", 6, 5e-4)["steps"]]))
    out.append(("edge groups", [st["f"] for st in edge_run()["steps"]]))
    for sv in ("wcsph", "dfsph"):
        out.append(("%s, a group added and removed" % sv, [st["f"] for st in edit_run(sv)["steps"]]))
        out.append(("%s, particles removed and added" % sv, [st["f"] for st in particles_run(sv)["steps"]]))
    return out
