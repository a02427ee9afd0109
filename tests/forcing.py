"""Gravity as a vector, constant or harmonic: what tests/test_forcing_cpu.py, tests/test_forcing_gpu.py and tests/slab_forcing_worker.py share.
TEST INFRASTRUCTURE ONLY.

The second restatement carries the acceleration as a vector already (second_restatement.Solver.g_vec, read by every solver in it, PBF's subclass
included), so it is driven here with any vector, written before every step, without touching it.  Its rigid body builds the vector from the
scalar inside kinematic (second_restatement_rigid.py:197): ForcedBody hands that line the vector's components instead.

The library's side of a comparison is a handle (cfd_taichi_amd._native.Simulation); `lockstep` steps handles first, reads back the vector each
step used (SPH_S_ACCEL), feeds it to the restatement and compares every field on raw bits after every step."""
import numpy as np

import restatement_compare as rc
from harness import same_bits
from second_restatement import Solver
from second_restatement_pbf import PbfSolver
from second_restatement_rigid import Body

F = np.float32
TILT = (-4.9, -8.6, 2.0)                                   # the constant tilt of the GPU tests
AMP, OMEGA, PHASE = (3.0, 0.0, 2.0), (40.0, 0.0, 25.0), (0.0, 0.0, 1.0)      # ... and the harmonic forcing on top of it


def default_vector(cfg):
    """the three floats the reference forms: gravity * (0, -1, 0), as second_restatement.py:217 writes them"""
    g = cfg["scene"]["gravity"]
    return np.array([g * 0.0, g * -1.0, g * 0.0], dtype=F)


def accel_formula(g, amp, omega, phase, t):
    """a_k = (float)((double)g_k + A_k sin(w_k t + p_k)) in f64, rounded once; an axis without amplitude keeps g_k"""
    g32 = np.asarray(g, dtype=F)
    amp, omega, phase = (np.asarray(v, dtype=np.float64) for v in (amp, omega, phase))
    a = (g32.astype(np.float64) + amp * np.sin(omega * np.float64(t) + phase)).astype(F)
    return np.where(amp != 0.0, a, g32).astype(F)


def ulp_distance(a, b):
    """distance in f32 ulps between finite values of the same sign class (ordered-integer view)"""
    def key(x):
        i = np.ascontiguousarray(x, dtype=F).view(np.int32).astype(np.int64)
        return np.where(i < 0, np.int64(-(2 ** 31)) - i, i)
    return np.abs(key(a) - key(b))


class _Components:
    """stands where kinematic multiplies the scalar gravity by 0.0, -1.0, 0.0 in turn: the three products are the vector's components"""

    def __init__(self, vec):
        self._it = iter([float(v) for v in vec])

    def __mul__(self, _factor):
        return next(self._it)


class ForcedBody(Body):
    """Body whose kinematic adds g_vec where second_restatement_rigid.py:197 builds gravity * (0, -1, 0) from the scalar"""
    g_vec = None

    def kinematic(self, dt, gravity):
        super().kinematic(dt, _Components(self.g_vec))


def restatement(cfg, rg=None):
    """the second restatement of cfg's solver, its body (if any) a ForcedBody; g_vec starts as the default vector"""
    s = PbfSolver(cfg) if cfg["solver"]["name"] == "pbf" else Solver(cfg, rg)
    if s.name == "dfsph":
        s.max_dens = 100                                   # the library's cap on the density loop (reported as `capped`)
    if s.body is not None:
        s.body.__class__ = ForcedBody
        s.body.g_vec = s.g_vec.copy()
    return s


def step_with(s, vec, body_step=True):
    """one solver step (and, with an active body, the body step behind it) under the vector `vec`"""
    s.g_vec = np.asarray(vec, dtype=F).copy()
    if s.body is not None:
        s.body.g_vec = s.g_vec.copy()
    with np.errstate(all="ignore"):
        s.step()
        if body_step and s.body is not None and s.body.active:
            s.rigid_step()


def run_restatement(cfg, vectors, rg=None):
    """step the restatement once per vector; returns it"""
    s = restatement(cfg, rg)
    for v in vectors:
        step_with(s, v)
    return s


def inside_box(cfg, pos):
    lo, hi = np.array(cfg["scene"]["box_min"], dtype=F), np.array(cfg["scene"]["box_max"], dtype=F)
    return bool(np.isfinite(pos).all() and (pos >= lo).all() and (pos <= hi).all())


def stats_of(s):
    """(iteration counts, residuals) as compare_run holds them, per solver; None for wcsph and pbf"""
    if s.name == "dfsph":
        return (s.n_div, s.n_dens, F(s.div_first), F(s.div_err), F(s.dens_err), F(s.dt))
    if s.name in ("pcisph", "iisph"):
        return (s.n_dens, F(s.dens_err))
    return None


def stats_of_handle(solver, st):
    if solver == "dfsph":
        return (st.n_div, st.n_dens, F(st.div_first_err), F(st.div_err), F(st.dens_err), F(st.dt))
    if solver in ("pcisph", "iisph"):
        return (st.n_dens, F(st.dens_err))
    return None


def handle_fields(nat, sim, solver, names=None):
    names = names or rc.FIELDS[solver].values()
    return {n: sim.download(rc.F_ID[n]) for n in names}


def lockstep(nat, cfg, sims, steps, rg=None, forcing=None, fields=("pos", "vel", "rho"), dts=None, labels=None):
    """Step every handle of `sims` and the restatement `steps` times.  Per step: the handles go first; the vector the step used is read back
    (SPH_S_ACCEL, equal bits on every handle) and fed to the restatement; then `fields`, the iteration counts and residuals, and with a body
    the samples, centroid, vel and omega are compared on raw bits.  The clock: SPH_S_TIME equals the f64 running sum of the read-back
    delta_time values exactly.  forcing = (g, amp, omega, phase): SPH_S_ACCEL within 1 f32 ulp of accel_formula at the time the step began.
    dts: a delta_time written before each step.  Returns the restatement and what the run saw."""
    solver = cfg["solver"]["name"]
    s = restatement(cfg, rg)
    labels = labels or ["handle %d" % k for k in range(len(sims))]
    ev = {"iters": [], "lost": 0, "capped": 0, "ulps": 0, "vectors": [], "times": []}
    t_sum = [np.float64(0.0) for _ in sims]
    for k in range(1, steps + 1):
        used = None
        for n, sim in enumerate(sims):
            when = "%s, step %d" % (labels[n], k)
            if dts is not None:
                sim.set_dt(dts[k - 1])
            t_before = sim.time()
            assert t_before == t_sum[n], (when, t_before, t_sum[n])
            st = sim.step(1)
            if rg is not None and sim.scalar(nat.S_RIGID_ACTIVE):
                sim.rigid_step()
            t_sum[n] = t_sum[n] + np.float64(F(sim.scalar(nat.S_DELTA_TIME)))
            assert sim.time() == t_sum[n], (when, sim.time(), t_sum[n])
            a = sim.accel()
            if forcing is not None:
                want = accel_formula(*forcing, t_before)
                d = int(ulp_distance(a, want).max())
                ev["ulps"] = max(ev["ulps"], d)
                assert d <= 1, (when, a, want)
            if used is None:
                used = a
            same_bits(used, a, "%s: the step's vector" % when)
            if st is not None:
                ev["lost"] += int(st.lost)
                ev["capped"] += int(st.capped)
        ev["vectors"].append(used)
        ev["times"].append(float(t_sum[0]))
        if dts is not None:
            s.dt = F(dts[k - 1])
            s.cfg_dt = dts[k - 1]
        step_with(s, used)
        ev["iters"].append((s.n_div, s.n_dens) if solver == "dfsph" else s.n_dens)
        for n, sim in enumerate(sims):
            when = "%s, step %d" % (labels[n], k)
            if stats_of(s) is not None:
                assert stats_of(s) == stats_of_handle(solver, sim.last_stats), (when, stats_of(s))
            for name in fields:
                attr = [a_ for a_, f_ in rc.FIELDS[solver].items() if f_ == name][0]
                same_bits(getattr(s, attr), sim.download(rc.F_ID[name]), "%s: %s" % (when, name))
            if s.body is not None:
                b, sc = s.body, sim.rigid_scalars()
                same_bits(b.pos, sim.download(nat.F_RIGID_POS, nat.SPECIES_RIGID), "%s: body samples" % when)
                for mine, key in ((b.centroid, "centroid"), (b.vel, "vel"), (b.omega, "omega")):
                    same_bits(mine, sc[key], "%s: body %s" % (when, key))
    return s, ev
