"""Pinned-loop DFSPH stages: one step whose downloaded fields are the output of a known short chain of sweeps.

A free-running DFSPH step amplifies one ulp through discrete gates (loop trip counts, list membership at r = h, the `neighbour count < 20`
skip), which is why tests/test_relaxed_gpu.py can hold the relaxed arithmetic only to the reference's own nondeterminism envelope (1e-3).  With
the trip counts of both solver loops pinned through `solver.<attribute> = value` (SPH_P_* / Oracle.set_param) a step is a continuous function
of its input, and the f32 oracle and the f64 oracle (precision="f64") agree to 1e-7 ... 1e-4 per field on the same input: the yardstick the
relaxed sweeps are held to, sweep by sweep (tests/test_relaxed_sweeps_gpu.py), after tests/test_pinned_loops_cpu.py has shown on the reference
alone that the input states are fair.

Sweeps of a step (dfsph_solver.py): D1 rho, alpha | D2 warm start | D3 rho_derivative | D4 divergence correction | D5 external forces, v*,
CFL dt | D6 rho_adv | D7 density correction | D8 positions.

TEST INFRASTRUCTURE ONLY: nothing here imports the HIP library; a handle is anything with set_param / upload / step_dfsph / download."""
import functools

import numpy as np

from cfd_taichi_amd import scenes
from oracle import oracle as orc

# field ids are those of include/sph_mi355x.h, which the oracle shares
from oracle.oracle import F_ALPHA, F_NBR_COUNT, F_POS, F_RHO, F_RHO_ADV, F_RHO_DER, F_RIGID_FORCE, F_VEL, F_VEL_ADV, F_WARM_K  # noqa: E402,F401
FIELDS = (("rho", F_RHO), ("alpha", F_ALPHA), ("rho_der", F_RHO_DER), ("warm_k", F_WARM_K), ("rho_adv", F_RHO_ADV), ("vel_adv", F_VEL_ADV),
          ("pos", F_POS), ("vel", F_VEL))
# `solver.<attribute>`: name -> SPH_P_* (include/sph_mi355x.h)
PARAMS = {"density_threshold": 64, "min_iteration_density": 65, "min_iteration_density_divergence": 66, "max_iteration_density_divergence": 67,
          "density_divergence_threshold": 68, "warm_start": 69, "adaptive_dt": 70, "max_dt": 71}

_D3 = {"warm_start": 0, "max_iteration_density_divergence": 0, "adaptive_dt": 0, "min_iteration_density": 1, "density_threshold": 1e9}
_DIV3 = dict(_D3, warm_start=1, min_iteration_density_divergence=3, max_iteration_density_divergence=3, density_divergence_threshold=1e12)
# stage -> attributes.  What a field downloaded after ONE step then is:
#   d3     rho_der = D3(pos, vel) alone; rho_adv = D6 . D5; vel_adv = D7 . D6 . D5; pos, vel = D8 of that
#   warm   rho_der = D3 . D2 (warm_start_k uploaded)
#   div3   warm_k, rho_der after three D4 / D3 rounds
#   dens3  the third rho_adv, vel_adv after three D7
#   all    div3 + dens3 + the CFL rule: every field above, and dt
#   cfl    `all` with max_dt raised to 1e-2.  Under `all` the rule's result (4.6e-3 s at |v| <= 0.87 m/s) is cut to max_dt = 1e-3 on every
#          participant and dt says nothing about the maximum of |v*| that D5 reduces; here dt IS that maximum (0.4 d / max |v*| * 0.2)
# (density_threshold 1e9: the density loop runs exactly min_iteration_density times; the divergence loop's |err - past| < 1e-5 break,
#  dfsph_solver.py:410-412, is NOT governed by the minimum, hence every comparison first asserts equal counts)
STAGES = {
    "d3": _D3,
    "warm": dict(_D3, warm_start=1),
    "div3": _DIV3,
    "dens3": dict(_D3, min_iteration_density=3),
    "all": dict(_DIV3, min_iteration_density=3, adaptive_dt=1),
    "cfl": dict(_DIV3, min_iteration_density=3, adaptive_dt=1, max_dt=1e-2),
}

# the input states: lattice compressed about its centroid (the reference's density has no self term: bulk rho ~ 680 at rest, rho* = max(., rho_0)
# clamped almost everywhere, D6 / D7 invisible), every particle displaced by up to JITTER diameters per axis, random velocities and warm_start_k
COMPRESSION, JITTER, VEL_AMP, WARM_AMP = 0.88, 0.15, 0.5, 1e-4
# seeds at which tests/test_pinned_loops_cpu.py's conditions hold on every scene (2 and 7 leave under 5 % of dfsph_tiny_clamp with rho* > rho_0)
SEEDS = (1, 3)
# next to a body the column is compressed towards the face that looks at it and moved up to it (axis, side, shift): the scene starts with the
# body exactly one support radius away (no pair in reach), and a column compressed about its centroid would withdraw further
ANCHOR_FACE = {"dfsph_rigid_small": (0, "max", 0.04)}
FLOOR = 2.0 * 2.0 ** -24        # statistics that are exactly 0 on the reference side (clamped rho*): Oracle.get rounds f64 to f32
MARGIN = 4.0


def rigid_of(cfg):
    if "solid" not in cfg:
        return None
    from cfd_taichi_amd import mesh
    return mesh.rigid_from_config(cfg)


@functools.lru_cache(maxsize=None)
def state(scene, seed, compression=COMPRESSION, jitter=JITTER):
    """(pos, vel, warm_start_k) as f32 arrays: the same bits go to every participant."""
    cfg = scenes.get(scene)
    o = orc.Oracle(cfg, num_threads=1, rigid=rigid_of(cfg))
    lattice = o.get(orc.F_POS).astype(np.float64)
    o.close()
    rng = np.random.default_rng(seed)
    d = 2.0 * float(cfg["scene"]["particle_radius"])
    c = lattice.mean(0)
    if scene in ANCHOR_FACE:
        axis, side, shift = ANCHOR_FACE[scene]
        c[axis] = getattr(lattice[:, axis], side)()
        lattice[:, axis] += shift
        c[axis] += shift
    pos = c + (lattice - c) * compression + rng.uniform(-jitter * d, jitter * d, lattice.shape)
    vel = rng.uniform(-VEL_AMP, VEL_AMP, lattice.shape)
    warm = rng.uniform(-WARM_AMP, WARM_AMP, len(lattice))
    out = tuple(np.ascontiguousarray(a, dtype=np.float32) for a in (pos, vel, warm))
    for a in out:
        a.setflags(write=False)
    return out


class Result(dict):
    """name -> array of one participant after the step, plus .counts = (n_div, n_dens, n_div_evals), .dt, .nbr, .rigid_force (or None)"""


def _finish(res, stats, dt, nbr, rigid_force):          # dt: delta_time after the step, in the participant's own precision
    res.counts = (int(stats.n_div), int(stats.n_dens), int(stats.n_div_evals))
    res.dt = float(dt)
    res.nbr = nbr.astype(np.int64)
    res.rigid_force = rigid_force
    for a in res.values():
        a.setflags(write=False)
    return res


def run_oracle(scene, seed, stage, precision, num_threads=8):
    cfg = scenes.get(scene)
    rg = rigid_of(cfg)
    o = orc.Oracle(cfg, num_threads=num_threads, precision=precision, rigid=rg)
    for k, v in STAGES[stage].items():
        o.set_param(PARAMS[k], v)
    pos, vel, warm = state(scene, seed)
    o.set(orc.F_POS, pos); o.set(orc.F_VEL, vel); o.set(orc.F_WARM_K, warm)
    o.step_dfsph(1, 100)
    res = Result((name, o.get(f)) for name, f in FIELDS)
    _finish(res, o.last_stats, o.dt, o.get(orc.F_NBR_COUNT), o.get(orc.F_RIGID_FORCE) if rg is not None else None)
    o.close()
    return res


@functools.lru_cache(maxsize=None)
def references(scene, seed, stage):
    """(f32 oracle, f64 oracle) on state(scene, seed): computed once, shared by every test that needs them, never written to."""
    return run_oracle(scene, seed, stage, "f32"), run_oracle(scene, seed, stage, "f64")


def run_handle(sim, scene, seed, stage, rigid=False):
    """The same on a library handle (cfd_taichi_amd._native.Simulation) created by the caller under whatever overrides select the path."""
    for k, v in STAGES[stage].items():
        sim.set_param(k, v)
    pos, vel, warm = state(scene, seed)
    sim.upload(F_POS, pos); sim.upload(F_VEL, vel); sim.upload(F_WARM_K, warm)
    st = sim.step_dfsph(1)
    assert st.lost == 0 and st.capped == 0
    res = Result((name, sim.download(f)) for name, f in FIELDS)
    return _finish(res, st, st.dt, sim.download(F_NBR_COUNT), sim.download(F_RIGID_FORCE, 2) if rigid else None)


# ---- the comparison ----------------------------------------------------------------------------------------------------------------------

def errors(a, ref64):
    """Per-particle error e(i) = ||a_i - f64_i|| / max |f64|."""
    d = a.astype(np.float64) - ref64.astype(np.float64)
    e = np.abs(d) if d.ndim == 1 else np.sqrt((d * d).sum(1))
    return e / max(float(np.abs(ref64).max()), 1e-30)


def stats3(e):
    return tuple(float(v) for v in np.quantile(e, (0.5, 0.99))) + (float(e.max()),)


def wall_mask(scene, seed):
    """Particles of the input state within one support radius (4 r) of a box face: wall lists / k_rx_wall_grad / the clamp."""
    cfg = scenes.get(scene)
    h = 4.0 * float(cfg["scene"]["particle_radius"])
    pos = state(scene, seed)[0].astype(np.float64)
    lo, hi = np.asarray(cfg["scene"]["box_min"], dtype=np.float64), np.asarray(cfg["scene"]["box_max"], dtype=np.float64)
    return ((pos - lo < h) | (hi - pos < h)).any(1)


def populations(scene, seed, nbr):
    """name -> mask.  Where separate code runs: next to a wall / not; each class of the fluid count mod 8 (the padded tail group of the 16-bit
    lists).  (The count of F_NBR_COUNT: fluid neighbours, plus the rigid entries next to a body.)"""
    wall = wall_mask(scene, seed)
    pops = {"all": np.ones(len(nbr), dtype=bool), "wall": wall, "rest": ~wall}
    for k in range(8):
        pops["mod8=%d" % k] = nbr % 8 == k
    return pops


STATS = ("q50", "q99", "max")


def compare(e_cand, e_f32, margin=MARGIN):
    """[(stat, candidate, f32 oracle, ratio, ok)]: the candidate's statistic must be <= margin x the f32 oracle's + FLOOR; ratio <= margin is
    the same statement (ratio = candidate / (f32 + FLOOR / margin))."""
    out = []
    for name, c, r in zip(STATS, stats3(e_cand), stats3(e_f32)):
        out.append((name, c, r, c / (r + FLOOR / margin), c <= margin * r + FLOOR))
    return out


class Pool:
    """Per-particle errors of the candidate and of the f32 oracle, by (field, population), pooled over the seeds of one case."""

    def __init__(self, fields=FIELDS):
        """fields: ((name, field id), ...) of the solver under test (tests/pressure_states.py has its own)"""
        self.e = {}
        self.fields = fields

    def add(self, scene, seed, cand, r32, r64, pops=None, tag=None):
        """pops: name -> mask, default populations(scene, seed, r64.nbr); tag: what keeps the pooled entries apart, default the seed"""
        if pops is None:
            pops = populations(scene, seed, r64.nbr)
        if tag is None:
            tag = "seed%d" % seed
        for name, _ in self.fields:
            ec, er = errors(cand[name], r64[name]), errors(r32[name], r64[name])
            for pop, m in pops.items():
                key = (name, pop if pop.startswith("mod8") else "%s/%s" % (pop, tag))      # mod-8 classes pooled, the rest per seed
                a, b = self.e.get(key, (np.empty(0), np.empty(0)))
                self.e[key] = (np.concatenate([a, ec[m]]), np.concatenate([b, er[m]]))

    def add_raw(self, key, e_cand, e_f32):
        self.e[key] = (np.asarray(e_cand, dtype=np.float64), np.asarray(e_f32, dtype=np.float64))

    def rows(self):
        """[(field, population, n, stat, candidate, f32, ratio, ok)] over every non-empty population"""
        rows = []
        for (name, pop), (ec, er) in self.e.items():
            if len(ec) == 0:
                continue
            for stat, c, r, ratio, ok in compare(ec, er):
                rows.append((name, pop, len(ec), stat, c, r, ratio, ok))
        return rows

    def report(self, label):
        """Prints one line per field -- candidate / f32 oracle = ratio of the three whole-population statistics (the seed with the worst ratio), then
        the worst ratio of the wall, rest and mod-8 populations -- and returns the failures."""
        rows = self.rows()
        for name in dict.fromkeys(r[0] for r in rows):
            mine = [r for r in rows if r[0] == name]
            txt = []
            for stat in STATS:
                w = max((r for r in mine if r[1].startswith("all/") and r[3] == stat), key=lambda r: r[6])
                txt.append("%s %.2e/%.2e=%.2f" % (stat, w[4], w[5], w[6]))
            for group in dict.fromkeys("mod8" if r[1].startswith("mod8") else r[1].split("/")[0] for r in mine if not r[1].startswith("all/")):
                sub = [r for r in mine if r[1].startswith(group)]
                if sub:
                    w = max(sub, key=lambda r: r[6])
                    txt.append("%s %.2f (%s %s n=%d)" % (group, w[6], w[1], w[3], w[2]))
            print("%s %-9s %s" % (label, name, " | ".join(txt)))
        return ["%s %s[%s] %s: %.3e > %g x %.3e + %.1e (ratio %.2f, n = %d)" % (label, r[0], r[1], r[3], r[4], MARGIN, r[5], FLOOR, r[6], r[2])
                for r in rows if not r[7]]
