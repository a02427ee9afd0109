"""Mid-run API calls and re-seats: a handle's history must not show in its bits (TEST INFRASTRUCTURE: test_midrun_calls_cpu.py and
test_midrun_calls_gpu.py; nothing here imports the HIP library -- the GPU file hands in `nat`, cfd_taichi_amd._native).

The other suites hold the library to the oracle on handles that are created, perhaps given one state, and then only ever `step`.  Between two
steps the library keeps a good deal of state that only its host code keeps coherent (the device order and the ping-pong roles of the sorted
arrays, `nl_valid` / `density_valid`, the density loop's tile order and change stamps, Verlet lists behind a device-side `moved` word, captured
wcsph step pairs keyed by the buffer roles).  Two properties say that this state never shows:

1. INVISIBLE CALLS.  A handle runs K history steps and then, before each of M further steps (and, with a body, between `step` and `rigid_step`),
   a seeded random draw of 3 to 6 calls (`Disturber`): reads, profiling, the stages of a step, same-value writes, refused calls.  Every
   step's statistics and every downloadable field at the end equal, bit for bit, those of a twin handle that only stepped and -- under the exact
   arithmetic -- the oracle's in lock step.  After every draw the fields that travel from step to step (PERSISTENT) are compared with what they
   were before it: a field of the last step that a stage re-sorts away is caught there even if the next step recomputes it.
2. RE-SEAT.  K steps, then `upload` of a state S that has nothing to do with the current one, then M steps in lock step with the oracle, which is
   given the same S by `Oracle.set`; twice on the same handle.  S is the state of step K / 2 (rewind), the current state mirrored in x (mirror) or
   pinned_loops.state (foreign).

What survives an `Oracle.set(pos, vel[, warm_k])` on the oracle side (oracle/sph_oracle.c: orc_set writes the named array and nothing else; every
step begins with orc_build_grid and recomputes rho, alpha, the neighbour count, every force and every loop variable from pos / vel):
  dfsph   delta_time (dt, dt2, ps_dt: the CFL rule of the step before, read by D2 .. D4 before D5 re-derives it), simulate_cnt
  wcsph   nothing (delta_time is the configuration's)
  pcisph  nothing (delta is a constant of the handle, press_iter / press_force are zeroed at the head of the step: orc_step_pcisph)
  iisph   p_past, last step's pressure (press_iter starts from 0.5 * p_past, :68) -- no upload exists for it
  pbf     nothing (lambda and delta_pos are recomputed before they are read)
  a body  its pose, velocity, omega and the forces gathered since the last rigid_step: both sides share them through the common history
So a relaxed handle, which has neither an oracle nor a twin with the same history, can be held to a FRESH relaxed handle given S and the re-seated
handle's delta_time wherever that set is {delta_time} or empty: dfsph, wcsph (Verlet lists: both build them at S), pcisph, pbf -- not iisph.
"""
import collections
import copy
import functools

import numpy as np

import harness as h
import pinned_loops as pl
from cfd_taichi_amd import mesh, scenes
from cfd_taichi_amd._native import S_DELTA_TIME, S_SIMULATE_CNT, SPECIES_FLUID as FLUID, SPECIES_RIGID as RIGID, SPECIES_WALL as WALL
from harness import LINEAR, MORTON, ORACLE_STATS, same_values_nan_signed, squeezed
from oracle import oracle as orc
from oracle.oracle import (F_A_II, F_ACC, F_ALPHA, F_D_II, F_D_IJ, F_NBR_COUNT, F_PBF_DELTA_POS, F_PBF_LAMBDA, F_POS, F_POS_PREDICT, F_PRESS_FORCE, F_PRESS_ITER,
                           F_PRESSURE, F_RHO, F_RHO_ADV, F_RHO_DER, F_RIGID_FORCE, F_RIGID_MASS, F_RIGID_POS, F_RIGID_VERT, F_RIGID_VOL, F_VEL, F_VEL_ADV,
                           F_WALL_POS, F_WALL_VOL, F_WARM_K)

K, M = 40, 20
SEED = 20240807

# (field ids: the oracle's, which the library shares; scalar and species ids: the library's)
SCALARS = tuple(range(10)) + (30, 31, 32)
RIGID_SCALARS = tuple(range(10, 29))
PARAMS = {"density_threshold": 64, "min_iteration_density": 65, "min_iteration_density_divergence": 66, "max_iteration_density_divergence": 67,
          "density_divergence_threshold": 68, "warm_start": 69, "adaptive_dt": 70, "max_dt": 71, "min_dt": 72,
          "viscosity_c_s": 73, "viscosity_alpha": 74, "viscosity_epsilon": 75, "tension_k": 76}
DFSPH_PARAMS = tuple(k for k, v in PARAMS.items() if v <= 72)
FLUID_PARAMS = tuple(k for k, v in PARAMS.items() if v >= 73)

# what a step of each solver leaves downloadable, and is held to the oracle at the end of a run (the same ids on both sides)
SOLVER_FIELDS = {
    "wcsph": (F_POS, F_VEL, F_RHO, F_PRESSURE, F_ACC),
    "dfsph": (F_POS, F_VEL, F_RHO, F_ALPHA, F_WARM_K, F_RHO_DER, F_RHO_ADV, F_VEL_ADV, F_NBR_COUNT),
    "pcisph": (F_POS, F_VEL, F_RHO, F_PRESS_ITER, F_PRESS_FORCE, F_POS_PREDICT, F_RHO_ADV),
    "iisph": (F_POS, F_VEL, F_RHO, F_PRESS_ITER, F_PRESS_FORCE, F_D_II, F_D_IJ, F_A_II, F_RHO_ADV, F_VEL_ADV),
    "pbf": (F_POS, F_VEL, F_RHO, F_PBF_LAMBDA, F_PBF_DELTA_POS, F_POS_PREDICT),
}
# every fluid field sph_download hands out on a handle of the solver (the twin comparison and the `download` call)
DOWNLOADABLE = {s: tuple(dict.fromkeys(f + (F_RHO_ADV, F_RHO_DER, F_NBR_COUNT))) for s, f in SOLVER_FIELDS.items()}
# what sph_download_local hands out: on a dfsph handle, on the others
LOCAL_DFSPH = (F_POS, F_VEL, F_RHO, F_ALPHA, F_WARM_K, F_RHO_ADV, F_RHO_DER, F_VEL_ADV)
LOCAL_OTHERS = (F_POS, F_VEL, F_RHO, F_RHO_ADV, F_RHO_DER, F_ACC, F_PRESSURE)
# what travels from one step to the next through the library's re-sorts and must be untouched by every invisible call: the state itself, and the
# fields of the last step that no stage of a step recomputes (pbf: sph_build_neighbors carries lambda and delta_pos through its re-sort)
PERSISTENT = {"wcsph": (F_POS, F_VEL), "dfsph": (F_POS, F_VEL, F_WARM_K), "pcisph": (F_POS, F_VEL), "iisph": (F_POS, F_VEL),
              "pbf": (F_POS, F_VEL, F_PBF_LAMBDA, F_PBF_DELTA_POS)}
STATS = ("n_div", "n_dens", "n_div_evals", "div_first_err", "div_err", "dens_err", "dt", "lost", "max_nbrs")
# (harness.ORACLE_STATS is STATS[:7], OrcStepStats; `lost` is Oracle.lost, max_nbrs has no counterpart there: twin only)

Case = collections.namedtuple("Case", "name scene solver arith env oracle rigid squeeze chunks k m start compression")


def _case(name, scene, solver, arith="exact", env=LINEAR, oracle=None, rigid=False, squeeze=None, chunks=None, k=K, m=M, start=None, compression=pl.COMPRESSION):
    """k, m: history steps and disturbed steps of the invisible-call run (reseat_steps: those of a re-seat run); squeeze: the factor of
    test_pbf_gpu.squeeze on the rest lattice; start "foreign": the run begins at pinned_loops.state(scene, 0); compression: that of the foreign states.
    A run means something only if it reaches what it is meant to disturb, and tests/test_midrun_calls_cpu.py asserts on the oracle alone that it
    does: dfsph histories reach n_dens >= 3 (the density loop's working-tiles-first order gets set) and end a divergence loop below its cap of 15
    (the undo path runs); pcisph / iisph histories reach 3 pressure iterations; pbf's lambda is non-zero in the history and in every disturbed
    step; a body feels the fluid; and in the M steps after a re-seat no particle is lost, no loop is capped and n_dens >= 3 (lambda != 0) is
    reached again.  Where K = 40, M = 20, squeeze 0.9 and pinned_loops' compression of 0.88 do not give that, the mildest change that does:
      pbf     squeezed by 0.9 the column pushes particles out of the grid from step 9 on (7 lost after 60 steps): 0.95 loses none for 56 steps.
              The constraint is live for the first 20 steps only (339 particles with lambda != 0 at step 5, 9 at step 20, one from step 35 on):
              the calls are drawn before steps 5 .. 20 (k = 4, m = 16); a re-seat run has K = 30, M = 16 and foreign states at 0.94 (at 0.88 the
              first particles leave 18 steps later)
      pcisph  a foreign state at 0.88 runs the first pressure loop into its cap of 80 iterations; at 0.92 it takes 47
      wcsph with the body  the rest lattice is under-dense, its Tait pressure is clamped at 0 and the body feels nothing within 60 steps wherever it
              stands; from the foreign state (the column moved up to the body, pinned_loops.ANCHOR_FACE) it does from the first step
      dfsph_rigid_small  n_dens >= 3 from step 33 on (the falling body starts to squeeze the fluid): K = 40 holds it; its oracle takes 0.12 s a
              step, hence m = 12"""
    return Case(name, scene, solver, arith, dict(env), (arith == "exact") if oracle is None else oracle, rigid, squeeze, chunks, k, m, start, compression)


# wcsph steps in calls of mixed length: graph pairs, odd remainders and the key flips of a compute_density() in between interleave
CHUNKS = (2, 3, 1, 4)
CASES = collections.OrderedDict((c.name, c) for c in (
    _case("dfsph_tiny_wall", "dfsph_tiny_wall", "dfsph"),                                                      # linear cells, quad sweeps
    _case("dfsph_dam_x_cap1664", "dfsph_dam_x", "dfsph", env=dict(MORTON, SPH_STAGE_CAP="1664")),
    _case("dfsph_dam_x_cap300", "dfsph_dam_x", "dfsph", env=dict(MORTON, SPH_STAGE_CAP="300")),           # staged and unstaged tiles mix
    _case("dfsph_rigid_small", "dfsph_rigid_small", "dfsph", env=MORTON, rigid=True, m=12),      # (the oracle takes 0.12 s a step here)
    _case("dfsph_30k", "breaking_dam_30k_dfsph", "dfsph", env=MORTON, oracle=False),                       # hundreds of tiles: twin only
    _case("dfsph_30k_relaxed", "breaking_dam_30k_dfsph", "dfsph", arith="relaxed", env=MORTON),
    _case("wcsph_small", "wcsph_small", "wcsph", chunks=CHUNKS),
    _case("wcsph_small_relaxed", "wcsph_small", "wcsph", arith="relaxed", chunks=CHUNKS),                    # Verlet lists
    _case("wcsph_rigid", "dfsph_rigid_small", "wcsph", rigid=True, start="foreign"),
    _case("pcisph_linear", "dfsph_tiny_wall_pcisph", "pcisph", compression=0.92),
    _case("pcisph_morton", "dfsph_tiny_wall_pcisph", "pcisph", compression=0.92, env=MORTON),
    _case("pcisph_relaxed", "dfsph_tiny_wall_pcisph", "pcisph", compression=0.92, arith="relaxed", env=MORTON),              # staged sweeps with KF<true>
    _case("iisph_linear", "dfsph_tiny_wall_iisph", "iisph"),
    _case("iisph_morton", "dfsph_tiny_wall_iisph", "iisph", env=MORTON),
    _case("iisph_relaxed", "dfsph_tiny_wall_iisph", "iisph", arith="relaxed", env=dict(LINEAR, SPH_QUAD="0")),   # plain sweeps with KF<true>
    _case("pbf_quad", "pbf_tiny_wall", "pbf", squeeze=0.95, k=4, m=16, compression=0.94),
    _case("pbf_plain", "pbf_tiny_wall", "pbf", env=dict(LINEAR, SPH_QUAD="0"), squeeze=0.95, k=4, m=16, compression=0.94),
    _case("pbf_quad_relaxed", "pbf_tiny_wall", "pbf", arith="relaxed", squeeze=0.95, k=4, m=16, compression=0.94),
    _case("pbf_plain_relaxed", "pbf_tiny_wall", "pbf", arith="relaxed", env=dict(LINEAR, SPH_QUAD="0"), squeeze=0.95, k=4, m=16, compression=0.94),
))
ORACLE_CASES = tuple(n for n, c in CASES.items() if c.oracle)
# relaxed handles whose oracle-side surviving set is {delta_time} or empty (module docstring)
RELAXED_RESEAT_CASES = tuple(n for n, c in CASES.items() if c.arith == "relaxed" and c.solver != "iisph")
# the scenes the oracle is the yardstick of, once each (the exact cases of one scene differ only in what the library does with it; the 30 k dam
# break is held to its twin alone: its oracle takes 0.4 s a step)
ORACLE_SCENES = tuple(dict.fromkeys((c.scene, c.solver) for c in CASES.values() if c.oracle))
WCSPH_BODY_DT = 2.5e-4                     # dfsph_rigid_small as wcsph: rigid_modes.DT["wcsph"]


@functools.lru_cache(maxsize=None)
def _config(scene, solver):
    cfg = scenes.get(scene)
    if cfg["solver"]["name"] != solver:            # dfsph_rigid_small as wcsph
        cfg["solver"]["name"] = solver
        cfg["solver"]["delta_time"] = WCSPH_BODY_DT
    return cfg


def config(case):
    return copy.deepcopy(_config(case.scene, case.solver))


def rigid_of(case):
    return mesh.rigid_from_config(config(case)) if case.rigid else None


def oracle_of(case, num_threads=8):
    return h.make_oracle(config(case), case.solver, rigid=rigid_of(case), num_threads=num_threads)


def stats_bits(st, names=STATS):
    return h.stats_bits(st, names)


# ---- states S of a re-seat -----------------------------------------------------------------------------------------------------------------

def mirrored(case, pos, vel):
    """x -> box_min.x + box_max.x - x in f32, v_x -> -v_x"""
    sc = config(case)["scene"]
    p, v = pos.copy(), vel.copy()
    p[:, 0] = (np.float32(sc["box_min"][0]) + np.float32(sc["box_max"][0])) - p[:, 0]
    v[:, 0] = -v[:, 0]
    return p, v


def foreign(case, seed):
    """pinned_loops.state of the scene: the lattice compressed and jittered, random velocities and warm_start_k"""
    return pl.state(case.scene, seed, case.compression)


def inside_box(case, pos):
    sc = config(case)["scene"]
    return bool(((pos >= np.asarray(sc["box_min"], dtype=np.float32)) & (pos <= np.asarray(sc["box_max"], dtype=np.float32))).all())


RESEAT_ORDERS = (("rewind", "foreign"), ("mirror", "rewind"), ("foreign", "mirror"))     # every kind first once and second once


def reseat_state(case, kind, current, half, seed):
    """(pos, vel, warm_k or None): `current` / `half` = (pos, vel, warm_k or None) now and at step K / 2"""
    if kind == "rewind":
        return half
    if kind == "mirror":
        return mirrored(case, current[0], current[1]) + (current[2],)
    p, v, w = foreign(case, seed)
    return p, v, (w if case.solver == "dfsph" else None)


def oracle_state(o, solver):
    return (o.get(orc.F_POS), o.get(orc.F_VEL), o.get(orc.F_WARM_K) if solver == "dfsph" else None)


def oracle_set(o, state):
    o.set(orc.F_POS, state[0]); o.set(orc.F_VEL, state[1])
    if state[2] is not None:
        o.set(orc.F_WARM_K, state[2])


# ---- the oracle-side equivalents of the invisible calls (test_midrun_calls_cpu.py) ------------------------------------------------------------

def oracle_disturb(o, case, rng):
    """build_grid / compute_rho / compute_alpha / compute_nbr_count, set(F, get(F)), set_dt(dt), set_param(k, param(k)) in a seeded order"""
    calls = [o.build_grid, lambda: (o.build_grid(), o.compute_rho()), lambda: (o.build_grid(), o.compute_nbr_count()),
             lambda: o.set(orc.F_POS, o.get(orc.F_POS)), lambda: o.set(orc.F_VEL, o.get(orc.F_VEL)), lambda: o.set_dt(o.dt)]
    if case.solver == "dfsph":
        calls += [lambda: (o.build_grid(), o.compute_rho(), o.compute_alpha()), lambda: o.set(orc.F_WARM_K, o.get(orc.F_WARM_K))]
        calls += [lambda k=k: o.set_param(PARAMS[k], o.param(PARAMS[k])) for k in DFSPH_PARAMS]
    if case.solver != "pbf":
        calls += [lambda k=k: o.set_param(PARAMS[k], o.param(PARAMS[k])) for k in FLUID_PARAMS]
    for i in rng.permutation(len(calls)):
        calls[i]()


# ---- the invisible calls on a library handle ----------------------------------------------------------------------------------------------

class Disturber:
    """Draws the invisible calls on `sim` (a _native.Simulation of `case`).  `nat` = cfd_taichi_amd._native, `raises` = pytest.raises."""

    def __init__(self, sim, case, nat, raises, seed):
        self.sim, self.case, self.nat, self.raises = sim, case, nat, raises
        self.rng = np.random.default_rng(seed)
        self.verlet = case.solver == "wcsph" and case.arith == "relaxed"
        self.calls = self._calls()
        self.issued = collections.Counter()
        self.queue = [n for n in self.rng.permutation(sorted(self.calls)) if not n.startswith("profile_")]      # every call at least once per case
        self.profiling = False
        self.log = []

    # -- reads
    def _download(self):
        sim, c = self.sim, self.case
        for f in DOWNLOADABLE[c.solver]:
            sim.download(f)
        if sim.n_wall:
            sim.download(F_WALL_POS, WALL); sim.download(F_WALL_VOL, WALL)
        if c.rigid:
            for f in (F_RIGID_POS, F_RIGID_VOL, F_RIGID_FORCE, F_RIGID_MASS, F_RIGID_VERT):
                sim.download(f, RIGID)

    def _download_local(self):
        for f in (LOCAL_DFSPH if self.case.solver == "dfsph" else LOCAL_OTHERS):
            ids, vals = self.sim.download_local(f)
            assert len(ids) == self.sim.n_fluid == len(vals) and (ids >= 0).all()

    def _scalars(self):
        for s in SCALARS + (RIGID_SCALARS if self.case.rigid else ()):
            self.sim.scalar(s)

    def _params(self):
        for k in PARAMS:
            self.sim.param(k)

    # -- profiling: on at one draw, read / reset / off at a later one (wcsph: eager launches instead of graph replays in between)
    def _profile_on(self):
        self.sim.profile_enable(True)
        self.profiling = True

    def _profile_off(self):
        prof = self.sim.profile()
        assert prof and all(n > 0 and ms >= 0.0 for ms, n in prof.values()), prof
        self.sim.profile_reset()
        assert self.sim.profile() == {}
        self.sim.profile_enable(False)
        self.profiling = False

    # -- same-value writes
    def _writable(self):
        s = self.case.solver
        return (DFSPH_PARAMS + FLUID_PARAMS) if s == "dfsph" else () if s == "pbf" else FLUID_PARAMS

    def _set_params(self):
        for k in self._writable():
            self.sim.set_param(k, self.sim.param(k))

    def _upload(self, f):
        before = self.sim.download(f)
        self.sim.upload(f, before)
        assert h.bits_equal(self.sim.download(f), before), f

    # -- refused calls
    def _refused(self, fn):
        with self.raises(self.nat.SphError):
            fn()

    def _wrong_length(self):
        sim = self.sim
        a = np.zeros(3 * sim.n_fluid, dtype=np.float32)
        sim._check(sim._lib.sph_upload(sim._h, FLUID, F_POS, a.ctypes.data, a.size - 3))

    def _other_step(self):
        sim = self.sim
        for s in ("wcsph", "dfsph", "pcisph", "iisph", "pbf"):
            if s != self.case.solver:
                self._refused(lambda s=s: getattr(sim, "step_" + s)(1))

    def _foreign_params(self):
        """a valid value for every attribute the solver does not have: the dfsph loop attributes elsewhere, every attribute on pbf"""
        for k in PARAMS:
            if k not in self._writable():
                before = self.sim.param(k)
                self._refused(lambda k=k: self.sim.set_param(k, before))
                assert self.sim.param(k) == before, k

    def _nan_params(self):
        for k in self._writable() or ("viscosity_alpha",):          # pbf: refused as an attribute it does not have
            if k not in ("warm_start", "adaptive_dt"):                   # these two are truth values: NaN != 0 reads as true, nothing to refuse
                before = self.sim.param(k)
                self._refused(lambda k=k: self.sim.set_param(k, float("nan")))
                assert self.sim.param(k) == before, k

    def _calls(self):
        sim, c = self.sim, self.case
        calls = {
            "download": self._download, "download_local": self._download_local, "scalars": self._scalars, "params": self._params,
            "overrides": sim.overrides, "synchronize": sim.synchronize,
            "profile_on": self._profile_on, "profile_off": self._profile_off,
            "build_neighbors": sim.build_neighbors, "build_neighbors_twice": lambda: (sim.build_neighbors(), sim.build_neighbors()),
            "compute_density": sim.compute_density,
            "density_then_build": lambda: (sim.compute_density(), sim.build_neighbors()),
            "build_then_density": lambda: (sim.build_neighbors(), sim.compute_density()),
            "set_dt": lambda: sim.set_dt(sim.scalar(S_DELTA_TIME)),
            "refused_read_only": lambda: self._refused(lambda: sim.upload(F_RHO, np.zeros(sim.n_fluid, dtype=np.float32))),
            "refused_wrong_length": lambda: self._refused(self._wrong_length),
            "refused_nan": self._nan_params, "refused_other_step": self._other_step,
            "refused_slab_overlap": lambda: self._refused(lambda: sim.set_slab_overlap(True)),
            # the between-step features that read, or write what is there already: through the handle's validity flags (derived runs compute_density),
            # its API-order read-back, and the drop of the captured wcsph step pairs (a gravity vector is a launch-time fact even when it is the same)
            "diagnostics": sim.diagnostics, "derived": lambda: [sim.derived(q) for q in ("vorticity", "cover")],
            "wall_neighbor_counts": sim.wall_neighbor_counts, "geometry": sim.geometry,
            "set_gravity": lambda: sim.set_gravity(sim.gravity_vec()),
        }
        if c.solver != "pbf":
            calls["set_params"] = self._set_params
        if c.solver != "dfsph":
            calls["refused_foreign_params"] = self._foreign_params
        if c.rigid:
            calls["rigid_scalars"] = sim.rigid_scalars
        else:
            calls["refused_rigid_set_active"] = lambda: self._refused(lambda: sim.rigid_set_active(True))
        if not self.verlet:          # a rebuild at other positions legitimately reorders the relaxed sums: upload is not invisible on Verlet handles
            calls["upload_pos"] = lambda: self._upload(F_POS)
            calls["upload_vel"] = lambda: self._upload(F_VEL)
        if c.solver == "dfsph":
            calls["compute_alpha"] = sim.compute_alpha
            calls["alpha_then_build"] = lambda: (sim.compute_alpha(), sim.build_neighbors())
            calls["build_then_alpha"] = lambda: (sim.build_neighbors(), sim.compute_alpha())
            calls["upload_warm_k"] = lambda: self._upload(F_WARM_K)
            # sph_tune_time: 0 the divergence residual, 2 the density residual, 3 sort + list build write only what the next step recomputes
            # (include/sph_mi355x.h); 1 and 4 .. 7 advance the velocities or the loop state and are for throw-away handles
            for which in (0, 2, 3):
                calls["tune_time_%d" % which] = lambda which=which: sim.tune_time(which, 0, 2)
        else:
            calls["refused_warm_k"] = lambda: self._refused(lambda: sim.upload(F_WARM_K, np.zeros(sim.n_fluid, dtype=np.float32)))
            calls["refused_compute_alpha"] = lambda: self._refused(sim.compute_alpha)
            calls["refused_tune_time"] = lambda: self._refused(lambda: sim.tune_time(0, 0, 1))
        return calls

    def persistent(self):
        sim = self.sim
        fields = [f for f in PERSISTENT[self.case.solver] if f not in (F_PBF_LAMBDA, F_PBF_DELTA_POS) or sim.scalar(S_SIMULATE_CNT) > 0]
        out = {f: sim.download(f) for f in fields}
        out["dt"] = sim.scalar(S_DELTA_TIME)
        if self.case.rigid:
            out["rigid"] = np.float32([v for k in ("centroid", "omega", "vel") for v in sim.rigid_scalars()[k]])
            out["rigid_force"] = sim.download(F_RIGID_FORCE, RIGID)
            out["rigid_pos"] = sim.download(F_RIGID_POS, RIGID)
        return out

    def draw(self, when, profile=None, left=1):
        """3 to 6 calls (more where the `left` draws that remain could not issue every call once otherwise); the PERSISTENT fields afterwards
        are those from before.  profile: "on" / "off" joins this draw."""
        before = self.persistent()
        n = max(int(self.rng.integers(3, 7)), -(-len(self.queue) // max(1, left)))
        names = [self.queue.pop() for _ in range(min(n, len(self.queue)))]
        pool = [k for k in sorted(self.calls) if not k.startswith("profile_")]
        names += [pool[int(self.rng.integers(len(pool)))] for _ in range(n - len(names))]
        if profile:
            names.insert(int(self.rng.integers(len(names) + 1)), "profile_" + profile)
        for name in names:
            self.log.append((when, name))
            self.calls[name]()
            self.issued[name] += 1
        after = self.persistent()
        for f in before:
            if f == "dt":
                assert before[f] == after[f], (when, names, before[f], after[f])
            else:
                same_values_nan_signed(after[f], before[f], "%s: field %s after %s" % (when, f, names))

    def finish(self):
        """every call was issued at least once"""
        missing = sorted(set(self.calls) - set(self.issued))
        assert not missing and not self.queue and not self.profiling, (missing, self.queue, self.profiling)


def profile_plan(rng, m):
    """{draw index: "on" | "off"}: profiling goes on before one of the first steps and off a few steps later"""
    a = int(rng.integers(1, max(2, m // 2)))
    b = int(rng.integers(a + 2, m)) if a + 2 < m else m - 1
    return {a: "on", b: "off"}


def step_plan(case, n):
    """the lengths of the step calls that make n steps: 1, 1, ... or, for wcsph, CHUNKS repeated (the last one cut)"""
    if not case.chunks:
        return [1] * n
    out = []
    while sum(out) < n:
        out.append(min(case.chunks[len(out) % len(case.chunks)], n - sum(out)))
    return out


# ---- the two runs, on the oracle alone (sim None: test_midrun_calls_cpu.py) or with a library handle in lock step --------------------------------

def reseat_steps(case):
    """(K, M) of a re-seat run.  dfsph_rigid_small reaches n_dens >= 3 at step 33 only (the falling body starts to squeeze the fluid): K = 64 puts
    the rewind state, step K / 2, right before it, and its oracle costs 0.12 s a step, hence the short M"""
    return (64, 8) if case.name == "dfsph_rigid_small" else (30, 16) if case.solver == "pbf" else (case.k, case.m)


def reseat_orders(case):
    return RESEAT_ORDERS[:2] if case.name == "dfsph_rigid_small" else RESEAT_ORDERS


def begin(case, o=None, sims=()):
    """the state a run starts from, into the oracle and into fresh handles"""
    if case.squeeze:
        sq = squeezed(pl.state(case.scene, 0, 1.0, 0.0)[0], case.squeeze)         # (compression 1, no jitter: the rest lattice)
        if o is not None:
            o.set(orc.F_POS, sq)
        for sim in sims:
            sim.upload(F_POS, sq)
    if case.start == "foreign":
        p, v, _ = foreign(case, 0)
        if o is not None:
            o.set(orc.F_POS, p); o.set(orc.F_VEL, v)
        for sim in sims:
            sim.upload(F_POS, p); sim.upload(F_VEL, v)


def lockstep(case, o, sim, when, rec):
    """One step (and rigid_step) of the oracle and, if given, of the handle in lock step; rec collects what the CPU file's conditions are about."""
    r = h.oracle_step(o, case.solver, bits_view=True)
    rec["lost"] = max(rec.get("lost", 0), o.lost)
    if r is not None:
        rec.setdefault("n_dens", []).append(o.last_stats.n_dens)
        rec.setdefault("n_div", []).append(o.last_stats.n_div)
        rec["capped"] = max(rec.get("capped", 0), int(r[1]))
    if case.solver == "pbf":
        rec.setdefault("lambda", []).append(int((o.get(orc.F_PBF_LAMBDA) != 0).sum()))
    if sim is not None:
        st = sim.step(1)
        if r is not None:
            got = stats_bits(st, ORACLE_STATS) + (int(st.lost),)
            assert got == r[0], (when, dict(zip(ORACLE_STATS + ("lost",), zip(got, r[0]))))
            assert st.capped == int(r[1]), (when, st.capped, r[1])
        else:
            same_values_nan_signed(sim.download(F_POS), o.get(orc.F_POS), "%s: pos" % when)
            assert np.float32(sim.scalar(S_DELTA_TIME)) == np.float32(o.dt), when
    if case.rigid:
        force = o.get(orc.F_RIGID_FORCE)
        rec["force"] = max(rec.get("force", 0.0), float(np.abs(force).max()))
        if sim is not None:
            same_values_nan_signed(sim.download(F_RIGID_FORCE, RIGID), force, "%s: force on the body" % when)
            sim.rigid_step()
        o.rigid_step()
        if sim is not None:
            a, b = sim.rigid_scalars(), o.rigid_scalars()
            for k in ("centroid", "omega", "vel"):
                same_values_nan_signed(np.float32(a[k]), np.float32(b[k]), "%s: body %s" % (when, k))


def same_as_oracle(case, sim, o, when):
    """every field a step leaves downloadable, and the body"""
    for f in SOLVER_FIELDS[case.solver]:
        same_values_nan_signed(sim.download(f), o.get(f), "%s: field %d" % (when, f))
    assert np.float32(sim.scalar(S_DELTA_TIME)) == np.float32(o.dt), when
    if case.rigid:
        for f in (F_RIGID_POS, F_RIGID_FORCE, F_RIGID_VERT):
            same_values_nan_signed(sim.download(f, RIGID), o.get(f), "%s: rigid field %d" % (when, f))


def stage_fields_as_oracle(case, sim, o, when):
    """compute_density (dfsph: + alpha) and the neighbour count of the state both sides hold now, through the validity flags of the handle"""
    sim.compute_density()
    o.build_grid(); o.compute_rho(); o.compute_nbr_count()
    same_values_nan_signed(sim.download(F_RHO), o.get(orc.F_RHO), "%s: rho of compute_density" % when)
    same_values_nan_signed(sim.download(F_NBR_COUNT), o.get(orc.F_NBR_COUNT), "%s: neighbour count" % when)
    if case.solver == "dfsph":
        sim.compute_alpha(); o.compute_alpha()
        same_values_nan_signed(sim.download(F_ALPHA), o.get(orc.F_ALPHA), "%s: alpha of compute_alpha" % when)


def reseat_run(case, order, sim=None, seed=1):
    """K steps, S, M steps, the second S, M steps.  Returns [history record, record of the M steps after each S]: what the CPU file's conditions are about."""
    k, m = reseat_steps(case)
    o = oracle_of(case)
    begin(case, o, [sim] if sim is not None else [])
    recs, half = [{"kind": "history"}], None
    for s in range(k):
        if s == k // 2:
            half = oracle_state(o, case.solver)
        lockstep(case, o, sim, "history step %d" % (s + 1), recs[0])
    for n, kind in enumerate(order):
        when = "re-seat %d (%s)" % (n + 1, kind)
        state = reseat_state(case, kind, oracle_state(o, case.solver), half, seed + n)
        rec = {"kind": kind, "inside": inside_box(case, state[0])}
        if sim is not None:
            # (both flags of the handle say "valid" when the new state arrives: what sph_upload resets is what keeps the stages below honest)
            stage_fields_as_oracle(case, sim, o, when + ", before")
            sim.upload(F_POS, state[0]); sim.upload(F_VEL, state[1])
            if state[2] is not None:
                sim.upload(F_WARM_K, state[2])
        oracle_set(o, state)
        if sim is not None:
            stage_fields_as_oracle(case, sim, o, when + ", after the upload")
        for s in range(m):
            lockstep(case, o, sim, "%s, step +%d" % (when, s + 1), rec)
        recs.append(rec)
        if sim is not None:
            same_as_oracle(case, sim, o, when + ", the end")
    o.close()
    return recs
