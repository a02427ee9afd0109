"""Input states and the comparison for the relaxed WCSPH, PCISPH and IISPH steps: SPH_ARITH_RELAXED through the Verlet kernels of
csrc/sph_relaxed_kernels.h (k_wcsph_density_rx, k_wcsph_force_rx, rx_wg_clamped) and through KF<true> (csrc/sph_device.h) in the k_pci_* / k_ii_*
sweeps, held step by step to the f64 oracle with the f32 oracle's own error on the same input as the yardstick (tests/pinned_loops.py: errors,
compare, Pool, MARGIN, FLOOR).

No loop is pinned here.  On these states the pressure loops of the f32 oracle, the f64 oracle and seeded legal f32 schedules leave after the same
number of iterations through the same exit (tests/test_pressure_states_cpu.py asserts it for every case below, step by step), so a step is
compared as it runs.

  state   pinned_loops.state's construction: the lattice compressed about its centroid (0.88 / 0.97 / 1.0), jitter 0.15 d, |v| <= 0.5 m/s per axis
          (REUSE_VEL_AMP on the list-reuse case).  On a clamp scene the column is then translated so that on each axis the 5 % quantile of the
          coordinates lies on the lower clamp plane -- in f64, rounded to f32 once, the same bits for every participant; a column compressed
          about its centroid otherwise withdraws from every plane and the clamp branch never runs.
  scenes  scenes.SCENES by name, and `<scene>+clamp`: the scene's dict with boundary_handle set to False.

TEST INFRASTRUCTURE ONLY: nothing here imports the HIP library (handles() is handed it); a handle is anything with upload / step / download /
build_neighbors."""
import functools

import numpy as np

from cfd_taichi_amd import scenes
from harness import same_values
from oracle import oracle as orc
from pinned_loops import FLOOR, JITTER, MARGIN, STATS, VEL_AMP, Pool, compare, errors, stats3  # noqa: F401  (re-exported)

# field ids are those of include/sph_mi355x.h, which the oracle shares
from oracle.oracle import F_A_II, F_ACC, F_D_II, F_D_IJ, F_NBR_COUNT, F_POS, F_POS_PREDICT, F_PRESS_FORCE, F_PRESS_ITER, F_PRESSURE, F_RHO, F_VEL  # noqa: E402,F401
FIELDS = {
    "wcsph": (("rho", F_RHO), ("pressure", F_PRESSURE), ("acc", F_ACC), ("vel", F_VEL), ("pos", F_POS)),
    "pcisph": (("rho", F_RHO), ("press_iter", F_PRESS_ITER), ("press_force", F_PRESS_FORCE), ("pos_predict", F_POS_PREDICT), ("vel", F_VEL),
               ("pos", F_POS)),
    "iisph": (("rho", F_RHO), ("d_ii", F_D_II), ("a_ii", F_A_II), ("d_ij", F_D_IJ), ("press_iter", F_PRESS_ITER), ("press_force", F_PRESS_FORCE),
              ("vel", F_VEL), ("pos", F_POS)),
}
# the field whose sign splits the particles into those the pressure sweeps work on and those they skip (zero_press / zero_dij tiles)
PRESSURE_FIELD = {"wcsph": "pressure", "pcisph": "press_iter", "iisph": "press_iter"}
CLAMP_QUANTILE = 0.05
# particles on a clamp plane that a clamp case must show after every step (measured minima on the f64 oracle: 97, 39, 93)
MIN_CLAMPED = {"wcsph": 90, "pcisph": 35, "iisph": 90}
# the pressure split enters a step's comparison when both sides hold this many particles: q50 and q99 of a handful of particles are that handful's
# minimum and maximum, and seeded legal schedules of the f32 oracle itself reach 4.1-4.2 x on sides of 3 and 11 particles (measured on the CPU at
# compression 0.97, where under 2 % of the particles carry pressure).  Every particle stays in the all / wall / rest / mod-8 populations.
MIN_SPLIT = 32
STEPS = 3
# (scene, seed, compression): the cases of tests/test_pressure_states_cpu.py and of both GPU files.  Per solver two seeds, the compressions 0.88
# and 1.0 on the 640-particle wall scene, one clamp scene, one 5 880-particle scene (23 workgroups, a ragged last one).
# No case at 0.97: there 1-16 of the 640 particles carry all the pressure, so every class statistic of pressure, press_iter and press_force is one
# particle's, quantised at one ulp of that particle's rho (3e-6 of the largest pressure), which the f32 oracle hits or misses by chance.  Seeded
# schedules of the f32 oracle miss the bar themselves there: pcisph 5.21 / 4.24 / 4.80 at seeds 3 / 1 / 5, wcsph 4.81 at seed 3 (sixteen schedules
# each), iisph 8.57 at seed 3 (a hundred).  The CPU test asks every case for MIN_SPLIT particles with pressure in its first step.
# (For the record: on wcsph at (seed 1, 0.97), where a hundred schedules stay below 2.6, the relaxed handle measured 5.84 on pressure in one class
# of the count mod 8 -- 116 particles of which one carries pressure, its rho one ulp off where the f32 oracle's is none; over all particles 0.95.)
CASES = {
    "wcsph": (("wcsph_tiny_wall", 1, 0.88), ("wcsph_tiny_wall", 1, 1.0), ("wcsph_tiny_wall", 3, 1.0), ("wcsph_tiny_clamp", 3, 0.88),
              ("wcsph_small", 1, 0.88)),
    "pcisph": (("dfsph_tiny_wall_pcisph", 1, 0.88), ("dfsph_tiny_wall_pcisph", 3, 1.0), ("dfsph_tiny_wall_pcisph", 1, 1.0),
               ("dfsph_tiny_wall_pcisph+clamp", 3, 0.88), ("pcisph_config_backup", 1, 0.88)),
    "iisph": (("dfsph_tiny_wall_iisph", 1, 0.88), ("dfsph_tiny_wall_iisph", 3, 1.0), ("dfsph_tiny_wall_iisph", 1, 1.0),
              ("dfsph_tiny_wall_iisph+clamp", 3, 0.88), ("iisph_config_backup", 1, 0.88)),
}
LARGE = ("wcsph_small", "pcisph_config_backup", "iisph_config_backup")          # 5 880 particles
# the list-reuse case of tests/test_relaxed_wcsph_sweeps_gpu.py: REUSE_STEPS free-running steps of a compressed column (pressure on half the
# particles, as the cases above ask) at |v| <= 2 m/s per axis, which carry a particle skin / 2 away from where the lists were built within a step
# or two of 2.5e-4 s.  REUSE_BUILDS: SPH_VERLET_SKIN (None: the default, 0.05 h) -> S_VERLET_BUILDS after each step, by predicted_builds on the
# oracles (the CPU test asserts it).  At the default skin (skin / 2 = 2.5 mm) step 2 runs on the lists of step 1 and every later step follows a
# rebuild; at 0.1 h steps 2, 4, 6 and 8 reuse lists and steps 3, 5 and 7 follow a rebuild (at most 76 fluid and 23 wall entries per list,
# capacity 80).  (The same eight steps of the uncompressed column, seed 1 at 1.0, measured 4.76 at a zero skin and 6.75 at the default one on
# pressure in the smallest class of the count mod 8 -- 23 particles per step, two or three of them with pressure -- against 2.77 for sixteen
# schedules and 1.7 over all particles: the sparse-pressure statistic again, which is why the list-reuse case is a compressed column.)
REUSE_CASE, REUSE_STEPS, REUSE_VEL_AMP = ("wcsph_tiny_wall", 1, 0.88), 8, 2.0
REUSE_BUILDS = {None: [1, 1, 2, 3, 4, 5, 6, 7], "0.1": [1, 1, 2, 2, 3, 3, 4, 4]}
VERLET_SKIN = 0.05                                                              # csrc/sph_host_scene.h: the default, as a fraction of h


def config(scene):
    base, _, variant = scene.partition("+")
    cfg = scenes.get(base)
    if variant:
        assert variant == "clamp", scene
        cfg["solver"]["boundary_handle"] = False
    return cfg


def solver_of(scene):
    return config(scene)["solver"]["name"]


def clamp_offset(cfg):
    """distance of the clamp planes from the box faces: a diameter for wcsph (wcsph_solver.py:54-63), a radius for pcisph and iisph"""
    r = float(cfg["scene"]["particle_radius"])
    return 2.0 * r if cfg["solver"]["name"] == "wcsph" else r


@functools.lru_cache(maxsize=None)
def state(scene, seed, compression, vel_amp=VEL_AMP):
    """(pos, vel) as read-only f32 arrays: the same bits go to every participant.  pinned_loops.state's construction and random stream."""
    cfg = config(scene)
    o = orc.Oracle(cfg, num_threads=1)
    lattice = o.get(orc.F_POS).astype(np.float64)
    o.close()
    rng = np.random.default_rng(seed)
    d = 2.0 * float(cfg["scene"]["particle_radius"])
    c = lattice.mean(0)
    pos = c + (lattice - c) * compression + rng.uniform(-JITTER * d, JITTER * d, lattice.shape)
    vel = rng.uniform(-vel_amp, vel_amp, lattice.shape)
    if not cfg["solver"].get("boundary_handle", True):
        plane = np.asarray(cfg["scene"]["box_min"], dtype=np.float64) + clamp_offset(cfg)
        pos += plane - np.quantile(pos, CLAMP_QUANTILE, axis=0)
    out = tuple(np.ascontiguousarray(a, dtype=np.float32) for a in (pos, vel))
    for a in out:
        a.setflags(write=False)
    return out


def planes(cfg):
    """per axis the f32 values a clamped coordinate can have: the plane as the f32 participants form it and the f64 plane rounded to f32"""
    sc = cfg["scene"]
    off = clamp_offset(cfg)
    lo = [{np.float32(np.float32(b) + np.float32(off)), np.float32(float(b) + off)} for b in sc["box_min"]]
    hi = [{np.float32(np.float32(b) - np.float32(off)), np.float32(float(b) - off)} for b in sc["box_max"]]
    return lo, hi


def clamped(cfg, pos):
    """bool (N, 3): entries sitting exactly on a clamp plane.  Empty where the scene has wall particles instead of clamp planes."""
    pos = np.asarray(pos, dtype=np.float32)
    out = np.zeros(pos.shape, dtype=bool)
    if cfg["solver"].get("boundary_handle", True):
        return out
    lo, hi = planes(cfg)
    for a in range(3):
        for v in lo[a] | hi[a]:
            out[:, a] |= pos[:, a] == v
    return out


class Result(dict):
    """name -> array of one participant after one step, plus .counts = (n_dens, n_div, capped) -- pressure iterations, iisph's exit flag (1: the
    loop left on "trend to divergence"), 1 at the iteration cap; zeros for wcsph --, .nbr = neighbour counts of the step's INPUT positions
    (wcsph: of the uploaded state, in every step), .lost and .probe (whatever the caller's probe returned after the step)"""


def _finish(res, counts, nbr, lost=0, probe=None):
    res.counts = tuple(int(v) for v in counts)
    res.nbr = nbr.astype(np.int64)
    res.lost = int(lost)
    res.probe = probe
    for a in res.values():
        a.setflags(write=False)
    res.nbr.setflags(write=False)
    return res


def run_oracle(scene, seed, compression, steps, precision, schedule=0, vel_amp=VEL_AMP, num_threads=8):
    """[Result after step 1, ..., after step `steps`], free-running from state(scene, seed, compression).  schedule != 0: one seeded legal execution of
    the reference's races."""
    cfg = config(scene)
    solver = cfg["solver"]["name"]
    o = orc.Oracle(cfg, num_threads=num_threads, precision=precision)
    if schedule:
        o.set_schedule(schedule, 1)
    pos, vel = state(scene, seed, compression, vel_amp)
    o.set(orc.F_POS, pos); o.set(orc.F_VEL, vel)
    out, nbr = [], None
    for s in range(steps):
        if nbr is None or solver != "wcsph":          # F_NBR_COUNT is refreshed inside an iisph step, not inside a pcisph or wcsph one: count here
            o.build_grid(); o.compute_nbr_count()
            nbr = o.get(orc.F_NBR_COUNT)
        if solver == "wcsph":
            o.step_wcsph(1)
            counts = (0, 0, 0)
        else:
            capped = (o.step_pcisph if solver == "pcisph" else o.step_iisph)(1)
            counts = (o.last_stats.n_dens, o.last_stats.n_div, capped)
        res = Result((name, o.get(f)) for name, f in FIELDS[solver])
        out.append(_finish(res, counts, nbr, o.lost))
    o.close()
    return out


@functools.lru_cache(maxsize=None)
def references(scene, seed, compression, steps=STEPS, vel_amp=VEL_AMP):
    """(f32 oracle, f64 oracle) per step: computed once, shared by every test that needs them, never written to."""
    return (run_oracle(scene, seed, compression, steps, "f32", vel_amp=vel_amp), run_oracle(scene, seed, compression, steps, "f64", vel_amp=vel_amp))


def run_handle(sim, scene, seed, compression, steps, vel_amp=VEL_AMP, probe=None):
    """The same on a library handle (cfd_taichi_amd._native.Simulation) created by the caller under whatever overrides select the path."""
    solver = solver_of(scene)
    pos, vel = state(scene, seed, compression, vel_amp)
    sim.upload(F_POS, pos); sim.upload(F_VEL, vel)
    out, nbr = [], None
    for s in range(steps):
        if nbr is None or solver != "wcsph":
            sim.build_neighbors()
            nbr = sim.download(F_NBR_COUNT)
        st = sim.step(1)
        counts, lost = ((st.n_dens, st.n_div, st.capped), st.lost) if st is not None else ((0, 0, 0), 0)
        res = Result((name, sim.download(f)) for name, f in FIELDS[solver])
        out.append(_finish(res, counts, nbr, lost, probe(sim) if probe else None))
    return out


def wall_mask(scene, pos0):
    """Particles of the input positions within one support radius (4 r) of a box face: wall lists, the cached wall sums, the clamp."""
    cfg = config(scene)
    h = 4.0 * float(cfg["scene"]["particle_radius"])
    p = np.asarray(pos0, dtype=np.float64)
    lo, hi = np.asarray(cfg["scene"]["box_min"], dtype=np.float64), np.asarray(cfg["scene"]["box_max"], dtype=np.float64)
    return ((p - lo < h) | (hi - p < h)).any(1)


@functools.lru_cache(maxsize=None)
def _wall_positions(scene):
    o = orc.Oracle(config(scene), num_threads=1)
    wall = o.get(orc.F_WALL_POS).astype(np.float64)
    o.close()
    return wall


def wall_neighbours(scene, pos0):
    """Particles of the input positions with a wall particle within h: those the wall sums (and, where they carry pressure, the wall pressure
    term) act on."""
    h = 4.0 * float(config(scene)["scene"]["particle_radius"])
    p, wall = np.asarray(pos0, dtype=np.float64), _wall_positions(scene)
    out = np.zeros(len(p), dtype=bool)
    for i in range(0, len(p), 256):
        out[i:i + 256] = (((p[i:i + 256, None, :] - wall[None, :, :]) ** 2).sum(2) <= h * h).any(1)
    return out


def populations(scene, pos0, r64):
    """name -> mask.  pinned_loops.populations' (all, next to a box face / not, each class of the neighbour count mod 8) and the particles whose
    f64 pressure is > 0 against those where it is 0: the worked tiles of the pressure sweeps against the skipped ones."""
    wall = wall_mask(scene, pos0)
    pops = {"all": np.ones(len(wall), dtype=bool), "wall": wall, "rest": ~wall}
    p = r64[PRESSURE_FIELD[solver_of(scene)]]
    if min(int((p > 0).sum()), int((~(p > 0)).sum())) >= MIN_SPLIT:
        pops["p>0"], pops["p=0"] = p > 0, ~(p > 0)
    for k in range(8):
        pops["mod8=%d" % k] = r64.nbr % 8 == k
    return pops


def pool(scene):
    return Pool(FIELDS[solver_of(scene)])


def add_step(pl, scene, seed, compression, step, cand, r32, r64, vel_amp=VEL_AMP):
    """one step of one candidate into a Pool: the populations other than the mod-8 classes per step"""
    pl.add(scene, seed, cand, r32, r64, pops=populations(scene, state(scene, seed, compression, vel_amp)[0], r64), tag="step%d" % (step + 1))


def predicted_builds(pos0, positions, skin=VERLET_SKIN, h=None):
    """The Verlet build count after each step as k_wcsph_force_rx's rule gives it on positions `positions[s]` (after step s + 1): the integrator of
    a step flags a rebuild when a particle ends more than skin / 2 (times h) from where the lists were last built, and the next step rebuilds.
    Returns (counts, margins): margins[s] = max displacement after step s + 1 / threshold."""
    thr = 0.5 * skin * h
    x0, builds, flagged, counts, margins = np.asarray(pos0, dtype=np.float64), 0, True, [], []
    prev = x0
    for p in positions:
        if flagged:
            builds, x0 = builds + 1, prev
        p = np.asarray(p, dtype=np.float64)
        far = float(np.sqrt(((p - x0) ** 2).sum(1)).max()) / thr if thr > 0 else np.inf
        flagged = far > 1.0
        counts.append(builds); margins.append(far)
        prev = p
    return counts, margins


# ---- what both GPU files do with a case ----------------------------------------------------------------------------------------------------

KNOB_NAMES = ("SPH_CELL_ORDER", "SPH_STAGE_CAP", "SPH_QUAD", "SPH_TILE_SKIP", "SPH_STAGE", "SPH_ARITH", "SPH_VERLET_SKIN")


def handles(nat, cfg, knobs, monkeypatch, rigid=None, exact=True):
    """nat: cfd_taichi_amd._native, handed in by the GPU files.  (relaxed, exact) created under the development overrides `knobs`; the library must
    name every one of them (sim.overrides()) and no other.  (SPH_VERLET_SKIN is read, and named, by Verlet handles only: not by the exact one.)"""
    for name in KNOB_NAMES:
        monkeypatch.delenv(name, raising=False)
    for name, value in knobs.items():
        monkeypatch.setenv(name, value)
    rx = nat.Simulation(nat.config_from_dict(cfg, arith=nat.ARITH_RELAXED), rigid=rigid)
    ex = nat.Simulation(nat.config_from_dict(cfg), rigid=rigid) if exact else None
    for name in KNOB_NAMES:
        monkeypatch.delenv(name, raising=False)
    for sim in (rx, ex) if exact else (rx,):
        named = sim.overrides()
        for name in KNOB_NAMES:
            want = {"%s=%s" % (name, knobs[name])} if name in knobs and not (sim is ex and name == "SPH_VERLET_SKIN") else set()
            assert {t for t in named if t.startswith(name + "=")} == want, (knobs, named)
    return rx, ex


def check_steps(label, scene, seed, compression, a, b, r32, r64, pool, vel_amp=VEL_AMP, nbr_of_relaxed=True):
    """items 2-6 of the docstring for the steps of one case: a = relaxed handle, b = exact handle (or None)"""
    cfg, solver = config(scene), solver_of(scene)
    for s in range(len(a)):
        tag = "%s step %d" % (label, s + 1)
        runs = [("relaxed", a[s]), ("f32 oracle", r32[s])] + ([("exact", b[s])] if b is not None else [])
        print("%s: counts %s" % (tag, " ".join("%s %s" % (who, r.counts) for who, r in runs + [("f64 oracle", r64[s])])))
        for who, r in runs:
            assert r.counts == r64[s].counts, (tag, who, r.counts, r64[s].counts)
            if who != "relaxed" or nbr_of_relaxed:
                assert np.array_equal(r.nbr, r64[s].nbr), (tag, who, int((r.nbr != r64[s].nbr).sum()))
        if b is not None:          # the exact handle IS the f32 oracle
            for name, _ in FIELDS[solver]:
                same_values(b[s][name], r32[s][name], "%s %s, exact handle and f32 oracle" % (tag, name))
        if not cfg["solver"].get("boundary_handle", True):
            ca, c64 = clamped(cfg, a[s]["pos"]), clamped(cfg, r64[s]["pos"])
            assert np.array_equal(ca, c64), "%s: the clamped set of the relaxed handle is not the f64 oracle's (%d entries differ)" % (tag, int((ca != c64).sum()))
            assert c64.any(1).sum() >= MIN_CLAMPED[solver], tag
        add_step(pool, scene, seed, compression, s, a[s], r32[s], r64[s], vel_amp)
        assert a[s].lost == 0 and all(np.isfinite(x).all() for x in a[s].values()), tag
