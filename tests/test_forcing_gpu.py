"""GPU suite: gravity as a vector, constant or harmonic (sph_set_gravity / sph_set_forcing, SPH_S_TIME / SPH_S_ACCEL / SPH_S_GRAVITY_VEC).

The library against the second restatement driven by tests/forcing.py: the restatement is fed, step by step, the vector the handle reports
it used, and every compared field must then be bit-equal.  Scenes: the 640-particle tiny wall / clamp scenes and the tiny coupled scene of
tests/coupled_scenes.py, 10 steps unless stated.  Each solver runs on the two kernel families a scene of this size reaches: the quad sweeps (the
default below 65 536 particles) and the plain ones (SPH_QUAD=0, named by sim.overrides()).

The 1-ulp bound on SPH_S_ACCEL is derived, not measured: the formula is evaluated in f64 and rounded once to f32; the device's f64 sin may be a
few f64 ulps off numpy's, which can move that single rounding across at most one f32 boundary."""
import os

import numpy as np
import pytest

from cfd_taichi_amd import _native as nat
from cfd_taichi_amd import scenes
import coupled_scenes as cs
import forcing as fo
import restatement_compare as rc
from harness import MORTON, make_handle, same_bits

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
WALL = {"wcsph": "wcsph_tiny_wall", "dfsph": "dfsph_tiny_wall", "pcisph": "dfsph_tiny_wall_pcisph", "iisph": "dfsph_tiny_wall_iisph", "pbf": "pbf_tiny_wall"}
CLAMP = {"wcsph": "wcsph_tiny_clamp", "dfsph": "dfsph_tiny_clamp", "pbf": "pbf_tiny_clamp"}
FORCING = (fo.TILT, fo.AMP, fo.OMEGA, fo.PHASE)


def make(monkeypatch, cfg, rg=None, quad=True, arith=nat.ARITH_EXACT, staged=False):
    """a handle on the quad sweeps (default) or the plain ones (SPH_QUAD=0), or with its cells along the Morton curve and the staged sweeps
    (the large-scene path, where dfsph's relaxed arithmetic runs the kernels of csrc/sph_relaxed_kernels.h); the overrides in force are asserted"""
    knobs = {}
    if not quad:
        knobs["SPH_QUAD"] = "0"
    if staged:
        knobs.update(MORTON)
    sim = make_handle(cfg, monkeypatch, knobs, arith, rigid=rg, max_density_iters=100 if cfg["solver"]["name"] == "dfsph" else 0)
    for name in knobs:
        monkeypatch.delenv(name, raising=False)
    named = [o for o in sim.overrides() if o.split("=")[0] in ("SPH_QUAD", "SPH_CELL_ORDER")]
    assert named == (["SPH_QUAD=0"] if not quad else []) + (["SPH_CELL_ORDER=morton"] if staged else []), sim.overrides()
    return sim


def relaxed_pair(monkeypatch, cfg, solver, staged=False):
    """(exact, relaxed) handles on sweeps where the relaxed arithmetic of this solver is in force at 640 particles: pcisph and iisph keep their quad
    sweeps exact, so they take the plain ones"""
    quad = solver not in ("pcisph", "iisph")
    ex = make(monkeypatch, cfg, quad=quad, staged=staged)
    rx = make(monkeypatch, cfg, quad=quad, staged=staged, arith=nat.ARITH_RELAXED)
    return ex, rx


def both_families(monkeypatch, cfg, rg=None):
    return [make(monkeypatch, cfg, rg, quad=True), make(monkeypatch, cfg, rg, quad=False)], ["quad sweeps", "plain sweeps (SPH_QUAD=0)"]


def force(sim):
    sim.set_gravity(fo.TILT)
    sim.set_forcing(fo.AMP, fo.OMEGA, fo.PHASE)


def all_fields(sim, solver):
    return {name: sim.download(rc.F_ID[name]) for name in rc.FIELDS[solver].values()}


def same_handles(a, b, solver, what, names=None):
    fa, fb = all_fields(a, solver), all_fields(b, solver)
    for name in names or fa:
        same_bits(fa[name], fb[name], "%s: %s" % (what, name))


def close(*sims):
    for s in sims:
        s.close()


# ---- 1. the explicit default equals an untouched handle ---------------------------------------------------------------------------------------

# (the staged relaxed kernels with a gravity site of their own are dfsph's: csrc/sph_relaxed_kernels.h, k_dfsph_ext_rx)
@pytest.mark.parametrize("solver,arith", [(s, a) for a in ("exact", "relaxed") for s in WALL] + [("dfsph", "relaxed-staged")])
def test_explicit_default_equals_untouched(solver, arith, monkeypatch):
    cfg = scenes.get(WALL[solver])
    G = F(cfg["scene"]["gravity"])
    kw = {} if arith == "exact" else dict(arith=nat.ARITH_RELAXED, quad=solver not in ("pcisph", "iisph"), staged=arith.endswith("staged"))
    a, b = make(monkeypatch, cfg, **kw), make(monkeypatch, cfg, **kw)
    try:
        same_bits(a.accel(), [G * F(0.0), G * F(-1.0), G * F(0.0)], "the default vector")
        same_bits(a.gravity_vec(), a.accel(), "g of an untouched handle")
        b.set_gravity([G * F(0.0), G * F(-1.0), G * F(0.0)])
        same_bits(b.accel(), a.accel(), "the vector after set_gravity(default)")
        a.step(10); b.step(10)
        same_handles(a, b, solver, "%s, 10 steps" % solver)
        assert a.time() == b.time() and a.time() > 0.0
        assert a.scalar(nat.S_ARITH_RELAXED) == b.scalar(nat.S_ARITH_RELAXED) == (0.0 if arith == "exact" else 1.0)
    finally:
        close(a, b)


def test_gravity_as_a_list_in_the_config_gives_the_same_bits():
    """`gravity: G` and `gravity: [0, -G, 0]` through config reading (gravity_calls applied right after creation)"""
    cfg = scenes.get("dfsph_tiny_wall")
    vec = scenes.get("dfsph_tiny_wall")
    vec["scene"]["gravity"] = [0, -cfg["scene"]["gravity"], 0]
    a, b = nat.Simulation(nat.config_from_dict(cfg), config=cfg), nat.Simulation(nat.config_from_dict(vec), config=vec)
    try:
        same_bits(a.accel(), b.accel(), "the vector")
        a.step(10); b.step(10)
        same_handles(a, b, "dfsph", "number against list")
    finally:
        close(a, b)


# ---- 2. a constant tilt against the restatement -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("scene", list(WALL.values()) + list(CLAMP.values()))
def test_constant_tilt(scene, monkeypatch):
    cfg = scenes.get(scene)
    sims, labels = both_families(monkeypatch, cfg)
    try:
        for sim in sims:
            sim.set_gravity(fo.TILT)
            same_bits(sim.accel(), F(fo.TILT), "the vector after set_gravity")
        s, ev = fo.lockstep(nat, cfg, sims, 10, labels=labels)
        print("%s: iterations %s" % (scene, ev["iters"]))
        assert ev["lost"] == 0 and ev["capped"] == 0, ev
        assert fo.inside_box(cfg, s.pos), "a particle left the box: the comparison could hide behind lost particles"
        for v in ev["vectors"]:
            same_bits(v, F(fo.TILT), "the vector of a step")
    finally:
        close(*sims)


# ---- 3. harmonic forcing ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("solver", ["dfsph", "wcsph", "pbf"])
def test_harmonic_forcing(solver, monkeypatch):
    cfg = scenes.get(WALL[solver])
    sims, labels = both_families(monkeypatch, cfg)
    try:
        for sim in sims:
            force(sim)
            assert sim.time() == 0.0
            assert fo.ulp_distance(sim.accel(), fo.accel_formula(*FORCING, 0.0)).max() <= 1      # read back before the first step
            same_bits(sim.gravity_vec(), F(fo.TILT), "g")
        s, ev = fo.lockstep(nat, cfg, sims, 10, forcing=FORCING, labels=labels)
        print("%s: largest distance to the f64 formula %d ulp; times %s" % (solver, ev["ulps"], ev["times"]))
        assert ev["lost"] == 0 and fo.inside_box(cfg, s.pos)
        assert len({v.tobytes() for v in ev["vectors"]}) == 10, "the vector did not change from step to step"
        for v in ev["vectors"]:
            assert v[1] == F(fo.TILT[1])                                              # no amplitude on y: g's own bits
    finally:
        close(*sims)


# ---- 4. a different dt before every step ------------------------------------------------------------------------------------------------------

def test_varying_dt(monkeypatch):
    cfg = scenes.get("wcsph_tiny_wall")
    dts = [2.5e-4, 1.0e-4, 3.0e-4, 2.0e-4, 1.5e-4, 2.5e-4]
    sims, labels = both_families(monkeypatch, cfg)
    try:
        for sim in sims:
            force(sim)
        s, ev = fo.lockstep(nat, cfg, sims, 6, forcing=FORCING, dts=dts, labels=labels)
        want = np.float64(0.0)
        for dt in dts:
            want = want + np.float64(F(dt))
        assert ev["times"][-1] == float(want), (ev["times"], want)
    finally:
        close(*sims)


# ---- 5. one call equals many ------------------------------------------------------------------------------------------------------------------

def _state(sim):
    return sim.download(nat.F_POS), sim.download(nat.F_VEL), np.float64(sim.time()), sim.accel()


def _same_state(a, b, what):
    sa, sb = _state(a), _state(b)
    same_bits(sa[0], sb[0], what + ": pos"); same_bits(sa[1], sb[1], what + ": vel"); same_bits(sa[3], sb[3], what + ": accel")
    assert sa[2] == sb[2] and sa[2] > 0, (what, sa[2], sb[2])


@pytest.mark.parametrize("solver", ["wcsph", "dfsph", "pbf"])
def test_one_call_equals_many(solver, monkeypatch):
    cfg = scenes.get(WALL[solver])
    a, b = make(monkeypatch, cfg), make(monkeypatch, cfg)
    try:
        force(a); force(b)
        a.step(7)
        for _ in range(7):
            b.step(1)
        _same_state(a, b, "%s: 7 steps in one call against 7 calls" % solver)
        if solver == "wcsph":
            assert a.scalar(nat.S_GRAPH_LAUNCHES) > 0, "the captured step pairs never replayed"
            assert b.scalar(nat.S_GRAPH_LAUNCHES) == 0
    finally:
        close(a, b)


def test_set_gravity_between_two_replayed_calls(monkeypatch):
    """wcsph: a set call between two 4-step calls reaches the replayed graph"""
    cfg = scenes.get("wcsph_tiny_wall")
    a, b = make(monkeypatch, cfg), make(monkeypatch, cfg)
    other = (1.5, -9.0, -3.0)
    try:
        force(a); force(b)
        a.step(4)
        launches = a.scalar(nat.S_GRAPH_LAUNCHES)
        a.set_gravity(other)
        a.step(4)
        for k in range(8):
            if k == 4:
                b.set_gravity(other)
            b.step(1)
        assert launches > 0 and a.scalar(nat.S_GRAPH_LAUNCHES) > launches
        _same_state(a, b, "4 + set_gravity + 4 against single steps")
        same_bits(a.gravity_vec(), F(other), "g")
        # ... and forcing switched off between two calls: the vector is g again, with no arithmetic
        a.set_forcing(None); b.set_forcing(None)
        same_bits(a.accel(), F(other), "the vector with forcing off")
        a.step(4)
        for _ in range(4):
            b.step(1)
        _same_state(a, b, "forcing off, 4 against single steps")
        same_bits(a.accel(), F(other), "the vector with forcing off, after steps")
    finally:
        close(a, b)


# ---- 6. a dynamic body reads the vector, a fixed one does not move -----------------------------------------------------------------------------

@pytest.mark.parametrize("solver", ["wcsph", "dfsph", "pcisph", "iisph"])
def test_dynamic_body_under_tilt(solver, monkeypatch):
    cfg = cs.coupled(solver)
    rg = cs.rigid(cfg)
    sims, labels = both_families(monkeypatch, cfg, rg)
    try:
        for sim in sims:
            sim.set_gravity(fo.TILT)
        s, ev = fo.lockstep(nat, cfg, sims, 10, rg=rg, labels=labels)
        assert abs(float(s.body.vel[0])) > 0 and abs(float(s.body.vel[2])) > 0, "the body never felt the tilt"
        print("%s: body vel %s, iterations %s" % (solver, s.body.vel, ev["iters"]))
    finally:
        close(*sims)


def test_dynamic_body_under_harmonic_forcing(monkeypatch):
    """the body's host step takes the vector the device formed for the solver step before it"""
    cfg = cs.coupled("dfsph")
    rg = cs.rigid(cfg)
    sim = make(monkeypatch, cfg, rg)
    try:
        force(sim)
        fo.lockstep(nat, cfg, [sim], 6, rg=rg, forcing=FORCING)
    finally:
        sim.close()


def test_fixed_body_keeps_its_positions_under_tilt(monkeypatch):
    cfg = cs.coupled("dfsph")
    sim = make(monkeypatch, cfg, cs.rigid(cfg))
    try:
        sim.rigid_set_mode("fixed")
        sim.set_gravity(fo.TILT)
        start = sim.download(nat.F_RIGID_POS, nat.SPECIES_RIGID).copy()
        centroid = sim.rigid_scalars()["centroid"]
        for _ in range(10):
            sim.step(1)
            sim.rigid_step()
        same_bits(start, sim.download(nat.F_RIGID_POS, nat.SPECIES_RIGID), "the fixed body's samples")
        assert sim.rigid_scalars()["centroid"] == centroid
        assert float(np.abs(sim.rigid_load()[0]).max()) > 0, "the fluid never pushed the obstacle"
    finally:
        sim.close()


# ---- 7. the relaxed arithmetic under tilt -----------------------------------------------------------------------------------------------------

def rel(a, b):
    """tests/test_relaxed_gpu.py:47"""
    return float(np.abs(a.astype(np.float64) - b.astype(np.float64)).max() / max(float(np.abs(b).max()), 1e-30))


@pytest.mark.parametrize("solver", list(WALL) + ["dfsph-staged"])
def test_relaxed_under_tilt(solver, monkeypatch):
    """5 steps from rest: positions within north_star's 1e-5 (max norm) of the exact handle under the same tilt; dfsph iteration counts equal"""
    solver, staged = solver.split("-")[0], solver.endswith("staged")
    cfg = scenes.get(WALL[solver])
    ex, rx = relaxed_pair(monkeypatch, cfg, solver, staged=staged)
    try:
        iters = []
        for sim in (ex, rx):
            sim.set_gravity(fo.TILT)
            mine = []
            for _ in range(5):
                st = sim.step(1)
                if solver == "dfsph":
                    mine.append((st.n_div, st.n_dens))
            iters.append(mine)
        err = rel(rx.download(nat.F_POS), ex.download(nat.F_POS))
        print("%s: relaxed against exact under tilt, 5 steps: %.3e" % (solver, err))
        assert err <= 1e-5, err
        assert iters[0] == iters[1], iters
        assert ex.time() == rx.time()
        # (asked after the steps: a staged handle settles its layout, and with it the kernels it runs, at the first list build)
        assert rx.scalar(nat.S_ARITH_RELAXED) == 1.0 and ex.scalar(nat.S_ARITH_RELAXED) == 0.0
    finally:
        close(ex, rx)


# ---- 8. refusals ------------------------------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_handle_unchanged(monkeypatch):
    cfg = scenes.get("dfsph_tiny_wall")
    a, b = make(monkeypatch, cfg), make(monkeypatch, cfg)
    nan, inf = float("nan"), float("inf")
    try:
        force(a); force(b)
        a.step(2); b.step(2)
        before = (a.accel(), a.gravity_vec(), a.time())
        bad_calls = [lambda: a.set_gravity([nan, -9.8, 0.0]), lambda: a.set_gravity([0.0, inf, 0.0]), lambda: a.set_gravity([0.0, -9.8, -inf]),
                     lambda: a.set_forcing([nan, 0.0, 0.0]), lambda: a.set_forcing([1.0, inf, 0.0], [1.0, 1.0, 1.0]),
                     lambda: a.set_forcing([1.0, 1.0, 1.0], [nan, 1.0, 1.0]), lambda: a.set_forcing([1.0, 1.0, 1.0], [1.0, 1.0, 1.0], [0.0, 0.0, inf]),
                     lambda: a.set_forcing([1.0, 1.0, 1.0], None, [0.0, nan, 0.0]), lambda: a.set_time(nan), lambda: a.set_time(inf)]
        for call in bad_calls:
            with pytest.raises(nat.SphError) as e:
                call()
            assert e.value.code == nat.SPH_E_INVALID
        same_bits(before[0], a.accel(), "the vector after the refusals"); same_bits(before[1], a.gravity_vec(), "g after the refusals")
        assert before[2] == a.time()
        a.step(3); b.step(3)
        same_handles(a, b, "dfsph", "3 steps after the refusals")
        _same_state(a, b, "3 steps after the refusals")
    finally:
        close(a, b)


def test_time_is_writable_and_the_vector_follows(monkeypatch):
    cfg = scenes.get("pbf_tiny_wall")
    a = make(monkeypatch, cfg)
    try:
        force(a)
        a.set_time(0.25)
        assert a.time() == 0.25
        assert fo.ulp_distance(a.accel(), fo.accel_formula(*FORCING, 0.25)).max() <= 1
        a.step(1)
        assert a.time() == np.float64(0.25) + np.float64(F(a.scalar(nat.S_DELTA_TIME)))
        a.build_neighbors(); a.compute_density()                                   # stage calls do not advance the clock
        assert a.time() == np.float64(0.25) + np.float64(F(a.scalar(nat.S_DELTA_TIME)))
    finally:
        a.close()


# ---- 9. the runner on the shipped scene -------------------------------------------------------------------------------------------------------

def test_runner_on_the_sloshing_scene():
    from cfd_taichi_amd import run
    cfg = scenes.get("sloshing_dfsph")
    frames, t, _ = run.main(["--config", os.path.join(ROOT, "config", "sloshing_dfsph.json"), "--steps", "5"])
    ps, solver = run.LAST["ps"], run.LAST["solver"]
    pos = ps.fluid_particles.pos.to_numpy()
    assert frames == 5 and len(pos) == 2288
    assert fo.inside_box(cfg, pos)
    assert solver._sim.last_stats.lost == 0
    assert solver.time[None] > 0.0 and abs(solver.time[None] - t) < 1e-9
    a = solver._sim.accel()
    assert a[0] != 0.0 and a[1] == F(-9.8) and a[2] == 0.0, a                    # the config's forcing reached the handle
    assert solver.gravity == 9.8
