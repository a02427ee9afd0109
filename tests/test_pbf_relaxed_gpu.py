"""GPU suite: the relaxed PBF sweeps (csrc/sph_pbf_kernels.h, RX; SphConfig.arith = SPH_ARITH_RELAXED) against the f64 oracle.

A PBF step has no solver loop; apart from lambda's `con == 0` branch and the clamp planes it is a continuous function of its input, and on the
states of tests/pbf_states.py the f32 and the f64 oracle agree to 1e-7 (pos) ... 2e-5 (vel) with identical discrete sets
(tests/test_pbf_relaxed_cpu.py).  Four participants run the same uploaded state: the relaxed handle, the exact handle, the f32 oracle, the f64
oracle.
  1. the relaxed handle reports SPH_S_ARITH_RELAXED = 1, the exact one 0, and their rho differ in at least one bit;
  2. the exact handle equals the f32 oracle bit for bit on rho, pbf_lambda, delta_pos, pos, vel;
  3. the relaxed handle's `lambda != 0` set and its set of coordinates on a clamp plane are the f64 oracle's;
  4. per field, the per-particle error against the f64 oracle e(i) = ||a_i - f64_i|| / max |f64|: the relaxed handle's q50, q99 and max are
     <= 4 x the f32 oracle's own + 2 x 2^-24 over all particles, over those within a support radius of a box face, and over the rest.
Why 4: the yardstick is the reference's own f32 rounding on the same input.  The exact pair term is a chain of correctly
rounded operations; the relaxed one has v_rsq_f32 (1 ulp), r = r^2 (1 / r) and a handful of FMAs -- the same size of per-term error in sums of
the same order: a factor 2 for that, and a factor 2 for regrouped sums (here: the constant factors taken out of every sum).  The measured ratios
are printed per case (DESIGN.md section 4b holds the table)."""
import numpy as np
import pytest

import pbf_states as pb
from cfd_taichi_amd import _native as nat
from cfd_taichi_amd import scenes
from harness import same_values, squeezed
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

KNOB_NAMES = ("SPH_QUAD", "SPH_CELL_ORDER", "SPH_CELL_TILE")
# the four handles of tests/test_second_restatement_gpu.py's PBF cases: which kernels and which cell order
VARIANTS = {"quad-linear": {},
         "plain-linear": {"SPH_QUAD": "0"},
         "quad-morton": {"SPH_CELL_ORDER": "morton", "SPH_CELL_TILE": "4"},
         "plain-morton": {"SPH_CELL_ORDER": "morton", "SPH_CELL_TILE": "4", "SPH_QUAD": "0"}}


def handles(cfg, knobs, monkeypatch):
    """(relaxed, exact) under the development overrides `knobs`; every knob that was set must be named by sim.overrides()"""
    for name in KNOB_NAMES:
        monkeypatch.delenv(name, raising=False)
    for name, value in knobs.items():
        monkeypatch.setenv(name, value)
    rx = nat.Simulation(nat.config_from_dict(cfg, arith=nat.ARITH_RELAXED))
    ex = nat.Simulation(nat.config_from_dict(cfg))
    for name in KNOB_NAMES:
        monkeypatch.delenv(name, raising=False)
    for sim in (rx, ex):
        named = sim.overrides()
        for name in KNOB_NAMES:
            assert [t for t in named if t.startswith(name + "=")] == (["%s=%s" % (name, knobs[name])] if name in knobs else []), (knobs, named)
    return rx, ex


def held(label, cfg, pos0, cand, r32, r64, ratios, fields=None, sets=True):
    """items 3 and 4 of the docstring for one step of one participant; collects the worst ratio per field.  sets: on the states whose discrete sets
    tests/test_pbf_relaxed_cpu.py has shown to agree between the two oracles"""
    for who, r in (("f32 oracle", r32), ("relaxed handle", cand)) if sets else ():
        for what, a, b in zip(("lambda != 0", "clamped"), pb.discrete_sets(cfg, r), pb.discrete_sets(cfg, r64)):
            assert np.array_equal(a, b), "%s: the %s set of the %s is not the f64 oracle's (%d entries differ)" % (label, what, who, int((a != b).sum()))
    for a in cand.values():
        assert np.isfinite(a).all(), label
    failures, worst = pb.check(label, cfg, pos0, cand, r32, r64, fields)
    for name, w in worst.items():
        ratios[name] = max(ratios.get(name, 0.0), w)
    return failures


def report(label, ratios):
    print("%s worst ratio (relaxed / (f32 oracle + floor)) per field: %s" % (label, "  ".join("%s %.2f" % kv for kv in ratios.items())))


CHAIN = [(sc, kind, kn) for sc, kind, _ in pb.CASES for kn in VARIANTS]


@pytest.mark.parametrize("scene,kind,knobs", CHAIN, ids=["%s-%s-%s" % c for c in CHAIN])
def test_one_relaxed_step_against_the_f64_oracle(scene, kind, knobs, monkeypatch):
    """one sweep chain at a time: a single step_pbf(1) from each input state on the four kinds of handle"""
    cfg = scenes.get(scene)
    label = "%s %s %s:" % (scene, kind, knobs)
    failures, ratios = [], {}
    for seed in pb.SEEDS:
        rx, ex = handles(cfg, VARIANTS[knobs], monkeypatch)
        try:
            a, b = pb.run_handle(rx, scene, kind, seed, 1)[0], pb.run_handle(ex, scene, kind, seed, 1)[0]
            assert rx.scalar(nat.S_ARITH_RELAXED) == 1.0 and ex.scalar(nat.S_ARITH_RELAXED) == 0.0
        finally:
            rx.close(); ex.close()
        r32, r64 = (r[0] for r in pb.references(scene, kind, seed, dict((c[:2], c[2]) for c in pb.CASES)[(scene, kind)]))
        for name, _ in pb.FIELDS:          # the exact handle IS the f32 oracle
            same_values(b[name], r32[name], "%s seed %d %s, exact handle and f32 oracle" % (label, seed, name))
        assert not np.array_equal(a["rho"], b["rho"]), "the relaxed handle gave the exact handle's rho: it ran the exact sweeps"
        if kind == "clamp":
            assert pb.clamped(cfg, a["pos"]).any(1).sum() >= 50
        failures += held("%s seed %d" % (label, seed), cfg, pb.pbf_state(scene, kind, seed)[0], a, r32, r64, ratios)
    report(label, ratios)
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("scene,kind,steps", [pb.CASES[0], pb.CASES[2]], ids=["wall-bulk-5", "clamp-clamp-3"])
def test_free_running_relaxed_steps(scene, kind, steps, monkeypatch):
    """the default relaxed handle over the windows in which the CPU test shows the discrete sets of the two oracles to agree: the bound in
    every step, against the f32 oracle's error in that step"""
    cfg = scenes.get(scene)
    failures = []
    for seed in pb.SEEDS:
        rx, ex = handles(cfg, {}, monkeypatch)
        ex.close()
        try:
            got = pb.run_handle(rx, scene, kind, seed, steps)
            assert rx.scalar(nat.S_ARITH_RELAXED) == 1.0
        finally:
            rx.close()
        r32, r64 = pb.references(scene, kind, seed, steps)
        for s in range(steps):
            ratios = {}
            label = "%s %s seed %d step %d:" % (scene, kind, seed, s + 1)
            failures += held(label, cfg, pb.pbf_state(scene, kind, seed)[0], got[s], r32[s], r64[s], ratios)
            report(label, ratios)
    assert not failures, "\n".join(failures)


# ---- blocks of any size (tests/test_pbf_gpu.py: water_block, squeeze) ----------------------------------------------------------------------

def water_block(nx, ny, nz, margin=0.5):
    """pbf_tiny_wall's scene (r = 0.025, Akinci walls) with a block of nx x ny x nz particles at (0.1, 0.1, 0.1) in a box `margin` larger than it"""
    cfg = scenes.get("pbf_tiny_wall")
    d = 2 * cfg["scene"]["particle_radius"]
    ws = [round(n * d, 6) for n in (nx, ny, nz)]
    cfg["scene"]["box_max"] = [round(w + margin, 6) for w in ws]
    cfg["fluid"].update(start_pos=[0.1, 0.1, 0.1], water_size=ws)
    return cfg


def squeezed_oracles(cfg, steps, num_threads, after=None):
    """(start positions, f32 fields, f64 fields) after `steps` squeezed steps (and `after(o)`) on both oracles"""
    out, pos0 = [], None
    for precision in ("f32", "f64"):
        o = orc.Oracle(cfg, num_threads=num_threads, precision=precision)
        if pos0 is None:
            pos0 = squeezed(o.get(orc.F_POS), 0.9)
        o.set(orc.F_POS, pos0)
        o.step_pbf(steps)
        if after:
            after(o)
        out.append(pb.snapshot(o.get))
        o.close()
    return pos0, out[0], out[1]


@pytest.mark.parametrize("quad", ["1", "0"], ids=["quad", "plain"])
def test_relaxed_ragged_last_workgroup(quad, monkeypatch):
    """629 particles, neither a multiple of 64 nor of 256: the guards of the last workgroup in the three relaxed kernels, quad and plain"""
    cfg = water_block(9, 10, 7)
    rx, ex = handles(cfg, {} if quad == "1" else {"SPH_QUAD": "0"}, monkeypatch)
    ex.close()
    try:
        assert rx.n_fluid == 629 and rx.n_fluid % 64 and rx.n_fluid % 256
        pos0, r32, r64 = squeezed_oracles(cfg, 1, 4)
        rx.upload(nat.F_POS, pos0)
        rx.step_pbf(1)
        got = pb.snapshot(rx.download)
        assert rx.scalar(nat.S_ARITH_RELAXED) == 1.0
    finally:
        rx.close()
    assert (r64["pbf_lambda"] != 0).any()
    ratios = {}
    failures = held("629 particles, %s:" % ("quad" if quad == "1" else "plain"), cfg, pos0, got, r32, r64, ratios, sets=False)
    report("629 particles, %s:" % ("quad" if quad == "1" else "plain"), ratios)
    assert not failures, "\n".join(failures)


def test_relaxed_default_dispatch_above_the_quad_threshold(monkeypatch):
    """67 200 particles, no override: an unforced handle launches the plain relaxed kernels"""
    for name in KNOB_NAMES:
        monkeypatch.delenv(name, raising=False)
    cfg = water_block(42, 40, 40)
    rx = nat.Simulation(nat.config_from_dict(cfg, arith=nat.ARITH_RELAXED))
    try:
        assert rx.overrides() == [], rx.overrides()
        assert rx.n_fluid == 67200
        pos0, r32, r64 = squeezed_oracles(cfg, 1, 16)
        rx.upload(nat.F_POS, pos0)
        rx.step_pbf(1)
        got = pb.snapshot(rx.download)
        assert rx.scalar(nat.S_ARITH_RELAXED) == 1.0
    finally:
        rx.close()
    assert (r64["pbf_lambda"] != 0).any()
    ratios = {}
    failures = held("67 200 particles:", cfg, pos0, got, r32, r64, ratios, sets=False)
    report("67 200 particles:", ratios)
    assert not failures, "\n".join(failures)


def test_compute_density_on_a_relaxed_handle(monkeypatch):
    """sim.compute_density() (k_pbf_lambda's rho_only path in the step's own instantiation) after three squeezed steps: rho within the bound of
    the f64 oracle's compute_all_rho; pbf_lambda, delta_pos, pos and vel untouched"""
    cfg = scenes.get("pbf_tiny_wall")
    rx, ex = handles(cfg, {}, monkeypatch)
    ex.close()
    try:
        pos0, r32, r64 = squeezed_oracles(cfg, 3, 8, after=lambda o: (o.build_grid(), o.compute_rho()))
        rx.upload(nat.F_POS, pos0)
        rx.step_pbf(3)
        before = pb.snapshot(rx.download)
        rx.compute_density()
        got = pb.snapshot(rx.download)
        assert rx.scalar(nat.S_ARITH_RELAXED) == 1.0
    finally:
        rx.close()
    assert (before["pbf_lambda"] != 0).any(), "pbf_lambda is all zero: 'untouched' would prove nothing"
    for name in ("pbf_lambda", "delta_pos", "pos", "vel"):
        same_values(got[name], before[name], "%s before and after compute_density" % name)
    ratios = {}
    failures = held("compute_density:", cfg, pos0, got, r32, r64, ratios, fields=("rho",), sets=False)
    report("compute_density:", ratios)
    assert not failures, "\n".join(failures)


def test_mirror_api(monkeypatch):
    from cfd_taichi_amd import ParticleSystem, pbf_solver
    for name in KNOB_NAMES + ("SPH_ARITH",):
        monkeypatch.delenv(name, raising=False)
    cfg = scenes.get("pbf_tiny_wall")
    solver = pbf_solver(ParticleSystem(cfg), cfg, arith="relaxed")
    assert solver.arith == "relaxed" and solver._sim.scalar(nat.S_ARITH_RELAXED) == 1.0
    ps = ParticleSystem(cfg, arith="relaxed")
    solver = pbf_solver(ps, cfg)
    assert solver.arith == "relaxed" and solver._sim.scalar(nat.S_ARITH_RELAXED) == 1.0
    ps = ParticleSystem(cfg)
    solver = pbf_solver(ps, cfg)
    assert solver.arith == "exact" and solver._sim.scalar(nat.S_ARITH_RELAXED) == 0.0
    o = orc.Oracle(cfg, num_threads=8)
    try:
        pos0 = squeezed(o.get(orc.F_POS), 0.9)
        o.set(orc.F_POS, pos0)
        ps.fluid_particles.pos.from_numpy(pos0)
        solver.step(2); o.step_pbf(2)
        same_values(ps.fluid_particles.pos.to_numpy(), o.get(orc.F_POS), "pos")
        same_values(ps.fluid_particles.vel.to_numpy(), o.get(orc.F_VEL), "vel")
        same_values(solver.pbf_lambda.to_numpy(), o.get(orc.F_PBF_LAMBDA), "pbf_lambda")
        assert (solver.pbf_lambda.to_numpy() != 0).any()
    finally:
        o.close()
