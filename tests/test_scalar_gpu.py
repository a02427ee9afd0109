"""GPU suite of the carried scalar (sph_scalar_* / Simulation.enable_scalar, .scalar, .scalar_rate).

The yardsticks are tests/scalar_ref.py (shown fair and sharp without the library by test_scalar_cpu.py): yardstick A, the definition in numpy f32
in canonical list order, bit for bit -- the sweep through scalar_rate(), the step through T before and after it; yardstick B, the f64 sums with
their derived bound, where the order of a list is not the canonical one (a Verlet handle between two builds).  Both run from the handle's own
downloads.  Trajectories are compared bit for bit.  Every test fails without the entry points."""
import copy
import json
import os

import numpy as np
import pytest

import derived_ref as dr
import forcing as fo
import harness as h
import midrun_calls as mc
import particle_flow as pf
import scalar_ref as sc
import slab_pbf_states as sp
from cfd_taichi_amd import _native as nat
from cfd_taichi_amd import mesh, run, scenes

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
D = 0.05
BIG = 1e6
KAPPA = 2.5e-3                                  # the diffusivity of these tests: dt sum_j c_ij = 1e-3 * 17.1 * 2.5e-3 / 0.01 = 4e-3 on the lattice
PLAIN = dict(h.LINEAR, SPH_QUAD="0")
LAYOUTS = {"plain": PLAIN, "quad": None, "morton": h.MORTON}
SOLVER_ENVS = [("wcsph", None), ("dfsph", h.MORTON), ("pcisph", None), ("iisph", h.MORTON), ("pbf", None)]
SOLVER_IDS = ["wcsph", "dfsph-morton", "pcisph", "iisph-morton", "pbf"]


def disturb(sim, seed, T=None):
    """displaced positions and noisy velocities onto the handle; the scalar on, with a smooth field plus noise (or T)"""
    pos = dr.displaced(sim.download(nat.F_POS), D, seed)
    sim.upload(nat.F_POS, pos)
    sim.upload(nat.F_VEL, dr.velocities(pos, seed))
    sim.enable_scalar(KAPPA, 0.0, 0.5, values=sc.smooth(pos, seed) if T is None else T)


def state_of(sim, diffusivity=KAPPA, body=False):
    return sc.State(sim.download(nat.F_POS), sim.scalar(), sim.scalar(nat.S_PARTICLE_M), sim.scalar(nat.S_SUPPORT_RADIUS), diffusivity,
                    sim.download(nat.F_RIGID_POS, nat.SPECIES_RIGID) if body else None, sim.download(nat.F_RIGID_VOL, nat.SPECIES_RIGID) if body else None)


def rate_a(sim, cfg, diffusivity=KAPPA):
    st = state_of(sim, diffusivity)
    return sc.yardstick_a(st, dr.canonical_lists(dr.Cells(cfg, st.h), st))


def against_a(sim, cfg, when, diffusivity=KAPPA):
    want = rate_a(sim, cfg, diffusivity)
    got = sim.scalar_rate()
    h.same_bits(got, want, "%s: scalar_rate against yardstick A" % when)
    return got


# ---- 1: the sweep against yardstick A, bit for bit; the layouts among themselves ---------------------------------------------------------------------
SEEN = {}


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("walls", ["wall", "clamp"])
@pytest.mark.parametrize("solver", pf.SOLVERS)
def test_sweep_bit_for_bit_against_yardstick_a(solver, walls, layout, monkeypatch):
    cfg = pf.config(solver, walls, 640)
    sim = h.make_handle(cfg, monkeypatch, LAYOUTS[layout])
    disturb(sim, 21)
    got = against_a(sim, cfg, "%s %s %s" % (solver, walls, layout))
    assert np.abs(got).max() > 0.1                     # (not a field of zeros)
    SEEN.setdefault((solver, walls), {})[layout] = got
    for other, earlier in SEEN[(solver, walls)].items():
        h.same_bits(got, earlier, "%s %s: layout %s against layout %s" % (solver, walls, layout, other))
    sim.step(2)
    against_a(sim, cfg, "%s %s %s, two steps on" % (solver, walls, layout))
    sim.close()


@pytest.mark.parametrize("solver,env", [("dfsph", h.MORTON), ("dfsph", h.LINEAR), ("pbf", h.LINEAR)], ids=["dfsph-morton", "dfsph-linear", "pbf-linear"])
def test_relaxed_handles_use_the_same_arithmetic(solver, env, monkeypatch):
    cfg = pf.config(solver, "wall", 640)
    sim = h.make_handle(cfg, monkeypatch, env, arith="relaxed")
    disturb(sim, 22)
    against_a(sim, cfg, "relaxed %s" % solver)
    sim.step(3)
    assert sim.scalar(nat.S_ARITH_RELAXED) == 1.0
    against_a(sim, cfg, "relaxed %s, three steps on" % solver)
    sim.close()


def test_verlet_lists_with_pairs_beyond_h(monkeypatch):
    cfg = pf.config("wcsph", "wall", 640)
    sim = h.make_handle(cfg, monkeypatch, arith="relaxed")
    assert sim.scalar(nat.S_ARITH_RELAXED) == 1.0
    disturb(sim, 41)
    at_build = sim.download(nat.F_POS)               # the upload asks for a rebuild: the next step's lists are built from these positions
    sim.step(1)                                      # ... and its integrator moves them by less than skin / 2: nothing asks for another build
    builds = sim.scalar(nat.S_VERLET_BUILDS)
    assert builds == 1.0
    got = sim.scalar_rate()
    assert sim.scalar(nat.S_VERLET_BUILDS) == builds, "the lists were rebuilt: no stale list was walked"
    st = state_of(sim)
    sup = float(st.h)
    d0 = np.linalg.norm(at_build[:, None, :].astype(np.float64) - at_build[None, :, :], axis=2)
    d1 = np.linalg.norm(st.pos[:, None, :].astype(np.float64) - st.pos[None, :, :], axis=2)
    beyond = int(((d0 <= 1.04 * sup) & (d1 > sup * (1 + 1e-6))).sum())
    print("Verlet handle: %d listed pairs beyond h" % beyond)
    assert beyond > 0
    val, bnd, _ = sc.yardstick_b(st)
    ratio = sc.worst_ratio(got, val, bnd)
    print("Verlet handle: worst error / bound %.3f" % ratio)
    assert ratio <= 1.0
    sim.close()


def test_layouts_agree_on_many_workgroups(monkeypatch):
    """the 5.9 k scene (5879 particles, 23 workgroups, ragged cells): linear and Morton cells, 32-bit lists, and SPH_STAGE_CAP=300 (staged and unstaged
    workgroups in one handle); yardstick A on every 13th particle"""
    cfg = scenes.get("dfsph_small")
    got = {}
    for name, env in (("linear", h.LINEAR), ("morton", h.MORTON), ("nl32", dict(h.MORTON, SPH_NL16="0")), ("mixed", dict(h.MORTON, SPH_STAGE_CAP="300"))):
        sim = h.make_handle(cfg, monkeypatch, env)
        assert sim.n_fluid == 5879
        disturb(sim, 24)
        sim.step(2)
        got[name] = sim.scalar_rate()
        if name == "linear":
            st = state_of(sim)
        sim.close()
    rows = np.arange(3, 5879, 13)
    want = sc.yardstick_a(st, sc.canonical_lists_rows(dr.Cells(cfg, st.h), st, rows), rows=rows)
    h.same_bits(got["linear"][rows], want, "5.9 k particles, linear cells against yardstick A")
    assert np.abs(want).max() > 0.1
    for name in ("morton", "nl32", "mixed"):
        h.same_bits(got[name], got["linear"], "5.9 k particles, %s against linear cells" % name)


def test_layouts_agree_nl16_off_and_a_capacity_without_staging(monkeypatch):
    cfg = pf.config("dfsph", "wall", 640)
    got = {}
    for name, env in (("linear", h.LINEAR), ("nl16", h.MORTON), ("nl32", dict(h.MORTON, SPH_NL16="0")), ("cap64", dict(h.MORTON, SPH_STAGE_CAP="64"))):
        sim = h.make_handle(cfg, monkeypatch, env)
        disturb(sim, 23)
        sim.step(2)
        got[name] = sim.scalar_rate()
        sim.close()
    for name in ("nl16", "nl32", "cap64"):
        h.same_bits(got[name], got["linear"], "640 particles, %s against linear cells" % name)


# ---- 2: a body is insulated -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["coupled", "one-way", "inactive"])
def test_a_body_adds_nothing(mode, monkeypatch):
    for k in h.KNOBS:
        monkeypatch.delenv(k, raising=False)
    cfg = scenes.get("dfsph_rigid_small")
    if mode == "one-way":
        cfg["solver"]["fs_couple"] = False
    if mode == "inactive":
        cfg["solid"]["active"] = False
    sim = nat.Simulation(nat.config_from_dict(cfg), rigid=mesh.rigid_from_config(cfg))
    pos, samples = sim.download(nat.F_POS), sim.download(nat.F_RIGID_POS, nat.SPECIES_RIGID)
    pos[:, 0] += (samples[:, 0].min() - F(0.04)) - pos[:, 0].max()           # the column up to the box: its last layer 0.4 h from the samples
    sim.upload(nat.F_POS, pos)
    sim.enable_scalar(KAPPA, 0.0, 0.5, values=sc.smooth(pos, 5))
    for _ in range(3):
        sim.step(1)
        if mode != "inactive":
            sim.rigid_step()
    got = sim.scalar_rate()
    st = state_of(sim, body=True)
    near = (np.sqrt(((st.pos[:, None, :] - st.body_pos[None, :, :]) ** 2).sum(axis=2)) <= st.h).any(axis=1)
    print("%s body: %d of %d fluid particles have a sample within h" % (mode, int(near.sum()), st.n))
    assert near.any()
    rng = np.random.default_rng(5)
    rows = np.unique(np.concatenate([np.flatnonzero(near)[:250], rng.choice(st.n, 150, replace=False)]))
    cells = dr.Cells(cfg, st.h)
    lists = sc.canonical_lists_rows(cells, st, rows)
    assert (lists.fi[np.arange(lists.fi.shape[1])[None, :] < lists.fc[:, None]] >= st.n).any()      # the lists do hold samples
    want = sc.yardstick_a(st, lists, rows=rows)
    h.same_bits(got[rows], want, "%s body: scalar_rate against yardstick A with the samples ignored" % mode)
    if mode == "coupled":
        val, bnd, _ = sc.yardstick_b(st, rows)
        assert sc.worst_ratio(got[rows], val, bnd) <= 1.0
        counted = sc.yardstick_a(st, lists, mutant="rigid_counted", rows=rows)
        ratio = sc.worst_ratio(counted, val, bnd)
        print("coupled body: a counted sample is %.3g bounds away" % ratio)
        assert ratio > 1.0
    sim.close()


# ---- 3: stepping ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver,env", SOLVER_ENVS, ids=SOLVER_IDS)
def test_five_single_steps_against_yardstick_a(solver, env, monkeypatch):
    cfg = pf.config(solver, "wall", 640)
    sim = h.make_handle(cfg, monkeypatch, env)
    disturb(sim, 31)
    sim.profile_enable(True)
    sim.profile_reset()
    for k in range(5):
        before = sim.scalar()
        rate = rate_a(sim, cfg)
        sim.step(1)
        dt = sim.scalar(nat.S_DELTA_TIME)                      # (the step that the step used: dfsph's CFL rule sits inside it)
        want, _ = sc.advance_a(before, np.zeros((640, 3), dtype=F), rate, dt, 0.0, 0.5, [0, 0, 0])
        h.same_bits(sim.scalar(), want, "%s step %d: T against yardstick A's Euler step" % (solver, k + 1))
        assert not np.array_equal(want, before)
    sim.synchronize()
    assert sim.profile()["scalar"][1] == 5, sim.profile()["scalar"]            # one sweep per step
    sim.close()


@pytest.mark.parametrize("solver,env", SOLVER_ENVS, ids=SOLVER_IDS)
def test_one_call_of_four_steps_equals_four_calls(solver, env, monkeypatch):
    cfg = pf.config(solver, "wall", 640)
    a, b = h.make_handle(cfg, monkeypatch, env), h.make_handle(cfg, monkeypatch, env)
    for s in (a, b):
        disturb(s, 32)
        s.enable_scalar(KAPPA, 0.2, 0.5)
    a.step(4)
    for _ in range(4):
        b.step(1)
    if solver == "wcsph":
        assert a.scalar(nat.S_GRAPH_LAUNCHES) > 0 and b.scalar(nat.S_GRAPH_LAUNCHES) == 0        # two replayed step pairs against four eager steps
    h.same_bits(a.scalar(), b.scalar(), solver + ": T")
    for f in (nat.F_POS, nat.F_VEL):
        h.same_bits(a.download(f), b.download(f), "%s: field %d" % (solver, f))
    a.step(4); b.step(2); b.step(2)                            # ... and a replay of the graphs captured above
    h.same_bits(a.scalar(), b.scalar(), solver + ": T, eight steps")
    h.same_bits(a.download(nat.F_POS), b.download(nat.F_POS), solver + ": pos, eight steps")
    a.close(); b.close()


# ---- 4: invisible when passive ------------------------------------------------------------------------------------------------------------------------
def same_handles(a, b, solver, when):
    fields = (nat.F_POS, nat.F_VEL, nat.F_RHO) + ((nat.F_WARM_K,) if solver == "dfsph" else ()) + ((nat.F_PRESS_ITER,) if solver in ("pcisph", "iisph") else ())
    for f in fields:
        h.same_bits(a.download(f), b.download(f), "%s: field %d" % (when, f))
    for which in mc.SCALARS + (nat.S_TIME,):
        sa, sb = np.float64(a.scalar(which)), np.float64(b.scalar(which))
        assert sa.view(np.uint64) == sb.view(np.uint64), "%s: scalar %d is %r, the twin's %r" % (when, which, float(sa), float(sb))


@pytest.mark.parametrize("solver,env,arith", [(s, e, "exact") for s, e in SOLVER_ENVS] + [("dfsph", h.MORTON, "relaxed"), ("wcsph", None, "relaxed")],
                         ids=SOLVER_IDS + ["dfsph-morton-relaxed", "wcsph-relaxed"])
def test_a_passive_scalar_is_invisible(solver, env, arith, monkeypatch):
    cfg = pf.config(solver, "wall", 640)
    a, b, c = (h.make_handle(cfg, monkeypatch, env, arith=arith) for _ in range(3))
    pos = a.download(nat.F_POS)
    a.enable_scalar(KAPPA, 0.0, 0.5, values=sc.two_valued(pos))
    c.enable_scalar(KAPPA, 0.7, 0.5, values=sc.two_valued(pos))
    c.disable_scalar()                                         # enabled, then disabled: as if never enabled
    for k in range(10):
        sa, sb, s3 = a.step(1), b.step(1), c.step(1)
        if sa is not None:
            assert mc.stats_bits(sa) == mc.stats_bits(sb) == mc.stats_bits(s3), "step %d: statistics" % (k + 1)
    same_handles(a, b, solver, "%s %s after 10 steps, beta = 0" % (solver, arith))
    same_handles(c, b, solver, "%s %s after 10 steps, enabled and disabled" % (solver, arith))
    assert not np.array_equal(a.scalar(), sc.two_valued(pos))   # ... while T did diffuse
    a.close(); b.close(); c.close()


def test_a_passive_scalar_is_invisible_to_a_coupled_body(monkeypatch):
    for k in h.KNOBS:
        monkeypatch.delenv(k, raising=False)
    cfg = scenes.get("dfsph_rigid_small")
    rg = mesh.rigid_from_config(cfg)
    a, b = (nat.Simulation(nat.config_from_dict(cfg), rigid=rg) for _ in range(2))
    a.enable_scalar(KAPPA, 0.0, 0.5, values=sc.two_valued(a.download(nat.F_POS), axis=1))
    for k in range(10):
        sa, sb = a.step(1), b.step(1)
        assert mc.stats_bits(sa) == mc.stats_bits(sb), "step %d: statistics" % (k + 1)
        a.rigid_step(); b.rigid_step()
    for f in (nat.F_POS, nat.F_VEL, nat.F_RHO, nat.F_WARM_K):
        h.same_bits(a.download(f), b.download(f), "coupled scene: field %d" % f)
    h.same_bits(a.download(nat.F_RIGID_POS, nat.SPECIES_RIGID), b.download(nat.F_RIGID_POS, nat.SPECIES_RIGID), "coupled scene: the samples")
    assert a.rigid_scalars() == b.rigid_scalars()
    a.close(); b.close()


# ---- 5: buoyancy ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver,env,forced", [(s, e, False) for s, e in SOLVER_ENVS] + [("dfsph", h.MORTON, True)], ids=SOLVER_IDS + ["dfsph-morton-harmonic"])
def test_the_kick_is_the_stated_one(solver, env, forced, monkeypatch):
    cfg = pf.config(solver, "wall", 640)
    a, b = h.make_handle(cfg, monkeypatch, env), h.make_handle(cfg, monkeypatch, env)
    beta, ref = 0.25, 0.5
    T = sc.two_valued(a.download(nat.F_POS))
    for s in (a, b):
        if forced:
            s.set_gravity(fo.TILT)
            s.set_forcing(fo.AMP, fo.OMEGA, fo.PHASE)
    a.enable_scalar(0.0, beta, ref, values=T)
    a.step(1); b.step(1)
    dt, accel = a.scalar(nat.S_DELTA_TIME), a.accel()
    assert dt == b.scalar(nat.S_DELTA_TIME) and np.array_equal(accel, b.accel())
    if forced:
        assert not np.array_equal(accel, F(fo.TILT))
    _, want = sc.advance_a(T, b.download(nat.F_VEL), np.zeros(640, dtype=F), dt, beta, ref, accel)
    h.same_bits(a.download(nat.F_VEL), want, "%s: vel against the twin's plus the kick" % solver)
    h.same_bits(a.download(nat.F_POS), b.download(nat.F_POS), "%s: pos after one step (the kick follows the integrator)" % solver)
    h.same_bits(a.scalar(), T, "%s: T with D = 0" % solver)
    assert not np.array_equal(want, b.download(nat.F_VEL))
    a.step(4); b.step(4)
    assert not np.array_equal(a.download(nat.F_POS), b.download(nat.F_POS))
    a.close(); b.close()


# ---- 6: conservation -----------------------------------------------------------------------------------------------------------------------------------
def test_conservation_over_a_tiny_dam_break(monkeypatch):
    cfg = pf.config("dfsph", "wall", 640)
    flat, two = h.make_handle(cfg, monkeypatch, h.MORTON), h.make_handle(cfg, monkeypatch, h.MORTON)
    flat.enable_scalar(KAPPA, 0.0, 0.5, values=np.full(640, F(0.7)))
    two.enable_scalar(KAPPA, 0.0, 0.5, values=sc.two_valued(two.download(nat.F_POS)))
    worst = 0.0
    for k in range(20):
        got = two.scalar_rate()
        _, bnd, _ = sc.yardstick_b(state_of(two))
        total, allowed = abs(float(got.astype(np.float64).sum())), float(bnd.sum())
        worst = max(worst, total / allowed)
        assert total <= allowed, "step %d: |sum rate| = %.3e, the sum of the bounds %.3e" % (k, total, allowed)
        flat.step(1); two.step(1)
    print("two-valued T over 20 steps: |sum rate| / sum of bounds at most %.3f; mean T %.9f" % (worst, float(two.scalar().astype(np.float64).mean())))
    h.same_bits(flat.scalar(), np.full(640, F(0.7)), "a uniform T after 20 steps")
    assert np.unique(two.scalar()).size > 2
    flat.close(); two.close()


# ---- 7: particle flow ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver,env", [("wcsph", None), ("dfsph", h.MORTON)], ids=["wcsph", "dfsph-morton"])
def test_677_particles_after_add_particles(solver, env, monkeypatch):
    cfg = pf.config(solver, "wall", 640, capacity=704)
    sim = h.make_handle(cfg, monkeypatch, env)
    disturb(sim, 51)
    sim.step(2)
    before = sim.scalar()
    vel = np.tile(F([0.25, -1, 0.5]), (37, 1))
    assert sim.add_particles(pf.layer_above(cfg, 640, 37), vel, scalar=3.5) == 640 and sim.n_fluid == 677
    T = sim.scalar()
    h.same_bits(T[:640], before, "old rows")
    assert (T[640:] == F(3.5)).all()
    against_a(sim, cfg, solver + " 677, added")
    sim.step(3)
    against_a(sim, cfg, solver + " 677, three steps on")
    assert sim.add_particles(pf.layer_above(cfg, 704, 27), None) == 677          # the inflow value was restored: T_ref
    assert (sim.scalar()[677:] == F(0.5)).all()
    sim.close()


def remove_where(sim, lo, hi, expect):
    inside = pf.in_box(sim.download(nat.F_POS), lo, hi)
    assert int(inside.sum()) == expect, (int(inside.sum()), expect)
    before = sim.scalar()
    assert sim.remove_in_box(lo, hi) == expect
    h.same_bits(sim.scalar(), before[~inside], "the download after remove_in_box: the old one squeezed")


def levels(sim, axis):
    v = np.unique(sim.download(nat.F_POS)[:, axis])
    return v, F(0.5) * (v[1] - v[0])


def shrink_to(sim, survivors, lattice_levels):
    """1, 63, 64 or 65 survivors of the 8 x 10 x 8 lattice (index order x, z, y: a layer is 64 particles); lattice_levels: levels() of the three axes,
    taken while the particles stood on the lattice (one step moves them by a millionth of the spacing)"""
    (x, hx), (y, hy), (z, hz) = lattice_levels
    n = sim.n_fluid
    if survivors == 65:
        remove_where(sim, [-BIG, y[1] + hy, -BIG], [BIG, BIG, BIG], n - 128)
        remove_where(sim, [x[0] + hx, y[0] + hy, -BIG], [BIG, BIG, BIG], 56)
        remove_where(sim, [-BIG, y[0] + hy, z[0] + hz], [BIG, BIG, BIG], 7)
    else:
        remove_where(sim, [-BIG, y[0] + hy, -BIG], [BIG, BIG, BIG], n - 64)
        if survivors == 63:
            remove_where(sim, [x[3] - hx, -BIG, z[5] - hz], [x[3] + hx, BIG, z[5] + hz], 1)
        elif survivors == 1:
            remove_where(sim, [x[0] + hx, -BIG, -BIG], [BIG, BIG, BIG], 56)
            remove_where(sim, [-BIG, -BIG, z[0] + hz], [BIG, BIG, BIG], 7)
    assert sim.n_fluid == survivors


@pytest.mark.parametrize("survivors", [1, 63, 64, 65])
def test_small_counts_after_remove_in_box(survivors, monkeypatch):
    cfg = pf.config("wcsph", "clamp", 640)
    sim = h.make_handle(cfg, monkeypatch)
    pos = sim.download(nat.F_POS)
    sim.enable_scalar(KAPPA, 0.0, 0.5, values=sc.smooth(pos, 60 + survivors))
    lattice_levels = [levels(sim, axis) for axis in range(3)]
    sim.step(1)                                                # (the device order is no longer the API order)
    shrink_to(sim, survivors, lattice_levels)
    got = against_a(sim, cfg, "%d survivors" % survivors)
    assert got.shape == (survivors,)
    assert (got == 0).all() if survivors == 1 else np.abs(got).max() > 0
    if survivors > 1:
        sim.step(2)
        against_a(sim, cfg, "%d survivors, two steps on" % survivors)
    sim.close()


# ---- 8: refusals against an undisturbed twin ----------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_unchanged(monkeypatch):
    cfg = pf.config("dfsph", "wall", 640)
    a, b = h.make_handle(cfg, monkeypatch), h.make_handle(cfg, monkeypatch)
    a.step(3); b.step(3)
    lib, buf = a._lib, np.full(648, F(7.0), dtype=F)
    for call in (a.scalar, a.scalar_rate, lambda: a.set_scalar(buf[:640]), lambda: a.set_scalar_inflow(1.0)):
        assert "before sph_scalar_enable" in h.refused(nat.SPH_E_STATE, call)
    for args in ((-1.0, 0.0, 0.0), (float("nan"), 0.0, 0.0), (float("inf"), 0.0, 0.0), (1.0, float("nan"), 0.0), (1.0, 0.0, float("inf")), (1.0, 1e300, 0.0)):
        h.refused(nat.SPH_E_INVALID, lambda: a.enable_scalar(*args))
    h.refused(nat.SPH_E_STATE, a.scalar)                       # ... and none of them enabled it
    a.disable_scalar()                                         # not enabled: nothing happens
    T = sc.two_valued(a.download(nat.F_POS))
    a.enable_scalar(KAPPA, 0.0, 0.5, values=T)
    for fn in (lib.sph_scalar_download, lib.sph_scalar_upload, lib.sph_scalar_rate):
        assert fn(a._h, None, 640) == nat.SPH_E_INVALID
        assert fn(a._h, buf.ctypes.data, 639) == nat.SPH_E_INVALID and fn(a._h, buf.ctypes.data, 641) == nat.SPH_E_INVALID
        assert fn(None, buf.ctypes.data, 640) == nat.SPH_E_INVALID
    assert (buf == F(7.0)).all()
    bad = T.copy(); bad[17] = np.nan
    h.refused(nat.SPH_E_INVALID, lambda: a.set_scalar(bad))
    h.refused(nat.SPH_E_INVALID, lambda: a.set_scalar_inflow(float("inf")))
    h.refused(nat.SPH_E_INVALID, lambda: a.enable_scalar(-KAPPA, 0.0, 0.5))
    h.same_bits(a.scalar(), T, "T after refused calls")
    h.same_bits(a.download(nat.F_ALPHA), b.download(nat.F_ALPHA), "alpha of the last step (a refused call re-sorts nothing)")
    a.enable_scalar(2 * KAPPA, 0.0, 1.5)                       # a second call: the parameters change, T stays
    h.same_bits(a.scalar(), T, "T after a second enable")
    against_a(a, cfg, "after a second enable", 2 * KAPPA)
    for _ in range(3):
        sa, sb = a.step(1), b.step(1)
        assert mc.stats_bits(sa) == mc.stats_bits(sb)
    same_handles(a, b, "dfsph", "after refused calls")
    a.close(); b.close()


def test_a_slab_handle_refuses(tmp_path):
    cfg = copy.deepcopy(sp.config("long_wall"))               # the long tank of the sharded tests: two slabs that both hold fluid
    cfg["solver"]["name"], cfg["solver"]["delta_time"] = "dfsph", 1e-3
    scene, out = tmp_path / "scene.json", tmp_path / "out.json"
    scene.write_text(json.dumps(cfg))
    r = h.run_ranks(os.path.join(ROOT, "tests", "slab_scalar_worker.py"), ["--scene", scene, "--world", 2, "--steps", 3, "--out", out], 2, "loopback", out)
    assert r["world"] == 2 and r["n"] == sp.N_LONG
    for name in ("enable", "disable", "download", "upload", "rate", "set_inflow"):
        assert r["codes"][name] == [r["state_code"]] * 2, (name, r["codes"][name])
        assert all("slab" in m for m in r["messages"][name]), r["messages"][name]
    assert r["first_difference"] is None, r["first_difference"]


# ---- 9: the runner and the profile ----------------------------------------------------------------------------------------------------------------------
def read_ply(path):
    with open(path) as f:
        lines = f.read().splitlines()
    end = lines.index("end_header")
    return lines[:end + 1], np.array([[float(v) for v in line.split()] for line in lines[end + 1:]])


def test_the_runner_writes_the_scalar_column(tmp_path, monkeypatch):
    for k in h.KNOBS:
        monkeypatch.delenv(k, raising=False)
    cfg = scenes.get("lock_exchange_dfsph")
    cfg["scene"]["output_fps"] = 2000                 # a frame per step of 1e-3 s
    path = str(tmp_path / "lock.json")
    with open(path, "w") as f:
        json.dump(cfg, f)
    with_dir, plain_dir = str(tmp_path / "with"), str(tmp_path / "plain")
    run.main(["--config", path, "--steps", "3", "--ply-dir", with_dir, "--ply-fields", "cover,scalar"])
    sim = run.LAST["ps"]._sim
    T, pos = sim.scalar(), sim.download(nat.F_POS)
    frames = sorted(os.listdir(with_dir))
    head, table = read_ply(os.path.join(with_dir, frames[-1]))
    assert [l.split()[2] for l in head if l.startswith("property")] == ["x", "y", "z", "red", "green", "blue", "alpha", "cover", "scalar"]
    assert table.shape == (sim.n_fluid, 9) and np.abs(table[:, 8] - T).max() <= 0.5e-6 + 1e-7 and np.abs(table[:, 0:3] - pos).max() <= 0.5e-6 + 1e-7
    assert T.min() >= 0 and T.max() <= 1 and np.unique(T).size > 2 and (T[pos[:, 0] < 0.3] > 0.5).all() and (T[pos[:, 0] > 0.9] < 0.5).all()
    vel = sim.download(nat.F_VEL)
    assert vel[T > 0.9, 1].mean() > vel[T < 0.1, 1].mean()       # the warm half is lifted against the cold one
    run.main(["--config", path, "--steps", "3", "--ply-dir", plain_dir])
    head_plain, table_plain = read_ply(os.path.join(plain_dir, frames[-1]))
    assert [l.split()[2] for l in head_plain if l.startswith("property")] == ["x", "y", "z", "red", "green", "blue", "alpha"]
    assert np.array_equal(table_plain, table[:, :7])


def test_the_dye_scene_runs(monkeypatch):
    for k in h.KNOBS:
        monkeypatch.delenv(k, raising=False)
    frames, t, _ = run.main(["--config", os.path.join(ROOT, "config", "dye_dam_wcsph.json"), "--steps", "3"])
    sim = run.LAST["ps"]._sim
    T, pos = sim.scalar(), sim.download(nat.F_POS)
    assert frames == 3 and T.min() >= 0 and T.max() <= 1 and 0.4 < float((T > 0.5).mean()) < 0.6
    assert (T[pos[:, 1] > 1.7] > 0.5).all() and (T[pos[:, 1] < 1.3] < 0.5).all()


def test_the_profile_counts_one_sweep_per_step(monkeypatch):
    cfg = pf.config("wcsph", "wall", 640)
    on, off = h.make_handle(cfg, monkeypatch), h.make_handle(cfg, monkeypatch)
    on.enable_scalar(KAPPA, 0.1, 0.5, values=sc.two_valued(on.download(nat.F_POS)))
    for s in (on, off):
        s.profile_enable(True)
        s.profile_reset()
        s.step(6)
        s.synchronize()
    assert on.profile()["scalar"][1] == 6 and "scalar" not in off.profile(), (on.profile()["scalar"], off.profile())        # (profile() lists what ran)
    on.scalar_rate()
    on.synchronize()
    assert on.profile()["scalar"][1] == 7
    on.close(); off.close()
