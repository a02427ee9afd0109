"""GPU suite of the run diagnostics (sph_diagnostics / sph_diag_record / sph_diag_read).

The yardstick is tests/diagnostics_ref.py (shown fair without the library by test_diagnostics_cpu.py): the sums exact and rounded once, compared
within the derived bound (n + 8) 2^-53 sum |t_i|; n, the step counter, the largest speed and its id, the extent, rho's minimum and maximum, time
and dt bit for bit.  Every figure is printed before it is asserted.  Trajectories are compared bit for bit (particle_flow.same)."""
import ctypes
import os

import numpy as np
import pytest

import adaptive_dt as ad
import diagnostics_ref as dr
import midrun_calls as mc
import harness as h
import particle_flow as pf
from cfd_taichi_amd import _native as nat
from cfd_taichi_amd import mesh, run, scenes

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
TILTED = [1.5, -9.0, 2.5]
BIG = 1e6                                     # "everything on this side" in a removal box


def row_bits(row):
    """the 32 slots of a row (a dict by name, or a record of DIAG_DTYPE) as u64: NaN compares like any other pattern"""
    return h.bits(np.array([float(row[k]) for k in dr.SLOTS], dtype=np.float64))


def same_rows(a, b, when, slots=32):
    ba, bb = row_bits(a)[:slots], row_bits(b)[:slots]
    assert np.array_equal(ba, bb), "%s: slots %s differ: %r vs %r" % (when, [dr.SLOTS[k] for k in np.flatnonzero(ba != bb)],
                                                                      [float(a[dr.SLOTS[k]]) for k in np.flatnonzero(ba != bb)],
                                                                      [float(b[dr.SLOTS[k]]) for k in np.flatnonzero(ba != bb)])


def accel_of(sim):
    return F([sim.scalar(nat.S_ACCEL + k) for k in range(3)])


def reference(sim, rho):
    """row() and bounds() of the state the handle holds now, through its downloads and scalars"""
    pos, vel = sim.download(nat.F_POS), sim.download(nat.F_VEL)
    r = sim.download(nat.F_RHO) if rho else None
    m, a = sim.scalar(nat.S_PARTICLE_M), accel_of(sim)
    ref = dr.row(pos, vel, r, m, a, time=sim.time(), dt=sim.scalar(nat.S_DELTA_TIME), step=sim.scalar(nat.S_SIMULATE_CNT))
    return ref, dr.bounds(pos, vel, r, m, a)


def check(sim, when, rho=False):
    """one on-demand row against the reference; returns it"""
    got = sim.diagnostics()
    ref, bnd = reference(sim, rho)
    for name in ("time", "dt", "step"):
        assert got[name] == ref[name], "%s: %s is %r, the handle reports %r" % (when, name, got[name], ref[name])
    assert got["n"] == sim.n_fluid
    dr.check_row(got, ref, bnd, when, rho=rho)
    return got


def remove_where(sim, lo, hi, expect):
    """sph_remove_in_box with a box chosen from a download: the count is what the test says"""
    inside = int(pf.in_box(sim.download(nat.F_POS), lo, hi).sum())
    assert inside == expect, (inside, expect)
    assert sim.remove_in_box(lo, hi) == expect


def levels(sim, axis):
    """the lattice's coordinates on an axis, ascending, and half a spacing"""
    v = np.unique(sim.download(nat.F_POS)[:, axis])
    return v, F(0.5) * (v[1] - v[0])


def shrink_to(sim, survivors):
    """1, 63, 64 or 65 survivors of the 8 x 10 x 8 lattice (index order x, z, y: a layer is 64 particles)"""
    (x, hx), (y, hy), (z, hz) = levels(sim, 0), levels(sim, 1), levels(sim, 2)
    n = sim.n_fluid
    if survivors == 65:                       # the bottom layer and one particle of the second
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


# ---- 1: on demand against the reference ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["linear", "morton"])
@pytest.mark.parametrize("walls", ["wall", "clamp"])
@pytest.mark.parametrize("solver", pf.SOLVERS)
def test_on_demand_against_the_reference(solver, walls, order, monkeypatch):
    sim = h.make_handle(pf.config(solver, walls, 640), monkeypatch, h.MORTON if order == "morton" else h.LINEAR)
    when = "%s %s %s" % (solver, walls, order)
    r0 = check(sim, when + ", step 0")
    assert r0["kinetic"] == 0.0 and r0["vmax"] == 0.0 and r0["vmax_id"] == 0.0 and r0["step"] == 0.0
    sim.step(1)
    check(sim, when + ", step 1")
    sim.step(9)
    r10 = check(sim, when + ", step 10")                  # right after a step: the densities do not describe the new positions
    assert r10["kinetic"] > 0.0 and r10["time"] > 0.0 and r10["step"] == 10.0
    sim.compute_density()
    check(sim, when + ", step 10, after compute_density", rho=True)
    sim.close()


@pytest.mark.parametrize("solver", ["wcsph", "dfsph"])
def test_an_odd_count_after_add_particles(solver, monkeypatch):
    cfg = pf.config(solver, "wall", 640, capacity=704)
    sim = h.make_handle(cfg, monkeypatch)
    sim.step(2)
    assert sim.add_particles(pf.layer_above(cfg, 640, 37), np.tile(F([0.25, -1, 0.5]), (37, 1))) == 640 and sim.n_fluid == 677
    assert check(sim, solver + " 677, added")["n"] == 677.0
    sim.step(3)
    check(sim, solver + " 677, three steps on")
    sim.compute_density()
    check(sim, solver + " 677, with densities", rho=True)
    sim.close()


@pytest.mark.parametrize("survivors", [1, 63, 64, 65])
def test_small_counts_after_remove_in_box(survivors, monkeypatch):
    sim = h.make_handle(pf.config("wcsph", "wall", 640), monkeypatch)
    shrink_to(sim, survivors)
    sim.upload(nat.F_VEL, ad.velocities(survivors, 2.0, seed=survivors))
    assert check(sim, "%d survivors, uploaded velocities" % survivors)["n"] == float(survivors)
    sim.step(2)
    check(sim, "%d survivors, two steps on" % survivors)
    sim.close()


def test_uploaded_velocities_uniform_unique_and_tied(monkeypatch):
    sim = h.make_handle(pf.config("dfsph", "wall", 640), monkeypatch, h.MORTON)
    sim.step(2)                                            # the device order is the cell order now, not the order of the ids
    sim.upload(nat.F_VEL, np.zeros((640, 3), dtype=F))
    rest = check(sim, "at rest")
    assert rest["vmax"] == 0.0 and rest["vmax_id"] == 0.0                    # all tied at 0: the lowest id
    v = F([0.75, -0.5, 0.25])
    sim.upload(nat.F_VEL, np.tile(v, (640, 1)))
    uni = check(sim, "uniform velocity")
    m = sim.scalar(nat.S_PARTICLE_M)
    for k, a in enumerate("xyz"):
        assert uni["momentum_" + a] == 640 * m * float(v[k])               # n v is exact in f64, so is the sum of 640 equal terms
        assert uni["com_" + a] == rest["com_" + a]
    assert uni["vmax_id"] == 0.0
    vel = ad.velocities(640, 1.0)
    vel[411] = [3, 0, 4]
    sim.upload(nat.F_VEL, vel)
    one = check(sim, "a unique fastest particle")
    assert (one["vmax"], one["vmax_id"]) == (5.0, 411.0)
    vel[600], vel[17], vel[300] = [0, -5, 0], [4, 3, 0], [0, 0, 5]
    sim.upload(nat.F_VEL, vel)
    tie = check(sim, "four particles tied")
    assert (tie["vmax"], tie["vmax_id"]) == (5.0, 17.0)
    sim.close()


def test_tilted_gravity_uses_all_three_components(monkeypatch):
    sim = h.make_handle(pf.config("dfsph", "wall", 640), monkeypatch)
    flat = check(sim, "default gravity")
    sim.set_gravity(TILTED)
    assert list(accel_of(sim)) == list(F(TILTED))
    tilted = check(sim, "tilted, step 0")
    assert tilted["potential"] != flat["potential"]
    sim.step(3)
    check(sim, "tilted, step 3")
    sim.close()


# ---- 2: the stride loop -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [64512, 66560])
def test_the_stride_loop_runs(n, monkeypatch):
    """k_diag_partials launches at most 256 workgroups of 256 threads: 64 512 particles are 252 workgroups, 66 560 need the stride loop"""
    sim = h.make_handle(pf.threshold_config("wcsph", n), monkeypatch)
    assert sim.n_fluid == n and (n > 256 * 256) == (n == 66560)
    vel = ad.velocities(n, 1.0)
    vel[n - 3] = [0, 6, 8]                                 # the fastest particle sits in the loop's second trip at 66 560
    sim.upload(nat.F_VEL, vel)
    got = check(sim, "%d particles, uploaded velocities" % n)
    assert (got["vmax"], got["vmax_id"]) == (10.0, float(n - 3))
    sim.step(1)
    check(sim, "%d particles, one step on" % n)
    sim.close()


# ---- 3: determinism ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", ["dfsph", "pbf"])
def test_same_state_same_bits(solver, monkeypatch):
    cfg = pf.config(solver, "wall", 640)
    a, b = h.make_handle(cfg, monkeypatch, h.MORTON), h.make_handle(cfg, monkeypatch, h.MORTON)
    for s in (a, b):
        s.step(7)
        s.compute_density()
    first = a.diagnostics()
    assert not np.isnan(first["rho_mean"])
    same_rows(first, a.diagnostics(), solver + ": two calls with nothing between them")
    same_rows(first, b.diagnostics(), solver + ": two handles with the same history")
    a.close(); b.close()


# ---- 4: recorded rows are the on-demand rows ------------------------------------------------------------------------------------------------------
def twin_rows(b, steps):
    """twelve step(1) calls with diagnostics() after each, and what the recorded row's density slots must be: the reference of download(F_RHO)"""
    rows, rho = [], []
    for _ in range(steps):
        b.step(1)
        rows.append(b.diagnostics())
        r = b.download(nat.F_RHO)
        rho.append((float(r.min()), float(r.max()), float(dr.exact_sum([r.astype(np.float64)]) / len(r)), (len(r) + 8) * 2.0 ** -53 * float(np.abs(r).sum(dtype=np.float64)) / len(r)))
    return rows, rho


def recorded_equal_on_demand(rec, rows, rho, when):
    assert len(rec) == len(rows), (when, len(rec), len(rows))
    for k, (got, want, (lo, hi, mean, bound)) in enumerate(zip(rec, rows, rho)):
        same_rows(got, want, "%s, row %d" % (when, k + 1), slots=24)
        print("%s, row %d: rho min %.9g max %.9g mean %.17g, reference %.9g %.9g %.17g, bound %.3e" % (when, k + 1, got["rho_min"], got["rho_max"], got["rho_mean"], lo, hi, mean, bound))
        assert (got["rho_min"], got["rho_max"]) == (lo, hi), (when, k + 1)
        assert abs(got["rho_mean"] - mean) <= bound, (when, k + 1, got["rho_mean"], mean, bound)
        assert all(got[n] == 0.0 for n in dr.SLOTS[27:])


RECORDED = [("wcsph", None, "exact"), ("dfsph", h.MORTON, "exact"), ("pcisph", None, "exact"), ("iisph", h.MORTON, "exact"), ("pbf", None, "exact"),
            ("wcsph", None, "relaxed"), ("pcisph", h.MORTON, "relaxed"), ("pbf", None, "relaxed")]


@pytest.mark.parametrize("solver,env,arith", RECORDED, ids=["%s-%s%s" % (s, "morton-" if e else "", a) for s, e, a in RECORDED])
def test_recorded_rows_are_the_on_demand_rows(solver, env, arith, monkeypatch):
    cfg = pf.config(solver, "wall", 640)
    a, b = h.make_handle(cfg, monkeypatch, env, arith), h.make_handle(cfg, monkeypatch, env, arith)
    if arith == "relaxed":
        assert a.scalar(nat.S_ARITH_RELAXED) == 1.0
    a.record_diagnostics(1)
    a.step(12)                                             # one call; wcsph: captured step pairs, replayed
    if solver == "wcsph":
        assert a.scalar(nat.S_GRAPH_LAUNCHES) > 0
    rec, dropped = a.diagnostics_log()
    assert dropped == 0 and list(rec["step"]) == list(range(1, 13))
    rows, rho = twin_rows(b, 12)
    recorded_equal_on_demand(rec, rows, rho, "%s %s" % (solver, arith))
    again, dropped = a.diagnostics_log()
    assert len(again) == 0 and dropped == 0
    for f in (nat.F_POS, nat.F_VEL, nat.F_RHO):
        h.same_bits(a.download(f), b.download(f), "%s: field %d of the recording handle and its twin" % (solver, f))
    a.close(); b.close()


@pytest.mark.parametrize("solver", ["wcsph", "iisph"])
def test_every_third_step_and_a_ring_of_five(solver, monkeypatch):
    cfg = pf.config(solver, "wall", 640)
    a, b, c = (h.make_handle(cfg, monkeypatch) for _ in range(3))
    rows, rho = twin_rows(b, 12)
    a.record_diagnostics(3, rows=8)
    a.step(12)
    rec, dropped = a.diagnostics_log()
    assert dropped == 0 and list(rec["step"]) == [3, 6, 9, 12]
    recorded_equal_on_demand(rec, rows[2::3], rho[2::3], solver + " every third step")
    c.record_diagnostics(1, rows=5)
    c.step(5); c.step(7)
    rec, dropped = c.diagnostics_log()
    assert dropped == 7 and list(rec["step"]) == [8, 9, 10, 11, 12]                 # total = 12: the first seven were overwritten
    recorded_equal_on_demand(rec, rows[7:], rho[7:], solver + " ring of five")
    again, dropped = c.diagnostics_log()
    assert len(again) == 0 and dropped == 7
    c.step(2)                                              # recording goes on behind a read
    rec, dropped = c.diagnostics_log()
    assert list(rec["step"]) == [13, 14] and dropped == 7
    for s in (a, b, c):
        s.close()


@pytest.mark.parametrize("solver", ["wcsph", "pcisph"])
def test_recorded_dt_under_the_adaptive_time_step(solver, monkeypatch):
    cfg = pf.config(solver, "wall", 640)
    max_dt, min_dt = ad.bounds(solver)
    a, b = h.make_handle(cfg, monkeypatch), h.make_handle(cfg, monkeypatch)
    vel = ad.velocities(640, ad.AMPLITUDE[solver])
    for s in (a, b):
        s.upload(nat.F_VEL, vel)
        s.set_param("step_max_dt", max_dt); s.set_param("step_min_dt", min_dt); s.set_param("step_adaptive_dt", 1)
    a.record_diagnostics(1)
    a.step(ad.STEPS)
    rec, _ = a.diagnostics_log()
    dts, times = [], []
    for _ in range(ad.STEPS):
        st = b.step(1)
        dts.append(b.scalar(nat.S_DELTA_TIME)); times.append(b.time())
        if solver == "pcisph":
            assert float(F(st.dt)) == dts[-1]
    print("recorded dt", list(rec["dt"]), "reported", dts)
    assert list(rec["dt"]) == dts and list(rec["time"]) == times and len(set(dts)) > 1
    a.close(); b.close()


def test_recorded_count_follows_add_particles(monkeypatch):
    cfg = pf.config("wcsph", "wall", 640, capacity=704)
    a, b = h.make_handle(cfg, monkeypatch), h.make_handle(cfg, monkeypatch)
    new, vel = pf.layer_above(cfg, 640, 37), np.tile(F([0, -1, 0]), (37, 1))
    a.record_diagnostics(1)
    a.step(2); a.add_particles(new, vel); a.step(2)
    rec, dropped = a.diagnostics_log()
    assert dropped == 0 and list(rec["n"]) == [640, 640, 677, 677] and list(rec["step"]) == [1, 2, 3, 4]
    m = a.scalar(nat.S_PARTICLE_M)
    assert list(rec["mass"]) == [640 * m, 640 * m, 677 * m, 677 * m]
    rows = []
    for k in range(4):
        if k == 2:
            b.add_particles(new, vel)
        b.step(1)
        rows.append(b.diagnostics())
    for k in range(4):
        same_rows(rec[k], rows[k], "count change, row %d" % (k + 1), slots=24)
    a.close(); b.close()


# ---- 5: recording and calling are invisible --------------------------------------------------------------------------------------------------------
def same_handles(a, b, solver, when):
    for f in (nat.F_POS, nat.F_VEL, nat.F_RHO) + ((nat.F_WARM_K,) if solver == "dfsph" else ()):
        h.same_bits(a.download(f), b.download(f), "%s: field %d" % (when, f))
    for which in mc.SCALARS + (nat.S_TIME,):                   # the carried scalars, bit for bit
        sa, sb = np.float64(a.scalar(which)), np.float64(b.scalar(which))
        assert sa.view(np.uint64) == sb.view(np.uint64), "%s: scalar %d is %r, the twin's %r" % (when, which, float(sa), float(sb))


@pytest.mark.parametrize("solver", ["dfsph", "pbf"])
def test_recording_and_calling_are_invisible(solver, monkeypatch):
    cfg = pf.config(solver, "wall", 640)
    a, b = h.make_handle(cfg, monkeypatch, h.MORTON), h.make_handle(cfg, monkeypatch, h.MORTON)
    rng = np.random.default_rng(11)
    a.record_diagnostics(2, rows=4)
    for k in range(20):
        if rng.random() < 0.4:
            a.diagnostics()
        if k == 7:
            a.record_diagnostics(0)
        if k == 12:
            a.record_diagnostics(1, rows=3)
        sa, sb = a.step(1), b.step(1)
        if solver == "dfsph":
            assert mc.stats_bits(sa) == mc.stats_bits(sb), "step %d: statistics" % (k + 1)
    a.diagnostics()
    same_handles(a, b, solver, solver + " after 20 steps")
    rec, dropped = a.diagnostics_log()
    assert list(rec["step"]) == [18, 19, 20] and dropped == 5
    a.close(); b.close()


def test_recording_is_invisible_in_one_wcsph_call(monkeypatch):
    cfg = pf.config("wcsph", "wall", 640)
    a, b = h.make_handle(cfg, monkeypatch), h.make_handle(cfg, monkeypatch)
    a.record_diagnostics(1, rows=32)
    a.step(20); b.step(20)
    assert a.scalar(nat.S_GRAPH_LAUNCHES) > 0 and a.scalar(nat.S_GRAPH_LAUNCHES) == b.scalar(nat.S_GRAPH_LAUNCHES)
    same_handles(a, b, "wcsph", "wcsph step(20)")
    a.record_diagnostics(0)                                # the captured pairs hold the two nodes: dropped with the switch
    a.step(4); b.step(4)
    same_handles(a, b, "wcsph", "wcsph, recording off again")
    rec, dropped = a.diagnostics_log()
    assert list(rec["step"]) == list(range(1, 21)) and dropped == 0
    a.close(); b.close()


def test_recording_is_invisible_to_a_coupled_body(monkeypatch):
    for k in h.KNOBS:
        monkeypatch.delenv(k, raising=False)
    cfg = scenes.get("dfsph_rigid_small")
    rg = mesh.rigid_from_config(cfg)
    a, b = (nat.Simulation(nat.config_from_dict(cfg), rigid=rg) for _ in range(2))
    a.record_diagnostics(1)
    for k in range(10):
        if k in (3, 6):
            check(a, "coupled scene, step %d" % k)         # the fluid's row of a handle with a body
        sa, sb = a.step(1), b.step(1)
        assert mc.stats_bits(sa) == mc.stats_bits(sb), "step %d: statistics" % (k + 1)
        a.rigid_step(); b.rigid_step()
    for f in (nat.F_POS, nat.F_VEL, nat.F_RHO):
        h.same_bits(a.download(f), b.download(f), "coupled scene: field %d" % f)
    ra, rb = a.rigid_scalars(), b.rigid_scalars()
    assert ra == rb, (ra, rb)
    rec, _ = a.diagnostics_log()
    assert list(rec["step"]) == list(range(1, 11)) and (rec["n"] == a.n_fluid).all()
    a.close(); b.close()


# ---- 6: refusals against an undisturbed twin -------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_unchanged(monkeypatch):
    cfg = pf.config("dfsph", "wall", 640)
    slab = h.make_handle(pf.config("wcsph", "wall", 640), monkeypatch, slab_count=2, slab_rank=0)
    h.refused(nat.SPH_E_STATE, slab.diagnostics)
    h.refused(nat.SPH_E_STATE, lambda: slab.record_diagnostics(1))
    h.refused(nat.SPH_E_STATE, slab.diagnostics_log)
    slab.close()
    a, b = h.make_handle(cfg, monkeypatch), h.make_handle(cfg, monkeypatch)
    a.step(3); b.step(3)
    a.record_diagnostics(1, rows=6)
    a.step(2); b.step(2)
    for every, rows in ((-1, 16), (1, 0), (1, -4), (2, (1 << 20) + 1), (1, 2 ** 31 - 1)):
        h.refused(nat.SPH_E_INVALID, lambda: a.record_diagnostics(every, rows))
    lib, n, buf = a._lib, ctypes.c_size_t(99), np.zeros(4, dtype=nat.DIAG_DTYPE)
    assert lib.sph_diagnostics(a._h, None) == nat.SPH_E_INVALID
    assert lib.sph_diagnostics(None, buf.ctypes.data) == nat.SPH_E_INVALID
    assert lib.sph_diag_record(None, 1, 4) == nat.SPH_E_INVALID
    assert lib.sph_diag_read(a._h, None, 4, ctypes.byref(n), None) == nat.SPH_E_INVALID
    assert lib.sph_diag_read(a._h, buf.ctypes.data, 4, None, None) == nat.SPH_E_INVALID
    assert lib.sph_diag_read(None, buf.ctypes.data, 4, ctypes.byref(n), None) == nat.SPH_E_INVALID
    assert n.value == 99 and not buf.view(np.uint8).any()
    for _ in range(3):
        sa, sb = a.step(1), b.step(1)
        assert mc.stats_bits(sa) == mc.stats_bits(sb)
    same_handles(a, b, "dfsph", "after refused calls")
    rec, dropped = a.diagnostics_log()                     # the recording the refusals did not touch: every = 1, six rows
    assert list(rec["step"]) == [4, 5, 6, 7, 8] and dropped == 0
    a.close(); b.close()


# ---- 7: the runner -----------------------------------------------------------------------------------------------------------------------------------
def test_the_runner_writes_the_csv(tmp_path, monkeypatch):
    for k in h.KNOBS:
        monkeypatch.delenv(k, raising=False)
    path = str(tmp_path / "slosh.csv")
    base = ["--config", os.path.join(ROOT, "config", "sloshing_dfsph.json"), "--steps", "20"]
    run.main(base + ["--diag-csv", path, "--diag-every", "2"])
    with_csv = run.LAST["ps"].fluid_particles.pos.to_numpy().copy()
    with open(path) as f:
        lines = f.read().splitlines()
    assert lines[0].split(",") == list(nat.DIAG_SLOTS) and len(lines) == 11
    table = np.array([[float(v) for v in line.split(",")] for line in lines[1:]])
    assert len(set(table[:, 3])) == 1 and table[0, 3] == len(with_csv)
    assert (np.diff(table[:, 0]) > 0).all() and list(table[:, 2]) == list(range(2, 21, 2))
    assert len(set(table[:, 13])) > 1                      # the shaken tank's centre of mass moves along x
    run.main(base)
    h.same_bits(with_csv, run.LAST["ps"].fluid_particles.pos.to_numpy(), "final positions with and without --diag-csv")
