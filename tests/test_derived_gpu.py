"""GPU suite of the derived per-particle fields (sph_derived / Simulation.derived).

The yardsticks are tests/derived_ref.py (shown fair and sharp without the library by test_derived_cpu.py): yardstick A, the definition in numpy f32
in canonical list order, bit for bit; yardstick B, the f64 sums with their derived bound, where the order of a list is not the canonical one (a
Verlet handle between two builds) or the state is too large for A's lists (the body scene).  Both run from the handle's own downloads.  Trajectories
are compared bit for bit (particle_flow.same).  Every test fails without the entry point."""
import ctypes
import os

import numpy as np
import pytest

import derived_ref as dr
import midrun_calls as mc
import harness as h
import particle_flow as pf
from cfd_taichi_amd import _native as nat
from cfd_taichi_amd import mesh, run, scenes

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
D = 0.05
BIG = 1e6
NAMES = tuple(name for name, _, _ in dr.QUANTITIES)
PLAIN = dict(h.LINEAR, SPH_QUAD="0")
LAYOUTS = {"plain": PLAIN, "quad": None, "morton": h.MORTON}


def disturb(sim, seed):
    """displaced positions and velocities A x + b + noise onto the handle"""
    pos = dr.displaced(sim.download(nat.F_POS), D, seed)
    sim.upload(nat.F_POS, pos)
    sim.upload(nat.F_VEL, dr.velocities(pos, seed))


def derived17(sim):
    """all five quantities as one (n, 17) array in the order of derived_ref.SLOTS"""
    return np.concatenate([sim.derived(name).reshape(sim.n_fluid, -1) for name in NAMES], axis=1)


def state_of(sim, cfg, body=False):
    """what the sweep read, through the handle's downloads (after sim.derived: rho is the handle's density of these positions)"""
    walls = bool(cfg["solver"].get("boundary_handle", True)) and sim.n_wall > 0
    return dr.State(sim.download(nat.F_POS), sim.download(nat.F_VEL), sim.download(nat.F_RHO), sim.scalar(nat.S_PARTICLE_M), sim.scalar(nat.S_SUPPORT_RADIUS),
                    sim.download(nat.F_WALL_POS, nat.SPECIES_WALL) if walls else None, sim.download(nat.F_WALL_VOL, nat.SPECIES_WALL) if walls else None,
                    sim.download(nat.F_RIGID_POS, nat.SPECIES_RIGID) if body else None, sim.download(nat.F_RIGID_VOL, nat.SPECIES_RIGID) if body else None)


def against_a(sim, cfg, when):
    got = derived17(sim)
    st = state_of(sim, cfg)
    want = dr.yardstick_a(st, dr.canonical_lists(dr.Cells(cfg, st.h), st))
    for name, first, width in dr.QUANTITIES:
        h.same_bits(got[:, first:first + width], want[:, first:first + width], "%s: %s against yardstick A" % (when, name))
    return got


# ---- 1, 2: bit for bit against yardstick A; the layouts among themselves ---------------------------------------------------------------------------
SEEN = {}            # (solver, walls) -> {layout: (n, 17)}: what the cases of (1) returned, for (2)


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("walls", ["wall", "clamp"])
@pytest.mark.parametrize("solver", pf.SOLVERS)
def test_bit_for_bit_against_yardstick_a(solver, walls, layout, monkeypatch):
    cfg = pf.config(solver, walls, 640)
    sim = h.make_handle(cfg, monkeypatch, LAYOUTS[layout])
    disturb(sim, 21)
    got = against_a(sim, cfg, "%s %s %s" % (solver, walls, layout))
    assert np.abs(got[:, 0:9]).max() > 1.0 and np.abs(got[:, 13:16]).max() > 1.0 and got[:, 16].max() > 0.9        # (not a field of zeros)
    SEEN.setdefault((solver, walls), {})[layout] = got
    for other, earlier in SEEN[(solver, walls)].items():
        h.same_bits(got, earlier, "%s %s: layout %s against layout %s" % (solver, walls, layout, other))
    sim.close()


@pytest.mark.parametrize("solver,env", [("dfsph", h.MORTON), ("dfsph", h.LINEAR), ("pbf", h.LINEAR)], ids=["dfsph-morton", "dfsph-linear", "pbf-linear"])
def test_relaxed_handles_use_the_exact_kernel_functions(solver, env, monkeypatch):
    cfg = pf.config(solver, "wall", 640)
    sim = h.make_handle(cfg, monkeypatch, env, arith="relaxed")
    disturb(sim, 22)
    against_a(sim, cfg, "relaxed %s" % solver)
    sim.step(3)
    assert sim.scalar(nat.S_ARITH_RELAXED) == 1.0               # (settled by the first list build)
    against_a(sim, cfg, "relaxed %s, three steps on" % solver)
    sim.close()


def test_layouts_agree_nl16_off_and_a_mixed_handle(monkeypatch):
    """640 particles, dfsph on Morton cells: 16-bit lists (the default), 32-bit lists (SPH_NL16=0), and a capacity at which no workgroup is staged"""
    cfg = pf.config("dfsph", "wall", 640)
    got = {}
    for name, env in (("linear", h.LINEAR), ("nl16", h.MORTON), ("nl32", dict(h.MORTON, SPH_NL16="0")), ("cap64", dict(h.MORTON, SPH_STAGE_CAP="64"))):
        sim = h.make_handle(cfg, monkeypatch, env)
        disturb(sim, 23)
        sim.step(2)
        got[name] = derived17(sim)
        sim.close()
    for name in ("nl16", "nl32", "cap64"):
        h.same_bits(got[name], got["linear"], "640 particles, %s against linear cells" % name)


def test_layouts_agree_on_many_workgroups(monkeypatch):
    """the 5.9 k scene (5879 particles, 23 workgroups, ragged cells): linear and Morton cells, 32-bit lists, and SPH_STAGE_CAP=300 (staged and unstaged workgroups in
    one handle, as tests/test_relaxed_sweeps_gpu.py selects them)"""
    cfg = scenes.get("dfsph_small")
    got = {}
    for name, env in (("linear", h.LINEAR), ("morton", h.MORTON), ("nl32", dict(h.MORTON, SPH_NL16="0")), ("mixed", dict(h.MORTON, SPH_STAGE_CAP="300"))):
        sim = h.make_handle(cfg, monkeypatch, env)
        assert sim.n_fluid == 5879
        disturb(sim, 24)
        sim.step(2)
        got[name] = derived17(sim)
        sim.close()
    assert np.abs(got["linear"][:, 9:12]).max() > 1.0
    for name in ("morton", "nl32", "mixed"):
        h.same_bits(got[name], got["linear"], "5.9 k particles, %s against linear cells" % name)


# ---- 3: ragged counts ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver,env", [("wcsph", None), ("dfsph", h.MORTON)], ids=["wcsph", "dfsph-morton"])
def test_677_particles_after_add_particles(solver, env, monkeypatch):
    cfg = pf.config(solver, "wall", 640, capacity=704)
    sim = h.make_handle(cfg, monkeypatch, env)
    sim.step(2)
    before = sim.derived("cover")
    assert sim.add_particles(pf.layer_above(cfg, 640, 37), np.tile(F([0.25, -1, 0.5]), (37, 1))) == 640 and sim.n_fluid == 677
    got = against_a(sim, cfg, solver + " 677, added")
    assert got.shape == (677, 17) and before.shape == (640,)
    sim.step(3)
    against_a(sim, cfg, solver + " 677, three steps on")
    sim.close()


def remove_where(sim, lo, hi, expect):
    inside = int(pf.in_box(sim.download(nat.F_POS), lo, hi).sum())
    assert inside == expect, (inside, expect)
    assert sim.remove_in_box(lo, hi) == expect


def levels(sim, axis):
    v = np.unique(sim.download(nat.F_POS)[:, axis])
    return v, F(0.5) * (v[1] - v[0])


def shrink_to(sim, survivors):
    """1, 63, 64 or 65 survivors of the 8 x 10 x 8 lattice (index order x, z, y: a layer is 64 particles)"""
    (x, hx), (y, hy), (z, hz) = levels(sim, 0), levels(sim, 1), levels(sim, 2)
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
    cfg = pf.config("wcsph", "clamp", 640)           # (no wall samples: a lone particle has no neighbour of any kind)
    sim = h.make_handle(cfg, monkeypatch)
    sim.derived("velgrad")                            # the feature's memory exists before the count shrinks
    shrink_to(sim, survivors)
    disturb(sim, 30 + survivors)
    got = against_a(sim, cfg, "%d survivors" % survivors)
    assert got.shape == (survivors, 17)
    if survivors == 1:
        assert (got == 0).all(), got
    else:
        assert np.abs(got).max() > 0
    sim.close()


# ---- 4: a Verlet handle between two builds ----------------------------------------------------------------------------------------------------------
def test_verlet_lists_with_pairs_beyond_h(monkeypatch):
    cfg = pf.config("wcsph", "wall", 640)
    sim = h.make_handle(cfg, monkeypatch, arith="relaxed")
    assert sim.scalar(nat.S_ARITH_RELAXED) == 1.0
    disturb(sim, 41)
    at_build = sim.download(nat.F_POS)               # the upload asks for a rebuild: the next step's lists are built from these positions
    sim.step(1)                                      # ... and its integrator moves them by less than skin / 2: nothing asks for another build
    builds = sim.scalar(nat.S_VERLET_BUILDS)
    assert builds == 1.0
    got = derived17(sim)
    assert sim.scalar(nat.S_VERLET_BUILDS) == builds, "the lists were rebuilt: no stale list was walked"
    st = state_of(sim, cfg)
    sup = float(st.h)
    d0 = np.linalg.norm(at_build[:, None, :].astype(np.float64) - at_build[None, :, :], axis=2)
    d1 = np.linalg.norm(st.pos[:, None, :].astype(np.float64) - st.pos[None, :, :], axis=2)
    beyond = int(((d0 <= 1.04 * sup) & (d1 > sup * (1 + 1e-6))).sum())          # listed (the skin is 0.05 h), and now outside the support
    moved = float(np.abs(st.pos - at_build).max())
    print("Verlet handle: %d listed pairs beyond h, largest move %.3e (skin / 2 = %.3e)" % (beyond, moved, 0.025 * sup))
    assert beyond > 0 and 0 < moved < 0.025 * sup
    val, bnd = dr.yardstick_b(st)
    ratio = dr.worst_ratio(got, val, bnd)
    print("Verlet handle: worst error / bound %.3f" % ratio)
    assert ratio <= 1.0
    sim.close()


# ---- 5: a body -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["coupled", "one-way", "inactive"])
def test_a_body_enters_normal_and_cover_only_when_coupled(mode, monkeypatch):
    for k in h.KNOBS:
        monkeypatch.delenv(k, raising=False)
    cfg = scenes.get("dfsph_rigid_small")
    if mode == "one-way":
        cfg["solver"]["fs_couple"] = False
    if mode == "inactive":
        cfg["solid"]["active"] = False
    sim = nat.Simulation(nat.config_from_dict(cfg), rigid=mesh.rigid_from_config(cfg))
    pos, samples = sim.download(nat.F_POS), sim.download(nat.F_RIGID_POS, nat.SPECIES_RIGID)
    pos[:, 0] += (samples[:, 0].min() - F(0.04)) - pos[:, 0].max()           # the column up to the box: its last layer 0.04 = 0.4 h from the samples
    sim.upload(nat.F_POS, pos)
    for _ in range(3):
        sim.step(1)
        if mode != "inactive":
            sim.rigid_step()
    got = derived17(sim)
    st = state_of(sim, cfg, body=True)
    near = (np.sqrt(((st.pos[:, None, :] - st.body_pos[None, :, :]) ** 2).sum(axis=2)) <= st.h).any(axis=1)
    print("%s body: %d of %d fluid particles have a sample within h" % (mode, int(near.sum()), st.n))
    assert near.any()
    if not st.body_vol.any():            # a body that was never binned has no sample volumes yet: the "with" variant takes a typical one
        assert mode == "inactive"
        st.body_vol = np.full(len(st.body_pos), F(0.8 * D ** 3), dtype=F)
    rng = np.random.default_rng(5)
    rows = np.unique(np.concatenate([np.flatnonzero(near)[:250], rng.choice(st.n, 150, replace=False)]))
    with_body = dr.yardstick_b(st, rows)
    st.body_pos, st.body_vol = st.body_pos[:0], st.body_vol[:0]
    without = dr.yardstick_b(st, rows)
    r_with, r_without = dr.worst_ratio(got[rows], *with_body), dr.worst_ratio(got[rows], *without)
    print("%s body: worst error / bound %.3g with the samples in F, %.3g without" % (mode, r_with, r_without))
    if mode == "coupled":
        assert r_with <= 1.0 and r_without > 1.0
        velgrad_only = dr.worst_ratio(got[rows][:, :13], without[0][:, :13], without[1][:, :13])      # nothing of the body in G
        assert velgrad_only <= 1.0
    else:
        assert r_without <= 1.0 and r_with > 1.0
    sim.close()


# ---- 6: invisible ----------------------------------------------------------------------------------------------------------------------------------------
def same_handles(a, b, solver, when):
    fields = (nat.F_POS, nat.F_VEL, nat.F_RHO) + ((nat.F_WARM_K,) if solver == "dfsph" else ()) + ((nat.F_PRESS_ITER,) if solver in ("pcisph", "iisph") else ())
    for f in fields:
        h.same_bits(a.download(f), b.download(f), "%s: field %d" % (when, f))
    for which in mc.SCALARS + (nat.S_TIME,):
        sa, sb = np.float64(a.scalar(which)), np.float64(b.scalar(which))
        assert sa.view(np.uint64) == sb.view(np.uint64), "%s: scalar %d is %r, the twin's %r" % (when, which, float(sa), float(sb))


@pytest.mark.parametrize("solver,env", [("wcsph", None), ("dfsph", h.MORTON), ("pcisph", None), ("iisph", h.MORTON), ("pbf", None)],
                         ids=["wcsph", "dfsph-morton", "pcisph", "iisph-morton", "pbf"])
def test_calling_between_steps_is_invisible(solver, env, monkeypatch):
    cfg = pf.config(solver, "wall", 640)
    a, b = h.make_handle(cfg, monkeypatch, env), h.make_handle(cfg, monkeypatch, env)
    for k in range(10):
        if k % 3 != 2:
            a.derived(NAMES[k % 5])
        if k == 4:
            a.derived("normal"); a.derived("velgrad")
        sa, sb = a.step(1), b.step(1)
        if sa is not None:
            assert mc.stats_bits(sa) == mc.stats_bits(sb), "step %d: statistics" % (k + 1)
    same_handles(a, b, solver, solver + " after 10 steps")
    a.close(); b.close()


def test_calling_is_invisible_across_a_replayed_wcsph_call(monkeypatch):
    cfg = pf.config("wcsph", "wall", 640)
    a, b = h.make_handle(cfg, monkeypatch), h.make_handle(cfg, monkeypatch)
    a.step(4); b.step(4)
    a.derived("vorticity"); a.derived("cover")
    a.step(6); b.step(6)
    assert a.scalar(nat.S_GRAPH_LAUNCHES) > 0 and a.scalar(nat.S_GRAPH_LAUNCHES) == b.scalar(nat.S_GRAPH_LAUNCHES)     # the captured graphs stay usable
    same_handles(a, b, "wcsph", "wcsph step(4), derived, step(6)")
    a.close(); b.close()


def test_calling_is_invisible_to_a_coupled_body(monkeypatch):
    for k in h.KNOBS:
        monkeypatch.delenv(k, raising=False)
    cfg = scenes.get("dfsph_rigid_small")
    rg = mesh.rigid_from_config(cfg)
    a, b = (nat.Simulation(nat.config_from_dict(cfg), rigid=rg) for _ in range(2))
    for k in range(10):
        if k in (0, 3, 6):
            a.derived("normal"); a.derived("normal")
        sa, sb = a.step(1), b.step(1)
        assert mc.stats_bits(sa) == mc.stats_bits(sb), "step %d: statistics" % (k + 1)
        if k == 7:
            a.derived("divergence")                  # between the fluid's step and the body's
        a.rigid_step(); b.rigid_step()
    for f in (nat.F_POS, nat.F_VEL, nat.F_RHO, nat.F_WARM_K):
        h.same_bits(a.download(f), b.download(f), "coupled scene: field %d" % f)
    h.same_bits(a.download(nat.F_RIGID_POS, nat.SPECIES_RIGID), b.download(nat.F_RIGID_POS, nat.SPECIES_RIGID), "coupled scene: the samples")
    ra, rb = a.rigid_scalars(), b.rigid_scalars()
    assert ra == rb, (ra, rb)
    a.close(); b.close()


# ---- 7: the cache --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver,env", [("dfsph", h.MORTON), ("wcsph", None)], ids=["dfsph-morton", "wcsph"])
def test_one_sweep_serves_all_quantities_until_the_state_changes(solver, env, monkeypatch):
    cfg = pf.config(solver, "wall", 640)
    sim = h.make_handle(cfg, monkeypatch, env)
    disturb(sim, 71)
    sim.step(2)
    sim.profile_enable(True)
    sim.profile_reset()
    first = sim.derived("velgrad")
    h.same_bits(sim.derived("velgrad"), first, "two calls")
    vort, div = sim.derived("vorticity"), sim.derived("divergence")
    sim.synchronize()
    assert sim.profile()["derived"][1] == 1, sim.profile()          # one sweep; the later calls launched only the un-sort
    G = first
    h.same_bits(vort, np.stack([G[:, 2, 1] - G[:, 1, 2], G[:, 0, 2] - G[:, 2, 0], G[:, 1, 0] - G[:, 0, 1]], axis=1), "vorticity from the returned velgrad")
    h.same_bits(div, (G[:, 0, 0] + G[:, 1, 1]) + G[:, 2, 2], "divergence from the returned velgrad")
    sim.step(1)
    stepped = sim.derived("velgrad")
    assert sim.profile()["derived"][1] == 2 and not np.array_equal(stepped, first)
    vel = sim.download(nat.F_VEL)
    sim.upload(nat.F_VEL, (vel * F(1.5)).astype(F))
    faster = sim.derived("velgrad")
    assert sim.profile()["derived"][1] == 3 and not np.array_equal(faster, stepped)
    cover = sim.derived("cover")
    sim.compute_density(); sim.build_neighbors()                    # a re-sort: the device order changed under the kept result
    h.same_bits(sim.derived("cover"), cover, "after a re-sort of the same state")
    sim.close()


# ---- 8: refusals against an undisturbed twin -----------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_unchanged(monkeypatch):
    slab = h.make_handle(pf.config("wcsph", "wall", 640), monkeypatch, slab_count=2, slab_rank=0)
    assert "slab" in h.refused(nat.SPH_E_STATE, lambda: slab.derived("cover"))
    slab.close()
    cfg = pf.config("dfsph", "wall", 640)
    a, b = h.make_handle(cfg, monkeypatch), h.make_handle(cfg, monkeypatch)
    a.step(3); b.step(3)
    lib, buf = a._lib, np.full(9 * 640 + 8, F(7.0), dtype=F)
    h.refused(nat.SPH_E_INVALID, lambda: a.derived(5))
    h.refused(nat.SPH_E_INVALID, lambda: a.derived(-1))
    assert lib.sph_derived(a._h, nat.D_VORTICITY, buf.ctypes.data, 640) == nat.SPH_E_INVALID
    assert lib.sph_derived(a._h, nat.D_COVER, buf.ctypes.data, 641) == nat.SPH_E_INVALID
    assert lib.sph_derived(a._h, nat.D_VELGRAD, buf.ctypes.data, 3 * 640) == nat.SPH_E_INVALID
    assert lib.sph_derived(a._h, nat.D_COVER, None, 640) == nat.SPH_E_INVALID
    assert lib.sph_derived(None, nat.D_COVER, buf.ctypes.data, 640) == nat.SPH_E_INVALID
    assert (buf == F(7.0)).all()
    h.same_bits(a.download(nat.F_ALPHA), b.download(nat.F_ALPHA), "alpha of the last step (a refused call re-sorts nothing)")
    for _ in range(3):
        sa, sb = a.step(1), b.step(1)
        assert mc.stats_bits(sa) == mc.stats_bits(sb)
    same_handles(a, b, "dfsph", "after refused calls")
    a.close(); b.close()


# ---- 9: the runner ---------------------------------------------------------------------------------------------------------------------------------------
def read_ply(path):
    with open(path) as f:
        lines = f.read().splitlines()
    end = lines.index("end_header")
    return lines[:end + 1], np.array([[float(v) for v in line.split()] for line in lines[end + 1:]])


def test_the_runner_writes_the_extra_columns(tmp_path, monkeypatch):
    import json
    for k in h.KNOBS:
        monkeypatch.delenv(k, raising=False)
    cfg = pf.config("dfsph", "wall", 640)
    cfg["scene"]["output_fps"] = 2000                 # a frame per step of 1e-3 s
    path = str(tmp_path / "tiny.json")
    with open(path, "w") as f:
        json.dump(cfg, f)
    with_dir, plain_dir = str(tmp_path / "with"), str(tmp_path / "plain")
    run.main(["--config", path, "--steps", "2", "--ply-dir", with_dir, "--ply-fields", "vorticity,cover"])
    sim = run.LAST["ps"]._sim
    vort, cover, pos = sim.derived("vorticity"), sim.derived("cover"), sim.download(nat.F_POS)
    frames = sorted(os.listdir(with_dir))
    assert frames == ["output_000000.ply", "output_000001.ply"]
    head, table = read_ply(os.path.join(with_dir, frames[-1]))
    assert [l.split()[2] for l in head if l.startswith("property")] == ["x", "y", "z", "red", "green", "blue", "alpha", "vort_x", "vort_y", "vort_z", "cover"]
    assert table.shape == (640, 11)
    assert np.abs(table[:, 0:3] - pos).max() <= 0.5e-6 + 1e-7 and np.abs(table[:, 7:10] - vort).max() <= 0.5e-6 + 1e-6 * np.abs(vort).max()
    assert np.abs(table[:, 10] - cover).max() <= 0.5e-6 + 1e-7 and np.abs(vort).max() > 0
    run.main(["--config", path, "--steps", "2", "--ply-dir", plain_dir])
    head_plain, table_plain = read_ply(os.path.join(plain_dir, frames[-1]))
    assert head_plain == ["ply", "format ascii 1.0", "comment created by cfd_taichi_amd", "element vertex 640"] + \
        ["property float %s" % n for n in ("x", "y", "z", "red", "green", "blue", "alpha")] + ["end_header"]
    assert table_plain.shape == (640, 7) and np.array_equal(table_plain, table[:, :7])          # the flag changed no trajectory either
