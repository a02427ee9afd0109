"""The yardsticks of the carried scalar (tests/scalar_ref.py) shown fair and sharp WITHOUT the library, the discrete maximum principle under the
documented time-step limit, and the Python side: the box initialiser, the config keys, the emitter's key, the PLY column and the binding's names
(DESIGN.md section 6k).  A few seconds in all.

The mutants' worst error / bound ratios as measured (test_the_bound_is_sharp prints them; every one must exceed 1):
    sign 3.9e5 / 3.8e5 / 3.6e5 (wall / clamp / body), no_eta2 7.2e3 / 7.5e3 / 7.3e3, factor_6 9.6e4 / 9.4e4 / 9.1e4,
    t_i_for_t_j 1.9e5 / 1.9e5 / 1.8e5, m_over_rho_j 1.9e5 / 3.5e5 / 3.0e5, reference_gradient 9.6e5 / 9.4e5 / 9.1e5,
    rigid_counted 1.4e6 (body), no_gate 1.4e3 / 1.1e3 / 1.0e3 (on the 5 % skin list)
while yardstick A itself stays below 0.05 of the bound in every order (canonical, two shuffles, the skin list)."""
import math
import os
import re

import numpy as np
import pytest

import derived_ref as dr
import particle_flow as pf
import scalar_ref as sc
import second_restatement as sr
from cfd_taichi_amd import _native as nat
from cfd_taichi_amd import emitter, run, scenes

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = 0.05                                       # particle spacing of the tiny scenes; h = 2 D
DIFFUSIVITY = 2.5e-3
LATTICE_SUM_H2 = 17.0953                       # the undisturbed lattice (spacing 2 r, h = 4 r): sum_j c_ij = 17.0953 D / h^2, so dt <= 0.0585 h^2 / D


def scene_state(walls, seed, body=False):
    """the tiny wall / clamp scene at 640 particles, displaced, with a smooth T plus noise; rho as the reference's density sum of those positions
    (only the m / rho_j mutant reads it).  body: a block of 5 x 5 x 5 samples sunk into the top of the column"""
    cfg = pf.config("dfsph", walls, 640)
    s = sr.Solver(cfg)
    s.pos = dr.displaced(s.pos, D, seed)
    s.prologue()
    s.compute_all_rho()
    bp = bw = None
    if body:
        top = s.pos[:, 1].max()
        mid = F(0.5) * (s.pos.min(axis=0) + s.pos.max(axis=0))
        g = np.arange(5, dtype=F) * F(D)
        bp = (np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3) + F([mid[0] - 2 * D, top - 2 * D, mid[2] - 2 * D])).astype(F) + F(0.013)
        bw = np.full(len(bp), F(0.8 * D ** 3), dtype=F)
    st = sc.State(s.pos, sc.smooth(s.pos, seed), s.m, s.h, DIFFUSIVITY, bp, bw, rho=s.rho)
    return st, dr.Cells(cfg, s.h)


@pytest.fixture(scope="module")
def states():
    """name -> (state, canonical lists, yardstick B's rate, bound and sum_j c_ij): computed once, never changed"""
    out = {}
    for name, walls, seed, body in (("wall", "wall", 11, False), ("clamp", "clamp", 12, False), ("body", "clamp", 13, True)):
        st, cells = scene_state(walls, seed, body)
        out[name] = (st, dr.canonical_lists(cells, st)) + sc.yardstick_b(st)
    return out


# ---- normalisation ------------------------------------------------------------------------------------------------------------------------------
def test_normalisation_on_a_lattice():
    pos, h, m, centre = sc.lattice()
    x = pos.astype(np.float64)
    cfg = pf.config("dfsph", "clamp", 640)
    shifted = (pos + F(0.3)).astype(F)                         # (the canonical lists want positions inside the grid; T is taken at the unshifted ones)
    for T, laplacian, figure in ((x[:, 0] ** 2, 2.0, 1.98310), (x[:, 0] ** 2 + x[:, 1] ** 2 + 0.3 * x[:, 2] + 0.1, 4.0, 3.96620)):
        st = sc.State(pos, T.astype(F), m, h, 1.0)
        val, bnd, csum = sc.yardstick_b(st, [centre])
        print("lattice centre: rate / D = %.6f (analytic %.0f), bound %.2e, sum_j c_ij h^2 / D = %.4f" % (val[0], laplacian, bnd[0], csum[0] * float(h) ** 2))
        assert dr._within(pos[[centre]], pos, h, True, [centre]).sum() == 32
        assert abs(val[0] - figure) <= 1e-4 * figure
        assert abs(val[0] - laplacian) <= 0.02 * laplacian
        assert abs(csum[0] * float(h) ** 2 - LATTICE_SUM_H2) <= 1e-3
        sh = sc.State(shifted, T.astype(F), m, h, 1.0)
        a = sc.yardstick_a(sh, dr.canonical_lists(dr.Cells(cfg, h), sh))
        vs, bs, _ = sc.yardstick_b(sh, [centre])
        assert abs(float(a[centre]) - vs[0]) <= bs[0], (a[centre], vs[0], bs[0])


# ---- antisymmetry ------------------------------------------------------------------------------------------------------------------------------
def test_pair_terms_are_antisymmetric_bit_for_bit(states):
    st, lists = states["wall"][:2]
    eta2, _ = sc.constants(st)
    i, j = np.nonzero(dr._within(st.pos, st.pos, st.h, True))
    assert len(i) > 5000
    tij, _ = sc.pair_terms(st.pos[i], st.pos[j], st.T[i], st.T[j], st.h, eta2)
    tji, _ = sc.pair_terms(st.pos[j], st.pos[i], st.T[j], st.T[i], st.h, eta2)
    differ = st.T[i] != st.T[j]                                # (equal values give +0 times f on both sides: the same zero, not opposite ones)
    assert differ.sum() > 5000 and (tij[differ] != 0).any()
    assert np.array_equal(tij[differ].view(np.uint32), (-tji[differ]).view(np.uint32))
    assert (tij[~differ] == 0).all()


def test_a_uniform_field_has_rate_zero(states):
    for name in ("wall", "body"):
        st, lists = states[name][:2]
        flat = sc.State(st.pos, np.full(st.n, F(0.7)), st.m, st.h, st.D, st.body_pos, st.body_w)
        assert (sc.yardstick_a(flat, lists) == 0).all()
        val, bnd, _ = sc.yardstick_b(flat)
        assert (val == 0).all() and (bnd == 0).all()


# ---- the explicit scheme's limit ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["wall", "clamp"])
def test_maximum_principle_at_half_the_documented_limit(states, name):
    st, lists, _, _, csum = states[name]
    h = float(st.h)
    dt = 0.5 * h * h / (LATTICE_SUM_H2 * st.D)
    print("%s: dt = %.4e (half the lattice's limit), dt max_i sum_j c_ij = %.3f on this displaced state" % (name, dt, dt * csum.max()))
    assert dt * csum.max() <= 1.0
    T = st.T.copy()
    lo, hi = T.min(), T.max()
    spread = float(hi - lo)
    for _ in range(10):
        rate = sc.yardstick_a(sc.State(st.pos, T, st.m, st.h, st.D), lists)
        T, _ = sc.advance_a(T, np.zeros((st.n, 3), dtype=F), rate, dt, 0.0, 0.0, [0, 0, 0])
        assert T.min() >= lo and T.max() <= hi
    assert float(T.max() - T.min()) < spread                   # ... and it did diffuse


# ---- the bound: fair and sharp ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["wall", "clamp", "body"])
def test_the_bound_is_fair(states, name):
    st, lists, val, bnd, _ = states[name]
    assert np.abs(val).max() > 0 and (bnd > 0).all()
    for what, ls in (("canonical", lists), ("shuffle 1", dr.shuffled(lists, 1)), ("shuffle 2", dr.shuffled(lists, 2))):
        ratio = sc.worst_ratio(sc.yardstick_a(st, ls), val, bnd)
        print("%s, %s order: worst error / bound %.3f" % (name, what, ratio))
        assert ratio <= 1.0
    skin = dr.skin_lists(st, 1.05 * float(st.h))
    assert (skin.fc > lists.fc).any()
    ratio = sc.worst_ratio(sc.yardstick_a(st, skin), val, bnd)
    print("%s, a list with 5 %% skin: worst error / bound %.3f" % (name, ratio))
    assert ratio <= 1.0


@pytest.mark.parametrize("mutant", sc.MUTANTS)
def test_the_bound_is_sharp(states, mutant):
    applied = 0
    for name, (st, lists, val, bnd, _) in states.items():
        if mutant == "rigid_counted" and not len(st.body_pos):
            continue
        ls = dr.skin_lists(st, 1.05 * float(st.h)) if mutant == "no_gate" else lists
        ratio = sc.worst_ratio(sc.yardstick_a(st, ls, mutant=mutant), val, bnd)
        print("%s on %s: worst error / bound %.3g" % (mutant, name, ratio))
        assert ratio > 1.0, "%s stays inside the bound on %s" % (mutant, name)
        applied += 1
    assert applied == (1 if mutant == "rigid_counted" else 3)


def test_one_particle_and_a_coincident_pair():
    cfg = pf.config("dfsph", "clamp", 640)
    h = F(2 * D)
    one = sc.State(F([[0.2, 0.2, 0.2]]), F([3.0]), 1000 * D ** 3, h, 1.0)
    assert (sc.yardstick_a(one, dr.canonical_lists(dr.Cells(cfg, h), one)) == 0).all()
    two = sc.State(F([[0.2, 0.2, 0.2], [0.2, 0.2, 0.2]]), F([1.0, 2.0]), 1000 * D ** 3, h, 1.0)
    lists = dr.canonical_lists(dr.Cells(cfg, h), two)
    assert list(lists.fc) == [1, 1]
    a = sc.yardstick_a(two, lists)
    assert np.isfinite(a).all() and (a == 0).all()             # g r = 0 over eta2 > 0


# ---- the step's end -------------------------------------------------------------------------------------------------------------------------------------
def test_the_kick_and_the_euler_step():
    T, vel, rate = F([1.0, 0.0, 0.5]), F([[0, 0, 0], [1, 2, 3], [0.1, 0.2, 0.3]]), F([-2.0, 2.0, 0.0])
    t1, v1 = sc.advance_a(T, vel, rate, 1e-3, 0.0, 0.5, [0, -9.8, 0])
    assert v1 is vel or np.array_equal(v1.view(np.uint32), vel.view(np.uint32))
    assert np.array_equal(t1, T + F(1e-3) * rate)
    t2, v2 = sc.advance_a(T, vel, rate, 1e-3, 0.3, 0.5, [0, -9.8, 0])
    assert np.array_equal(t2, t1)
    assert v2[0, 1] > 0 and v2[1, 1] < vel[1, 1] and v2[2, 1] == vel[2, 1]            # warm rises, cold sinks, T = T_ref is left alone
    assert np.array_equal(v2[:, [0, 2]], vel[:, [0, 2]])
    assert v2[0, 1] == F(F(1e-3) * -(F(0.3) * F(0.5))) * F(-9.8)


# ---- Python: the box initialiser, the config keys, the emitter, the PLY column, the names -------------------------------------------------------------
def test_box_initialiser():
    pos = F([[0.1, 0.1, 0.1], [0.5, 0.1, 0.1], [0.6, 0.1, 0.1], [0.9, 0.5, 0.1]])
    init = {"value": 2.0, "boxes": [{"min": [0.0, 0.0, 0.0], "max": [0.6, 1.0, 1.0], "value": 1.0}, {"min": [0.4, 0.0, 0.0], "max": [1.0, 0.2, 1.0], "value": -3.0}]}
    got = nat.scalar_init_values(pos, init)
    assert got.dtype == F and list(got) == [1.0, -3.0, -3.0, 2.0]          # later boxes win; lo <= x < hi: x = 0.6 (f32) is outside the first box
    assert list(nat.scalar_init_values(pos, {"boxes": []}, default=0.5)) == [0.5] * 4
    edge = F([[np.nextafter(F(0.6), F(0)), 0.1, 0.1], [0.0, 0.0, 0.0]])
    assert list(nat.scalar_init_values(edge, {"value": 0.0, "boxes": [init["boxes"][0]]})) == [1.0, 1.0]
    for bad in ({"values": 1}, {"boxes": [{"min": [0, 0, 0], "max": [1, 1, 1]}]}, {"boxes": [{"min": [0, 0], "max": [1, 1, 1], "value": 1}]}):
        with pytest.raises(ValueError):
            nat.scalar_init_values(pos, bad)


def test_config_keys():
    cfg = pf.config("dfsph", "wall", 640)
    assert nat.scalar_call(cfg) is None
    cfg["scene"]["scalar"] = {"diffusivity": 1e-3, "beta": 0.2}
    assert nat.scalar_call(cfg) == ({"diffusivity": 1e-3, "beta": 0.2, "ref": 0.0}, None)
    cfg["scene"]["scalar"] = {"diffusivity": 0, "ref": 1, "init": {"value": 3}}
    assert nat.scalar_call(cfg) == ({"diffusivity": 0.0, "beta": 0.0, "ref": 1.0}, {"value": 3})
    for bad in ({"diffusivity": -1.0}, {"beta": float("nan")}, {"ref": float("inf")}, {"diffusivty": 1.0}, {"beta": True}, [1, 2]):
        cfg["scene"]["scalar"] = bad
        with pytest.raises(ValueError):
            nat.scalar_call(cfg)


def test_shipped_scenes():
    import json
    for name, solver, beta in (("lock_exchange_dfsph", "dfsph", 0.3), ("dye_dam_wcsph", "wcsph", 0.0)):
        cfg = scenes.get(name)
        with open(os.path.join(ROOT, "config", name + ".json")) as f:
            assert json.load(f) == cfg
        kw, init = nat.scalar_call(cfg)
        assert cfg["solver"]["name"] == solver and kw["beta"] == beta and kw["diffusivity"] > 0 and len(init["boxes"]) == 1
        h = 4 * cfg["scene"]["particle_radius"]
        assert cfg["solver"]["delta_time"] <= 0.5 * h * h / (LATTICE_SUM_H2 * kw["diffusivity"])      # far inside the explicit scheme's limit
        s = sr.Solver(cfg) if name == "lock_exchange_dfsph" else None
        if s is not None:                                     # half warm, half cold
            T = nat.scalar_init_values(s.pos, init, default=kw["ref"])
            assert set(T) == {F(0.0), F(1.0)} and abs(int((T == 1).sum()) - len(T) // 2) <= len(T) // 10


class FakeSim(pf.FakeSim):
    def add_particles(self, pos, vel=None, scalar=None):
        self.scalars = getattr(self, "scalars", []) + [scalar]
        return super().add_particles(pos, vel)


def test_emitter_scalar_key():
    cfg = pf.config("dfsph", "wall", 640, capacity=2048)
    cfg["scene"]["emitters"] = [{"center": [0.3, 0.8, 0.3], "direction": [0, -1, 0], "size": [0.1, 0.1], "speed": 1.0, "scalar": 2.5},
                                {"center": [0.5, 0.8, 0.5], "direction": [0, -1, 0], "size": [0.1, 0.1], "speed": 1.0}]
    ems, _ = emitter.from_config(cfg)
    assert ems[0].scalar == 2.5 and ems[1].scalar is None
    sim = FakeSim(640, 2048)
    sim.t = 0.2
    emitter.apply(sim, ems, [])
    assert sim.scalars == [2.5, None]
    with pytest.raises(ValueError):
        emitter.Emitter([0, 0, 0], [0, 1, 0], [0.1, 0.1], 1.0, radius=0.025, scalar=float("nan"))


class PlySim:
    n_fluid = 3

    def derived(self, name):
        return np.full(3, F(4.0))

    def scalar(self):
        return F([0.25, 0.5, 0.75])


def test_the_ply_writer_with_the_scalar_column(tmp_path):
    pos = F([[0, 0, 0], [1, 2, 3], [4, 5, 6]])
    rgba = np.tile(F([0.0, 0.26, 0.68, 1.0]), (3, 1))
    assert run.parse_ply_fields("scalar, cover") == ["cover", "scalar"] and run.parse_ply_fields("scalar") == ["scalar"]
    plain, extra = tmp_path / "plain.ply", tmp_path / "extra.ply"
    run.write_ply_ascii(str(plain), pos, rgba, run.ply_extra(PlySim(), []))
    run.write_ply_ascii(str(extra), pos, rgba, run.ply_extra(PlySim(), ["cover", "scalar"]))
    a, b = plain.read_text().split("\n"), extra.read_text().split("\n")
    props = lambda lines: [l.split()[2] for l in lines if l.startswith("property float ")]      # noqa: E731
    assert props(a) == ["x", "y", "z", "red", "green", "blue", "alpha"] and props(b) == props(a) + ["cover", "scalar"]
    assert b[b.index("end_header") + 2] == a[a.index("end_header") + 2] + " 4.000000 0.500000"


def test_names_against_the_header():
    text = open(os.path.join(ROOT, "include", "sph_mi355x.h")).read()
    entries = ("sph_scalar_enable", "sph_scalar_disable", "sph_scalar_upload", "sph_scalar_download", "sph_scalar_set_inflow", "sph_scalar_rate")
    for name in entries:
        assert re.search(r"int %s\(SphHandle \*h" % name, text), name
        assert name in nat.EXPORTS and name in nat.OPTIONAL_EXPORTS and name not in nat.CORE_EXPORTS
    assert re.search(r"#define SPH_ABI_VERSION 5\b", text)
    for method in ("enable_scalar", "disable_scalar", "scalar", "set_scalar", "scalar_rate", "set_scalar_inflow"):
        assert callable(getattr(nat.Simulation, method))
    assert math.isclose(1.0 / LATTICE_SUM_H2, 0.0585, rel_tol=2e-3) and "0.0585 h^2 / D" in text
