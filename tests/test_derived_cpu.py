"""The yardsticks of the derived per-particle fields (tests/derived_ref.py) shown fair and sharp WITHOUT the library, the PLY writer's extra columns and
the binding's names.  A few seconds in all."""
import os
import re

import numpy as np
import pytest

import derived_ref as dr
import particle_flow as pf
import second_restatement as sr
from cfd_taichi_amd import _native as nat
from cfd_taichi_amd import run

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = 0.05                                       # particle spacing of the tiny scenes; h = 2 D


def scene_state(walls, seed, body=False):
    """the tiny wall / clamp scene at 640 particles, displaced, with velocities A x + b + noise; rho as the reference's density sum of those positions
    (second_restatement.Solver.compute_all_rho).  body: a block of 5 x 5 x 5 samples sunk into the top of the column"""
    cfg = pf.config("dfsph", walls, 640)
    s = sr.Solver(cfg)
    s.pos = dr.displaced(s.pos, D, seed)
    s.prologue()
    s.compute_all_rho()
    wall = (s.sc.wall_pos, s.sc.wall_vol) if walls == "wall" else (None, None)
    bp = bv = None
    if body:
        top = s.pos[:, 1].max()
        mid = F(0.5) * (s.pos.min(axis=0) + s.pos.max(axis=0))
        g = np.arange(5, dtype=F) * F(D)
        bp = (np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3) + F([mid[0] - 2 * D, top - 2 * D, mid[2] - 2 * D])).astype(F) + F(0.013)
        bv = np.full(len(bp), F(0.8 * D ** 3), dtype=F)
    st = dr.State(s.pos, dr.velocities(s.pos, seed), s.rho, s.m, s.h, wall[0], wall[1], bp, bv)
    return st, dr.Cells(cfg, s.h)


@pytest.fixture(scope="module")
def states():
    """name -> (state, canonical lists, yardstick B's values and bounds): computed once, never changed"""
    out = {}
    for name, walls, seed, body in (("wall", "wall", 11, False), ("clamp", "clamp", 12, False), ("body", "clamp", 13, True)):
        st, cells = scene_state(walls, seed, body)
        out[name] = (st, dr.canonical_lists(cells, st)) + dr.yardstick_b(st)
    return out


def lattice_state(nx=11):
    """an undisturbed cubic lattice of nx^3 particles, no walls, v = A x + b exactly; rho: the plain density sum (uniform around the centre)"""
    g = np.arange(nx, dtype=F) * F(D)
    pos = (np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3) + F(0.3)).astype(F)
    h, m = F(2 * D), F(1000 * D ** 3)
    ok = dr._within(pos, pos, h, True)
    d = pos[:, None, :] - pos[None, :, :]
    r = np.sqrt((d * d).sum(axis=2)).astype(F)
    rho = (m * np.where(ok, sr.cubic_kernel(r, h), F(0))).sum(axis=1).astype(F)
    return dr.State(pos, dr.velocities(pos, 0, noise=0.0), rho, m, h), nx


def test_sign_and_index_convention_on_a_lattice():
    st, nx = lattice_state()
    val, bnd = dr.yardstick_b(st)
    c = nx // 2
    centre = (c * nx + c) * nx + c
    G = val[centre, 0:9].reshape(3, 3)
    kappa = G[0, 0] / dr.A_MATRIX[0, 0]
    print("lattice centre: velgrad / A = %.4f (the gradient carries the reference's factor 6)" % kappa)
    assert kappa > 0
    assert np.array_equal(np.sign(G), np.sign(dr.A_MATRIX))
    assert np.allclose(G, kappa * dr.A_MATRIX, rtol=1e-5, atol=0)                 # row a, column b: d v_a / d x_b, not its transpose
    assert not np.allclose(G, kappa * dr.A_MATRIX.T, rtol=1e-2, atol=0)
    A = dr.A_MATRIX
    curl = np.array([A[2, 1] - A[1, 2], A[0, 2] - A[2, 0], A[1, 0] - A[0, 1]])
    assert np.array_equal(np.sign(val[centre, 9:12]), np.sign(curl))
    assert np.allclose(val[centre, 9:12], kappa * curl, rtol=1e-5)
    assert np.isclose(val[centre, 12], kappa * np.trace(A), rtol=1e-5)
    # inside: the sums of vol grad W cancel by symmetry, what is left is rounding; cover is that of a full neighbourhood
    assert (np.abs(val[centre, 13:16]) <= bnd[centre, 13:16]).all(), (val[centre, 13:16], bnd[centre, 13:16])
    top = (c * nx + (nx - 1)) * nx + c                                           # index (c, nx - 1, c): the middle of the top layer
    normal = val[top, 13:16]
    assert np.argmax(np.abs(normal)) == 1 and normal[1] > 0.1, normal
    print("cover: centre %.4f, top layer %.4f; top-layer normal %s" % (val[centre, 16], val[top, 16], normal))
    assert abs(val[centre, 16] - 1.0) < 1e-3 and val[top, 16] < val[centre, 16] - 0.03      # (rho_j falls with it: the self-normalised sum falls slowly)


@pytest.mark.parametrize("name", ["wall", "clamp", "body"])
def test_the_bound_is_fair(states, name):
    st, lists, val, bnd = states[name]
    for what, ls in (("canonical", lists), ("shuffle 1", dr.shuffled(lists, 1)), ("shuffle 2", dr.shuffled(lists, 2))):
        ratio = dr.worst_ratio(dr.yardstick_a(st, ls), val, bnd)
        print("%s, %s order: worst error / bound %.3f" % (name, what, ratio))
        assert ratio <= 1.0
    skin = dr.skin_lists(st, 1.05 * float(st.h))
    assert (skin.fc > lists.fc).any()
    ratio = dr.worst_ratio(dr.yardstick_a(st, skin), val, bnd)
    print("%s, a list with 5 %% skin: worst error / bound %.3f" % (name, ratio))
    assert ratio <= 1.0


@pytest.mark.parametrize("mutant", dr.MUTANTS)
def test_the_bound_is_sharp(states, mutant):
    for name, (st, lists, val, bnd) in states.items():
        if mutant == "no_walls" and not len(st.wall_pos):
            continue
        ls = dr.skin_lists(st, 1.05 * float(st.h)) if mutant == "no_gate" else lists
        ratio = dr.worst_ratio(dr.yardstick_a(st, ls, mutant=mutant), val, bnd)
        print("%s on %s: worst error / bound %.3g" % (mutant, name, ratio))
        assert ratio > 1.0, "%s stays inside the bound on %s" % (mutant, name)


def test_one_particle_and_two_at_exactly_h():
    cfg = pf.config("dfsph", "clamp", 640)
    h = F(2 * D)
    one = dr.State(F([[0.2, 0.2, 0.2]]), F([[1, 2, 3]]), F([0.001]), 1000 * D ** 3, h)
    a = dr.yardstick_a(one, dr.canonical_lists(dr.Cells(cfg, h), one))
    val, bnd = dr.yardstick_b(one)
    assert (a == 0).all() and (val == 0).all() and (bnd == 0).all() and dr.worst_ratio(a, val, bnd) == 0.0
    two = dr.State(F([[0.1, 0.1, 0.1], [0.2, 0.1, 0.1]]), F([[1, 0, 0], [0, 1, 0]]), F([0, 0]), 1000 * D ** 3, h)
    assert two.pos[1, 0] - two.pos[0, 0] == h
    lists = dr.canonical_lists(dr.Cells(cfg, h), two)
    assert list(lists.fc) == [1, 1]                                              # r = h is a neighbour (the reference skips r > h only)
    a = dr.yardstick_a(two, lists)
    val, bnd = dr.yardstick_b(two)
    assert np.isfinite(a).all() and (a == 0).all() and np.isfinite(val).all() and (val == 0).all()


class FakeSim:
    n_fluid = 3

    def derived(self, name):
        base = {"vorticity": 1.0, "divergence": 2.0, "normal": 3.0, "cover": 4.0}[name]
        width = 3 if name in ("vorticity", "normal") else 1
        return (base + 0.1 * np.arange(3 * width, dtype=F).reshape((3, 3) if width == 3 else (3,))).astype(F)


def test_the_ply_writer_with_extra_columns(tmp_path):
    pos = F([[0, 0, 0], [1, 2, 3], [4, 5, 6]])
    rgba = np.tile(F([0.0, 0.26, 0.68, 1.0]), (3, 1))
    plain, extra = tmp_path / "plain.ply", tmp_path / "extra.ply"
    run.write_ply_ascii(str(plain), pos, rgba)
    assert run.parse_ply_fields("cover, vorticity") == ["vorticity", "cover"] and run.parse_ply_fields(None) == []
    with pytest.raises(SystemExit):
        run.parse_ply_fields("vorticity,enstrophy")
    run.write_ply_ascii(str(extra), pos, rgba, run.ply_extra(FakeSim(), ["vorticity", "cover"]))
    a, b = plain.read_text().split("\n"), extra.read_text().split("\n")
    props = lambda lines: [l.split()[2] for l in lines if l.startswith("property float ")]      # noqa: E731
    assert props(a) == ["x", "y", "z", "red", "green", "blue", "alpha"]
    assert props(b) == props(a) + ["vort_x", "vort_y", "vort_z", "cover"]
    body_a, body_b = a[a.index("end_header") + 1:], b[b.index("end_header") + 1:]
    assert body_a[1] == "1.000000 2.000000 3.000000 0.000000 0.260000 0.680000 1.000000"
    assert body_b[1] == body_a[1] + " 1.300000 1.400000 1.500000 4.100000"
    assert [l[:len(m)] for l, m in zip(body_b, body_a)] == body_a
    run.write_ply_ascii(str(extra), pos, rgba, run.ply_extra(FakeSim(), run.parse_ply_fields("vorticity,divergence,normal,cover")))
    assert props(extra.read_text().split("\n"))[7:] == ["vort_x", "vort_y", "vort_z", "div", "normal_x", "normal_y", "normal_z", "cover"]


def test_names_against_the_header():
    text = open(os.path.join(ROOT, "include", "sph_mi355x.h")).read()
    ids = {name.lower(): int(v) for name, v in re.findall(r"#define SPH_D_(\w+) (\d+)", text)}
    assert ids == nat.DERIVED and sorted(ids.values()) == [0, 1, 2, 3, 4]
    assert (nat.D_VELGRAD, nat.D_VORTICITY, nat.D_DIVERGENCE, nat.D_NORMAL, nat.D_COVER) == tuple(ids[k] for k in ("velgrad", "vorticity", "divergence", "normal", "cover"))
    assert {k: int(np.prod(s, dtype=int)) for k, s in nat.DERIVED_SHAPE.items()} == {ids[name]: width for name, _, width in dr.QUANTITIES}
    assert re.search(r"int sph_derived\(SphHandle \*h, int which, float \*host, size_t n_floats\);", text)
    assert "sph_derived" in nat.EXPORTS and "sph_derived" in nat.OPTIONAL_EXPORTS and "sph_derived" not in nat.CORE_EXPORTS
    assert [c for _, cols in run.PLY_FIELDS for c in cols] == ["vort_x", "vort_y", "vort_z", "div", "normal_x", "normal_y", "normal_z", "cover"]
