"""CPU suite: the inputs of tests/test_pbf_edges_gpu.py (tests/pbf_edge_states.py) are fair, shown on the reference's two precisions alone.

Conditions, not measurements (the figures are printed, and those of the commit that added this file stand next to each condition):
  ragged      N is 1, 6, 73, 82; with SQUEEZE = 0.8 lambda != 0 on at least 5 particles in some step for both scenes' N = 73 (55 and 36 in step 1;
              at 0.9 the clamp scene's 73 reach exactly 5 and its 82 none); the one step the relaxed kernels are held to has equal `lambda != 0` sets
              and f32 errors below CAP
  coincident  pair (a) stays bit-coincident (position and velocity) in both oracles through 3 steps and both of its particles have lambda != 0 in the
              f64 oracle's step 1; pair (b) has separated after one step; over the 3 steps the `lambda != 0` and clamped sets of the two oracles are
              equal and the f32 oracle's max-norm error is below CAP = 2e-5 in every field (worst: vel 1.7e-5 on the clamp scene, step 1)
  spray       the same set and cap conditions over 3 steps (delta_pos 8.1e-6 in step 3; 2.1e-5 in step 4 and 6.6e-5 in step 5: the exact check runs
              6 steps, the relaxed one cannot fairly); the 40 particles of the clump have lambda != 0
  outside     over 5 steps: in some step at least 30 of the 48 moved particles have rho > 1 (they see fluid or wall), in some step at least 5 have
              lambda != 0, in some step at least one is lost, the two oracles count the same lost particles, and every value is finite
              (wall scene: 39-40 / 12 / 9-24; clamp scene, where the planes bring every particle back after step 1: 43-45 / 7-9 / 9)
  wall        the moved fluid particle sits on a wall particle of the f32 oracle bit for bit, and the two oracles disagree about it (why that
              input gets no relaxed check): their lambda for that particle differ by more than max |lambda| of the f64 oracle"""
import numpy as np
import pytest

import pbf_edge_states as pe
import pbf_states as pb
from oracle import oracle as orc

CAP = 2e-5          # tests/test_pbf_relaxed_cpu.py


def fair_sets_and_cap(inp, steps, tag):
    r32, r64 = pe.references(inp, steps)
    for s in range(steps):
        (l32, c32), (l64, c64) = pb.discrete_sets(inp.cfg, r32[s]), pb.discrete_sets(inp.cfg, r64[s])
        worst = {name: float(pb.errors(r32[s][name], r64[s][name]).max()) for name, _ in pb.FIELDS}
        print("%s step %d: lambda != 0 on %d of %d, %d clamped particles, f32 max-norm errors %s" % (
            tag, s + 1, int(l64.sum()), len(l64), int(c64.any(1).sum()), " ".join("%s %.1e" % kv for kv in worst.items())))
        assert np.array_equal(l32, l64), (tag, s + 1, int((l32 != l64).sum()))
        assert np.array_equal(c32, c64), (tag, s + 1, int((c32 != c64).sum()))
        for name, e in worst.items():
            assert e < CAP, (tag, s + 1, name, e)
    return r32, r64


@pytest.mark.parametrize("scene", pe.SCENES)
def test_the_ragged_blocks_are_fair(scene):
    assert pe.SQUEEZE == 0.8
    for water, n in pe.RAGGED.items():
        inp = pe.ragged(scene, water)
        assert len(inp.pos) == n, (scene, water, len(inp.pos))
        r32, r64 = pe.references(inp, 25)
        active = [int((r["pbf_lambda"] != 0).sum()) for r in r64]
        print("%s: lambda != 0 per step %s" % (inp.label, active))
        assert all(np.isfinite(r[name]).all() for r in r32 + r64 for name, _ in pb.FIELDS)
        if n == 73:
            assert max(active) >= 5 and active[0] >= 5, (inp.label, active)
            fair_sets_and_cap(inp, 1, inp.label)          # the relaxed check's one step


@pytest.mark.parametrize("scene", pe.SCENES)
@pytest.mark.parametrize("seed", pe.SEEDS)
def test_the_coincident_states_are_fair(scene, seed):
    inp = pe.coincident(scene, seed)
    (i, j), (bi, bj), (ci, cj), d = inp.marks["a"], inp.marks["b"], inp.marks["c"], inp.marks["d"]
    assert len({i, j, bi, bj, ci, cj, d}) == 7
    assert np.array_equal(inp.pos[i], inp.pos[j]) and np.array_equal(inp.vel[i], inp.vel[j])
    assert np.array_equal(inp.pos[bi], inp.pos[bj]) and not np.array_equal(inp.vel[bi], inp.vel[bj])
    gap = inp.pos[cj].astype(np.float64) - inp.pos[ci]
    assert (gap > 0).all() and (gap < 2e-7).all(), gap
    assert np.array_equal(inp.pos[d], np.float32([0.4, 0.5, 0.6]))
    r32, r64 = fair_sets_and_cap(inp, 3, inp.label)
    for s in range(3):
        for who, r in (("f32", r32), ("f64", r64)):
            assert np.array_equal(r[s]["pos"][i], r[s]["pos"][j]) and np.array_equal(r[s]["vel"][i], r[s]["vel"][j]), (who, s + 1)
    lam = r64[0]["pbf_lambda"]
    print("%s: pair (a) = %s, f64 lambda %s of max |lambda| %.3e" % (inp.label, (i, j), lam[[i, j]], float(np.abs(lam).max())))
    assert lam[i] != 0 and lam[j] != 0
    for who, r in (("f32", r32), ("f64", r64)):
        assert not np.array_equal(r[0]["pos"][bi], r[0]["pos"][bj]), "pair (b) did not separate in the %s oracle" % who


@pytest.mark.parametrize("scene", pe.SCENES)
def test_spray_and_clump_is_fair(scene):
    inp = pe.spray_and_clump(scene)
    assert len(inp.marks["clump"]) == 40
    cell = np.floor(inp.pos[inp.marks["clump"]].astype(np.float64) / 0.1).astype(int)
    assert (cell == cell[0]).all(), "the clump is not inside one cell"
    r32, r64 = fair_sets_and_cap(inp, 3, inp.label)
    assert (r64[0]["pbf_lambda"][inp.marks["clump"]] != 0).all()


@pytest.mark.parametrize("scene", pe.SCENES)
@pytest.mark.parametrize("seed", pe.SEEDS)
def test_the_outside_states_are_fair(scene, seed):
    inp = pe.outside(scene, seed)
    m = inp.marks["moved"]
    box = np.asarray(inp.cfg["scene"]["box_max"], dtype=np.float32)
    assert len(m) == pe.N_OUTSIDE == 48 and ((inp.pos[m] < 0) | (inp.pos[m] > box)).any(1).all()
    rest = np.setdiff1d(np.arange(len(inp.pos)), m)
    assert abs(float(inp.pos[rest].min()) - 0.02) < 0.01 and ((inp.pos[rest] > 0) & (inp.pos[rest] < box)).all()
    r32, r64 = pe.references(inp, 5)
    sees, active, lost = [], [], []
    for s in range(5):
        for r in (r32[s], r64[s]):
            assert all(np.isfinite(r[name]).all() for name, _ in pb.FIELDS), (inp.label, s + 1)
        assert r32[s]["lost"] == r64[s]["lost"], (inp.label, s + 1, r32[s]["lost"], r64[s]["lost"])
        sees.append(int((r64[s]["rho"][m] > 1).sum())); active.append(int((r64[s]["pbf_lambda"][m] != 0).sum())); lost.append(r64[s]["lost"])
    print("%s: of the 48 moved particles per step: rho > 1 %s, lambda != 0 %s; lost %s" % (inp.label, sees, active, lost))
    assert max(sees) >= 30 and max(active) >= 5 and max(lost) >= 1, (sees, active, lost)


@pytest.mark.parametrize("seed", pe.SEEDS)
def test_the_particle_on_a_wall_particle(seed):
    inp = pe.on_a_wall_particle(seed)
    i, w = inp.marks["w"]
    assert np.array_equal(inp.pos[i], inp.wall[w])
    o = orc.Oracle(inp.cfg, num_threads=1)
    try:
        assert np.array_equal(o.get(orc.F_WALL_POS), inp.wall)
    finally:
        o.close()
    r32, r64 = pe.references(inp, 5)
    l32, l64 = float(r32[0]["pbf_lambda"][i]), float(r64[0]["pbf_lambda"][i])
    scale = float(np.abs(r64[0]["pbf_lambda"]).max())
    print("%s: lambda of the particle f32 %.4e, f64 %.4e, max |lambda| %.4e: they differ by %.2f of it" % (inp.label, l32, l64, scale, abs(l32 - l64) / scale))
    assert l32 != 0 and l64 != 0 and abs(l32 - l64) > scale
    assert all(np.isfinite(r[name]).all() for r in r32 + r64 for name, _ in pb.FIELDS)
