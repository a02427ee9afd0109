"""GPU suite: the relaxed WCSPH step on Verlet lists (k_wcsph_density_rx, k_wcsph_force_rx, rx_wg_clamped in csrc/sph_relaxed_kernels.h) against
the f64 oracle, step by step.

tests/test_relaxed_gpu.py holds this path to 1e-5 max norm (or 3 x a legal schedule) in pos and vel after hundreds of steps.  The two kernels have
the most code of their own of any relaxed path -- wall sums regrouped into a cached G, m and kw folded out of the sums, p / rho^2 carried in V.w,
lists that hold pairs beyond h and are reused across steps -- and a 1e-4 error in the wall term, a dropped wall volume or a skin pair that
contributes a little all fit inside that envelope.  Here the participants of tests/test_relaxed_pressure_sweeps_gpu.py -- relaxed handle, exact
handle, f32 oracle, f64 oracle -- run the states of tests/pressure_states.py, handles in the linear and in the Morton cell order (the Verlet kernels
have one instantiation; the cell order is what varies the list build):
  1. SPH_S_ARITH_RELAXED is 1 on the relaxed handle and 0 on the exact one, and some field of the two differs in at least one bit;
  3. the exact handle equals the f32 oracle bit for bit on rho, pressure, acc, vel, pos at every step;
  4. on the clamp scene the relaxed handle's coordinates on a clamp plane are the f64 oracle's;
  5. per field and population, q50, q99 and max of the per-particle error against the f64 oracle <= 4 x the f32 oracle's own + 2 x 2^-24;
  6. every field finite.
(2: wcsph has no loop.  The neighbour counts of the uploaded state are equal on the exact handle and both oracles; a Verlet handle counts its LIST,
which holds the pairs within h + skin: never fewer than the oracle's, more for some particle -- the lists under test do hold pairs beyond h -- and
the oracle's exactly at SPH_VERLET_SKIN=0.)

  one step     every wcsph case, one step from the uploaded state;
  list reuse   pressure_states.REUSE_CASE: 8 free-running steps at |v| <= 2 m/s per axis, at the default skin and at SPH_VERLET_SKIN=0.1.
               SPH_S_VERLET_BUILDS after each step is 1 1 2 3 4 5 6 7 and 1 1 2 2 3 3 4 4 (predicted on the CPU from the oracles' positions,
               tests/test_pressure_states_cpu.py): at the default skin step 2 runs on the lists of step 1 and every later step follows a
               rebuild; at 0.1 h steps 2, 4, 6, 8 run on lists built a step earlier, steps 3, 5, 7 follow a rebuild.  The bar holds at every step;
  skin         the same 8 steps on two relaxed handles, SPH_VERLET_SKIN=0 (8 builds, no pair beyond h ever listed, neighbour counts the oracle's)
               and the default skin: both within the bar at every step.  After step 1 the particles whose default-skin list holds a pair beyond
               h are a population of their own for every field (at these densities all but a handful: 639 of 640; the handful, where there is
               one, is the other).  Their rho is NOT compared bit for bit between the two handles: the default-skin handle bins into cells of edge
               h + skin, so the same neighbours arrive in another order and the f32 sums differ in their last bits (the number of particles that
               do differ is printed); each handle is compared against the f64 oracle per particle instead.  What holds a contributing skin
               pair to account is the bar itself: one such pair moves rho by 1e-5 ... 8e-5 of its value, the bar on rho is 1.5e-6."""
import numpy as np
import pytest

import pressure_states as ps
from cfd_taichi_amd import _native as nat

pytestmark = pytest.mark.gpu

ORDERS = {"linear": {}, "morton": {"SPH_CELL_ORDER": "morton"}}
CASES = [(order,) + case for case in ps.CASES["wcsph"] for order in ORDERS]


def builds(sim):
    return int(sim.scalar(nat.S_VERLET_BUILDS))


def skin_pairs(label, a, r64):
    """a Verlet handle's count against the oracle's: bool mask of the particles whose list holds a pair beyond h"""
    extra = a[0].nbr - r64[0].nbr
    assert (extra >= 0).all(), (label, int((extra < 0).sum()))
    return extra > 0


@pytest.mark.parametrize("order,scene,seed,compression", CASES, ids=["%s-%s-%d-%g" % c for c in CASES])
def test_one_relaxed_wcsph_step_against_the_f64_oracle(order, scene, seed, compression, monkeypatch):
    label = "%s %s seed %d %g:" % (order, scene, seed, compression)
    rx, ex = ps.handles(nat, ps.config(scene), ORDERS[order], monkeypatch)
    try:
        a, b = ps.run_handle(rx, scene, seed, compression, 1, probe=builds), ps.run_handle(ex, scene, seed, compression, 1)
        assert rx.scalar(nat.S_ARITH_RELAXED) == 1.0 and ex.scalar(nat.S_ARITH_RELAXED) == 0.0
    finally:
        rx.close(); ex.close()
    assert a[0].probe == 1, a[0].probe
    assert any(not np.array_equal(a[0][name], b[0][name]) for name, _ in ps.FIELDS["wcsph"]), "the relaxed handle gave the exact handle's bits"
    r32, r64 = ps.references(scene, seed, compression)
    skin = skin_pairs(label, a, r64)
    print("%s %d of %d particles list a pair beyond h" % (label, int(skin.sum()), len(skin)))
    assert skin.any(), label
    pool = ps.pool(scene)
    ps.check_steps(label, scene, seed, compression, a, b, r32[:1], r64[:1], pool, nbr_of_relaxed=False)
    failures = pool.report(label)
    assert not failures, "\n".join(failures)


REUSE = [(order, skin) for order in ORDERS for skin in ps.REUSE_BUILDS]


@pytest.mark.parametrize("order,skin", REUSE, ids=["%s-skin-%s" % (o, s or "default") for o, s in REUSE])
def test_reused_lists_hold_the_bar_at_every_step(order, skin, monkeypatch):
    scene, seed, compression = ps.REUSE_CASE
    k, amp = ps.REUSE_STEPS, ps.REUSE_VEL_AMP
    label = "%s skin %s list reuse %s seed %d %g:" % (order, skin or "default", scene, seed, compression)
    rx, ex = ps.handles(nat, ps.config(scene), dict(ORDERS[order], **({"SPH_VERLET_SKIN": skin} if skin else {})), monkeypatch)
    try:
        a, b = ps.run_handle(rx, scene, seed, compression, k, amp, probe=builds), ps.run_handle(ex, scene, seed, compression, k, amp)
        assert rx.scalar(nat.S_ARITH_RELAXED) == 1.0 and ex.scalar(nat.S_ARITH_RELAXED) == 0.0
    finally:
        rx.close(); ex.close()
    got = [r.probe for r in a]
    print("%s list builds after each step %s" % (label, got))
    assert got == ps.REUSE_BUILDS[skin], (got, ps.REUSE_BUILDS[skin])
    assert any(x == y for x, y in zip(got, got[1:])) and any(y > x >= 1 for x, y in zip(got, got[1:]))
    r32, r64 = ps.references(scene, seed, compression, k, amp)
    assert skin_pairs(label, a, r64).any()
    pool = ps.pool(scene)
    ps.check_steps(label, scene, seed, compression, a, b, r32, r64, pool, vel_amp=amp, nbr_of_relaxed=False)
    failures = pool.report(label)
    assert not failures, "\n".join(failures)


def test_a_skin_pair_contributes_nothing(monkeypatch):
    scene, seed, compression = ps.REUSE_CASE
    k, amp = ps.REUSE_STEPS, ps.REUSE_VEL_AMP
    cfg = ps.config(scene)
    r32, r64 = ps.references(scene, seed, compression, k, amp)
    runs = {}
    for name, knobs in (("skin 0", {"SPH_VERLET_SKIN": "0"}), ("default skin", {})):
        rx, _ = ps.handles(nat, cfg, knobs, monkeypatch, exact=False)
        try:
            runs[name] = ps.run_handle(rx, scene, seed, compression, k, amp, probe=builds)
            assert rx.scalar(nat.S_ARITH_RELAXED) == 1.0
        finally:
            rx.close()
    assert [r.probe for r in runs["skin 0"]] == list(range(1, k + 1)), [r.probe for r in runs["skin 0"]]
    assert [r.probe for r in runs["default skin"]] == ps.REUSE_BUILDS[None]
    assert np.array_equal(runs["skin 0"][0].nbr, r64[0].nbr), "at a zero skin the lists are the oracle's"
    skin = skin_pairs("default skin", runs["default skin"], r64)
    a0, d0 = runs["skin 0"][0], runs["default skin"][0]
    print("after step 1: %d of %d particles list a pair beyond h; rho differs between the two handles on %d of them and on %d of the others" % (
        int(skin.sum()), len(skin), int((a0["rho"] != d0["rho"])[skin].sum()), int((a0["rho"] != d0["rho"])[~skin].sum())))
    assert skin.sum() >= ps.MIN_SPLIT, int(skin.sum())          # (all but a handful of particles list such a pair)
    failures = []
    for name, run in runs.items():
        label = "%s %s seed %d %g:" % (name, scene, seed, compression)
        pool = ps.pool(scene)
        ps.check_steps(label, scene, seed, compression, run, None, r32, r64, pool, vel_amp=amp, nbr_of_relaxed=False)
        for field, _ in ps.FIELDS["wcsph"]:          # step 1 by `has a pair beyond h in the default-skin list`
            ec, er = ps.errors(run[0][field], r64[0][field]), ps.errors(r32[0][field], r64[0][field])
            pool.add_raw((field, "skinpair/step1"), ec[skin], er[skin])
            if (~skin).any():
                pool.add_raw((field, "noskinpair/step1"), ec[~skin], er[~skin])
        failures += pool.report(label)
    assert not failures, "\n".join(failures)
