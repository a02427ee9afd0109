"""GPU suite: a handle's history does not show in its bits (tests/midrun_calls.py; test_midrun_calls_cpu.py proves on the oracle alone that the
yardstick has the property and that the runs reach what they are meant to reach).

  1. calls that must be invisible: seeded random draws of reads, profiling, the stages of a step, same-value writes and refused calls between
     the steps of a handle with history, against a twin that only stepped and, under the exact arithmetic, the oracle in lock step;
  2. re-seat: a handle with history takes an unrelated state by `upload` and follows the oracle, twice; a relaxed handle equals a fresh relaxed
     handle given the same state and delta_time;
  3. a CHANGED solver attribute or delta_time reaches the captured wcsph step pairs (the same-value writes of 1. cannot tell).

Bit equality throughout: np.array_equal(..., equal_nan=True), the sign of zero through the uint32 view (harness.same_values_nan_signed)."""
import numpy as np
import pytest

import harness as h
import midrun_calls as mc
from cfd_taichi_amd import _native as nat
from oracle import oracle as orc

pytestmark = pytest.mark.gpu


def handle(case, monkeypatch):
    return h.make_handle(mc.config(case), monkeypatch, case.env, case.arith, rigid=mc.rigid_of(case))


def is_relaxed(sim):
    return sim.scalar(nat.S_ARITH_RELAXED) == 1.0


def same_handles(case, a, b, when):
    """every downloadable field of every species, the scalars a step moves, the body"""
    for f in mc.DOWNLOADABLE[case.solver]:
        h.same_values_nan_signed(a.download(f), b.download(f), "%s: field %d" % (when, f))
    for s in (nat.S_DELTA_TIME, nat.S_SIMULATE_CNT, nat.S_PS_DELTA_TIME):
        assert a.scalar(s) == b.scalar(s), (when, s)
    if case.rigid:
        for f in (nat.F_RIGID_POS, nat.F_RIGID_FORCE, nat.F_RIGID_VERT, nat.F_RIGID_VOL, nat.F_RIGID_MASS):
            h.same_values_nan_signed(a.download(f, nat.SPECIES_RIGID), b.download(f, nat.SPECIES_RIGID), "%s: rigid field %d" % (when, f))
        ra, rb = a.rigid_scalars(), b.rigid_scalars()
        for k in ra:
            h.same_values_nan_signed(np.float32(ra[k]), np.float32(rb[k]), "%s: body %s" % (when, k))


def history_is_real(case, n_dens, n_div):
    """The history conditions on the handle's own statistics (test_midrun_calls_cpu.py asserts them on the oracle, but not for the 30 k dam break
    and not for relaxed handles): the density loop went beyond its second iteration, so its working-tiles-first order was set, and a divergence
    loop ended below its cap of 15, so the undo path ran; pcisph / iisph iterated."""
    if case.solver in ("dfsph", "pcisph", "iisph"):
        assert max(n_dens) >= 3, n_dens
    if case.solver == "dfsph":
        assert min(n_div) < 15, n_div


# ---- 1 ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(mc.CASES))
def test_midrun_calls_are_invisible(name, monkeypatch):
    case = mc.CASES[name]
    seed = mc.SEED + list(mc.CASES).index(name)
    print("case %s, seed %d" % (name, seed))
    a, b = handle(case, monkeypatch), handle(case, monkeypatch)                  # the disturbed handle and its twin
    single = handle(case, monkeypatch) if case.chunks and case.oracle else None  # wcsph: one step per call, never a graph replay
    o = mc.oracle_of(case) if case.oracle else None
    mc.begin(case, o, [s for s in (a, b, single) if s is not None])
    d = mc.Disturber(a, case, nat, pytest.raises, seed)
    verlet = case.solver == "wcsph" and case.arith == "relaxed"
    done = [0]
    n_dens, n_div = [], []

    def step_all(n, between):
        when = "step %d" % (done[0] + n)
        sa, sb = a.step(n), b.step(n)
        if sa is not None:
            ga, gb = mc.stats_bits(sa, mc.STATS + ("capped",)), mc.stats_bits(sb, mc.STATS + ("capped",))
            assert ga == gb, (when, d.log[-8:], dict(zip(mc.STATS + ("capped",), zip(ga, gb))))
            n_dens.append(sa.n_dens); n_div.append(sa.n_div)
        if single is not None:
            single.step(1) if n == 1 else [single.step(1) for _ in range(n)]
        if o is not None:
            for _ in range(n):
                r = h.oracle_step(o, case.solver, bits_view=True)
            if r is not None:
                got = mc.stats_bits(sa, h.ORACLE_STATS) + (int(sa.lost),)
                assert got == r[0] and sa.capped == int(r[1]), (when, d.log[-8:], dict(zip(h.ORACLE_STATS + ("lost",), zip(got, r[0]))))
            else:
                h.same_values_nan_signed(a.download(nat.F_POS), o.get(orc.F_POS), "%s: pos against the oracle after %s" % (when, d.log[-8:]))
        if verlet:
            assert a.scalar(nat.S_VERLET_BUILDS) == b.scalar(nat.S_VERLET_BUILDS), (when, d.log[-8:])
        if case.rigid:
            if between:
                d.draw("between %s and its rigid_step" % when)
            fa = a.download(nat.F_RIGID_FORCE, nat.SPECIES_RIGID)
            h.same_values_nan_signed(fa, b.download(nat.F_RIGID_FORCE, nat.SPECIES_RIGID), "%s: force on the body against the twin, after %s" % (when, d.log[-8:]))
            if o is not None:
                h.same_values_nan_signed(fa, o.get(orc.F_RIGID_FORCE), "%s: force on the body against the oracle, after %s" % (when, d.log[-8:]))
                o.rigid_step()
            a.rigid_step(); b.rigid_step()
        done[0] += n

    for n in mc.step_plan(case, case.k):
        step_all(n, False)
    assert is_relaxed(a) == is_relaxed(b) == (case.arith == "relaxed")
    history_is_real(case, n_dens, n_div)
    plan = mc.step_plan(case, case.m)
    prof = mc.profile_plan(d.rng, len(plan))
    for i, n in enumerate(plan):
        d.draw("before step %d" % (done[0] + 1), prof.get(i), left=len(plan) - i)
        step_all(n, i < len(plan) - 1)          # (no draw behind the last step: a compute_density there is the rho the run ends with)
    d.finish()
    print("calls issued:", dict(d.issued))
    same_handles(case, a, b, "the end, against the twin")
    if o is not None:
        mc.same_as_oracle(case, a, o, "the end, against the oracle")
    if single is not None:
        mc.same_as_oracle(case, single, o, "stepped one call per step, against the oracle")
        assert single.scalar(nat.S_GRAPH_LAUNCHES) == 0 and b.scalar(nat.S_GRAPH_LAUNCHES) > 0 and a.scalar(nat.S_GRAPH_LAUNCHES) > 0
    if verlet:
        assert a.scalar(nat.S_VERLET_BUILDS) < done[0], "the lists were rebuilt every step: no reuse to disturb"
    for s in (a, b, single, o):
        if s is not None:
            s.close()


# ---- 2 ---------------------------------------------------------------------------------------------------------------------------------------
RESEATS = [(n, order) for n in mc.ORACLE_CASES for order in mc.reseat_orders(mc.CASES[n])]


@pytest.mark.parametrize("name,order", RESEATS, ids=["%s-%s-%s" % ((n,) + o) for n, o in RESEATS])
def test_reseat_follows_the_oracle(name, order, monkeypatch):
    case = mc.CASES[name]
    sim = handle(case, monkeypatch)
    recs = mc.reseat_run(case, order, sim)
    assert not is_relaxed(sim)
    print(name, order, [(r["kind"], r.get("n_dens"), r.get("lost")) for r in recs])
    sim.close()


def handle_state(sim, case):
    return (sim.download(nat.F_POS), sim.download(nat.F_VEL), sim.download(nat.F_WARM_K) if case.solver == "dfsph" else None)


def give_handle_state(sim, state):
    sim.upload(nat.F_POS, state[0]); sim.upload(nat.F_VEL, state[1])
    if state[2] is not None:
        sim.upload(nat.F_WARM_K, state[2])


RELAXED_RESEATS = [(n, order) for n in mc.RELAXED_RESEAT_CASES for order in mc.RESEAT_ORDERS[:2 if "30k" in n else 3]]


@pytest.mark.parametrize("name,order", RELAXED_RESEATS, ids=["%s-%s-%s" % ((n,) + o) for n, o in RELAXED_RESEATS])
def test_relaxed_reseat_equals_a_fresh_handle(name, order, monkeypatch):
    """Relaxed handles have no oracle and no twin with the same history; where the oracle carries nothing but delta_time over a `set`
    (midrun_calls' docstring) the re-seated handle equals a fresh relaxed handle given S and that delta_time -- Verlet handles included: both build
    their lists at S, and from then on rebuild at the same steps."""
    case = mc.CASES[name]
    a = handle(case, monkeypatch)
    mc.begin(case, None, [a])
    verlet = case.solver == "wcsph"
    k, m = mc.reseat_steps(case)
    half, n_dens, n_div = None, [], []
    for s in range(k):
        if s == k // 2:
            half = handle_state(a, case)
        st = a.step(1)
        if st is not None:
            n_dens.append(st.n_dens); n_div.append(st.n_div)
    assert is_relaxed(a)
    history_is_real(case, n_dens, n_div)
    for n, kind in enumerate(order):
        when = "re-seat %d (%s)" % (n + 1, kind)
        state = mc.reseat_state(case, kind, handle_state(a, case), half, 1 + n)
        assert mc.inside_box(case, state[0]), when
        a.compute_density()                       # both validity flags say "valid" when the new state arrives
        builds = a.scalar(nat.S_VERLET_BUILDS)
        give_handle_state(a, state)
        f = handle(case, monkeypatch)
        give_handle_state(f, state)
        f.set_dt(a.scalar(nat.S_DELTA_TIME))
        after = []
        for n_steps in mc.step_plan(case, m):
            sa, sf = a.step(n_steps), f.step(n_steps)
            if sa is not None:
                after.append(sa.n_dens)
                ga, gf = mc.stats_bits(sa, mc.STATS + ("capped",)), mc.stats_bits(sf, mc.STATS + ("capped",))
                assert ga == gf, (when, dict(zip(mc.STATS + ("capped",), zip(ga, gf))))
                assert sa.lost == 0 and sa.capped == 0, when
            if verlet:
                assert a.scalar(nat.S_VERLET_BUILDS) - builds == f.scalar(nat.S_VERLET_BUILDS), when
        for fld in mc.DOWNLOADABLE[case.solver]:
            h.same_values_nan_signed(a.download(fld), f.download(fld), "%s: field %d against the fresh handle" % (when, fld))
        assert a.scalar(nat.S_DELTA_TIME) == f.scalar(nat.S_DELTA_TIME)
        if case.solver == "dfsph":
            assert max(after) >= 3, (when, after)          # the density loop's tile order, taken from the state before S, was used and set again
        if verlet:
            assert 1 <= f.scalar(nat.S_VERLET_BUILDS) <= m         # (a foreign state, 0.5 m/s and compressed, outruns the skin every step)
        f.close()
    a.close()


# ---- 3 ---------------------------------------------------------------------------------------------------------------------------------------
def test_changed_attributes_reach_the_captured_wcsph_steps(monkeypatch):
    """wcsph step pairs are captured with the solver's constants and delta_time as launch arguments: writing another value between two calls must
    show in the very next replay, as it does on the oracle."""
    case = mc.CASES["wcsph_small"]
    sim, o = handle(case, monkeypatch), mc.oracle_of(case)
    launches = 0
    for write in (None, lambda: (sim.set_param("viscosity_alpha", 0.03), o.set_param(mc.PARAMS["viscosity_alpha"], 0.03)),
                  lambda: (sim.set_param("tension_k", 0.35), o.set_param(mc.PARAMS["tension_k"], 0.35)),
                  lambda: (sim.set_dt(2e-4), o.set_dt(2e-4))):
        if write:
            write()
        sim.step_wcsph(6); o.step_wcsph(6)
        assert sim.scalar(nat.S_GRAPH_LAUNCHES) == launches + 3          # replays, not eager steps
        launches += 3
        mc.same_as_oracle(case, sim, o, "after %d graph replays" % launches)
    sim.close(); o.close()
