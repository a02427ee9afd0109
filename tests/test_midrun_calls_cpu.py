"""CPU suite: the yardstick of tests/test_midrun_calls_gpu.py does not move, and its runs exercise what they are meant to (tests/midrun_calls.py).

  * the oracle has the property: with the oracle-side equivalents of the invisible calls before each of the last M steps it gives the statistics
    and fields of an undisturbed oracle, on every scene of the GPU file;
  * the history is real: the K history steps reach the density loop's later iterations (n_dens >= 3: the working-tiles-first order is set), end a
    divergence loop below its cap, iterate the pcisph / iisph pressure loops, activate pbf's constraint;
  * every S of a re-seat is usable: inside the box, nothing lost, no loop capped in the M steps that follow, and those M steps reach n_dens >= 3
    (lambda != 0) again."""
import numpy as np
import pytest

import harness as h
import midrun_calls as mc
from oracle import oracle as orc


def first_case(scene, solver):
    return next(c for c in mc.CASES.values() if (c.scene, c.solver) == (scene, solver))


@pytest.mark.parametrize("scene,solver", mc.ORACLE_SCENES)
def test_the_oracle_has_the_property(scene, solver):
    """... on the very run of the GPU file's invisible-call test (the case's K and M), so the conditions of that run are asserted here: the K history
    steps reach n_dens >= 3 and, on dfsph, end a divergence loop below its cap; pbf's lambda is non-zero in the history and in EVERY one of the M
    disturbed steps (the carry of pbf_lambda / delta_pos through a re-sort is checked on what is non-zero then); the body feels the fluid."""
    case = first_case(scene, solver)
    assert all((c.k, c.m) == (case.k, case.m) for c in mc.CASES.values() if (c.scene, c.solver) == (scene, solver))
    a, b = mc.oracle_of(case), mc.oracle_of(case)
    mc.begin(case, a); mc.begin(case, b)
    rng = np.random.default_rng(mc.SEED)
    print("seed", mc.SEED)
    n_dens, n_div, lam, force = [], [], [], 0.0
    for s in range(case.k + case.m):
        if s >= case.k:
            mc.oracle_disturb(a, case, rng)
        ra, rb = h.oracle_step(a, solver, bits_view=True), h.oracle_step(b, solver, bits_view=True)
        assert ra == rb, (scene, s, ra, rb)
        if ra is not None:
            n_dens.append(b.last_stats.n_dens); n_div.append(b.last_stats.n_div)
        if solver == "pbf":
            lam.append(int((b.get(orc.F_PBF_LAMBDA) != 0).sum()))
        if case.rigid:
            if case.k <= s < case.k + case.m - 1:        # (not behind the last step: a compute_rho there is the rho the run ends with)
                mc.oracle_disturb(a, case, rng)
            h.same_values_nan_signed(a.get(orc.F_RIGID_FORCE), b.get(orc.F_RIGID_FORCE), "step %d: force on the body" % (s + 1))
            force = max(force, float(np.abs(b.get(orc.F_RIGID_FORCE)).max()))
            a.rigid_step(); b.rigid_step()
            assert a.rigid_scalars() == b.rigid_scalars(), s
        h.same_values_nan_signed(a.get(orc.F_POS), b.get(orc.F_POS), "step %d: pos" % (s + 1))
    for f in mc.SOLVER_FIELDS[solver]:
        h.same_values_nan_signed(a.get(f), b.get(f), "field %d" % f)
    assert a.dt == b.dt
    print(scene, solver, "n_dens", n_dens, "n_div", n_div, "lambda != 0", lam, "force", force)
    if solver in ("dfsph", "pcisph", "iisph"):
        assert max(n_dens[:case.k]) >= 3, n_dens
    if solver == "dfsph":
        assert min(n_div[:case.k]) < 15, n_div
    if solver == "pbf":
        assert max(lam[:case.k]) > 0 and min(lam[case.k:]) > 0, lam
    if case.rigid:
        assert force > 0.0
    a.close(); b.close()


# (the exact cases of one scene are the same run on the oracle: what differs between them is the library's cell order and staging)
RESEATS = [(first_case(*ss).name, order) for ss in mc.ORACLE_SCENES for order in mc.reseat_orders(first_case(*ss))]


@pytest.mark.parametrize("name,order", RESEATS, ids=["%s-%s-%s" % ((n,) + o) for n, o in RESEATS])
def test_the_history_is_real_and_every_state_is_usable(name, order):
    case = mc.CASES[name]
    recs = mc.reseat_run(case, order)
    print(name, order, [(r["kind"], r.get("n_dens"), r.get("lambda"), r.get("lost"), r.get("force")) for r in recs])
    hist = recs[0]
    if case.solver == "dfsph":
        assert max(hist["n_dens"]) >= 3, hist["n_dens"]                           # dens_sparse was set
        assert min(hist["n_div"]) < 15, hist["n_div"]                             # a divergence loop ended below its cap: the undo path ran
    if case.solver in ("pcisph", "iisph"):
        assert max(hist["n_dens"]) >= 3, hist["n_dens"]
    if case.solver == "pbf":
        assert max(hist["lambda"]) > 0
    if case.rigid:
        assert hist["force"] > 0.0                                                  # the body feels the fluid within the history
    for rec in recs[1:]:
        assert rec["inside"], rec["kind"]
        assert rec["lost"] == 0 and rec.get("capped", 0) == 0, rec
        if case.solver == "dfsph":
            assert max(rec["n_dens"]) >= 3, rec
        if case.solver == "pbf":
            assert max(rec["lambda"]) > 0, rec


def test_every_case_has_its_conditions_checked():
    """every case of the GPU file runs a scene whose conditions are asserted above -- but the 30 k dam break, whose oracle takes 0.4 s a step: the
    GPU file asserts the history conditions of its two cases on the handle's own statistics, which its twin pins; no relaxed re-seat where the
    oracle carries more than delta_time over a `set`"""
    assert {(c.scene, c.solver) for c in mc.CASES.values() if c.scene != "breaking_dam_30k_dfsph"} == set(mc.ORACLE_SCENES)
    assert all(mc.CASES[n].solver != "iisph" for n in mc.RELAXED_RESEAT_CASES)
