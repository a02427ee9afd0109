"""Loads on walls and geometry on the device (sph_wall_load_*, Simulation.measure_loads / wall_load / wall_impulse / wall_forces; DESIGN.md
section 6m).

The yardstick is tests/wall_load_ref.py (shown fair, and pinned to the physics by action and reaction, in test_wall_load_cpu.py): the second
restatement with every wall sample's sums taken in the sample's own walk order.  Per-sample forces are compared with it bit for bit
(harness.same_bits) after every step; the group sums with the exact rational sums of those forces within the bound of the device's f64
reduction, (n + 8) 2^-53 sum |t_i| (wall_load_ref.load_bound); handles are compared among themselves bit for bit.  Every test here fails without
the entry points.

The state: the pressed state of wall_load_ref (480 particles, 2 510 wall samples: the box and CARVE_PLATE, group 1)."""
import copy
import os

import numpy as np
import pytest

import geometry_ref as gr
import harness as h
import restatement_compare as rc
import wall_load_ref as wl
from cfd_taichi_amd import _native as nat
from cfd_taichi_amd import run, scenes

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
PLAIN = dict(h.LINEAR, SPH_QUAD="0")
KINDS = {"plain": PLAIN, "quad": None, "morton": h.MORTON}
SOLVERS = ("wcsph", "dfsph", "pcisph", "iisph")
E53 = 2.0 ** -53
GATE_FRAMES = 600             # frames (one step each) after which the column of dam_gate_wcsph leans on its gate


def give(sim, state, solver):
    """harness.give_sim; iisph's last pressure cannot be uploaded and is zero on both sides at the start: pos and vel are its whole state"""
    if solver == "iisph":
        sim.upload(nat.F_POS, state["pos"]); sim.upload(nat.F_VEL, state["vel"])
    else:
        h.give_sim(sim, state, solver)


def pressed(solver, monkeypatch, env=None, label="library", state=None):
    """a restatement_compare.NativeSide in the pressed state: the plate added and carved (480 of 640 remain), the state uploaded"""
    for k in h.KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    sd = rc.NativeSide(scenes.get(gr.SCENES[solver]), None, solver, label)
    for k in (env or {}):
        assert any(t.startswith(k + "=") for t in sd.sim.overrides()), (k, sd.sim.overrides())
    sim = sd.sim
    assert sim.add_geometry(gr.CARVE_PLATE) == 1 and sim.carve(1, F(gr.D)) == 160 and sim.n_fluid == 480
    give(sim, state if state is not None else wl.run(solver)["state"], solver)
    return sd


def rows_of(ref, group):
    first, count = ref["plate"] if group == 1 else ref["box"]
    return slice(first, first + count)


def check_forces(sim, ref, k, when, groups=(1, 0)):
    """step k (1-based) of the reference: the fluid in lockstep, and every measured group's per-sample forces, bit for bit"""
    st = ref["steps"][k - 1]
    h.same_bits(sim.download(nat.F_POS), st["pos"], "%s, step %d: pos" % (when, k))
    for g in groups:
        h.same_bits(sim.wall_forces(g), st["f"][rows_of(ref, g)], "%s, step %d: per-sample forces of group %d" % (when, k, g))


def check_group_sums(sim, x, f, group, when, abouts=(None, wl.PLATE_CENTRE)):
    for about in abouts:
        c = (0.0, 0.0, 0.0) if about is None else about
        (Fx, Tx), (bF, bT) = wl.exact_load(x, f, c), wl.load_bound(x, f, c)
        force, torque = sim.wall_load(group, about)
        again = sim.wall_load(group, about)
        h.same_bits(force, again[0], "%s: the force read twice" % when)
        h.same_bits(torque, again[1], "%s: the torque read twice" % when)
        print("%s about %s: F %s (err/bound %.3f) T %s (err/bound %.3f)" % (when, c, force, float(np.max(np.abs(force - Fx) / np.maximum(bF, 1e-300))), torque,
                                                                             float(np.max(np.abs(torque - Tx) / np.maximum(bT, 1e-300)))))
        assert (np.abs(force - Fx) <= bF).all(), (when, about, force, Fx, bF)
        assert (np.abs(torque - Tx) <= bT).all(), (when, about, torque, Tx, bT)
    return Fx


# ---- 1: per-sample forces -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("solver", SOLVERS)
def test_per_sample_forces(solver, kind, monkeypatch):
    ref = wl.run(solver)
    sd = pressed(solver, monkeypatch, KINDS[kind], kind)
    try:
        sd.sim.measure_loads(["box", 1])
        assert (sd.sim.wall_forces(1) == 0).all() and (sd.sim.wall_load(None)[0] == 0).all()       # before any step
        for k in range(1, 4):
            sd.step()
            check_forces(sd.sim, ref, k, "%s %s" % (solver, kind))
    finally:
        sd.close()


def test_wcsph_graph_replay_in_multi_step_calls(monkeypatch):
    ref = wl.run("wcsph")
    sd = pressed("wcsph", monkeypatch)
    sim = sd.sim
    try:
        sim.measure_loads([1, "box"])
        before = sim.scalar(nat.S_GRAPH_LAUNCHES)
        sim.step(3)                                                 # a replayed pair and one eager step
        assert sim.scalar(nat.S_GRAPH_LAUNCHES) == before + 1
        check_forces(sim, ref, 3, "step(3)")
        sim.step(2)
        assert sim.scalar(nat.S_GRAPH_LAUNCHES) == before + 2
        check_forces(sim, ref, 5, "step(2) behind it")
    finally:
        sd.close()


# ---- 2: group force and torque -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", ["wcsph", "dfsph", "pcisph"])
def test_group_force_and_torque(solver, monkeypatch):
    ref = wl.run(solver)
    sd = pressed(solver, monkeypatch)
    sim = sd.sim
    try:
        sim.measure_loads(["box", 1])
        sim.step(3)
        f, x = ref["steps"][2]["f"], ref["wall_pos"]
        check_forces(sim, ref, 3, solver)
        for g in (1, 0):
            check_group_sums(sim, x[rows_of(ref, g)], f[rows_of(ref, g)], g, "%s group %d" % (solver, g))
        # all selected: the two groups' f64 results added in selection order -- one more rounding
        for about in (None, wl.PLATE_CENTRE):
            parts = [sim.wall_load(g, about) for g in (0, 1)]
            both = sim.wall_load(None, about)
            h.same_bits(both[0], parts[0][0] + parts[1][0], "all selected: force")
            h.same_bits(both[1], parts[0][1] + parts[1][1], "all selected: torque")
    finally:
        sd.close()


# ---- 3: impulse and seconds ----------------------------------------------------------------------------------------------------------------------
def impulse_reference(ref, group, steps, about):
    """sum dt_k F_k and sum dt_k T_k from the exact per-step sums, and the tolerance: the per-step bounds of the reduction times dt, two roundings
    per step in the accumulation (the product and the addition, each within 2^-53 of sum |dt F|), and for a torque about c != 0 the host's
    L_0 - c x J (three more roundings on |L_0| + |c x J|, bounded through the per-step torque terms about the origin)"""
    x = ref["wall_pos"][rows_of(ref, group)]
    J, L, tolJ, tolL, T = np.zeros(3), np.zeros(3), np.zeros(3), np.zeros(3), 0.0
    absJ, absL = np.zeros(3), np.zeros(3)
    c = np.zeros(3) if about is None else np.asarray(about, dtype=np.float64)
    for k in steps:
        st = ref["steps"][k - 1]
        f, dt = st["f"][rows_of(ref, group)], st["dt"]
        (Fk, Tk), (bF, bT) = wl.exact_load(x, f, c), wl.load_bound(x, f, (0.0, 0.0, 0.0))
        ft, tt = wl.load_terms(x, f, (0.0, 0.0, 0.0))
        J += dt * Fk; L += dt * Tk; T += dt
        tolJ += dt * bF; tolL += dt * bT
        absJ += dt * np.abs(ft).sum(axis=0); absL += dt * np.abs(tt).sum(axis=(0, 2))
    n = len(list(steps))
    tolJ += (2 * n + 2) * E53 * absJ
    cj = np.abs(c).max() * absJ.sum()
    tolL += (2 * n + 8) * E53 * (absL + cj) + np.abs(c).max() * tolJ.sum() * 2
    return J, L, T, tolJ, tolL


def check_impulse(sim, ref, group, steps, when, about=None, reset=False):
    J, L, T, tolJ, tolL = impulse_reference(ref, group, steps, about)
    j, l, sec = sim.wall_impulse(group, about, reset=reset)
    print("%s: J %s (err/tol %.3f), L %s (err/tol %.3f), seconds %.9g" % (when, j, float(np.max(np.abs(j - J) / np.maximum(tolJ, 1e-300))), l,
                                                                       float(np.max(np.abs(l - L) / np.maximum(tolL, 1e-300))), sec))
    assert (np.abs(j - J) <= tolJ).all(), (when, j, J, tolJ)
    assert (np.abs(l - L) <= tolL).all(), (when, l, L, tolL)
    assert abs(sec - T) <= len(list(steps)) * E53 * T, (when, sec, T)


@pytest.mark.parametrize("solver", ["wcsph", "dfsph"])
def test_impulse_and_seconds(solver, monkeypatch):
    """six steps one at a time and in one call (wcsph: replayed pairs), dfsph under its own dt -- not the delta_time the host was given; a reset starts
    the next window"""
    ref = wl.run(solver) if solver == "wcsph" else wl.run(solver, 6, 5e-4)
    if solver == "dfsph":          # delta_time is set to 5e-4 before the first step and dfsph moves to its own 1e-3: the host's value is not the steps'
        assert all(st["dt"] != float(F(ref["state"]["dt"])) for st in ref["steps"]), "dfsph kept the dt it was given"
    one, six = (pressed(solver, monkeypatch, label=label, state=ref["state"]) for label in ("one at a time", "one call"))
    try:
        for sd in (one, six):
            sd.sim.measure_loads(["box", 1])
        for k in range(1, 4):
            one.step()
        for g in (0, 1):
            check_impulse(one.sim, ref, g, range(1, 4), "%s group %d, steps 1-3" % (solver, g))                      # a read without a reset ...
        check_impulse(one.sim, ref, 1, range(1, 4), "%s plate about its centre" % solver, about=wl.PLATE_CENTRE, reset=True)      # ... and one with
        assert one.sim.wall_impulse(1, reset=False)[2] == 0.0 and (one.sim.wall_impulse(1, reset=False)[0] == 0).all()
        for k in range(4, 7):
            one.step()
        check_impulse(one.sim, ref, 1, range(4, 7), "%s plate, the window after the reset" % solver)
        check_impulse(one.sim, ref, 0, range(1, 7), "%s box, all six steps" % solver)
        six.sim.step(6)
        check_forces(six.sim, ref, 6, "%s step(6)" % solver)
        for g in (0, 1):
            check_impulse(six.sim, ref, g, range(1, 7), "%s group %d after one step(6) call" % (solver, g), about=wl.PLATE_CENTRE if g else None)
        a, b = one.sim.wall_impulse(0, reset=False), six.sim.wall_impulse(0, reset=False)
        for u, v, what in zip(a, b, ("impulse", "angular impulse", "seconds")):
            h.same_bits(np.float64(u), np.float64(v), "%s: %s, six calls against one" % (solver, what))
        p = six.sim.wall_impulse(1, reset=False)
        allj = six.sim.wall_impulse(None, reset=True)                                                              # all selected, and every group reset
        h.same_bits(allj[0], b[0] + p[0], "all selected: the groups' impulses in selection order")
        h.same_bits(allj[1], b[1] + p[1], "all selected: the groups' angular impulses in selection order")
        assert allj[2] == b[2] == p[2]
        assert six.sim.wall_impulse(0, reset=False)[2] == 0.0 and six.sim.wall_impulse(1, reset=False)[2] == 0.0
        # one.sim reset the plate alone behind step 3: its groups have measured for different times, and "all selected" is no window of anything
        assert one.sim.wall_impulse(0, reset=False)[2] != one.sim.wall_impulse(1, reset=False)[2]
        h.refused(nat.SPH_E_STATE, lambda: one.sim.wall_impulse(None, reset=True))
        assert one.sim.wall_impulse(0, reset=False)[2] > 0                                                         # (the refused read reset nothing)
        one.sim.wall_impulse(0, reset=True); one.sim.wall_impulse(1, reset=True)
        assert one.sim.wall_impulse(None, reset=False)[2] == 0.0
    finally:
        one.close(); six.close()


@pytest.mark.parametrize("solver", ["wcsph", "pcisph"])
def test_impulse_under_the_adaptive_time_step(solver, monkeypatch):
    """SPH_P_STEP_ADAPTIVE_DT: the dt of every step is the device's.  One handle steps one at a time and reads F_k and dt_k behind every step, its
    twin takes the six steps in one call: the impulse is sum dt_k F_k (two roundings per step) and the two handles agree bit for bit"""
    state = wl.run(solver)["state"]
    one, six = pressed(solver, monkeypatch, state=state), pressed(solver, monkeypatch, state=state)
    try:
        for sd in (one, six):
            sd.sim.set_param("step_max_dt", 4e-4)
            sd.sim.set_param("step_adaptive_dt", 1.0)
            sd.sim.measure_loads([1, "box"])
        J, T, absJ, dts = np.zeros(3), 0.0, np.zeros(3), []
        for k in range(6):
            one.sim.step(1)
            dt = float(F(one.sim.scalar(nat.S_DELTA_TIME)))
            Fk = one.sim.wall_load(1)[0]
            J += dt * Fk; T += dt; absJ += dt * np.abs(Fk); dts.append(dt)
        assert all(d != float(F(state["dt"])) for d in dts), dts      # (the rule's own: not the delta_time the host holds as a launch argument)
        six.sim.step(6)
        j, _, sec = six.sim.wall_impulse(1, reset=False)
        print("%s adaptive: dt %s, J %s vs %s" % (solver, dts, j, J))
        assert (np.abs(j - J) <= 14 * E53 * absJ).all() and abs(sec - T) <= 6 * E53 * T and np.abs(J).max() > 0
        for u, v in zip(one.sim.wall_impulse(1, reset=False), six.sim.wall_impulse(1, reset=False)):
            h.same_bits(np.float64(u), np.float64(v), "%s: six calls against one" % solver)
    finally:
        one.close(); six.close()


# ---- 4: reduction edges ----------------------------------------------------------------------------------------------------------------------------
EDGE = wl.EDGE


@pytest.mark.parametrize("selection", [[5, 2, 4, 0], [3, 1], [4, 3, 5, 2, 1, 0]], ids=["65-1-64-box", "63-plate", "all-six"])
def test_reduction_edges(selection, monkeypatch):
    """groups of 1, 63, 64 and 65 samples (a lane, a wave less one, a wave, a wave and one), selections that are not contiguous in the wall set and
    not in its order (wall_load_ref.edge_run)"""
    ref = wl.edge_run()
    sd = pressed("wcsph", monkeypatch, state=ref["state"])
    sim = sd.sim
    try:
        for n, g in zip((1, 63, 64, 65), (2, 3, 4, 5)):
            assert sim.add_geometry(EDGE[n]) == g
        sim.measure_loads(selection)
        for k in (1, 2):
            sim.step(1)
            st = ref["steps"][k - 1]
            h.same_bits(sim.download(nat.F_POS), st["pos"], "step %d: pos" % k)
            for g in selection:
                first, count = ref["box"] if g == 0 else ref["info"][g]
                f, x = st["f"][first:first + count], ref["wall_pos"][first:first + count]
                h.same_bits(sim.wall_forces(g), f, "step %d: per-sample forces of group %d" % (k, g))
                check_group_sums(sim, x, f, g, "step %d group %d (%d samples)" % (k, g, count), abouts=(None, (0.2, 0.3, 0.2)))
                assert (f != 0).any(), "group %d feels nothing in step %d" % (g, k)
    finally:
        sd.close()


# ---- 5: edits ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", ["wcsph", "dfsph"])
def test_a_group_added_selected_and_removed(solver, monkeypatch):
    """wall_load_ref.edit_run: two steps with the plate measured; a group is added and the selection renewed with it (impulses restart); two steps;
    the new group is removed and leaves the selection, the plate's impulse goes on; the last step's forces read zero until a step has run"""
    ref = wl.edit_run(solver)
    sd = pressed(solver, monkeypatch, state=ref["state"])
    sim = sd.sim
    plate, edge = slice(2402, 2510), slice(2510, 2575)

    def step(k, groups):
        st = ref["steps"][k - 1]
        sd.step()
        h.same_bits(sim.download(nat.F_POS), st["pos"], "step %d: pos" % k)
        for g, rows in groups:
            h.same_bits(sim.wall_forces(g), st["f"][rows], "step %d: per-sample forces of group %d" % (k, g))
        return st["dt"], wl.exact_load(st["wall_pos"][plate], st["f"][plate])[0], np.abs(st["f"][plate].astype(np.float64)).sum(axis=0)

    try:
        sim.measure_loads([1])
        for k in (1, 2):
            step(k, [(1, plate)])
        assert sim.add_geometry(EDGE[65]) == 2
        assert sim.measured_groups == [1] and (sim.wall_forces(1) == 0).all()                       # kept by id; zero until a step has run
        assert sim.wall_impulse(1, reset=False)[2] > 0                                              # ... and the impulse went on through the edit
        sim.measure_loads([2, 1])                                                                   # the renewed selection starts at zero
        assert sim.wall_impulse(1, reset=False)[2] == 0.0
        J, T, absJ = np.zeros(3), 0.0, np.zeros(3)
        for k in (3, 4):
            dt, Fk, a = step(k, [(1, plate), (2, edge)])
            J += dt * Fk; T += dt; absJ += dt * a
        sim.remove_geometry(2)
        assert sim.measured_groups == [1] and (sim.wall_forces(1) == 0).all() and (sim.wall_load(1)[0] == 0).all()
        h.refused(nat.SPH_E_INVALID, lambda: sim.wall_forces(2))
        for k in (5, 6):
            dt, Fk, a = step(k, [(1, plate)])
            J += dt * Fk; T += dt; absJ += dt * a
        j, _, sec = sim.wall_impulse(1, reset=False)
        print("%s: the plate's impulse across the removal %s vs %s, %.9g s" % (solver, j, J, sec))
        assert (np.abs(j - J) <= (108 + 8 + 10) * E53 * absJ).all() and abs(sec - T) <= 4 * E53 * T and np.abs(J).max() > 0
        sim.remove_geometry(1)                                                                      # nobody left: measuring is off
        assert sim.measured_groups == []
        h.refused(nat.SPH_E_STATE, lambda: sim.wall_load(None))
    finally:
        sd.close()


@pytest.mark.parametrize("solver", ["wcsph", "dfsph"])
def test_particles_removed_and_added_between_steps(solver, monkeypatch):
    """wall_load_ref.particles_run: remove_in_box takes the column's top away after two steps -- the measured lists hold entries of particles that
    are gone -- and add_particles puts a few back: the forces stay the yardstick's"""
    ref = wl.particles_run(solver)
    sd = pressed(solver, monkeypatch, state=ref["state"])
    sim = sd.sim

    def step(k):
        st = ref["steps"][k - 1]
        sd.step()
        h.same_bits(sim.download(nat.F_POS), st["pos"], "step %d: pos" % k)
        h.same_bits(sim.wall_forces(1), st["f"][2402:], "step %d: the plate" % k)
        h.same_bits(sim.wall_forces(0), st["f"][:2402], "step %d: the box" % k)

    try:
        sim.measure_loads(["box", 1])
        for k in (1, 2):
            step(k)
        assert 100 < ref["gone"] < 400 and sim.remove_in_box(*wl.REMOVE_BOX) == ref["gone"]
        for k in (3, 4):
            step(k)
        sim.add_particles(wl.ADDED)
        for k in (5, 6):
            step(k)
    finally:
        sd.close()


# ---- 6: a coupled body beside measured walls ------------------------------------------------------------------------------------------------------------
def test_coupled_body_beside_measured_walls(monkeypatch):
    """the restatement's tiny coupled scene (coupled_scenes.coupled), the box measured: the walls' per-sample forces and the body's both hold,
    three solver and body steps"""
    import coupled_scenes as cs
    cfg = cs.coupled("dfsph")
    rg = cs.rigid(cfg)
    s = wl.LoadSolver(cfg, rg)
    s.max_dens = 100
    for k in h.KNOBS:
        monkeypatch.delenv(k, raising=False)
    sd = rc.NativeSide(cfg, rg, "dfsph")
    try:
        sd.sim.measure_loads(["box"])
        for k in range(1, 4):
            with np.errstate(all="ignore"):
                s.step()
            sd.step()
            h.same_bits(sd.get("pos"), s.pos, "step %d: pos" % k)
            h.same_bits(sd.get("rigid_force"), s.body.force, "step %d: the body's per-sample force" % k)
            h.same_bits(sd.sim.wall_forces("box"), s.f_b, "step %d: the box's per-sample force" % k)
            assert (s.f_b != 0).any(axis=1).sum() >= 30 and np.abs(s.body.force).max() > 0
            check_group_sums(sd.sim, s.sc.wall_pos, s.f_b, 0, "coupled, step %d" % k, abouts=(None,))
            with np.errstate(all="ignore"):
                s.rigid_step()
            sd.rigid_step()
            rc._same_body(s.body, sd, "after rigid step %d" % k, True)
    finally:
        sd.close()


# ---- 7: invisibility ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", SOLVERS)
def test_measuring_is_invisible_to_the_fluid(solver, monkeypatch):
    """selecting, reading and resetting against an undisturbed twin over 10 steps; an unselecting handle's steps are those of one that never selected"""
    state = wl.run(solver)["state"]
    a, b = pressed(solver, monkeypatch, state=state), pressed(solver, monkeypatch, state=state)
    try:
        for k in range(1, 11):
            if k == 2:
                a.sim.measure_loads(["box", 1])
            if k == 5:
                a.sim.measure_loads([1])
            if k == 8:
                a.sim.measure_loads([])
            sa, sb = a.step(), b.step()
            h.same_stats(sa, sb, solver, "step %d: statistics" % k)
            for f in (nat.F_POS, nat.F_VEL):
                h.same_bits(a.sim.download(f), b.sim.download(f), "step %d: field %d" % (k, f))
            if 2 <= k < 8:
                a.sim.wall_load(None, wl.PLATE_CENTRE); a.sim.wall_forces(1); a.sim.wall_impulse(1, reset=k % 2 == 0)
        h.refused(nat.SPH_E_STATE, lambda: a.sim.wall_load(None))            # switched off: a read before any selection
        a.sim.step(4); b.sim.step(4)                                        # (wcsph: captured pairs again)
        for f in (nat.F_POS, nat.F_VEL, nat.F_RHO):
            h.same_bits(a.sim.download(f), b.sim.download(f), "after a multi-step call: field %d" % f)
    finally:
        a.close(); b.close()


# ---- 8: refusals -------------------------------------------------------------------------------------------------------------------------------------
def twins_step_alike(a, b, what, steps=2):
    for k in range(steps):
        a.step(1); b.step(1)
    for f in (nat.F_POS, nat.F_VEL):
        h.same_bits(a.download(f), b.download(f), "%s: field %d against the undisturbed twin" % (what, f))


def test_refusals_leave_the_handle_unchanged(monkeypatch):
    st, inv = nat.SPH_E_STATE, nat.SPH_E_INVALID
    # handles that cannot measure: refused, and then stepped beside a twin that was never asked
    for what, cfg, code, kw in (("relaxed", scenes.get("dfsph_tiny_wall"), st, {"arith": "relaxed"}), ("pbf", scenes.get("pbf_tiny_wall"), st, {}),
                                ("clamp walls", scenes.get("dfsph_tiny_clamp"), inv, {})):
        a, b = h.make_handle(cfg, monkeypatch, **kw), h.make_handle(cfg, monkeypatch, **kw)
        a.step(1); b.step(1)
        h.refused(code, lambda: a.measure_loads(["box"]))
        for call in (lambda: a.wall_load(None), lambda: a.wall_impulse(0), lambda: a.wall_forces(0)):
            h.refused(code, call)
        assert a.measured_groups == []
        twins_step_alike(a, b, what)
        a.close(); b.close()
    # a slab handle: one rank of two cannot step without its peer; its own particles and scalars are compared with a twin rank's instead
    cfg = scenes.get("wcsph_tiny_wall")
    a, b = (h.make_handle(cfg, monkeypatch, slab_count=2, slab_rank=0) for _ in range(2))
    h.refused(st, lambda: a.measure_loads(["box"]))
    h.refused(st, lambda: a.wall_load(None))
    assert a.measured_groups == [] and a.n_fluid == b.n_fluid and a.n_wall == b.n_wall
    for f in (nat.F_POS, nat.F_VEL):
        (ia, va), (ib, vb) = a.download_local(f), b.download_local(f)
        h.same_values(ia, ib, "slab rank 0: resident ids against the undisturbed twin")
        h.same_bits(va, vb, "slab rank 0: field %d against the undisturbed twin" % f)
    assert a.scalar(nat.S_DELTA_TIME) == b.scalar(nat.S_DELTA_TIME) and a.scalar(nat.S_SIMULATE_CNT) == b.scalar(nat.S_SIMULATE_CNT)
    a.close(); b.close()
    state = wl.run("dfsph")["state"]
    a, b = pressed("dfsph", monkeypatch, state=state), pressed("dfsph", monkeypatch, state=state)
    try:
        sim = a.sim
        for call in (lambda: sim.wall_load(None), lambda: sim.wall_load(1), lambda: sim.wall_impulse(0), lambda: sim.wall_forces(0)):
            h.refused(st, call)                                             # a read before any selection
        for bad in ([2], [1, 2], [-1], [1, 1], [0, 1, 0]):
            h.refused(inv, lambda: sim.measure_loads(bad))
        with pytest.raises(ValueError):
            sim.measure_loads(["gate"])
        select = sim._lib.sph_wall_load_select
        assert select(sim._h, None, 2) == inv                               # null groups
        many = np.zeros(1025, dtype=np.int32)
        assert select(sim._h, many.ctypes.data, 1025) == inv
        a.step(); b.step()
        sim.measure_loads([1])
        a.step(); b.step()
        kept = (sim.wall_forces(1), sim.wall_load(1), sim.wall_impulse(1, reset=False))
        for bad in ([2], [1, 1]):                                           # a refused selection leaves the standing one
            h.refused(inv, lambda: sim.measure_loads(bad))
        h.refused(inv, lambda: sim.wall_load(0))                            # not selected
        h.refused(inv, lambda: sim.wall_impulse(7))
        h.refused(inv, lambda: sim.wall_forces(0))
        h.refused(inv, lambda: sim.wall_forces(-1))                         # "all selected" has no sample order of its own
        get, imp, forces = sim._lib.sph_wall_load_get, sim._lib.sph_wall_load_impulse, sim._lib.sph_wall_load_forces
        v = np.zeros(3)
        sec = nat.ctypes.c_double(0.0)
        assert get(sim._h, 1, None, None, v.ctypes.data) == inv and get(sim._h, 1, None, v.ctypes.data, None) == inv
        assert imp(sim._h, 1, None, v.ctypes.data, v.ctypes.data, None, 0) == inv and imp(sim._h, 1, None, None, v.ctypes.data, nat.ctypes.byref(sec), 1) == inv
        room = np.zeros(3 * 109, dtype=F)
        assert forces(sim._h, 1, None, 324) == inv and forces(sim._h, 1, room.ctypes.data, 327) == inv and forces(sim._h, 1, room.ctypes.data, 321) == inv
        h.refused(inv, lambda: sim.add_geometry(F([[0.7, 0.5, 0.7]])))      # a refused edit (an isolated sample) leaves the selection as it was
        after = (sim.wall_forces(1), sim.wall_load(1), sim.wall_impulse(1, reset=False))
        assert sim.measured_groups == [1]
        h.same_bits(after[0], kept[0], "per-sample forces after the refused calls")
        for u, w in zip(after[1] + after[2], kept[1] + kept[2]):
            h.same_bits(np.float64(u), np.float64(w), "loads and impulses after the refused calls")
        for k in range(3):
            h.same_stats(a.step(), b.step(), "dfsph", "step %d after the refusals" % k)
        for f in (nat.F_POS, nat.F_VEL, nat.F_RHO):
            h.same_bits(a.sim.download(f), b.sim.download(f), "field %d against the undisturbed twin" % f)
    finally:
        a.close(); b.close()


def test_a_measured_row_beyond_kmax_overflows(monkeypatch):
    """Two coincident samples at a face centre of the rest lattice, inside the column: 36 particles within h of them, 30 at most of a particle.
    With room for the fluid's rows and not for the samples', the handle that measures them reports the existing SPH_E_OVERFLOW from its step; its
    twin, which does not, steps on"""
    from second_restatement import Neighbours, Solver
    cfg = scenes.get("dfsph_tiny_wall")
    pts = F([[0.225, 0.275, 0.2], [0.225, 0.275, 0.2]])
    s = Solver(cfg)
    s.prologue()
    fluid, sample = int(s.nf.count.max()), int(Neighbours(s.sc, pts, s.pos, same=False).count.max())
    assert (fluid, sample) == (30, 36)
    a, b = h.make_handle(cfg, monkeypatch, max_neighbors=fluid), h.make_handle(cfg, monkeypatch, max_neighbors=fluid)
    assert fluid <= a.max_neighbors < sample, a.max_neighbors      # (the library rounds a row's capacity up to whole groups of four entries)
    for sim in (a, b):
        assert sim.add_geometry(pts) == 1
    a.measure_loads([1])
    msg = h.refused(nat.SPH_E_OVERFLOW, lambda: a.step(1))
    assert "overflow" in msg, msg
    b.step(1)
    a.close(); b.close()


# ---- 9: config and runner --------------------------------------------------------------------------------------------------------------------------
def test_scene_loads_of_a_config(monkeypatch):
    cfg = copy.deepcopy(scenes.get("dfsph_tiny_wall"))
    cfg["scene"]["geometry"] = [{"name": "cut", "type": "points", "points": gr.CARVE_PLATE.tolist(), "carve": True}]
    cfg["scene"]["loads"] = ["box", "cut"]
    for k in h.KNOBS:
        monkeypatch.delenv(k, raising=False)
    sim = nat.Simulation(nat.config_from_dict(cfg), config=cfg)
    assert sim.measured_groups == [0, 1] and sim.n_fluid == 480
    sim.step(2)
    assert sim.wall_forces("cut").shape == (108, 3) and sim.wall_forces("box").shape == (2402, 3) and sim.wall_impulse("cut")[2] > 0
    sim.close()


def test_runner_writes_the_load_csv(monkeypatch, tmp_path):
    """dam_gate_wcsph for 20 frames (from rest the gate feels nothing yet: the shape of the file), then for GATE_FRAMES, when the column has settled
    against the gate: the columns carry the handle's own nonzero numbers, each in its place"""
    for k in h.KNOBS:
        monkeypatch.delenv(k, raising=False)
    config = os.path.join(ROOT, "config", "dam_gate_wcsph.json")
    path, geo = str(tmp_path / "loads.csv"), str(tmp_path / "geo")
    run.main(["--config", config, "--steps", "20", "--load-csv", path, "--geometry-ply", geo])
    lines = open(path).read().splitlines()
    assert lines[0] == ",".join(run.LOAD_COLUMNS) and len(lines) == 21
    rows = [ln.split(",") for ln in lines[1:]]
    assert [r[0] for r in rows] == [str(k) for k in range(1, 21)] and {r[2] for r in rows} == {"gate"}
    head = open(os.path.join(geo, "geometry_000000.ply")).read().split("end_header")[0]
    assert "property float fx" in head
    run.main(["--config", config, "--steps", str(GATE_FRAMES), "--load-csv", path])
    sim = run.LAST["ps"]._sim
    rows = [ln.split(",") for ln in open(path).read().splitlines()[1:]]
    assert len(rows) == GATE_FRAMES
    vals = np.array([[float(v) for v in r[3:]] for r in rows])                 # seconds, mean F (3), mean T (3), last F (3)
    assert np.isfinite(vals).all() and (vals[:, 0] > 0).all()
    force, torque = sim.wall_load("gate")
    print("dam_gate_wcsph, %d frames: the gate's last force %s, torque %s" % (GATE_FRAMES, force, torque))
    assert force[0] > 1.0 and force[0] > max(abs(force[1]), abs(force[2])), force                    # the column leans on the gate: along +x
    assert [float(v) for v in rows[-1][10:]] == [float(v) for v in force]                            # the last step's force, bit for bit
    # one step per frame: a frame's mean force and torque are its only step's, (dt F) / dt -- two roundings.  (The contact comes and goes while
    # the column settles, wcsph's pressure clamping at zero in between: the frames that carry a load are compared)
    loaded = np.abs(vals[:, 7]) > 0
    assert loaded.sum() >= 3 and loaded[-1], int(loaded.sum())
    assert np.allclose(vals[loaded, 1:4], vals[loaded, 7:10], rtol=4 * E53, atol=0) and (vals[~loaded, 1:4] == 0).all()
    assert np.allclose(vals[-1, 4:7], torque, rtol=4 * E53, atol=0) and np.abs(torque).max() > 0
    assert float(rows[-1][1]) == pytest.approx(GATE_FRAMES * 2.5e-4) and vals[-1, 0] == pytest.approx(2.5e-4)
    assert len({tuple(v) for v in vals[loaded, 1:4]}) == loaded.sum()                                # a load that moves from frame to frame


@pytest.mark.parametrize("name", ["dam_pillars_dfsph", "dam_gate_wcsph"])
def test_shipped_scenes_still_open_where_loads_cannot_be_measured(name, monkeypatch, capsys):
    """`scene.loads` is applied on handles that can measure and skipped, with one printed line, on relaxed and slab handles, which ran these scenes
    before the key existed; an explicit measure_loads is refused there as ever"""
    cfg = scenes.get(name)
    assert cfg["scene"]["loads"]
    for k in h.KNOBS:
        monkeypatch.delenv(k, raising=False)
    exact = nat.Simulation(nat.config_from_dict(cfg), config=cfg)
    assert len(exact.measured_groups) == len(cfg["scene"]["loads"])
    exact.close()
    capsys.readouterr()
    relaxed = nat.Simulation(nat.config_from_dict(cfg, arith=nat.ARITH_RELAXED), config=cfg)
    assert "scene.loads skipped" in capsys.readouterr().out
    assert relaxed.measured_groups == [] and len(relaxed.geometry()) == len(cfg["scene"]["geometry"]) and relaxed.scalar(nat.S_ARITH_RELAXED) == 1.0
    relaxed.step(3)
    assert np.isfinite(relaxed.download(nat.F_POS)).all()
    h.refused(nat.SPH_E_STATE, lambda: relaxed.measure_loads(cfg["scene"]["loads"]))
    relaxed.close()
    slab = nat.Simulation(nat.config_from_dict(cfg, slab_count=2, slab_rank=0), config=cfg)
    assert "scene.loads skipped" in capsys.readouterr().out
    assert slab.measured_groups == [] and len(slab.geometry()) == len(cfg["scene"]["geometry"])
    h.refused(nat.SPH_E_STATE, lambda: slab.measure_loads(["box"]))
    slab.close()
