"""GPU suite: scripted and fixed rigid bodies (sph_rigid_set_mode / sph_rigid_set_motion / sph_rigid_get_load) -- bit for bit, no tolerances.

  1. a scripted body (constant vel and omega) against the second restatement with tests/scripted_body.ScriptedBody, four solvers, default and
     Morton handles, every field restatement_compare.compare_run compares, plus load, acc and alpha after every body step;
  2. a fixed obstacle against the restatement; the samples and vertices keep the bits of creation while the forces are non-zero;
  3. replay on the library alone: a scripted handle fed a dynamic handle's (vel, omega, acc, alpha) step by step retraces it -- fluid, body,
     stats and load (the premise, inside the restatement: test_scripted_body_cpu.py);
  4. let go: fixed for 5 steps, dynamic for 5, against the restatement doing the same;
  5. refusals (no body, unknown mode, NaN motion, a motion that leaves the grid) leave the handle as it was;
  6. the mirror API: a config with solid.motion through ParticleSystem and rigid_solver equals a handle driven by direct calls."""
import copy
import hashlib

import numpy as np
import pytest

from cfd_taichi_amd import _native as nat
import coupled_scenes as cs
import restatement_compare as rc
from harness import same_bits
import scripted_body as sb
import second_restatement_rigid as srr
from test_scripted_body_cpu import REPLAY_OFFSET, REPLAY_STEPS
from test_second_restatement import _past_minimum

pytestmark = pytest.mark.gpu

VEL, OMEGA = (-0.5, -1.0, 0.25), (2.0, -3.0, 1.5)
SCRIPTED_STEPS = {"wcsph": 12, "dfsph": 4, "pcisph": 6, "iisph": 6}
SOLVERS = ["wcsph", "dfsph", "pcisph", "iisph"]
# wcsph at rest has rho < rho_0 next to the upright body and clamps such a pressure to zero: in the second restatement the water first pushes the
# fixed body at step 74 (a window of 20 steps, the first plan, sees forces of exactly zero on every side); two steps beyond that
FIXED_WCSPH_STEPS = 76


def compare(monkeypatch, cfg, steps, plan):
    monkeypatch.setattr(srr, "Body", sb.body_class(plan))
    return rc.compare_run(cfg, steps, sb.sides(monkeypatch, plan), rg=cs.rigid(cfg))


def check_pushed(solver, ev):
    assert max(ev["force"]) > 0, "the fluid never pushed the body"
    if solver != "wcsph":
        assert _past_minimum(solver, ev["iters"]), "the pressure loop never ran past its minimum"


@pytest.mark.parametrize("solver", SOLVERS)
def test_scripted_body_against_the_restatement(solver, monkeypatch):
    cfg = cs.coupled(solver, tilted=True, offset=REPLAY_OFFSET)
    ev = compare(monkeypatch, cfg, SCRIPTED_STEPS[solver], sb.constant(sb.SCRIPTED, VEL, OMEGA))
    print("%s scripted: iterations %s; largest per-sample force %.4g" % (solver, ev["iters"], max(ev["force"])))
    check_pushed(solver, ev)
    b = ev["solver"].body
    assert b.steps == SCRIPTED_STEPS[solver] and np.array_equal(b.vel, np.array(VEL, dtype=np.float32))


@pytest.mark.parametrize("solver", SOLVERS)
def test_fixed_obstacle_against_the_restatement(solver, monkeypatch):
    cfg = cs.coupled(solver)
    steps = FIXED_WCSPH_STEPS if solver == "wcsph" else cs.STEPS[solver]
    ev = compare(monkeypatch, cfg, steps, sb.constant(sb.FIXED))          # (PlannedSide holds rigid_pos / rigid_vert to the bits of creation)
    print("%s fixed: iterations %s; largest per-sample force %.4g" % (solver, ev["iters"], max(ev["force"])))
    assert max(ev["force"]) > 0, "the fluid never pushed the obstacle"


def _native(cfg, solver):
    return rc.NativeSide(cfg, cs.rigid(cfg), solver)


def _body_state(side):
    sc = side.sim.rigid_scalars(motion=True)
    return {"rigid_pos": side.get("rigid_pos"), "rigid_vert": side.get("rigid_vert"), "centroid": sc["centroid"], "inertia_inv": sc["inertia_inv"],
            "vel": sc["vel"], "omega": sc["omega"], "acc": sc["acc"], "alpha": sc["alpha"]}


@pytest.mark.parametrize("solver", SOLVERS)
def test_replay_on_the_library(solver):
    cfg = cs.coupled(solver, tilted=True, offset=REPLAY_OFFSET)
    dyn, scr = _native(cfg, solver), _native(cfg, solver)
    try:
        scr.sim.rigid_set_mode("scripted")
        g = np.float32(cfg["scene"]["gravity"])
        largest = 0.0
        for k in range(1, REPLAY_STEPS[solver] + 1):
            st_d, st_s = dyn.step(), scr.step()
            if solver != "wcsph":
                assert (st_d.n_dens, np.float32(st_d.dens_err), np.float32(st_d.dt)) == (st_s.n_dens, np.float32(st_s.dens_err), np.float32(st_s.dt)), k
            if solver == "dfsph":
                assert (st_d.n_div, np.float32(st_d.div_err), np.float32(st_d.div_first_err)) == (st_s.n_div, np.float32(st_s.div_err), np.float32(st_s.div_first_err)), k
            for name in ("pos", "vel", "rho", "rigid_force"):
                same_bits(dyn.get(name), scr.get(name), "%s before body step %d" % (name, k))
            largest = max(largest, float(np.abs(dyn.get("rigid_force")).max()))
            dyn.rigid_step()
            sc = dyn.sim.rigid_scalars(motion=True)
            scr.sim.rigid_set_motion(sc["vel"], sc["omega"], sc["acc"], sc["alpha"])
            scr.rigid_step()
            a, b = _body_state(dyn), _body_state(scr)
            for name in a:
                same_bits(a[name], b[name], "body %s after body step %d" % (name, k))
            (fd, td), (fs, ts) = dyn.sim.rigid_load(), scr.sim.rigid_load()
            assert fd.tobytes() == fs.tobytes() and td.tobytes() == ts.tobytes(), (k, fd, fs, td, ts)
            # the dynamic handle's acc is its own load over its mass, plus gravity (rigid_solver.py:40-41)
            mass = np.float32(sc["mass"])
            want = fd.astype(np.float32) / mass + np.array([g * np.float32(0.0), g * np.float32(-1.0), g * np.float32(0.0)], dtype=np.float32)
            same_bits(want, sc["acc"], "acc == F32(force) / mass + g at step %d" % k)
        assert largest > 0, "the fluid never pushed the body"
    finally:
        dyn.close()
        scr.close()


@pytest.mark.parametrize("solver", ["wcsph", "pcisph"])
def test_let_go(solver, monkeypatch):
    """the tilted body in the water (pushed from step 1): held for 5 steps, then released into the flow it has shaped"""
    cfg = cs.coupled(solver, tilted=True, offset=REPLAY_OFFSET)
    ev = compare(monkeypatch, cfg, 10, sb.let_go(5))
    b = ev["solver"].body
    assert min(ev["force"]) > 0 and b.vel.any() and b.omega.any(), "the released obstacle never moved"


def _digest(side, solver):
    h = hashlib.sha256()
    for name in ("pos", "vel", "rho"):
        h.update(side.get(name).tobytes())
    if side.sim.n_rigid:
        for v in _body_state(side).values():
            h.update(np.asarray(v, dtype=np.float32).tobytes())
        h.update(side.get("rigid_force").tobytes())
    return h.hexdigest()


def _refused(call, code):
    with pytest.raises(nat.SphError) as e:
        call()
    assert e.value.code == code, e.value


@pytest.mark.parametrize("solver", ["wcsph", "dfsph"])
def test_refusals_leave_the_handle_alone(solver):
    cfg = cs.coupled(solver, tilted=True, offset=REPLAY_OFFSET)
    bare = rc.NativeSide(cs.coupled(solver, solid=False), None, solver)
    try:
        for call in (lambda: bare.sim.rigid_set_mode("fixed"), lambda: bare.sim.rigid_set_motion(VEL, OMEGA), bare.sim.rigid_load):
            _refused(call, nat.SPH_E_STATE)                                    # no body
    finally:
        bare.close()
    asked, twin = _native(cfg, solver), _native(cfg, solver)
    try:
        for side in (asked, twin):
            side.sim.rigid_set_mode("scripted")
            side.sim.rigid_set_motion(VEL, OMEGA)
        _refused(asked.sim.rigid_load, nat.SPH_E_STATE)                        # before the first body step
        for side in (asked, twin):
            side.step()
            side.rigid_step()
        was = _digest(asked, solver)
        _refused(lambda: asked.sim.rigid_set_mode(3), nat.SPH_E_INVALID)
        _refused(lambda: asked.sim.rigid_set_mode(-1), nat.SPH_E_INVALID)
        _refused(lambda: asked.sim.rigid_set_motion((0.0, float("nan"), 0.0), OMEGA), nat.SPH_E_INVALID)
        _refused(lambda: asked.sim.rigid_set_motion(VEL, OMEGA, alpha=(float("inf"), 0.0, 0.0)), nat.SPH_E_INVALID)
        assert asked.sim.rigid_scalars(motion=True)["mode"] == nat.RIGID_SCRIPTED and _digest(asked, solver) == was
        # the guard: a motion whose sphere leaves the grid is refused by the step, on the host, before anything is launched
        asked.step(), twin.step()
        was, load = _digest(asked, solver), asked.sim.rigid_load()
        asked.sim.rigid_set_motion((0.0, -1000.0, 0.0), OMEGA)
        _refused(asked.rigid_step, nat.SPH_E_INVALID)
        assert _digest(asked, solver) == was and np.abs(asked.get("rigid_force")).max() > 0
        assert asked.sim.rigid_load()[0].tobytes() == load[0].tobytes()
        asked.sim.rigid_set_motion(VEL, OMEGA)                                 # the motion of before: the refused step did not count
        asked.rigid_step(), twin.rigid_step()
        for _ in range(5):
            for side in (asked, twin):
                side.step()
                side.rigid_step()
            assert _digest(asked, solver) == _digest(twin, solver)
        assert asked.sim.rigid_load()[1].tobytes() == twin.sim.rigid_load()[1].tobytes()
    finally:
        asked.close()
        twin.close()


@pytest.mark.parametrize("mode", ["fixed", "scripted"])
def test_mirror_api(mode):
    """main.py's order: ParticleSystem(config), the solver, rigid_solver(ps, config); then solver.step(), rigid.step() per frame"""
    from cfd_taichi_amd import ParticleSystem, pcisph_solver, rigid_solver
    cfg = cs.coupled("pcisph", tilted=True, offset=REPLAY_OFFSET)
    direct = _native(cfg, "pcisph")
    mirrored = copy.deepcopy(cfg)
    mirrored["solid"]["motion"] = {"mode": mode} if mode == "fixed" else {"mode": mode, "vel": list(VEL), "omega": list(OMEGA)}
    ps = ParticleSystem(mirrored)
    solver = pcisph_solver(ps, mirrored)
    rigid = rigid_solver(ps, mirrored)
    try:
        assert rigid.mode == mode
        direct.sim.rigid_set_mode(mode)
        if mode == "scripted":
            direct.sim.rigid_set_motion(VEL, OMEGA)
        for k in range(4):
            direct.step()
            direct.rigid_step()
            solver.step()
            rigid.step()
            same_bits(direct.get("pos"), ps.fluid_particles.pos.to_numpy(), "fluid pos, step %d" % k)
            same_bits(direct.get("rigid_pos"), ps.rigid_particles.pos.to_numpy(), "sample pos, step %d" % k)
            same_bits(direct.rigid_scalars()["centroid"], ps.rigid_centriod[None], "centroid, step %d" % k)
            assert direct.sim.rigid_load()[0].tobytes() == rigid.load()[0].tobytes()
        assert np.abs(rigid.load()[0]).max() > 0
    finally:
        direct.close()
        ps._sim.close()
