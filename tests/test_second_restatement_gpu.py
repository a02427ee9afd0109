"""GPU suite: the LIBRARY against the second restatement (tests/second_restatement.py, tests/second_restatement_rigid.py), with no oracle
in the loop.  Same scenes, same fields and the same step-by-step bit comparison as tests/test_second_restatement.py (the loop is
coupled_scenes.compare_run); everything is downloaded through the C ABI (F_*, SPECIES_RIGID, rigid_scalars(), StepStats).

Every case runs the restatement once and two handles beside it: a default one, and one created under SPH_CELL_ORDER=morton -- the
reference-order cells with the quad and plain sweeps, and the Morton curve with the staged 16-bit-list sweeps."""
import numpy as np
import pytest

from cfd_taichi_amd import scenes
import coupled_scenes as cs
import restatement_compare as rc
from test_second_restatement import KINDS, _past_minimum, check_uncoupled, uncoupled_case

pytestmark = pytest.mark.gpu


def handles(monkeypatch):
    def default(cfg, rg, solver):
        monkeypatch.delenv("SPH_CELL_ORDER", raising=False)
        return rc.NativeSide(cfg, rg, solver, "library (default handle)")

    def morton(cfg, rg, solver):
        monkeypatch.setenv("SPH_CELL_ORDER", "morton")
        monkeypatch.setenv("SPH_CELL_TILE", "4")
        side = rc.NativeSide(cfg, rg, solver, "library (SPH_CELL_ORDER=morton)")
        assert "SPH_CELL_ORDER=morton" in side.sim.overrides(), side.sim.overrides()
        return side

    return [default, morton]


@pytest.mark.parametrize("scene", ["wcsph_tiny_wall", "wcsph_tiny_clamp", "dfsph_tiny_wall", "dfsph_tiny_clamp"])
def test_wcsph_dfsph_ten_steps(scene, monkeypatch):
    """the scenes of test_wcsph_ten_steps / test_dfsph_ten_steps"""
    cfg = scenes.get(scene)
    ev = rc.compare_run(cfg, 10, handles(monkeypatch))
    print("%s: iterations %s" % (scene, ev["iters"]))
    if scene.startswith("dfsph"):
        assert _past_minimum("dfsph", ev["iters"]), "neither solver loop ever ran past its minimum"


@pytest.mark.parametrize("scene", ["wcsph_tiny_wall", "dfsph_tiny_wall"])
def test_jittered_state_five_steps(scene, monkeypatch):
    cfg = scenes.get(scene)
    rc.compare_run(cfg, 5, handles(monkeypatch), state=cs.jitter(cfg))


@pytest.mark.parametrize("solver", ["pcisph", "iisph"])
@pytest.mark.parametrize("kind", KINDS)
def test_pcisph_iisph_steps(solver, kind, monkeypatch):
    cfg, steps, state = uncoupled_case(solver, kind)
    check_uncoupled(solver, kind, rc.compare_run(cfg, steps, handles(monkeypatch), state=state))


@pytest.mark.parametrize("solver", ["dfsph", "pcisph", "iisph", "wcsph"])
@pytest.mark.parametrize("tilted", [False, True], ids=["upright", "tilted"])
def test_coupled_scene(solver, tilted, monkeypatch):
    cfg = cs.coupled(solver, tilted=tilted)
    ev = rc.compare_run(cfg, cs.TILTED_STEPS[solver] if tilted else cs.STEPS[solver], handles(monkeypatch), rg=cs.rigid(cfg))
    print("%s %s: iterations %s; impulse steps %s; largest per-sample force %.4g" % (solver, "tilted" if tilted else "upright", ev["iters"],
                                                                                   ev["hit_steps"], max(ev["force"])))
    assert max(ev["force"]) > 0, "the fluid never pushed the body"
    if tilted and solver == "wcsph":
        assert ev["outside_deposits"] > 0, "no fluid particle outside the grid deposited a force"
    if solver != "wcsph":
        assert _past_minimum(solver, ev["iters"]), "the pressure loop never ran past its minimum"
    if not tilted:
        assert ev["hit_steps"], "no step took the wall-impulse branch (collision_point_cnt > 0)"


@pytest.mark.parametrize("solver", ["dfsph", "pcisph"])
def test_one_way_body(solver, monkeypatch):
    cfg = cs.coupled(solver, fs_couple=False)
    ev = rc.compare_run(cfg, cs.ONEWAY_STEPS, handles(monkeypatch), rg=cs.rigid(cfg))
    print("%s one-way: impulse steps %s; quirk count differs for %d particle-steps" % (solver, ev["hit_steps"], ev["quirk"]))
    assert max(ev["force"]) == 0, "a force on a body the fluid does not couple to"
    assert ev["hit_steps"], "the body never reached the floor impulse"
    assert ev["quirk"] > 0, "the quirk count never differed from the plain fluid count"


def test_inactive_body_equals_no_body(monkeypatch):
    with_body, without = cs.coupled("pcisph", active=False), cs.coupled("pcisph", solid=False)
    a = rc.compare_run(with_body, 5, handles(monkeypatch), rg=cs.rigid(with_body))["solver"]
    b = rc.compare_run(without, 5, handles(monkeypatch))["solver"]
    rc.same(a.pos, b.pos, "positions with an inactive body and with none")
    rc.same(a.vel, b.vel, "velocities with an inactive body and with none")
