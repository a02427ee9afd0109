"""GPU suite: the LIBRARY against the second restatement (tests/second_restatement.py, tests/second_restatement_rigid.py), with no oracle
in the loop.  Same scenes, same fields and the same step-by-step bit comparison as tests/test_second_restatement.py (the loop is
coupled_scenes.compare_run); everything is downloaded through the C ABI (F_*, SPECIES_RIGID, rigid_scalars(), StepStats).

Every case runs the restatement once and two handles beside it: a default one, and one created under SPH_CELL_ORDER=morton -- the
reference-order cells with the quad and plain sweeps, and the Morton curve with the staged 16-bit-list sweeps.

PBF (tests/second_restatement_pbf.py) has no staged sweeps; its kernels come in a quad (four lanes per particle, up to 65 536 particles) and a
plain instantiation, and k_pbf_xsph walks the cell lists itself, through the Morton slots from 131 072 particles on.  Its cases put FOUR
handles beside the restatement (pbf_handles): default = k_pbf_{lambda,delta,xsph}<true> on linear cells; SPH_QUAD=0 = the three <false>
kernels on linear cells; SPH_CELL_ORDER=morton = <true> on the Morton curve; morton + SPH_QUAD=0 = <false> on the Morton curve, which is
what a handle of 131 072 particles or more runs.  Found by test_pbf_compute_density_alone and fixed: compute_density() left delta_pos in
the order of the previous sort (sph_compute_density carried only pbf_lambda through the re-sort)."""
import numpy as np
import pytest

from cfd_taichi_amd import scenes
import coupled_scenes as cs
import restatement_compare as rc
from harness import same_bits
from test_second_restatement import KINDS, PBF_KINDS, _past_minimum, check_pbf, check_pbf_rho_bound, check_uncoupled, pbf_case, pbf_squeezed, uncoupled_case

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
    same_bits(a.pos, b.pos, "positions with an inactive body and with none")
    same_bits(a.vel, b.vel, "velocities with an inactive body and with none")


# ---- PBF: quad and plain kernels, linear and Morton cells, against tests/second_restatement_pbf.py ------------------------------------------

PBF_KNOBS = {"default (quad, linear cells)": {},
             "SPH_QUAD=0 (plain, linear cells)": {"SPH_QUAD": "0"},
             "SPH_CELL_ORDER=morton (quad, Morton cells)": {"SPH_CELL_ORDER": "morton", "SPH_CELL_TILE": "4"},
             "SPH_CELL_ORDER=morton SPH_QUAD=0 (plain, Morton cells)": {"SPH_CELL_ORDER": "morton", "SPH_QUAD": "0"}}


def pbf_handles(monkeypatch):
    """the four handles of a PBF case; every knob that was set must be named by sim.overrides() (they are ignored without SPH_DEV=1)"""
    def maker(label, knobs):
        def make(cfg, rg, solver):
            for name in ("SPH_QUAD", "SPH_CELL_ORDER", "SPH_CELL_TILE"):
                monkeypatch.delenv(name, raising=False)
            for name, value in knobs.items():
                monkeypatch.setenv(name, value)
            side = rc.NativeSide(cfg, rg, solver, "library (%s)" % label)
            for name in ("SPH_QUAD", "SPH_CELL_ORDER", "SPH_CELL_TILE"):
                monkeypatch.delenv(name, raising=False)
            named = side.sim.overrides()
            for name in ("SPH_QUAD", "SPH_CELL_ORDER", "SPH_CELL_TILE"):
                assert [t for t in named if t.startswith(name + "=")] == (["%s=%s" % (name, knobs[name])] if name in knobs else []), (label, named)
            return side
        return make

    return [maker(label, knobs) for label, knobs in PBF_KNOBS.items()]


@pytest.mark.parametrize("kind", PBF_KINDS)
def test_pbf_steps(kind, monkeypatch):
    """the cases of test_second_restatement.test_pbf_steps on the four handles: rho, pbf_lambda, delta_pos, pos, vel after every step"""
    cfg, steps, state = pbf_case(kind)
    check_pbf(kind, rc.compare_run(cfg, steps, pbf_handles(monkeypatch), state=state))


def test_pbf_compute_density_alone(monkeypatch):
    """sim.compute_density() (k_pbf_lambda's rho_only path, quad and plain) after 3 squeezed steps: rho as compute_all_rho alone gives it,
    pbf_lambda, delta_pos, pos and vel untouched"""
    cfg = scenes.get("pbf_tiny_wall")
    ev = rc.compare_run(cfg, 3, pbf_handles(monkeypatch), state=pbf_squeezed(cfg), density_after=True)
    assert ev["lambda_active"][-1] > 0, "pbf_lambda is all zero: 'untouched' would prove nothing"


def test_pbf_density_within_the_f64_bound(monkeypatch):
    """rho of compute_density() on the jittered wall state against a plain f64 all-pairs poly6 sum of the same positions, per particle within
    the derived bound of check_pbf_rho_bound -- a check that rests on no restatement's reading.  The second restatement's own rho satisfies the
    bound (test_pbf_rho_of_the_restatement_within_the_f64_bound, CPU), so the library, bit-equal to it, must."""
    cfg = scenes.get("pbf_tiny_wall")
    pos, vel = cs.jitter(cfg)
    for make in pbf_handles(monkeypatch):
        side = make(cfg, None, "pbf")
        try:
            side.set_state(pos, vel)
            side.density_only()
            nat = side.nat
            wall_pos, wall_vol = side.sim.download(nat.F_WALL_POS, nat.SPECIES_WALL), side.sim.download(nat.F_WALL_VOL, nat.SPECIES_WALL)
            check_pbf_rho_bound(cfg, side.get("pos"), wall_pos, wall_vol, side.get("rho"), side.label)
        finally:
            side.close()
