"""CPU only: what test_scripted_body_gpu.py rests on, inside the second restatement alone (tests/scripted_body.py), and the binding.

  (a) the replay premise: a ScriptedBody fed the (vel, omega, acc, alpha) a dynamic Body had after each of its steps reproduces the dynamic
      run bit for bit -- fluid and body -- as long as the dynamic body meets no wall.  The scene is coupled_scenes.coupled(solver, tilted=True,
      offset=[0.47, 0.2, 0.12]): 640 fluid particles, 168 samples, the body in the water and clear of every wall.  Windows: wcsph 12 steps,
      dfsph 4, iisph 6, pcisph 3 (pcisph throws the body into a wall at its step 4).  The precondition is asserted: no wall hit, and the
      centroid moved by exactly vel dt every step (no wall clamp), with non-zero forces;
  (b) a FIXED body keeps every bit of its positions while the fluid pushes it;
  (c) a library without the new entry points (oracle/liborc_abi.so) still binds, and the new methods raise SphError(SPH_E_STATE);
  (d) header and binding agree on the new names and numbers."""
import os
import re

import numpy as np
import pytest

from cfd_taichi_amd import _native as nat
import coupled_scenes as cs
import scripted_body as sb
import second_restatement_rigid as srr
from harness import bits_equal, same_bits
from second_restatement import F, Solver

REPLAY_OFFSET = [0.47, 0.2, 0.12]
REPLAY_STEPS = {"wcsph": 12, "dfsph": 4, "iisph": 6, "pcisph": 3}


def make_solver(monkeypatch, cfg, plan):
    monkeypatch.setattr(srr, "Body", sb.body_class(plan))
    s = Solver(cfg, cs.rigid(cfg))
    if cfg["solver"]["name"] == "dfsph":
        s.max_dens = 100
    return s


def run_dynamic(monkeypatch, solver, steps):
    """the dynamic run of the replay scene: (cfg, per-step snapshots, the recording), preconditions asserted"""
    cfg = cs.coupled(solver, tilted=True, offset=REPLAY_OFFSET)
    s = make_solver(monkeypatch, cfg, sb.constant(sb.DYNAMIC))
    snaps, largest = [], 0.0
    with np.errstate(all="ignore"):
        for k in range(1, steps + 1):
            s.step()
            largest = max(largest, float(np.abs(s.body.force).max()))
            before = s.body.centroid.copy()
            dt = s.ps_dt if s.ps_dt > 0 else F(s.cfg_dt)
            s.rigid_step()
            b = s.body
            assert b.hit == 0, "the dynamic body met a wall at step %d: nothing a scripted body could replay" % k
            same_bits(b.centroid, before + b.vel * dt, "centroid step == vel dt at step %d (no wall clamp)" % k)
            snaps.append({name: getattr(s, name).copy() for name in ("pos", "vel", "rho")} |
                         {"rigid_pos": b.pos.copy(), "vert": b.vert.copy(), "centroid": b.centroid.copy(), "inertia_inv": b.inertia_inv.copy(),
                          "load": b.load})
    assert largest > 0, "the fluid never pushed the body"
    return cfg, snaps, s.body.recording


@pytest.mark.parametrize("solver", ["wcsph", "dfsph", "iisph", "pcisph"])
def test_replay_premise(solver, monkeypatch):
    steps = REPLAY_STEPS[solver]
    cfg, snaps, recording = run_dynamic(monkeypatch, solver, steps)
    assert len(recording) == steps
    s = make_solver(monkeypatch, cfg, sb.replay(recording))
    with np.errstate(all="ignore"):
        for k in range(1, steps + 1):
            s.step()
            s.rigid_step()
            want, b = snaps[k - 1], s.body
            for name in ("pos", "vel", "rho"):
                same_bits(want[name], getattr(s, name), "replayed fluid %s, step %d" % (name, k))
            for name, mine in (("rigid_pos", b.pos), ("vert", b.vert), ("centroid", b.centroid), ("inertia_inv", b.inertia_inv),
                               ("load", np.array(b.load))):
                same_bits(np.array(want[name]), mine, "replayed body %s, step %d" % (name, k))


def test_fixed_body_keeps_its_bits(monkeypatch):
    cfg = cs.coupled("dfsph")
    s = make_solver(monkeypatch, cfg, sb.constant(sb.FIXED))
    pos0, vert0, c0, inv0 = s.body.pos.copy(), s.body.vert.copy(), s.body.centroid.copy(), s.body.inertia_inv.copy()
    largest = 0.0
    with np.errstate(all="ignore"):
        for _ in range(4):
            s.step()
            largest = max(largest, float(np.abs(s.body.force).max()))
            s.rigid_step()
            b = s.body
            for was, now in ((pos0, b.pos), (vert0, b.vert), (c0, b.centroid), (inv0, b.inertia_inv)):
                assert bits_equal(was, now)
            assert not b.force.any() and not b.vel.any() and not b.s_omega.any() and not b.acc.any() and not b.s_alpha.any()
            assert np.abs(b.load[0]).max() > 0
    assert largest > 0, "the fluid never pushed the obstacle"


def test_library_without_the_entry_points_still_loads_and_refuses():
    from oracle import oracle as orc
    from rigid_release import rigid, scene
    orc.build()
    lib = nat.bind_core(orc.ABI_LIB)
    for name in ("sph_rigid_set_mode", "sph_rigid_set_motion", "sph_rigid_get_load"):
        assert not hasattr(lib, name)
    cfg = scene("dfsph", True)
    sim = nat.Simulation(nat.config_from_dict(cfg), rigid=rigid(cfg), lib=lib)
    for call in (lambda: sim.rigid_set_mode("fixed"), lambda: sim.rigid_set_motion([0, 0, 0], [0, 0, 0]), sim.rigid_load):
        with pytest.raises(nat.SphError) as e:
            call()
        assert e.value.code == nat.SPH_E_STATE
    assert set(sim.rigid_scalars()) == {"centroid", "omega", "vel", "mass", "inertia_inv"}
    with pytest.raises(nat.SphError):
        sim.rigid_scalars(motion=True)
    sim.step(1)
    sim.rigid_step()
    sim.close()


def test_header_and_binding_agree_on_the_new_names():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "sph_mi355x.h")).read()
    for name, value in (("SPH_S_RIGID_ACC", nat.S_RIGID_ACC), ("SPH_S_RIGID_ALPHA", nat.S_RIGID_ALPHA), ("SPH_S_RIGID_MODE", nat.S_RIGID_MODE),
                        ("SPH_RIGID_DYNAMIC", nat.RIGID_DYNAMIC), ("SPH_RIGID_SCRIPTED", nat.RIGID_SCRIPTED), ("SPH_RIGID_FIXED", nat.RIGID_FIXED)):
        assert int(re.search(r"#define %s (\d+)" % name, text).group(1)) == value, name
    assert (nat.S_RIGID_ACC, nat.S_RIGID_ALPHA, nat.S_RIGID_MODE) == (33, 36, 39)
    assert (sb.DYNAMIC, sb.SCRIPTED, sb.FIXED) == (nat.RIGID_DYNAMIC, nat.RIGID_SCRIPTED, nat.RIGID_FIXED)
    # every scalar owns its numbers: the three-component ones three in a row, the inverse inertia nine
    width = {"SPH_S_RIGID_CENTROID": 3, "SPH_S_RIGID_OMEGA": 3, "SPH_S_RIGID_VEL": 3, "SPH_S_RIGID_INERTIA_INV": 9, "SPH_S_RIGID_ACC": 3, "SPH_S_RIGID_ALPHA": 3}
    taken = []
    for name, value in re.findall(r"#define (SPH_S_\w+) (\d+)", text):
        taken += list(range(int(value), int(value) + width.get(name, 1)))
    assert len(taken) == len(set(taken)), sorted(v for v in set(taken) if taken.count(v) > 1)
    for name in ("sph_rigid_set_mode", "sph_rigid_set_motion", "sph_rigid_get_load"):
        assert name in nat.EXPORTS and name in nat.OPTIONAL_EXPORTS
        assert re.search(r"\bint %s\(SphHandle \*h, " % name, text), name
    assert int(re.search(r"#define SPH_ABI_VERSION (\d+)", text).group(1)) == nat.ABI_VERSION == 5
