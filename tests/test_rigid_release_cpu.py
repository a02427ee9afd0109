"""CPU only: the preconditions of test_rigid_release_gpu.py, on the oracle alone, so that a green GPU suite means something (scenes and the
hand-over: tests/rigid_release.py).

  (a) the placements exercise the release: a fresh oracle created with `active: true` and given an inactive oracle's fluid state of step K
      does not stay equal to the inactive oracle -- after the 30 further steps the fluid positions differ for every solver with
      `fs_couple: true`, and for one-way dfsph the neighbour count (get_neighbour_count's rigid-entry quirk) differs;
  (b) pcisph's delta (pcisph_solver.py:28-47) is bit-identical with the body active and inactive at the two-way placement.  A release keeps the
      delta of construction and the oracle cannot be told one, so only where (b) holds can a released pcisph handle be held to the oracle.
      It HOLDS for rigid_release.TWO_WAY (the first placement tried after dfsph_rigid_small's own), so the pcisph cases of the GPU suite compare
      with the oracle.  It does not hold in rigid_modes' corner placement (test_rigid_modes_cpu.py): the one-way release runs dfsph alone.

Also here: the binding's behaviour on a library without the two entry points (oracle/liborc_abi.so behind Simulation).  A slab handle cannot be
made without a device: that refusal is covered in the GPU file."""
import numpy as np
import pytest

from cfd_taichi_amd import _native as nat
from oracle import oracle as orc
from harness import fluid_state, give, oracle_step
from rigid_release import AFTER, K, ONE_WAY, SOLVERS, TWO_WAY, body_oracle, scene


def released_and_inactive(solver, fs_couple):
    """(the inactive oracle after K + AFTER steps, the fresh active oracle given its step-K fluid state after AFTER coupled steps, neighbour
    counts that differed on the way)"""
    off = body_oracle(scene(solver, False, fs_couple), solver)
    for _ in range(K):
        oracle_step(off, solver)
    on = give(body_oracle(scene(solver, True, fs_couple), solver), fluid_state(off, solver), solver)
    counts = 0
    for _ in range(AFTER):
        oracle_step(off, solver)
        oracle_step(on, solver)
        on.rigid_step()
        if solver == "dfsph":
            counts += int((off.get(orc.F_NBR_COUNT) != on.get(orc.F_NBR_COUNT)).sum())
    return off, on, counts


@pytest.mark.parametrize("solver", SOLVERS)
def test_two_way_release_changes_the_fluid(solver):
    off, on, _ = released_and_inactive(solver, True)
    assert (off.get(orc.F_POS) != on.get(orc.F_POS)).any(), "the released body left no trace in the fluid after %d steps: wrong placement" % AFTER
    assert np.isfinite(on.get(orc.F_POS)).all() and on.rigid_scalars()["vel"][1] < 0
    off.close(); on.close()


def test_one_way_release_changes_the_neighbour_count():
    off, on, counts = released_and_inactive("dfsph", False)
    assert counts > 0, "the quirk count never differed from the fluid count: the body is not where the quirk fires"
    assert not on.get(orc.F_RIGID_FORCE).any() and on.rigid_scalars()["vel"][1] < 0
    off.close(); on.close()


def test_pcisph_delta_does_not_see_the_two_way_placement():
    a, b = body_oracle(scene("pcisph", True), "pcisph"), body_oracle(scene("pcisph", False), "pcisph")
    assert np.float32(a.pcisph_delta) == np.float32(b.pcisph_delta) and a.pcisph_max_index == b.pcisph_max_index, (TWO_WAY, a.pcisph_delta, b.pcisph_delta)
    assert np.isfinite(a.pcisph_delta) and a.pcisph_max_index[0] >= 0
    a.close(); b.close()
    # ... and does see the corner placement of the one-way scenes: no pcisph case there
    a, b = body_oracle(scene("pcisph", True, False), "pcisph"), body_oracle(scene("pcisph", False, False), "pcisph")
    assert np.float32(a.pcisph_delta) != np.float32(b.pcisph_delta), (ONE_WAY, a.pcisph_delta)
    a.close(); b.close()


def test_library_without_the_entry_points_still_loads_and_refuses():
    """tests/test_backend_swap.py puts oracle/liborc_abi.so behind Simulation; it exports neither sph_rigid_set_active nor sph_rigid_init_data.
    Binding it must go on working, and calling either method raises SphError(SPH_E_STATE)."""
    orc.build()
    lib = nat.bind_core(orc.ABI_LIB)
    assert not hasattr(lib, "sph_rigid_set_active") and not hasattr(lib, "sph_rigid_init_data")
    cfg = scene("dfsph", False)
    from rigid_release import rigid
    sim = nat.Simulation(nat.config_from_dict(cfg), rigid=rigid(cfg), lib=lib)
    for call in (lambda: sim.rigid_set_active(1), sim.rigid_init_data):
        with pytest.raises(nat.SphError) as e:
            call()
        assert e.value.code == nat.SPH_E_STATE
    sim.step(1)             # the handle is as usable as before
    sim.close()


def test_header_and_binding_agree_on_the_new_names():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "sph_mi355x.h")).read()
    assert int(re.search(r"#define SPH_S_RIGID_ACTIVE (\d+)", text).group(1)) == nat.S_RIGID_ACTIVE
    taken = [int(v) for v in re.findall(r"#define SPH_S_\w+ (\d+)", text)]
    assert taken.count(nat.S_RIGID_ACTIVE) == 1 and not (10 <= nat.S_RIGID_ACTIVE < 29), "the scalar's number is taken"
    for name in nat.OPTIONAL_EXPORTS:
        assert re.search(r"\bint %s\(SphHandle \*h" % name, text), name
    assert int(re.search(r"#define SPH_ABI_VERSION (\d+)", text).group(1)) == nat.ABI_VERSION == 5
