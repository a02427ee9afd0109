"""CPU only: the scenes of test_rigid_modes_gpu.py (tests/rigid_modes.py) exercise what that suite asserts.  Without these a body moved
out of the water column's low-index corner would leave the GPU suite green and empty: the quirk count would equal the plain count, and
one-way coupling would look the same as no body at all.

  * dfsph one-way: get_neighbour_count's rigid-entry quirk (the oracle) differs from the plain fluid count (tests/second_restatement.py's
    brute-force search) on some particle, and moves some particle across the `< 20` gate (dfsph_solver.py:258-261);
  * pcisph one-way: delta differs from the same scene with the body inactive;
  * inactive body, `active: false` or no `active` key: the oracle's state after the GPU suite's steps is bit-identical to the scene
    without a solid block."""
import numpy as np
import pytest

from oracle import oracle as orc
from harness import oracle_step
from rigid_modes import STEPS, rigid, scene
from second_restatement import Neighbours, Scene


def make(solver, mode):
    cfg = scene(solver, mode)
    return cfg, orc.Oracle(cfg, solver=solver, num_threads=8, rigid=rigid(cfg))


def test_dfsph_oneway_quirk_count_fires():
    cfg, o = make("dfsph", "oneway")
    sc = Scene(cfg)
    differs = crosses = 0
    for s in range(STEPS):
        pos = o.get(orc.F_POS)                                   # the positions the step's lists are built from
        oracle_step(o, "dfsph")
        o.rigid_step()
        quirk = o.get(orc.F_NBR_COUNT).astype(np.int64)
        plain = Neighbours(sc, pos, pos, same=True).count
        differs = int((quirk != plain).sum())
        crosses = int(((quirk < 20) != (plain < 20)).sum())
        if differs and crosses:
            break
    o.close()
    assert differs > 0, "no particle's quirk count differs from its fluid count in %d steps: the body is not where the quirk fires" % STEPS
    assert crosses > 0, "the quirk moved no particle across the < 20 gate in %d steps" % STEPS


def test_pcisph_oneway_delta_sees_the_body():
    _, one = make("pcisph", "oneway")
    _, off = make("pcisph", "inactive")
    assert np.float32(one.pcisph_delta) != np.float32(off.pcisph_delta), (one.pcisph_delta, off.pcisph_delta)
    assert one.pcisph_max_index[0] >= 0 and np.isfinite(one.pcisph_delta)
    one.close(); off.close()


FIELDS = (orc.F_POS, orc.F_VEL, orc.F_RHO)


@pytest.mark.parametrize("solver", ["dfsph", "wcsph", "pcisph", "iisph"])
def test_inactive_body_is_no_body(solver):
    runs = {m: make(solver, m)[1] for m in ("inactive", "no_active_key", "no_solid")}
    if solver == "pcisph":
        assert len({np.float32(o.pcisph_delta) for o in runs.values()}) == 1
    for s in range(STEPS):
        stats = {m: oracle_step(o, solver) for m, o in runs.items()}
        if solver != "wcsph":
            assert len({(st.n_div, st.n_dens, st.div_err, st.dens_err, st.dt) for st in stats.values()}) == 1, s
    ref = runs["no_solid"]
    for m in ("inactive", "no_active_key"):
        for f in FIELDS:
            assert np.array_equal(runs[m].get(f), ref.get(f)), (m, f)
        if solver == "dfsph":
            assert np.array_equal(runs[m].get(orc.F_NBR_COUNT), ref.get(orc.F_NBR_COUNT)), m
    a, b = runs["inactive"].rigid_scalars(), runs["no_active_key"].rigid_scalars()
    for k in a:
        assert np.array_equal(np.float32(a[k]), np.float32(b[k]), equal_nan=True), k
    assert np.isnan(np.float32(a["centroid"])).all()          # zero volumes: 0 / 0
    for o in runs.values():
        o.close()


def test_one_way_body_on_slab_handles_is_refused():
    """A one-way body is followed on single-GPU handles only: sph_create_rigid refuses a slab handle with one, and does so
    before it touches a device."""
    from cfd_taichi_amd import _native as nat
    cfg = scene("dfsph", "oneway")
    with pytest.raises(nat.SphError, match="one-way rigid body"):
        nat.Simulation(nat.config_from_dict(cfg, slab_rank=0, slab_count=2, slab_ghost_layers=2), rigid=rigid(cfg))
