"""Scenes and helpers of the release / freeze suites (TEST INFRASTRUCTURE: test_rigid_release_cpu.py and test_rigid_release_gpu.py).

The reference treats `ps.active_rigid` as a runtime value (ParticleSystem.py:63-64, :399-407, main.py:100-106, :170): let the fluid settle with
the body inactive, then `ps.active_rigid[None] = 1; ps.reset_grid(); ps.update_grid(); ps.init_rigid_particles_data()` and the body drops into
the fluid as it is then.  The oracle has no setter for the flag.  What the suites check is the equivalence the reference's sequence implies:
an inactive body never moves, so "created inactive, K steps, release" equals "a fresh oracle created with `active: true` and given the fluid
state of step K" (`fluid_state` / `give`: everything a step reads of the fluid, as tests/test_handover_fullsize_gpu.py moves it).

Placements (the geometry is dfsph_rigid_small's throughout):
  * TWO_WAY: dfsph_rigid_small's own `pos_offset` moved 0.05 towards the water column (x 0.75 -> 0.70): the nearest samples stand 0.05 from
    the nearest fluid particles, inside the support radius of 0.1 from the first step after the release (at 0.75 the gap is exactly 0.1 and
    only dfsph, through the quirk count, notices the body within 40 steps).  It is away from the low-index corner of the column, which is all
    get_neighbour_count's rigid-entry quirk reaches, so pcisph's delta (pcisph_solver.py:28-47, kept from construction: the oracle cannot
    be told one) is the same with the body in the grid or not -- test_rigid_release_cpu.py proves both.
  * rigid_modes.OFFSET: the body inside that corner, for one-way coupling (the quirk count is all a one-way body changes in the fluid).  There
    pcisph's delta does see the body (test_rigid_modes_cpu.py), so the one-way release runs with dfsph alone."""
import numpy as np

import rigid_modes
from cfd_taichi_amd import scenes
from harness import make_oracle
from rigid_modes import DT, SOLVERS, rigid  # noqa: F401  (re-exported for the two suites)

K, AFTER = 10, 30                       # steps with the body inactive, steps after the release
TWO_WAY = [round(v - d, 3) for v, d in zip(scenes.get("dfsph_rigid_small")["solid"]["pos_offset"], (0.05, 0.0, 0.0))]      # [0.70, 0.1, 0.5]
ONE_WAY = list(rigid_modes.OFFSET)


def scene(solver, active, fs_couple=True, offset=None):
    """dfsph_rigid_small's geometry with `solver`, the DT table of rigid_modes, the body at `offset` (default: TWO_WAY for a coupled body,
    ONE_WAY for fs_couple false); active None: no solid block at all."""
    cfg = rigid_modes.scene(solver, "no_solid" if active is None else "inactive")
    cfg["solver"]["fs_couple"] = bool(fs_couple)
    if active is None:
        return cfg
    cfg["solid"]["pos_offset"] = list(offset if offset is not None else (TWO_WAY if fs_couple else ONE_WAY))
    cfg["solid"]["active"] = bool(active)
    return cfg


def body_oracle(cfg, solver):
    return make_oracle(cfg, solver, rigid=rigid(cfg))


def same_fields(a, b):
    return all(np.array_equal(a[k], b[k]) for k in a)
