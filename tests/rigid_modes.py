"""Scenes of the two rigid-body branches that `scenes._with_solid` never builds (TEST INFRASTRUCTURE: test_rigid_modes_cpu.py and
test_rigid_modes_gpu.py):

  * one-way coupling: `solver.fs_couple: false`, active body.  The fluid ignores the body, but the body is still binned into the grid
    (ParticleSystem.py:399-407), so its samples still enter get_neighbour_count's rigid-entry quirk (:424-445: dfsph's `< 20` gate,
    dfsph_solver.py:258-261, and pcisph's fullest neighbourhood, pcisph_solver.py:28-47); it falls under gravity and bounces off
    the walls (rigid_solver.py:216-232, main.py:169-171).
  * an inactive body: `solid.active: false`, or no `active` key at all (ParticleSystem.py:63-64 defaults to inactive): never binned,
    never stepped.

The geometry is dfsph_rigid_small's with the body moved into the low-index corner of the water column: there the quirk measures from
a fluid particle to the FLUID particles whose ids are the local indices of the rigid samples in its cells, which lie in that same
corner, so the quirk count differs from the plain fluid count (test_rigid_modes_cpu.py proves it for every scene used here).  The body
stands 0.005 above the height at which the wall impulse acts (box_min + diameter, rigid_solver.py:56): it reaches the floor after
about 32 steps of 1e-3."""
import copy

from cfd_taichi_amd import mesh, scenes

SOLVERS = ("dfsph", "wcsph", "pcisph", "iisph")
# delta_time of each solver as the small scenes of scenes.SCENES set it (dfsph_tiny_wall, wcsph_tiny_wall, dfsph_tiny_wall_pcisph /
# dfsph_tiny_wall_iisph)
DT = {"dfsph": 1e-3, "wcsph": 2.5e-4, "pcisph": 1e-3, "iisph": 1e-3}
OFFSET = [0.4, 0.055, 0.15]
STEPS = 40
MODES = ("oneway", "inactive", "no_active_key")


def scene(solver, mode):
    """mode: 'oneway' (fs_couple false, active body), 'inactive' (active false, fs_couple left true), 'no_active_key' (the `active` key
    removed), 'no_solid' (the solid block removed: what an inactive body must be equal to)."""
    cfg = copy.deepcopy(scenes.get("dfsph_rigid_small"))
    cfg["solver"]["name"] = solver
    cfg["solver"]["delta_time"] = DT[solver]
    solid = cfg["solid"]
    solid["pos_offset"] = list(OFFSET)
    if mode == "oneway":
        cfg["solver"]["fs_couple"] = False
        solid["active"] = True
    elif mode == "inactive":
        solid["active"] = False
    elif mode == "no_active_key":
        del solid["active"]
    elif mode == "no_solid":
        del cfg["solid"]
    else:
        raise ValueError(mode)
    return cfg


def rigid(cfg):
    return mesh.rigid_from_config(cfg) if "solid" in cfg else None
