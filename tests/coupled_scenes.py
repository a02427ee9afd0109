"""The scenes of the second restatement's tests beyond scenes.SCENES (TEST INFRASTRUCTURE: test_second_restatement.py and
test_second_restatement_gpu.py; the step-by-step comparison both share is restatement_compare.py).

  * clamp twins of dfsph_tiny_wall_pcisph / dfsph_tiny_wall_iisph: `boundary_handle: false`, start_pos 0.1 as in dfsph_tiny_clamp -- from rest
    (ten steps of free fall), and thrown at the floor (clamp_thrown) so that particles sit on the clamp planes and the pressure loop works;
  * a tiny coupled scene: dfsph_tiny_wall (640 fluid, 2 402 wall particles) with `fs_couple: true` and a small box (cube1.stl scaled by 0.3,
    168 samples) standing in the water's support radius from step 1, 0.002 above the height where the wall impulse acts;
  * its tilted, lighter twin (attitude_offset [20, 0, 35], rho_0 500), raised so that no sample starts below box_min + diameter;
  * the same geometry with `fs_couple: false` (one-way) and with `active: false`."""
import copy

import numpy as np

from cfd_taichi_amd import mesh, scenes

DT = {"dfsph": 1e-3, "pcisph": 1e-3, "iisph": 1e-3, "wcsph": 2.5e-4}
OFFSET = [0.47, 0.052, 0.1]
TILTED_OFFSET = [0.47, 0.13, 0.1]
# pcisph throws the upright body sideways before it reaches the floor; its own, lower start puts the impulse inside the window
PCISPH_OFFSET = [0.47, 0.0505, 0.1]
# steps compared: the body's first wall impulse lies inside each window (asserted by the tests; these scenes print it at step 20 for dfsph
# and iisph, 10 for pcisph, 81 for wcsph)
STEPS = {"dfsph": 22, "iisph": 22, "pcisph": 12, "wcsph": 84}
ONEWAY_STEPS = 22
# the tilted twin has no impulse to wait for: 12 steps (a water particle has slipped through a wall and pushes the body from outside the
# grid by step 10 of wcsph; the body tumbles from step 2 of pcisph and dfsph)
TILTED_STEPS = {"dfsph": 6, "pcisph": 12, "iisph": 12, "wcsph": 12}      # (dfsph's density loop runs into its cap of 100 from step 5 on)


def clamp_twin(solver):
    cfg = copy.deepcopy(scenes.get("dfsph_tiny_clamp"))
    cfg["solver"]["name"] = solver
    cfg["solver"]["delta_time"] = DT[solver]
    return cfg


def coupled(solver, tilted=False, fs_couple=True, active=True, solid=True, offset=None):
    cfg = copy.deepcopy(scenes.get("dfsph_tiny_wall"))
    cfg["solver"]["name"] = solver
    cfg["solver"]["delta_time"] = DT[solver]
    if not solid:
        return cfg
    cfg["solver"]["fs_couple"] = fs_couple
    if offset is None:
        offset = TILTED_OFFSET if tilted else (PCISPH_OFFSET if solver == "pcisph" and fs_couple else OFFSET)
    cfg["solid"] = {"mesh": "assets/cube1.stl", "voxel_radius": 0.025, "scale": 0.3, "rho_0": 500 if tilted else 2000,
                    "pos_offset": list(offset), "attitude_offset": [20.0, 0.0, 35.0] if tilted else [0.0, 0.0, 0.0],
                    "fill": True, "active": active}
    return cfg


def rigid(cfg):
    return mesh.rigid_from_config(cfg) if "solid" in cfg else None


CLAMP_THROWN_STEPS = 30


def jitter(cfg, seed=20261005):
    """the seeded ragged state of test_jittered_state_five_steps: up to 0.3 d of displacement, up to 0.5 m/s of velocity"""
    from second_restatement import Scene
    pos0 = Scene(cfg).pos
    rng = np.random.default_rng(seed)
    d = np.float32(2 * cfg["scene"]["particle_radius"])
    pos = (pos0 + rng.uniform(-0.3, 0.3, pos0.shape).astype(np.float32) * d).astype(np.float32)
    vel = rng.uniform(-0.5, 0.5, (len(pos0), 3)).astype(np.float32)
    return pos, vel


def clamp_thrown(cfg):
    """the ragged state thrown down and into the x = 0 corner at 4 m/s: the block, 0.075 above the clamp plane box_min + radius, reaches
    the floor and the side plane within 20 steps of 1e-3 and is compressed against them"""
    pos, vel = jitter(cfg)
    vel = (vel + np.array([-4.0, -4.0, 0.0], dtype=np.float32)).astype(np.float32)
    return pos, vel
