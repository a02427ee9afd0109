"""CPU suite: the inputs of tests/test_slab_pbf_gpu.py are fair, shown on the f32 oracle alone (tests/slab_pbf_states.py).

The sharded PBF runs are held to the one-GPU handle bit for bit.  That says something about the slab path only if, on these inputs,
  * particles migrate across EVERY cut a decomposition can choose: every column boundary x = 0.1 k strictly inside the fluid's initial x-extent is
    crossed by >= 15 particles between step 0 and step 60;
  * the lambda halo carries values: pbf_lambda != 0 on >= 30 % of the particles after step 1;
  * no particle leaves the grid (a slab handle bins strictly: a particle outside the grid sits in no cell): every position stays strictly inside
    the box through step 60;
  * the one-message particle exchange holds: the largest speed x dt stays under a quarter cell;
  * on long_clamp the clamp branch runs: >= 100 coordinates sit exactly on a clamp plane after step 60.
Conditions, not measurements.  Measured when this file was added (seed 1, seed 3): smallest crossing count 20, 20 on long_wall and 20, 21 on
long_clamp; lambda != 0 on 40 %, 41 %; smallest coordinate of any step 0.026, 0.016 on long_wall (0.019 after step 60); largest speed 35, 40 m/s
x 2.5e-4 s = 10 mm against a 100 mm cell; 174, 136 coordinates on a clamp plane."""
import numpy as np
import pytest

import slab_pbf_states as sp


@pytest.mark.parametrize("scene", ["long_wall", "long_clamp"])
@pytest.mark.parametrize("seed", sp.SEEDS)
def test_the_long_states_are_fair(scene, seed):
    cfg = sp.config(scene)
    h = sp.support_radius(cfg)
    pos0, _ = sp.state(scene, seed)
    assert len(pos0) == sp.N_LONG
    run = sp.oracle_run(scene, seed)
    col0, col1 = sp.columns(cfg, pos0), sp.columns(cfg, run[sp.STEPS]["pos"])
    lo, hi = int(col0.min()), int(col0.max())
    assert hi - lo + 1 == 15, (lo, hi)                                    # 15 fluid columns (of a 21-column grid: four slabs all hold fluid)
    crossings = {b: int(((col0 < b) != (col1 < b)).sum()) for b in range(lo + 1, hi + 1)}
    lam_share = float((run[1]["pbf_lambda"] != 0).mean())
    box_lo, box_hi = np.asarray(cfg["scene"]["box_min"], dtype=np.float64), np.asarray(cfg["scene"]["box_max"], dtype=np.float64)
    path = np.stack(run["pos_path"]).astype(np.float64)
    on_plane = sp.clamp_plane_hits(cfg, run[sp.STEPS]["pos"])
    print("%s seed %d: N %d, fluid columns %d..%d, smallest crossing count %d, lambda != 0 on %.0f %%, coordinates in [%.3f, %.3f] x [%.3f, %.3f] x "
          "[%.3f, %.3f], largest speed %.1f m/s, %d coordinates on a clamp plane" % (
              scene, seed, len(pos0), lo, hi, min(crossings.values()), 100 * lam_share, path[..., 0].min(), path[..., 0].max(), path[..., 1].min(),
              path[..., 1].max(), path[..., 2].min(), path[..., 2].max(), run["max_speed"], on_plane))
    assert min(crossings.values()) >= 15, crossings
    assert lam_share >= 0.30, lam_share
    assert np.isfinite(path).all() and (path > box_lo).all() and (path < box_hi).all()
    assert run["max_speed"] * float(cfg["solver"]["delta_time"]) < 0.25 * h, run["max_speed"]
    if scene == "long_clamp":
        assert on_plane >= 100, on_plane
