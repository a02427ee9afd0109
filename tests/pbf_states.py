"""Input states and the comparison for the relaxed PBF sweeps (csrc/sph_pbf_kernels.h, RX): a PBF step has no solver loop whose trip count can
flip and is a continuous function of its input apart from the clamp planes and lambda's `con == 0` branch, so the sweep-by-sweep method of
tests/pinned_loops.py carries over with the f64 oracle as reference and the f32 oracle's own error on the same input as yardstick.

  bulk    pinned_loops.state(scene, seed): the lattice compressed to 0.88 about its centroid, jitter 0.15 d, velocities +-0.5 m/s
  clamp   (pbf_tiny_clamp) the bulk state translated so that on each axis the 5 % quantile of the coordinates lies on the lower clamp plane
          box_min + particle_radius -- in f64, rounded to f32 once, the same bits for every participant.  The compressed column otherwise withdraws
          from every plane and the clamp branch never runs.

tests/test_pbf_relaxed_cpu.py shows on the two oracles alone that these inputs are fair (lambda active on a fair share of the particles, equal
discrete sets, the yardstick tight); tests/test_pbf_relaxed_gpu.py holds the library to them.

TEST INFRASTRUCTURE ONLY: nothing here imports the HIP library; a handle is anything with upload / step_pbf / download."""
import functools

import numpy as np

from cfd_taichi_amd import scenes
from oracle import oracle as orc
from pinned_loops import FLOOR, MARGIN, STATS, compare, errors, state, stats3, wall_mask  # noqa: F401  (re-exported)

# field ids are those of include/sph_mi355x.h, which the oracle shares
from oracle.oracle import F_PBF_DELTA_POS, F_PBF_LAMBDA, F_POS, F_RHO, F_VEL  # noqa: E402,F401
FIELDS = (("rho", F_RHO), ("pbf_lambda", F_PBF_LAMBDA), ("delta_pos", F_PBF_DELTA_POS), ("pos", F_POS), ("vel", F_VEL))
SEEDS = (1, 3)
# (scene, state kind, steps): the cases of both test files
CASES = (("pbf_tiny_wall", "bulk", 5), ("pbf_tiny_clamp", "bulk", 5), ("pbf_tiny_clamp", "clamp", 3))
CLAMP_QUANTILE = 0.05


@functools.lru_cache(maxsize=None)
def pbf_state(scene, kind, seed):
    """(pos, vel) as read-only f32 arrays"""
    pos, vel, _ = state(scene, seed)
    if kind == "bulk":
        return pos, vel
    assert kind == "clamp" and scene == "pbf_tiny_clamp", (scene, kind)
    sc = scenes.get(scene)["scene"]
    p = pos.astype(np.float64)
    plane = np.asarray(sc["box_min"], dtype=np.float64) + float(sc["particle_radius"])
    p += plane - np.quantile(p, CLAMP_QUANTILE, axis=0)
    p = np.ascontiguousarray(p, dtype=np.float32)
    p.setflags(write=False)
    return p, vel


def planes(cfg):
    """per axis the f32 values a clamped coordinate can have: the plane as the f32 participants form it and the f64 plane rounded to f32"""
    sc = cfg["scene"]
    r32, r64 = np.float32(sc["particle_radius"]), float(sc["particle_radius"])
    lo = [{np.float32(np.float32(b) + r32), np.float32(float(b) + r64)} for b in sc["box_min"]]
    hi = [{np.float32(np.float32(b) - r32), np.float32(float(b) - r64)} for b in sc["box_max"]]
    return lo, hi


def clamped(cfg, pos):
    """bool (N, 3): entries sitting exactly on a clamp plane.  Empty where the scene has wall particles instead of clamp planes."""
    pos = np.asarray(pos, dtype=np.float32)
    out = np.zeros(pos.shape, dtype=bool)
    if cfg["solver"].get("boundary_handle", True):
        return out
    lo, hi = planes(cfg)
    for a in range(3):
        for v in lo[a] | hi[a]:
            out[:, a] |= pos[:, a] == v
    return out


def snapshot(get):
    res = {name: np.array(get(f)) for name, f in FIELDS}
    for a in res.values():
        a.setflags(write=False)
    return res


def run_oracle(scene, kind, seed, steps, precision, num_threads=8):
    """[fields after step 1, ..., after step `steps`]"""
    cfg = scenes.get(scene)
    o = orc.Oracle(cfg, num_threads=num_threads, precision=precision)
    pos, vel = pbf_state(scene, kind, seed)
    o.set(orc.F_POS, pos); o.set(orc.F_VEL, vel)
    out = []
    for _ in range(steps):
        o.step_pbf(1)
        out.append(snapshot(o.get))
    o.close()
    return out


@functools.lru_cache(maxsize=None)
def references(scene, kind, seed, steps):
    """(f32 oracle, f64 oracle) per step on pbf_state(scene, kind, seed): computed once, shared by every test that needs them, never written to."""
    return run_oracle(scene, kind, seed, steps, "f32"), run_oracle(scene, kind, seed, steps, "f64")


def run_handle(sim, scene, kind, seed, steps):
    """The same on a library handle (cfd_taichi_amd._native.Simulation) created by the caller under whatever overrides select the path."""
    pos, vel = pbf_state(scene, kind, seed)
    sim.upload(F_POS, pos); sim.upload(F_VEL, vel)
    out = []
    for _ in range(steps):
        sim.step_pbf(1)
        out.append(snapshot(sim.download))
    return out


def populations(cfg, pos0):
    """name -> mask over the particles of the input positions: within one support radius (4 r) of a box face / not"""
    h = 4.0 * float(cfg["scene"]["particle_radius"])
    p = np.asarray(pos0, dtype=np.float64)
    lo, hi = np.asarray(cfg["scene"]["box_min"], dtype=np.float64), np.asarray(cfg["scene"]["box_max"], dtype=np.float64)
    wall = ((p - lo < h) | (hi - p < h)).any(1)
    return {"all": np.ones(len(p), dtype=bool), "wall": wall, "rest": ~wall}


def check(label, cfg, pos0, cand, r32, r64, fields=None):
    """One participant's fields against the f64 oracle's, by the f32 oracle's own error: q50, q99 and max of the per-particle error over the three
    populations, each <= MARGIN x the f32 oracle's + FLOOR.  Returns (failures, {field: worst ratio})."""
    failures, worst = [], {}
    pops = populations(cfg, pos0)
    for name, _ in FIELDS:
        if fields is not None and name not in fields:
            continue
        ec, er = errors(cand[name], r64[name]), errors(r32[name], r64[name])
        worst[name] = 0.0
        for pop, m in pops.items():
            if not m.any():
                continue
            for stat, c, r, ratio, ok in compare(ec[m], er[m]):
                worst[name] = max(worst[name], ratio)
                if not ok:
                    failures.append("%s %s[%s] %s: %.3e > %g x %.3e + %.1e (ratio %.2f, n = %d)" % (label, name, pop, stat, c, MARGIN, r, FLOOR, ratio,
                                                                                                 int(m.sum())))
    return failures, worst


def discrete_sets(cfg, res):
    """(lambda != 0, clamped entries) of one participant's fields"""
    return res["pbf_lambda"] != 0, clamped(cfg, res["pos"])
