"""CPU suite: the input states of tests/test_relaxed_sweeps_gpu.py are fair, on the reference alone (tests/pinned_loops.py).

The f32 and the f64 oracle run every pinned-loop stage on every (scene, seed) the GPU file uses.  A comparison of a sweep against the f64
oracle means something only if the state exercises the sweep and no discrete gate separates the two precisions:
  * equal iteration counts (n_div, n_dens, n_div_evals);
  * F_NBR_COUNT identical for every particle: a pair within one ulp of r = h flips list membership between the precisions;
  * rho* > rho_0 in the f64 oracle for enough particles (else D6 / D7 are invisible behind max(., rho_0)), D rho > 0 for enough (D3 / D4
    behind max(., 0)), and both sides of the `neighbour count < 20` skip present.
The printed f32-vs-f64 statistics are the yardstick the GPU file holds the relaxed sweeps to."""
import numpy as np
import pytest

import pinned_loops as pl

SMALL = ("dfsph_tiny_wall", "dfsph_tiny_clamp")          # 640 particles
# scene -> stages the GPU file runs on it
SCENE_STAGES = {"dfsph_tiny_wall": tuple(pl.STAGES), "dfsph_tiny_clamp": tuple(pl.STAGES), "dfsph_small": tuple(pl.STAGES), "dfsph_rigid_small": ("all",)}
EXPECTED_COUNTS = {"d3": (0, 1, 1), "warm": (0, 1, 1), "div3": (3, 1, 4), "dens3": (0, 3, 1), "all": (3, 3, 4), "cfl": (3, 3, 4)}


@pytest.mark.parametrize("scene", sorted(SCENE_STAGES))
def test_states_are_fair_on_the_reference_alone(scene):
    small = scene in SMALL
    for seed in pl.SEEDS:
        for stage in SCENE_STAGES[scene]:
            r32, r64 = pl.references(scene, seed, stage)
            n = len(r64.nbr)
            dense = float((r64["rho_adv"] > 1000.0).mean())          # rho* > rho_0
            diverging = float((r64["rho_der"] > 0.0).mean())         # D rho > 0
            sparse = float((r64.nbr < 20).mean())
            print("%s seed %d %-5s: %d particles, counts %s, rho* > rho_0 %.1f %%, D rho > 0 %.1f %%, under 20 neighbours %.1f %%, within h of a box face %.1f %%, dt %.6g" % (
                scene, seed, stage, n, r64.counts, 100 * dense, 100 * diverging, 100 * sparse, 100 * float(pl.wall_mask(scene, seed).mean()), r64.dt))
            for name, _ in pl.FIELDS:
                print("    f32 vs f64 %-8s q50 %.2e q99 %.2e max %.2e" % ((name,) + pl.stats3(pl.errors(r32[name], r64[name]))))
            if r64.rigid_force is not None:
                coupled = int((np.abs(r64.rigid_force).sum(1) > 0).sum())
                print("    f32 vs f64 %-8s q50 %.2e q99 %.2e max %.2e (%d of %d samples feel the fluid)" % (
                    ("rigid_f",) + pl.stats3(pl.errors(r32.rigid_force, r64.rigid_force)) + (coupled, len(r64.rigid_force))))
                assert coupled >= 0.05 * len(r64.rigid_force), (scene, seed, stage, coupled)
            assert r32.counts == r64.counts == EXPECTED_COUNTS[stage], (scene, seed, stage, r32.counts, r64.counts)
            assert np.array_equal(r32.nbr, r64.nbr), (scene, seed, stage, int((r32.nbr != r64.nbr).sum()))
            assert dense >= (0.05 if small else 0.25), (scene, seed, stage, dense)
            assert diverging >= (0.05 if small else 0.15), (scene, seed, stage, diverging)
            assert 0.0 < sparse < 1.0 and (not small or sparse >= 0.01), (scene, seed, stage, sparse)
            assert np.all(r32["rho_der"][r32.nbr < 20] == 0.0) and np.all(r64["rho_der"][r64.nbr < 20] == 0.0)
            if stage == "cfl":
                assert r64.dt < 1e-2 and r32.dt < 1e-2          # the CFL rule's own result, not the cap
            elif stage == "all":
                assert np.float32(r64.dt) == np.float32(r32.dt) == np.float32(1e-3)          # the cap, on both
    # every class of the count mod 8 is met once the seeds are pooled
    pooled = np.concatenate([pl.references(scene, seed, SCENE_STAGES[scene][0])[1].nbr for seed in pl.SEEDS])
    assert set(np.unique(pooled % 8)) == set(range(8))
    if scene == "dfsph_tiny_wall":
        assert pl.wall_mask(scene, pl.SEEDS[0]).mean() >= 0.2


def _pool(scene, stage, candidate_of):
    pool = pl.Pool()
    for seed in pl.SEEDS:
        r32, r64 = pl.references(scene, seed, stage)
        pool.add(scene, seed, candidate_of(seed, r32), r32, r64)
    return pool


def test_comparator_accepts_the_yardstick_itself():
    assert _pool("dfsph_tiny_wall", "all", lambda seed, r32: r32).report("f32 oracle as its own candidate") == []


@pytest.mark.parametrize("field", ["rho", "rho_der", "rho_adv", "vel_adv", "vel"])
def test_comparator_rejects_1e4_on_the_wall_particles(field):
    """The f32 oracle's own fields with ONE field scaled by 1 + 1e-4 on the particles next to a box face -- the size of error a wrong wall term
    would make, and one the envelope tests pass: rejected, in that field's wall population, and nowhere else."""
    scene, stage = "dfsph_tiny_wall", "all"

    def perturbed(seed, r32):
        out = pl.Result(r32)
        a = r32[field].copy()
        a[pl.wall_mask(scene, seed)] *= np.float32(1.0 + 1e-4)
        out[field] = a
        return out
    failures = _pool(scene, stage, perturbed).report("perturbed " + field)
    assert failures and all((" %s[" % field) in f for f in failures), failures
    assert any("[wall/" in f for f in failures) and not any("[rest/" in f for f in failures), failures


def test_comparator_floor_only_covers_rounding_of_the_download():
    """A statistic that is exactly 0 on the reference side (clamped rho*) leaves the candidate the floor, 2 x 2^-24 of the field's maximum, no more."""
    ref = np.full(100, 1000.0)
    ok = pl.compare(pl.errors(ref * (1 + 2.0 ** -24), ref), pl.errors(ref, ref))
    bad = pl.compare(pl.errors(ref * (1 + 4.0 * 2.0 ** -24), ref), pl.errors(ref, ref))
    assert all(r[4] for r in ok) and not any(r[4] for r in bad)
