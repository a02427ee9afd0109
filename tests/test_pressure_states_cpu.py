"""CPU suite: the input states of tests/test_relaxed_pressure_sweeps_gpu.py and tests/test_relaxed_wcsph_sweeps_gpu.py are fair, shown on the
reference alone (tests/pressure_states.py).

The relaxed WCSPH, PCISPH and IISPH steps are held to MARGIN x the f32 oracle's own error against the f64 oracle with no loop pinned.  That says
something only if, on every (scene, seed, compression, step) the GPU files use,
  * the pressure loop runs the same number of iterations and leaves through the same exit on the f32 oracle, the f64 oracle and sixteen seeded
    legal f32 schedules (four on the 5 880-particle scenes), and the neighbour counts of the step's input positions are identical (a pair within one ulp of r = h flips list membership);
  * on the clamp scenes the coordinates on a clamp plane are the same set on all four, and many;
  * the seeded schedules -- the reference against itself -- pass the GPU files' own bar; the worst ratio is printed;
  * the cases exercise what they are there for: a pcisph step that ends on the cap of 80 and one well below it, an iisph step that leaves through
    the residual test and one through "trend to divergence", and at compression 1.0 a share of particles without pressure next to a share with.
A case that fails is replaced HERE (pressure_states.CASES), never excused on the GPU.

Measured at the commit that added this file: worst seeded-schedule ratio 3.97 (pcisph clamp scene, press_force, one class of the count mod 8, 253
entries; 3.79 and 3.48 on pcisph at compression 1.0, 3.42 on iisph; wcsph at most 2.14, the 5 880-particle scenes at most 1.78).  A hundred
schedules instead of sixteen reach 5.1 on those small classes of press_iter: the bar is not loose for the pressure fields of the loop solvers.
Iterations: pcisph 80 (cap) / 72 / 45 at 0.88 and 36 / 16 / 12, 40 / 15 / 16 at 1.0; iisph 5 (left on "trend to divergence") / 1 / 4 at 0.88.
Particles on a clamp plane: wcsph 97-118, pcisph 191 / 66 / 39, iisph 100 / 93 / 107.
Replaced on the way, each for a reason found here: every case at compression 0.97 (pressure_states.CASES says why), pcisph_config_backup at
(seed 1, 0.97) and (seed 3, 0.88) and iisph_config_backup at (seed 3, 0.88) (f32 and f64 neighbour counts differ in step 2 or 3), and
dfsph_tiny_wall_pcisph at (seed 3, 0.88) (one schedule runs another number of iterations)."""
import numpy as np
import pytest

import pressure_states as ps

SCHEDULES = tuple(range(1, 17))          # seeded legal executions of the f32 oracle per 640-particle case; the first four on 5 880 particles
ALL_CASES = [(solver,) + case for solver, cases in ps.CASES.items() for case in cases]
CAP = 5e-5          # the f32 oracle's max-norm error against f64, every field of every step: the yardstick is tight (a condition; largest seen 3.7e-5)


@pytest.fixture(scope="module")
def legal():
    cache = {}

    def get(scene, seed, compression, steps=ps.STEPS, vel_amp=ps.VEL_AMP):
        key = (scene, seed, compression, steps, vel_amp)
        if key not in cache:
            cache[key] = [ps.run_oracle(scene, seed, compression, steps, "f32", schedule=s, vel_amp=vel_amp) for s in (SCHEDULES[:4] if scene in ps.LARGE else SCHEDULES)]
        return cache[key]
    return get


def bar(scene, seed, compression, steps, cands, r32, r64, vel_amp=ps.VEL_AMP):
    """(failures, worst row) of candidates against the GPU files' bar"""
    failures, worst = [], None
    for k, cand in enumerate(cands):
        pool = ps.pool(scene)
        for s in range(steps):
            ps.add_step(pool, scene, seed, compression, s, cand[s], r32[s], r64[s], vel_amp)
        failures += ["%s seed %d %g schedule %d: %s[%s] %s: %.3e > %g x %.3e + %.1e (ratio %.2f, n = %d)" % (
            scene, seed, compression, SCHEDULES[k], r[0], r[1], r[3], r[4], ps.MARGIN, r[5], ps.FLOOR, r[6], r[2]) for r in pool.rows() if not r[7]]
        w = max(pool.rows(), key=lambda r: r[6])
        worst = w if worst is None or w[6] > worst[6] else worst
    return failures, worst


@pytest.mark.parametrize("solver,scene,seed,compression", ALL_CASES, ids=["%s-%d-%g" % c[1:] for c in ALL_CASES])
def test_case_is_fair_on_the_reference_alone(solver, scene, seed, compression, legal):
    cfg = ps.config(scene)
    r32, r64 = ps.references(scene, seed, compression)
    others = legal(scene, seed, compression)
    n = len(r64[0].nbr)
    assert n == (5879 if scene in ps.LARGE else 640)
    for s in range(ps.STEPS):
        tag = "%s seed %d %g step %d" % (scene, seed, compression, s + 1)
        runs = [r32[s], r64[s]] + [o[s] for o in others]
        share = float((r64[s][ps.PRESSURE_FIELD[solver]] > 0).mean())
        sets = [ps.clamped(cfg, r["pos"]) for r in runs]
        n_clamped = int(sets[1].any(1).sum())
        print("%s: counts %s, pressure > 0 on %.1f %%, %d clamped particles, f32 max-norm errors %s" % (
            tag, r64[s].counts, 100 * share, n_clamped, " ".join("%s %.1e" % (name, ps.errors(r32[s][name], r64[s][name]).max()) for name, _ in ps.FIELDS[solver])))
        for r in runs:
            assert r.counts == r64[s].counts, (tag, [x.counts for x in runs])
            assert np.array_equal(r.nbr, r64[s].nbr), (tag, int((r.nbr != r64[s].nbr).sum()))
            assert r.lost == 0 and all(np.isfinite(a).all() for a in r.values()), tag
        for c in sets:
            assert np.array_equal(c, sets[1]), (tag, int((c != sets[1]).sum()))
        if cfg["solver"].get("boundary_handle", True):
            assert n_clamped == 0, (tag, n_clamped)
        else:
            assert n_clamped >= ps.MIN_CLAMPED[solver], (tag, n_clamped)
        for name, _ in ps.FIELDS[solver]:
            assert ps.errors(r32[s][name], r64[s][name]).max() < CAP, (tag, name)
        if s == 0:          # pressure carried by enough particles that no statistic of it is one particle's
            assert (r64[s][ps.PRESSURE_FIELD[solver]] > 0).sum() >= ps.MIN_SPLIT, (tag, share)
        if compression == 1.0:          # skipped and worked tiles side by side
            assert 0 < share < 1, (tag, share)
            if s == 0:
                assert 0.05 <= 1.0 - share <= 0.95, (tag, share)
    failures, worst = bar(scene, seed, compression, ps.STEPS, others, r32, r64)
    print("%s seed %d %g: worst seeded-schedule ratio %.2f (%s %s %s, n = %d)" % ((scene, seed, compression, worst[6]) + worst[:2] + (worst[3], worst[2])))
    assert not failures, "\n".join(failures)


def test_cases_cover_what_the_issue_of_each_solver_is():
    for solver, cases in ps.CASES.items():
        assert len({c[1] for c in cases}) >= 2, solver                                                                      # two seeds
        wall = [c for c in cases if ps.config(c[0])["solver"].get("boundary_handle", True) and c[0] not in ps.LARGE]
        assert len({c[2] for c in wall}) >= 2 and {c[2] for c in cases} <= {0.88, 0.97, 1.0}, solver                         # two compressions
        assert any(not ps.config(c[0])["solver"].get("boundary_handle", True) for c in cases), solver                        # a clamp scene
        assert any(c[0] in ps.LARGE for c in cases), solver                                                                  # 5 880 particles
        assert all(ps.solver_of(c[0]) == solver for c in cases)
        # the wall terms act on particles that carry pressure (wcsph: -rho_0 p_i / rho_i^2 sum_b V_b grad W is 0 where p_i is): measured 16, 63, 58
        # on the three wcsph_tiny_wall cases, and all the pressure of the two uncompressed ones sits next to a wall
        pressed = [int((ps.wall_neighbours(c[0], ps.state(*c)[0]) & (ps.references(*c)[1][0][ps.PRESSURE_FIELD[solver]] > 0)).sum()) for c in wall]
        assert max(pressed) >= ps.MIN_SPLIT, (solver, pressed)
    counts = {solver: [r.counts for c in ps.CASES[solver] for r in ps.references(*c)[1]] for solver in ("pcisph", "iisph")}
    assert any(c == (80, 0, 1) for c in counts["pcisph"]), counts["pcisph"]                        # on the cap
    assert any(c[0] <= 20 and c[2] == 0 for c in counts["pcisph"]), counts["pcisph"]               # well below it
    assert any(c[0] > 1 and c[1] == 0 and c[2] == 0 for c in counts["iisph"]), counts["iisph"]     # several iterations, left through the residual test
    assert any(c[1] == 1 for c in counts["iisph"]), counts["iisph"]                                # "trend to divergence"


def test_list_reuse_case_rebuilds_where_the_gpu_file_expects_it(legal):
    """REUSE_STEPS free-running wcsph steps at REUSE_VEL_AMP: by k_wcsph_force_rx's rule (a particle skin / 2 from where the lists were built flags
    a rebuild for the next step) the list builds fall where pressure_states.REUSE_BUILDS says, for the default skin and for 0.1 h -- some step runs
    on lists built earlier, some step follows a rebuild other than the first -- on both oracles and every schedule, with the deciding displacement
    at least 5 % off the threshold in every step (the participants differ by 1e-7).  The oracles stay within 1e-5 of each other in pos and vel,
    5e-5 in every field."""
    scene, seed, compression = ps.REUSE_CASE
    k, amp = ps.REUSE_STEPS, ps.REUSE_VEL_AMP
    assert k <= 8
    r32, r64 = ps.references(scene, seed, compression, k, amp)
    others = legal(scene, seed, compression, k, amp)
    h = 4.0 * float(ps.config(scene)["scene"]["particle_radius"])
    pos0 = ps.state(scene, seed, compression, amp)[0]
    assert (r64[0]["pressure"] > 0).sum() >= ps.MIN_SPLIT
    for skin, expected in ps.REUSE_BUILDS.items():
        for run in [r32, r64] + others:
            builds, margins = ps.predicted_builds(pos0, [r["pos"] for r in run], skin=float(skin or ps.VERLET_SKIN), h=h)
            assert builds == expected, (skin, builds)
            assert all(abs(m - 1.0) >= 0.05 for m in margins), (skin, margins)
        print("skin %s h: builds after each step %s, largest displacement / (skin / 2) %s" % (skin or ps.VERLET_SKIN, builds, " ".join("%.3f" % m for m in margins)))
        assert any(a == b for a, b in zip(expected, expected[1:]))                              # a step on lists built earlier
        assert any(b > a >= 1 for a, b in zip(expected, expected[1:]))                          # a rebuild other than the first
    for s in range(k):
        assert np.array_equal(r32[s].nbr, r64[s].nbr)
        for name, _ in ps.FIELDS["wcsph"]:
            e = float(ps.errors(r32[s][name], r64[s][name]).max())
            assert e < (1e-5 if name in ("pos", "vel") else CAP), (s + 1, name, e)
    failures, worst = bar(scene, seed, compression, k, others, r32, r64, amp)
    print("list reuse: worst seeded-schedule ratio %.2f (%s %s %s, n = %d)" % ((worst[6],) + worst[:2] + (worst[3], worst[2])))
    assert not failures, "\n".join(failures)


def test_comparator_rejects_1e4_in_the_wall_term_and_a_skin_pair():
    """What the envelope tests let through and this bar does not: the f32 oracle's own fields with the acceleration of the particles next to a box
    face off by 1e-4, and with the density of ten particles raised by 2e-5 (a skin pair
    beyond h that contributes a little)."""
    scene, seed, compression = ps.CASES["wcsph"][0]
    r32, r64 = ps.references(scene, seed, compression)
    wall = ps.wall_mask(scene, ps.state(scene, seed, compression)[0])
    for field, change in (("acc", lambda a: np.where(wall[:, None], a * np.float32(1 + 1e-4), a)),
                          ("rho", lambda a: np.concatenate([a[:10] * np.float32(1 + 2e-5), a[10:]]))):
        cand = ps.Result(r32[0])
        cand[field] = change(r32[0][field])
        cand.nbr = r32[0].nbr
        pool = ps.pool(scene)
        ps.add_step(pool, scene, seed, compression, 0, cand, r32[0], r64[0])
        failures = pool.report("perturbed %s:" % field)
        assert failures and all((" %s[" % field) in f for f in failures), failures
    pool = ps.pool(scene)
    ps.add_step(pool, scene, seed, compression, 0, r32[0], r32[0], r64[0])
    assert pool.report("f32 oracle as its own candidate:") == []
