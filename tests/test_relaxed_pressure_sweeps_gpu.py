"""GPU suite: the relaxed PCISPH and IISPH steps (KF<true>, csrc/sph_device.h, in k_pci_ext / k_pci_predict_rho / k_pci_press and k_ii_advect /
k_ii_rho_adv / k_ii_dij / k_ii_update_p, with the zero_press / zero_dij tile skipping of csrc/sph_host_pressure.h) against the f64 oracle, step
by step.

tests/test_relaxed_gpu.py holds these handles to max(1e-5, 3 x a legal schedule) after dozens of free-running steps with iteration counts within
max(2, 10 %): a wrong constant in one branch of the kernel function, a missing clamp at q > 1 (pcisph evaluates list pairs at PREDICTED positions)
or a sign slip the pressure loop irons out fit inside.  Here four participants -- the relaxed handle, the exact handle, the f32 oracle, the f64
oracle -- run three steps from one uploaded state of tests/pressure_states.py (one step from the state, two free-running, each carrying its own
p_past), on which tests/test_pressure_states_cpu.py has shown the reference alone to be fair.  In this order:
  1. the relaxed handle reports SPH_S_ARITH_RELAXED = 1, the exact one 0, and some field of the two differs in at least one bit;
  2. iteration count, exit flag (iisph: left on "trend to divergence"), cap flag and the neighbour counts of the step's input positions are equal
     on all four, at every step;
  3. the exact handle equals the f32 oracle bit for bit on every field at every step;
  4. on the clamp scenes the relaxed handle's coordinates on a clamp plane are the f64 oracle's;
  5. per field and population (all particles, within a support radius of a box face / not, each class of the neighbour count mod 8 pooled over
     the steps, f64 pressure > 0 / = 0 where both sides hold 32 particles), q50, q99 and max of the per-particle error against the f64 oracle are
     <= 4 x the f32 oracle's own + 2 x 2^-24;
  6. every field finite, no particle lost.
Why 4: tests/test_relaxed_sweeps_gpu.py -- a factor 2 for v_rsq_f32 / v_rcp_f32 and the FMAs, a factor 2 for regrouped sums; KF<true> is the same
pair arithmetic.  Seeded legal schedules of the f32 oracle reach 3.45 on these cases (the CPU test prints it).  The measured ratios are printed
per case; DESIGN.md section 4b holds the table.

Handle paths: morton (SPH_CELL_ORDER=morton: staged sweeps), plain (SPH_QUAD=0: one lane per particle) and, on the 5 880-particle scenes, mixed
(morton with SPH_STAGE_CAP=300: staged and unstaged workgroups side by side)."""
import numpy as np
import pytest

import coupled_scenes
import pressure_states as ps
from cfd_taichi_amd import _native as nat
from harness import same_values
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

PATHS = {
    "morton": {"SPH_CELL_ORDER": "morton"},
    "plain": {"SPH_QUAD": "0"},
    "mixed": {"SPH_CELL_ORDER": "morton", "SPH_STAGE_CAP": "300"},
    "quad": {},
}
CASES = [(solver, path) + case for solver in ("pcisph", "iisph") for case in ps.CASES[solver] for path in ("morton", "plain", "mixed")
         if path != "mixed" or case[0] in ps.LARGE]


@pytest.mark.parametrize("solver,path,scene,seed,compression", CASES, ids=["%s-%s-%d-%g" % c[1:] for c in CASES])
def test_relaxed_pressure_steps_against_the_f64_oracle(solver, path, scene, seed, compression, monkeypatch):
    label = "%s %s seed %d %g:" % (path, scene, seed, compression)
    rx, ex = ps.handles(nat, ps.config(scene), PATHS[path], monkeypatch)
    try:
        a, b = ps.run_handle(rx, scene, seed, compression, ps.STEPS), ps.run_handle(ex, scene, seed, compression, ps.STEPS)
        assert rx.scalar(nat.S_ARITH_RELAXED) == 1.0 and ex.scalar(nat.S_ARITH_RELAXED) == 0.0
    finally:
        rx.close(); ex.close()
    assert any(not np.array_equal(a[0][name], b[0][name]) for name, _ in ps.FIELDS[solver]), "the relaxed handle gave the exact handle's bits: it ran the exact sweeps"
    r32, r64 = ps.references(scene, seed, compression)
    pool = ps.pool(scene)
    ps.check_steps(label, scene, seed, compression, a, b, r32, r64, pool)
    failures = pool.report(label)
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("solver", ["pcisph", "iisph"])
def test_a_relaxed_request_the_quad_sweeps_do_not_cover_runs_exact(solver, monkeypatch):
    """relaxed_pressure() (csrc/sph_host_rigid.h) leaves the quad sweeps of small scenes exact: a default handle of the 640-particle scene asked
    for arith = relaxed reports SPH_S_ARITH_RELAXED = 0 and IS the f32 oracle after the three steps -- not half relaxed"""
    scene, seed, compression = ps.CASES[solver][0]
    rx, _ = ps.handles(nat, ps.config(scene), PATHS["quad"], monkeypatch, exact=False)
    try:
        assert rx.overrides() == [], rx.overrides()
        a = ps.run_handle(rx, scene, seed, compression, ps.STEPS)
        assert rx.scalar(nat.S_ARITH_RELAXED) == 0.0
    finally:
        rx.close()
    r32, _ = ps.references(scene, seed, compression)
    for s in range(ps.STEPS):
        assert a[s].counts == r32[s].counts and np.array_equal(a[s].nbr, r32[s].nbr), (s, a[s].counts, r32[s].counts)
        for name, _ in ps.FIELDS[solver]:
            same_values(a[s][name], r32[s][name], "%s step %d %s, handle and f32 oracle" % (scene, s + 1, name))


def test_a_relaxed_request_next_to_a_coupled_body_runs_exact(monkeypatch):
    """... and so do the RIGID instantiations: a pcisph handle with a coupled body (tests/coupled_scenes.py: 640 fluid particles, 168 samples in
    the water's support radius) on the plain path, which without the body would qualify.  The water starts from the compressed state of the
    first pcisph case -- the scene's fluid is dfsph_tiny_wall's --, so that it carries pressure and pushes the body from step 1."""
    cfg = coupled_scenes.coupled("pcisph")
    rg = coupled_scenes.rigid(cfg)
    rx, _ = ps.handles(nat, cfg, PATHS["plain"], monkeypatch, rigid=rg, exact=False)
    o = orc.Oracle(cfg, num_threads=8, rigid=rg)
    pos, vel = ps.state(*ps.CASES["pcisph"][0])
    rx.upload(nat.F_POS, pos); rx.upload(nat.F_VEL, vel)
    o.set(orc.F_POS, pos); o.set(orc.F_VEL, vel)
    felt = 0.0
    try:
        for s in range(ps.STEPS):
            st = rx.step_pcisph(1)
            capped = o.step_pcisph(1)
            assert (st.n_dens, st.capped, st.lost) == (o.last_stats.n_dens, capped, 0), s
            for name, f in ps.FIELDS["pcisph"]:
                same_values(rx.download(f), o.get(f), "coupled pcisph step %d %s, handle and f32 oracle" % (s + 1, name))
            force = o.get(orc.F_RIGID_FORCE)
            same_values(rx.download(nat.F_RIGID_FORCE, nat.SPECIES_RIGID), force, "coupled pcisph step %d, force on the samples" % (s + 1))
            felt += float(np.abs(force).sum())
            rx.rigid_step(); o.rigid_step()
        assert felt > 0, "the body never felt the fluid: the RIGID sweeps did not run"
        assert rx.scalar(nat.S_ARITH_RELAXED) == 0.0
    finally:
        rx.close(); o.close()
