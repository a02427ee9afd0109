"""GPU suite: PBF at the edges (tests/pbf_edge_states.py; tests/test_pbf_edge_states_cpu.py shows the inputs fair on the two oracles alone).

What tests/test_edge_cases_gpu.py and test_particles_outside_the_grid ask of the four older solvers, asked of the solver that walks its 27 cells
itself (k_pbf_xsph: batches of four, its own Morton slot look-up) and has a second set of pair bodies (RX, csrc/sph_pbf_kernels.h).  One oracle run
per input, compared with the four handles of tests/test_pbf_relaxed_gpu.py's VARIANTS (quad or plain kernels, linear or Morton cells); every knob that
was set is asserted to appear in sim.overrides().

  exact     rho, pbf_lambda, delta_pos, pos, vel bit for bit against the f32 oracle after EVERY step: ragged 25 steps, coincident 5, a fluid
            particle on a wall particle 5, spray and clump 6 (F_NBR_COUNT.max() >= 39 after build_neighbors), outside the grid 5.  (sph_step_pbf
            returns no SphStepStats, so there is no `lost` on the handle's side to compare: the count is compared between the two oracles on the
            CPU, and a particle that one side lists and the other loses shows in rho.)
  relaxed   by the method of tests/test_pbf_relaxed_gpu.py -- q50 / q99 / max of the per-particle error against the f64 oracle over the three
            populations <= MARGIN x the f32 oracle's own + FLOOR, equal `lambda != 0` and clamped sets -- on coincident (3 steps), spray and clump
            (3 steps) and the 73 ragged particles (1 step): the windows in which the CPU file shows the sets equal and the yardstick below its cap.
            The relaxed handle reports SPH_S_ARITH_RELAXED = 1 and its rho differs from the exact handle's in at least one bit.  For the two
            particles of the coincident pair (a) the bound on lambda is asserted BY INDEX as well: |lambda_i - f64_i| / max |f64| <= MARGIN x the f32
            oracle's max-norm error + FLOOR.  A coincident pair contributes 0 to lambda's sum of squared gradients in the reference (its q > 0
            gate); kernels that added the limit r -> 0+ there, (45 / (pi h^4 rho0))^2, halved both particles' lambda (-9.97e-6 for -2.18e-5) and
            missed this bound by a factor of 1e5 -- the kernels of the commit before this file, all eight cases, on one MI355X:
                coincident pbf_tiny_clamp seed 1 step 1: pbf_lambda[all] max: 5.423e-01 > 4 x 9.598e-07 + 1.2e-07 (ratio 547997.20, n = 640)
                coincident pbf_tiny_clamp seed 1 step 1 pbf_lambda of particle 300 of the coincident pair (a): 5.423e-01 > 4 x 9.598e-07 + 1.2e-07
            With pbf_sq_rx's select the worst ratios are those of the smooth states: lambda 1.45, rho 1.19, delta_pos 1.23, pos 0.96, vel 1.14
            (coincident); rho 1.29 (spray and clump); lambda 1.21 (73 particles).
            The particle on a wall particle gets no relaxed check: the f64 oracle builds its wall lattice in f64 and does not agree that the pair is
            coincident (the two oracles' lambda differ by 4.6 max |lambda| there): no fair yardstick."""
import numpy as np
import pytest

import pbf_edge_states as pe
import pbf_states as pb
from cfd_taichi_amd import _native as nat
from harness import same_values
from test_pbf_relaxed_gpu import VARIANTS, handles, held, report

pytestmark = pytest.mark.gpu

RAGGED = [(sc, w) for sc in pe.SCENES for w in pe.RAGGED]
RAGGED_IDS = ["%s-N%d" % (sc, pe.RAGGED[w]) for sc, w in RAGGED]
SEEDED = [(sc, seed) for sc in pe.SCENES for seed in pe.SEEDS]
SEEDED_IDS = ["%s-seed%d" % c for c in SEEDED]


def lockstep(inp, steps, knobs, monkeypatch, before=None):
    """the exact handle under `knobs` against the f32 oracle's run of the same input, every field after every step"""
    r32 = pe.references(inp, steps)[0]
    rx, ex = handles(inp.cfg, VARIANTS[knobs], monkeypatch)
    rx.close()
    try:
        assert ex.n_fluid == len(inp.pos) and ex.scalar(nat.S_ARITH_RELAXED) == 0.0
        pe.upload(ex, inp)
        if before:
            before(ex)
        for s in range(steps):
            ex.step_pbf(1)
            got = pb.snapshot(ex.download)
            for name, _ in pb.FIELDS:
                same_values(got[name], r32[s][name], "%s, %s: %s after step %d, exact handle and f32 oracle" % (inp.label, knobs, name, s + 1))
    finally:
        ex.close()
    return r32


@pytest.mark.parametrize("knobs", VARIANTS)
@pytest.mark.parametrize("scene,water", RAGGED, ids=RAGGED_IDS)
def test_ragged_particle_counts(scene, water, knobs, monkeypatch):
    """1, 6, 73 and 82 particles: below one quad workgroup's 64, just above it, far below a plain workgroup's 256"""
    inp = pe.ragged(scene, water)
    assert len(inp.pos) == pe.RAGGED[water]
    lockstep(inp, 25, knobs, monkeypatch)


@pytest.mark.parametrize("knobs", VARIANTS)
@pytest.mark.parametrize("scene,seed", SEEDED, ids=SEEDED_IDS)
def test_coincident_particles_and_cell_faces(scene, seed, knobs, monkeypatch):
    inp = pe.coincident(scene, seed)
    r32 = lockstep(inp, 5, knobs, monkeypatch)
    i, j = inp.marks["a"]
    assert r32[0]["pbf_lambda"][i] != 0 and r32[0]["pbf_lambda"][j] != 0
    b = inp.marks["b"]
    assert not np.array_equal(r32[0]["pos"][b[0]], r32[0]["pos"][b[1]]), "pair (b) did not separate: its xsph term was not seen"


@pytest.mark.parametrize("knobs", VARIANTS)
@pytest.mark.parametrize("seed", pe.SEEDS)
def test_fluid_particle_on_a_wall_particle(seed, knobs, monkeypatch):
    inp = pe.on_a_wall_particle(seed)
    i, w = inp.marks["w"]

    def walls_agree(sim):
        wall = sim.download(nat.F_WALL_POS, nat.SPECIES_WALL)
        same_values(wall, inp.wall, "wall positions, handle and f32 oracle")
        assert np.array_equal(wall[w], inp.pos[i])
    r32 = lockstep(inp, 5, knobs, monkeypatch, before=walls_agree)
    assert r32[0]["pbf_lambda"][i] != 0


@pytest.mark.parametrize("knobs", VARIANTS)
@pytest.mark.parametrize("scene", pe.SCENES)
def test_spray_and_clump(scene, knobs, monkeypatch):
    """k_pbf_xsph's batches of four over cells of 1 and of 40 or 41 particles (j == i in mid-batch), and lists of 39 and more"""
    inp = pe.spray_and_clump(scene)

    def clump_is_there(sim):
        sim.build_neighbors()
        assert sim.download(nat.F_NBR_COUNT).max() >= 39
    r32 = lockstep(inp, 6, knobs, monkeypatch, before=clump_is_there)
    assert (r32[0]["pbf_lambda"][inp.marks["clump"]] != 0).all()


@pytest.mark.parametrize("knobs", VARIANTS)
@pytest.mark.parametrize("scene,seed", SEEDED, ids=SEEDED_IDS)
def test_particles_outside_the_grid(scene, seed, knobs, monkeypatch):
    """48 particles beyond the six faces: some in the cell margin and in the lists, some in wrapped cells, some in no cell at all"""
    inp = pe.outside(scene, seed)
    r32 = lockstep(inp, 5, knobs, monkeypatch)
    assert max(r["lost"] for r in r32) >= 1


# ---- the relaxed kernels -----------------------------------------------------------------------------------------------------------------------

def relaxed(inp, steps, knobs, monkeypatch, ratios):
    """failures of the relaxed handle under `knobs` over `steps` steps of one input; the exact handle next to it must be the f32 oracle"""
    r32, r64 = pe.references(inp, steps)
    rx, ex = handles(inp.cfg, VARIANTS[knobs], monkeypatch)
    try:
        pe.upload(rx, inp); pe.upload(ex, inp)
        got, twin = [], []
        for _ in range(steps):
            rx.step_pbf(1); ex.step_pbf(1)
            got.append(pb.snapshot(rx.download)); twin.append(pb.snapshot(ex.download))
        assert rx.scalar(nat.S_ARITH_RELAXED) == 1.0 and ex.scalar(nat.S_ARITH_RELAXED) == 0.0
    finally:
        rx.close(); ex.close()
    assert not np.array_equal(got[0]["rho"], twin[0]["rho"]), "the relaxed handle gave the exact handle's rho: it ran the exact sweeps"
    failures = []
    for s in range(steps):
        label = "%s step %d:" % (inp.label, s + 1)
        for name, _ in pb.FIELDS:
            same_values(twin[s][name], r32[s][name], "%s %s, exact handle and f32 oracle" % (label, name))
        try:
            failures += held(label, inp.cfg, inp.pos, got[s], r32[s], r64[s], ratios)
        except AssertionError as e:        # a discrete set or a non-finite value: reported with the bounds of the other steps, not instead of them
            failures.append(str(e).splitlines()[0])
    return failures, got


@pytest.mark.parametrize("knobs", VARIANTS)
@pytest.mark.parametrize("scene", pe.SCENES)
def test_relaxed_coincident_particles(scene, knobs, monkeypatch):
    failures, ratios = [], {}
    for seed in pe.SEEDS:
        inp = pe.coincident(scene, seed)
        f, got = relaxed(inp, 3, knobs, monkeypatch, ratios)
        failures += f
        r32, r64 = pe.references(inp, 3)
        for s in range(3):
            ref = r64[s]["pbf_lambda"]
            e32, e = pb.errors(r32[s]["pbf_lambda"], ref), pb.errors(got[s]["pbf_lambda"], ref)
            bound = pb.MARGIN * float(e32.max()) + pb.FLOOR
            for i in inp.marks["a"]:           # the coincident pair itself, by index
                print("%s step %d: lambda of particle %d of pair (a): relaxed %.6e, f64 %.6e, error %.3e of max |lambda|, bound %.3e" % (
                    inp.label, s + 1, i, got[s]["pbf_lambda"][i], ref[i], e[i], bound))
                if not e[i] <= bound:
                    failures.append("%s step %d pbf_lambda of particle %d of the coincident pair (a): %.3e > %g x %.3e + %.1e" % (
                        inp.label, s + 1, i, e[i], pb.MARGIN, float(e32.max()), pb.FLOOR))
    report("coincident %s %s:" % (scene, knobs), ratios)
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("knobs", VARIANTS)
@pytest.mark.parametrize("scene", pe.SCENES)
def test_relaxed_spray_and_clump(scene, knobs, monkeypatch):
    ratios = {}
    failures, _ = relaxed(pe.spray_and_clump(scene), 3, knobs, monkeypatch, ratios)
    report("spray and clump %s %s:" % (scene, knobs), ratios)
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("knobs", VARIANTS)
@pytest.mark.parametrize("scene", pe.SCENES)
def test_relaxed_ragged_73(scene, knobs, monkeypatch):
    inp = pe.ragged(scene, next(w for w, n in pe.RAGGED.items() if n == 73))
    ratios = {}
    failures, _ = relaxed(inp, 1, knobs, monkeypatch, ratios)
    report("%s %s:" % (inp.label, knobs), ratios)
    assert not failures, "\n".join(failures)
