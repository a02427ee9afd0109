"""Loads on walls and geometry, the part that needs no GPU: the yardstick tests/wall_load_ref.py itself.

  * fairness: in every compared step of the pressed state at least 5 plate samples and at least 30 box samples carry a nonzero f_b, on every
    solver -- asserted on the restatement, not measured on the library;
  * action and reaction: sum_b f_b over ALL wall samples equals - sum_i (the wall force the restatement applies to particle i), the same f32 pair
    terms summed in two orders, within a bound derived from sum |pair terms|.  This pins the definition to the physics, and for pcisph shows the
    deviation from the body's rule (one event behind the loop) to be the right one;
  * the bound the GPU suite holds the device's f64 reduction to, (n + 8) 2^-53 sum |t_i|, is fair under random and chunked orders;
  * the Python layer: names against the header, `scene.loads` parsing, the runner's CSV writer on a fake simulation."""
import copy
import math
import os

import numpy as np
import pytest

import wall_load_ref as wl
from cfd_taichi_amd import _native as nat
from cfd_taichi_amd import geometry, run, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOLVERS = ("wcsph", "dfsph", "pcisph", "iisph")
STEPS = 6


@pytest.mark.parametrize("solver", SOLVERS)
def test_the_pressed_state_is_fair(solver):
    ref = wl.run(solver, STEPS)
    assert len(ref["state"]["pos"]) == 480 and len(ref["wall_pos"]) == 2510 and ref["plate"] == (2402, 108)
    for k, st in enumerate(ref["steps"], 1):
        plate, box = wl.fair_counts(st["f"])
        print("%s step %d: %d plate and %d box samples with a nonzero f_b, %d events, fullest rows %d (particle) / %d (sample)"
              % (solver, k, plate, box, st["events"], st["kf"], st["ks"]))
        assert plate >= 5 and box >= 30, (solver, k, plate, box)
        assert np.isfinite(st["f"]).all()
        assert st["events"] == (st["n_dens"] if solver == "dfsph" else 1)


def test_every_compared_run_is_fair():
    """the condition on every restatement run the GPU suite compares against (wall_load_ref.compared_runs): the six-step runs, dfsph from another
    delta_time, the edge groups, a group added and removed, particles removed and added -- every compared step of each"""
    runs = wl.compared_runs()
    assert len(runs) == 10
    for name, fs in runs:
        counts = [wl.fair_counts(f) for f in fs]
        print("%s: (plate, box) samples with a nonzero f_b per step %s" % (name, counts))
        assert all(p >= 5 and b >= 30 for p, b in counts), (name, counts)
        assert all(np.isfinite(f).all() for f in fs), name


@pytest.mark.parametrize("solver", SOLVERS)
def test_action_and_reaction(solver):
    """Both sides are sums of the same pair terms t_ib, each rounded to f32 a little differently (where rho_0 and m multiply): at most 8 roundings
    per term between them, then kf (the fullest wall row of a particle) resp. ks (of a sample) f32 additions; the sums over particles / samples
    are taken exactly here.  |sum_b f_b + sum_i F_i| <= (kf + ks + 8) 2^-24 sum |t_ib| per component, and sum |t_ib| is bounded by the total over
    components that the yardstick records."""
    for k, st in enumerate(wl.run(solver, STEPS)["steps"], 1):
        walls = np.array([math.fsum(st["f"][:, a].astype(np.float64)) for a in range(3)])
        fluid = np.array([math.fsum(st["fluid"][:, a]) for a in range(3)])
        bound = (st["kf"] + st["ks"] + 8) * 2.0 ** -24 * st["abs"]
        print("%s step %d: walls %s fluid %s, |sum| %.3e, bound %.3e" % (solver, k, walls, fluid, np.abs(walls + fluid).max(), bound))
        assert np.abs(walls).max() > 1e3 * bound, "nothing to compare"
        assert (np.abs(walls + fluid) <= bound).all(), (solver, k, walls, fluid, bound)


def test_the_body_rule_would_overcount_pcisph():
    """the reference's rule for a body -- a deposit in every iteration from the accumulating press_iter -- summed over a step is several times what
    the fluid receives; the yardstick's one event behind the loop is not"""
    class BodyRule(wl.LoadSolver):
        def update_press_force(self):
            super().update_press_force()
            V, rho_2, p = self.sc.wall_vol, self.rho * self.rho, self.press_iter
            kept = (self.f_b, self.abs_terms, self.events)
            self.f_b = np.zeros_like(self.f_b)
            self._deposit(lambda i: ((V * self.rho_0 * p[i])[:, None] * self._grad(i) / rho_2[i][:, None]) * self.m)
            self.every = self.every + self.f_b
            self.f_b, self.abs_terms, self.events = kept

    _, s, _, _ = wl.pressed_solver("pcisph", BodyRule)
    s.every = 0
    with np.errstate(all="ignore"):
        s.step()
    assert s.n_dens >= 3
    once, every = np.abs(s.f_b[:, 0]).sum(), np.abs(s.every[:, 0]).sum()
    print("pcisph, %d iterations: sum |f_x| %.4g by the one event, %.4g by a deposit per iteration" % (s.n_dens, once, every))
    assert every > 1.5 * once > 0


def sequential(a):
    return float(np.add.accumulate(np.asarray(a, dtype=np.float64))[-1])


def chunked(a, width):
    """sequential sums of runs of `width`, then the runs' sums in order: the shape of a wave / workgroup reduction"""
    return sequential([sequential(a[k:k + width]) for k in range(0, len(a), width)])


@pytest.mark.parametrize("solver", ["wcsph", "dfsph"])
@pytest.mark.parametrize("about", [(0.0, 0.0, 0.0), wl.PLATE_CENTRE], ids=["origin", "plate-centre"])
def test_the_bound_is_fair(solver, about):
    """f64 summation of the device's terms in random orders and in chunked orders of 64 and 256 stays within load_bound of the exact sums"""
    ref = wl.run(solver, STEPS)
    rng = np.random.default_rng(5)
    worst = 0.0
    for first, count in (ref["plate"], ref["box"]):
        x, f = ref["wall_pos"][first:first + count], ref["steps"][2]["f"][first:first + count]
        (F, T), (bF, bT) = wl.exact_load(x, f, about), wl.load_bound(x, f, about)
        ft, tt = wl.load_terms(x, f, about)
        for a in range(3):
            for terms, exact, bnd in ((ft[:, a], F[a], bF[a]), (tt[:, a, 0] + tt[:, a, 1], T[a], bT[a])):
                orders = [terms, terms[::-1]] + [terms[rng.permutation(count)] for _ in range(6)]
                for v in [sequential(o) for o in orders] + [chunked(o, w) for o in orders[:4] for w in (64, 256)]:
                    assert abs(v - exact) <= bnd, (solver, about, a, v, exact, bnd)
                    worst = max(worst, abs(v - exact) / bnd) if bnd else worst
    assert worst < 1.0


def test_exact_load_on_a_hand_made_state():
    x = np.float32([[1, 2, 3], [0.5, -1, 2]])
    f = np.float32([[1, 0, 0], [0, 2, 0]])
    F, T = wl.exact_load(x, f)
    assert F.tolist() == [1.0, 2.0, 0.0] and T.tolist() == [-4.0, 3.0, -1.0]            # (0, 3, -2) + (-4, 0, 1)
    F, T = wl.exact_load(x, f, (1.0, 2.0, 3.0))
    assert T.tolist() == [2.0, 0.0, -1.0]                                                # (-0.5, -3, -1) x (0, 2, 0)
    bF, bT = wl.load_bound(x, f)
    assert bF.tolist() == [10 * 2.0 ** -53 * 1, 10 * 2.0 ** -53 * 2, 0.0] and bT[0] == 10 * 2.0 ** -53 * 4


# ---- the Python layer ------------------------------------------------------------------------------------------------------------------------
def test_names_against_the_header():
    with open(os.path.join(ROOT, "include", "sph_mi355x.h")) as f:
        header = f.read()
    for name in ("sph_wall_load_select", "sph_wall_load_get", "sph_wall_load_impulse", "sph_wall_load_forces"):
        assert "int %s(SphHandle *h" % name in header and name in nat.EXPORTS and name in nat.OPTIONAL_EXPORTS
    assert "#define SPH_ABI_VERSION %d" % nat.ABI_VERSION in header
    for method in ("measure_loads", "wall_load", "wall_impulse", "wall_forces"):
        assert callable(getattr(nat.Simulation, method))


def test_scene_loads_parsing():
    cfg = scenes.get("dam_pillars_dfsph")
    assert geometry.config_loads(cfg) == ["pillar_0", "pillar_1", "pillar_2"] and geometry.config_loads(scenes.get("dam_gate_wcsph")) == ["gate"]
    assert geometry.config_loads(scenes.get("pbf_step_pbf")) == [] and geometry.config_loads(scenes.get("dfsph_tiny_wall")) == []
    ok = copy.deepcopy(cfg)
    ok["scene"]["loads"] = ["box", "pillar_2"]
    assert geometry.config_loads(ok) == ["box", "pillar_2"]
    for bad in ("gate", ["pillar_9"], ["box", "box"], [0], {"box": 1}):
        c = copy.deepcopy(cfg)
        c["scene"]["loads"] = bad
        with pytest.raises(ValueError):
            geometry.config_loads(c)
    plain = copy.deepcopy(scenes.get("dfsph_tiny_wall"))
    plain["scene"]["loads"] = ["box"]
    assert geometry.config_loads(plain) == ["box"]

    class Sim:
        calls = []

        def measure_loads(self, groups):
            self.calls.append(list(groups))

    sim = Sim()
    assert geometry.apply_loads(sim, ok) == ["box", "pillar_2"] and sim.calls == [["box", "pillar_2"]]
    assert geometry.apply_loads(sim, scenes.get("dfsph_tiny_wall")) == [] and len(sim.calls) == 1


def test_scene_loads_is_skipped_where_loads_cannot_be_measured(capsys):
    """a handle that answers SPH_E_STATE (slab, relaxed, pbf, a library without the entry points) runs the scene as it always did: one printed line,
    nothing measured; any other refusal is the config's mistake and is raised"""
    cfg = scenes.get("dam_gate_wcsph")

    class Sim:
        def __init__(self, code):
            self.code = code

        def measure_loads(self, groups):
            raise nat.SphError(self.code, "not here")

    assert geometry.apply_loads(Sim(nat.SPH_E_STATE), cfg) == []
    out = capsys.readouterr().out
    assert out.count("\n") == 1 and "scene.loads skipped" in out and "not here" in out
    with pytest.raises(nat.SphError):
        geometry.apply_loads(Sim(nat.SPH_E_INVALID), cfg)


class FakeSim:
    """what run.load_rows and run.write_geometry_ply read of a Simulation"""
    geometry_groups = {"gate": 1}
    measured_groups = [0, 1]
    n_wall = 5

    def __init__(self):
        self.resets = []

    def wall_impulse(self, group, about=None, reset=True):
        self.resets.append((group, reset))
        return np.array([2.0, 0.0, -4.0]) * (group + 1), np.array([0.5, 0.25, 0.0]), 0.5 if group else 0.0

    def wall_load(self, group=None, about=None):
        return np.array([1.0, 2.0, 3.0 + group]), np.zeros(3)

    def wall_forces(self, group):
        return np.full((3 if group == 0 else 2, 3), 1.5 + group, dtype=np.float32)

    def geometry(self):
        return [(1, 3, 2)]

    def download(self, field, species):
        return np.arange(15, dtype=np.float32).reshape(5, 3)


def test_load_csv_writer_on_a_fake_simulation(tmp_path):
    sim = FakeSim()
    rows = run.load_rows(sim, 1, 0.25) + run.load_rows(sim, 2, 0.5)
    assert sim.resets == [(0, True), (1, True)] * 2 and len(rows) == 4
    assert rows[1][:4] == (1, 0.25, "gate", 0.5) and rows[1][4:10] == (8.0, 0.0, -16.0, 1.0, 0.5, 0.0) and rows[1][10:] == (1.0, 2.0, 4.0)
    assert rows[0][2] == "box" and all(math.isnan(v) for v in rows[0][4:10])            # a window of no seconds
    path = str(tmp_path / "loads.csv")
    run.write_load_csv(path, rows)
    lines = open(path).read().splitlines()
    assert lines[0] == ",".join(run.LOAD_COLUMNS) and len(run.LOAD_COLUMNS) == 13 and len(lines) == 5
    assert lines[2] == "1,0.25,gate,0.5,8,0,-16,1,0.5,0,1,2,4"
    assert lines[3].startswith("2,0.5,box,0,nan,")


def test_geometry_ply_gains_force_columns(tmp_path):
    path = str(tmp_path / "g.ply")
    run.write_geometry_ply(path, FakeSim())
    head, body = open(path).read().split("end_header\n")
    assert head.splitlines()[-3:] == ["property float fx", "property float fy", "property float fz"] and "property int group" in head
    rows = [r.split() for r in body.splitlines()]
    assert [r[3] for r in rows] == ["0", "0", "0", "1", "1"] and [r[4] for r in rows] == ["1.5"] * 3 + ["2.5"] * 2
    sim = FakeSim()
    sim.measured_groups = []
    run.write_geometry_ply(path, sim)
    assert "fx" not in open(path).read()
