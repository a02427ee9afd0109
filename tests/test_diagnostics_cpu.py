"""CPU suite of the run diagnostics: the yardstick of test_diagnostics_gpu.py on its own -- tests/diagnostics_ref.py on
oracle states, the fairness of its derived bound, the tie rule, the slot names against the header, and the runner's CSV writer on a fake
simulation.  No GPU, and the HIP library is not loaded."""
import math
import os
from fractions import Fraction

import numpy as np
import pytest

import diagnostics_ref as dr
import harness as h
import particle_flow as pf
from cfd_taichi_amd import _native as nat
from cfd_taichi_amd import run
from oracle import oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
TILTED = F([1.5, -9.0, 2.5])


@pytest.fixture(scope="module")
def states():
    """(pos, vel, rho, m) of the oracle after 0 and 10 steps of the tiny wall scene, dfsph and wcsph: the scenes the GPU suite sums"""
    out = {}
    for solver in ("dfsph", "wcsph"):
        cfg = pf.config(solver, "wall", 640)
        o = h.make_oracle(cfg)
        m = float(F(1000.0 * (2 * cfg["scene"]["particle_radius"]) ** 3))
        for steps in (0, 10):
            for _ in range(10 if steps else 0):
                h.oracle_step(o, solver)
            out[solver, steps] = (o.get(orc.F_POS).copy(), o.get(orc.F_VEL).copy(), o.get(orc.F_RHO).copy(), m)
        o.close()
    return out


def test_slot_names_are_the_headers():
    with open(os.path.join(ROOT, "include", "sph_mi355x.h")) as f:
        names = dr.header_slots(f.read())
    assert len(names) == 32
    assert names == tuple(nat.DIAG_SLOTS) == dr.SLOTS
    assert nat.DIAG_DTYPE.itemsize == 32 * 8 and nat.DIAG_DTYPE.names == names
    assert all(nat.DIAG_DTYPE.fields[n][1] == 8 * k for k, n in enumerate(names))
    for name in ("sph_diagnostics", "sph_diag_record", "sph_diag_read"):
        assert name in nat.EXPORTS and name in nat.OPTIONAL_EXPORTS


def test_reference_on_a_hand_made_state():
    pos = F([[1, 2, 3], [0.5, -1, 2], [4, 0, -2]])
    vel = F([[1, 0, 0], [0, 2, 0], [0, 0, -2]])
    rho = F([1000, 1004, 990])
    r = dr.row(pos, vel, rho, 0.125, F([0, -8, 0]), time=0.5, dt=0.25, step=3)
    assert (r["time"], r["dt"], r["step"], r["n"], r["mass"]) == (0.5, 0.25, 3.0, 3.0, 0.375)
    assert (r["momentum_x"], r["momentum_y"], r["momentum_z"]) == (0.125, 0.25, -0.25)
    # x cross v: (1,2,3)x(1,0,0) = (0,3,-2); (0.5,-1,2)x(0,2,0) = (-4,0,1); (4,0,-2)x(0,0,-2) = (0,8,0)
    assert (r["angular_momentum_x"], r["angular_momentum_y"], r["angular_momentum_z"]) == (-0.5, 1.375, -0.125)
    assert r["kinetic"] == 0.5 * 0.125 * 9 and r["potential"] == 0.125 * 8 * 1.0
    assert (r["com_x"], r["com_y"], r["com_z"]) == (5.5 / 3, 1 / 3, 1.0)
    assert (r["vmax"], r["vmax_id"]) == (2.0, 1.0)
    assert [r["pos_min_" + a] for a in "xyz"] == [0.5, -1, -2] and [r["pos_max_" + a] for a in "xyz"] == [4, 2, 3]
    assert (r["rho_min"], r["rho_max"], r["rho_mean"]) == (990.0, 1004.0, 998.0)
    assert all(r[k] == 0.0 for k in dr.SLOTS[27:])
    none = dr.row(pos, vel, None, 0.125, F([0, -8, 0]))
    assert all(math.isnan(none[k]) for k in dr.RHO)


def test_reference_sums_are_exact_on_oracle_states(states):
    """exact_sum against plain rational arithmetic, every summed slot, on a state that has moved"""
    pos, vel, rho, m = states["dfsph", 10]
    assert np.abs(vel).max() > 0
    r = dr.row(pos, vel, rho, m, TILTED)
    for name, cols in dr.terms(pos, vel, TILTED).items():
        exact = sum((Fraction(float(v)) for c in cols for v in c), Fraction(0)) * dr.scale(name, m, len(pos))
        assert r[name] == float(exact), name
    assert r["rho_mean"] == float(sum((Fraction(float(v)) for v in rho), Fraction(0)) / len(rho))
    assert r["mass"] == len(pos) * m


def sequential(a):
    return float(np.add.accumulate(np.asarray(a, dtype=np.float64))[-1])


def chunked(a, width):
    """sequential sums of runs of `width`, then the runs' sums in order: the shape of a wave / workgroup reduction"""
    return sequential([sequential(a[k:k + width]) for k in range(0, len(a), width)])


@pytest.mark.parametrize("key", [("dfsph", 0), ("dfsph", 10), ("wcsph", 10)], ids=lambda k: "%s-%d" % k)
def test_the_bound_is_fair(states, key):
    """f64 summation of the reference's own terms in random orders and in chunked orders of 64 and 256 stays within bounds()"""
    pos, vel, rho, m = states[key]
    n = len(pos)
    ref, bnd = dr.row(pos, vel, rho, m, TILTED), dr.bounds(pos, vel, rho, m, TILTED)
    t = dr.device_terms(pos, vel, TILTED)
    t["rho_mean"] = rho.astype(np.float64)
    rng = np.random.default_rng(5)
    worst = 0.0
    for name, a in t.items():
        s = float(dr.scale(name, m, n))
        orders = [a, a[::-1]] + [a[rng.permutation(n)] for _ in range(6)]
        sums = [sequential(o) for o in orders] + [chunked(o, w) for o in orders[:4] for w in (64, 256)] + [float(np.sum(a))]
        for v in sums:
            got = v / n if s == 1.0 / n else s * v
            err = abs(got - ref[name])
            assert err <= bnd[name], (name, got, ref[name], err, bnd[name])
            worst = max(worst, err / bnd[name]) if bnd[name] else worst
    assert worst < 1.0
    assert bnd["mass"] >= abs(n * m - ref["mass"])


def test_tie_rule():
    vel = np.zeros((70, 3), dtype=F)
    assert dr.fastest(vel) == (F(0), 0)                        # all at rest: the lowest id
    vel[41] = [3, 0, 4]
    assert dr.fastest(vel) == (F(5), 41)
    vel[17] = [0, -5, 0]; vel[66] = [4, 3, 0]                  # the same f32 speed three times
    assert dr.fastest(vel) == (F(5), 17)
    vel[69] = [0, 0, np.nextafter(F(5), F(6))]
    assert dr.fastest(vel) == (np.nextafter(F(5), F(6)), 69)


class FakeSim:
    """what run.drain_diag needs of a simulation: a ring of `rows` rows that loses the oldest"""

    def __init__(self, rows):
        self.rows, self.pending, self.total, self.seen = rows, [], 0, 0

    def step(self, k):
        for _ in range(k):
            self.total += 1
            r = np.zeros(1, dtype=nat.DIAG_DTYPE)
            r["time"], r["step"], r["n"], r["com_x"] = 1e-3 * self.total, self.total, 640, 0.1 + 1.0 / 3 * self.total
            self.pending = (self.pending + [r])[-self.rows:]

    def diagnostics_log(self):
        out = np.concatenate(self.pending) if self.pending else np.zeros(0, dtype=nat.DIAG_DTYPE)
        self.seen += len(out)
        self.pending = []
        return out, self.total - self.seen


def test_csv_writer_on_a_fake_simulation(tmp_path):
    sim, chunks, lost = FakeSim(rows=4), [], 0
    for frame in (3, 0, 6, 2):                                 # a frame without rows; a frame that overruns the ring by two
        sim.step(frame)
        lost = run.drain_diag(sim, chunks, lost)
    assert lost == 2 and sum(len(c) for c in chunks) == 9
    path = str(tmp_path / "diag.csv")
    run.write_diag_csv(path, chunks)
    with open(path) as f:
        lines = f.read().splitlines()
    assert lines[0].split(",") == list(nat.DIAG_SLOTS) and len(lines) == 10
    table = np.array([[float(v) for v in line.split(",")] for line in lines[1:]])
    assert table.shape == (9, 32)
    assert list(table[:, 2]) == [1, 2, 3, 6, 7, 8, 9, 10, 11]
    assert np.array_equal(table[:, 13], [0.1 + 1.0 / 3 * k for k in table[:, 2]])      # %.17g: the f64 comes back bit for bit
    assert (table[:, 3] == 640).all() and (np.diff(table[:, 0]) > 0).all()
