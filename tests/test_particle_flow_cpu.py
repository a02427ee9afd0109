"""CPU suite of the inlets and sinks (tests/particle_flow.py): the lattice counts and the pcisph precondition on the oracle alone, the
host-side Emitter / Sink against a simulation with a scripted clock, the config key."""
import math

import numpy as np
import pytest

import harness as h
import particle_flow as pf
from cfd_taichi_amd import _native as nat
from cfd_taichi_amd import emitter, scenes


@pytest.mark.parametrize("walls", ["wall", "clamp"])
def test_lattice_counts_and_prefix(walls):
    """640, 704, 832 particles, and the tall lattices begin with the short one, id for id"""
    pos = {}
    for n in pf.HEIGHTS:
        o = h.make_oracle(pf.config("dfsph", walls, n), num_threads=1)
        assert o.N == n
        pos[n] = o.get(pf.orc.F_POS)
        o.close()
    for n in (704, 832):
        h.same_bits(pos[n][:640], pos[640], "the first 640 of %d" % n)
        assert (pos[n][640:, 1] > pos[640][:, 1].max()).all()        # whole layers above
    lo, hi = pf.inner_box(pf.config("dfsph", walls, 640))
    assert 0 < pf.in_box(pos[640], lo, hi).sum() <= 64
    above = pf.layer_above(pf.config("dfsph", walls, 640), 640, 64)
    assert above[:, 1].min() > pos[640][:, 1].max() + pf.D and (above < 1.0).all()


def test_threshold_counts():
    for n in pf.THRESHOLD:
        o = h.make_oracle(pf.threshold_config("dfsph", n), num_threads=1)
        assert o.N == n
        o.close()
    assert 64512 < 65536 < 66560 <= 100000


@pytest.mark.parametrize("walls", ["wall", "clamp"])
def test_pcisph_delta_is_the_same_on_both_lattices(walls):
    """the precondition of the pcisph cases (pcisph's delta is a constant of construction and is not recomputed when particles arrive): delta
    and max_count are equal on the 640, 704 and 832 lattices, bit for bit.  max_index -- the particle pre_compute took its neighbourhood from,
    a reported scalar that no step reads -- is equal on 704 and 832 (557) but not on 640 (493: the last of the tied particles sits a layer
    pair lower in the shorter column).  So the pcisph append case runs on 640 -> 832, where everything a step reads agrees, AND on the pair
    704 -> 832, on which all three agree."""
    got = []
    for n in (640, 704, 832):
        o = h.make_oracle(pf.config("pcisph", walls, n), num_threads=1)
        got.append((np.float32(o.pcisph_delta).tobytes(), o.pcisph_max_index))
        o.close()
    assert got[0][0] == got[1][0] == got[2][0] and got[0][1][1] == got[1][1][1] == got[2][1][1], got
    assert got[1] == got[2], got


# ---- Emitter / Sink ------------------------------------------------------------------------------------------------------------------------

def test_layer_geometry():
    e = emitter.Emitter(center=[0.5, 0.7, 0.4], direction=[0.0, -2.0, 0.0], size=(0.2, 0.3), speed=2.0, radius=0.025)
    assert (e.nu, e.nv, e.layer_size) == (4, 6, 24) and e.d == 0.05
    np.testing.assert_allclose(e.direction, [0, -1, 0])
    np.testing.assert_allclose(np.abs(e.u), [0, 0, 1]); np.testing.assert_allclose(np.abs(e.v), [1, 0, 0])      # direction x x^, then direction x u
    rel = e.layer - e.center
    np.testing.assert_allclose(rel.mean(axis=0), 0, atol=1e-15)                                                  # centred
    cu, cv = np.unique(np.round(rel @ e.u, 12)), np.unique(np.round(rel @ e.v, 12))
    np.testing.assert_allclose(np.diff(cu), e.d, rtol=0, atol=1e-12); np.testing.assert_allclose(np.diff(cv), e.d, rtol=0, atol=1e-12)
    assert len(cu) == 4 and len(cv) == 6 and np.abs(rel @ e.direction).max() == 0
    # a general direction: u = direction x y^ normalised, v = direction x u, a right-handed orthonormal frame
    g = emitter.Emitter(center=[0, 0, 0], direction=[1.0, 0.0, 1.0], size=(0.05, 0.01), speed=1.0, radius=0.025)
    n = np.array([1.0, 0.0, 1.0]) / math.sqrt(2.0)
    np.testing.assert_allclose(g.u, np.cross(n, [0, 1, 0]) / np.linalg.norm(np.cross(n, [0, 1, 0])))
    np.testing.assert_allclose(g.v, np.cross(n, g.u))
    assert (g.nu, g.nv) == (1, 1) and np.array_equal(g.layer, [[0, 0, 0]])                                       # at least 1 x 1
    assert emitter.Emitter(center=[0, 0, 0], direction=[1, 0, 0], size=(0.3, 0.3), speed=1.0, radius=0.05).nu == 3  # 0.3 / 0.1 in f64 is 2.99...


def test_schedule_and_advance():
    """t_k = start + k d / speed; every due layer once, several in one update, uneven steps; advanced by speed (t - t_k); one call per update"""
    e = emitter.Emitter(center=[0.5, 0.5, 0.5], direction=[1, 0, 0], size=(0.1, 0.1), speed=2.0, start=0.01, radius=0.025)      # a layer every 25 ms
    sim = pf.FakeSim(100, 10000)
    assert e.update(sim) == 0 and not sim.added                      # t = 0 < start
    sim.t = 0.01
    assert e.update(sim) == 0                                        # t_0 < t is strict
    emitted = 0
    for t in (0.0101, 0.02, 0.0849, 0.0851, 0.2, 0.2):               # uneven: 1, 0, 2, 1, 4 layers and none
        sim.t = t
        before = len(sim.added)
        n = e.update(sim)
        due = sum(1 for k in range(100) if 0.01 + k * 0.05 / 2.0 < t)
        assert e.layers_due(t) == due and n == (due - emitted) * 4
        assert len(sim.added) == before + (1 if n else 0)            # all of an update's layers in one add_particles call
        if n:
            _, pos, vel = sim.added[-1]
            ks = np.arange(emitted, due)
            want = (e.layer[None, :, :] + (2.0 * (t - (0.01 + ks * 0.05 / 2.0)))[:, None, None] * e.direction[None, None, :]).reshape(-1, 3)
            assert np.array_equal(pos, want.astype(np.float32))        # f64, rounded to f32 once
            assert np.array_equal(vel, np.broadcast_to(np.float32([2, 0, 0]), pos.shape))
        emitted = due
    assert e.emitted == emitted * 4 == sim.n_fluid - 100 and e.layers_emitted == emitted and not e.exhausted
    assert sim.clock_reads == 8                                      # one read per update


def test_stop_max_particles_and_capacity():
    mk = lambda **kw: emitter.Emitter(center=[0.5, 0.5, 0.5], direction=[0, 0, 1], size=(0.1, 0.1), speed=1.0, radius=0.025, **kw)   # noqa: E731  (a layer of 4 every 50 ms)
    e, sim = mk(stop=0.12), pf.FakeSim(0, 1000)
    sim.t = 1.0
    assert e.update(sim) == 12 and e.layers_due(1.0) == 3 and not e.exhausted        # t_k = 0, 0.05, 0.1 < stop
    sim.t = 2.0
    assert e.update(sim) == 0
    e, sim = mk(max_particles=10), pf.FakeSim(0, 1000)
    sim.t = 1.0
    assert e.update(sim) == 8 and e.exhausted and sim.n_fluid == 8                    # the third layer would make 12: never a partial layer
    assert e.update(sim) == 0 and len(sim.added) == 1
    e, sim = mk(), pf.FakeSim(93, 100)
    sim.t = 0.2
    assert e.update(sim) == 4 and e.exhausted and sim.n_fluid == 97                   # room for 7: one whole layer
    e, sim = mk(), pf.FakeSim(98, 100)
    sim.t = 0.2
    assert e.update(sim) == 0 and e.exhausted and not sim.added


def test_sink_and_apply():
    s = emitter.Sink([0.1, 0.2, 0.3], [0.4, 0.5, 0.6])
    sim = pf.FakeSim(50, 100)
    sim.in_box = 7
    assert s.apply(sim) == 7 and s.removed == 7 and sim.n_fluid == 43
    lo, hi = sim.boxes[0]
    assert np.array_equal(lo, [0.1, 0.2, 0.3]) and np.array_equal(hi, [0.4, 0.5, 0.6])
    # apply: the sinks first, then the emitters, one clock read for all of them; none once every emitter is exhausted
    es = [emitter.Emitter(center=[0.5, 0.5, 0.5], direction=[0, 0, 1], size=(0.1, 0.1), speed=1.0, radius=0.025, max_particles=4) for _ in range(2)]
    sim.t, sim.clock_reads = 0.01, 0
    assert emitter.apply(sim, es, [s]) == (7, 8) and sim.clock_reads == 1 and sim.n_fluid == 44
    sim.t = 1.0
    assert emitter.apply(sim, es, [s]) == (7, 0) and all(e.exhausted for e in es)
    emitter.apply(sim, es, [s])
    assert sim.clock_reads == 2


def test_config_keys():
    cfg = scenes.get("dfsph_tiny_wall")
    assert nat.config_from_dict(cfg).fluid_capacity == 0 and emitter.from_config(cfg) == ([], [])
    cfg["fluid"]["capacity"] = 4096
    assert nat.config_from_dict(cfg).fluid_capacity == 4096
    for bad in (-1, 1.5, "10", True):
        cfg["fluid"]["capacity"] = bad
        with pytest.raises(ValueError):
            nat.config_from_dict(cfg)
    for name in ("filling_tank_dfsph", "channel_wcsph"):
        cfg = scenes.get(name)
        c = nat.config_from_dict(cfg)
        d = 2 * cfg["scene"]["particle_radius"]
        w = cfg["fluid"]["water_size"]
        assert c.fluid_capacity >= 3 * int(w[0] / d * w[1] / d * w[2] / d)
        es, ss = emitter.from_config(cfg)
        assert len(es) == 1 and es[0].radius == cfg["scene"]["particle_radius"] and len(ss) == (1 if name == "channel_wcsph" else 0)
        lo, hi = np.float64(cfg["scene"]["box_min"]), np.float64(cfg["scene"]["box_max"])
        assert ((es[0].layer > lo) & (es[0].layer < hi)).all()
    cfg["scene"]["emitters"][0]["colour"] = "red"
    with pytest.raises(ValueError):
        emitter.from_config(cfg)
