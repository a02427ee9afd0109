"""tests/slab_ranks.py, the plumbing every slab worker stands on, with fake handles: no GPU, no library.  The multi-GPU suite holds the slab path
to "bit-equal to one GPU" through this module, so a join that leaves a rank running, a gather that passes a non-partition or a comparison that
takes -0.0 for +0.0 would weaken every one of those tests at once."""
import os
import sys
import threading
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import slab_ranks as sr  # noqa: E402
from harness import bits_equal  # noqa: E402


class FakeError(RuntimeError):
    def __init__(self, code):
        super().__init__("fake error %d" % code)
        self.code = code


class FakeSim:
    """what Ranks touches of nat.Simulation; owns the particles `ids` of `source`"""

    def __init__(self, cfg, ids=(), source=None):
        self.cfg, self.ids, self.source = cfg, np.asarray(ids, dtype=np.int64), source
        self.n_fluid = 0 if source is None else len(source)
        self.attached = None

    def rccl_attach(self, uid, capacity):
        self.attached = uid

    def download_owned(self, field):
        return self.ids, self.source[self.ids]


def fake_nat():
    made = []

    def config_from_dict(cfg, **kw):
        return types.SimpleNamespace(solver=1, kw=kw)

    def simulation(cfg, rigid=None):
        made.append(FakeSim(cfg))
        return made[-1]
    return types.SimpleNamespace(SOLVER_WCSPH=0, F_POS=0, SphError=FakeError, config_from_dict=config_from_dict, Simulation=simulation,
                                 rccl_unique_id=lambda: b"id")


def test_the_constructor_makes_every_rank_and_attaches_them_all():
    g = sr.Ranks(fake_nat(), {}, 3, per_rank={2: {"slab_capacity": 600}}, slab_overlap=2)
    assert [s.cfg.kw for s in g.sims] == [dict(slab_rank=r, slab_count=3, slab_overlap=2, **({"slab_capacity": 600} if r == 2 else {})) for r in range(3)]
    assert [s.attached for s in g.sims] == [b"id"] * 3 and g.errors == [None] * 3


def test_each_runs_the_ranks_at_once_and_joins_all_before_it_raises():
    g = sr.Ranks(fake_nat(), {}, 3)
    meet = threading.Barrier(3, timeout=10)
    assert g.each(lambda r, s: meet.wait() >= 0 and r * r) == [0, 1, 4]          # one after the other they would never meet
    go, finished = threading.Event(), []

    def fn(r, s):
        if r == 1:
            try:
                raise FakeError(-4)
            finally:
                go.set()
        assert go.wait(10)              # the others end only after rank 1 has failed
        finished.append(r)
    with pytest.raises(FakeError):
        g.each(fn)
    assert sorted(finished) == [0, 2]
    assert [type(e) for e in g.errors] == [type(None), FakeError, type(None)]


def test_codes_reports_the_failing_rank_alone():
    g = sr.Ranks(fake_nat(), {}, 3)

    def fn(r, s):
        if r == 1:
            raise FakeError(-4)
    assert g.codes(fn) == [0, -4, 0]
    assert g.codes(lambda r, s: None) == [0, 0, 0]


def group_over(source, owned):
    g = sr.Ranks(fake_nat(), {}, len(owned))
    g.sims = [FakeSim(None, ids, source) for ids in owned]
    return g


def test_gather_by_id_returns_a_partition_in_id_order_bit_for_bit():
    source = np.arange(18, dtype=np.float32).reshape(6, 3)
    source[2, 1], source[4, 0] = np.nan, -0.0
    g = group_over(source, [[4, 0], [], [5, 3, 1, 2]])
    out, seen = sr.gather_by_id(g.sims, 0)
    assert seen.tolist() == [1] * 6 and bits_equal(out, source)
    assert bits_equal(g.gather(0), source)


def test_a_missing_and_a_duplicated_id_show_in_the_counts_and_fail_the_gather():
    source = np.arange(6, dtype=np.float32)
    g = group_over(source, [[0, 1, 2], [2, 4, 5]])             # 3 is nobody's, 2 is owned twice
    out, seen = sr.gather_by_id(g.sims, 0)
    assert seen.tolist() == [1, 1, 2, 0, 1, 1] and np.isnan(out[3])
    with pytest.raises(AssertionError, match="1 missing, 1 duplicated"):
        g.gather(0)


def test_same_bits_is_a_comparison_of_bits():
    a = np.array([0.0, np.nan], dtype=np.float32)
    assert not bits_equal(a, np.array([-0.0, np.nan], dtype=np.float32))
    assert bits_equal(a, a.copy()) and not np.array_equal(a, a.copy())
    assert not bits_equal(a, a[:1])


def test_stat_row():
    assert sr.stat_row(None) is None
    st = types.SimpleNamespace(n_div=2, n_dens=3, n_div_evals=4, div_first_err=np.float32(0.5), div_err=np.float32(0.25), dens_err=np.float32(0.125), dt=np.float32(1e-3))
    assert sr.stat_row(st) == [2, 3, 4, 0.5, 0.25, 0.125, float(np.float32(1e-3))]


def test_owned_samples_counts_the_columns_lo_to_hi():
    x = np.array([0.05, 0.15, 0.25, 0.35], dtype=np.float32)
    assert sr.owned_samples(x, np.float32(0.1), [1, 3]) == 2 and sr.owned_samples(x, np.float32(0.1), [3, 3]) == 0
