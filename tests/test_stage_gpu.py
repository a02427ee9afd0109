"""The LDS staging routine of the staged sweeps (stage_operands, csrc/sph_kernels.h) on its own: one workgroup stages a plan the test
supplies (sph_selftest_stage) and the LDS image comes back -- compared bit for bit with a numpy expansion of the same runs.

The sizes sit on both sides of everything the routine branches on: a thread's batch is 7 elements per trip, so 256 x 7 = 1792 staged
particles are one trip and 1793 open the second (the default capacity of 1664 never does: no scene-level test reaches that trip); 255 / 256 /
257 are the last thread of the first batch element; 2560 is the largest capacity.  Whatever nst is not a multiple of 256 exercises the clamp
of the gather index at nst - 1.  Scaling is a multiplication by 2^32: exact, numpy's f32 product has the same bits."""
import numpy as np
import pytest

from cfd_taichi_amd import _native as nat
from harness import bits_equal

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 255, 256, 257, 1791, 1792, 1793, 2559, 2560]
LAYOUTS = list(nat.STAGE_LAYOUTS)
N_SRC, INSIDE, OUTSIDE = 8192, 7000, 8000        # every run lies below INSIDE; OUTSIDE is a source index no plan holds
STAGED, IDLE = 1, 2


def sources(seed=5):
    rng = np.random.default_rng(seed)
    A = rng.uniform(0.5, 2.0, (N_SRC, 4)).astype(np.float32) * rng.choice([-1.0, 1.0], (N_SRC, 4)).astype(np.float32)
    B = rng.uniform(0.5, 2.0, (N_SRC, 4)).astype(np.float32)
    S = rng.uniform(0.5, 2.0, N_SRC).astype(np.float32)
    changed = np.ones(N_SRC, dtype=np.uint8)
    return A, B, S, changed


def plan(kind, nst, rng):
    """Runs (first, count) of `nst` particles in all."""
    if nst == 0:
        return np.zeros((0, 2), dtype=np.uint32)
    if kind == "long":                              # one long run
        counts = [nst]
    elif kind == "singles":                         # runs of 1 particle; from 300 particles on exactly 300 runs (> 256: a thread expands two)
        counts = [1] * min(nst, 299) + ([nst - 299] if nst > 299 else [])
    else:                                           # cells: 1..13 particles, one run of more than 65 where it fits
        counts = [100] if nst >= 100 else []
        while sum(counts) < nst:
            counts.append(min(int(rng.integers(1, 14)), nst - sum(counts)))
        counts = list(rng.permutation(counts))
    firsts = [int(rng.integers(0, INSIDE - c)) for c in counts]          # non-monotonic across runs
    return np.array(list(zip(firsts, counts)), dtype=np.uint32)


def expand(runs):
    return np.concatenate([np.arange(f, f + c) for f, c in runs] + [np.zeros(0, dtype=np.int64)]).astype(np.int64)


def image(layout, idx, A, B, S):
    """What the layout holds per staged element, as the six floats sph_selftest_stage copies out."""
    out = np.zeros((len(idx), 6), dtype=np.float32)
    a, b = A[idx], B[idx]
    out[:, :4] = a
    if layout.endswith("_scaled"):
        out[:, :3] = a[:, :3] * np.float32(2.0 ** 32)
    if layout.startswith("ps"):
        out[:, 3] = S[idx]
    elif layout.startswith("pv"):
        out[:, 3] = b[:, 0]
        out[:, 4:6] = b[:, 1:3]
    elif layout == "f4s":
        out[:, 4] = S[idx]
    elif layout == "f4src":
        out[:, 4] = idx.astype(np.uint32).view(np.float32)
    return out


@pytest.mark.parametrize("nst", SIZES)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_staged_image_is_the_expansion_of_the_runs(layout, nst):
    A, B, S, changed = sources()
    rng = np.random.default_rng(1000 + nst)
    for kind in ("long", "singles", "cells"):
        runs = plan(kind, nst, rng)
        idx = expand(runs)
        assert len(idx) == nst
        want = image(layout, idx, A, B, S)
        for pre in (False, True):                   # the plan's head fetched by the routine, or handed in by the caller: the same image
            got, verdict = nat.selftest_stage(layout, "none", runs, A, B, S, changed, use_pre=pre)
            assert verdict == STAGED, (kind, pre)
            assert bits_equal(got[:nst], want), (kind, pre)
            assert not got[nst:].any(), (kind, pre)                 # nothing past the staged set


def key_of(layout):
    return "S" if layout.startswith("ps") else ("changed" if layout.startswith("pv") else "A.w")


@pytest.mark.parametrize("check", ["with", "first"])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_check_verdicts(layout, check):
    """kCheckWith promises the copy whatever the verdict; kCheckFirst copies only where a key is set.  A key set at a source index outside the
    plan does not count (the clamped duplicates of the batch stay inside the staged set)."""
    A0, B, S0, _ = sources()
    rng = np.random.default_rng(77)
    for nst in (1, 257, 1792, 1793, 2560):
        runs = plan("cells", nst, rng)
        idx = expand(runs)
        for where, hot in (("none", None), ("first", idx[0]), ("last", idx[-1]), ("outside", OUTSIDE)):
            A, S, changed = A0.copy(), S0.copy(), np.zeros(N_SRC, dtype=np.uint8)
            key = {"S": S, "changed": changed, "A.w": A[:, 3]}[key_of(layout)]
            key[:] = 0
            if hot is not None:
                key[hot] = 3
            expect = STAGED if where in ("first", "last") else IDLE
            for pre in (False, True):
                got, verdict = nat.selftest_stage(layout, check, runs, A, B, S, changed, use_pre=pre)
                assert verdict == expect, (nst, where, pre)
                if check == "with" or verdict == STAGED:
                    assert bits_equal(got[:nst], image(layout, idx, A, B, S)), (nst, where, pre)


@pytest.mark.parametrize("check", list(nat.STAGE_CHECKS))
def test_unstaged_and_empty_plans(check):
    """stage_cnt = -1: "not staged", whatever the runs say (the LDS is unspecified).  A staged set of no particles: the call site names the
    answer -- "staged" by default, "idle" where a sweep's zero tiles want it (k_correct on the packed float4, k_pci_press, k_ii_dij) --
    and gets it in every check mode; nothing is copied either way."""
    A, B, S, changed = sources()
    runs = plan("cells", 300, np.random.default_rng(3))
    for layout in LAYOUTS:
        for pre in (False, True):
            for idle in (False, True):
                assert nat.selftest_stage(layout, check, runs, A, B, S, changed, use_pre=pre, not_staged=True, empty_idle=idle)[1] == 0
                got, verdict = nat.selftest_stage(layout, check, runs[:0], A, B, S, changed, use_pre=pre, empty_idle=idle)
                assert verdict == (IDLE if idle else STAGED) and not got.any()
                # the named answer is for the empty set only: a set of one particle with its key set is "staged" (and copied) regardless
                got, verdict = nat.selftest_stage(layout, check, runs[:1], A, B, S, changed, use_pre=pre, empty_idle=idle)
                assert verdict == STAGED and bits_equal(got[:runs[0, 1]], image(layout, expand(runs[:1]), A, B, S))
