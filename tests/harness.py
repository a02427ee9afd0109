"""The one harness of the suites (TEST INFRASTRUCTURE): what "the same" means, how a handle and an oracle are made and stepped, how ranks are
launched.  A plain module: nothing here builds or loads the HIP library at import time (`nat.load()` happens when a handle is made).

"Bit-equal" in a suite's docstring names one of four meanings, each a raising predicate `(a, b, what)` with one message format:

  same_values             shapes equal and np.array_equal: -0.0 equals +0.0, any NaN fails
  same_values_nan_signed  values equal, NaNs equal NaNs of any payload, and the sign of zero must agree
  same_bits               the raw words (u32 of f32, u64 where both inputs are f64): -0.0 is not +0.0, a NaN equals only the NaN of the same payload
  same_nan_mask           the NaN masks agree and everything else is equal by value (-0.0 equals +0.0)

`bits(x)` is the view same_bits compares, `bits_equal(a, b)` its answer as a bool (for workers that report instead of raising).
"""
import json
import os
import socket
import subprocess
import sys

import numpy as np

from cfd_taichi_amd import _native as nat
from oracle import oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ---- comparisons ------------------------------------------------------------------------------------------------------------------------------


_WORDS = {np.dtype(t): np.dtype(u) for t, u in ((np.float64, np.uint64), (np.int64, np.uint64), (np.uint64, np.uint64), (np.int32, np.uint32), (np.uint32, np.uint32))}


def _f32(x):
    """f64 and 4- or 8-byte integer arrays keep their type; everything else (f32, lists, Python scalars) is f32, the number format of the library
    and the oracle"""
    return np.asarray(x) if getattr(x, "dtype", None) in _WORDS else np.asarray(x, dtype=np.float32)


def bits(x):
    """the raw words of x: u32 of f32 and of 4-byte integers, u64 of an f64 or 8-byte integer array"""
    x = np.ascontiguousarray(_f32(x))
    return x.view(_WORDS.get(x.dtype, np.uint32))


def _pair(a, b):
    """both as they are where both are arrays of one kept type (_f32), else both as f32"""
    if getattr(a, "dtype", None) in _WORDS and getattr(a, "dtype", None) == getattr(b, "dtype", None):
        return np.asarray(a), np.asarray(b)
    return np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)


def bits_equal(a, b):
    a, b = _pair(a, b)
    return a.shape == b.shape and bool(np.array_equal(bits(a), bits(b)))


def _differs(what, a, b, bad):
    """the one message: how many of how many, the relative error where both sides are finite numbers, the first index with both values"""
    bad = np.argwhere(bad)
    rel = ""
    if a.dtype.kind in "fiu" and b.dtype.kind in "fiu" and a.size:
        a64, b64 = a.astype(np.float64), b.astype(np.float64)
        if np.isfinite(a64).all() and np.isfinite(b64).all():
            rel = ", rel err %.3e" % (float(np.abs(a64 - b64).max()) / max(float(np.abs(b64).max()), 1e-30))
    i = tuple(bad[0])
    raise AssertionError("%s differs at %d of %d entries%s, first %s: %r vs %r" % (what, len(bad), a.size, rel, [int(k) for k in i], a[i].item(), b[i].item()))


def same_values(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, "%s: shapes %s vs %s" % (what, a.shape, b.shape)
    if not np.array_equal(a, b):
        _differs(what, a, b, a != b)


def same_values_nan_signed(a, b, what):
    a, b = _pair(a, b)
    assert a.shape == b.shape, "%s: shapes %s vs %s" % (what, a.shape, b.shape)
    bad = ~((a == b) | (np.isnan(a) & np.isnan(b))) | ((np.signbit(a) & (a == 0)) != (np.signbit(b) & (b == 0)))
    if bad.any():
        _differs(what, a, b, bad)


def same_bits(a, b, what):
    a, b = _pair(a, b)
    assert a.shape == b.shape, "%s: shapes %s vs %s" % (what, a.shape, b.shape)
    if not np.array_equal(bits(a), bits(b)):
        _differs(what, a, b, bits(a) != bits(b))


def same_nan_mask(a, b, what):
    a, b = _pair(a, b)
    assert a.shape == b.shape, "%s: shapes %s vs %s" % (what, a.shape, b.shape)
    assert np.array_equal(np.isnan(a), np.isnan(b)), "%s: NaN at different places: %r vs %r" % (what, a, b)
    if not np.array_equal(a, b, equal_nan=True):
        _differs(what, a, b, ~((a == b) | np.isnan(a)))


# ---- handles ----------------------------------------------------------------------------------------------------------------------------------

# every development override the library reads through dev_env( in cfd_taichi_amd/csrc/ (tests/test_harness_cpu.py holds the list to the
# sources): make_handle clears them all, so a suite that says it runs on the product defaults does so whatever the ambient environment holds
KNOBS = ("SPH_ARITH", "SPH_BNL_SPLIT", "SPH_CELL_ORDER", "SPH_CELL_TILE", "SPH_DENS_PUSH", "SPH_KR_SPLIT", "SPH_LATTICE_F64", "SPH_LAYER_GENERIC",
         "SPH_NBR_CAP", "SPH_NL16", "SPH_QUAD", "SPH_SLAB_GATHER", "SPH_SLAB_GRID_FULL", "SPH_STAGE", "SPH_STAGE_CAP", "SPH_STATE_CHUNK", "SPH_TILE_SKIP",
         "SPH_VERLET_SKIN", "SPH_WALL_CACHE")
# ... except what a test process must keep from its parent:
KNOBS_KEPT = (
    "SPH_RCCL_LIB",       # the stand-in transport library: slab_ranks.loopback_env sets it for the whole rank process, and every later handle loads through it
    "SPH_SLAB_CHECK",     # the parent-side launchers (run_ranks) and slab_ranks.loopback_env switch the bookkeeping check on for the whole rank process
)
# (the other slab knobs -- SPH_SLAB_GATHER, SPH_SLAB_GRID_FULL, SPH_LAYER_GENERIC, SPH_STATE_CHUNK -- are per-launch choices a parent hands to a worker
# through env_extra and the worker's handles read; no in-process factory relies on an inherited one, so they are cleared like the rest)
MORTON = {"SPH_CELL_ORDER": "morton", "SPH_CELL_TILE": "4"}      # cells along the Morton curve, and with them the staged sweeps
LINEAR = {"SPH_CELL_ORDER": "linear"}


def make_handle(cfg, monkeypatch, env=None, arith="exact", rigid=None, **config_kw):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    return nat.Simulation(nat.config_from_dict(cfg, arith=nat.arith_id(arith), **config_kw), rigid=rigid)


def refused(code, call):
    """`call` must raise SphError with `code`; returns the message"""
    try:
        call()
    except nat.SphError as e:
        assert e.code == code, (e.code, code, str(e))
        return str(e)
    raise AssertionError("the call was not refused (expected code %d)" % code)


# ---- the oracle side ----------------------------------------------------------------------------------------------------------------------------

ORACLE_STATS = ("n_div", "n_dens", "n_div_evals", "div_first_err", "div_err", "dens_err", "dt")       # OrcStepStats


def make_oracle(cfg, solver=None, rigid=None, num_threads=8):
    return orc.Oracle(cfg, solver=solver, num_threads=num_threads, rigid=rigid)


def stats_bits(st, names):
    """the named statistics as integers: floats by their f32 words"""
    return tuple(int(bits(np.float32(v)).reshape(-1)[0]) if isinstance(v, float) else int(v) for v in (getattr(st, n) for n in names))


def oracle_step(o, solver, bits_view=False):
    """One step of the oracle's restatement of `solver` (the dfsph density loop capped at 100).  Returns its statistics object; bits_view: None
    for wcsph / pbf (no statistics), else (stats_bits of ORACLE_STATS + (o.lost,), capped)."""
    capped = o.step_dfsph(1, 100) if solver == "dfsph" else getattr(o, "step_" + solver)(1)
    if not bits_view:
        return o.last_stats
    return None if solver in ("wcsph", "pbf") else (stats_bits(o.last_stats, ORACLE_STATS) + (o.lost,), capped)


def stats_tuple(st, solver):
    """What the suites compare of a step's statistics (wcsph and pbf have none)."""
    if solver == "dfsph":
        return (st.n_div, st.n_dens, st.div_first_err, st.div_err, st.dens_err, st.dt)
    if solver in ("wcsph", "pbf"):
        return ()
    return (st.n_dens, st.dens_err)


def same_stats(st, ot, solver, what):
    """stats_tuple of two sides under same_bits (wcsph and pbf: nothing to compare)"""
    same_bits(np.float32(stats_tuple(st, solver)), np.float32(stats_tuple(ot, solver)), what)


def fluid_state(x, solver):
    """Everything a step of `solver` reads of the fluid, from an Oracle or a Simulation."""
    if isinstance(x, orc.Oracle):
        st = {"pos": x.get(orc.F_POS), "vel": x.get(orc.F_VEL), "dt": x.dt}
        if solver == "dfsph":
            st["warm_k"] = x.get(orc.F_WARM_K)
        if solver == "iisph":
            st["p_past"] = x.get(orc.F_P_PAST)
        return st
    st = {"pos": x.download(nat.F_POS), "vel": x.download(nat.F_VEL), "dt": x.scalar(nat.S_DELTA_TIME)}
    if solver == "dfsph":
        st["warm_k"] = x.download(nat.F_WARM_K)
    if solver == "iisph":
        st["p_past"] = x.download(nat.F_PRESS_ITER)         # last step's pressure (iisph_solver.py:68, :209-210)
    return st


def give(o, st, solver):
    """Hand a fluid state to a fresh oracle."""
    o.set(orc.F_POS, st["pos"]); o.set(orc.F_VEL, st["vel"])
    if solver == "dfsph":
        o.set(orc.F_WARM_K, st["warm_k"])
        o.set_dt(st["dt"])
    if solver == "iisph":
        o.set(orc.F_P_PAST, st["p_past"])
    return o


def give_sim(sim, st, solver):
    """The same into a Simulation (iisph's last pressure cannot be uploaded: dfsph, wcsph and pcisph only)."""
    assert solver != "iisph"
    sim.upload(nat.F_POS, st["pos"]); sim.upload(nat.F_VEL, st["vel"])
    if solver == "dfsph":
        sim.upload(nat.F_WARM_K, st["warm_k"])
        sim.set_dt(st["dt"])
    return sim


def squeezed(pos, factor):
    """The rest lattice is under-dense by the reference's density sum (no self term): pbf's constraint max(rho / rho_0 - 1, 0) would stay at zero
    until the column has collapsed.  Squeezing the lattice about its low corner makes lambda and delta_pos act from the first step."""
    about = pos.min(0)
    return (about + (pos - about) * np.float32(factor)).astype(np.float32)


def squeeze(sim, o, factor=0.9):
    sq = squeezed(o.get(orc.F_POS), factor)
    o.set(orc.F_POS, sq); sim.upload(nat.F_POS, sq)


# ---- rank launches, parent side ---------------------------------------------------------------------------------------------------------------

def free_port():
    """a port that was free a moment ago (run_ranks knows what that is worth)"""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def run_ranks(worker, args, world, transport, out, env_extra=None, timeout=300):
    """Run `worker args` and return the JSON it wrote to `out`: under torch.distributed.run with `world` processes for transport "gloo", as one
    process (whose ranks are threads) otherwise.  SPH_SLAB_CHECK: every step, the host's bookkeeping of the edge-column populations is compared
    with the sorted arrays; the ranks share one GPU and the box's CPUs."""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="2", SPH_SLAB_CHECK="1")
    env.update(env_extra or {})
    tail = [worker] + [str(a) for a in args]
    for attempt in range(2):
        if transport == "gloo":
            cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world), "--master-addr", "127.0.0.1",
                   "--master-port", str(free_port())] + tail
        else:
            cmd = [sys.executable] + tail
        p = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
        # free_port() names a port that was free a moment ago; if someone else on the machine took it before the launcher's store could listen,
        # no worker was started: once more, with another port
        if p.returncode == 0 or "EADDRINUSE" not in p.stderr:
            break
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    with open(str(out)) as f:
        return json.load(f)
