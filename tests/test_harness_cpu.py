"""CPU suite of tests/harness.py: the four meanings of "the same" stay apart, the knob list follows the library's sources, the launcher builds
the command lines the suites used to build by hand and re-launches once, and only, on a port that was taken."""
import glob
import json
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest

import harness as h

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
SIZES = (1, 2, 63, 64, 65, 256, 257)
PREDICATES = (h.same_values, h.same_values_nan_signed, h.same_bits, h.same_nan_mask)


def test_importing_the_harness_loads_no_library():
    code = "import harness; from cfd_taichi_amd import _native; assert _native._lib is None; print('not loaded')"
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")]))
    p = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "not loaded" in p.stdout, p.stdout[-2000:] + p.stderr[-2000:]


def accepts(pred, a, b):
    try:
        pred(a, b, "case")
    except AssertionError:
        return False
    return True


def nan(payload):
    return np.array([0x7fc00000 | payload], dtype=np.uint32).view(np.float32)[0]


def pair(n, at, x, y):
    a = np.linspace(1.0, 2.0, n, dtype=np.float32)
    b = a.copy()
    a[at], b[at] = x, y
    return a, b


# what each predicate says to a pair that differs in one entry: (values, nan_signed, bits, nan_mask)
CASES = {
    "equal": (F(1.5), F(1.5), (True, True, True, True)),
    "zeros of both signs": (F(0.0), F(-0.0), (True, False, False, True)),
    "NaNs of two payloads": (nan(1), nan(2), (False, True, False, True)),
    "the same NaN": (nan(1), nan(1), (False, True, True, True)),
    "NaN against a number": (nan(1), F(1.5), (False, False, False, False)),
    "one ulp": (F(1.5), np.nextafter(F(1.5), F(2.0)), (False, False, False, False)),
}


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("case", list(CASES))
def test_predicates_keep_their_meanings(case, n):
    x, y, want = CASES[case]
    for at in sorted({0, n // 2, n - 1}):
        a, b = pair(n, at, x, y)
        got = tuple(accepts(p, a, b) for p in PREDICATES)
        assert got == want, (case, n, at, got)
        assert h.bits_equal(a, b) == want[2]
    if n > 1:
        a, b = pair(n, 0, x, x)
        for p in PREDICATES:
            assert not accepts(p, a, b[:-1]), "%s accepts a shape mismatch" % p.__name__
            assert not accepts(p, a.reshape(1, n), b), "%s accepts a shape mismatch" % p.__name__
        assert not h.bits_equal(a, b[:-1])


def word(x):
    return int(h.bits(x).reshape(-1)[0])


def test_bits_are_the_words_of_the_input():
    assert h.bits(F(-0.0)).dtype == np.uint32 and word(F(-0.0)) == 0x80000000
    assert h.bits(np.array([-0.0])).dtype == np.uint64 and word(np.array([-0.0])) == 1 << 63
    assert h.bits([1.0, 2.0]).dtype == np.uint32                                   # a list is f32, the library's number format
    a = np.array([1.0, 1.0 + 2.0 ** -40])                                          # two f64 values of one f32 value
    assert not accepts(h.same_bits, a, a[::-1].copy()) and accepts(h.same_bits, a.astype(np.float32), a[::-1].astype(np.float32))
    with pytest.raises(AssertionError, match=r"x differs at 1 of 3 entries, rel err 5\.000e-01, first \[1\]: 2\.0 vs 1\.0$"):
        h.same_values(np.float32([1, 2, 2]), np.float32([1, 1, 2]), "x")


def test_knobs_are_the_overrides_the_library_reads():
    read = set()
    for path in glob.glob(os.path.join(ROOT, "cfd_taichi_amd", "csrc", "*")):
        if os.path.isfile(path):
            with open(path, errors="replace") as f:
                read |= set(re.findall(r'dev_env\([^,()]*,\s*"(SPH_\w+)"', f.read()))
    assert len(read) > 15
    assert set(h.KNOBS) | set(h.KNOBS_KEPT) == read
    assert not set(h.KNOBS) & set(h.KNOBS_KEPT) and "SPH_RCCL_LIB" in h.KNOBS_KEPT
    assert len(set(h.KNOBS)) == len(h.KNOBS)
    assert set(h.MORTON) | set(h.LINEAR) <= set(h.KNOBS)


def test_stats_tuple_of_the_five_solvers():
    st = types.SimpleNamespace(n_div=3, n_dens=5, n_div_evals=7, div_first_err=0.5, div_err=0.25, dens_err=0.125, dt=1e-3, lost=0)
    assert h.stats_tuple(st, "dfsph") == (3, 5, 0.5, 0.25, 0.125, 1e-3)
    assert h.stats_tuple(st, "pcisph") == h.stats_tuple(st, "iisph") == (5, 0.125)
    assert h.stats_tuple(st, "wcsph") == h.stats_tuple(st, "pbf") == ()
    assert h.stats_tuple(None, "wcsph") == ()                                      # a step without statistics returns None
    assert h.stats_bits(st, h.ORACLE_STATS) == (3, 5, 7, 0x3f000000, 0x3e800000, 0x3e000000, word(F(1e-3)))
    h.same_stats(st, st, "dfsph", "statistics")
    with pytest.raises(AssertionError):
        h.same_stats(st, types.SimpleNamespace(**dict(vars(st), dens_err=-0.125)), "iisph", "statistics")


class Launches:
    """subprocess.run, stubbed: records the calls, writes the worker's JSON, fails as scripted"""

    def __init__(self, out, failures=()):
        self.out, self.failures, self.calls = out, list(failures), []

    def __call__(self, cmd, **kw):
        self.calls.append((cmd, kw))
        if self.failures:
            code, err = self.failures.pop(0)
            return types.SimpleNamespace(returncode=code, stdout="", stderr=err)
        with open(self.out, "w") as f:
            json.dump({"ok": len(self.calls)}, f)
        return types.SimpleNamespace(returncode=0, stdout="", stderr="")


def test_run_ranks_builds_both_command_lines(tmp_path, monkeypatch):
    out = tmp_path / "out.json"
    run = Launches(out)
    monkeypatch.setattr(subprocess, "run", run)
    monkeypatch.setenv("SPH_SLAB_CHECK", "0")
    assert h.run_ranks("w.py", ["--steps", 3, "--out", out], 3, "gloo", out, {"SPH_CELL_ORDER": "morton"}, timeout=900) == {"ok": 1}
    assert h.run_ranks("w.py", ("--world", 2), 2, "loopback", out) == {"ok": 2}
    (gloo, kw), (plain, kw2) = run.calls
    port = gloo[9]
    assert gloo == [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "3", "--master-addr", "127.0.0.1", "--master-port", port,
                    "w.py", "--steps", "3", "--out", str(out)] and 0 < int(port) < 65536
    assert plain == [sys.executable, "w.py", "--world", "2"]
    for k in (kw, kw2):
        assert k["cwd"] == ROOT and k["capture_output"] and k["text"]
        assert (k["env"]["SPH_SLAB_CHECK"], k["env"]["OMP_NUM_THREADS"], k["env"]["HSA_ENABLE_IPC_MODE_LEGACY"]) == ("1", "2", "0")
    assert kw["timeout"] == 900 and kw["env"]["SPH_CELL_ORDER"] == "morton"
    assert kw2["timeout"] == 300 and "SPH_CELL_ORDER" not in kw2["env"]


@pytest.mark.parametrize("transport", ["gloo", "loopback"])
def test_run_ranks_launches_again_once_and_only_for_a_taken_port(tmp_path, monkeypatch, transport):
    out = tmp_path / "out.json"
    taken = (1, "RuntimeError: The server socket has failed to listen on any local network address. EADDRINUSE")
    run = Launches(out, [taken])
    monkeypatch.setattr(subprocess, "run", run)
    assert h.run_ranks("w.py", [], 2, transport, out) == {"ok": 2}
    assert len(run.calls) == 2
    if transport == "gloo":
        assert run.calls[0][0][:9] == run.calls[1][0][:9] and run.calls[0][0][10:] == run.calls[1][0][10:]
    for failures, launches in (([taken, taken], 2), ([(1, "Memory access fault")], 1), ([(-6, "")], 1), ([(0, "EADDRINUSE")], 1)):
        run = Launches(out, failures)
        monkeypatch.setattr(subprocess, "run", run)
        if failures[-1][0] == 0:
            out.write_text("{}")
            assert h.run_ranks("w.py", [], 2, transport, out) == {}
        else:
            with pytest.raises(AssertionError):
                h.run_ranks("w.py", [], 2, transport, out)
        assert len(run.calls) == launches, failures
