"""GPU suite: every entry point that acts between steps answers as it did before the host layer's staleness routine, side-memory owner and
API-order read-back existed (csrc/sph_host_scene.h) -- the same return code and sph_last_error text for every call, the same bytes from every call
that returns data, and after every edit the same positions, the same launches per kernel, the same graph replays and Verlet list builds over the steps
that follow.

tests/golden/between_steps_matrix.json was recorded from the library of the commit before those routines (tests/golden/make_between_steps_matrix.py
says how, and what a row holds); here the same recorder runs on the library under test, one case per row; the slab rows in a process of their own
(the stand-in transport is chosen before the library loads).  No tolerance: codes are integers, texts are compared as they are, bytes by SHA-256.
A digest or count that differed between two recordings of the older library itself reads "dropped" in the fixture and is not compared."""
import importlib.util
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORDER = os.path.join(ROOT, "tests", "golden", "make_between_steps_matrix.py")
_spec = importlib.util.spec_from_file_location("make_between_steps_matrix", RECORDER)
matrix = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(matrix)


@pytest.fixture(scope="module")
def recorded():
    return matrix.load(os.path.join(ROOT, "tests", "golden", "between_steps_matrix.json"))


def leaves(x):
    if isinstance(x, dict):
        return [v for k in x for v in leaves(x[k])]
    if isinstance(x, list):
        return [v for k in x for v in leaves(k)]
    return [x]


def differences(got, want, path=""):
    """every leaf where the two nested dicts / lists differ, as 'path: got != want'"""
    if isinstance(want, dict) and isinstance(got, dict):
        return [d for k in sorted(set(want) | set(got)) for d in differences(got.get(k, "missing"), want.get(k, "missing"), "%s/%s" % (path, k))]
    if isinstance(want, list) and isinstance(got, list) and len(want) == len(got):
        return [d for k, (g, w) in enumerate(zip(got, want)) for d in differences(g, w, "%s[%d]" % (path, k))]
    return [] if got == want or want == matrix.DROPPED else ["%s: %r != %r" % (path, got, want)]


def test_the_fixture_holds_every_row_and_call(recorded):
    assert sorted(recorded) == sorted(matrix.ROWS)
    for name, row in recorded.items():
        assert sorted(row) == ["after_%d_steps" % matrix.STEPS, "before_first_step"], name
        for calls in row.values():
            assert sorted(calls) == sorted(c.name for c in matrix.CALLS), name
            for call in matrix.CALLS:
                assert sorted(calls[call.name]["variants"]) == sorted(label for label, _ in call.variants), (name, call.name)
                for entries in calls[call.name]["variants"].values():
                    assert len(entries) == (2 if name.startswith("slab2:") else 1), (name, call.name)
    every = leaves(recorded)
    assert every.count(matrix.DROPPED) * 100 <= len(every)


def test_every_edit_is_followed_somewhere(recorded):
    """every call marked as an edit succeeded, and was followed through its steps, on at least one row and in both phases"""
    for call in matrix.CALLS:
        if call.stale:
            for ph in ("before_first_step", "after_%d_steps" % matrix.STEPS):
                assert any("stale" in row[ph][call.name] for row in recorded.values()), (call.name, ph)


@pytest.mark.parametrize("row", matrix.ROWS)
def test_calls_between_steps_equal_the_recorded_matrix(row, recorded, tmp_path):
    if row.startswith("slab2:"):
        out = tmp_path / "row.json"
        p = subprocess.run([sys.executable, RECORDER, "--row", row, "--out", str(out)], cwd=ROOT, capture_output=True, text=True, timeout=240)
        assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
        got = matrix.load(str(out))[row]
    else:
        got = json.loads(json.dumps(matrix.record(row)))
    diff = differences(got, recorded[row])
    assert not diff, "%d entries differ from the recorded matrix, first: %s" % (len(diff), diff[:12])
