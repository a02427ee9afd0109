"""GPU suite: sph_download, sph_upload and sph_download_local answer every field id on every kind of handle as they did before the field table
(csrc/sph_host_fields.h) existed -- the same return code for every call, the same bytes from every call that succeeds, the same positions three
steps after every upload that is taken.

tests/golden/field_matrix.json was recorded from the library of the commit before the table (tests/golden/make_field_matrix.py says how, and what
a row holds); here the same recorder runs on the library under test, one row per case: the five solvers on their 640-particle tiny wall scene,
dfsph_rigid_small for the wall and rigid species, and the five fluid scenes on two slab handles over the loopback transport (a process of their
own each: the stand-in transport is chosen before the library loads).  No tolerance: codes are integers, bytes are compared by SHA-256."""
import importlib.util
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORDER = os.path.join(ROOT, "tests", "golden", "make_field_matrix.py")
_spec = importlib.util.spec_from_file_location("make_field_matrix", RECORDER)
matrix = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(matrix)


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(ROOT, "tests", "golden", "field_matrix.json")) as f:
        return json.load(f)


def differences(got, want, path=""):
    """every leaf where the two nested dicts / lists differ, as 'path: got != want'"""
    if isinstance(want, dict) and isinstance(got, dict):
        return [d for k in sorted(set(want) | set(got)) for d in differences(got.get(k, "missing"), want.get(k, "missing"), "%s/%s" % (path, k))]
    if isinstance(want, list) and isinstance(got, list) and len(want) == len(got):
        return [d for k, (g, w) in enumerate(zip(got, want)) for d in differences(g, w, "%s[%d]" % (path, k))]
    return [] if got == want else ["%s: %r != %r" % (path, got, want)]


def test_the_fixture_holds_every_row(recorded):
    assert sorted(recorded) == sorted(matrix.ROWS)
    for name, row in recorded.items():
        phases = ["after_3_steps", "before_first_step"] + (["after_build_neighbors"] if name == "slab2:pbf_tiny_wall" else [])
        assert sorted(row) == sorted(phases), name
        for views in row.values():
            assert len(views) == (2 if name.startswith("slab2:") else 1)
            for view in views:
                assert len(view["download"]) == len(matrix.FIELDS) == len(view["upload"]) and len(view["local"]) == 25, name


@pytest.mark.parametrize("row", matrix.ROWS)
def test_codes_and_bytes_equal_the_recorded_matrix(row, recorded, tmp_path):
    if row.startswith("slab2:"):
        out = tmp_path / "row.json"
        p = subprocess.run([sys.executable, RECORDER, "--row", row, "--out", str(out)], cwd=ROOT, capture_output=True, text=True, timeout=240)
        assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
        got = json.loads(out.read_text())[row]
    else:
        got = json.loads(json.dumps(matrix.record(row)))
    diff = differences(got, recorded[row])
    assert not diff, "%d entries differ from the recorded matrix, first: %s" % (len(diff), diff[:12])
