"""Records tests/golden/field_matrix.json: what sph_download, sph_upload and sph_download_local answer for every field id on every kind of handle.

The fixture pins the accept / refuse decisions, the return codes and the bytes of the three entry points, so that the table they are written on
(csrc/sph_host_fields.h) can be edited without changing any of them unnoticed.  It was recorded from the library as it stood BEFORE the table
existed, loaded through the SPH_LIB development override:

    SPH_DEV=1 SPH_LIB=/path/to/the/older/libsph_mi355x.so python tests/golden/make_field_matrix.py --out tests/golden/field_matrix.json

tests/test_field_table_gpu.py runs `record(row)` on the library under test, row by row, and compares.

Rows: the five solvers on their 640-particle tiny wall scene, dfsph_rigid_small (the wall and rigid species carry data there), and the five fluid
scenes again as two slab handles of one process on the loopback transport (tests/slab_ranks.py; "slab2:<scene>", run in a process of their own
because the stand-in transport is chosen before the library loads).  Per row and phase -- before the first step, after three steps, and for pbf on
slabs once more after a further sph_build_neighbors -- every (species, field) of FIELDS is asked of each entry point with every array size the
species knows (3 n and n floats; rigid: the vertices' 3 n too), so the size checks are pinned with the rest.  An entry is the return code, or for a
call that succeeded the SHA-256 of the bytes it returned.  sph_upload gets back what sph_download returned (zeros where that was refused); where it
succeeds, on a handle of its own, the entry is the SHA-256 of pos three steps later.
"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

FLUID_SCENES = ["wcsph_tiny_wall", "dfsph_tiny_wall", "dfsph_tiny_wall_pcisph", "dfsph_tiny_wall_iisph", "pbf_tiny_wall"]
ROWS = FLUID_SCENES + ["dfsph_rigid_small"] + ["slab2:" + s for s in FLUID_SCENES]
FLUID, WALL, RIGID = 0, 1, 2
# every fluid field id 0 .. 24, the undefined ones included; the wall's and the body's fields and one id past each group
FIELDS = [(FLUID, f) for f in range(25)] + [(WALL, f) for f in (32, 33, 34)] + [(RIGID, f) for f in (48, 49, 50, 51, 52, 53)]
STEPS = 3


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def sizes(sim, species, resident=None):
    """the array sizes a caller could offer for a field of this species, labelled"""
    if resident is not None:
        return {"3n": 3 * resident, "n": resident}
    if species == WALL:
        return {"3n": 3 * sim.n_wall, "n": sim.n_wall}
    if species == RIGID:
        return {"3n": 3 * sim.n_rigid, "n": sim.n_rigid, "3v": 3 * sim.n_vertices}
    return {"3n": 3 * sim.n_fluid, "n": sim.n_fluid}


def download(sim, species, field, count):
    out = np.full(max(count, 1), np.float32(np.nan), dtype=np.float32)
    rc = sim._lib.sph_download(sim._h, species, field, out.ctypes.data, count)
    return (rc, out[:count])


def download_local(sim, field, count):
    out = np.full(max(count, 1), np.float32(np.nan), dtype=np.float32)
    rc = sim._lib.sph_download_local(sim._h, field, out.ctypes.data, count)
    return (rc, out[:count])


def upload(sim, species, field, arr):
    arr = np.ascontiguousarray(arr, dtype=np.float32)
    keep = arr if arr.size else np.zeros(1, dtype=np.float32)
    return sim._lib.sph_upload(sim._h, species, field, keep.ctypes.data, arr.size)


def entry(rc, arr):
    return sha(arr) if rc == 0 else rc


class OneGpu:
    """a row on one handle; .fresh(steps) is another handle of the same scene, that many steps on"""

    def __init__(self, nat, scene):
        from cfd_taichi_amd import mesh, scenes
        self.nat, self.cfg = nat, scenes.get(scene)
        self.rigid = mesh.rigid_from_config(self.cfg) if scene == "dfsph_rigid_small" else None
        self.sims = [self.make()]

    def make(self):
        return self.nat.Simulation(self.nat.config_from_dict(self.cfg), rigid=self.rigid)

    def step(self, sims, n):
        for _ in range(n):
            for s in sims:
                s.step(1)
                if self.rigid is not None:
                    s.rigid_step()

    def fresh(self, steps):
        sims = [self.make()]
        self.step(sims, steps)
        return sims

    def build_neighbors(self, sims):
        for s in sims:
            s.build_neighbors()

    def close(self, sims):
        for s in sims:
            s.close()


class Slabs(OneGpu):
    """the same over two slab handles on the loopback transport: steps and list builds are collective"""

    def __init__(self, nat, scene):
        from cfd_taichi_amd import scenes
        from slab_ranks import Ranks
        self.nat, self.cfg, self.rigid, self.Ranks = nat, scenes.get(scene), None, Ranks
        self.groups = {}
        self.sims = self.fresh(0)

    def fresh(self, steps):
        g = self.Ranks(self.nat, self.cfg, 2)
        self.groups[id(g.sims)] = g
        self.step(g.sims, steps)
        return g.sims

    def step(self, sims, n):
        for _ in range(n):
            self.groups[id(sims)].step()

    def build_neighbors(self, sims):
        self.groups[id(sims)].each(lambda r, s: s.build_neighbors())

    def close(self, sims):
        self.groups.pop(id(sims)).close()


def phase(row, same_state):
    """every entry point on every field of the row's handles as they stand.  The uploads go to a second set of handles in the same state
    (same_state() makes one), replaced after every upload that succeeded (a refused one leaves its handle unchanged, include/sph_mi355x.h)"""
    out = []
    trial = None
    for k, sim in enumerate(row.sims):
        view = {"download": {}, "local": {}, "upload": {}}
        resident = sum(sim.slab_info()[key] for key in ("owned", "ghosts")) if isinstance(row, Slabs) else sim.n_fluid
        for species, field in FIELDS:
            name = "%d/%d" % (species, field)
            got = {label: download(sim, species, field, n) for label, n in sizes(sim, species).items()}
            view["download"][name] = {label: entry(*g) for label, g in got.items()}
            if species == FLUID:
                view["local"][name] = {label: entry(*download_local(sim, field, n)) for label, n in sizes(sim, species, resident).items()}
            view["upload"][name] = {}
            for label, (rc, arr) in got.items():
                trial = trial or same_state()
                if rc == 0:         # the trial handle's own download (the same bytes, by the two recordings of the download entry)
                    rc, arr = download(trial[k], species, field, arr.size)
                    assert rc == 0, (name, label, rc)
                else:
                    arr = np.zeros(arr.size, dtype=np.float32)
                urc = upload(trial[k], species, field, arr)
                if urc == 0:
                    row.step(trial, STEPS)
                    urc = sha(trial[k].download(row.nat.F_POS))
                    row.close(trial)
                    trial = None
                view["upload"][name][label] = urc
        out.append(view)
    if trial:
        row.close(trial)
    return out


def record(name):
    """the matrix row `name` of the library that cfd_taichi_amd._native loads"""
    if name.startswith("slab2:"):
        from slab_ranks import loopback_env
        loopback_env()
    from cfd_taichi_amd import _native as nat
    row = Slabs(nat, name[6:]) if name.startswith("slab2:") else OneGpu(nat, name)
    res = {"before_first_step": phase(row, lambda: row.fresh(0))}
    row.step(row.sims, STEPS)
    res["after_%d_steps" % STEPS] = phase(row, lambda: row.fresh(STEPS))
    if name == "slab2:pbf_tiny_wall":       # a slab handle's pbf fields do not survive a re-sort
        def rebuilt():
            sims = row.fresh(STEPS)
            row.build_neighbors(sims)
            return sims
        row.build_neighbors(row.sims)
        res["after_build_neighbors"] = phase(row, rebuilt)
    row.close(row.sims)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--row", action="append", help="a row of ROWS (default: all; slab rows need a process of their own, so they are spawned)")
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    rows = args.row or ROWS
    if len(rows) == 1:
        result = {rows[0]: record(rows[0])}
    else:
        import subprocess
        import tempfile
        result = {}
        for name in rows:       # one process per row: a slab row chooses its transport before the library loads
            with tempfile.TemporaryDirectory() as tmp:
                part = os.path.join(tmp, "row.json")
                subprocess.run([sys.executable, os.path.abspath(__file__), "--row", name, "--out", part], check=True, cwd=ROOT, timeout=600)
                with open(part) as f:
                    result.update(json.load(f))
    with open(args.out, "w") as f:
        json.dump(result, f, indent=0, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
