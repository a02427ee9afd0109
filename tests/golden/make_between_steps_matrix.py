"""Records tests/golden/between_steps_matrix.json: what every entry point that acts BETWEEN steps answers, and what it leaves behind for the steps
that follow, on every kind of handle.

The fixture pins the host layer's decisions -- which refusal wins, the return codes, the sph_last_error texts, the bytes of every read-back, and after
every edit which lists are rebuilt, which densities recomputed and which captured wcsph step pairs dropped -- so that the routines those decisions are
written on (csrc/sph_host_scene.h: the staleness routine, the side memories, the API-order read-back) can be edited without changing any of them
unnoticed.  It was recorded from the library of the commit BEFORE those routines existed, loaded through the SPH_LIB development override:

    SPH_DEV=1 SPH_LIB=/path/to/the/older/libsph_mi355x.so python tests/golden/make_between_steps_matrix.py --out tests/golden/between_steps_matrix.json

tests/test_between_steps_gpu.py runs `record(row)` on the library under test, row by row, and compares with what `load` reads from the fixture.

Rows (ROWS): the five solvers on their 640-particle tiny wall scene, wcsph and pbf with clamp walls, dfsph under the relaxed arithmetic,
dfsph_rigid_small, and dfsph / wcsph as two slab handles of one process on the loopback transport (tests/slab_ranks.py; "slab2:<scene>", in a process
of their own because the stand-in transport is chosen before the library loads).

Per row and phase -- before the first step, after three steps -- every call of CALLS is made.  A call has variants: its valid smallest argument, a null
pointer where it takes one, a wrong element count where it takes one; a call of a feature that must be enabled first is made without that (no `prep`,
on the phase's shared handle) and with it.  An entry is [return code, sph_last_error text] and, for a call that returned data, the SHA-256 of the
bytes.  Calls that neither edit the handle nor need a feature share one handle per phase, in the order of CALLS; every other call gets a handle of its
own in the phase's state.  After a call that succeeded and edits the handle (`stale`): three further steps with profiling on -- the SHA-256 of pos, the
launches per kernel id, SPH_S_GRAPH_LAUNCHES and SPH_S_VERLET_BUILDS -- and, because a profiled wcsph handle launches eagerly, three more steps
without it (`tail`): a step pair captured before the edit and wrongly kept would replay there with its old arguments.  Reads that mean something only
after steps (`after`) follow.

main() records every row TWICE.  Return codes and texts are host decisions: a difference between the two recordings is an error.  A digest or count
that differs is replaced by DROPPED and named; more than 1 % of them is an error (the scenario is wrong then, not the cap).
"""
import argparse
import copy
import ctypes
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

TINY = ["wcsph_tiny_wall", "dfsph_tiny_wall", "dfsph_tiny_wall_pcisph", "dfsph_tiny_wall_iisph", "pbf_tiny_wall"]
ROWS = TINY + ["wcsph_tiny_clamp", "pbf_tiny_clamp", "relaxed:dfsph_tiny_wall", "dfsph_rigid_small", "slab2:dfsph_tiny_wall", "slab2:wcsph_tiny_wall"]
STEPS = 3
SPARE = 64                       # one-GPU fluid rows: room for sph_add_particles (SphConfig.fluid_capacity = the lattice's count + SPARE)
DROPPED = "dropped"
S_DELTA_TIME, S_GRAPH_LAUNCHES, S_VERLET_BUILDS, S_RIGID_ACTIVE = 0, 5, 31, 32
F_POS = 0


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def ptr(a):
    return None if a is None else a.ctypes.data


class Ctx:
    """what a variant sees: the handle, and the facts of the row's scene its arguments are made from"""

    def __init__(self, sim, cfg):
        self.sim, self.lib, self.h = sim, sim._lib, sim._h
        sc = cfg["scene"]
        self.r = float(sc["particle_radius"])
        self.lo, self.hi = np.float32(sc["box_min"]), np.float32(sc["box_max"])

    @property
    def n(self):
        self.sim._refresh_count()
        return self.sim.n_fluid

    def pos(self):
        """the fluid positions if the handle hands them out in API order (a slab handle does not: the lattice's corner stands in)"""
        out = np.zeros((self.n, 3), dtype=np.float32)
        if self.lib.sph_download(self.h, 0, F_POS, out.ctypes.data, out.size) != 0:
            out[:] = self.lo + np.float32(0.3) * (self.hi - self.lo)
        return out

    def patch(self):
        """four wall samples a particle diameter apart, one diameter above the topmost particle: near enough for a carve to remove something"""
        p = self.pos()
        top = p[int(np.argmax(p[:, 1]))]
        d = np.float32(2.0 * self.r)
        return np.ascontiguousarray([top + np.float32([a * d, d, b * d]) for a in (0, 1) for b in (0, 1)], dtype=np.float32)

    def scalar(self, which):
        out = ctypes.c_double()
        rc = self.lib.sph_get_scalar(self.h, which, ctypes.byref(out))
        return out.value if rc == 0 else float("nan")


# ---- the calls: fn(ctx) -> (return code, data or None) ----------------------------------------------------------------------------------------

def add_particles(points=1, null=False):
    def fn(c):
        n = points if points >= 0 else int(c.scalar(47)) - c.n + 1          # -1: one more than the capacity has room for
        pos = np.tile(c.lo + np.float32(0.75) * (c.hi - c.lo), (max(n, 1), 1)).astype(np.float32)
        pos[:, 0] -= np.arange(len(pos), dtype=np.float32) * np.float32(1e-3)
        first = ctypes.c_int32(-1)
        rc = c.lib.sph_add_particles(c.h, None if null else ptr(pos), None, n, ctypes.byref(first))
        return rc, np.int32([first.value])
    return fn


def remove_in_box(null=False):
    def fn(c):
        p = c.pos()[0]
        lo, hi = (p - np.float32(1.5 * c.r)).astype(np.float32), (p + np.float32(1.5 * c.r)).astype(np.float32)
        removed = ctypes.c_int32(-1)
        rc = c.lib.sph_remove_in_box(c.h, None if null else ptr(lo), ptr(hi), ctypes.byref(removed))
        return rc, np.int32([removed.value])
    return fn


def geometry_add(null=False, count=None):
    def fn(c):
        pts = c.patch()
        group = ctypes.c_int32(-1)
        rc = c.lib.sph_geometry_add(c.h, None if null else ptr(pts), len(pts) if count is None else count, ctypes.byref(group))
        return rc, np.int32([group.value])
    return fn


def geometry_remove(group):
    return lambda c: (c.lib.sph_geometry_remove(c.h, group), None)


def geometry_info(cap=8, null=None):
    def fn(c):
        g, f, k = (np.full(8, -1, dtype=np.int32) for _ in range(3))
        n = ctypes.c_size_t(99)
        rc = c.lib.sph_geometry_info(c.h, None if null == "arrays" else ptr(g), ptr(f), ptr(k), cap, None if null == "n" else ctypes.byref(n))
        return rc, np.concatenate([g, f, k, np.int32([n.value])])
    return fn


def geometry_carve(group=-1, clearance=None):
    def fn(c):
        removed = ctypes.c_int32(-1)
        rc = c.lib.sph_geometry_carve(c.h, group, float(np.float32(4.0 * c.r if clearance is None else clearance)), ctypes.byref(removed))
        return rc, np.int32([removed.value])
    return fn


def wall_counts(null=False, off=0):
    def fn(c):
        out = np.full(c.n + 1, -1, dtype=np.int32)
        return c.lib.sph_geometry_wall_counts(c.h, None if null else ptr(out), c.n + off), out[:c.n]
    return fn


def wl_select(groups, null=False, count=None):
    def fn(c):
        ids = np.ascontiguousarray(groups, dtype=np.int32)
        return c.lib.sph_wall_load_select(c.h, None if null else ptr(ids), len(ids) if count is None else count), None
    return fn


def wl_get(group=0, null=False, about=None):
    def fn(c):
        f, t = np.zeros(3), np.zeros(3)
        a = None if about is None else np.float64(about)
        return c.lib.sph_wall_load_get(c.h, group, ptr(a), None if null else ptr(f), ptr(t)), np.concatenate([f, t])
    return fn


def wl_impulse(group=0, null=False, reset=1):
    def fn(c):
        j, l, sec = np.zeros(3), np.zeros(3), ctypes.c_double(-1.0)
        rc = c.lib.sph_wall_load_impulse(c.h, group, None, None if null else ptr(j), ptr(l), ctypes.byref(sec), reset)
        return rc, np.concatenate([j, l, [sec.value]])
    return fn


def wl_forces(group=0, null=False, off=0):
    def fn(c):
        n = 3 * c.sim.n_wall
        out = np.zeros(n + 3, dtype=np.float32)
        return c.lib.sph_wall_load_forces(c.h, group, None if null else ptr(out), n + off), out[:n]
    return fn


def scalar_enable(d=1e-3, beta=0.0, ref=1.0):
    return lambda c: (c.lib.sph_scalar_enable(c.h, d, beta, ref), None)


def scalar_disable():
    return lambda c: (c.lib.sph_scalar_disable(c.h), None)


def scalar_upload(null=False, off=0):
    def fn(c):
        v = np.linspace(0.0, 2.0, c.n + 1, dtype=np.float32)
        return c.lib.sph_scalar_upload(c.h, None if null else ptr(v), c.n + off), None
    return fn


def scalar_download(null=False, off=0):
    def fn(c):
        v = np.zeros(c.n + 1, dtype=np.float32)
        return c.lib.sph_scalar_download(c.h, None if null else ptr(v), c.n + off), v[:c.n]
    return fn


def scalar_rate(null=False, off=0):
    def fn(c):
        v = np.zeros(c.n + 1, dtype=np.float32)
        return c.lib.sph_scalar_rate(c.h, None if null else ptr(v), c.n + off), v[:c.n]
    return fn


def scalar_inflow(value):
    return lambda c: (c.lib.sph_scalar_set_inflow(c.h, value), None)


DERIVED_WIDTH = {0: 9, 1: 3, 2: 1, 3: 3, 4: 1}


def derived(which, null=False, off=0):
    def fn(c):
        n = DERIVED_WIDTH.get(which, 1) * c.n
        out = np.zeros(n + 1, dtype=np.float32)
        return c.lib.sph_derived(c.h, which, None if null else ptr(out), n + off), out[:n]
    return fn


def diagnostics(null=False):
    def fn(c):
        row = np.zeros(32, dtype=np.float64)
        return c.lib.sph_diagnostics(c.h, None if null else ptr(row)), row
    return fn


def diag_record(every, rows):
    return lambda c: (c.lib.sph_diag_record(c.h, every, rows), None)


def diag_read(null=False, cap=8):
    def fn(c):
        out = np.zeros((8, 32), dtype=np.float64)
        n, total = ctypes.c_size_t(99), ctypes.c_int64(-1)
        rc = c.lib.sph_diag_read(c.h, ptr(out), cap, None if null else ctypes.byref(n), ctypes.byref(total))
        return rc, np.concatenate([out.ravel(), [float(n.value), float(total.value)]])
    return fn


def rigid_set_active(flip=True):
    return lambda c: (c.lib.sph_rigid_set_active(c.h, int(c.scalar(S_RIGID_ACTIVE) == 0.0) if flip else 1), None)


def rigid_init_data():
    return lambda c: (c.lib.sph_rigid_init_data(c.h), None)


def rigid_set_mode(mode):
    return lambda c: (c.lib.sph_rigid_set_mode(c.h, mode), None)


def rigid_set_motion(null=False, nan=False):
    def fn(c):
        vel, om = np.float32([0.1, 0.0, float("nan") if nan else 0.0]), np.float32([0.0, 0.5, 0.0])
        return c.lib.sph_rigid_set_motion(c.h, None if null else ptr(vel), ptr(om), None, None), None
    return fn


def rigid_get_load(null=False):
    def fn(c):
        f, t = np.zeros(3), np.zeros(3)
        return c.lib.sph_rigid_get_load(c.h, None if null else ptr(f), ptr(t)), np.concatenate([f, t])
    return fn


def set_gravity(vec):
    def fn(c):
        g = None if vec is None else np.float32(vec)
        return c.lib.sph_set_gravity(c.h, ptr(g)), None
    return fn


def set_forcing(amp, omega=(30.0, 30.0, 30.0)):
    def fn(c):
        a, w = (None if amp is None else np.float64(amp)), np.float64(omega)
        return c.lib.sph_set_forcing(c.h, ptr(a), ptr(w), None), None
    return fn


def set_scalar(which, value=None, scale=None):
    """value, or scale x the scalar as it stands"""
    return lambda c: (c.lib.sph_set_scalar(c.h, which, float(value) if scale is None else scale * c.scalar(which)), None)


class Call:
    """name: the entry point (and, after ':', what distinguishes this scenario); prep: calls made first on a handle of the scenario's own (the feature
    is enabled); variants: (label, fn) in order, the valid one last; stale: the valid variant edits the handle; after: (label, fn) made behind the
    steps that follow an edit"""

    def __init__(self, name, variants, prep=(), stale=False, after=()):
        self.name, self.variants, self.prep, self.stale, self.after = name, list(variants), list(prep), stale, list(after)


NAN = float("nan")
ADD, SELECT, ENABLE = ("geometry_add", geometry_add()), ("wall_load_select", wl_select([0])), ("scalar_enable", scalar_enable())
CALLS = [
    # inlets and sinks
    Call("sph_add_particles", [("null", add_particles(null=True)), ("count", add_particles(points=-1)), ("none", add_particles(points=0)), ("valid", add_particles())], stale=True),
    Call("sph_remove_in_box", [("null", remove_in_box(null=True)), ("valid", remove_in_box())], stale=True),
    # static geometry
    Call("sph_geometry_remove:before", [("valid", geometry_remove(1))]),
    Call("sph_geometry_info:before", [("null_n", geometry_info(null="n")), ("null_arrays", geometry_info(null="arrays")), ("valid", geometry_info())]),
    Call("sph_geometry_carve:before", [("group", geometry_carve(group=1)), ("valid", geometry_carve())]),
    Call("sph_geometry_wall_counts", [("null", wall_counts(null=True)), ("count", wall_counts(off=-1)), ("valid", wall_counts())]),
    Call("sph_geometry_add", [("null", geometry_add(null=True)), ("count", geometry_add(count=0)), ("valid", geometry_add())], stale=True,
         after=[("sph_geometry_info", geometry_info()), ("sph_geometry_wall_counts", wall_counts())]),
    Call("sph_geometry_remove", [("group", geometry_remove(99)), ("valid", geometry_remove(1))], prep=[ADD], stale=True, after=[("sph_geometry_info", geometry_info())]),
    Call("sph_geometry_info", [("count", geometry_info(cap=0)), ("valid", geometry_info())], prep=[ADD]),
    Call("sph_geometry_carve", [("clearance", geometry_carve(clearance=0.0)), ("group", geometry_carve(group=99)), ("valid", geometry_carve())], prep=[ADD], stale=True),
    # loads on walls and geometry
    Call("sph_wall_load_get:before", [("valid", wl_get())]),
    Call("sph_wall_load_impulse:before", [("valid", wl_impulse())]),
    Call("sph_wall_load_forces:before", [("valid", wl_forces())]),
    Call("sph_wall_load_select", [("null", wl_select([0], null=True)), ("count", wl_select([0] * 1025)), ("group", wl_select([7])), ("twice", wl_select([0, 0])), ("valid", wl_select([0]))],
         stale=True, after=[("sph_wall_load_get", wl_get()), ("sph_wall_load_get:about", wl_get(group=-1, about=(0.5, 0.5, 0.5))), ("sph_wall_load_forces", wl_forces()),
                            ("sph_wall_load_impulse:keep", wl_impulse(reset=0))]),
    Call("sph_wall_load_select:off", [("valid", wl_select([], null=True))], prep=[SELECT], stale=True),
    Call("sph_wall_load_select:geometry", [("valid", wl_select([1, 0]))], prep=[ADD], stale=True, after=[("sph_wall_load_forces", wl_forces(group=0)), ("sph_wall_load_get", wl_get(group=1))]),
    Call("sph_geometry_add:measured", [("valid", geometry_add())], prep=[SELECT], stale=True, after=[("sph_wall_load_get", wl_get())]),
    Call("sph_wall_load_get", [("null", wl_get(null=True)), ("group", wl_get(group=5)), ("valid", wl_get())], prep=[SELECT]),
    Call("sph_wall_load_impulse", [("null", wl_impulse(null=True)), ("valid", wl_impulse())], prep=[SELECT], stale=True, after=[("sph_wall_load_impulse", wl_impulse())]),
    Call("sph_wall_load_forces", [("null", wl_forces(null=True)), ("count", wl_forces(off=-3)), ("all", wl_forces(group=-1)), ("valid", wl_forces())], prep=[SELECT]),
    # the carried scalar
    Call("sph_scalar_disable:before", [("valid", scalar_disable())]),
    Call("sph_scalar_upload:before", [("null", scalar_upload(null=True)), ("valid", scalar_upload())]),
    Call("sph_scalar_download:before", [("null", scalar_download(null=True)), ("valid", scalar_download())]),
    Call("sph_scalar_set_inflow:before", [("valid", scalar_inflow(2.0))]),
    Call("sph_scalar_rate:before", [("valid", scalar_rate())]),
    Call("sph_scalar_enable", [("negative", scalar_enable(d=-1.0)), ("nan", scalar_enable(beta=NAN)), ("valid", scalar_enable(beta=0.5))], stale=True,
         after=[("sph_scalar_download", scalar_download()), ("sph_scalar_rate", scalar_rate())]),
    Call("sph_scalar_enable:again", [("valid", scalar_enable(d=2e-3))], prep=[ENABLE], stale=True),
    Call("sph_scalar_disable", [("valid", scalar_disable())], prep=[ENABLE], stale=True, after=[("sph_scalar_download", scalar_download())]),
    Call("sph_scalar_upload", [("null", scalar_upload(null=True)), ("count", scalar_upload(off=1)), ("valid", scalar_upload())], prep=[ENABLE], stale=True,
         after=[("sph_scalar_download", scalar_download())]),
    Call("sph_scalar_download", [("null", scalar_download(null=True)), ("count", scalar_download(off=-1)), ("valid", scalar_download())], prep=[ENABLE]),
    Call("sph_scalar_set_inflow", [("nan", scalar_inflow(NAN)), ("valid", scalar_inflow(2.0))], prep=[ENABLE], stale=True),
    Call("sph_scalar_rate", [("null", scalar_rate(null=True)), ("count", scalar_rate(off=1)), ("valid", scalar_rate()), ("valid_again", scalar_rate())], prep=[ENABLE]),
    Call("sph_add_particles:scalar", [("valid", add_particles(points=3))], prep=[ENABLE], stale=True, after=[("sph_scalar_download", scalar_download())]),
    Call("sph_remove_in_box:scalar", [("valid", remove_in_box())], prep=[ENABLE, ("sph_scalar_upload", scalar_upload())], stale=True, after=[("sph_scalar_download", scalar_download())]),
    # derived per-particle fields
    Call("sph_derived", [("null", derived(1, null=True)), ("count", derived(1, off=1)), ("unknown", derived(9))] + [("valid_%d" % q, derived(q)) for q in range(5)] + [("valid_again", derived(0))]),
    # run diagnostics
    Call("sph_diagnostics", [("null", diagnostics(null=True)), ("valid", diagnostics())]),
    Call("sph_diag_read:before", [("null", diag_read(null=True)), ("valid", diag_read())]),
    Call("sph_diag_record", [("negative", diag_record(-1, 8)), ("rows", diag_record(1, 0)), ("valid", diag_record(1, 8))], stale=True,
         after=[("sph_diag_read:null", diag_read(null=True)), ("sph_diag_read:count", diag_read(cap=2)), ("sph_diag_read", diag_read()), ("sph_diagnostics", diagnostics())]),
    Call("sph_diag_record:stop", [("valid", diag_record(0, 0))], prep=[("sph_diag_record", diag_record(2, 4))], stale=True, after=[("sph_diag_read", diag_read())]),
    # the body
    Call("sph_rigid_get_load", [("null", rigid_get_load(null=True)), ("valid", rigid_get_load())]),
    Call("sph_rigid_set_active", [("valid", rigid_set_active())], stale=True, after=[("sph_rigid_get_load", rigid_get_load())]),
    Call("sph_rigid_init_data", [("valid", rigid_init_data())], stale=True),
    Call("sph_rigid_set_mode", [("unknown", rigid_set_mode(7)), ("valid", rigid_set_mode(2))], stale=True, after=[("sph_rigid_get_load", rigid_get_load())]),
    Call("sph_rigid_set_motion", [("null", rigid_set_motion(null=True)), ("nan", rigid_set_motion(nan=True)), ("valid", rigid_set_motion())], prep=[("sph_rigid_set_mode", rigid_set_mode(1))], stale=True,
         after=[("sph_rigid_get_load", rigid_get_load())]),
    # gravity, forcing, delta_time and the solver attributes
    Call("sph_set_gravity", [("null", set_gravity(None)), ("nan", set_gravity((0.0, NAN, 0.0))), ("valid", set_gravity((0.5, -9.0, 0.25)))], stale=True),
    Call("sph_set_forcing", [("nan", set_forcing((0.0, NAN, 0.0))), ("valid", set_forcing((0.0, 1.0, 0.0)))], stale=True),
    Call("sph_set_forcing:off", [("valid", set_forcing(None))], prep=[("sph_set_forcing", set_forcing((0.0, 1.0, 0.0)))], stale=True),
    Call("sph_set_scalar:delta_time", [("negative", set_scalar(S_DELTA_TIME, -1.0)), ("valid", set_scalar(S_DELTA_TIME, scale=0.5))], stale=True),
    Call("sph_set_scalar:unknown", [("valid", set_scalar(63, 1.0))]),
    Call("sph_set_scalar:min_iteration_density", [("fraction", set_scalar(65, 2.5)), ("valid", set_scalar(65, 3))], stale=True),                # an iteration count
    Call("sph_set_scalar:density_threshold", [("nan", set_scalar(64, NAN)), ("valid", set_scalar(64, 0.05))], stale=True),                      # a finite value
    Call("sph_set_scalar:warm_start", [("valid", set_scalar(69, 0))], stale=True),                                                              # a truth value
    Call("sph_set_scalar:max_dt", [("negative", set_scalar(71, -1.0)), ("valid", set_scalar(71, 5e-4))], stale=True),                           # a value > 0
    Call("sph_set_scalar:viscosity_alpha", [("nan", set_scalar(74, NAN)), ("valid", set_scalar(74, 0.05))], stale=True),                        # a fluid attribute
    Call("sph_set_scalar:step_adaptive_dt", [("fraction", set_scalar(77, 0.5)), ("valid", set_scalar(77, 1))], stale=True),                     # the adaptive time step
    Call("sph_set_scalar:step_max_dt", [("negative", set_scalar(78, -1.0)), ("valid", set_scalar(78, scale=0.5))], prep=[("sph_set_scalar", set_scalar(77, 1))], stale=True),
]


# ---- the rows' handles ------------------------------------------------------------------------------------------------------------------------

class OneGpu:
    """a row on one handle; .fresh(steps) is another handle of the same scene, that many steps on"""
    world = 1

    def __init__(self, nat, name):
        from cfd_taichi_amd import mesh, scenes
        self.nat = nat
        self.arith = nat.ARITH_RELAXED if name.startswith("relaxed:") else nat.ARITH_EXACT
        scene = name.split(":")[-1]
        self.cfg = copy.deepcopy(scenes.get(scene))
        self.rigid = mesh.rigid_from_config(self.cfg) if scene == "dfsph_rigid_small" else None
        if self.rigid is None:
            probe = self.make()
            self.cfg["fluid"]["capacity"] = probe.n_fluid + SPARE
            probe.close()

    def make(self):
        return self.nat.Simulation(self.nat.config_from_dict(self.cfg, arith=self.arith), rigid=self.rigid)

    def fresh(self, steps):
        sims = [self.make()]
        self.step(sims, steps)
        return sims

    def each(self, sims, fn):
        return [fn(s) for s in sims]

    def step(self, sims, n):
        if self.rigid is None:
            if n:
                sims[0].step(n)           # one call: a wcsph handle captures and replays its step pairs
            return
        for _ in range(n):
            sims[0].step(1)
            sims[0].rigid_step()

    def pos(self, sims):
        out = []
        for s in sims:
            s._refresh_count()
            out.append(sha(s.download(F_POS)))
        return out

    def close(self, sims):
        for s in sims:
            s.close()


class Slabs(OneGpu):
    """the same over two slab handles on the loopback transport: a call is made on both ranks at once, steps are collective"""
    world = 2

    def __init__(self, nat, name):
        from cfd_taichi_amd import scenes
        from slab_ranks import Ranks
        self.nat, self.cfg, self.rigid, self.Ranks = nat, scenes.get(name.split(":")[-1]), None, Ranks
        self.groups = {}

    def fresh(self, steps):
        g = self.Ranks(self.nat, self.cfg, 2)
        self.groups[id(g.sims)] = g
        self.step(g.sims, steps)
        return g.sims

    def each(self, sims, fn):
        return self.groups[id(sims)].each(lambda r, s: fn(s))

    def step(self, sims, n):
        for _ in range(n):
            self.groups[id(sims)].step()

    def pos(self, sims):
        out = []
        for s in sims:
            ids, vals = s.download_owned(F_POS)
            order = np.argsort(ids, kind="stable")
            out.append(sha(np.concatenate([ids[order].astype(np.float32)[:, None], vals[order]], axis=1)))
        return out

    def close(self, sims):
        self.groups.pop(id(sims)).close()


def entry(ctx, fn):
    rc, data = fn(ctx)
    err = (ctx.lib.sph_last_error(ctx.h) or b"").decode() if rc else ""
    return [rc, err] + ([sha(data)] if rc == 0 and data is not None else [])


def make_calls(row, sims, fns):
    """{label: one entry per rank} of the (label, fn) in order, every fn on all ranks at once"""
    out = {}
    for label, fn in fns:
        out[label] = row.each(sims, lambda s: entry(Ctx(s, row.cfg), fn))
    return out


def staleness(row, sims):
    try:
        return followed(row, sims)
    except row.nat.SphError as e:          # a step the library refuses after the edit (a scripted body about to leave the grid): a host decision like the others
        return {"refused": [e.code, str(e)]}


def followed(row, sims):
    row.each(sims, lambda s: (s.profile_reset(), s.profile_enable(True)))
    row.step(sims, STEPS)
    out = {"launches": row.each(sims, lambda s: {k: n for k, (ms, n) in sorted(s.profile().items())}), "pos": row.pos(sims)}
    row.each(sims, lambda s: s.profile_enable(False))
    for key, which in (("graph_launches", S_GRAPH_LAUNCHES), ("verlet_builds", S_VERLET_BUILDS)):
        out[key] = row.each(sims, lambda s: s.scalar(which))
    row.step(sims, STEPS)
    out["tail"] = {"pos": row.pos(sims), "graph_launches": row.each(sims, lambda s: s.scalar(S_GRAPH_LAUNCHES)), "verlet_builds": row.each(sims, lambda s: s.scalar(S_VERLET_BUILDS))}
    return out


def phase(row, steps):
    out = {}
    shared = row.fresh(steps)
    for call in CALLS:
        own = bool(call.prep) or call.stale
        sims = row.fresh(steps) if own else shared
        res = {}
        if call.prep:
            res["prep"] = make_calls(row, sims, call.prep)
        res["variants"] = make_calls(row, sims, call.variants)
        if call.stale and all(e[0] == 0 for e in res["variants"][call.variants[-1][0]]):
            res["stale"] = staleness(row, sims)
            if call.after and "refused" not in res["stale"]:
                res["after"] = make_calls(row, sims, call.after)
        out[call.name] = res
        if own:
            row.close(sims)
    row.close(shared)
    return out


def record(name):
    """the matrix row `name` of the library that cfd_taichi_amd._native loads"""
    if name.startswith("slab2:"):
        from slab_ranks import loopback_env
        loopback_env()
    from cfd_taichi_amd import _native as nat
    row = Slabs(nat, name) if name.startswith("slab2:") else OneGpu(nat, name)
    return {"before_first_step": phase(row, 0), "after_%d_steps" % STEPS: phase(row, STEPS)}


# ---- two recordings into one fixture ------------------------------------------------------------------------------------------------------------

def is_entry(x):
    return isinstance(x, list) and len(x) in (2, 3) and isinstance(x[0], int) and isinstance(x[1], str)


def merge(a, b, path, dropped, counted):
    """a where the two recordings agree; DROPPED for a digest or count that differs; a code or text that differs is an error"""
    if is_entry(a) and is_entry(b):
        if a[:2] != b[:2] or len(a) != len(b):
            raise SystemExit("%s: a return code or message differs between two recordings of one library: %r != %r" % (path, a, b))
        if len(a) == 3:
            counted[0] += 1
            if a[2] != b[2]:
                dropped.append(path)
                return a[:2] + [DROPPED]
        return a
    if isinstance(a, dict) and isinstance(b, dict) and sorted(a) == sorted(b):
        return {k: merge(a[k], b[k], "%s/%s" % (path, k), dropped, counted) for k in a}
    if isinstance(a, list) and isinstance(b, list) and len(a) == len(b):
        return [merge(x, y, "%s[%d]" % (path, k), dropped, counted) for k, (x, y) in enumerate(zip(a, b))]
    if isinstance(a, (dict, list)) or isinstance(b, (dict, list)):
        raise SystemExit("%s: the two recordings differ in shape" % path)
    counted[0] += 1
    if a != b:
        dropped.append(path)
        return DROPPED
    return a


# ---- the fixture file: every distinct subtree once ----------------------------------------------------------------------------------------------
# The matrix repeats itself: the same refusal text on every row, the same launch counts after most edits, whole call results shared by rows and
# phases.  The file therefore holds a table of the distinct values -- long strings, long lists and every dict below a phase, one per line, a value
# inside another written as "#<its line in the table>" -- and the rows' phases as {call: "#n"}.  load() gives back the plain nested matrix.

def dump(matrix, path):
    table, index = [], {}

    def put(v):
        text = json.dumps(v, sort_keys=True, separators=(",", ":"))
        if text not in index:
            index[text] = len(table)
            table.append(text)
        return "#%d" % index[text]

    def pack(x):
        if isinstance(x, dict):
            return put({k: pack(v) for k, v in x.items()})
        if isinstance(x, list):
            v = [pack(c) for c in x]
            return put(v) if len(json.dumps(v)) > 24 else v
        if isinstance(x, str):
            assert not x.startswith("#"), x
            return put(x) if len(x) > 8 else x
        return x
    rows = {name: {ph: {call: pack(res) for call, res in calls.items()} for ph, calls in phases.items()} for name, phases in matrix.items()}
    with open(path, "w") as f:
        f.write('{"table": [\n%s\n],\n"rows": {\n%s\n}}\n' % (",\n".join(table), ",\n".join(
            "%s: %s" % (json.dumps(name), json.dumps(rows[name], sort_keys=True, separators=(",", ":"))) for name in sorted(rows))))


def load(path):
    with open(path) as f:
        packed = json.load(f)
    table = packed["table"]

    def unpack(x):
        if isinstance(x, dict):
            return {k: unpack(v) for k, v in x.items()}
        if isinstance(x, list):
            return [unpack(v) for v in x]
        if isinstance(x, str) and x.startswith("#"):
            return unpack(table[int(x[1:])])
        return x
    return unpack(packed["rows"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--row", action="append", help="a row of ROWS (default: all, each recorded twice in processes of their own)")
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    if args.row and len(args.row) == 1:
        result = {args.row[0]: json.loads(json.dumps(record(args.row[0])))}
    else:
        import subprocess
        import tempfile
        result, dropped, counted = {}, [], [0]
        for name in args.row or ROWS:
            twice = []
            for _ in range(2):
                with tempfile.TemporaryDirectory() as tmp:
                    part = os.path.join(tmp, "row.json")
                    subprocess.run([sys.executable, os.path.abspath(__file__), "--row", name, "--out", part], check=True, cwd=ROOT, timeout=600)
                    with open(part) as f:
                        twice.append(json.load(f)[name])
            result[name] = merge(twice[0], twice[1], name, dropped, counted)
            print("%s: recorded twice, %d digests and counts so far, %d dropped" % (name, counted[0], len(dropped)), flush=True)
        for path in dropped:
            print("dropped (differs between two recordings of one library): %s" % path)
        if len(dropped) * 100 > counted[0]:
            raise SystemExit("%d of %d digests and counts differ between two recordings: more than 1 %%, the scenario is wrong" % (len(dropped), counted[0]))
    dump(result, args.out)


if __name__ == "__main__":
    main()
