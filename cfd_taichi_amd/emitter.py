"""Fluid inlets and sinks on a live handle: `Emitter` feeds layers of particles through a rectangular opening, `Sink` removes what enters a
box.  Pure host Python on top of two calls of the library (sph_add_particles, sph_remove_in_box): all either class needs
from a simulation is `.time()`, `.n_fluid`, `.capacity`, `.add_particles(pos, vel)` and `.remove_in_box(lo, hi)` -- a `_native.Simulation`
created with a `fluid.capacity`, or anything with those five.

    sim = Simulation(config_from_dict(config))           # config["fluid"]["capacity"] = the most particles the run will hold
    emitters, sinks = emitter.from_config(config)         # scene.emitters / scene.sinks
    while ...:
        sim.step()
        emitter.apply(sim, emitters, sinks)               # the sinks, then the emitters

Neither class tests for overlap with the fluid already there (nor do the emitters of other SPH codes): an emitter that points into standing
fluid, or whose `speed` is too low to clear its own opening, puts particles on top of particles, and the pressure solver answers with a
burst.  Place the opening clear of the fluid and give the jet a speed of at least a particle diameter per few steps.
"""
import math

import numpy as np


def _vec3(value, what):
    a = np.asarray(value, dtype=np.float64).reshape(-1)
    if a.shape != (3,) or not np.isfinite(a).all():
        raise ValueError("%s must be three finite numbers, got %r" % (what, value))
    return a


class Sink:
    """Removes every particle with box_min <= x < box_max on all three axes (f32 compares on the device)."""

    def __init__(self, box_min, box_max):
        self.box_min, self.box_max = _vec3(box_min, "box_min"), _vec3(box_max, "box_max")
        self.removed = 0          # particles removed so far

    def apply(self, sim):
        """one remove_in_box; returns the number removed.  A box that holds every particle is refused by the library (no empty handle)."""
        n = int(sim.remove_in_box(self.box_min, self.box_max))
        self.removed += n
        return n


class Emitter:
    """A rectangular opening of `size` = (w, h) centred on `center` that feeds fluid along `direction` at `speed`.

    d = 2 radius.  u = direction x y^ normalised (direction x x^ where the direction is parallel to y^), v = direction x u.  A layer is the
    floor(w / d) x floor(h / d) lattice (at least 1 x 1) of spacing d centred on `center` in the (u, v) plane.  Layer k is due at
    t_k = start + k d / speed: consecutive layers are a diameter apart along the jet.  `update(sim)` reads t = sim.time() once and emits, in one
    add_particles call, every layer with t_k < min(t, stop) that has not been emitted yet, each advanced by speed (t - t_k) along the direction
    -- where it would be had it left the opening at t_k -- with the velocity speed * direction.  All of it in f64, rounded to f32 once.
    A layer that would exceed the simulation's capacity or `max_particles` ends the emitter (`exhausted`); partial layers are never emitted.
    `scalar`: the carried scalar of what it pours in (add_particles(pos, vel, scalar=v); the simulation's scalar must be enabled); None: the
    simulation's inflow value.
    """

    def __init__(self, center, direction, size, speed, start=0.0, stop=math.inf, max_particles=None, radius=None, scalar=None):
        if radius is None or not (float(radius) > 0.0):
            raise ValueError("Emitter needs radius > 0 (from_config passes scene.particle_radius)")
        self.center = _vec3(center, "center")
        n = _vec3(direction, "direction")
        length = math.sqrt(float(n @ n))
        if not (length > 0.0):
            raise ValueError("direction must not be the zero vector")
        self.direction = n / length
        size = np.asarray(size, dtype=np.float64).reshape(-1)
        if size.shape != (2,) or not np.isfinite(size).all() or not (size > 0).all():
            raise ValueError("size must be two positive numbers (w, h), got %r" % (size,))
        self.size = size
        self.speed, self.start, self.stop = float(speed), float(start), float(stop)
        if not (self.speed > 0.0) or not math.isfinite(self.speed) or not math.isfinite(self.start) or math.isnan(self.stop):
            raise ValueError("speed must be finite and > 0, start finite, stop a number or inf")
        self.max_particles = None if max_particles is None else int(max_particles)
        self.scalar = None if scalar is None else float(scalar)
        if self.scalar is not None and not math.isfinite(self.scalar):
            raise ValueError("scalar must be a finite number, got %r" % (scalar,))
        self.radius = float(radius)
        self.d = 2.0 * self.radius
        y, x = np.array([0.0, 1.0, 0.0]), np.array([1.0, 0.0, 0.0])
        u = np.cross(self.direction, y)
        if float(u @ u) < 1e-24:                       # the direction is parallel to y^
            u = np.cross(self.direction, x)
        self.u = u / math.sqrt(float(u @ u))
        self.v = np.cross(self.direction, self.u)
        # (the 1e-9: 0.3 / 0.1 is 2.9999999999999996 in f64, and an opening of three diameters holds three particles)
        self.nu = max(1, int(math.floor(self.size[0] / self.d + 1e-9)))
        self.nv = max(1, int(math.floor(self.size[1] / self.d + 1e-9)))
        iu = (np.arange(self.nu, dtype=np.float64) - 0.5 * (self.nu - 1)) * self.d
        iv = (np.arange(self.nv, dtype=np.float64) - 0.5 * (self.nv - 1)) * self.d
        self.layer = (self.center[None, None, :] + iu[:, None, None] * self.u[None, None, :] + iv[None, :, None] * self.v[None, None, :]).reshape(-1, 3)
        self.layers_emitted = 0
        self.emitted = 0           # particles emitted so far
        self.exhausted = False

    @property
    def layer_size(self):
        return self.nu * self.nv

    def due_time(self, k):
        """t_k: when layer k leaves the opening"""
        return self.start + k * self.d / self.speed

    def layers_due(self, t):
        """the number of layers with t_k < min(t, stop): what update(sim) has emitted once sim.time() == t, capacity and max_particles permitting"""
        end = min(float(t), self.stop)
        k = max(0, int(math.floor((end - self.start) * self.speed / self.d)) - 1)
        while self.due_time(k) < end:                 # (the estimate may sit a layer or two low: settle it on due_time itself)
            k += 1
        return k

    def update(self, sim, t=None):
        """emit what is due at t = sim.time() (read once; `apply` reads it once for all emitters of a scene); returns the number of particles added"""
        if self.exhausted:
            return 0
        t = float(sim.time() if t is None else t)
        end = min(t, self.stop)
        room = int(sim.capacity) - int(sim.n_fluid)
        if self.max_particles is not None:
            room = min(room, self.max_particles - self.emitted)
        rows = []
        k = self.layers_emitted
        while self.due_time(k) < end:
            if (len(rows) + 1) * self.layer_size > room:
                self.exhausted = True
                break
            rows.append(self.layer + (self.speed * (t - self.due_time(k))) * self.direction[None, :])
            k += 1
        if not rows:
            return 0
        pos = np.concatenate(rows).astype(np.float32)
        vel = np.broadcast_to((self.speed * self.direction).astype(np.float32), pos.shape)
        if self.scalar is None:
            sim.add_particles(pos, np.ascontiguousarray(vel))
        else:
            sim.add_particles(pos, np.ascontiguousarray(vel), scalar=self.scalar)
        self.layers_emitted = k
        self.emitted += len(pos)
        return len(pos)


_EMITTER_KEYS = {"center", "direction", "size", "speed", "start", "stop", "max_particles", "radius", "scalar"}


def from_config(config):
    """(emitters, sinks) of a config dict: `scene.emitters` is a list of Emitter's keyword dicts (`radius` defaults to scene.particle_radius),
    `scene.sinks` a list of {"box_min": [...], "box_max": [...]}.  Both keys are optional."""
    scene = config["scene"]
    emitters, sinks = [], []
    for e in scene.get("emitters", []) or []:
        if not isinstance(e, dict) or set(e) - _EMITTER_KEYS or not {"center", "direction", "size", "speed"} <= set(e):
            raise ValueError("scene.emitters: each entry needs center, direction, size, speed (optional: start, stop, max_particles, radius, scalar), got %r" % (e,))
        kw = dict(e)
        kw.setdefault("radius", scene["particle_radius"])
        emitters.append(Emitter(**kw))
    for s in scene.get("sinks", []) or []:
        if not isinstance(s, dict) or set(s) != {"box_min", "box_max"}:
            raise ValueError("scene.sinks: each entry is {\"box_min\": [...], \"box_max\": [...]}, got %r" % (s,))
        sinks.append(Sink(s["box_min"], s["box_max"]))
    return emitters, sinks


def apply(sim, emitters, sinks):
    """after a solver step: the sinks, then the emitters.  Returns (removed, added)."""
    removed = sum(s.apply(sim) for s in sinks)
    live = [e for e in emitters if not e.exhausted]
    t = sim.time() if live else None              # one clock read per step, and only where something may still be emitted
    added = sum(e.update(sim, t) for e in live)
    return removed, added
