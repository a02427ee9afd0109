"""Static geometry for a handle's wall set: deterministic samplers that turn a box, a parallelogram, a sphere or a mesh
into wall sample positions, and the `scene.geometry` block of a config.  Pure host Python: numpy in, (n, 3) float32 out, in a documented order;
the same arguments give the same bytes.  `Simulation.add_geometry(points)` takes what the samplers return.

A single layer of samples at the particle spacing is what the tank box itself is; like the box it leaks under enough pressure.  A closed shell
keeps the lattice fluid that starts inside it: sample a mesh with fill=True, or carve (`Simulation.carve`)."""
import math

import numpy as np


def _vec(value, what):
    v = np.asarray(value, dtype=np.float64).reshape(-1)
    if v.shape != (3,) or not np.isfinite(v).all():
        raise ValueError("%s must be three finite numbers, got %r" % (what, value))
    return v


def _spacing(spacing):
    s = float(spacing)
    if not (s > 0 and math.isfinite(s)):
        raise ValueError("spacing must be a positive finite number, got %r" % (spacing,))
    return s


def _intervals(length, spacing):
    """the number of equal intervals nearest to length / spacing (0 for a degenerate edge)"""
    return int(round(length / spacing + 1e-9))


def plate(origin, u, v, spacing):
    """The parallelogram origin + s u + t v, 0 <= s, t <= 1, as (nu + 1)(nv + 1) samples: nu = round(|u| / spacing) equal intervals along u, nv
    likewise along v (so the pitch is the nearest to `spacing` that ends on the far edges).  Order: the index along u outermost.  Ramps and gates
    are plates."""
    o, u, v, sp = _vec(origin, "origin"), _vec(u, "u"), _vec(v, "v"), _spacing(spacing)
    nu, nv = _intervals(np.linalg.norm(u), sp), _intervals(np.linalg.norm(v), sp)
    s = np.arange(nu + 1, dtype=np.float64) / max(nu, 1)
    t = np.arange(nv + 1, dtype=np.float64) / max(nv, 1)
    pts = o[None, None, :] + s[:, None, None] * u[None, None, :] + t[None, :, None] * v[None, None, :]
    return np.ascontiguousarray(pts.reshape(-1, 3), dtype=np.float32)


def box_shell(lo, hi, spacing):
    """The surface lattice of the axis-aligned box [lo, hi]: per axis n = round((hi - lo) / spacing) equal intervals, the points lo + (i, j, k) *
    (hi - lo) / n with at least one index on a face.  Order: C order of (i, j, k), x slowest."""
    lo, hi, sp = _vec(lo, "lo"), _vec(hi, "hi"), _spacing(spacing)
    if not (hi >= lo).all():
        raise ValueError("box_shell: hi must not lie below lo, got %r, %r" % (lo.tolist(), hi.tolist()))
    n = [_intervals(hi[a] - lo[a], sp) for a in range(3)]
    idx = np.stack(np.meshgrid(*[np.arange(k + 1) for k in n], indexing="ij"), axis=-1).reshape(-1, 3)
    face = np.zeros(len(idx), dtype=bool)
    for a in range(3):
        face |= (idx[:, a] == 0) | (idx[:, a] == n[a])
    step = np.array([(hi[a] - lo[a]) / max(n[a], 1) for a in range(3)])
    return np.ascontiguousarray(lo[None, :] + idx[face] * step[None, :], dtype=np.float32)


def sphere_shell(centre, radius, spacing):
    """n = max(4, round(4 pi r^2 / spacing^2)) samples on the sphere along the Fibonacci spiral (one sample per spacing^2 of surface): sample k at
    height z = 1 - (2 k + 1) / n and longitude k * pi (3 - sqrt 5).  Order: k ascending, top to bottom."""
    c, sp = _vec(centre, "centre"), _spacing(spacing)
    r = float(radius)
    if not (r > 0 and math.isfinite(r)):
        raise ValueError("radius must be a positive finite number, got %r" % (radius,))
    n = max(4, int(round(4.0 * math.pi * r * r / (sp * sp))))
    k = np.arange(n, dtype=np.float64)
    z = 1.0 - (2.0 * k + 1.0) / n
    rho = np.sqrt(np.maximum(0.0, 1.0 - z * z))
    phi = k * (math.pi * (3.0 - math.sqrt(5.0)))
    pts = c[None, :] + r * np.stack([rho * np.cos(phi), rho * np.sin(phi), z], axis=1)
    return np.ascontiguousarray(pts, dtype=np.float32)


def mesh_samples(path, spacing, scale=1, translate=(0, 0, 0), fill=False):
    """A mesh (STL / OBJ: mesh.load_mesh) scaled, then voxelised at pitch `spacing` (mesh.voxelize: voxel centres on the lattice {k * spacing} of
    the scaled mesh's frame, in C order of the voxel index), then translated.  fill=False: the surface shell; fill=True: the solid."""
    from . import mesh
    sp, t = _spacing(spacing), _vec(translate, "translate")
    vertices, faces = mesh.load_mesh(mesh._resolve(path))
    pts = mesh.voxelize(vertices * float(scale), faces, sp, fill=bool(fill))
    return np.ascontiguousarray(pts + t[None, :], dtype=np.float32)


# ---- the `scene.geometry` block of a config -------------------------------------------------------------------------------------------------
TYPES = {"box": {"min", "max"}, "plate": {"origin", "u", "v"}, "sphere": {"centre", "radius"}, "mesh": {"mesh"}, "points": {"points"}}
_COMMON = {"name", "type", "carve"}
OPTIONAL = {"box": {"spacing"}, "plate": {"spacing"}, "sphere": {"spacing"}, "mesh": {"spacing", "scale", "translate", "fill"}, "points": set()}


def config_groups(config):
    """`scene.geometry` = [{"name", "type": "box" | "plate" | "sphere" | "mesh" | "points", ..., "spacing": particle diameter, "carve": false}, ...]
    as a list of (name, points, carve) in the order of the block; carve is False, True (the default clearance) or a clearance.  Per type: box
    "min", "max"; plate "origin", "u", "v"; sphere "centre", "radius"; mesh "mesh" (a path as `solid.mesh`), "scale", "translate", "fill"; points
    "points" ((n, 3) as given, no spacing).  Pure Python; a key the entry's type does not take, an unknown type, a missing or repeated name raises ValueError.  No block: an empty list."""
    block = config["scene"].get("geometry")
    if block is None:
        return []
    if not isinstance(block, list):
        raise ValueError("scene.geometry must be a list of objects, got %r" % (block,))
    d = 2.0 * float(config["scene"]["particle_radius"])
    out, seen = [], set()
    for e in block:
        if not isinstance(e, dict) or e.get("type") not in TYPES:
            raise ValueError("scene.geometry: each entry needs a type of %s, got %r" % (sorted(TYPES), e))
        kind, name = e["type"], e.get("name")
        if not isinstance(name, str) or not name or name in seen:
            raise ValueError("scene.geometry: each entry needs a name of its own, got %r" % (name,))
        seen.add(name)
        need = TYPES[kind]
        if need - set(e) or set(e) - need - _COMMON - OPTIONAL[kind]:
            raise ValueError("scene.geometry[%s]: a %s takes %s (and %s), got %s" % (name, kind, sorted(need), sorted(OPTIONAL[kind] | {"carve"}), sorted(e)))
        sp = e.get("spacing", d)
        if kind == "box":
            pts = box_shell(e["min"], e["max"], sp)
        elif kind == "plate":
            pts = plate(e["origin"], e["u"], e["v"], sp)
        elif kind == "sphere":
            pts = sphere_shell(e["centre"], e["radius"], sp)
        elif kind == "mesh":
            pts = mesh_samples(e["mesh"], sp, scale=e.get("scale", 1), translate=e.get("translate", (0, 0, 0)), fill=e.get("fill", False))
        else:
            pts = np.ascontiguousarray(e["points"], dtype=np.float32)
            if pts.ndim != 2 or pts.shape[1] != 3 or not len(pts):
                raise ValueError("scene.geometry[%s]: points must be (n, 3) with n > 0" % name)
        carve = e.get("carve", False)
        if not isinstance(carve, (bool, int, float)) or (not isinstance(carve, bool) and not carve > 0):
            raise ValueError("scene.geometry[%s]: carve must be false, true or a clearance > 0, got %r" % (name, carve))
        out.append((name, pts, carve))
    return out


def config_loads(config):
    """`scene.loads` = ["box", "pillar_a", ...]: the wall groups whose load is measured, "box" or names of `scene.geometry`,
    as a list in the order given.  Pure Python; anything but a list of such names, or a name twice, raises ValueError.  No key: an empty list."""
    block = config["scene"].get("loads")
    if block is None:
        return []
    if not isinstance(block, list) or not all(isinstance(n, str) for n in block):
        raise ValueError("scene.loads must be a list of names, got %r" % (block,))
    geo = config["scene"].get("geometry")
    known = ["box"] + [e.get("name") for e in geo if isinstance(e, dict)] if isinstance(geo, list) else ["box"]
    for n in block:
        if n not in known:
            raise ValueError("scene.loads: no wall group '%s' (scene.geometry has %s, and there is \"box\")" % (n, ", ".join(known[1:]) or "none"))
        if block.count(n) > 1:
            raise ValueError("scene.loads: '%s' is named twice" % n)
    return list(block)


def apply_loads(sim, config):
    """The call `scene.loads` asks of a new handle (anything with measure_loads), after apply_config; no key or an empty list: no call.  A handle
    that cannot measure -- the library answers SPH_E_STATE: a slab handle, a relaxed handle, pbf, a library without the entry points -- runs the
    scene as it always did: the key is skipped with one printed line, and an explicit measure_loads is still refused.  Returns the names measured."""
    names = config_loads(config)
    if not names:
        return []
    try:
        sim.measure_loads(names)
    except RuntimeError as e:
        if getattr(e, "code", None) != -5:              # SPH_E_STATE (include/sph_mi355x.h)
            raise
        print("scene.loads skipped, this handle measures no loads: %s" % e)
        return []
    return names


def apply_config(sim, config):
    """Make the calls `scene.geometry` asks of a new handle (anything with add_geometry / carve): every group is added in order, then carved where
    its entry says so.  Returns {name: group}."""
    groups = {}
    for name, pts, carve in config_groups(config):
        groups[name] = sim.add_geometry(pts)
        if carve is not False:
            sim.carve(groups[name], None if carve is True else float(carve))
    return groups
