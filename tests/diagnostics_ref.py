"""The yardstick of the run diagnostics (TEST INFRASTRUCTURE of test_diagnostics_cpu.py and test_diagnostics_gpu.py).
Nothing here imports the HIP library: the GPU file hands in downloaded f32 arrays.

row() computes all 32 slots of an SphDiagnostics row from f32 arrays in API order (index = original id).  The sums are exact -- every term is a
sum of products of two f32 values, each product exact in f64, and math.fsum adds such numbers without error -- and rounded once; the extrema, the
largest speed and its id are numpy f32 with the expression the device uses.  bounds() gives, per summed slot, the derived error bound the device's
f64 summation is held to."""
import math
import re
from fractions import Fraction

import numpy as np

F = np.float32
SLOTS = ("time", "dt", "step", "n", "mass", "momentum_x", "momentum_y", "momentum_z",
         "angular_momentum_x", "angular_momentum_y", "angular_momentum_z", "kinetic", "potential", "com_x", "com_y", "com_z",
         "vmax", "vmax_id", "pos_min_x", "pos_min_y", "pos_min_z", "pos_max_x", "pos_max_y", "pos_max_z", "rho_min", "rho_max", "rho_mean",
         "reserved_0", "reserved_1", "reserved_2", "reserved_3", "reserved_4")
SUMMED = ("mass",) + SLOTS[5:16] + ("rho_mean",)                    # compared within bounds()
EXACT = ("n", "vmax", "vmax_id") + SLOTS[18:24] + ("rho_min", "rho_max")      # bit-equal (time, dt, step: against the handle's scalars)
RHO = ("rho_min", "rho_max", "rho_mean")


def header_slots(text):
    """the flat slot names of `struct SphDiagnostics` in include/sph_mi355x.h: members in order, name[3] -> _x, _y, _z, name[k] -> _0 .. _k-1"""
    body = re.search(r"typedef struct SphDiagnostics \{(.*?)\} SphDiagnostics;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for kind, name, dim in re.findall(r"(\w+)\s+(\w+)(?:\[(\d+)\])?\s*;", body):
        assert kind == "double", (kind, name)
        if not dim:
            names.append(name)
        elif int(dim) == 3:
            names += [name + "_" + a for a in "xyz"]
        else:
            names += ["%s_%d" % (name, k) for k in range(int(dim))]
    return tuple(names)


def exact_sum(columns):
    """the exact sum of f64 numbers as a Fraction: fsum rounds the exact sum once, a second fsum recovers what the first lost (to 2^-106 relative,
    far below anything compared here)"""
    terms = np.concatenate([np.asarray(c, dtype=np.float64).ravel() for c in columns])
    hi = math.fsum(terms)
    lo = math.fsum(np.append(terms, -hi))
    return Fraction(hi) + Fraction(lo)


def terms(pos, vel, accel):
    """per summed quantity, the list of f64 arrays whose entries add up to a particle's term: every entry is one f32 x f32 product (or one f32),
    exact in f64.  Keyed by slot name, without the scaling"""
    p, v = np.asarray(pos, dtype=F).astype(np.float64), np.asarray(vel, dtype=F).astype(np.float64)
    a = np.asarray(accel, dtype=F).astype(np.float64)
    x, y, z = p.T
    vx, vy, vz = v.T
    return {
        "momentum_x": [vx], "momentum_y": [vy], "momentum_z": [vz],
        "angular_momentum_x": [y * vz, -(z * vy)], "angular_momentum_y": [z * vx, -(x * vz)], "angular_momentum_z": [x * vy, -(y * vx)],
        "kinetic": [vx * vx, vy * vy, vz * vz],
        "potential": [a[0] * x, a[1] * y, a[2] * z],
        "com_x": [x], "com_y": [y], "com_z": [z],
    }


def scale(name, m, n):
    """the factor applied once, at the end, as an exact rational"""
    m = Fraction(float(m))
    if name.startswith("com") or name == "rho_mean":
        return Fraction(1, n)
    return {"kinetic": m / 2, "potential": -m}.get(name, m)


def speed(vel):
    """the f32 value sqrtf((vx vx + vy vy) + vz vz)"""
    v = np.asarray(vel, dtype=F)
    return np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2], dtype=F)


def fastest(vel):
    """(largest speed, lowest index among the particles that have it); arrays in API order: the index is the original id"""
    s = speed(vel)
    return s.max(), int(np.flatnonzero(s == s.max())[0])


def row(pos, vel, rho, m, accel, time=0.0, dt=0.0, step=0):
    """every slot, keyed by name.  rho None: the three rho slots are NaN.  m: SPH_S_PARTICLE_M (the f32 mass, widened); accel: SPH_S_ACCEL"""
    pos, vel = np.asarray(pos, dtype=F), np.asarray(vel, dtype=F)
    n = len(pos)
    out = dict.fromkeys(SLOTS, 0.0)
    out.update(time=float(time), dt=float(dt), step=float(step), n=float(n), mass=float(Fraction(n) * Fraction(float(m))))
    for name, cols in terms(pos, vel, accel).items():
        out[name] = float(exact_sum(cols) * scale(name, m, n))
    out["vmax"], out["vmax_id"] = (float(v) for v in fastest(vel))
    for k, a in enumerate("xyz"):
        out["pos_min_" + a], out["pos_max_" + a] = float(pos[:, k].min()), float(pos[:, k].max())
    if rho is None:
        out.update(rho_min=math.nan, rho_max=math.nan, rho_mean=math.nan)
    else:
        rho = np.asarray(rho, dtype=F)
        out.update(rho_min=float(rho.min()), rho_max=float(rho.max()), rho_mean=float(exact_sum([rho.astype(np.float64)]) * Fraction(1, n)))
    return out


def bounds(pos, vel, rho, m, accel):
    """The derived bound on |device - exact| per summed slot: (n + 8) 2^-53 sum_i |t_i|, scaled like the slot.

    Derivation.  A particle's term t_i is m times a sum or difference of at most three products of two f32 values.  Each product has at most 48
    significant bits and is exact in f64, so forming t_i takes at most two f64 additions and the multiplication by m: c <= 3 roundings, each of
    relative size u = 2^-53 (the device multiplies by m once, after the sum; counting it per term only makes the bound larger).  Adding n such
    terms in ANY order -- thread-strided, the wave butterfly, the waves, the workgroups' rows -- is n - 1 additions, and every term passes through at
    most n - 1 of them, so to first order |sum_computed - sum_exact| <= (n - 1 + c) u sum_i |t_i| (Higham, Accuracy and Stability of Numerical
    Algorithms, section 4.2, whatever the order).  The final scalings (m, 1/2, 1/n: at most three more roundings) bring c to <= 6; the second-order
    terms are below (n u)^2, i.e. 1e-22 of the bound at the sizes used.  (n + 8) covers n - 1 + c with room for the rounding of the bound's own
    evaluation.  mass = n m is one rounding: its bound is 2^-53 |n m|, and n = 1 .. 66 560 times a 24-bit m is in fact exact.
    sum_i |t_i| is taken with |t_i| the absolute value of the particle's exact term (fsum of its products), scaled by |scale|."""
    n = len(pos)
    u = 2.0 ** -53
    out = {"mass": u * n * float(m)}
    for name, cols in terms(pos, vel, accel).items():
        per_particle = np.abs(np.array([math.fsum(c) for c in zip(*cols)])) if len(cols) > 1 else np.abs(cols[0])
        out[name] = (n + 8) * u * math.fsum(per_particle) * abs(float(scale(name, m, n)))
    if rho is not None:
        out["rho_mean"] = (n + 8) * u * math.fsum(np.abs(np.asarray(rho, dtype=F).astype(np.float64))) / n
    return out


def device_terms(pos, vel, accel):
    """the f64 term of every particle as the device forms it (products, then the three-term sum, each rounded), unscaled: what the fairness tests
    of test_diagnostics_cpu.py add up in other orders"""
    t = {}
    for name, cols in terms(pos, vel, accel).items():
        acc = cols[0].copy()
        for c in cols[1:]:
            acc = acc + c
        t[name] = acc
    return t


def check_row(got, ref, bnd, when, rho=True):
    """a device row (dict by name) against row() / bounds(): the exact slots bit for bit, the summed slots within their bound, reserved slots 0"""
    for name in EXACT:
        if name in RHO and not rho:
            continue
        assert got[name] == ref[name], "%s: %s is %r, the reference has %r" % (when, name, got[name], ref[name])
    for name in SUMMED:
        if name in RHO and not rho:
            continue
        err = abs(got[name] - ref[name])
        print("%s: %-20s device %.17g reference %.17g |diff| %.3e bound %.3e" % (when, name, got[name], ref[name], err, bnd[name]))
        assert err <= bnd[name], "%s: %s is %r, the reference has %r: off by %.3e, the bound is %.3e" % (when, name, got[name], ref[name], err, bnd[name])
    if not rho:
        assert all(math.isnan(got[k]) for k in RHO), (when, [got[k] for k in RHO])
    assert all(got[k] == 0.0 for k in SLOTS[27:]), when
