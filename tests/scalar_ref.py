"""Yardsticks of the carried scalar (sph_scalar_*).  TEST INFRASTRUCTURE ONLY: test_scalar_cpu.py shows them fair and sharp
without the library, test_scalar_gpu.py holds the library to them.  Nothing here imports the HIP library.

Both run from what a handle downloads (positions, T, the body's samples, m and h) and the parameters the test gave it.

The definition, once (include/sph_mi355x.h).  Constants, formed in f64 from the f32 values and rounded once:
    eta2 = (float)(0.01 h h),   kw = 8 / (pi h^3) in f32 (solver_base.py:79),   kq = (float)(12 D (m / rho0) kw / h)
The rate of particle i, over the FLUID entries j of its fluid list in list order, f32, every operation rounded on its own:
    d = x_i - x_j;  r2 = (dx dx + dy dy) + dz dz;  r = sqrt(r2);  r > h: nothing;  q = r / h;
    g = q <= 0.5 ? (3 (q q) - 2 q) : -((1 - q) (1 - q));  f = (g r) / (r2 + eta2);  acc += (T_i - T_j) f
    rate_i = kq acc
A body sample's entry adds nothing, the wall lists are not walked, no self term.  The step's end, with the dt the step used and its acceleration
vector a:  beta != 0: s = -(beta (T_i - T_ref)), vel_i += (dt s) a per component (from T^n);  T_i <- T_i + dt rate_i.

YARDSTICK A (yardstick_a, advance_a): the text above in numpy f32, pair by pair in the order of the lists it is given -- canonically those of
derived_ref.canonical_lists (second_restatement.Neighbours: cell offset with dx outermost, then index; a cell's body samples behind its fluid).
The library is held to it bit for bit.

YARDSTICK B (yardstick_b): the same sums in f64 over all pairs with f32 distance <= h, any order, with a bound for ANY f32 evaluation of the
definition in ANY order of a list that holds at least those pairs.  Derived, not measured; u = 2^-24, first order in u, the neglected second order
covered by the factor (1 + 2^-10).  Inputs (positions, T, the three constants) are f32 and exact; relative errors unless said otherwise:
    d_a: one rounding, u.   d_a d_a: 2u + u = 3u; the two additions of non-negative numbers: u each: r2 carries 5u.
    r = sqrt(r2): 2.5u + u = 3.5u.   q = r / h: 4.5u, so |dq| <= 4.5u q.
    g, inner piece (q <= 1/2): q q carries 10u, 3 (q q) 11u, 2 q 4.5u (the doubling is exact); the difference one more.  Relative to
        |g| = q (2 - 3 q):  (33 q + 9) / (2 - 3 q) u + u <= 52u  (largest at q = 1/2).
    g, outer piece: t = 1 - q has the ABSOLUTE error |dq| + u t <= 4.5u + u t, which no multiple of t^2 bounds as q -> 1:
        |d(t t)| <= 2 t (4.5u + u t) + u t^2 = 3u t^2 + 9u t;  the negation is exact.  The second term is kept as an absolute term per pair.
    g r: 3.5u (r) + u (product) on top: inner 56.5u, outer 7.5u + the absolute term.
    r2 + eta2: 5u on r2 (eta2 exact, both positive) + u = 6u.   The quotient: u.   f: inner 63.5u, outer 14.5u + the absolute term.
    T_i - T_j: u.   The product with f: u.   So every term t is within
        65.5u |t| (inner),   16.5u |t| + 9u |T_i - T_j| |1 - q| r / (r2 + eta2) (outer)
    of its exact value.  A sequential f32 sum of n terms adds at most (n - 1) u sum |t|; the product with kq one more u |acc| <= u sum |t|.
        bound = u ((count + c) sum |t| + sum of the absolute terms) kq (1 + 2^-10),     c = 66    (65.5 + 1 - 1, rounded up)
    The branch of a pair within |dq| of q = 1/2 may differ from the exact one: both pieces agree there in value (-1/4) and first derivative (1), a
    second-order effect.  A pair within |dq| of q = 1 may pass the gate on one side only: its term is O(u^2).
"""
import math

import numpy as np

import derived_ref as dr
from second_restatement import F, Neighbours, _ipow

U = 2.0 ** -24
C_TERM = 66.0
SECOND_ORDER = 1.0 + 2.0 ** -10
RHO0 = F(1000.0)             # Consts.rho0 (density_0 of every scene)


class State:
    """what the sums read: f32 arrays and scalars, and the parameters of the handle.  body_pos / body_w: the samples of a COUPLED body and what the
    device holds in their .w (the sample volume) -- only the "rigid entry counted" mutant reads body_w; rho: only the "m / rho_j" mutant reads it.
    Looks like a derived_ref.State to canonical_lists / skin_lists (pos, body_pos, wall_pos, n)."""

    def __init__(self, pos, T, m, h, D, body_pos=None, body_w=None, rho=None):
        self.pos, self.T = np.ascontiguousarray(pos, dtype=F), np.ascontiguousarray(T, dtype=F)
        self.m, self.h, self.D = F(m), F(h), float(D)
        self.body_pos = np.zeros((0, 3), dtype=F) if body_pos is None else np.ascontiguousarray(body_pos, dtype=F)
        self.body_w = np.zeros(len(self.body_pos), dtype=F) if body_w is None else np.ascontiguousarray(body_w, dtype=F)
        self.wall_pos = np.zeros((0, 3), dtype=F)          # the walls are insulated: no wall list is walked
        self.rho = None if rho is None else np.ascontiguousarray(rho, dtype=F)
        self.n = len(self.pos)


def constants(st, factor=12.0):
    """(eta2, kq) as the host forms them: f64 from the f32 values, rounded once"""
    h, m = float(st.h), float(st.m)
    kw = F(8) / (F(math.pi) * _ipow(st.h, 3))
    return F(0.01 * h * h), F(factor * st.D * (m / float(RHO0)) * float(kw) / h)


MUTANTS = ("sign", "no_eta2", "factor_6", "t_i_for_t_j", "m_over_rho_j", "reference_gradient", "rigid_counted", "no_gate")


def pair_terms(xi, xj, Ti, Tj, h, eta2, mutant=None):
    """(term, r) of yardstick A for arrays of pairs: (T_i - T_j) f in f32, every operation rounded on its own.  No gate here."""
    d = xi - xj
    r2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    r = np.sqrt(r2)
    q = r / h
    t = F(1) - q
    g = np.where(q <= F(0.5), F(3) * (q * q) - F(2) * q, -(t * t)).astype(F)
    if mutant == "reference_gradient":            # cubic_kernel_derivative's scalar carries a further factor 6
        g = F(6) * g
    with np.errstate(divide="ignore", invalid="ignore"):
        f = (g * r) / (r2 if mutant == "no_eta2" else r2 + eta2)
    dT = {"sign": Tj - Ti, "t_i_for_t_j": Ti - Ti}.get(mutant, Ti - Tj)
    term = dT * f
    assert term.dtype == F and r.dtype == F
    return term, r


def canonical_lists_rows(cells, st, rows):
    """derived_ref.canonical_lists for the particles `rows` only (a large state: the pair matrices are len(rows) x n): the same entries in the same
    order.  The walker meets itself where Neighbours is told that centres and others differ; that one entry is taken out of its row."""
    rows = np.asarray(rows)
    nf = Neighbours(cells, st.pos[rows], np.concatenate([st.pos, st.body_pos]), same=False)
    index = nf.index.copy()
    for k, i in enumerate(rows):
        at = int(np.flatnonzero(index[k, :nf.count[k]] == i)[0])
        index[k, at:-1] = index[k, at + 1:]
    return dr.Lists(index, nf.count - 1, np.zeros((len(rows), 1), dtype=np.int64), np.zeros(len(rows), dtype=np.int64))


def yardstick_a(st, lists, mutant=None, rows=None):
    """rate f32 in the order of `lists`: (n,), or of the particles `rows` alone (lists: canonical_lists_rows)"""
    assert mutant is None or mutant in MUTANTS
    n, h = st.n, st.h
    pos_i, T_i = (st.pos, st.T) if rows is None else (st.pos[rows], st.T[rows])
    eta2, kq = constants(st, 6.0 if mutant == "factor_6" else 12.0)
    if mutant == "m_over_rho_j":                 # the per-pair volume m / rho_j instead of the constant V0 = m / rho0
        kq = F(float(kq) / (float(st.m) / float(RHO0)))
    others = np.concatenate([st.pos, st.body_pos])
    T_all = np.concatenate([st.T, st.body_w])
    acc = np.zeros(len(pos_i), dtype=F)
    for k in range(lists.fi.shape[1]):
        live = k < lists.fc
        j = lists.fi[:, k]
        solid = j >= n
        term, r = pair_terms(pos_i, others[j], T_i, T_all[j], h, eta2, mutant)
        if mutant == "m_over_rho_j":
            term = term * (st.m / st.rho[np.where(solid, 0, j)])
        gate = live if mutant == "no_gate" else live & ~(r > h)
        if mutant != "rigid_counted":
            gate = gate & ~solid
        acc = np.where(gate, acc + term, acc)
    rate = kq * acc
    assert rate.dtype == F
    return rate


def advance_a(T, vel, rate, dt, beta, ref, accel):
    """(T, vel) after the step's end, numpy f32: the kick from T^n (only when beta != 0), then T + dt rate"""
    T, vel, rate, dt, beta, ref = (np.asarray(T, dtype=F), np.asarray(vel, dtype=F), np.asarray(rate, dtype=F), F(dt), F(beta), F(ref))
    out_v = vel
    if beta != 0:
        b = dt * -(beta * (T - ref))
        out_v = (vel + b[:, None] * np.asarray(accel, dtype=F)[None, :]).astype(F)
        assert b.dtype == F
    out_T = T + dt * rate
    assert out_T.dtype == F and out_v.dtype == F
    return out_T, out_v


def yardstick_b(st, rows=None):
    """(rate (n,) f64, bound (n,) f64, sum_c (n,) f64): the f64 sums over all fluid pairs with f32 distance <= h, the bound of the docstring, and
    sum_j c_ij with c_ij = -kq f_ij >= 0, the quantity the explicit scheme's limit dt sum_j c_ij <= 1 is about.  rows: of these particles only"""
    rows = np.arange(st.n) if rows is None else np.asarray(rows)
    eta2, kq = (float(v) for v in constants(st))
    h = float(st.h)
    centres = st.pos[rows]
    ok = dr._within(centres, st.pos, st.h, True, rows)
    d = centres.astype(np.float64)[:, None, :] - st.pos.astype(np.float64)[None, :, :]
    r2 = (d * d).sum(axis=2)
    r = np.sqrt(r2)
    q = r / h
    t = 1.0 - q
    inner = q <= 0.5
    g = np.where(inner, 3.0 * q * q - 2.0 * q, -(t * t))
    f = np.where(ok, g * r / (r2 + eta2), 0.0)
    dT = st.T.astype(np.float64)[rows][:, None] - st.T.astype(np.float64)[None, :]
    term = dT * f
    absolute = np.where(ok & ~inner, 9.0 * np.abs(dT) * np.abs(t) * r / (r2 + eta2), 0.0)
    count = ok.sum(axis=1)
    bound = U * ((count + C_TERM) * np.abs(term).sum(axis=1) + absolute.sum(axis=1)) * kq * SECOND_ORDER
    return kq * term.sum(axis=1), bound, -kq * f.sum(axis=1)


def worst_ratio(got, val, bnd):
    return dr.worst_ratio(got, val, bnd)


def lattice(nx=5, spacing=0.05):
    """an undisturbed cubic lattice of nx^3 particles centred on the origin, spacing 2 r, h = 4 r, m = rho0 (2 r)^3 as sph_create forms it; the index
    of its centre particle"""
    g = (np.arange(nx) - nx // 2).astype(F) * F(spacing)
    pos = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3).astype(F)
    c = nx // 2
    return pos, F(2 * spacing), F(1000.0 * spacing ** 3), (c * nx + c) * nx + c


def dt_limit(st, rows=None):
    """the explicit scheme's limit of a state: 1 / max_i sum_j c_ij (f64)"""
    return 1.0 / float(yardstick_b(st, rows)[2].max())


def two_valued(pos, axis=0):
    """T = 1 in the half of the particles with the larger coordinate on `axis`, 0 in the other"""
    x = np.asarray(pos)[:, axis]
    return (x > np.median(x)).astype(F)


def smooth(pos, seed):
    """a smooth field plus noise: T of order 1 with differences of every size between neighbours"""
    rng = np.random.default_rng(seed + 2000)
    p = np.asarray(pos, dtype=np.float64)
    return (1.0 + np.sin(7.0 * p[:, 0]) * np.cos(5.0 * p[:, 1]) + 0.5 * p[:, 2] + 0.05 * rng.uniform(-1.0, 1.0, size=len(p))).astype(F)
