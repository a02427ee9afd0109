"""Yardsticks of the derived per-particle fields (sph_derived).  TEST INFRASTRUCTURE ONLY: test_derived_cpu.py shows them fair
and sharp without the library, test_derived_gpu.py holds the library to them.  Nothing here imports the HIP library.

Both run from what a handle downloads (positions, velocities, its own densities, the wall and body samples, m and h): no density is recomputed.

The definition, once (include/sph_mi355x.h).  For fluid particle i, over the entries of its fluid list in list order, d = x_i - x_j, r = |d|,
an entry with r > h contributes nothing; vol = rho_j > 0 ? m / rho_j : 0; g = grad W(d), w = W(r) (solver_base.py:74-103, the gradient with the
factor 6 the reference carries):
    fluid entry j:    G_ab += (vol (v_j,a - v_i,a)) g_b;   F_b += vol g_b;   F_c += vol w
    body sample r:    F_b += V_r g_b;   F_c += V_r w                        (a coupled body only)
    wall entry b:     B_b += V_b g_b;   B_c += V_b w                        (separate accumulators)
    velgrad = G;  vorticity = (G_zy - G_yz, G_xz - G_zx, G_yx - G_xy);  divergence = (G_xx + G_yy) + G_zz;
    normal_a = -(h (F_a + B_a));  cover = F_c + B_c
The 17 output slots in the order of SLOTS.

YARDSTICK A (yardstick_a): the text above in numpy f32, pair by pair in the order of the lists it is given -- canonically those of
second_restatement.Neighbours (brute-force pairs, cell offset with dx outermost, then index; a cell's body samples behind its fluid) -- with
cubic_kernel and cubic_kernel_derivative of second_restatement.py.  The library is held to it bit for bit.

YARDSTICK B (yardstick_b): the same sums in f64 over all pairs with f32 distance <= h, any order, with a bound for ANY f32 evaluation of the
definition in ANY order of a list that holds at least those pairs.  The bound is derived, not measured; u = 2^-24, first order in u, the neglected
second order covered by the factor (1 + 2^-10):

  inputs are f32 and exact.  d_a: one rounding, u.  r = sqrt((dx^2 + dy^2) + dz^2): 2u (d) + u (squares) + 2u (sums) on r^2, halved by the root,
  plus its own: 3.5u.  q = r / h: 4.5u, so |dq| <= 4.5u q.  h r: 4.5u.
  grad W, inner piece (q <= 1/2): s = kg6 (3 q^2 - 2 q).  3 q^2 carries 11u, 2 q 4.5u, the difference u more; relative to |s| = kg6 q (2 - 3q):
      (33 q + 9) / (2 - 3 q) u + u <= 52u at q = 1/2, 53u with the product by kg6.
  grad W, outer piece: t = 1 - q has the ABSOLUTE error |dq| + u t, which no multiple of |t^2| bounds as q -> 1:
      |d(kg6 t^2)| <= 4u kg6 t^2 + 9u kg6 |t|.        The second term is kept as an absolute term per pair.
  g_b = (s d_b) / (h r): u (d_b), u (product), 4.5u (h r), u (quotient): 7.5u on top of s -- inner 60.5u, outer 11.5u + the absolute term.
  W, inner piece: k (6 (q^3 - q^2) + 1).  |d(q^2)| <= 10u q^2, |d(q^3)| <= 15.5u q^3; bracket b >= 1/4 with |db| <= 29.2u at q = 1/2: 117u, 118u with k.
  W, outer piece: 2k t^3: 6u relative + the absolute term 13.5u (2 k t^2) q <= 13.5u (2 k t^2).
  coefficients: vol = m / rho_j: u.  vol (v_j - v_i)_a: 3u.  A product coefficient x kernel value: u.
  So every term t of an accumulator that takes gradients is within (3 + 1 + 60.5 = 64.5 <= 66) u |t| + |coef| 9u kg6 |t_q| |d_b| / (h r) of its
  exact value, every term of F_c / B_c within (1 + 1 + 118 = 120 <= 122) u |t| + |coef| 13.5u 2k t_q^2 (the absolute parts for outer pairs only).
  A sequential f32 sum of n terms adds at most (n - 1) u sum |t|.  Per accumulator:
      bound = u ((count + c) sum |t| + sum absolute terms) (1 + 2^-10),     c = 66 (gradients), 122 (kernel values)
  The branch of a pair within |dq| of q = 1/2 may differ from the exact one: both pieces agree there in value and first derivative, a second-order
  effect.  A pair within |dq| of q = 1 may pass the gate on one side only: its term is O(u^2) (gradients) or O(u^3).
  Epilogue: a difference or sum of accumulators adds their bounds and u per addition of the magnitudes added; normal: h (bound F + bound B) +
  2u h |F + B|; cover: bound F_c + bound B_c + u |cover|.
"""
import math

import numpy as np

from second_restatement import F, Neighbours, _ipow, _norm, cubic_kernel, cubic_kernel_derivative

U = 2.0 ** -24
C_GRAD, C_W = 66.0, 122.0
SECOND_ORDER = 1.0 + 2.0 ** -10
SLOTS = ("G_xx", "G_xy", "G_xz", "G_yx", "G_yy", "G_yz", "G_zx", "G_zy", "G_zz", "vort_x", "vort_y", "vort_z", "div", "normal_x", "normal_y", "normal_z",
         "cover")
QUANTITIES = (("velgrad", 0, 9), ("vorticity", 9, 3), ("divergence", 12, 1), ("normal", 13, 3), ("cover", 16, 1))      # name, first slot, width
A_MATRIX = np.array([[0.3, -1.1, 0.7], [0.9, -0.4, -1.6], [-0.5, 1.3, 0.2]])      # a full matrix, neither symmetric nor antisymmetric
B_VECTOR = np.array([0.2, -0.3, 0.1])


class State:
    """what the sums read: f32 arrays and scalars.  wall_* / body_*: None or empty where the handle has none (a body: only while it is coupled)"""

    def __init__(self, pos, vel, rho, m, h, wall_pos=None, wall_vol=None, body_pos=None, body_vol=None):
        self.pos, self.vel, self.rho = (np.ascontiguousarray(a, dtype=F) for a in (pos, vel, rho))
        self.m, self.h = F(m), F(h)
        empty3, empty = np.zeros((0, 3), dtype=F), np.zeros(0, dtype=F)
        self.wall_pos = empty3 if wall_pos is None else np.ascontiguousarray(wall_pos, dtype=F)
        self.wall_vol = empty if wall_vol is None else np.ascontiguousarray(wall_vol, dtype=F)
        self.body_pos = empty3 if body_pos is None else np.ascontiguousarray(body_pos, dtype=F)
        self.body_vol = empty if body_vol is None else np.ascontiguousarray(body_vol, dtype=F)
        self.n = len(self.pos)


class Cells:
    """the grid of ParticleSystem.py:100-101, 490-494, as second_restatement.Scene states it, without the scene"""

    def __init__(self, config, h):
        scene = config["scene"]
        support = 4 * scene["particle_radius"]
        self.grid = [int(math.ceil((scene["box_max"][a] - scene["box_min"][a]) / support)) + 1 for a in range(3)]
        self.C = self.grid[0] * self.grid[1] * self.grid[2]
        self.h = F(h)

    def cell(self, pos):
        return np.floor(pos / self.h).astype(np.int32)


class Lists:
    """index (n, kmax) and count (n,) of the fluid list (entries >= n: body sample entry - n) and of the wall list"""

    def __init__(self, fi, fc, wi, wc):
        self.fi, self.fc, self.wi, self.wc = fi, np.asarray(fc), wi, np.asarray(wc)


def canonical_lists(cells, st):
    """the reference's walk order (second_restatement.Neighbours)"""
    nf = Neighbours(cells, st.pos, np.concatenate([st.pos, st.body_pos]), same=True)
    if len(st.wall_pos):
        nw = Neighbours(cells, st.pos, st.wall_pos, same=False)
        return Lists(nf.index, nf.count, nw.index, nw.count)
    return Lists(nf.index, nf.count, np.zeros((st.n, 1), dtype=np.int64), np.zeros(st.n, dtype=np.int64))


def _within(centres, others, cutoff, same, rows=None):
    """pairs with f32 distance <= cutoff; same: centre k is others[rows[k]] (rows None: others[k]) and not its own neighbour"""
    d = centres[:, None, :] - others[None, :, :]
    dist = np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])
    ok = ~(dist > F(cutoff))
    if same:
        ok[np.arange(len(centres)), np.arange(len(centres)) if rows is None else rows] = False
    return ok


def _pack(ok):
    count = ok.sum(axis=1)
    order = np.argsort(~ok, axis=1, kind="stable")
    return order[:, :max(int(count.max()) if len(count) else 0, 1)], count


def skin_lists(st, cutoff):
    """every pair within `cutoff` (a Verlet list's h + skin), in index order"""
    fi, fc = _pack(_within(st.pos, np.concatenate([st.pos, st.body_pos]), cutoff, True))
    if len(st.wall_pos):
        wi, wc = _pack(_within(st.pos, st.wall_pos, cutoff, False))
    else:
        wi, wc = np.zeros((st.n, 1), dtype=np.int64), np.zeros(st.n, dtype=np.int64)
    return Lists(fi, fc, wi, wc)


def shuffled(lists, seed):
    """every particle's entries in a seeded random order"""
    rng = np.random.default_rng(seed)

    def one(index, count):
        out = index.copy()
        for i in range(len(count)):
            out[i, :count[i]] = index[i, rng.permutation(int(count[i]))]
        return out
    return Lists(one(lists.fi, lists.fc), lists.fc, one(lists.wi, lists.wc), lists.wc)


MUTANTS = ("drop_last", "no_walls", "rho_i", "transposed", "inner_constant", "no_gate")


def _kernels(d, r, h, mutant):
    """(W, grad W) of yardstick A; the mutants that sit in the kernel functions"""
    w, g = cubic_kernel(r, h), cubic_kernel_derivative(d, h)
    if mutant == "inner_constant":            # the constant 6 of the q <= 1/2 pieces off by 1 %
        q = r / h
        inner = q <= F(0.5)
        k = F(8) / (F(math.pi) * _ipow(h, 3))
        w = np.where(inner, k * (F(6.06) * (q * q * q - q * q) + F(1)), w).astype(F)
        g = np.where(inner[:, None], g * F(1.01), g).astype(F)
    if mutant == "no_gate":                   # the outer piece of the gradient as the device's list form has it: no test of q <= 1 (W has one)
        q = r / h
        k = F(48) / (F(math.pi) * _ipow(h, 3))
        with np.errstate(divide="ignore", invalid="ignore"):
            outer = ((-k * F(6)) * _ipow(F(1) - q, 2))[:, None] * d / (h * r)[:, None]
        g = np.where((q > F(1))[:, None], outer, g).astype(F)
    return w, g


def yardstick_a(st, lists, mutant=None):
    """(n, 17) f32"""
    assert mutant is None or mutant in MUTANTS
    n, h, m = st.n, st.h, st.m
    others = np.concatenate([st.pos, st.body_pos])
    G, Fb, Fc = np.zeros((n, 3, 3), dtype=F), np.zeros((n, 3), dtype=F), np.zeros(n, dtype=F)
    Bb, Bc = np.zeros((n, 3), dtype=F), np.zeros(n, dtype=F)
    fc = lists.fc - 1 if mutant == "drop_last" else lists.fc
    for k in range(lists.fi.shape[1]):
        live = k < fc
        j = lists.fi[:, k]
        solid = j >= n
        jf = np.where(solid, 0, j)
        d = st.pos - others[j]
        r = _norm(d)
        gate = live if mutant == "no_gate" else live & ~(r > h)
        w, g = _kernels(d, r, h, mutant)
        rho_j = st.rho if mutant == "rho_i" else st.rho[jf]
        with np.errstate(divide="ignore"):
            vol = np.where(rho_j > F(0), m / rho_j, F(0)).astype(F)
        coef = np.where(solid, st.body_vol[np.where(solid, j - n, 0)], vol).astype(F) if len(st.body_vol) else vol
        s = vol[:, None] * (st.vel[jf] - st.vel)
        t = s[:, None, :] * g[:, :, None] if mutant == "transposed" else s[:, :, None] * g[:, None, :]
        G = np.where((gate & ~solid)[:, None, None], G + t, G)
        Fb = np.where(gate[:, None], Fb + coef[:, None] * g, Fb)
        Fc = np.where(gate, Fc + coef * w, Fc)
    if mutant != "no_walls":
        for k in range(lists.wi.shape[1] if len(st.wall_pos) else 0):
            live = k < lists.wc
            b = lists.wi[:, k]
            d = st.pos - st.wall_pos[b]
            r = _norm(d)
            gate = live if mutant == "no_gate" else live & ~(r > h)
            w, g = _kernels(d, r, h, mutant)
            vb = st.wall_vol[b]
            Bb = np.where(gate[:, None], Bb + vb[:, None] * g, Bb)
            Bc = np.where(gate, Bc + vb * w, Bc)
    out = np.zeros((n, 17), dtype=F)
    out[:, 0:9] = G.reshape(n, 9)
    out[:, 9] = G[:, 2, 1] - G[:, 1, 2]
    out[:, 10] = G[:, 0, 2] - G[:, 2, 0]
    out[:, 11] = G[:, 1, 0] - G[:, 0, 1]
    out[:, 12] = (G[:, 0, 0] + G[:, 1, 1]) + G[:, 2, 2]
    out[:, 13:16] = -(h * (Fb + Bb))
    out[:, 16] = Fc + Bc
    assert out.dtype == F and G.dtype == F and Fb.dtype == F and Bc.dtype == F
    return out


def _pair_sums(centres, others, coef, h, same, dv=None, rows=None):
    """f64 sums over the pairs with f32 distance <= h: (sum coef g_b, its sum |t|, its absolute terms, the same three for coef w, count) and, with
    dv[i, j, a] = (v_j - v_i)_a, the three for G"""
    ok = _within(centres, others, h, same, rows)
    h64 = float(h)
    d = centres.astype(np.float64)[:, None, :] - others.astype(np.float64)[None, :, :]
    r = np.sqrt((d * d).sum(axis=2))
    q = r / h64
    kw = float(F(8) / (F(math.pi) * _ipow(F(h), 3)))
    kg6 = float((F(48) / (F(math.pi) * _ipow(F(h), 3))) * F(6))
    t = 1.0 - q
    inner = q <= 0.5
    w = np.where(inner, kw * (6.0 * (q ** 3 - q ** 2) + 1.0), 2.0 * kw * t ** 3)
    s = np.where(inner, kg6 * (3.0 * q * q - 2.0 * q), -kg6 * t * t)
    with np.errstate(divide="ignore", invalid="ignore"):
        unit = np.where((q > 1e-5)[..., None], d / (h64 * r)[..., None], 0.0)
    g = s[..., None] * unit
    g_abs = np.where(inner, 0.0, 9.0 * kg6 * np.abs(t))[..., None] * np.abs(unit)
    w_abs = np.where(inner, 0.0, 13.5 * 2.0 * kw * t * t)
    c = np.where(ok, coef[None, :], 0.0)
    res = {"count": ok.sum(axis=1),
           "g": (c[..., None] * g).sum(axis=1), "g_sum": (np.abs(c)[..., None] * np.abs(g)).sum(axis=1), "g_abs": (np.abs(c)[..., None] * g_abs).sum(axis=1),
           "w": (c * w).sum(axis=1), "w_sum": (np.abs(c) * np.abs(w)).sum(axis=1), "w_abs": (np.abs(c) * w_abs).sum(axis=1)}
    if dv is not None:
        sa = c[..., None] * dv                                                  # (n, n, a)
        res["G"] = np.einsum("ija,ijb->iab", sa, g)
        res["G_sum"] = np.einsum("ija,ijb->iab", np.abs(sa), np.abs(g))
        res["G_abs"] = np.einsum("ija,ijb->iab", np.abs(sa), g_abs)
    return res


def yardstick_b(st, rows=None):
    """(values (n, 17) f64, bounds (n, 17) f64); rows: of these particles only (a large state: the pair matrices are len(rows) x n)"""
    rows = np.arange(st.n) if rows is None else np.asarray(rows)
    n, h, centres = len(rows), float(st.h), st.pos[rows]
    rho = st.rho.astype(np.float64)
    with np.errstate(divide="ignore"):
        vol = np.where(rho > 0, float(st.m) / rho, 0.0)
    v = st.vel.astype(np.float64)
    fl = _pair_sums(centres, st.pos, vol, st.h, True, dv=v[None, :, :] - v[rows][:, None, :], rows=rows)

    def bound(cnt, c, total, absolute):
        return U * ((cnt.reshape((-1,) + (1,) * (total.ndim - 1)) + c) * total + absolute) * SECOND_ORDER

    G, bG = fl["G"], bound(fl["count"], C_GRAD, fl["G_sum"], fl["G_abs"])
    Fb, Fb_sum, Fb_abs, Fc, Fc_sum, Fc_abs, cnt = fl["g"], fl["g_sum"], fl["g_abs"], fl["w"], fl["w_sum"], fl["w_abs"], fl["count"]
    if len(st.body_pos):
        bd = _pair_sums(centres, st.body_pos, st.body_vol.astype(np.float64), st.h, False)
        Fb, Fb_sum, Fb_abs = Fb + bd["g"], Fb_sum + bd["g_sum"], Fb_abs + bd["g_abs"]
        Fc, Fc_sum, Fc_abs, cnt = Fc + bd["w"], Fc_sum + bd["w_sum"], Fc_abs + bd["w_abs"], cnt + bd["count"]
    bFb, bFc = bound(cnt, C_GRAD, Fb_sum, Fb_abs), bound(cnt, C_W, Fc_sum, Fc_abs)
    Bb, Bc, bBb, bBc = np.zeros((n, 3)), np.zeros(n), np.zeros((n, 3)), np.zeros(n)
    if len(st.wall_pos):
        wl = _pair_sums(centres, st.wall_pos, st.wall_vol.astype(np.float64), st.h, False)
        Bb, Bc = wl["g"], wl["w"]
        bBb, bBc = bound(wl["count"], C_GRAD, wl["g_sum"], wl["g_abs"]), bound(wl["count"], C_W, wl["w_sum"], wl["w_abs"])
    val, bnd = np.zeros((n, 17)), np.zeros((n, 17))
    val[:, 0:9], bnd[:, 0:9] = G.reshape(n, 9), bG.reshape(n, 9)
    for k, (p, m_) in enumerate((((2, 1), (1, 2)), ((0, 2), (2, 0)), ((1, 0), (0, 1)))):
        val[:, 9 + k] = G[:, p[0], p[1]] - G[:, m_[0], m_[1]]
        bnd[:, 9 + k] = bG[:, p[0], p[1]] + bG[:, m_[0], m_[1]] + U * np.abs(val[:, 9 + k]) * SECOND_ORDER
    val[:, 12] = G[:, 0, 0] + G[:, 1, 1] + G[:, 2, 2]
    bnd[:, 12] = bG[:, 0, 0] + bG[:, 1, 1] + bG[:, 2, 2] + 2 * U * (np.abs(G[:, 0, 0]) + np.abs(G[:, 1, 1]) + np.abs(G[:, 2, 2])) * SECOND_ORDER
    val[:, 13:16] = -(h * (Fb + Bb))
    bnd[:, 13:16] = h * (bFb + bBb) + 2 * U * h * (np.abs(Fb) + np.abs(Bb)) * SECOND_ORDER
    val[:, 16] = Fc + Bc
    bnd[:, 16] = bFc + bBc + U * (np.abs(Fc) + np.abs(Bc)) * SECOND_ORDER
    return val, bnd


def worst_ratio(got, val, bnd):
    """max over particles and slots of |got - val| / bound; where the bound is 0 the value must be exactly the yardstick's (ratio 0 or inf)"""
    err = np.abs(np.asarray(got, dtype=np.float64) - val)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bnd > 0, err / bnd, np.where(err == 0, 0.0, np.inf))
    return float(ratio.max()) if ratio.size else 0.0


def split(out17):
    """{quantity name: array in the shape Simulation.derived returns} of an (n, 17) array"""
    n = len(out17)
    shapes = {"velgrad": (n, 3, 3), "vorticity": (n, 3), "divergence": (n,), "normal": (n, 3), "cover": (n,)}
    return {name: out17[:, first:first + width].reshape(shapes[name]) for name, first, width in QUANTITIES}


def displaced(pos, spacing, seed):
    """every particle moved by up to 0.15 spacings per axis"""
    rng = np.random.default_rng(seed)
    return (pos + (F(0.15) * F(spacing)) * rng.uniform(-1.0, 1.0, size=pos.shape).astype(F)).astype(F)


def velocities(pos, seed, noise=0.05):
    """A x + b plus uniform noise of +-0.05 m/s"""
    rng = np.random.default_rng(seed + 1000)
    v = pos.astype(np.float64) @ A_MATRIX.T + B_VECTOR
    return (v + noise * rng.uniform(-1.0, 1.0, size=pos.shape)).astype(F)
