"""A SECOND, independent restatement of the reference's PBF step -- numpy f32, brute-force O(N^2) neighbour search, on the Scene, Neighbours
and per-particle sums of tests/second_restatement.py.

TEST INFRASTRUCTURE ONLY (tests/test_second_restatement.py holds the oracle against it, tests/test_second_restatement_gpu.py the library's
quad, plain and Morton-order PBF kernels).  Written from the reference's text alone -- pbf_solver.py:26-187, solver_base.py:41-51, 113-143,
ParticleSystem.py:337-366, 388-397, 447-469 (Jukgei/CFD_Taichi @ 2024_08_07), cited at every function -- without looking at
oracle/sph_oracle.c or csrc/sph_pbf_kernels.h, and sharing no code with them.

pbf_solver.py cannot be transcribed word for word: it is stale at that commit and one of its kernels races.  What this file takes it to say:

 1. THE STALE CALLBACKS.  for_all_neighbor hands a task two particle STRUCTS (`task(particle, particle_j)`, ParticleSystem.py:469; `particle`
    is the copy get_particle(i) made when the walk began, :450), while pbf_solver's fluid callbacks still index fields with their arguments
    (`self.ps.fluid_particles.pos[i]`, :100, :120, :135, :146, :168).  Read: an argument stands for its struct, `fluid_particles.pos[x]` is
    x.pos, `fluid_particles.vel[x]` is x.vel, and `self.pbf_lambda[j]` (:153) is indexed by particle_j.index.  The boundary callbacks get what
    they were written for (`task(i, particle_j)`, two indices, ParticleSystem.py:366) and are taken as written.
 2. THE SCHEDULE OF update_all_pos (:66-95).  One parallel loop moves particle i and then reads its neighbours' pos and vel, which other
    iterations of the same loop write.  The schedule taken here is three phases with a barrier between them:
      phase 1, every particle: pos_predict += delta_pos; vel = (pos_predict - pos) / dt; under the clamp handle each coordinate is clamped to
               box_min + radius / box_max - radius, the lower plane tested first, and vel[j] *= v_decay_proportion = 0.5 (solver_base.py:18 --
               positive: the velocity is halved, not reflected as in the other solvers' -0.5); pos = pos_predict                      (:70-85)
      phase 2, every particle: v = sum_j (vel_j - vel_i) * poly_kernel(|pos_i - pos_j|), all four operands those of phase 1's end    (:88-89, :100)
      phase 3, every particle: vel += c * v                                                                                           (:94, :96)
    The wall part of the viscosity sum (:91-92, :104) is computed and discarded by the reference (:93 is a comment), so it is not computed.
 3. THE NEIGHBOUR SET OF PHASE 2.  Nothing rebuilds the grid inside a step: the lists (ParticleSystem.py:396) and belong_grid (:397), which
    for_all_neighbor takes as its centre cell (:451), are those of update_grid at the step's start, i.e. of the OLD positions.  The
    distance test `> support_radius` (:466) and the kernel's argument (:100) read the struct copies, i.e. the NEW positions.  Hence
    Neighbours(cells from the old positions, distances from the new ones); the walk order is that of the old cells.
 4. THE ORDER OF THE STEP (:176-186).  solver_base.step (grid from the current pos, acc = gravity), then externel_force_predict_pos:
    vel += dt * acc, pos_predict = pos + dt * vel (:26-30).  compute_all_lambda, compute_all_delta_pos and the density in them read
    `fluid_particles.pos`, the CURRENT positions -- pos_predict is used by nothing before update_all_pos.
 5. DETAILS.  rho starts at 0.001 (solver_base.py:44) and the wall sum enters as rho + rho_boundary * rho_0 (:49).  constrain =
    max(rho / rho_0 - 1, 0) (:130); constrain == 0.0 gives lambda = 0.0 (:39-40).  The denominator is (cd . cd + sum) + sum_boundary
    (:48), cd . cd + sum without walls (:50), plus epsilon = 1e-6 (:52).  s_corr is the quotient of two poly6 values, squared twice (the
    fourth power), then multiplied by -k (:148-151, :159-162).  Its divisor poly_kernel(s_corr_factor * kernel_h, kernel_h) has a
    Python-float argument: 0.3 * kernel_h is folded in f64 and rounded once, then divided by the f32 h like any other r.  The fluid factor is
    (lambda_i + lambda_j) + s_corr (:153), the wall factor lambda_i + s_corr (:164); delta_pos = (fluid sum + wall sum) / rho_0 (:63, :65).
 6. ARITHMETIC: the conventions of second_restatement.py, unchanged -- the h of a kernel function is an f32 value; a sub-expression of Python
    scalars only (64 * pi, -k, 0.3 * kernel_h) is folded in f64 and rounded once; ** by a literal integer is binary exponentiation; norm and
    dot associate as (x^2 + y^2) + z^2; no FMA; IEEE divide and sqrt.

Held against the oracle (tests/test_second_restatement.py) and the library's four kinds of handle (tests/test_second_restatement_gpu.py) this
reading met no disagreement in any field of any step.  The one finding was outside the step: sim.compute_density() re-sorts the particles and
carried pbf_lambda through the new order but not delta_pos, which then read back permuted; sph_compute_density carries both now.
"""
import math

import numpy as np

from second_restatement import F, Neighbours, Solver, _dot, _ipow, _norm


def poly_kernel(r, h):
    """solver_base.py:122-129"""
    q = r / h
    q2 = q * q
    ret = F(315) / (F(64 * math.pi) * _ipow(h, 3)) * _ipow(F(1) - q2, 3)
    return np.where(q <= F(1), ret, F(0.0))


def spiky_kernel_derivative(r, h):
    """solver_base.py:113-120: `- (45 * (1 - q) ** 2) * r / (pi * (h ** 4) * r_norm)`, the minus sign on the scalar factor"""
    r_norm = _norm(r)
    q = r_norm / h
    with np.errstate(divide="ignore", invalid="ignore"):
        ret = (-(F(45) * _ipow(F(1) - q, 2)))[..., None] * r / (F(math.pi) * _ipow(h, 4) * r_norm)[..., None]
    return np.where(((q <= F(1)) & (q > F(0)))[..., None], ret, F(0.0))


class PbfSolver(Solver):
    """pbf_solver on a Scene"""

    def __init__(self, config):
        assert config["solver"]["name"] == "pbf"
        super().__init__(config)
        self.epsilon, self.k, self.c, self.s_corr_factor = 1.0e-6, 1e-7, 9e-6, 0.3       # pbf_solver.py:17-21
        self.v_decay_proportion = 0.5                                                    # solver_base.py:18
        self.rho = np.zeros(self.N, dtype=F)
        self.pbf_lambda = np.zeros(self.N, dtype=F)                                      # :16
        self.delta_pos = np.zeros((self.N, 3), dtype=F)                                  # :14
        self.pos_predict = np.zeros((self.N, 3), dtype=F)                                # :13
        self.cell_changes = self.on_plane = 0                                            # evidence for the tests, per step
        self.xsph_max = 0.0

    def _spiky_f(self, j):
        return spiky_kernel_derivative(self.pos - self.pos[j], self.h)

    def _spiky_w(self, b):
        return spiky_kernel_derivative(self.pos - self.sc.wall_pos[b], self.h)

    def compute_all_rho(self):
        """solver_base.py:41-51 with pbf_solver.py:166-174 as its callbacks; writes rho and nothing else"""
        rho = np.full(self.N, F(0.001), dtype=F)
        for k in range(self.nf.kmax):
            live = k < self.nf.count
            j = self.nf.index[:, k]
            rho = np.where(live, rho + self.m * poly_kernel(_norm(self.pos - self.pos[j]), self.h), rho)
        if self.walls:
            rb = self._wall_sum((), lambda b: self.sc.wall_vol[b] * poly_kernel(_norm(self.pos - self.sc.wall_pos[b]), self.h))
            rho = rho + rb * self.rho_0
        self.rho = rho.astype(F)

    def density_only(self):
        """what a caller of compute_all_rho alone gets: the grid of the current positions (solver_base.step :139-141), then the sum"""
        self.prologue()
        self.compute_all_rho()

    def externel_force_predict_pos(self):
        """:26-30; acc is what reset() filled it with (solver_base.py:131-133)"""
        self.vel = self.vel + self.dt * np.tile(self.g_vec, (self.N, 1))
        self.pos_predict = self.pos + self.dt * self.vel

    def compute_all_lambda(self):
        """:32-52, :106-142"""
        self.compute_all_rho()
        c = self.rho / self.rho_0 - F(1.0)
        self.constrain = np.where(c > F(0.0), c, F(0.0)).astype(F)                       # ti.max(., 0.0) :130
        cd = self._fluid_sum((3,), lambda j: self._spiky_f(j) / self.rho_0)              # :109-110, :120
        if self.walls:
            cd = cd + self._wall_sum((3,), lambda b: self._spiky_w(b) / self.rho_0)      # :112-114, :124
        self.constrain_derivative = cd

        def around(g):
            ret = g / self.rho_0                                                         # :135-136, :141-142
            return _dot(ret, ret)

        s = self._fluid_sum((), lambda j: around(self._spiky_f(j)))
        if self.walls:
            s = (_dot(cd, cd) + s) + self._wall_sum((), lambda b: around(self._spiky_w(b)))      # :48
        else:
            s = _dot(cd, cd) + s                                                         # :50
        lam = -self.constrain / (s + F(self.epsilon))                                    # :52
        self.pbf_lambda = np.where(self.constrain == F(0.0), F(0.0), lam).astype(F)      # :39-40

    def _s_corr(self, x_ij_norm):
        """:148-151 = :159-162"""
        s = poly_kernel(x_ij_norm, self.h) / poly_kernel(F(self.s_corr_factor * self.kernel_h), self.h)
        s = s * s
        s = s * s
        return s * F(-self.k)

    def compute_all_delta_pos(self):
        """:55-65, :144-164"""
        lam = self.pbf_lambda

        def fterm(j):
            x_ij = self.pos - self.pos[j]
            return ((lam + lam[j]) + self._s_corr(_norm(x_ij)))[:, None] * spiky_kernel_derivative(x_ij, self.h)

        def wterm(b):
            x_ij = self.pos - self.sc.wall_pos[b]
            return (lam + self._s_corr(_norm(x_ij)))[:, None] * spiky_kernel_derivative(x_ij, self.h)

        d = self._fluid_sum((3,), fterm)
        if self.walls:
            d = d + self._wall_sum((3,), wterm)
        self.delta_pos = (d / self.rho_0).astype(F)

    def update_all_pos(self):
        """:66-96 under the schedule of convention 2, the neighbour set of convention 3"""
        old = self.pos
        pp = self.pos_predict + self.delta_pos                                           # phase 1
        vel = (pp - self.pos) / self.dt
        if not self.walls:
            for a in range(3):
                lo = F(self.sc.box_min[a]) + F(self.sc.radius)
                hi = F(self.sc.box_max[a]) - F(self.sc.radius)
                low = pp[:, a] <= lo
                pp[:, a] = np.where(low, lo, pp[:, a])
                vel[:, a] = np.where(low, vel[:, a] * F(self.v_decay_proportion), vel[:, a])
                high = pp[:, a] >= hi
                pp[:, a] = np.where(high, hi, pp[:, a])
                vel[:, a] = np.where(high, vel[:, a] * F(self.v_decay_proportion), vel[:, a])
        self.pos_predict, self.pos, self.vel = pp, pp.copy(), vel
        listed, self.nf = self.nf, Neighbours(self.sc, self.pos, self.pos, same=True, cell_centres=old, cell_others=old)      # phase 2
        v = self._fluid_sum((3,), lambda j: (self.vel[j] - self.vel) * poly_kernel(_norm(self.pos - self.pos[j]), self.h)[:, None])
        self.nf = listed
        self.vel = (self.vel + F(self.c) * v).astype(F)                                  # phase 3
        self.xsph = v
        self.cell_changes = int(np.any(self.sc.cell(old) != self.sc.cell(self.pos), axis=1).sum())
        self.xsph_max = float(np.abs(v).max())

    def step(self):
        """:176-186"""
        self.prologue()                                                                  # solver_base.step :136-143
        self.externel_force_predict_pos()
        self.compute_all_lambda()
        self.compute_all_delta_pos()
        self.update_all_pos()
