"""The yardstick of the static-geometry suites (TEST INFRASTRUCTURE: test_geometry_cpu.py, test_geometry_gpu.py, test_slab_geometry_gpu.py; nothing
here loads the HIP library).

tests/second_restatement.py and second_restatement_pbf.py read walls only through solver.sc.wall_pos, .wall_vol and .Nb and rebuild their neighbour
sets every step; they are imported unchanged.  `Walls` appends or removes groups on a built Solver and recomputes wall_vol with the
Neighbours(sc, wp, wp, same=True) loop of Scene.__init__ -- the f32 statement of DESIGN.md section 6l (the wall set is the box samples, then
every live group in order of addition; after every edit the volumes of ALL samples are recomputed), written independently of the library.

The test geometry on the tiny wall scenes (640 particles, d = 0.05, h = 0.1, 2 402 box samples): PLATE, 108 samples at x = 0.475, y = 0.05 .. 0.60,
z = 0.05 .. 0.45 on the d lattice; BLOCK, the 26-sample shell of a 3 x 3 x 3 block from (0.10, 0.05, 0.475); CARVE_PLATE, the plate moved to
x = 0.225, which stands in the fluid column."""
import numpy as np

import restatement_compare as rc
from harness import same_bits, same_values
from second_restatement import F, Neighbours, Solver, _norm, cubic_kernel
from second_restatement_pbf import PbfSolver

D = 0.05
SCENES = {"wcsph": "wcsph_tiny_wall", "dfsph": "dfsph_tiny_wall", "pcisph": "dfsph_tiny_wall_pcisph", "iisph": "dfsph_tiny_wall_iisph", "pbf": "pbf_tiny_wall"}


def plate_at(x):
    """12 x 9 samples, y outermost"""
    return np.array([[x, D * j, D * k] for j in range(1, 13) for k in range(1, 10)], dtype=F)


PLATE = plate_at(0.475)
CARVE_PLATE = plate_at(0.225)
BLOCK = np.array([[0.10 + D * i, 0.05 + D * j, 0.475 + D * k] for i in range(3) for j in range(3) for k in range(3) if (i, j, k) != (1, 1, 1)], dtype=F)

_VOLUMES = {}          # wall set (its bytes) -> volumes: a set is met by many tests, its N^2 sum is taken once


def volumes(sc, wp):
    """compute_all_boundary_volume (ParticleSystem.py:309-320) over `wp`, as Scene.__init__ takes it"""
    key = (tuple(sc.grid), float(sc.h), wp.tobytes())
    if key not in _VOLUMES:
        nb = Neighbours(sc, wp, wp, same=True)
        vol = np.zeros(len(wp), dtype=F)
        for k in range(nb.kmax):
            live = k < nb.count
            j = nb.index[:, k]
            q = _norm(wp - wp[j])
            vol = np.where(live, vol + cubic_kernel(q, sc.h), vol)
        with np.errstate(divide="ignore"):
            _VOLUMES[key] = F(1.0) / vol
    return _VOLUMES[key].copy()


class Walls:
    """the wall set of a built Solver under edits: group ids 1, 2, ... never reused, a removal closes the gap"""

    def __init__(self, solver):
        self.s, self.sc = solver, solver.sc
        self.box = solver.sc.wall_pos.copy()
        self.groups, self.next_id = [], 1

    def _apply(self):
        sc = self.sc
        sc.wall_pos = np.concatenate([self.box] + [p for _, p in self.groups]).astype(F)
        sc.Nb = len(sc.wall_pos)
        sc.wall_vol = volumes(sc, sc.wall_pos)

    def add(self, points):
        gid = self.next_id
        self.next_id += 1
        self.groups.append((gid, np.asarray(points, dtype=F).copy()))
        self._apply()
        return gid

    def remove(self, gid):
        assert gid in [g for g, _ in self.groups]
        self.groups = [(g, p) for g, p in self.groups if g != gid]
        self._apply()

    def info(self):
        out, at = [], len(self.box)
        for g, p in self.groups:
            out.append((g, at, len(p)))
            at += len(p)
        return out

    def carve_mask(self, pos, gid=-1, clearance=F(D)):
        """norm3(x_i - x_b) < clearance for some sample b of the group (-1: of any added group), f32, against every sample"""
        pts = np.concatenate([p for g, p in self.groups if gid in (-1, g)])
        d = pos[:, None, :] - pts[None, :, :]
        dist = np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])
        return (dist < F(clearance)).any(axis=1)


def keep_rows(s, keep):
    """the restatement given the survivors of a removal: what a step reads of the fluid, squeezed"""
    s.pos, s.vel, s.warm = s.pos[keep].copy(), s.vel[keep].copy(), s.warm[keep].copy()
    if hasattr(s, "p_past"):
        s.p_past = s.p_past[keep].copy()
    s.N = len(s.pos)


def make_solver(cfg):
    s = PbfSolver(cfg) if cfg["solver"]["name"] == "pbf" else Solver(cfg)
    return s, Walls(s)


def wall_evidence(s, walls):
    """after a step: how many particles list a sample of each live group, and the fullest wall row"""
    per = {}
    listed = np.arange(s.nw.index.shape[1])[None, :] < s.nw.count[:, None]
    for g, first, count in walls.info():
        per[g] = int((listed & (s.nw.index >= first) & (s.nw.index < first + count)).any(axis=1).sum())
    return per, int(s.nw.count.max())


def step_and_compare(s, sides, k, solver):
    """one step of the restatement and of every side (restatement_compare.NativeSide); fields, iteration counts and residuals on raw bits -- the
    step of restatement_compare.compare_run, for a run whose wall set changes between steps, and the number of wall entries of every particle's list"""
    with np.errstate(all="ignore"):
        s.step()
    for side in sides:
        st = side.step()
        when = "%s, step %d" % (side.label, k)
        if solver == "dfsph":
            mine = (s.n_div, s.n_dens, F(s.div_first), F(s.div_err), F(s.dens_err), F(s.dt))
            assert mine == (st.n_div, st.n_dens, F(st.div_first_err), F(st.div_err), F(st.dens_err), F(st.dt)), (when, mine)
        elif solver not in ("wcsph", "pbf"):
            assert (s.n_dens, F(s.dens_err)) == (st.n_dens, F(st.dens_err)), (when, s.n_dens, st.n_dens, s.dens_err, st.dens_err)
        for attr, name in rc.FIELDS[solver].items():
            same_bits(getattr(s, attr), side.get(name), "%s: %s" % (when, attr))
        if s.nw is not None:           # the wall lists themselves, particle by particle, not only their sums
            same_values(side.sim.wall_neighbor_counts(), s.nw.count.astype(np.int32), "%s: wall neighbours per particle" % when)
