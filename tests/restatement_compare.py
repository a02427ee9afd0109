"""The step-by-step comparison tests/test_second_restatement.py (the oracle) and tests/test_second_restatement_gpu.py (the library) share:
one run of the second restatement, any number of other sides in lockstep, every field compared on raw bits after every step, and a record
of what the run exercised.  TEST INFRASTRUCTURE ONLY."""
import numpy as np

from harness import same_bits
from second_restatement import Solver
from second_restatement_pbf import PbfSolver

F_ID = {"pos": 0, "vel": 1, "acc": 2, "rho": 3, "pressure": 4, "alpha": 5, "warm": 6, "rho_adv": 7, "rho_derivative": 8, "vel_adv": 9,
        "ncount": 14, "press_iter": 16, "press_force": 17, "pos_predict": 18, "d_ii": 19, "a_ii": 20, "d_ij": 21,
        "pbf_lambda": 22, "pbf_delta_pos": 23,
        "rigid_pos": 48, "rigid_vol": 49, "rigid_force": 50, "rigid_vert": 52}       # include/sph_mi355x.h = oracle/sph_oracle.h
# restatement attribute -> field, per solver
FIELDS = {
    "wcsph": {"rho": "rho", "pressure": "pressure", "acc": "acc", "vel": "vel", "pos": "pos"},
    "dfsph": {"rho": "rho", "alpha": "alpha", "rho_derivative": "rho_derivative", "warm": "warm", "rho_adv": "rho_adv", "vel_adv": "vel_adv",
              "ncount": "ncount", "vel": "vel", "pos": "pos"},
    "pcisph": {"rho": "rho", "press_iter": "press_iter", "pos_predict": "pos_predict", "press_force": "press_force", "vel": "vel", "pos": "pos"},
    "iisph": {"rho": "rho", "p_iter": "press_iter", "f_press": "press_force", "d_ii": "d_ii", "a_ii": "a_ii", "d_ij": "d_ij", "vel": "vel", "pos": "pos"},
    "pbf": {"rho": "rho", "pbf_lambda": "pbf_lambda", "delta_pos": "pbf_delta_pos", "vel": "vel", "pos": "pos"},
}


class OracleSide:
    label = "oracle"

    def __init__(self, cfg, rg, solver):
        from oracle import oracle as orc
        self.solver = solver
        self.o = orc.Oracle(cfg, solver=solver, rigid=rg)

    def sizes(self):
        return self.o.N, self.o.Nb, self.o.Nr

    def set_state(self, pos, vel):
        self.o.set(F_ID["pos"], pos)
        self.o.set(F_ID["vel"], vel)

    def get(self, name):
        return self.o.get(F_ID[name])

    def pcisph(self):
        return self.o.pcisph_delta, self.o.pcisph_max_index

    def ncount_before_step(self):
        """get_neighbour_count on the grid the coming step will build (the oracle keeps the count per step for dfsph only)"""
        self.o.build_grid()
        self.o.compute_nbr_count()
        return self.o.get(F_ID["ncount"])

    def ncount_after_step(self):
        return None

    def density_only(self):
        self.o.build_grid()
        self.o.compute_rho()

    def step(self):
        if self.solver == "dfsph":
            self.o.step_dfsph(1, 100)
        else:
            getattr(self.o, "step_" + self.solver)(1)
        return self.o.last_stats

    def rigid_step(self):
        self.o.rigid_step()

    def rigid_scalars(self):
        return self.o.rigid_scalars()

    def close(self):
        self.o.close()


class NativeSide:
    """the library through its C ABI: download(F_*, SPECIES_*), scalars, StepStats"""

    def __init__(self, cfg, rg, solver, label="library"):
        from cfd_taichi_amd import _native as nat
        self.nat, self.solver, self.label = nat, solver, label
        self.sim = nat.Simulation(nat.config_from_dict(cfg, max_density_iters=100 if solver == "dfsph" else 0), rigid=rg)

    def sizes(self):
        return self.sim.n_fluid, self.sim.n_wall, self.sim.n_rigid

    def set_state(self, pos, vel):
        self.sim.upload(self.nat.F_POS, pos)
        self.sim.upload(self.nat.F_VEL, vel)

    def get(self, name):
        return self.sim.download(F_ID[name], self.nat.SPECIES_RIGID if name.startswith("rigid_") else self.nat.SPECIES_FLUID)

    def pcisph(self):
        s = self.sim.scalar
        return s(self.nat.S_PCISPH_DELTA), (int(s(self.nat.S_PCISPH_MAX_INDEX)), int(s(self.nat.S_PCISPH_MAX_COUNT)))

    def ncount_before_step(self):
        return None

    def ncount_after_step(self):
        """the count of the step's own list build"""
        return self.get("ncount")

    def density_only(self):
        self.sim.compute_density()

    def step(self):
        return getattr(self.sim, "step_" + self.solver)(1)

    def rigid_step(self):
        self.sim.rigid_step()

    def rigid_scalars(self):
        return self.sim.rigid_scalars()

    def close(self):
        self.sim.close()


def compare_run(cfg, steps, sides, state=None, rg=None, density_after=False):
    """Step the second restatement `steps` times and every side with it; after EVERY step compare the solver's fields, its iteration counts
    and residuals (pbf has none), and (with a body) the per-sample forces, then rigid_step everywhere (main.py:165-173) and compare the body.
    `sides`: callables (cfg, rg, solver) -> OracleSide / NativeSide.  density_after (pbf): after the last step compute_all_rho alone on every
    side -- rho as the restatement's, every other field of FIELDS left bit for bit as it was.  Returns what the run exercised."""
    solver = cfg["solver"]["name"]
    s = PbfSolver(cfg) if solver == "pbf" else Solver(cfg, rg)
    if solver == "dfsph" and rg is not None:
        s.max_dens = 100
    sides = [make(cfg, rg, solver) for make in sides]
    b = s.body
    ev = {"iters": [], "hit_steps": [], "force": [], "quirk": 0, "vy": [], "on_plane": 0, "minus_zero": 0,
          "lambda_active": [], "xsph_max": [], "cell_changes": []}                   # pbf, per step
    count_too = solver == "pcisph" and b is not None and b.active     # dfsph has ncount among its FIELDS; pcisph uses it at construction only
    r = np.float32(s.sc.radius if solver != "wcsph" else s.sc.diameter)
    lo, hi = np.array(s.sc.box_min, dtype=np.float32) + r, np.array(s.sc.box_max, dtype=np.float32) - r
    try:
        for side in sides:
            assert side.sizes() == (s.N, s.sc.Nb, b.Nr if b is not None else 0), side.label
            if state is not None:
                side.set_state(*state)
        if state is not None:
            s.pos, s.vel = state[0].copy(), state[1].copy()
        with np.errstate(all="ignore"):
            if solver == "pcisph":
                for side in sides:
                    delta, max_index = side.pcisph()
                    assert np.float32(delta) == s.delta and max_index == (s.max_index, s.max_count), (side.label, delta, s.delta, max_index, s.max_index, s.max_count)
            if b is not None:
                for side in sides:
                    _same_body(b, side, "at creation", b.active)
                    same_bits(b.vol, side.get("rigid_vol"), "%s: sample volumes" % side.label)
            for k in range(1, steps + 1):
                before = [side.ncount_before_step() if count_too else None for side in sides]
                s.step()
                for side, nc in zip(sides, before):
                    st = side.step()
                    when = "%s, step %d" % (side.label, k)
                    if count_too:
                        same_bits(s.ncount, nc if nc is not None else side.ncount_after_step(), "%s: ncount" % when)
                    if solver == "dfsph":
                        mine = (s.n_div, s.n_dens, np.float32(s.div_first), np.float32(s.div_err), np.float32(s.dens_err), np.float32(s.dt))
                        assert mine == (st.n_div, st.n_dens, np.float32(st.div_first_err), np.float32(st.div_err), np.float32(st.dens_err), np.float32(st.dt)), (when, mine)
                    elif solver not in ("wcsph", "pbf"):
                        assert (s.n_dens, np.float32(s.dens_err)) == (st.n_dens, np.float32(st.dens_err)), (when, s.n_dens, st.n_dens, s.dens_err, st.dens_err)
                    for attr, name in FIELDS[solver].items():
                        same_bits(getattr(s, attr), side.get(name), "%s: %s" % (when, attr))
                    if b is not None:
                        same_bits(b.force, side.get("rigid_force"), "%s: per-sample force" % when)
                ev["iters"].append((s.n_div, s.n_dens) if solver == "dfsph" else s.n_dens)
                if solver == "pbf":
                    ev["lambda_active"].append(int((s.pbf_lambda != 0).sum()))
                    ev["xsph_max"].append(s.xsph_max)
                    ev["cell_changes"].append(s.cell_changes)
                if not s.walls:
                    ev["on_plane"] += int(((s.pos == lo) | (s.pos == hi)).sum())          # the clamp branch put them there
                    if solver == "pcisph":
                        ev["minus_zero"] += int(((s.press_force == 0) & np.signbit(s.press_force)).sum())
                if b is not None:
                    ev["force"].append(float(np.abs(b.force).max()))
                    if b.active:
                        ev["quirk"] += int((s.ncount != s.nf.ok[:, :s.N].sum(axis=1)).sum())
                        s.rigid_step()
                        if b.hit:
                            ev["hit_steps"].append(k)
                        ev["vy"].append(float(b.vel[1]))
                        for side in sides:
                            side.rigid_step()
                            _same_body(b, side, "after rigid step %d" % k, True)
            if density_after:
                s.density_only()
                for side in sides:
                    kept = {name: side.get(name).copy() for name in FIELDS[solver].values() if name != "rho"}
                    side.density_only()
                    same_bits(s.rho, side.get("rho"), "%s: rho of compute_all_rho alone" % side.label)
                    for name, was in kept.items():
                        same_bits(was, side.get(name), "%s: %s across compute_all_rho alone" % (side.label, name))
                for attr, name in FIELDS[solver].items():       # ... and the restatement's own
                    same_bits(getattr(s, attr), sides[0].get(name), "%s after compute_all_rho alone" % attr)
    finally:
        for side in sides:
            side.close()
    ev["solver"] = s
    ev["outside_deposits"] = s.outside_deposits
    return ev


def _same_body(b, side, when, finite):
    sc = side.rigid_scalars()
    same_bits(b.pos, side.get("rigid_pos"), "%s: sample positions %s" % (side.label, when))
    same_bits(b.vert, side.get("rigid_vert"), "%s: vertices %s" % (side.label, when))
    if finite:
        for mine, key in ((b.centroid, "centroid"), (b.vel, "vel"), (b.omega, "omega"), (b.inertia_inv.ravel(), "inertia_inv")):
            same_bits(mine, sc[key], "%s: %s %s" % (side.label, key, when))
