"""A body whose motion is given, or that does not move, beside the second restatement (tests/second_restatement_rigid.py): the contract of
sph_rigid_step per body mode (include/sph_mi355x.h) restated in numpy f32, and the library sides that follow the same
plan.  TEST INFRASTRUCTURE ONLY.

A PLAN is a callable k -> (mode, motion): what the k-th body step (1, 2, ...) does.  motion is None (keep what was set) or (vel, omega, acc,
alpha), acc and alpha possibly None (zeros).  `constant`, `replay` and `let_go` build the plans of the tests.

second_restatement.Solver imports Body when it is constructed, so
    monkeypatch.setattr(second_restatement_rigid, "Body", body_class(plan))
puts a ScriptedBody into restatement_compare.compare_run unchanged; the library sides come from `sides(monkeypatch, plan)`."""
import numpy as np

import restatement_compare as rc
from harness import bits_equal, same_bits
import second_restatement_rigid as srr
from second_restatement import F, _cross

DYNAMIC, SCRIPTED, FIXED = 0, 1, 2


def constant(mode, vel=None, omega=None, acc=None, alpha=None):
    motion = None if vel is None else (vel, omega, acc, alpha)
    return lambda k: (mode, motion)


def replay(recording):
    """recording[k - 1]: (vel, omega, acc, alpha) a dynamic body had after its k-th step"""
    return lambda k: (SCRIPTED, recording[k - 1])


def let_go(fixed_steps):
    return lambda k: (FIXED if k <= fixed_steps else DYNAMIC, None)


def _vec(v):
    return np.zeros(3, dtype=F) if v is None else np.asarray(v, dtype=F).copy()


class ScriptedBody(srr.Body):
    plan = staticmethod(constant(DYNAMIC))
    current = None              # the body of the run in progress: the library sides compare their load with its

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        self.steps = 0
        self.motion = (_vec(None), _vec(None), _vec(None), _vec(None))
        self.load = None
        self.recording = []
        type(self).current = ScriptedBody.current = self

    def step(self, dt, gravity):
        self.steps += 1
        mode, motion = self.plan(self.steps)
        if motion is not None:
            self.motion = tuple(_vec(v) for v in motion)
        with np.errstate(all="ignore"):
            # every mode: the sums over the samples' forces, the torque about the centroid before the move (convention 7: exact, rounded once)
            self.load = (srr._exact(self.force), srr._exact(_cross(self.pos - self.centroid, self.force)))
            if mode == DYNAMIC:
                super().step(dt, gravity)
            elif mode == SCRIPTED:
                vel, omega, acc, alpha = self.motion
                self.omega = omega.copy()                                   # 1.
                self.attitude = self.omega * dt
                self.s_alpha = alpha.copy()
                self.rotation()                                             # 2. (always, also by zero angles: (p - c) + c is not p)
                self.force = np.zeros((self.Nr, 3), dtype=F)
                self.acc, self.vel = acc.copy(), vel.copy()                 # 3.
                disp = self.vel * dt
                self.hit = 0                                                # 4. no wall test, no impulse
                self.pos = self.pos + disp                                  # 5.
                self.vert = self.vert + disp
                self.centroid = self.centroid + disp
                self.s_omega = self.omega.copy()
            else:
                self.force = np.zeros((self.Nr, 3), dtype=F)
                self.hit = 0
                self.vel, self.acc, self.omega = _vec(None), _vec(None), _vec(None)
                self.s_omega, self.s_alpha = _vec(None), _vec(None)
        self.recording.append((self.vel.copy(), self.s_omega.copy(), self.acc.copy(), self.s_alpha.copy()))


def body_class(plan):
    return type("PlannedBody", (ScriptedBody,), {"plan": staticmethod(plan)})


class PlannedSide(rc.NativeSide):
    """the library following the plan: mode and motion set before the body step they belong to, the load compared after it"""

    def __init__(self, cfg, rg, solver, label, plan):
        super().__init__(cfg, rg, solver, label)
        self.plan, self.steps = plan, 0
        self.start = (self.get("rigid_pos").copy(), self.get("rigid_vert").copy())

    def rigid_step(self):
        self.steps += 1
        mode, motion = self.plan(self.steps)
        self.sim.rigid_set_mode(mode)
        if motion is not None:
            self.sim.rigid_set_motion(*motion)
        self.sim.rigid_step()
        b = ScriptedBody.current
        force, torque = self.sim.rigid_load()
        same_bits(b.load[0], force.astype(np.float32), "%s: load, force, body step %d" % (self.label, self.steps))
        same_bits(b.load[1], torque.astype(np.float32), "%s: load, torque, body step %d" % (self.label, self.steps))
        sc = self.sim.rigid_scalars(motion=True)
        same_bits(b.acc, sc["acc"], "%s: acc, body step %d" % (self.label, self.steps))
        same_bits(b.s_alpha, sc["alpha"], "%s: alpha, body step %d" % (self.label, self.steps))
        assert sc["mode"] == mode
        if all(self.plan(k)[0] == FIXED for k in range(1, self.steps + 1)):       # fixed so far: the bits of creation
            assert bits_equal(self.start[0], self.get("rigid_pos")), "%s: a fixed body's samples moved" % self.label
            assert bits_equal(self.start[1], self.get("rigid_vert")), "%s: a fixed body's vertices moved" % self.label


def sides(monkeypatch, plan):
    """a default handle and one under SPH_CELL_ORDER=morton, as test_second_restatement_gpu.handles makes them"""
    def default(cfg, rg, solver):
        monkeypatch.delenv("SPH_CELL_ORDER", raising=False)
        return PlannedSide(cfg, rg, solver, "library (default handle)", plan)

    def morton(cfg, rg, solver):
        monkeypatch.setenv("SPH_CELL_ORDER", "morton")
        monkeypatch.setenv("SPH_CELL_TILE", "4")
        side = PlannedSide(cfg, rg, solver, "library (SPH_CELL_ORDER=morton)", plan)
        assert "SPH_CELL_ORDER=morton" in side.sim.overrides(), side.sim.overrides()
        return side

    return [default, morton]
