"""rigid_solver with the reference's surface (rigid_solver.py:4-31, 216-232): one rigid body driven by the forces the
fluid sweeps accumulate on its sample particles.  The per-particle parts (torque/force sums, rotation, wall test,
translation) are HIP kernels; the 3x3 algebra between them runs on the host inside the native library."""
import numpy as np

from . import _native as nat
from .fields import ScalarField


class rigid_solver:
    def __init__(self, particle_system, config):
        solid_config = config.get("solid")
        if not solid_config or not particle_system.exist_rigid[None]:
            raise ValueError("rigid_solver needs a config with a 'solid' block (main.py:69-71)")
        self.ps = particle_system
        self._sim = particle_system._sim
        self.gravity = config["scene"].get("gravity")
        self.rho = solid_config.get("rho_0")
        self.particle_count = self.ps.rigid_particles_num
        self.v_decay_proportion = 0.1                       # rigid_solver.py:24
        self.simulate_cnt_host = 0
        self.simulate_cnt = ScalarField(lambda: self.simulate_cnt_host)
        self.omega = ScalarField(lambda: np.asarray(self.ps._sim.rigid_scalars()["omega"], dtype=np.float32))
        self.mass = ScalarField(lambda: self.ps._sim.rigid_scalars()["mass"])
        # not the reference's: `"motion": {"mode": "fixed"}` or `{"mode": "scripted", "vel": [...], "omega": [...]}` in the solid block makes the
        # body an obstacle or a paddle (an absent key: the reference's dynamic body)
        motion = solid_config.get("motion")
        if motion:
            if motion.get("mode", "dynamic") not in nat.RIGID_MODES:
                raise ValueError("solid.motion.mode must be one of %s, got %r" % (sorted(nat.RIGID_MODES), motion.get("mode")))
            if "vel" in motion or "omega" in motion:
                self.set_motion(motion.get("vel", [0.0, 0.0, 0.0]), motion.get("omega", [0.0, 0.0, 0.0]), motion.get("acc"), motion.get("alpha"))
            self.mode = motion.get("mode", "dynamic")

    @property
    def mode(self):
        """"dynamic" (rigid_solver.step as in the reference), "scripted" (the body follows set_motion) or "fixed"; writable between steps"""
        number = self.ps._sim.rigid_scalars(motion=True)["mode"]
        return [name for name, value in nat.RIGID_MODES.items() if value == number][0]

    @mode.setter
    def mode(self, value):
        self.ps._sim.rigid_set_mode(value)

    def set_motion(self, vel, omega, acc=None, alpha=None):
        """the velocity and angular velocity a scripted body has from the next step() on (acc, alpha: what the fluid extrapolates them with)"""
        self.ps._sim.rigid_set_motion(vel, omega, acc, alpha)

    def load(self):
        """(force, torque about the centroid) of the fluid on the body, as the last step() summed them"""
        return self.ps._sim.rigid_load()

    def step(self):
        self.simulate_cnt_host += 1
        self.ps._sim.rigid_step()
