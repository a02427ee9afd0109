/*
 * sph_mi355x.h -- C-ABI of the MI355X-native SPH step library (libsph_mi355x.so).
 *
 * The reference (Jukgei/CFD_Taichi @ 2024_08_07) has no FFI: its per-step path is Python
 * driving Taichi-JIT kernels, and the only caller contract is main.py:64-71,165-173
 * (`ParticleSystem(config)`, `<name>_solver(ps, config)`, `solver.step()`,
 * `solver.delta_time[None]`, `ps.fluid_particles.pos.to_numpy()`).  This header is what a
 * ctypes binding for that path binds instead; each entry point names the reference
 * interface it replaces.  Plain pointers and sizes only, no torch / HIP types.
 *
 * Conventions: every call returns SPH_OK (0) or a negative SPH_E_* code and never throws;
 * sph_last_error() gives the message of the last failing call on that handle (or of the
 * last failing sph_create when handle == NULL).  One host thread per handle, one HIP
 * stream per handle, no global state.  Host pointers are borrowed for the call only.
 * Particle data crosses the ABI in ORIGINAL particle order (the order of
 * ParticleSystem.init_particle_pos, ParticleSystem.py:142-151), f32, 3 floats per vector.
 */
#ifndef SPH_MI355X_H
#define SPH_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Version of this interface.  It changes whenever a struct grows or a signature changes (round 4: sph_replan_slabs gained ghost_layers, SphComm
 * gained exchange_counts_n / reduce_capacity; round 5: SPH_P_* scalars).  A binding checks sph_abi_version() == SPH_ABI_VERSION when it loads the
 * library (cfd_taichi_amd/_native.py does) instead of finding out through a misread struct. */
#define SPH_ABI_VERSION 5
int32_t sph_abi_version(void);

#define SPH_OK 0
#define SPH_E_INVALID (-1)   /* bad argument / size mismatch */
#define SPH_E_HIP (-2)       /* HIP runtime error (message has hipGetErrorString) */
#define SPH_E_NO_DEVICE (-3) /* no gfx950 device visible: the library has no CPU fallback */
#define SPH_E_OVERFLOW (-4)  /* a neighbour list overflowed its capacity.  Detected at the step's first read-back (wcsph: after the nsteps of the
                              * call), i.e. after sweeps have already run on truncated lists: the handle's particle state is UNDEFINED
                              * afterwards -- recreate the handle with a larger max_neighbors, or re-upload positions and velocities */
#define SPH_E_STATE (-5)     /* call not valid for this handle (e.g. dfsph step on a wcsph handle) */

#define SPH_SOLVER_WCSPH 0
#define SPH_SOLVER_DFSPH 1
#define SPH_SOLVER_PCISPH 2   /* pcisph_solver.py */
#define SPH_SOLVER_IISPH 3    /* iisph_solver.py */
#define SPH_SOLVER_PBF 4      /* pbf_solver.py (stale in the reference: read as csrc/sph_pbf_kernels.h states; no rigid body) */
/* (all five run on slab handles; wcsph, dfsph, pcisph and iisph with or without a coupled rigid body: sph_create_rigid) */

/* config/X.json of the reference, flattened (utils.py:3-11 reads it,
 * ParticleSystem.py:31-103 and solver_base.py:7-39 consume it).  Doubles carry the Python
 * scalars unrounded; the library rounds to f32 exactly where Taichi would. */
typedef struct SphConfig {
    double box_min[3];          /* scene.box_min */
    double box_max[3];          /* scene.box_max */
    double particle_radius;     /* scene.particle_radius */
    double gravity;             /* scene.gravity */
    double delta_time;          /* solver.delta_time */
    double start_pos[3];        /* fluid.start_pos */
    double water_size[3];       /* fluid.water_size */
    int32_t boundary_handle;    /* solver.boundary_handle (default 1: Akinci wall particles) */
    int32_t fs_couple;          /* solver.fs_couple (default 1) */
    int32_t solver;             /* SPH_SOLVER_* (solver.name) */
    int32_t device;             /* HIP device ordinal */
    int32_t max_neighbors;      /* fluid neighbour-list rows per particle; 0 = default (64) */
    int32_t max_wall_neighbors; /* wall neighbour-list rows per particle; 0 = default (64) */
    int32_t max_density_iters;  /* cap on correct_density_error (reference has none, dfsph_solver.py:225); 0 = default (100); reported in SphStepStats.capped */
    int32_t slab_rank;          /* multi-GPU x-slab rank, 0 for single GPU */
    int32_t slab_count;         /* number of slabs (world size), 0 or 1 for single GPU */
    int32_t slab_capacity;      /* particles (owned + ghosts) a slab handle can hold; 0 = default (1.75 N / slab_count + 256k) */
    int32_t slab_rebalance_every; /* re-cut the slabs from the current particle distribution every M steps; 0 = static cuts */
    int32_t arith;              /* SPH_ARITH_EXACT (0, default): every f32 operation of the reference in its order, bit-equal to oracle/;
                                   SPH_ARITH_RELAXED (1): the pair sweeps of every fluid solver (wcsph, dfsph, pcisph, iisph, pbf) may use
                                   approximate reciprocal square roots, FMA contraction and regrouped constant factors (north_star's 1e-5
                                   bar; see csrc/sph_relaxed_kernels.h, KF<true> in csrc/sph_device.h and RX in csrc/sph_pbf_kernels.h).
                                   A permission: handles the relaxed sweeps do not cover run the exact ones. */
    int32_t slab_ghost_layers;  /* slab handles: ghost cell columns per side.  0 = default: 2 for dfsph (the correction sweeps run on the inner
                                   ghost column too, so a solver iteration needs ONE halo refresh -- the residual's -- instead of two), 1 for
                                   the other solvers; 1 forces the one-column protocol.  Results do not depend on it. */
    int32_t slab_overlap;       /* slab handles, dfsph: the OVERLAPPED protocol runs the residual sweeps' edge tiles first, the halo of their results on a
                                   second stream under the interior tiles, and the residual's all-reduce + loop decision on a third under the next
                                   correction sweep; the IN-ORDER one runs everything on the handle's stream (same bits).  0 = default: the handle can do
                                   both and starts with the one that measured faster for its transport (native RCCL: in order, with the residual's
                                   triple riding in the halo's transfers; a synchronous callback transport: overlapped) -- sph_slab_set_overlap switches
                                   between steps; 1 = in order only (no second / third stream); 2 = start overlapped.  What "can do both" costs: two more
                                   HIP streams, four events, a tile order and 20 bytes per particle of slab capacity (what a divergence correction that
                                   runs ahead of its loop decision overwrites) -- allocated with the handle; pass 1 where that memory matters */
    int32_t fluid_capacity;     /* fluid particles the handle can ever hold (sph_add_particles); 0 = default: the lattice's own count, a handle whose
                                   count never changes.  > 0: at least the lattice's count and below 2^28; every per-particle array, the cell order
                                   (Morton from 2^17 particles, wcsph 2^19) and the staging of the sweeps are sized and chosen by it, the sweeps of a
                                   step by the live count.  SPH_E_INVALID on slab handles (slab_count > 1) and with a rigid body (sph_create_rigid) */
    int32_t reserved[1];
} SphConfig;

#define SPH_ARITH_EXACT 0
#define SPH_ARITH_RELAXED 1

typedef struct SphSizes {
    int32_t n_fluid;            /* ps.particle_num                 ParticleSystem.py:85 (the live count: sph_add_particles / sph_remove_in_box) */
    int32_t n_wall;             /* ps.boundary_particles_num       ParticleSystem.py:95 */
    int32_t n_rigid;            /* ps.rigid_particles_num */
    int32_t grid[3];            /* ps.grid_num                     ParticleSystem.py:101 */
    int32_t n_cells;
    int32_t max_neighbors;
    int32_t max_wall_neighbors;
} SphSizes;

/* what dfsph_solver.py prints at :233 and :416, plus health counters */
typedef struct SphStepStats {
    int32_t n_div;              /* divergence iterations */
    int32_t n_dens;             /* density iterations */
    int32_t n_div_evals;        /* derivative_iter_all_rho evaluations */
    int32_t capped;             /* 1 if max_density_iters stopped the density loop */
    float div_first_err;
    float div_err;
    float dens_err;             /* rho_avg - rho_0 */
    float dt;                   /* delta_time after the step */
    int32_t max_nbrs;           /* largest fluid-neighbour count seen in the last list build */
    int32_t max_wall_nbrs;
    int32_t lost;               /* particles outside the grid (reference prints an error, ParticleSystem.py:393-395) */
    int32_t reserved;
} SphStepStats;

/* the `solid` block of the reference's config (ParticleSystem.py:41-64) after mesh loading: sample points
 * (trimesh voxelized(pitch).fill().points in the reference; cfd_taichi_amd/mesh.py here) and mesh vertices, both in the
 * mesh frame, before attitude_offset / pos_offset are applied */
typedef struct SphRigid {
    int32_t n_particles;
    int32_t n_vertices;
    const float *points;         /* 3 * n_particles */
    const float *vertices;       /* 3 * n_vertices */
    double rho_0;                /* solid.rho_0 */
    double pos_offset[3];        /* solid.pos_offset */
    double attitude_offset[3];   /* solid.attitude_offset, degrees */
    int32_t active;              /* solid.active */
    int32_t reserved;
} SphRigid;

/* species for upload / download */
#define SPH_SPECIES_FLUID 0
#define SPH_SPECIES_WALL 1
#define SPH_SPECIES_RIGID 2

/* fields (fluid unless stated).  Vectors are 3 floats per particle. */
#define SPH_F_POS 0        /* fluid_particles.pos   (upload + download) */
#define SPH_F_VEL 1        /* fluid_particles.vel   (upload + download) */
#define SPH_F_ACC 2        /* fluid_particles.acc   (wcsph only, download) */
#define SPH_F_RHO 3        /* solver.rho */
#define SPH_F_PRESSURE 4   /* wcsph solver.pressure */
#define SPH_F_ALPHA 5      /* dfsph solver.alpha */
#define SPH_F_WARM_K 6     /* dfsph solver.warm_start_k (upload + download) */
#define SPH_F_RHO_ADV 7    /* dfsph solver.rho_adv */
#define SPH_F_RHO_DER 8    /* dfsph solver.rho_derivative */
#define SPH_F_VEL_ADV 9    /* dfsph solver.vel_adv */
#define SPH_F_NBR_COUNT 14 /* ps.get_neighbour_count(i), as float */
#define SPH_F_PRESS_ITER 16  /* pcisph solver.press_iter / iisph solver.p_iter after the last step */
#define SPH_F_PRESS_FORCE 17 /* pcisph solver.press_force / iisph solver.f_press */
#define SPH_F_POS_PREDICT 18 /* pcisph solver.pos_predict (pbf: equals pos after a step, pbf_solver.py:84) */
#define SPH_F_D_II 19        /* iisph solver.d_ii */
#define SPH_F_A_II 20        /* iisph solver.a_ii */
#define SPH_F_D_IJ 21        /* iisph solver.d_ij */
#define SPH_F_PBF_LAMBDA 22  /* pbf solver.pbf_lambda of the last step */
#define SPH_F_PBF_DELTA_POS 23 /* pbf solver.delta_pos of the last step */
#define SPH_F_WALL_POS 32  /* boundary_particles.pos    (species WALL) */
#define SPH_F_WALL_VOL 33  /* boundary_particles.volume (species WALL) */
#define SPH_F_RIGID_POS 48    /* rigid_particles.pos    (species RIGID) */
#define SPH_F_RIGID_VOL 49    /* rigid_particles.volume */
#define SPH_F_RIGID_FORCE 50  /* rigid_particles.force */
#define SPH_F_RIGID_MASS 51   /* rigid_particles.mass */
#define SPH_F_RIGID_VERT 52   /* ps.rigid_vertices (mesh vertices, for OBJ export) */

/* scalars for sph_get_scalar */
#define SPH_S_DELTA_TIME 0     /* solver.delta_time[None] */
#define SPH_S_SIMULATE_CNT 1   /* solver.simulate_cnt[None] */
#define SPH_S_PARTICLE_M 2     /* ps.particle_m */
#define SPH_S_SUPPORT_RADIUS 3 /* ps.support_radius */
#define SPH_S_PS_DELTA_TIME 4  /* ps.delta_time[None] */
#define SPH_S_GRAPH_LAUNCHES 5 /* diagnostics: hipGraph replays issued by sph_step_wcsph (each replays two steps) */
#define SPH_S_PCISPH_DELTA 6   /* pcisph solver.delta[None]         pcisph_solver.py:47 */
#define SPH_S_PCISPH_BETA 7    /* pcisph solver.beta                :23 */
#define SPH_S_PCISPH_MAX_INDEX 8 /* ps.get_max_neighbor_particle_index()  ParticleSystem.py:410-422 (single-thread reading) */
#define SPH_S_PCISPH_MAX_COUNT 9
#define SPH_S_RIGID_CENTROID 10   /* +0,1,2: ps.rigid_centriod[None] */
#define SPH_S_RIGID_OMEGA 13      /* +0,1,2: rigid_solver.omega[None] */
#define SPH_S_RIGID_VEL 16        /* +0,1,2: rigid_particles.vel (uniform over the body) */
#define SPH_S_RIGID_MASS 19       /* rigid_solver.mass[None] */
#define SPH_S_RIGID_INERTIA_INV 20 /* +0..8: ps.rigid_inertia_tensor_inv[None], row major */
#define SPH_S_RIGID_ACTIVE 32      /* ps.active_rigid[None] as it stands (sph_rigid_set_active writes it); 0 on a handle without a body */
#define SPH_S_RIGID_ACC 33         /* +0,1,2: rigid_particles.acc (uniform over the body): what the sweeps add to the body's velocity as acc * dt */
#define SPH_S_RIGID_ALPHA 36       /* +0,1,2: rigid_particles.alpha (uniform over the body) */
#define SPH_S_RIGID_MODE 39        /* SPH_RIGID_DYNAMIC / _SCRIPTED / _FIXED as sph_rigid_set_mode left it; 0 on a handle without a body */
#define SPH_S_TIME 40              /* the handle's simulated time, a device-resident f64: 0 at creation, += (double)delta_time at the end of every solver
                                    * step (dfsph: the CFL value the step leaves).  Writable through sph_set_scalar with a finite value */
#define SPH_S_ACCEL 41             /* +0,1,2: the acceleration vector as the last solver step used it, or as the next will if none has run since
                                    * sph_set_gravity / sph_set_forcing / a written SPH_S_TIME */
#define SPH_S_GRAVITY_VEC 44       /* +0,1,2: the base vector g of sph_set_gravity (default: scene.gravity * (0, -1, 0) in f32) */
#define SPH_S_FLUID_CAPACITY 47     /* read-only: fluid particles the handle can hold (SphConfig.fluid_capacity, or the lattice's count); SphSizes.n_fluid is
                                    * the live count */
#define SPH_S_VERLET_BUILDS 31    /* diagnostics: list builds so far on a Verlet handle (wcsph under the relaxed arithmetic: the lists carry a skin and are rebuilt on demand) */
#define SPH_S_PAIR_BITS 48          /* diagnostics, read-only: 1 if the solver-loop sweeps of the last dfsph step took the root's rounding step from the per-step
                                      pair-bit cache (staged 16-bit lists of a one-GPU handle without a binned body, exact arithmetic), else 0 */
#define SPH_S_ARITH_RELAXED 30    /* diagnostics: 1 if any pair sweep of this handle's solver runs the tolerance-grade kernels (SphConfig.arith asked AND the handle qualifies) */

/* Solver attributes a caller of the reference edits on the solver object after constructing it -- sph_set_scalar / sph_get_scalar.
 * The defaults are the reference's.  The dfsph loop attributes (64-68) are read by Python-scope loops at every step (dfsph_solver.py:225, :400)
 * and may be written between steps; the others are baked into Taichi kernels when they first compile, so the mirror classes
 * (cfd_taichi_amd/solver_base.py) forward them once, at the first step().  On slab handles every rank must write the same values. */
#define SPH_P_DENSITY_THRESHOLD 64                 /* dfsph_solver.density_threshold (percent of rho_0)      dfsph_solver.py:22, :225 */
#define SPH_P_MIN_ITERATION_DENSITY 65             /* dfsph_solver.min_iteration_density                     :21, :225 */
#define SPH_P_MIN_ITERATION_DENSITY_DIVERGENCE 66  /* dfsph_solver.min_iteration_density_divergence          :23, :400 */
#define SPH_P_MAX_ITERATION_DENSITY_DIVERGENCE 67  /* dfsph_solver.max_iteration_density_divergence          :24, :400 */
#define SPH_P_DENSITY_DIVERGENCE_THRESHOLD 68      /* dfsph_solver.density_divergence_threshold              :25, :400 */
#define SPH_P_WARM_START 69                        /* dfsph_solver.warm_start (0 / 1)                        :26, :396, :404 */
#define SPH_P_ADAPTIVE_DT 70                       /* dfsph_solver.adaptive_dt (0 / 1)                       :27, :113 */
#define SPH_P_MAX_DT 71                            /* dfsph_solver.max_dt                                    :28, :114-115 */
#define SPH_P_MIN_DT 72                            /* dfsph_solver.min_dt                                    :29, :117 */
#define SPH_P_VISCOSITY_C_S 73                     /* solver.viscosity_c_s      solver_base.py:24 (13), wcsph_solver.py:18 (10); :187 */
#define SPH_P_VISCOSITY_ALPHA 74                   /* solver.viscosity_alpha    solver_base.py:25, :187 */
#define SPH_P_VISCOSITY_EPSILON 75                 /* solver.viscosity_epsilon  solver_base.py:23, :188 */
#define SPH_P_TENSION_K 76                         /* solver.tension_k          solver_base.py:26 (0.5), wcsph_solver.py:20 (0.2); :216 */
/* The adaptive time step of wcsph, pcisph, iisph and pbf handles on one GPU -- this library's own: the reference adapts delta_time under dfsph only.
 * Off by default.  While it is on, every solver step starts by applying dfsph's rule (dfsph_solver.py:104-119) on the device to the velocities the
 * step starts with: dt = clamp(0.4 * particle_diameter / (max |v| + the body's term) * 0.2, min_dt, max_dt), written to delta_time, delta_time_2
 * and ps.delta_time; every sweep of the step uses it, the clock advances by it, pcisph's delta follows it (SPH_S_PCISPH_DELTA), sph_rigid_step takes it
 * like on a dfsph handle, SPH_S_DELTA_TIME / SPH_S_PS_DELTA_TIME / SphStepStats.dt report it, and a written SPH_S_DELTA_TIME lasts until the next
 * step.  No host wait is added to a step.  Switching it off leaves delta_time (and pcisph's delta) where the last step left them.  May be written
 * between steps.  SPH_E_STATE, handle unchanged: on a dfsph handle (which has 70-72) and on a slab handle. */
#define SPH_P_STEP_ADAPTIVE_DT 77                  /* 0 / 1 */
#define SPH_P_STEP_MAX_DT 78                       /* finite, > 0; default: the handle's delta_time as configured */
#define SPH_P_STEP_MIN_DT 79                       /* finite, > 0; default: 1e-5 (dfsph's) */

typedef struct SphHandle SphHandle;

/* replaces ParticleSystem(config) + <name>_solver(ps, config)   main.py:64-68.
 * Builds the fluid lattice and the wall particles (ParticleSystem.py:139-195), the static
 * wall cell list and wall volumes (:309-335), and allocates every device buffer. */
int sph_create(const SphConfig *cfg, SphHandle **out);
/* the same with a rigid body: replaces ParticleSystem(config) with a `solid` block + rigid_solver(ps, config)   main.py:69-71.
 * All four solvers couple to the body (wcsph_solver.py:118-127, dfsph_solver.py:204-212, pcisph_solver.py:200-211, iisph_solver.py:159-168).
 * On slab handles: a two-way coupled body (active, fs_couple 1) on dfsph with two ghost columns and on wcsph / pcisph / iisph with their one; the body
 * is replicated on every rank, three small all-reduces per step (the fluid positions and densities the reference's index quirks read, the per-sample
 * forces, each summed whole by the rank that owns the sample's cell column) keep every rank's copy bit-identical to the one-GPU run.  One sph_rigid_step
 * after every solver step: forces gathered over several solver steps are not supported there (column ownership changes between steps).  SPH_E_INVALID
 * on slab handles: dfsph with slab_ghost_layers = 1, a one-way body (active, fs_couple 0); on every handle: pbf (pbf_solver.py has no coupling). */
int sph_create_rigid(const SphConfig *cfg, const SphRigid *rigid, SphHandle **out);
/* replaces rigid_solver.step()   rigid_solver.py:216-232 */
int sph_rigid_step(SphHandle *h);
/* replaces `ps.active_rigid[None] = active`   ParticleSystem.py:63-64, main.py:102.  The flag and nothing else: from the next grid build an
 * active body is binned (and, with fs_couple, coupled), an inactive one is not -- its samples leave every neighbour walk and
 * get_neighbour_count's rigid-entry quirk -- and keeps its pose, velocity and omega.  Nothing is re-derived: pcisph's delta, dfsph's
 * warm_start_k and delta_time, rigid_particles.force stay as they are.  SPH_E_STATE (handle unchanged): no body; a slab handle; a one-way
 * body (active, fs_couple 0) under SPH_ARITH_RELAXED, as sph_create_rigid refuses it. */
int sph_rigid_set_active(SphHandle *h, int active);
/* replaces ps.init_rigid_particles_data()   ParticleSystem.py:249-291, main.py:106: sample volumes, masses, the centroid, the inertia tensor
 * and its inverse from the body's CURRENT sample positions, binned or not by the flag of this moment.  Velocity, omega, rigid_solver.mass
 * and its run_once_flag are left alone.  Host work, once per release.  A body created inactive has zero volumes (the reference's too); once it is
 * released, sph_step_* and sph_rigid_step return SPH_E_STATE until this call has run -- the reference would step on with NaN.
 * SPH_E_STATE: no body; a slab handle. */
int sph_rigid_init_data(SphHandle *h);

/* What sph_rigid_step does with the body (the reference has the first mode only).  The mode governs sph_rigid_step and nothing else: binning,
 * coupling, fs_couple, sph_rigid_set_active / sph_rigid_init_data, pcisph's delta and the fluid sweeps are as before -- the sweeps go on reading the
 * body's motion (vel + acc dt, omega + alpha dt, the centroid) and summing the fluid's force on every sample.  In every mode a step counts
 * (simulate_cnt), takes dt as before (dfsph: ps.delta_time), forms the f64 sums of the samples' forces and torques and zeroes the forces. */
#define SPH_RIGID_DYNAMIC 0   /* rigid_solver.step: the body is moved by the forces, the wall test and the wall impulse (the default) */
#define SPH_RIGID_SCRIPTED 1  /* the body is moved by the motion of sph_rigid_set_motion: omega = the given omega, attitude = omega dt, the samples, the
                               * vertices and the inverse inertia are rotated about the centroid as rigid_solver.rotation does (always, also by
                               * zero angles), then acc, vel = the given ones, and samples, vertices and centroid += vel dt.  No wall test, no impulse:
                               * a step whose sphere (centroid + vel dt, the largest sample distance from the centroid when the body's data were last
                               * derived, plus 0.1 %) does not lie inside the cell grid returns SPH_E_INVALID before anything is launched or changed
                               * (a conservative bound).  No read-back (dfsph: the one of ps.delta_time) */
#define SPH_RIGID_FIXED 2     /* the body never moves: positions, vertices, centroid and inverse inertia stay bit for bit; vel, acc, omega, alpha = 0 */
/* between steps; the body goes on from its current vel and omega when the mode returns to DYNAMIC.  SPH_E_STATE: no body; SPH_E_INVALID: an
 * unknown mode.  On slab handles every rank makes the same calls between the same steps (as with sph_set_scalar). */
int sph_rigid_set_mode(SphHandle *h, int mode);
/* the motion SPH_RIGID_SCRIPTED follows, kept until it is replaced; allowed in every mode.  acc / alpha may be NULL (zeros): they are what the
 * fluid sweeps extrapolate the body's velocity with during the NEXT solver step.  SPH_E_INVALID (handle unchanged): a value that is not finite,
 * vel or omega NULL; SPH_E_STATE: no body. */
int sph_rigid_set_motion(SphHandle *h, const float vel[3], const float omega[3], const float acc[3], const float alpha[3]);
/* the fluid's load on the body as the last sph_rigid_step summed it over the samples' forces, in f64: force, and torque about the centroid
 * before that step's move.  All three modes, identical on every rank of a slab run.  SPH_E_STATE: no body, or no sph_rigid_step yet. */
int sph_rigid_get_load(SphHandle *h, double force[3], double torque[3]);
/* Gravity as a vector, constant or harmonic: tilted tanks, tanks shaken along an axis (described in the tank's frame), zero g.  The handle's
 * acceleration vector a stands wherever the reference writes `gravity * (0, -1, 0)`: solver_base.py:131-133, dfsph_solver.py:91-96 (divided by
 * m later, as there), the ext-force lines of pcisph_solver.py / iisph_solver.py, pbf_solver.py:26-30, and rigid_solver.py:40-41 for a DYNAMIC
 * body (scripted and fixed bodies do not read it).  a_k = (float)((double)g_k + amp_k sin(omega_k t + phase_k)), evaluated in f64 on the device and
 * rounded once, t = SPH_S_TIME at the head of the solver step, held through the step and the sph_rigid_step behind it; an axis with amp_k == 0,
 * and every axis while no forcing is set, takes g_k as it is (no arithmetic).  The default g is the three floats the reference forms, so a handle
 * that never calls these, or calls sph_set_gravity with them, computes the same bits.  Stage calls and sph_rigid_step do not advance t;
 * sph_slab_set_state keeps t, g and the forcing.  A multi-step call stays asynchronous under forcing (one one-thread launch per step).
 * Both calls: between steps only; a value that is not finite gives SPH_E_INVALID and leaves the handle unchanged; the vector is evaluated at once
 * for the current t (SPH_S_ACCEL reads it back).  On slab handles every rank makes the same calls between the same steps (as with sph_set_scalar). */
int sph_set_gravity(SphHandle *h, const float g[3]);
/* amp == NULL switches the forcing off (omega and phase are ignored); omega or phase NULL: zeros */
int sph_set_forcing(SphHandle *h, const double amp[3], const double omega[3], const double phase[3]);
/* Inlets and sinks: fluid particles that arrive and leave between steps, on a single-GPU handle without a body.  Both calls
 * synchronise the handle's stream first.  A call that changes the count leaves the handle as a fresh handle that holds the same particles would be
 * before its first step -- the lists, rho and every other per-particle result of the last step are no longer valid for sph_download until a stage
 * or a step computes them again -- but for what travels: delta_time, SPH_S_TIME, gravity and forcing, the step counter, warm_start_k and iisph's last
 * pressure of the particles that stay, and pcisph's delta, a constant of construction.  Refusals leave the handle unchanged: SPH_E_STATE on a slab
 * handle or a handle with a body.
 * sph_add_particles appends n particles with the original ids n_fluid .. n_fluid + n - 1 (*first_id = n_fluid, may be NULL): everything indexed by
 * original id grows at the end, existing ids never change.  pos = 3 n floats, vel = 3 n floats or NULL (at rest).  A new particle has the state of a
 * particle at creation: warm_start_k = 0, iisph's last pressure 0, rho / pbf_lambda / delta_pos 0 until a step writes them.  No overlap test is made
 * against the fluid already there.  n == 0 is a no-op.  SPH_E_INVALID: a coordinate or velocity that is not finite, a position not strictly inside
 * box_min .. box_max, n_fluid + n > SPH_S_FLUID_CAPACITY (a handle created with fluid_capacity 0 refuses every add).
 * sph_remove_in_box removes every particle with lo[k] <= x[k] < hi[k] on all three axes (f32 compares); *removed = their number (may be NULL).
 * Survivors keep the order of their ids and are renumbered densely: new id = old id - the number of removed ids below it, so a download afterwards
 * is the old download with the removed rows squeezed out.  On the device, deterministic; the count comes back in one blocking read.  Nothing
 * removed: nothing changes, not even what is valid.  SPH_E_INVALID: a box that would remove every particle (an empty handle is not supported). */
int sph_add_particles(SphHandle *h, const float *pos, const float *vel, size_t n, int32_t *first_id);
int sph_remove_in_box(SphHandle *h, const float lo[3], const float hi[3], int32_t *removed);

/* Static geometry: obstacles, ramps, gates and meshes as wall samples, between steps, on a handle with Akinci walls
 * (boundary_handle 1) of any solver, either arithmetic, one GPU or slabs.  The wall set of a handle is the box samples (group 0, indices
 * 0 .. Nb0-1, as sph_create made them) and behind them every live group in order of addition; group ids are 1, 2, ... and never reused;
 * removing a group closes the gap (later groups move down and keep their ids).  After every edit the volumes of ALL samples, the box's included,
 * are recomputed by the rule of ParticleSystem.py:309-320 over the whole set, coincident samples each adding W(0); SPH_F_WALL_POS, SPH_F_WALL_VOL
 * and SphSizes.n_wall report the current set.  The samples stay at rest; no sweep is added or changed: every solver walks them as it walks the box.
 * An edit touches nothing else on the handle (fluid state, clock, delta_time, dfsph's warm start, pcisph's delta, gravity, the carried scalar, a
 * recording, the body) and invalidates what the last list build derived from the old set: a handle edited at step k continues exactly as a handle
 * that had that wall set all along and was given the same fluid state at step k.  On slab handles the walls are replicated: every rank makes the
 * same calls between the same steps (plain local calls, as sph_rigid_set_mode).  The rigid body's own wall test (sph_rigid_step) sees the box only.
 * Refusals come before any launch or upload and leave the handle unchanged.  SPH_E_INVALID: xyz == NULL, n == 0, a coordinate that is not finite, a
 * sample whose cell lies outside the grid, an unknown group, a clearance outside (0, h], an edit after which some sample has no other sample within h
 * (its volume would be infinite), a handle with clamp walls, 2^28 wall samples or more, a carve that would remove every particle.
 * SPH_E_STATE: sph_geometry_carve on a slab handle or a handle with a body (as sph_remove_in_box).
 * A step whose wall lists overflow returns SPH_E_OVERFLOW as ever (SphConfig.max_wall_neighbors). */
/* appends n samples (x, y, z in world coordinates) as a new group; *group = its id (may be NULL) */
int sph_geometry_add(SphHandle *h, const float *xyz, size_t n, int32_t *group);
int sph_geometry_remove(SphHandle *h, int32_t group);
/* the live groups in order with their ranges [first, first + count) in the wall arrays: up to cap entries are written, *n_groups = how many there are */
int sph_geometry_info(SphHandle *h, int32_t *groups, int32_t *first, int32_t *count, size_t cap, size_t *n_groups);
/* removes every fluid particle i with |x_i - x_b| < clearance for some sample b of `group` (-1: of any added group; the box never carves), f32,
 * (dx dx + dy dy) + dz dz under a correctly rounded root; 0 < clearance <= h.  Survivors are compacted exactly as by sph_remove_in_box (id order
 * kept, the carried scalar with them); *removed = how many went (may be NULL); nobody near: nothing changes, not even what is valid */
int sph_geometry_carve(SphHandle *h, int32_t group, float clearance, int32_t *removed);
/* how many wall samples, box and geometry, each particle's list holds as the last list build (a step, sph_build_neighbors) left it, in original
 * particle order; n must be the live particle count.  Who touches a wall.  On a handle whose lists carry a skin (relaxed wcsph) the entries within
 * h + skin.  SPH_E_INVALID: counts == NULL, n != n_fluid; SPH_E_STATE: a slab handle. */
int sph_geometry_wall_counts(SphHandle *h, int32_t *counts, size_t n);
/* Loads on walls and geometry: how hard the fluid presses on selected wall groups, measured on the device while the steps
 * run.  Group 0 is the box, ids >= 1 are the groups of sph_geometry_add.  During a step every sample b of a selected group collects f_b, the
 * reaction to the pressure term the fluid feels from it, pair by pair the expression the reference deposits on a rigid body's samples with V_b in
 * place of the sample's volume (no viscous term: the reference's walls exert none), summed in f32 over the fluid particles that list b, in the
 * sample's own cell-walk order: wcsph once per step from the step's pressures; dfsph once per executed iteration of the density loop (the
 * divergence loop's impulses are not counted, as the reference does not count them for a body); iisph and pcisph once, behind the pressure loop, from
 * the final pressures -- the pressures behind the pressure force the integration applies, so that sum_b f_b = - m sum_i (the wall acceleration of
 * particle i).  At the end of every step each selected group's force F = sum_b f_b and torque sum_b x_b x f_b are summed on the device in f64 in a
 * fixed order (the arithmetic contract of SphDiagnostics: the same state gives the same bits) and added, times the dt the step used, to the group's
 * impulse; no host wait is added to a step, a multi-step call or a replayed graph.  Selecting, reading and resetting are invisible to the fluid:
 * the steps that follow are bit for bit those of a handle that never called them.
 * An edit of the wall set keeps the selection by id: a removed group leaves it, the impulses of the others go on, and the last step's forces read
 * zero until a step has run.  A sample with more than SphConfig.max_neighbors fluid neighbours makes the step return SPH_E_OVERFLOW.
 * Refusals leave the handle unchanged.  SPH_E_STATE: a slab handle, a handle under the relaxed arithmetic, pbf, a read before any selection.
 * SPH_E_INVALID: a handle with clamp walls, an unknown, unselected or twice-named group, more than 1024 groups, a null pointer, a wrong size. */
/* measure the n groups named (any order; it is the order of "all selected" sums); n == 0 switches measuring off.  Impulses and seconds start at 0 */
int sph_wall_load_select(SphHandle *h, const int32_t *groups, size_t n);
/* the last step's force on `group` (-1: on all selected) and its torque sum_b (x_b - about) x f_b; about == NULL: the origin */
int sph_wall_load_get(SphHandle *h, int32_t group, const double about[3], double force[3], double torque[3]);
/* sum over the steps since the selection (or the last reset) of dt F and dt torque, and of dt: the mean force over the window is impulse / seconds.
 * The samples do not move, so the angular impulse about `about` is taken from the one about the origin: L_0 - about x impulse.  reset != 0: the
 * group's (-1: every selected group's) sums start at zero again behind this read.  group == -1 is one window of all selected groups: SPH_E_STATE
 * if their seconds differ, as they do after a reset of a single group (read the groups one by one and reset each, or select again) */
int sph_wall_load_impulse(SphHandle *h, int32_t group, const double about[3], double impulse[3], double angular[3], double *seconds, int reset);
/* the last step's f_b of every sample of `group`, 3 floats each, in the group's own sample order (the box: the order of SPH_F_WALL_POS);
 * n_floats must be 3 * the group's sample count */
int sph_wall_load_forces(SphHandle *h, int32_t group, float *xyz, size_t n_floats);
/* Run diagnostics of the FLUID of a single-GPU handle, summed on the device: every solver, exact or relaxed, with or without
 * a body (the body's own momentum and energy are not in the row).  One row is 32 doubles.  m = SPH_S_PARTICLE_M, x / v = SPH_F_POS / SPH_F_VEL.
 * Arithmetic: every f32 operand is widened to f64 first, products and the three-term sums inside a term are f64, the terms are summed in f64 in a
 * fixed order (no atomics; the same state in the same device order gives the same bits, another order after a re-sort may differ in the last
 * bits), and the scalings by m, 1/2, 1/n are applied once, at the end.  n, step, vmax, vmax_id, pos_min / pos_max, rho_min / rho_max are exact. */
typedef struct SphDiagnostics {
    double time;                  /* SPH_S_TIME */
    double dt;                    /* the delta_time the last step used (SPH_S_DELTA_TIME) */
    double step;                  /* SPH_S_SIMULATE_CNT */
    double n;                     /* the live particle count */
    double mass;                  /* n m */
    double momentum[3];           /* m sum v */
    double angular_momentum[3];   /* m sum x cross v, about the origin */
    double kinetic;               /* 1/2 m sum |v|^2 */
    double potential;             /* -m sum a . x, a = the handle's acceleration vector of the moment (SPH_S_ACCEL) */
    double com[3];                /* sum x / n */
    double vmax;                  /* the largest speed, the f32 value sqrtf((vx vx + vy vy) + vz vz) the adaptive time step forms */
    double vmax_id;               /* original id of the particle that has it (the lowest id among ties) */
    double pos_min[3];            /* the fluid's extent: per-axis minimum ... */
    double pos_max[3];            /* ... and maximum position (f32 values) */
    double rho_min;               /* f32 values ... */
    double rho_max;
    double rho_mean;              /* sum rho / n */
    double reserved[5];           /* 0 */
} SphDiagnostics;
/* On demand, between steps: synchronises, two launches, one blocking read.  Changes nothing on the handle: the steps that follow are bit for bit
 * those of a handle that never called it.  rho_min / rho_max / rho_mean are NaN unless the densities describe the current positions (after
 * sph_compute_density).  SPH_E_INVALID: out == NULL; SPH_E_STATE: a slab handle (the sums would need an all-reduce). */
int sph_diagnostics(SphHandle *h, SphDiagnostics *out);
/* Recorded: every >= 1 (re)starts recording into a ring of `rows` rows in device memory, every == 0 stops it (rows is ignored; the ring stays
 * readable).  While it is on, every solver step -- of all five sph_step_* calls, the steps inside a multi-step call and the replayed wcsph step
 * pairs included -- ends with the two launches; step k since the call is recorded when k is a multiple of `every` (decided on the device: no host
 * wait is added, a step that is not due costs two empty launches) into ring slot (rows recorded so far) % rows.  The row describes the state the
 * step leaves: the new positions and velocities, the advanced clock, the dt it used, and the densities its density sweep computed (pbf: its
 * lambda sweep).  Recording changes no trajectory.  sph_add_particles / sph_remove_in_box need nothing: the next row counts the new n.
 * SPH_E_INVALID (handle unchanged): every < 0; every >= 1 with rows < 1 or rows > 2^20.  SPH_E_STATE: a slab handle. */
int sph_diag_record(SphHandle *h, int every, int rows);
/* Synchronises and copies out the rows still in the ring, oldest first, at most max_rows; *n_rows = their number, *total (may be NULL) = rows
 * recorded since recording was switched on, so the caller sees how many were overwritten before they were read.  The read consumes the rows: the
 * next one returns what was recorded since.  A handle that never recorded returns no rows.  SPH_E_INVALID: n_rows == NULL, out == NULL with
 * max_rows > 0; SPH_E_STATE: a slab handle. */
int sph_diag_read(SphHandle *h, SphDiagnostics *out, size_t max_rows, size_t *n_rows, int64_t *total);

/* Derived per-particle fields of the fluid: the plain SPH estimates, without kernel-gradient correction, at the positions
 * and velocities the handle holds now, any of the five solvers, summed in f32 in the order of each particle's neighbour list with the exact kernel
 * functions (on relaxed handles too).  With vol_j = m / rho_j (rho: SPH_F_RHO as sph_compute_density leaves it), W and grad W over fluid
 * neighbours j, the samples r of a COUPLED body and wall samples b, no self term:
 *   velgrad[a][b] = sum_j vol_j (v_j,a - v_i,a) dW/dx_b        estimates d v_a / d x_b; 9 floats per particle, row a, column b
 *   vorticity     = (G_zy - G_yz, G_xz - G_zx, G_yx - G_xy)     3
 *   divergence    = (G_xx + G_yy) + G_zz                        1
 *   normal        = -h (sum_j vol_j grad W + sum_r V_r grad W + sum_b V_b grad W)     3; dimensionless, points out of the fluid: about 0 inside,
 *                                                               O(1) at a free surface
 *   cover         = sum_j vol_j W + sum_r V_r W + sum_b V_b W   1; about 1 inside the fluid, falls towards a free surface
 * A particle without neighbours gets zeros.  A free-surface flag is the caller's threshold on |normal| and cover.  A body's samples do not enter
 * velgrad.  grad W is the solvers' own (solver_base.py:90-103, with the factor 6 the reference carries), so velgrad, vorticity, divergence and
 * normal are six times the textbook estimates; cover is not affected. */
#define SPH_D_VELGRAD 0
#define SPH_D_VORTICITY 1
#define SPH_D_DIVERGENCE 2
#define SPH_D_NORMAL 3
#define SPH_D_COVER 4
/* `host` receives the quantity in API (original particle) order; n_floats must be its width times the live particle count.  The call runs
 * sph_compute_density first (which builds the lists if positions changed), so sph_compute_density's caveat holds here too: the re-sort leaves the
 * OTHER per-particle results of the last step (alpha, pressure, acc, press_iter, ...) not downloadable until they are computed again.  Like the
 * stage calls it changes no trajectory: called between steps any number of times, the steps that follow are bit for bit those of a handle that
 * never called it.  One sweep computes all five quantities; they are kept until a step, a sph_upload, sph_add_particles / sph_remove_in_box, a
 * re-sort or a change of the body's state or activity, so a second call on an unchanged state only copies.  The feature's device memory (30 floats
 * per particle of the capacity) is taken at the first call.  Refusals leave the handle unchanged -- SPH_E_STATE: a slab handle; SPH_E_INVALID:
 * host == NULL, an unknown `which`, a wrong n_floats. */
int sph_derived(SphHandle *h, int which, float *host, size_t n_floats);

/* One carried scalar per single-GPU handle: a temperature or a dye concentration T that rides with the particles, diffuses
 * between fluid neighbours and, with beta != 0, lifts the fluid.  Off by default; a handle that never enables it launches what it always launched.
 * Any of the five solvers, exact or relaxed arithmetic, with or without a body, with or without fluid_capacity.  T is kept by particle id (API
 * order) in memory of the feature's own, 24 B per particle of the capacity, taken at enable and freed at disable.
 * Per solver step, while enabled:
 *   behind the sort and the list build, at the positions x^n the step starts from:
 *     rate_i = kq sum_j (T_i - T_j) f_ij,   f_ij = (g(q) r) / (r^2 + eta2),   q = r / h,   g = q <= 1/2 ? 3 q^2 - 2 q : -(1 - q)^2
 *     over the FLUID entries j of i's list with r <= h, in list order, f32, unfused; eta2 = 0.01 h^2, kq = 12 D (m / rho0) kw / h, both formed in
 *     f64 and rounded once.  This is Brookshaw's Laplacian 2 D sum V0 (T_i - T_j) W'(r) r / (r^2 + eta2) with the constant particle volume
 *     V0 = m / rho0 and the TRUE W'(r) = 6 kw g / h (not the reference's gradient, which carries a further factor 6): D is a diffusivity in m^2/s.
 *     Walls and a body's samples are insulated (they add nothing).  No density is read; the pair term is antisymmetric bit for bit.
 *   behind the solver's integrator, with the dt the step used and a = the step's acceleration vector (SPH_S_ACCEL):
 *     beta != 0:  vel_i += (dt s) a,  s = -(beta (T_i - t_ref))  from T^n (a Boussinesq kick, first-order splitting: the next step's CFL rule and
 *     pressure solve see it); beta == 0: the velocities are not touched.  Then T_i += dt rate_i.
 * The scheme is explicit: the caller keeps dt sum_j c_ij <= 1, c_ij = -kq f_ij >= 0 (undisturbed lattice of spacing 2 r, h = 4 r: dt <= 0.0585 h^2 / D
 * -- DESIGN.md section 6k).  Nothing enforces it.
 * Between steps: sph_add_particles gives every new particle the inflow value; sph_remove_in_box keeps the survivors' values under their new ids;
 * sph_upload and sph_slab_set_state do not touch T; the stage calls, sph_derived and sph_diagnostics neither read nor advance it.
 * Refusals come before any launch and leave the handle unchanged -- SPH_E_STATE: a slab handle; download / upload / rate / set_inflow before
 * enable.  SPH_E_INVALID: a null pointer, n != the live particle count, a diffusivity that is negative or not finite, a beta, t_ref or value that
 * is not finite (upload: any of the n values). */
/* allocates, sets T = t_ref everywhere and the inflow value to t_ref.  On an enabled handle: changes the three parameters, keeps T and the inflow value */
int sph_scalar_enable(SphHandle *h, double diffusivity, double beta, double t_ref);
/* frees; the handle steps as if it had never been enabled.  Not enabled: nothing happens */
int sph_scalar_disable(SphHandle *h);
/* T in API (original particle) order; n must be the live particle count */
int sph_scalar_upload(SphHandle *h, const float *values, size_t n);
int sph_scalar_download(SphHandle *h, float *values, size_t n);
/* the value sph_add_particles gives to new particles from now on */
int sph_scalar_set_inflow(SphHandle *h, double value);
/* rate_i of the CURRENT state in API order.  Builds the lists first if positions changed since the last build (what sph_build_neighbors does; its
 * caveat applies); changes neither T nor any trajectory.  Profile id "scalar". */
int sph_scalar_rate(SphHandle *h, float *out, size_t n);
void sph_destroy(SphHandle *h);
int sph_get_sizes(SphHandle *h, SphSizes *out);
const char *sph_last_error(SphHandle *h);

/* replaces field.from_numpy / field.to_numpy on ps.fluid_particles.* and solver.*   main.py:159,190.
 * n_floats must equal the field's float count. */
int sph_upload(SphHandle *h, int species, int field, const float *host, size_t n_floats);
int sph_download(SphHandle *h, int species, int field, float *host, size_t n_floats);

/* replaces wcsph_solver.step() x nsteps   wcsph_solver.py:25-30 (asynchronous; sph_download /
 * sph_synchronize wait for it) */
int sph_step_wcsph(SphHandle *h, int nsteps);
/* replaces dfsph_solver.step() x nsteps   dfsph_solver.py:440-445; `last` (may be NULL) gets the
 * last step's statistics */
int sph_step_dfsph(SphHandle *h, int nsteps, SphStepStats *last);
/* replaces pcisph_solver.step() x nsteps  pcisph_solver.py:252-259.  last->n_dens = iter_cnt and last->dens_err = rho_err_avg as
 * printed at :71; last->capped = 1 when max_iteration (80) ended the loop */
int sph_step_pcisph(SphHandle *h, int nsteps, SphStepStats *last);
/* replaces iisph_solver.step() x nsteps   iisph_solver.py:340-347.  last->n_dens = l and last->dens_err = residual as printed at :102;
 * last->n_div = 1 when the loop left on "Iteration trend to divergence" (:97-99); last->capped = 1 at max_iter_cnt (180) */
int sph_step_iisph(SphHandle *h, int nsteps, SphStepStats *last);
/* replaces pbf_solver.step() x nsteps     pbf_solver.py:176-187 (update_all_pos under the barrier-synchronised schedule, csrc/sph_pbf_kernels.h).
 * On slab handles (one ghost column, any transport; in order on the handle's stream -- slab_overlap is ignored; exact or relaxed): per step the
 * particle exchange, then lambda of the ghosts after the lambda sweep (4 bytes per ghost), then their new position and phase-1 velocity in one
 * message after the delta_pos sweep (24 bytes per ghost) -- three point-to-point groups, no all-reduce.  The overflow verdict is taken once per
 * call by all ranks together (one host all-reduce): every rank returns SPH_E_OVERFLOW if any rank's lists overflowed.  Bit for bit the one-GPU
 * handle's pos, vel, rho, pbf_lambda and delta_pos. */
int sph_step_pbf(SphHandle *h, int nsteps);
/* stages of the step, for parity tests against the oracle's stages:
 * ps.reset_grid()+update_grid() (+ neighbour-list build), solver.compute_all_rho(), dfsph compute_all_alpha().
 * None of them changes a trajectory: called between two steps, any number of times and in any order, they leave positions, velocities, warm_start_k,
 * delta_time, pbf_lambda / delta_pos and a body's state as they were, and the steps that follow are bit for bit those of a handle that never
 * called them (tests/test_midrun_calls_gpu.py).  What they do change: sph_build_neighbors re-sorts the device arrays by cell, so the OTHER
 * per-particle results of the last step (rho, alpha, pressure, acc, rho_adv, rho_derivative, vel_adv, press_iter, press_force, pos_predict, d_ii,
 * a_ii, d_ij) are no longer valid for sph_download until they are computed again -- rho (dfsph: and alpha, wcsph: and pressure, which the fused
 * sweep writes with it) by sph_compute_density / sph_compute_alpha, the rest by the next step; SPH_F_NBR_COUNT becomes that of the current
 * positions.  sph_compute_density and sph_compute_alpha build the lists first if positions changed since the last build.
 * Slab handles: the three are collective (the re-sort starts with a particle exchange, and all ranks agree on one overflow verdict).  A pbf slab
 * handle does NOT carry pbf_lambda / delta_pos through the re-sort: there they are valid from a step until the next sort (sph_download_local). */
int sph_build_neighbors(SphHandle *h);
int sph_compute_density(SphHandle *h);
int sph_compute_alpha(SphHandle *h);

int sph_get_scalar(SphHandle *h, int which, double *out);
/* `solver.delta_time[None] = value` (the reference's 0-d field is writable, main.py:111; dfsph re-derives it every step from the CFL
 * rule, dfsph_solver.py:112-119, so a written value lasts one step there, as on a handle of another solver while SPH_P_STEP_ADAPTIVE_DT is on):
 * which = SPH_S_DELTA_TIME; with it a device state
 * (pos, vel, warm_start_k, delta_time) can be moved into another handle, or into the oracle, completely.
 * `solver.<attribute> = value`: which = SPH_P_* (above). */
int sph_set_scalar(SphHandle *h, int which, double value);
int sph_synchronize(SphHandle *h);
/* Development overrides in force on this handle: "NAME=value;NAME=value" (empty string: none).  The SPH_* environment knobs of the
 * library (layout / arithmetic switches used by tests and tools for A/B runs) are read only when SPH_DEV=1 is set; every one that took
 * effect is listed here, so a measurement can name the switches it ran under -- bench.py refuses to print a line otherwise. */
const char *sph_overrides(SphHandle *h);

/* Per-kernel timing with HIP events on the handle's stream (bench.py's roofline leg).
 * Enabling it records an event pair around every launch; totals are read back per kernel id. */
int sph_profile_enable(SphHandle *h, int on);
int sph_profile_reset(SphHandle *h);
int sph_profile_kernel_count(void);
const char *sph_profile_kernel_name(int kernel_id);
int sph_profile_get(SphHandle *h, int kernel_id, double *total_ms, int64_t *launches);

/* ---- multi-GPU: x-slab decomposition (new capability, the reference is single-device) ----
 * One process per GPU.  A handle created with slab_count > 1 owns the particles whose cell x-index lies in its slab
 * [x_lo, x_hi) plus one ghost cell layer on each side.  Every step it (1) migrates particles that left the slab,
 * (2) re-sends its two edge layers as ghosts, and after every sweep whose output the neighbours read (3) refreshes that
 * field on the ghosts; residual sums and the CFL maximum are all-reduced.  The library packs / unpacks on the device and
 * calls back into the host for the transport, so the same code runs over RCCL (device buffers) or any host transport.
 *
 * Buffers: four byte buffers of `capacity` bytes each, owned by the caller (e.g. torch tensors): send/recv x left/right.
 * With on_host = 0 they are device pointers (RCCL over xGMI reads/writes them directly); with on_host = 1 they are host
 * pointers and the library stages through them with hipMemcpy (used by the gloo tests).
 * Callbacks return 0 on success and are invoked on the calling thread.
 *
 * Two transport disciplines:
 *   - synchronous (stream_ordered = 0): the library synchronises its stream before exchange_buffers (the packed data is complete) and
 *     the callback returns when the receive buffers are filled.  Host transports (on_host = 1) are always of this kind.
 *   - stream-ordered (stream_ordered = 1, device buffers): the callbacks ENQUEUE the transfer on the handle's own stream
 *     (sph_get_stream) -- e.g. RCCL send/recv issued with that stream current -- and return at once; the library never blocks the
 *     host around them, so a whole chunk of solver iterations, halo refreshes and residual all-reduces is in flight at a time.
 * With allreduce_stream set, DFSPH runs its loops with the device-side control of the single-GPU path: the (sum, count) pair of a
 * residual is written to reduce_buf, all-reduced in place by allreduce_stream, and a second kernel takes the reference's loop
 * decision from it -- identical on every slab because all ranks see the same reduced values. */
typedef struct SphComm {
    void *user;
    /* send my counts to the left / right neighbour and receive theirs (absent neighbour: recv 0) */
    int (*exchange_counts)(void *user, int32_t send_left, int32_t send_right, int32_t *recv_left, int32_t *recv_right);
    /* send the first send_*_bytes of the send buffers, receive exactly recv_*_bytes into the recv buffers */
    int (*exchange_buffers)(void *user, size_t send_left_bytes, size_t send_right_bytes, size_t recv_left_bytes, size_t recv_right_bytes);
    /* in-place all-reduce of n doubles over all slabs; op 0 = sum, 1 = max */
    int (*allreduce)(void *user, double *values, int32_t n, int32_t op);
    void *send_left, *send_right, *recv_left, *recv_right;
    size_t capacity;
    int32_t on_host;
    int32_t stream_ordered;     /* 1: exchange_buffers / allreduce_stream enqueue on the handle's stream and return (device buffers only) */
    /* optional: in-place all-reduce of the first n doubles of reduce_buf (op 0 = sum, 1 = max), ordered like exchange_buffers */
    int (*allreduce_stream)(void *user, int32_t n, int32_t op);
    double *reduce_buf;         /* >= 4 doubles: device memory with on_host = 0, host memory (the library stages) with on_host = 1 */
    /* optional: exchange_counts with n (<= 8) ints per neighbour in one round trip -- the particle exchange of a step sends
     * (records, ghosts per column, migrants the sender keeps as ghosts per column) in ONE message; NULL: the library calls exchange_counts n times */
    int (*exchange_counts_n)(void *user, int32_t n, const int32_t *send_left, const int32_t *send_right, int32_t *recv_left, int32_t *recv_right);
    size_t reduce_capacity;     /* doubles reduce_buf holds; 0 = 4.  A slab handle with a rigid body sums arrays of 4 x (rigid sample count) doubles through it */
} SphComm;

int sph_set_comm(SphHandle *h, const SphComm *comm);
/* the same for a caller built against an older, SHORTER SphComm: comm_size = that caller's sizeof(SphComm); the fields it does not have read as 0 / NULL */
int sph_set_comm_sized(SphHandle *h, const SphComm *comm, size_t comm_size);
/* Native transport: instead of callbacks, the library itself issues ncclSend / ncclRecv to the left and right slab neighbour and
 * ncclAllReduce of the residual pair on its own stream (librccl is dlopen'ed).  Rank 0 obtains a 128-byte id with
 * sph_rccl_unique_id and the application broadcasts it by any means; every rank then calls sph_rccl_attach (collective:
 * ncclCommInitRank with rank = slab_rank, world = slab_count) instead of sph_set_comm.  sph_rccl_selftest all-reduces n doubles and
 * runs an empty neighbour exchange (a single-GPU handle attaches as a communicator of one rank for it). */
int sph_rccl_unique_id(void *id128);
int sph_rccl_attach(SphHandle *h, const void *id128, size_t capacity_bytes);
int sph_rccl_selftest(SphHandle *h, double *inout, int32_t n, int32_t op);
/* the handle's HIP stream (a hipStream_t), for stream-ordered transports */
int sph_get_stream(SphHandle *h, void **stream);
/* host-only planning (no device needed): cuts[0..slab_count] = cell-column boundaries of the slabs of the scene's initial lattice,
 * counts[k] = particles slab k owns at t = 0.  The cuts balance what a slab costs: its particles plus the ghosts of each cut it has
 * (the particles of the solver's ghost columns beyond the cut) -- the largest such load is minimised */
int sph_plan_slabs(const SphConfig *cfg, int32_t *cuts, int32_t *counts);
/* host-only: the re-balancing rule.  new_cuts = cuts of `column_histogram` (grid_x counts) that minimise the largest load (particles + the
 * particles of `ghost_layers` columns beyond each cut; ghost_layers = 0: plain equal counts), every slab >= 3 columns wide and
 * old_cuts[k-1] < new_cuts[k] < old_cuts[k+1] (a particle's new owner is its rank or a direct neighbour) */
int sph_replan_slabs(const int64_t *column_histogram, int32_t grid_x, int32_t slab_count, const int32_t *old_cuts, int32_t ghost_layers, int32_t *new_cuts);
/* between steps, on every slab alike: 1 = the dfsph solver loops run their halo and reductions on their own streams (the default where the
 * handle and its transport can), 0 = in order on the handle's stream.  Results are the same bits; which is faster depends on the link */
int sph_slab_set_overlap(SphHandle *h, int32_t on);
/* slab bookkeeping: out[0] = owned particles, out[1] = ghosts, out[2] = x_lo, out[3] = x_hi (cell units), out[4] = capacity,
 * out[5] = number of re-balancings that moved a cut, out[6] = slab_rebalance_every, out[7] = the halo protocol in force: ghost columns per side (1 or 2)
 * | 16 if the dfsph residual sweeps run their edge tiles first with the halo on its own stream | 32 if the residual's all-reduce and loop decision run
 * on a third stream under the next correction sweep (both need the native transport or a synchronous one) */
int sph_slab_info(SphHandle *h, int32_t *out8);
/* What the halo transport was asked to do since the last reset (whichever transport drives it: native RCCL, callbacks over RCCL or gloo):
 * out[0] point-to-point groups (a send / recv pair with each slab neighbour), out[1] bytes sent, out[2] bytes received, out[3] count
 * exchanges (one host round trip each), out[4] all-reduces ordered on the handle's stream, out[5] all-reduces through the host,
 * out[6] steps, out[7] 0.  bench.py reports them per step in config.rank0_comm so that a measured N > 1 line can be read against the
 * cost model of DESIGN.md section 6. */
int sph_comm_stats(SphHandle *h, int64_t *out8, int reset);
/* local (device-order) access for slab handles: all resident particles, owned and ghost; ids < 0 mark ghosts (~id).  pbf handles also give
 * SPH_F_PBF_LAMBDA, SPH_F_PBF_DELTA_POS and SPH_F_POS_PREDICT (= pos after a step): SPH_E_STATE before the first step, as from sph_download, and on
 * a slab handle from the next sort (sph_build_neighbors, sph_compute_density) or sph_slab_set_state until the step after it.  The ghosts' entries
 * of rho and delta_pos are not the owners' values (a ghost has no lists); their lambda, pos and vel are. */
int sph_download_local(SphHandle *h, int field, float *host, size_t n_floats);
int sph_download_ids(SphHandle *h, int32_t *host, size_t n);
/* Start (or continue) a sharded run from any state: replaces everything resident on a slab handle -- owned particles, ghosts, dead slots -- by
 * its share of one FULL state.  Collective: every rank of the slab group calls it with the same arrays in ORIGINAL particle order: pos = 3 n_fluid
 * floats, vel = 3 n_fluid floats or NULL (zeros), scalar = the per-particle scalar that travels with a particle on this solver (dfsph warm_start_k;
 * n_fluid floats) or NULL (zeros; it must be NULL where the solver carries none: wcsph, pcisph, pbf); delta_time > 0 is written as sph_set_scalar(SPH_S_DELTA_TIME) writes
 * it, 0 keeps the handle's.  The cuts are planned anew from the positions by the rule of sph_create (from a per-column histogram counted on the
 * device, the same on every rank); afterwards the handle is a newly created slab handle that holds this state -- the step counter and the
 * re-balancing counter keep their values, and the next step exchanges particles in two rounds, as after any change of the cuts.
 * Refusals leave every rank's handle as it was, and every rank returns the same code (one max-reduce of the ranks' verdicts through the
 * handle's transport, which therefore must be attached): SPH_E_STATE not a slab handle, or one with a rigid body; SPH_E_INVALID n_fluid is not the
 * scene's particle count, a position that is not finite or lies in no cell of the grid, a scalar where none travels; SPH_E_OVERFLOW a rank would
 * own more than its capacity (slab_capacity).  (sph_upload of a single field stays refused on slab handles.) */
int sph_slab_set_state(SphHandle *h, const float *pos, const float *vel, const float *scalar, size_t n_fluid, double delta_time);

/* device arithmetic self-test: out[i] = op(a[i], b[i]) evaluated on the GPU with the same
 * compiler flags as the sweeps (op 0: a/b, 1: sqrt(a), 2: cubic_kernel(a, h=b), 3..5:
 * component op-3 of cubic_kernel_derivative((a, b, 0.25*a), h=0.1), 6: the sweeps' own root sqrt_rn(a)).
 * Used by tests to prove the device's f32 divide/sqrt are correctly rounded like the oracle's.
 * The shared-denominator division of the sweeps (csrc/sph_device.h), piece by piece: 7: recip_prepare(b).y, the refined
 * reciprocal; 8: div_shared(a, recip_prepare(b)), the quotient the sweeps form; 9: div_shared_two_step(a, recip_prepare(b)),
 * the same with a second residual correction; 10: op 8 with the divisor raised to the sweeps' floor (kDenFloor) first. */
/* tuning aid: mean microseconds of `reps` launches of one dfsph sweep (0 divergence residual, 1 divergence correction, 2 density
 * residual, 3 sort + list build) with `lds_bytes` of dynamic LDS per block; see tools/tune_sweeps.py.
 * What it changes on the handle: all of them first bring the lists and rho / alpha up to date, as sph_compute_alpha does.  0, 2 and 3 then write
 * only what the next step recomputes before reading it (rho_derivative, rho_adv, the sorted order and the lists): the steps that follow are, bit for
 * bit, those of a handle that was never timed (tests/test_midrun_calls_gpu.py draws them between steps).  1 applies the divergence correction `reps`
 * times: it ADVANCES the velocities and warm_start_k; 4 .. 7 (a residual with its reduction, the reduction alone, residual + correction without and
 * with the reduction) write the loop-control block and, 6 and 7, the velocities as well.  1 and 4 .. 7 are for throw-away handles.  Any other
 * value of `which` is not refused: it times sort + list build, as 3 does. */
int sph_tune_time(SphHandle *h, int which, unsigned lds_bytes, int reps, double *avg_us);
int sph_selftest_math(int device, int op, const float *a, const float *b, float *out, size_t n);
/* wave primitive self-test: out[i] = what lane i % 64 holds after one cross-lane primitive over the 64 values in[64*(i/64) ..]
 * (op 0: f64 sum, 1: i32 sum, 2: f32 max, 3: i32 max -- reductions, documented result in lane 0; 4: i32 inclusive prefix sum).
 * The primitives are DPP / ds_swizzle / v_permlane32_swap butterflies (csrc/sph_device.h); n must be a multiple of 256. */
int sph_selftest_wave(int device, int op, const double *in, double *out, size_t n);
/* staging self-test: the routine that copies a workgroup's operands into LDS (stage_operands, csrc/sph_kernels.h) run by ONE workgroup of 256
 * threads on the caller's plan.  h: the handle whose device runs it and whose sph_last_error receives a failure; NULL: device 0.
 * runs: nruns pairs (first source index, count), at most 640 runs and 2560 particles in all; not_staged: the
 * plan says "this workgroup is not staged"; use_pre: the plan's head arrives the way the density loop prefetches it.  A, B: n_src float4 each,
 * S: n_src floats, changed: n_src bytes.  layout: 0 one float4 (A), 1 the same with xyz * 2^32, 2 (A.xyz, S), 3 the same scaled,
 * 4 (A.xyz, B.x) + (B.y, B.z), 5 the same scaled, 6 A + S in a second array, 7 A + the kept source index (its bits in float 4).
 * check: 0 none, 1 with the copy, 2 first (the key examined: A.w for layouts 0, 1, 6, 7; S for 2, 3; changed for 4, 5).
 * out: 2560 x 6 floats, the staged elements in order (floats the layout does not hold are 0); *verdict: 0 not staged, 1 staged, 2 staged and
 * no key set (check 2: nothing copied then).  An empty staged set gives 1, or 2 with empty_idle (the sweeps choose per call site). */
int sph_selftest_stage(SphHandle *h, int layout, int check, int empty_idle, int use_pre, int not_staged, const uint32_t *runs, int nruns,
                       const float *A, const float *B, const float *S, const unsigned char *changed, size_t n_src, float *out, int *verdict);

/* Self-test of the list walks of the sweeps (optional export): 256 particles walk the lists the caller supplies through one walk and one operand
 * source.  walk: 0 the pipelined 32-bit walk over memory, 1 its four-lanes-per-particle form, 2 the staged 32-bit walk, 3 the staged 16-bit walk.
 * src, walks 0 / 1: 0 (A) without entry word, 1 (A), 2 (A, B), 3 (A, S), 4 (A, B, C); walks 2 / 3, staged from the run (run_first, run_n <= 512) of
 * the source arrays: the layouts 0-6 of sph_selftest_stage, 7 A staged + B gathered through the kept index, 8 A and C.xyz staged + B gathered.
 * lists: 256 x 28 entries (24 + the spare group, all of them valid: indices into the source arrays for walks 0 / 1, into the staged run for
 * 2 / 3; with rigid != 0 an entry may carry bit 31 and then indexes RP); counts: 256 values in 0 .. 24.  rigid needs walk != 3 and not src 0 of
 * the memory walks.  A, B, C: n_src float4, S: n_src floats, RP: n_rig float4.  out: 4 words per thread (walk 1: 1024 threads, four per
 * particle; else 256): body calls, the hash h = h * 0x9E3779B1 + word over every call's operand bits and rigid flag, and (walk 1) the bits of two
 * sums that start at 0.001 and 0 and take a.x and a.y of every call in list order. */
/* walk_list16 with the pair-bit stream on one workgroup of 256 threads (csrc/sph_selftest_walk.h): lists 256 x 24 entries < 256, counts 0 .. 24, words 256 x 3
 * (read when write == 0, returned when write != 0: what the walk stored), verdicts 256 x 24 (recorded by body k when write != 0); seen 256 x 24: per body call
 * in order entry | (field & 0xff) << 16, 0xffffffff where no call wrote; calls 256.  h may be NULL (device 0).  Fields: SPH_S_PAIR_BITS. */
int sph_selftest_walk_bits(SphHandle *h, int write, const uint32_t *lists, const int32_t *counts, uint32_t *words, const int32_t *verdicts, uint32_t *seen, int32_t *calls);
int sph_selftest_walk(SphHandle *h, int walk, int src, int rigid, const uint32_t *lists, const int *counts, uint32_t run_first, uint32_t run_n,
                      const float *A, const float *B, const float *C, const float *S, size_t n_src, const float *RP, size_t n_rig, uint32_t *out);

#ifdef __cplusplus
}
#endif
#endif
