// sph_mi355x.hip -- host side of libsph_mi355x.so: scene construction, buffer ownership, the per-step
// launch sequences for WCSPH and DFSPH, and the C-ABI of include/sph_mi355x.h.
//
// There is no CPU fallback: without a HIP device sph_create fails with SPH_E_NO_DEVICE.
#include "../../include/sph_mi355x.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "sph_kernels.h"
#include <dlfcn.h>
#include <rccl/rccl.h>      // types only: librccl is dlopen'ed when a handle attaches the native transport
#include "sph_slab_kernels.h"
#include "sph_pressure_kernels.h"
#include "sph_rigid_kernels.h"
#include "sph_pbf_kernels.h"
#include "sph_relaxed_kernels.h"
#include "sph_diag_kernels.h"
#include "sph_derived_kernels.h"
#include "sph_scalar_kernels.h"
#include "sph_wall_load_kernels.h"
#include "sph_selftest_walk.h"

using namespace sph;

namespace {

enum KernelId {
    K_HASH = 0, K_SCAN, K_SCATTER, K_ORDER_GATHER, K_BUILD_NL, K_W_DENSITY, K_W_FORCE, K_D_DENSITY_ALPHA,
    K_D_WARM, K_D_DIV_RESIDUAL, K_D_DIV_CORRECT, K_D_EXT, K_D_DENS_RESIDUAL, K_D_DENS_CORRECT, K_D_INTEGRATE,
    K_FINALIZE, K_TRANSFER, K_SLAB, K_RIGID, K_P_EXT, K_P_PREDICT_RHO, K_P_PRESS, K_P_INTEGRATE, K_I_ADVECT, K_I_RHO_ADV, K_I_DIJ,
    K_I_UPDATE_P, K_I_INTEGRATE, K_B_LAMBDA, K_B_DELTA, K_B_XSPH, K_ACCEL, K_DERIVED, K_SCALAR, K_WALL_LOAD, K_COUNT
};
const char *kKernelNames[K_COUNT] = {
    "hash_count", "scan", "scatter", "order_gather", "build_nl", "wcsph_density", "wcsph_force", "dfsph_density_alpha",
    "dfsph_warm_start", "dfsph_div_residual", "dfsph_div_correct", "dfsph_ext_force", "dfsph_dens_residual",
    "dfsph_dens_correct", "dfsph_integrate", "finalize", "transfer", "slab_exchange", "rigid",
    "pcisph_ext_force", "pcisph_predict_rho", "pcisph_press_force", "pcisph_integrate", "iisph_advect", "iisph_rho_adv", "iisph_d_ij",
    "iisph_update_p", "iisph_integrate", "pbf_lambda", "pbf_delta_pos", "pbf_xsph", "accel_eval", "derived", "scalar", "wall_load"};

thread_local std::string g_create_error;
thread_local bool g_creating_with_rigid = false;     // sph_create_rigid builds the fluid handle first: no Verlet lists there (the body moves through the grid)

// Development overrides.  The SPH_* environment knobs (layout and arithmetic switches for A/B runs, tests and tools) take effect only
// when SPH_DEV=1 is set as well; without it a set knob is ignored with one line on stderr.  Every override that did take effect is
// recorded and reported by sph_overrides(), so that a measurement can name (or refuse) the switches it ran under.
const char *dev_env(std::string *record, const char *name)
{
    const char *e = getenv(name);
    if (!e) return nullptr;
    const char *dev = getenv("SPH_DEV");
    if (!(dev && dev[0] == '1' && dev[1] == 0)) {
        static thread_local std::string warned;
        if (warned.find(std::string(";") + name + ";") == std::string::npos) {
            warned += std::string(";") + name + ";";
            fprintf(stderr, "libsph_mi355x: %s is set but ignored (development overrides need SPH_DEV=1)\n", name);
        }
        return nullptr;
    }
    if (record && record->find(std::string(name) + "=") == std::string::npos) {
        if (!record->empty()) *record += ";";
        *record += std::string(name) + "=" + e;
    }
    return e;
}

// Memory with an owner.  DevMem: a plan of (pointer, element count) requests, committed as ONE hipMalloc -- every array on a
// 256-byte boundary, arrays of 2 MiB and more on a 2 MiB boundary, in the order of the requests -- zeroed on the caller's stream unless told not to,
// freed with its owner, move-only.  A commit that fails sets no pointer and holds no memory.  The handle's arenas (one per build phase: dalloc /
// dcommit, sph_host_scene.h), every feature's side memory and the self-tests' scratch are DevMems.  Releasing does not reach back into the pointers
// it handed out: whoever releases a live feature's memory clears them (scalar_disable).
struct DevFree { void operator()(void *p) const { (void)hipFree(p); } };
struct PinnedFree { void operator()(void *p) const { (void)hipHostFree(p); } };
struct DevMem {
    std::unique_ptr<char, DevFree> base;                     // (move-only through it)
    size_t bytes = 0;
    std::vector<std::pair<void **, size_t>> plan;            // requests not yet committed
    std::vector<std::pair<const void *, size_t>> blocks;     // every array of the allocation with its bytes
    explicit operator bool() const { return (bool)base; }
    void release() { base.reset(); bytes = 0; plan.clear(); blocks.clear(); }
    template <class T>
    void want(T **p, size_t count)
    {
        *p = nullptr;
        plan.push_back({(void **)p, sizeof(T) * (count > 0 ? count : 1)});
    }
    hipError_t commit(hipStream_t stream, bool zero = true)
    {
        const size_t big = (size_t)2 << 20;
        std::vector<size_t> off(plan.size());
        size_t cur = 0;
        for (size_t k = 0; k < plan.size(); ++k) {
            const size_t align = plan[k].second >= big ? big : 256;
            cur = (cur + align - 1) / align * align;
            off[k] = cur;
            cur += plan[k].second;
        }
        char *mem = nullptr;
        hipError_t e = hipMalloc((void **)&mem, cur > 0 ? cur : 1);
        if (e == hipSuccess && zero && (e = hipMemsetAsync(mem, 0, cur, stream)) != hipSuccess) (void)hipFree(mem);
        if (e != hipSuccess) { plan.clear(); return e; }
        base.reset(mem); bytes = cur; blocks.clear();
        for (size_t k = 0; k < off.size(); ++k) { *plan[k].first = mem + off[k]; blocks.push_back({mem + off[k], plan[k].second}); }
        plan.clear();
        return hipSuccess;
    }
    size_t bytes_of(const void *p) const           // bytes of one of its arrays (0: not one)
    {
        for (const auto &b : blocks) if (b.first == p) return b.second;
        return 0;
    }
};

// ... and its pinned twin: one hipHostMalloc with the caller's flags, the pointer handed out as DevMem hands out its own (null after a failure)
struct PinnedMem {
    std::unique_ptr<void, PinnedFree> base;
    void release() { base.reset(); }
    template <class T>
    hipError_t commit(T **p, size_t count, unsigned flags = hipHostMallocDefault)
    {
        void *mem = nullptr;
        const hipError_t e = hipHostMalloc(&mem, sizeof(T) * (count > 0 ? count : 1), flags);
        base.reset(e == hipSuccess ? mem : nullptr);
        *p = (T *)base.get();
        return e;
    }
};

}  // namespace

struct SphHandle {
    SphConfig cfg;
    Consts c;
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;
    std::string overrides;       // development overrides in force on this handle (dev_env)

    // the solver attributes a caller of the reference may edit before (or, for the Python-scope loops, between) steps: solver_base.py:23-26,
    // wcsph_solver.py:17-20, dfsph_solver.py:21-29; sph_set_scalar(SPH_P_*) writes them, apply_params() folds them into Consts / DevScalars
    struct Params {
        double density_threshold = 0.1, density_divergence_threshold = 10, max_dt = 1e-3, min_dt = 1e-5;
        int min_iteration_density = 2, min_iteration_density_divergence = 1, max_iteration_density_divergence = 15;
        int warm_start = 1, adaptive_dt = 1;
        double viscosity_c_s = 13, viscosity_alpha = 0.08, viscosity_epsilon = 0.01, tension_k = 0.5;
    } p;

    int N = 0, Nb = 0, Nr = 0;
    int nblocks = 0;
    float dt_wcsph = 0.f;
    // the adaptive time step of wcsph / pcisph / iisph / pbf (SPH_P_STEP_*).  While it is on the step's dt -- and pcisph's
    // delta -- live in DevScalars (k_step_dt) and dt_wcsph / pci_delta are what they were when it was switched on; switching it off reads them back
    bool step_adaptive = false;
    double step_max_dt = 0.0, step_min_dt = 1e-5;          // max_dt: delta_time as configured (build_scene)
    int simulate_cnt = 0;
    // gravity as a vector, constant or harmonic (sph_set_gravity / sph_set_forcing): the host's copy of DevScalars.frc.  frc.accel is exact here
    // while frc.on == 0 (= frc.g); under forcing the device forms it (k_accel_eval) and a read-back refreshes this copy
    DevScalars::Forcing frc = {};
    bool nl_valid = false;      // neighbour list matches the current positions
    bool density_valid = false;
    bool pbf_fields = false;    // pbf: pbf_lambda / delta_pos are those of the last step, in the current device order (slab handles lose them at a re-sort)

    // device state (sorted order); index [cur] is the live one
    float4 *P[2] = {nullptr, nullptr};
    float4 *V[2] = {nullptr, nullptr};
    float4 *VA[2] = {nullptr, nullptr};   // dfsph v* ping-pong; VA[0] doubles as wcsph acc and iisph v_adv (sph_host_fields.h)
    float *warm[2] = {nullptr, nullptr};
    int *id[2] = {nullptr, nullptr};
    int pcur = 0, vcur = 0, vacur = 0, wcur = 0, icur = 0;

    float *rho = nullptr, *aux = nullptr /* pressure | alpha | a_ii | pbf_lambda: sph_host_fields.h */, *drho = nullptr, *rho_adv = nullptr, *krho = nullptr /* k / rho (kr_split) */;
    float4 *X[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};   // per-solver working arrays: which is what is said once, by pci_fields / ii_fields / pbf_arrays (sph_host_fields.h)
    int pb_final = 0;            // which PB holds press_iter / p_iter after the last step
    unsigned sweep_lds = 0;      // sph_tune_time: dynamic LDS bytes per block on the unstaged DFSPH sweeps (caps the waves per CU)
    int last_iters = 2;          // iteration count of the last step's density / pressure loop: size of the next step's first chunk
    float pci_delta = 0.f, pci_beta = 0.f;   // pcisph_solver.py:23-24, :47
    float pci_s = 0.f;                       // :47, the sums under delta: (sum grad W)^2 + sum |grad W|^2 of the fullest neighbourhood
    int pci_max_index = -1, pci_max_count = -1;
    std::vector<float> pci_fluid_pos, rigid_pos_host;   // initial lattice / placed rigid samples, for pre_compute's 27-cell walk on the host
    int *cnt = nullptr;
    uint32_t *nl = nullptr, *nlb = nullptr;
    int *cell_of = nullptr, *rank = nullptr, *slot_src = nullptr;
    int *cell_count = nullptr, *cell_start = nullptr, *tile_sums = nullptr;
    int ntiles = 0;
    float4 *WP = nullptr;        // wall particles, cell-sorted: (x, y, z, V_b)
    int *wcell_start = nullptr;
    // Everything the handle owns on the device or pinned on the host, but the measured wall set's memory, which travels with its view (wl.mem):
    // sph_destroy lets go of it in one statement, a feature adds its owner HERE.  The pointers into these live beside what they serve, below
    struct Owned {
        DevMem arena_next;                           // dalloc() requests not yet committed
        std::vector<DevMem> arenas;                  // dcommit() allocations, one per build phase: every dalloc'd array with its bytes (dalloc_bytes)
        DevMem diag, diag_ring, diag_ctl;            // run diagnostics: the scratch of both uses, the ring, the device-resident counters
        DevMem derived, scalar, geometry;            // sections 6j, 6k, 6l
        DevMem comm, red, gath, cnt;                 // the transport's message buffers, reduction buffer, gathered triples and counts, where the library owns them
        PinnedMem ds, pub, rred, cnt_host, red_host, counters, col_hist;
    } own;
    int *tile_rank = nullptr;            // Consts.tile_rank
    // slab handles on the Morton curve keep the cell slots of THEIR columns only (slab_local_grid): the whole grid's tile ranks, and the slot count the
    // cell arrays were allocated for
    std::vector<int> tile_rank_full, tile_rank_local;
    int S_full = 0;
    bool staged = false;                 // LDS staging of the sweeps' gather operand (k_build_nl plan)
    int quad_below = 65536;              // quad sweeps (four lanes per particle) for unstaged single-GPU handles of up to this many particles
    bool opt_quad = true;                // SPH_QUAD=0 at sph_create: small scenes keep one lane per particle in the sweeps (A/B, tests)
    int opt_bnl_split = -1;              // SPH_BNL_SPLIT=0 | 3 | 9 at sph_create: never / always k_build_nl_split with that many waves (A/B, tests); -1: by size
    bool opt_nl16 = true, opt_kr_split = true;   // SPH_NL16=0 / SPH_KR_SPLIT=0 at sph_create (A/B, tests)
    bool relaxed = false;                        // SphConfig.arith == SPH_ARITH_RELAXED (or SPH_ARITH=relaxed in the environment: tools)
    float4 *wall_grad = nullptr;                 // relaxed handles: per-step wall sums (k_rx_wall_grad)
    float *wall_gsq = nullptr;                   //   ... and the walls' share of alpha's denominator
    float4 *wall_gc = nullptr;                   // exact dfsph sweeps: (grad W_ib, V_b) per wall-list entry, written by D1 (for_wall_cache)
    bool opt_wall_cache = true;                  // SPH_WALL_CACHE=0 at sph_create: D2-D7 walk the wall lists themselves (A/B, tests)
    // the pair-bit cache of the staged 16-bit walks (walk_list16 in sph_kernels.h): one word per lane per group of eight list entries, written by D1.
    // It belongs to ONE list build: nl_gen counts the builds, pair_bits_gen is the build D1 last wrote the cache for (pair_bits_for)
    uint32_t *pair_bits = nullptr;
    uint64_t nl_gen = 0, pair_bits_gen = ~(uint64_t)0;
    bool pair_bits_read = false;                 // SPH_S_PAIR_BITS: the last dfsph step's solver-loop sweeps read the cache
    // change propagation between the sweeps of the density loop (sph_kernels.h: stage_sources_flagged); SPH_TILE_SKIP=0 turns it off
    int *wave_dirty = nullptr;                   // per 64-particle wave: did the last density correction change a velocity there?
    unsigned char *changed8 = nullptr;           // ... and per particle (the second, exact level of the residual sweep's check)
    int *pci_zero_press = nullptr;               // pcisph: per tile, "press_force / pos_predict hold the zero-pressure values" (k_pci_press); iisph: "d_ij holds zeros" (k_ii_dij)
    bool opt_tile_skip = true, dens_first = true, tune_all = false;
    bool verlet = false;                         // wcsph under the relaxed arithmetic: lists with a skin, rebuilt on demand (sph_relaxed_kernels.h)
    float4 *x0 = nullptr;                        //   ... positions at the last list build
    // slab handles: what the transport was asked to do since the last sph_comm_stats(reset): [0] point-to-point groups (a send / recv
    // pair with each neighbour), [1] bytes sent, [2] bytes received, [3] count exchanges (one host round trip each), [4] all-reduces
    // ordered on the stream, [5] all-reduces through the host, [6] steps
    long long comm_stat[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    uint2 *stage_src = nullptr;          // cell runs of every workgroup's staged set (kStageMaxCells per workgroup)
    int *stage_cnt = nullptr;
    double *psum = nullptr; int *pcnt = nullptr; float *pmax = nullptr;
    DevScalars *ds = nullptr;    // device
    DevScalars *ds_host = nullptr;   // pinned mirror
    DevScalarsPub *pub_host = nullptr, *pub_dev = nullptr;      // the same block as the device publishes it itself (k_publish_scalars): pinned, mapped
    unsigned long long pub_seq = 0;
    int pub_late = 0;               // read_scalars_fast: consecutive reads whose word arrived only with the stream's drain
    float *staging = nullptr;    // 3*max(N,Nb) floats, device
    // host copies of the wall particles in original order (for download)
    std::vector<float> wall_pos_host, wall_vol_host;
    std::vector<int> wall_order_host;      // ... and wall_tables' order: the row of the wall set in sorted slot e

    // multi-GPU x-slab state (slab_count > 1)
    bool slab = false;
    int slab_rank = 0, nslab = 1;
    SlabGeom geom = {0, 0, 0, 0, 1, 0, 0};
    int ncap = 0;                 // capacity (particles) of every per-particle array
    int n_owned = 0, n_ghost = 0, n_dead = 0;
    bool comm_set = false;
    SphComm comm = {};
    void *dsend[2] = {nullptr, nullptr}, *drecv[2] = {nullptr, nullptr};   // device-side message buffers: the library's (own.comm) or the caller's (SphComm, on_host 0)
    int *dead = nullptr;
    // ordered edge lists, one per (side, direction): 0 ghost-left, 1 send-left, 2 send-right, 3 ghost-right.  With two ghost columns per side a
    // list holds the column next to the cut first (edge_n[k][0] entries), then the second one (edge_n[k][1]); edge_off[2 k + l] are the per-cell
    // offsets of column l of list k
    int *edge_off[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    int *edge_list[4] = {nullptr, nullptr, nullptr, nullptr};
    int edge_n[4][2] = {{0, 0}, {0, 0}, {0, 0}, {0, 0}};
    bool cuts_moved = false;          // this step's re-balancing moved a cut: the particle exchange runs its two-round form
    bool overlap = false;             // dfsph, two ghost columns: edge tiles of the residual sweeps first, halo on xstream under the interior tiles
    hipStream_t xstream = nullptr;    // the halo's stream when overlap is on
    hipEvent_t ev_edge = nullptr, ev_halo = nullptr;
    // ... and the residual's all-reduce + loop decision on a third stream, under the next correction sweep (slab_can_overlap; step_dfsph_device_loops)
    hipStream_t rstream = nullptr;
    hipEvent_t ev_red = nullptr, ev_dec = nullptr;
    float4 *spec_v = nullptr; float *spec_w = nullptr;      // what a divergence correction that ran ahead of its loop decision overwrote (SpecSave / SpecUndo)
    int *tile_flag = nullptr, *tile_order = nullptr;
    bool overlap_on = true;       // sph_slab_set_overlap: the split + the hidden all-reduce may be switched off between steps (same bits either way)
    std::vector<int> cuts;        // all slabs' cell-column cuts (identical on every rank)
    double *red_dev = nullptr;    // (sum, count) / max of this slab on its way through allreduce_stream
    // native transport (sph_rccl_attach): the library drives RCCL itself on its stream
    bool native = false;
    ncclComm_t nccl = nullptr;
    int red_cap = 4;              // doubles in red_dev
    int *cnt_dev = nullptr, *cnt_host = nullptr;     // neighbour count exchange: [send_left, send_right, recv_left, recv_right]
    double *red_host = nullptr;   // pinned staging for host-side all-reduces
    double *gath_dev = nullptr;   // native transport, in-order protocol: every slab's (sum, count, flags), four doubles per slab (native_exchange)
    bool opt_gather = true;       // SPH_SLAB_GATHER=0: the residual pair is all-reduced instead (A/B)
    // one GPU, density loop: working tiles first in the change-propagated launches (TilePhase.sparse / hot in sph_kernels.h)
    FinRide pending_div = kNoRide;      // one GPU: the divergence loop's last decision, taken by k_finalize_max's launch
    int *dens_hot = nullptr, *dens_order = nullptr;
    bool dens_sparse = false;
    // ... and the producer says who must run (DensFlow in sph_kernels.h): the tiles that stage each tile's particles (k_build_nl), the stamps the
    // density loop's sweeps push to them, per tile "its k / rho holds a nonzero", the two broadcast words.  SPH_DENS_PUSH=0 turns it off (A/B, tests)
    int *tile_nbr = nullptr, *need6 = nullptr, *need7 = nullptr, *tile_nz = nullptr, *dens_bcast = nullptr, *worked6 = nullptr, *worked7 = nullptr;
    int flow_stamp = 0, flow_last = 0;          // launch counter of the density loop's sweeps; the stamp of the sweep enqueued last
    DensFlow flow_d6 = kNoFlow;                 // ... and the residual sweep's whole block: a split sweep's second launch and the kernel that unpacks the ghosts' k / rho push with it
    bool opt_dens_push = true;
    bool opt_layer_generic = false;  // SPH_LAYER_GENERIC=1: k_layer_offsets in the form columns of more than 18 432 cells take (tests)
    bool opt_slab_check = false;     // SPH_SLAB_CHECK=1: the host's edge-column bookkeeping against the sorted arrays, every step (tests, soak runs)
    int rebalance_every = 0, steps_since_rebalance = 0, n_recuts = 0;
    int *col_hist = nullptr, *col_hist_host = nullptr;
    int *counters = nullptr, *counters_host = nullptr;
    int *class_cnt = nullptr;     // k_classify_*: per-workgroup counts / offsets, kSlabCounted arrays of (capacity / 256) ints
    std::vector<int> init_ids;    // original ids of the particles this handle owns at t = 0

    // rigid body (config 5)
    bool rigid = false;
    int rigid_active = 0;         // ps.active_rigid[None]: read at step time (rigid_binned / rigid_coupled), written by sph_rigid_set_active
    bool rigid_data_binned = false;   // the volumes / masses / centroid / inertia were last derived with the body binned (rigid_init_data)
    bool lists_predate_flag = false;  // sph_rigid_set_active ran after the last list build: cnt / ncount still count for the old flag
    int Nv = 0;
    float rigid_rho = 0.f;
    float4 *RPos = nullptr;       // [Nr] rigid particles in their own index order: (x, y, z, V_r)
    float4 *RPs = nullptr;        // [Nr] cell-sorted copy, rebuilt every step
    uint32_t *rnl = nullptr;             // fluid neighbours of the rigid sample particles (k_build_rnl), rcnt = their number
    int *rcnt = nullptr;
    int *rid = nullptr, *rcell_of = nullptr, *rrank = nullptr, *rslot = nullptr, *rcell_count = nullptr, *rcell_start = nullptr;
    float *rforce = nullptr;      // [3 Nr] rigid_particles.force
    float *rvert = nullptr;       // [3 Nv] mesh vertices
    float4 *pos_orig = nullptr;   // fluid positions by original id   (get_neighbour_count quirk)
    float *rho_orig = nullptr;    // fluid densities by original id   (viscosity quirk)
    int *ncount = nullptr;        // ps.get_neighbour_count(i) with rigid entries
    RigidReduce *rred = nullptr, *rred_host = nullptr;      // kRigidParts partials on the device, combined into rred_host[0] (read_rigid_reduce)
    float *rvmax_part = nullptr;
    std::vector<float> rvol_host, rmass_host;
    float centroid[3] = {0, 0, 0}, inertia_inv[9] = {0}, r_vel[3] = {0, 0, 0}, r_acc[3] = {0, 0, 0}, r_omega[3] = {0, 0, 0},
          r_alpha[3] = {0, 0, 0};
    float rs_dt = 0.f, rs_omega[3] = {0, 0, 0}, rs_attitude[3] = {0, 0, 0}, rs_mass = 0.f;
    bool rs_run_once = false;
    int rs_cnt = 0;
    // what sph_rigid_step does with the body (SPH_RIGID_*), the motion a scripted body follows, and the load of the last body step
    int rigid_mode = SPH_RIGID_DYNAMIC;
    float rm_vel[3] = {0, 0, 0}, rm_omega[3] = {0, 0, 0}, rm_acc[3] = {0, 0, 0}, rm_alpha[3] = {0, 0, 0};
    float rigid_radius = 0.f;     // largest |sample - centroid| when rigid_init_data last ran: the sphere of a scripted step's grid guard
    double *rload = nullptr;      // [6] force, torque of the last scripted / fixed step (k_rigid_load)
    double rload_host[6] = {0, 0, 0, 0, 0, 0};
    int rload_at = 0;             // 0: no body step yet, 1: rload_host (a dynamic step's host sums), 2: rload on the device

    // hipGraph replay of WCSPH step pairs (launch-bound at small N): one executable graph per buffer parity
    hipGraphExec_t wcsph_graph[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    bool graphs_enabled = true;
    long long graph_launches = 0;

    // run diagnostics: memory of its own, taken at the first use.  diag_part: the partial rows, diag_row: the on-demand row;
    // recording (diag_every > 0): the ring, the device-resident counters, and how many recorded rows sph_diag_read has handed out or seen overwritten
    double *diag_part = nullptr, *diag_row = nullptr, *diag_ring = nullptr;
    DiagCtl *diag_ctl = nullptr;
    int diag_every = 0, diag_rows = 0;
    long long diag_consumed = 0;

    // derived per-particle fields: memory of its own, taken at the first sph_derived.  drv_vr: (vel, rho) packed; drv_out: the
    // 17 planes of the result in device order; drv_api: one quantity in API order.  derived_valid: drv_out describes the state the handle holds --
    // taken down wherever density_valid is
    float4 *drv_vr = nullptr;
    float *drv_out = nullptr, *drv_api = nullptr;
    bool derived_valid = false;

    // the carried scalar: memory of its own, taken by sph_scalar_enable and freed by sph_scalar_disable; sc_T != null is
    // "enabled".  sc_T: the values by particle id (API order); sc_XT: (x, y, z, T) packed in device order; sc_rate: dT/dt in device order, scratch
    // between steps
    float4 *sc_XT = nullptr;
    float *sc_rate = nullptr, *sc_T = nullptr;
    double sc_D = 0.0;
    float sc_beta = 0.f, sc_ref = 0.f, sc_inflow = 0.f;

    // static geometry: the wall set is the box samples (group 0, the first Nb0) and behind them every live group in order of
    // addition.  own.geometry: memory of the feature's own, taken at the first sph_geometry_add and grown, never shrunk: WP of the edited set (h->WP
    // points into it from then on), wgroup (the group of every sample in sorted order) and the carve verdicts
    struct GeoGroup { int id, count; };
    std::vector<GeoGroup> geo_groups;
    int geo_next_id = 1;
    size_t geo_cap = 0;                    // wall samples own.geometry has room for (+ 64 of padding, as the arena's WP)
    int *geo_wgroup = nullptr, *geo_marked = nullptr;

    // loads on walls and geometry.  wl_groups: the selection in the caller's order (first: the group's first row of the
    // wall set); empty: measuring is off and no step launches anything of the feature.  wl: the measured set, memory of the feature's own, taken
    // by sph_wall_load_select and rebuilt by every edit of the wall set while a selection stands (sph_host_wall_load.h)
    struct WlGroup { int id, first, count; };
    std::vector<WlGroup> wl_groups;
    struct WlMem {
        DevMem mem;
        int nm = 0;                          // samples of the measured set
        size_t nl_bytes = 0;
        float4 *MP = nullptr;                // [nm + 64] (x, y, z, V_b) in the wall set's sorted order
        uint32_t *nl = nullptr;              // [(nm + 64) kpitch] the samples' fluid neighbours (k_build_rnl), cnt their number
        int *cnt = nullptr, *ident = nullptr /* 0 .. nm - 1: the forces stay in sorted order */, *slot = nullptr, *local = nullptr, *perm = nullptr, *seg = nullptr;
        float *force = nullptr, *out = nullptr;      // [3 nm] the step's per-sample totals; one group's in its own order (sph_wall_load_forces)
        double *part = nullptr, *load = nullptr, *acc = nullptr;      // the reduction's partial rows, its result per group, what a group accumulates
    } wl;

    // profiling
    bool profiling = false;
    struct Ev { hipEvent_t a, b; int kid; };
    std::vector<Ev> ev_pending;
    std::vector<hipEvent_t> ev_pool;
    double prof_ms[K_COUNT] = {0};
    int64_t prof_n[K_COUNT] = {0};
};

namespace {

int fail(SphHandle *h, int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    if (h) h->err = buf; else g_create_error = buf;
    return code;
}

#define HIP_TRY(h, expr)                                                                        \
    do {                                                                                        \
        hipError_t e_ = (expr);                                                                 \
        if (e_ != hipSuccess) return fail(h, SPH_E_HIP, "%s: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

hipEvent_t take_event(SphHandle *h)
{
    if (!h->ev_pool.empty()) { hipEvent_t e = h->ev_pool.back(); h->ev_pool.pop_back(); return e; }
    hipEvent_t e; (void)hipEventCreate(&e); return e;
}

struct ProfScope {
    SphHandle *h; int kid; hipEvent_t a = nullptr, b = nullptr; hipStream_t st;
    ProfScope(SphHandle *h_, int kid_, hipStream_t on = nullptr) : h(h_), kid(kid_), st(on ? on : h_->stream)
    {
        if (h->profiling) { a = take_event(h); b = take_event(h); (void)hipEventRecord(a, st); }
    }
    ~ProfScope()
    {
        if (h->profiling) { (void)hipEventRecord(b, st); h->ev_pending.push_back({a, b, kid}); }
    }
};

void drain_profile(SphHandle *h)
{
    if (h->ev_pending.empty()) return;
    (void)hipStreamSynchronize(h->stream);
    if (h->xstream) (void)hipStreamSynchronize(h->xstream);
    if (h->rstream) (void)hipStreamSynchronize(h->rstream);
    for (auto &e : h->ev_pending) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, e.a, e.b) == hipSuccess) { h->prof_ms[e.kid] += ms; h->prof_n[e.kid] += 1; }
        h->ev_pool.push_back(e.a); h->ev_pool.push_back(e.b);
    }
    h->ev_pending.clear();
}

inline dim3 grid_for(int n) { return dim3((unsigned)std::max(1, (n + kBlock - 1) / kBlock)); }   // an empty slab still launches one (idle) block

#include "sph_host_scene.h"
#include "sph_host_fields.h"
#include "sph_host_diag.h"
#include "sph_host_transport.h"
#include "sph_host_rigid.h"
#include "sph_host_wall_load.h"
#include "sph_host_scalar.h"
#include "sph_host_dfsph.h"
#include "sph_host_pressure.h"
#include "sph_host_derived.h"
#include "sph_host_flow.h"
#include "sph_host_geometry.h"

}  // namespace

// =============================================================================================
// C-ABI
// =============================================================================================
extern "C" {

const char *sph_last_error(SphHandle *h) { return h ? h->err.c_str() : g_create_error.c_str(); }

int sph_create(const SphConfig *cfg, SphHandle **out)
{
    if (!cfg || !out) return fail(nullptr, SPH_E_INVALID, "null argument");
    *out = nullptr;
    if (cfg->solver < SPH_SOLVER_WCSPH || cfg->solver > SPH_SOLVER_PBF)
        return fail(nullptr, SPH_E_INVALID, "unknown solver %d", cfg->solver);
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0)
        return fail(nullptr, SPH_E_NO_DEVICE, "no HIP device available (%s); libsph_mi355x has no CPU fallback",
                    e == hipSuccess ? "device count 0" : hipGetErrorString(e));
    if (cfg->device < 0 || cfg->device >= ndev) return fail(nullptr, SPH_E_INVALID, "device %d out of range [0,%d)", cfg->device, ndev);
    SphHandle *h = new SphHandle();
    h->cfg = *cfg;
    h->device = cfg->device;
    { const char *e = dev_env(&h->overrides, "SPH_SLAB_GATHER"); h->opt_gather = !(e && atoi(e) == 0); }
    { const char *e = dev_env(&h->overrides, "SPH_LAYER_GENERIC"); h->opt_layer_generic = e && atoi(e) != 0; }
    { const char *e = dev_env(&h->overrides, "SPH_SLAB_CHECK"); h->opt_slab_check = e && atoi(e) != 0; }       // ("0" is off: eight blocking read-backs per step otherwise)
    { const char *e = dev_env(&h->overrides, "SPH_NL16"); h->opt_nl16 = !(e && atoi(e) == 0); }
    { const char *e = dev_env(&h->overrides, "SPH_KR_SPLIT"); h->opt_kr_split = !(e && atoi(e) == 0); }
    { const char *e = dev_env(&h->overrides, "SPH_TILE_SKIP"); h->opt_tile_skip = !(e && atoi(e) == 0); }
    { const char *e = dev_env(&h->overrides, "SPH_DENS_PUSH"); h->opt_dens_push = !(e && atoi(e) == 0); }
    { const char *e = dev_env(&h->overrides, "SPH_WALL_CACHE"); h->opt_wall_cache = !(e && atoi(e) == 0); }
    { const char *e = dev_env(&h->overrides, "SPH_ARITH"); h->relaxed = cfg->arith == SPH_ARITH_RELAXED || (e && (e[0] == 'r' || e[0] == '1')); }
    { const char *e = dev_env(&h->overrides, "SPH_QUAD"); h->opt_quad = !(e && atoi(e) == 0); }
    { const char *e = dev_env(&h->overrides, "SPH_BNL_SPLIT"); const int v = e ? atoi(e) : -1; h->opt_bnl_split = (v == 0 || v == 3 || v == 9) ? v : -1; }
    int rc = SPH_OK;
    do {
        if (hipSetDevice(h->device) != hipSuccess) { rc = fail(h, SPH_E_HIP, "hipSetDevice(%d) failed", h->device); break; }
        if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) { rc = fail(h, SPH_E_HIP, "hipStreamCreate failed"); break; }
        HostScene sc;
        if ((rc = build_scene(h, sc))) break;
        if ((rc = alloc_device(h, sc))) break;
        if (h->cfg.solver == SPH_SOLVER_PCISPH) {
            if (!h->slab) h->pci_fluid_pos = sc.fluid_pos;
            if ((rc = pcisph_precompute(h))) break;
        }
        h->wall_pos_host = sc.wall_pos;
        h->wall_vol_host = sc.wall_vol;
    } while (0);
    if (rc) {
        g_create_error = h->err;
        sph_destroy(h);
        return rc;
    }
    *out = h;
    return SPH_OK;
}

int sph_create_rigid(const SphConfig *cfg, const SphRigid *rigid, SphHandle **out)
{
    if (!cfg || !rigid || !out) return fail(nullptr, SPH_E_INVALID, "null argument");
    // slab handles: a coupled body on every solver but pbf.  wcsph / pcisph / iisph run on one ghost column (a sample of an edge column finds its fluid
    // neighbours there, with the owners' values: k_rigid_force_p); dfsph's body needs the two-column protocol, whose inner ghosts run the sweeps themselves
    if (cfg->slab_count > 1 && cfg->solver == SPH_SOLVER_DFSPH && cfg->slab_ghost_layers == 1)
        return fail(nullptr, SPH_E_INVALID, "a rigid body on slab handles needs dfsph with two ghost columns (the body's fluid neighbours must be resident on the rank that owns its column)");
    if (rigid->n_particles <= 0 || !rigid->points) return fail(nullptr, SPH_E_INVALID, "rigid body has no sample points");
    if (cfg->solver == SPH_SOLVER_PBF) return fail(nullptr, SPH_E_INVALID, "pbf has no rigid coupling (pbf_solver.py has no material branches)");
    // a one-way body (active, fs_couple 0: binned, not coupled -- sph_host_rigid.h) is followed on single-GPU handles with the exact arithmetic.
    // The slab transport gathers the quirk's fluid positions for coupled bodies only, and the relaxed kernels count without the quirk: refused
    const bool one_way = rigid->active && !cfg->fs_couple;
    if (one_way && cfg->slab_count > 1)
        return fail(nullptr, SPH_E_INVALID, "a one-way rigid body (active, fs_couple 0) is not supported on slab handles: use slab_count 1 or fs_couple 1");
    g_creating_with_rigid = true;
    int rc = sph_create(cfg, out);
    g_creating_with_rigid = false;
    if (rc) return rc;
    SphHandle *h = *out;
    if (one_way && h->relaxed)
        rc = fail(h, SPH_E_INVALID, "a one-way rigid body (active, fs_couple 0) needs the exact arithmetic (SPH_ARITH_EXACT): the relaxed kernels do not "
                                    "take get_neighbour_count's rigid-entry quirk");
    if (!rc) rc = build_rigid(h, rigid);
    if (!rc && h->cfg.solver == SPH_SOLVER_PCISPH) rc = pcisph_precompute(h);   // the solver is constructed after the ParticleSystem: the grid holds the body
    if (rc) {
        g_create_error = h->err;
        sph_destroy(h);
        *out = nullptr;
    }
    return rc;
}

// `ps.active_rigid[None] = active` (ParticleSystem.py:63-64; main.py:102): the flag, and nothing that was derived from the body
int sph_rigid_set_active(SphHandle *h, int active)
{
    if (!h) return SPH_E_INVALID;
    if (!h->rigid) return fail(h, SPH_E_STATE, "handle has no rigid body");
    if (h->slab) return fail(h, SPH_E_STATE, "sph_rigid_set_active is not available on slab handles (the body is replicated on every rank)");
    if (active && !h->cfg.fs_couple && h->relaxed)
        return fail(h, SPH_E_STATE, "a one-way rigid body (active, fs_couple 0) needs the exact arithmetic (SPH_ARITH_EXACT): the relaxed kernels do not "
                                    "take get_neighbour_count's rigid-entry quirk");
    if (rigid_coupled(h) && !active) {
        // The sweeps fetch one group of list entries past a row's end -- "stale but valid indices" (walk_list, sph_kernels.h).  Rows written while
        // the body was coupled hold entries tagged with bit 31; beyond the shorter rows of the next build a sweep without the RIGID branches would
        // take them for fluid indices.  Index 0 is valid in every list format
        HIP_TRY(h, hipSetDevice(h->device));
        HIP_TRY(h, hipMemsetAsync(h->nl, 0, sizeof(uint32_t) * ((size_t)h->c.stride + 64) * (size_t)h->c.kpitch, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
    }
    h->rigid_active = active ? 1 : 0;
    // what the last list build derived with the old flag: the fluid lists (tagged rigid entries or none), cnt / ncount, the rigid sort, the body's
    // lists (rnl / rcnt), the exact / relaxed tile split (tile_order) -- stage_sort_and_lists rebuilds all of it from the flag it finds.  The
    // density loop's working-tiles-first order (dens_order) is a launch order only; it starts afresh as on a new handle
    mark_stale(h, STALE_BODY_FLAG);
    return SPH_OK;
}

// ps.init_rigid_particles_data() (ParticleSystem.py:249-291) from the body's CURRENT sample positions, binned or not by the flag of this moment
int sph_rigid_init_data(SphHandle *h)
{
    if (!h) return SPH_E_INVALID;
    if (!h->rigid) return fail(h, SPH_E_STATE, "handle has no rigid body");
    if (h->slab) return fail(h, SPH_E_STATE, "sph_rigid_init_data is not available on slab handles (the body is replicated on every rank)");
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t nr = (size_t)h->Nr;
    std::vector<float4> rp4(nr);
    HIP_TRY(h, hipMemcpyAsync(rp4.data(), h->RPos, sizeof(float4) * nr, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    std::vector<float> rpos(3 * nr);
    for (size_t i = 0; i < nr; ++i) { rpos[3 * i] = rp4[i].x; rpos[3 * i + 1] = rp4[i].y; rpos[3 * i + 2] = rp4[i].z; }
    int rc = rigid_init_data(h, rpos, rigid_binned(h));
    if (rc) return rc;
    // the new volumes into RPos[i].w (a strided copy: the positions stay the device's); RPs takes them at the next sort of the samples
    HIP_TRY(h, hipMemcpy2DAsync(&h->RPos[0].w, sizeof(float4), h->rvol_host.data(), sizeof(float), sizeof(float), nr, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    mark_stale(h, STALE_BODY_DATA);
    return SPH_OK;
}

int sph_rigid_step(SphHandle *h)
{
    if (!h) return SPH_E_INVALID;
    if (!h->rigid) return fail(h, SPH_E_STATE, "handle has no rigid body");
    if (int rc = rigid_released_unprepared(h)) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    float dt;
    if (int rc = rigid_next_dt(h, &dt)) return rc;
    if (h->rigid_mode == SPH_RIGID_SCRIPTED)
        if (int rc = rigid_scripted_guard(h, dt)) return rc;
    if (h->slab) {       // every sample's force was summed whole by the rank that owns its column (k_rigid_force): add the ranks' arrays up, x + 0 = x
        const int n3 = 3 * h->Nr;
        hipLaunchKernelGGL(k_floats_to_doubles, grid_for(n3), dim3(kBlock), 0, h->stream, n3, h->rforce, h->red_dev);
        int rc = slab_allreduce_stream(h, n3, 0);
        if (rc) return rc;
        hipLaunchKernelGGL(k_doubles_to_floats, grid_for(n3), dim3(kBlock), 0, h->stream, n3, h->red_dev, h->rforce);
    }
    return rigid_step(h, dt);
}

int sph_rigid_set_mode(SphHandle *h, int mode)
{
    if (!h) return SPH_E_INVALID;
    if (!h->rigid) return fail(h, SPH_E_STATE, "handle has no rigid body");
    if (mode != SPH_RIGID_DYNAMIC && mode != SPH_RIGID_SCRIPTED && mode != SPH_RIGID_FIXED) return fail(h, SPH_E_INVALID, "unknown rigid body mode %d", mode);
    h->rigid_mode = mode;
    return SPH_OK;
}

int sph_rigid_set_motion(SphHandle *h, const float vel[3], const float omega[3], const float acc[3], const float alpha[3])
{
    if (!h) return SPH_E_INVALID;
    if (!h->rigid) return fail(h, SPH_E_STATE, "handle has no rigid body");
    if (!vel || !omega) return fail(h, SPH_E_INVALID, "sph_rigid_set_motion: vel and omega must be given");
    const float *in[4] = {vel, omega, acc, alpha};
    for (int q = 0; q < 4; ++q)
        for (int a = 0; a < 3; ++a)
            if (in[q] && !std::isfinite(in[q][a])) return fail(h, SPH_E_INVALID, "sph_rigid_set_motion: a value that is not finite");
    for (int a = 0; a < 3; ++a) {
        h->rm_vel[a] = vel[a]; h->rm_omega[a] = omega[a];
        h->rm_acc[a] = acc ? acc[a] : 0.0f; h->rm_alpha[a] = alpha ? alpha[a] : 0.0f;
    }
    return SPH_OK;
}

int sph_rigid_get_load(SphHandle *h, double force[3], double torque[3])
{
    if (!h || !force || !torque) return SPH_E_INVALID;
    if (!h->rigid) return fail(h, SPH_E_STATE, "handle has no rigid body");
    if (h->rload_at == 0) return fail(h, SPH_E_STATE, "sph_rigid_get_load before the first sph_rigid_step");
    if (h->rload_at == 2) {
        HIP_TRY(h, hipSetDevice(h->device));
        HIP_TRY(h, hipMemcpyAsync(h->rload_host, h->rload, sizeof(double) * 6, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        h->rload_at = 1;
    }
    for (int a = 0; a < 3; ++a) { force[a] = h->rload_host[a]; torque[a] = h->rload_host[3 + a]; }
    return SPH_OK;
}

// ---- inlets and sinks (flow_refused, fluid_count_changed and remove_where: sph_host_flow.h) ----------------------
int sph_add_particles(SphHandle *h, const float *pos, const float *vel, size_t n, int32_t *first_id)
{
    if (!h) return SPH_E_INVALID;
    if (int rc = flow_refused(h, "sph_add_particles")) return rc;
    if (n == 0) { if (first_id) *first_id = h->N; return SPH_OK; }
    if (!pos) return fail(h, SPH_E_INVALID, "sph_add_particles: null positions");
    if (n > (size_t)(h->ncap - h->N))
        return fail(h, SPH_E_INVALID, "sph_add_particles: %d particles held, %zu more exceed the capacity of %d (SphConfig.fluid_capacity)", h->N, n, h->ncap);
    const float lo[3] = {(float)h->cfg.box_min[0], (float)h->cfg.box_min[1], (float)h->cfg.box_min[2]};
    const float hi[3] = {(float)h->cfg.box_max[0], (float)h->cfg.box_max[1], (float)h->cfg.box_max[2]};
    for (size_t i = 0; i < n; ++i)
        for (int a = 0; a < 3; ++a) {
            const float x = pos[3 * i + a];
            if (!std::isfinite(x) || (vel && !std::isfinite(vel[3 * i + a]))) return fail(h, SPH_E_INVALID, "sph_add_particles: particle %zu has a coordinate or velocity that is not finite", i);
            if (!(lo[a] < x && x < hi[a])) return fail(h, SPH_E_INVALID, "sph_add_particles: particle %zu lies at %g on axis %d, not strictly inside the box (%g, %g)", i, (double)x, a, (double)lo[a], (double)hi[a]);
        }
    HIP_TRY(h, hipSetDevice(h->device));
    hipStream_t s = h->stream;
    HIP_TRY(h, hipStreamSynchronize(s));
    // one copy of the new rows (positions, then velocities) and one k_append; the staging buffer holds 3 x capacity floats, so a call that brings
    // more than half the capacity WITH velocities goes in two
    const PbfFields pbf = h->cfg.solver == SPH_SOLVER_PBF ? pbf_arrays(h) : PbfFields{};      // the new rows' pbf_lambda and delta_pos start at zero
    const size_t per = vel ? 6 : 3, room = 3 * (size_t)h->c.stride / per;
    std::vector<float> rows;
    int at = h->N;
    for (size_t first = 0; first < n; first += room) {
        const size_t m = std::min(room, n - first);
        rows.assign(pos + 3 * first, pos + 3 * (first + m));
        if (vel) rows.insert(rows.end(), vel + 3 * first, vel + 3 * (first + m));
        HIP_TRY(h, hipMemcpyAsync(h->staging, rows.data(), sizeof(float) * rows.size(), hipMemcpyHostToDevice, s));
        ProfScope ps(h, K_TRANSFER);
        hipLaunchKernelGGL(k_append, grid_for((int)m), dim3(kBlock), 0, s, at, (int)m, at, (const float *)h->staging, vel ? 1 : 0, h->P[h->pcur], h->V[h->vcur],
                           carries_scalar(h) ? h->warm[h->wcur] : (float *)nullptr, h->id[h->icur], h->x0, h->rho, pbf.lambda, pbf.delta_pos);
        HIP_TRY(h, hipGetLastError());
        HIP_TRY(h, hipStreamSynchronize(s));          // (rows is reused)
        at += (int)m;
    }
    if (scalar_on(h))                                 // the new rows carry the handle's inflow value
        if (int rc = scalar_fill(h, h->N, at - h->N, h->sc_inflow)) return rc;
    if (first_id) *first_id = h->N;
    return fluid_count_changed(h, at);
}

int sph_remove_in_box(SphHandle *h, const float lo[3], const float hi[3], int32_t *removed)
{
    if (!h) return SPH_E_INVALID;
    if (int rc = flow_refused(h, "sph_remove_in_box")) return rc;
    if (!lo || !hi) return fail(h, SPH_E_INVALID, "sph_remove_in_box: null argument");
    RemoveBox box;
    for (int a = 0; a < 3; ++a) { box.lo[a] = lo[a]; box.hi[a] = hi[a]; }
    return remove_where(h, "sph_remove_in_box", "the box holds", box, [&](int n, const float4 *P, const int *id, int *flag_slot, int *flag_id) {
        hipLaunchKernelGGL(k_remove_flag, grid_for(n), dim3(kBlock), 0, h->stream, n, box, P, id, flag_slot, flag_id);
    }, removed);
}

// ---- static geometry -------------------------------------------------------------------------------------------
int sph_geometry_add(SphHandle *h, const float *xyz, size_t n, int32_t *group) { return h ? geometry_add(h, xyz, n, group) : SPH_E_INVALID; }
int sph_geometry_remove(SphHandle *h, int32_t group) { return h ? geometry_remove(h, group) : SPH_E_INVALID; }
int sph_geometry_info(SphHandle *h, int32_t *groups, int32_t *first, int32_t *count, size_t cap, size_t *n_groups)
{
    return h ? geometry_info(h, groups, first, count, cap, n_groups) : SPH_E_INVALID;
}
int sph_geometry_carve(SphHandle *h, int32_t group, float clearance, int32_t *removed) { return h ? geometry_carve(h, group, clearance, removed) : SPH_E_INVALID; }
int sph_geometry_wall_counts(SphHandle *h, int32_t *counts, size_t n) { return h ? geometry_wall_counts(h, counts, n) : SPH_E_INVALID; }

// ---- loads on walls and geometry (sph_host_wall_load.h) ----------------------------------------------------------
int sph_wall_load_select(SphHandle *h, const int32_t *groups, size_t n) { return h ? wall_load_select(h, groups, n) : SPH_E_INVALID; }
int sph_wall_load_get(SphHandle *h, int32_t group, const double about[3], double force[3], double torque[3])
{
    return h ? wall_load_get(h, group, about, force, torque) : SPH_E_INVALID;
}
int sph_wall_load_impulse(SphHandle *h, int32_t group, const double about[3], double impulse[3], double angular[3], double *seconds, int reset)
{
    return h ? wall_load_impulse(h, group, about, impulse, angular, seconds, reset) : SPH_E_INVALID;
}
int sph_wall_load_forces(SphHandle *h, int32_t group, float *xyz, size_t n_floats) { return h ? wall_load_forces(h, group, xyz, n_floats) : SPH_E_INVALID; }

void sph_destroy(SphHandle *h)
{
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    for (auto &e : h->ev_pending) { (void)hipEventDestroy(e.a); (void)hipEventDestroy(e.b); }
    for (auto &e : h->ev_pool) (void)hipEventDestroy(e);
    for (int k = 0; k < 8; ++k) if (h->wcsph_graph[k]) (void)hipGraphExecDestroy(h->wcsph_graph[k]);
    h->own = SphHandle::Owned();                               // every arena, side memory, message buffer and pinned buffer ...
    h->wl.mem.release();                                       // ... and the measured wall set's, which travels with its view
    if (h->nccl && rccl().ok) (void)rccl().CommDestroy(h->nccl);
    if (h->ev_edge) (void)hipEventDestroy(h->ev_edge);
    if (h->ev_halo) (void)hipEventDestroy(h->ev_halo);
    if (h->xstream) { (void)hipStreamSynchronize(h->xstream); (void)hipStreamDestroy(h->xstream); }
    if (h->ev_red) (void)hipEventDestroy(h->ev_red);
    if (h->ev_dec) (void)hipEventDestroy(h->ev_dec);
    if (h->rstream) { (void)hipStreamSynchronize(h->rstream); (void)hipStreamDestroy(h->rstream); }
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
}

int sph_get_sizes(SphHandle *h, SphSizes *out)
{
    if (!h || !out) return SPH_E_INVALID;
    out->n_fluid = h->N; out->n_wall = h->Nb; out->n_rigid = h->rigid ? h->Nr : 0;
    out->grid[0] = h->c.gx; out->grid[1] = h->c.gy; out->grid[2] = h->c.gz;
    out->n_cells = h->c.C;
    out->max_neighbors = h->c.kmax; out->max_wall_neighbors = h->c.kbmax;
    return SPH_OK;
}

int sph_upload(SphHandle *h, int species, int field, const float *host, size_t n_floats)
{
    if (!h || !host) return SPH_E_INVALID;
    HIP_TRY(h, hipSetDevice(h->device));
    size_t count;
    int rc = field_floats(h, species, field, &count);
    if (rc) return rc;
    if (count != n_floats) return fail(h, SPH_E_INVALID, "field %d holds %zu floats, got %zu", field, count, n_floats);
    const FieldRow *row = species == SPH_SPECIES_FLUID ? fluid_field(field) : nullptr;
    if (!row || !row->upload) return fail(h, SPH_E_INVALID, "field %d is read-only", field);
    if (h->slab) return fail(h, SPH_E_STATE, "sph_upload is not available on a slab handle: sph_slab_set_state replaces its whole state (pos, vel, the travelling scalar, delta_time)");
    if (!(row->upload & (1u << h->cfg.solver))) return fail(h, SPH_E_STATE, "%s", row->not_owner);
    FieldLoc f;
    if ((rc = locate_field(h, field, FV_API, &f))) return rc;
    hipStream_t s = h->stream;
    HIP_TRY(h, hipMemcpyAsync(h->staging, host, sizeof(float) * count, hipMemcpyHostToDevice, s));
    ProfScope ps(h, K_TRANSFER);
    launch_sort_in(h, h->staging, f);
    HIP_TRY(h, hipGetLastError());
    if (int rc = mark_stale(h, STALE_FIELD)) return rc;      // new positions: neither the lists of the last build (Verlet ones included) nor what was computed over them apply
    HIP_TRY(h, hipStreamSynchronize(s));
    return SPH_OK;
}

int sph_download(SphHandle *h, int species, int field, float *host, size_t n_floats)
{
    if (!h || !host) return SPH_E_INVALID;
    HIP_TRY(h, hipSetDevice(h->device));
    size_t count;
    int rc = field_floats(h, species, field, &count);
    if (rc) return rc;
    if (count != n_floats) return fail(h, SPH_E_INVALID, "field %d holds %zu floats, got %zu", field, count, n_floats);
    if (species == SPH_SPECIES_WALL) {
        const std::vector<float> &src = field == SPH_F_WALL_POS ? h->wall_pos_host : h->wall_vol_host;
        memcpy(host, src.data(), sizeof(float) * count);
        return SPH_OK;
    }
    if (species == SPH_SPECIES_RIGID) {
        if (field == SPH_F_RIGID_VOL || field == SPH_F_RIGID_MASS) {
            memcpy(host, (field == SPH_F_RIGID_VOL ? h->rvol_host : h->rmass_host).data(), sizeof(float) * count);
            return SPH_OK;
        }
        hipStream_t s = h->stream;
        if (field == SPH_F_RIGID_POS) {
            hipLaunchKernelGGL(k_copy_vec_local, grid_for(h->Nr), dim3(kBlock), 0, s, h->Nr, h->RPos, h->staging);
            HIP_TRY(h, hipGetLastError());
            HIP_TRY(h, hipMemcpyAsync(host, h->staging, sizeof(float) * count, hipMemcpyDeviceToHost, s));
        } else {
            HIP_TRY(h, hipMemcpyAsync(host, field == SPH_F_RIGID_FORCE ? h->rforce : h->rvert, sizeof(float) * count, hipMemcpyDeviceToHost, s));
        }
        HIP_TRY(h, hipStreamSynchronize(s));
        return SPH_OK;
    }
    if (h->slab) return fail(h, SPH_E_STATE, "slab handle: use sph_download_local + sph_download_ids (device order, owned and ghost particles)");
    // get_neighbour_count after sph_rigid_set_active: the count of the flag as it stands, not of the lists built before it changed
    if (field == SPH_F_NBR_COUNT && h->lists_predate_flag && (rc = sph_build_neighbors(h))) return rc;
    FieldLoc f;
    if ((rc = locate_field(h, field, FV_API, &f))) return rc;
    return fetch_api_order(h, [&] { launch_unsort(h, f, h->staging); }, h->staging, host, sizeof(float) * count);
}

int sph_plan_slabs(const SphConfig *cfg, int32_t *cuts, int32_t *counts)
{
    // host-only: runs the same scene construction as sph_create on a throw-away handle, no device needed
    if (!cfg || !cuts || !counts || cfg->slab_count < 1) return fail(nullptr, SPH_E_INVALID, "bad argument");
    SphHandle tmp;
    tmp.cfg = *cfg;
    HostScene sc;
    const int nslab = cfg->slab_count;
    tmp.cfg.slab_count = 1;                  // build the full lattice
    tmp.cfg.slab_rank = 0;
    int rc = build_scene(&tmp, sc);
    if (rc) { g_create_error = tmp.err; return rc; }
    std::vector<int> col, cut;
    std::string why;
    if (!plan_slab_cuts(sc.fluid_pos, tmp.N, tmp.c.h, tmp.c.gx, nslab, col, cut, why, slab_layers_of(*cfg))) return fail(nullptr, SPH_E_INVALID, "%s", why.c_str());
    for (int k = 0; k <= nslab; ++k) cuts[k] = cut[k];
    for (int k = 0; k < nslab; ++k) counts[k] = 0;
    for (int i = 0; i < tmp.N; ++i)
        for (int k = 0; k < nslab; ++k)
            if (col[i] >= cut[k] && col[i] < cut[k + 1]) { counts[k]++; break; }
    return SPH_OK;
}

int sph_replan_slabs(const int64_t *column_histogram, int32_t grid_x, int32_t slab_count, const int32_t *old_cuts, int32_t ghost_layers, int32_t *new_cuts)
{
    if (!column_histogram || !old_cuts || !new_cuts || grid_x < 2 || slab_count < 1 || grid_x < kMinSlabColumns * slab_count || ghost_layers < 0 || ghost_layers > 2)
        return fail(nullptr, SPH_E_INVALID, "bad argument");
    for (int k = 0; k < slab_count; ++k)
        if (old_cuts[k + 1] < old_cuts[k] + kMinSlabColumns || old_cuts[0] != 0 || old_cuts[slab_count] != grid_x)
            return fail(nullptr, SPH_E_INVALID, "old cuts must start at 0, end at grid_x and leave every slab >= %d columns", kMinSlabColumns);
    std::vector<long long> hist(column_histogram, column_histogram + grid_x);
    std::vector<int> oldc(old_cuts, old_cuts + slab_count + 1), cut;
    replan_slab_cuts(hist, grid_x, slab_count, oldc, cut, ghost_layers);
    for (int k = 0; k <= slab_count; ++k) new_cuts[k] = cut[k];
    return SPH_OK;
}

// the four device-side message buffers as the library's own (the native transport; a callback transport with host buffers): one allocation, not
// zeroed -- a message is written before it is sent.  Whether the library owns them is whether own.comm holds memory
static int own_message_buffers(SphHandle *h, size_t capacity_bytes)
{
    char *buf[4] = {nullptr, nullptr, nullptr, nullptr};
    for (int k = 0; k < 4; ++k) h->own.comm.want(&buf[k], capacity_bytes);
    HIP_TRY(h, h->own.comm.commit(h->stream, false));
    for (int k = 0; k < 2; ++k) { h->dsend[k] = buf[2 * k]; h->drecv[k] = buf[2 * k + 1]; }
    return SPH_OK;
}

int sph_rccl_unique_id(void *id128)
{
    if (!id128) return SPH_E_INVALID;
    RcclApi &n = rccl();
    if (!n.ok) return fail(nullptr, SPH_E_STATE, "RCCL is not available: %s", n.why.c_str());
    ncclUniqueId id;
    ncclResult_t r = n.GetUniqueId(&id);
    if (r != ncclSuccess) return fail(nullptr, SPH_E_HIP, "ncclGetUniqueId failed: %s", n.GetErrorString(r));
    memcpy(id128, id.internal, NCCL_UNIQUE_ID_BYTES);
    return SPH_OK;
}

int sph_rccl_attach(SphHandle *h, const void *id128, size_t capacity_bytes)
{
    if (!h || !id128) return SPH_E_INVALID;
    RcclApi &n = rccl();
    if (!n.ok) return fail(h, SPH_E_STATE, "RCCL is not available: %s", n.why.c_str());
    (void)dev_env(&h->overrides, "SPH_RCCL_LIB");       // reported by sph_overrides() when a stand-in transport library is in force
    if (h->native) return fail(h, SPH_E_STATE, "the native transport is already attached");
    if (capacity_bytes < 4096) return fail(h, SPH_E_INVALID, "halo buffers smaller than 4 KiB");
    HIP_TRY(h, hipSetDevice(h->device));
    // a single-GPU handle may attach as a communicator of one rank: that is all a 1-GPU box can exercise (tests), it never exchanges
    const int rank = h->slab ? h->slab_rank : 0, world = h->slab ? h->nslab : 1;
    ncclUniqueId id;
    memcpy(id.internal, id128, NCCL_UNIQUE_ID_BYTES);
    NCCL_TRY(h, n.CommInitRank(&h->nccl, world, id, rank));
    if (int rc = own_message_buffers(h, capacity_bytes)) return rc;
    h->red_cap = (int)std::max<size_t>(std::max(1024, h->c.gx + 8), slab_reduce_need(h));      // the re-balancing histogram (gx counts) and a rigid body's by-id sums go through it too
    h->own.red.want(&h->red_dev, (size_t)h->red_cap);
    HIP_TRY(h, h->own.red.commit(h->stream, false));
    HIP_TRY(h, h->own.red_host.commit(&h->red_host, (size_t)h->red_cap));
    h->own.gath.want(&h->gath_dev, 4 * (size_t)std::max(world, 1));
    HIP_TRY(h, h->own.gath.commit(h->stream));                      // (zeroed)
    h->own.cnt.want(&h->cnt_dev, 4 * kCountInts);
    HIP_TRY(h, h->own.cnt.commit(h->stream, false));
    HIP_TRY(h, h->own.cnt_host.commit(&h->cnt_host, 4 * kCountInts));
    memset(&h->comm, 0, sizeof(h->comm));
    h->comm.capacity = capacity_bytes;
    h->comm.stream_ordered = 1;
    // the native transport starts in order (one stream; the residual's triple rides with the halo): with transfers and collectives that take
    // 0-50 us to start it is the faster protocol in every replay (profiles/r04/loopback/link_latency_sweep.txt); slab_overlap = 2 starts overlapped,
    // sph_slab_set_overlap switches between steps (bench.py times both)
    h->overlap_on = h->cfg.slab_overlap == 2;
    h->native = true;
    h->comm_set = true;
    return SPH_OK;
}

int sph_rccl_selftest(SphHandle *h, double *inout, int32_t n, int32_t op)
{
    if (!h || !inout || n < 1) return SPH_E_INVALID;
    if (!h->native) return fail(h, SPH_E_STATE, "attach the native transport first (sph_rccl_attach)");
    HIP_TRY(h, hipSetDevice(h->device));
    int rc = slab_allreduce_host(h, inout, n, op);       // H2D, ncclAllReduce on the handle's stream, D2H
    if (rc) return rc;
    int32_t rl = -1, rr = -1;
    if ((rc = native_exchange_counts(h, 11, 22, &rl, &rr))) return rc;
    if (!h->slab && (rl != 0 || rr != 0)) return fail(h, SPH_E_STATE, "a one-rank communicator has no neighbours");
    return native_exchange(h, 0, 0, 0, 0);
}

int32_t sph_abi_version(void) { return SPH_ABI_VERSION; }

int sph_set_comm_sized(SphHandle *h, const SphComm *comm, size_t comm_size)
{
    if (!h || !comm) return SPH_E_INVALID;
    if (comm_size < offsetof(SphComm, allreduce_stream)) return fail(h, SPH_E_INVALID, "SphComm of %zu bytes is older than any this library knows", comm_size);
    SphComm full;
    memset(&full, 0, sizeof(full));
    memcpy(&full, comm, std::min(comm_size, sizeof(full)));
    return sph_set_comm(h, &full);
}

int sph_set_comm(SphHandle *h, const SphComm *comm)
{
    if (!h || !comm) return SPH_E_INVALID;
    if (!h->slab) return fail(h, SPH_E_STATE, "sph_set_comm needs a handle created with slab_count > 1");
    if (h->native) return fail(h, SPH_E_STATE, "the native RCCL transport is attached to this handle");
    if (!comm->exchange_counts || !comm->exchange_buffers || !comm->allreduce) return fail(h, SPH_E_INVALID, "SphComm callbacks must all be set");
    if (!comm->send_left || !comm->send_right || !comm->recv_left || !comm->recv_right || comm->capacity < 4096)
        return fail(h, SPH_E_INVALID, "SphComm buffers missing or smaller than 4 KiB");
    HIP_TRY(h, hipSetDevice(h->device));
    h->own.comm.release();
    h->comm = *comm;
    if (comm->on_host) {
        if (int rc = own_message_buffers(h, comm->capacity)) return rc;
    } else {
        h->dsend[0] = comm->send_left; h->dsend[1] = comm->send_right;
        h->drecv[0] = comm->recv_left; h->drecv[1] = comm->recv_right;
    }
    h->own.red.release();
    h->red_dev = nullptr;
    if (comm->allreduce_stream) {
        if (!comm->reduce_buf) return fail(h, SPH_E_INVALID, "SphComm.allreduce_stream needs reduce_buf");
        const size_t have = comm->reduce_capacity ? comm->reduce_capacity : 4;
        if (have < slab_reduce_need(h))
            return fail(h, SPH_E_INVALID, "SphComm.reduce_buf holds %zu doubles, this handle (rigid body of %d samples) needs %zu: set reduce_capacity", have, h->Nr, slab_reduce_need(h));
        h->red_cap = (int)std::min<size_t>(have, 0x7fffffff);
        if (comm->on_host) { h->own.red.want(&h->red_dev, have); HIP_TRY(h, h->own.red.commit(h->stream, false)); }
        else h->red_dev = comm->reduce_buf;
    } else if (h->rigid) {
        return fail(h, SPH_E_INVALID, "a rigid body on a slab handle needs a transport with allreduce_stream");
    }
    if (comm->stream_ordered && comm->on_host) return fail(h, SPH_E_INVALID, "a stream-ordered transport needs device buffers (on_host = 0)");
    h->overlap_on = true;          // (a synchronous transport is slow: the overlapped protocol wins there, profiles/r04/rehearsal_2ranks.json)
    h->comm_set = true;
    return SPH_OK;
}

int sph_get_stream(SphHandle *h, void **stream)
{
    if (!h || !stream) return SPH_E_INVALID;
    *stream = (void *)h->stream;
    return SPH_OK;
}

int sph_comm_stats(SphHandle *h, int64_t *out, int reset)
{
    if (!h || !out) return SPH_E_INVALID;
    for (int k = 0; k < 8; ++k) out[k] = (int64_t)h->comm_stat[k];
    if (reset) for (int k = 0; k < 8; ++k) h->comm_stat[k] = 0;
    return SPH_OK;
}

int sph_slab_info(SphHandle *h, int32_t *out)
{
    if (!h || !out) return SPH_E_INVALID;
    out[0] = h->n_owned; out[1] = h->slab ? h->c.n - h->n_owned : 0;
    out[2] = h->geom.x_lo; out[3] = h->slab ? h->geom.x_hi : h->c.gx; out[4] = h->ncap;
    out[5] = h->n_recuts; out[6] = h->rebalance_every;
    // the halo protocol in force: ghost columns per side | 16 if the residual sweeps run edge tiles first with the halo on its own stream | 32 if the
    // residual's all-reduce and loop decision run on a third stream under the next correction sweep (both need a transport that can: slab_can_overlap)
    out[7] = !h->slab ? 0 : h->geom.layers | ((h->geom.layers == 2 && h->comm_set && slab_can_overlap(h)) ? 16 : 0) |
                            ((h->geom.layers == 2 && h->comm_set && slab_can_overlap(h) && slab_async(h) && h->rstream && is_dfsph(h)) ? 32 : 0);
    return SPH_OK;
}

// Between steps, on every slab alike: run the dfsph loops with the halo and the reductions on their own streams (1; needs a handle created with
// slab_overlap != 1) or in order on the handle's stream (0).  The bits do not change; which is faster depends on the link and on the slab's
// size -- with the link time at zero a rank of 1.2 M particles steps 12 % faster in order, on a slow link the overlap wins:
// bench.py times both on the node it runs on.
int sph_slab_set_overlap(SphHandle *h, int32_t on)
{
    if (!h) return SPH_E_INVALID;
    if (!h->slab) return fail(h, SPH_E_STATE, "not a slab handle");
    if (on && !h->overlap) return fail(h, SPH_E_STATE, "this handle was created without the overlapped protocol (slab_overlap = 1, or one ghost column)");
    h->overlap_on = on != 0;
    return SPH_OK;
}

int sph_slab_set_state(SphHandle *h, const float *pos, const float *vel, const float *scalar, size_t n_fluid, double delta_time)
{
    if (!h) return SPH_E_INVALID;
    if (!h->slab) return fail(h, SPH_E_STATE, "sph_slab_set_state needs a handle created with slab_count > 1 (one GPU: sph_upload + sph_set_scalar)");
    if (!h->comm_set) return fail(h, SPH_E_STATE, "slab handle needs sph_set_comm or sph_rccl_attach before sph_slab_set_state (the slabs agree on one verdict)");
    HIP_TRY(h, hipSetDevice(h->device));
    return slab_set_state(h, pos, vel, scalar, n_fluid, delta_time);
}

int sph_download_ids(SphHandle *h, int32_t *host, size_t n)
{
    if (!h || !host) return SPH_E_INVALID;
    HIP_TRY(h, hipSetDevice(h->device));
    if (n != (size_t)h->c.n) return fail(h, SPH_E_INVALID, "%d particles resident, got room for %zu", h->c.n, n);
    HIP_TRY(h, hipMemcpyAsync(host, h->id[h->icur], sizeof(int) * n, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return SPH_OK;
}

int sph_download_local(SphHandle *h, int field, float *host, size_t n_floats)
{
    if (!h || !host) return SPH_E_INVALID;
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t n = (size_t)h->c.n;
    FieldLoc f;
    if (int rc = locate_field(h, field, FV_LOCAL, &f)) return rc;
    const bool vec = f.kind == FK_XYZ;               // (the local view offers xyz and float arrays only)
    const size_t want = vec ? 3 * n : n;
    if (n_floats != want) return fail(h, SPH_E_INVALID, "field %d holds %zu floats locally, got %zu", field, want, n_floats);
    if (vec) {
        ProfScope ps(h, K_TRANSFER);
        hipLaunchKernelGGL(k_copy_vec_local, grid_for((int)n), dim3(kBlock), 0, h->stream, (int)n, (const float4 *)f.data, h->staging);
        HIP_TRY(h, hipGetLastError());
        HIP_TRY(h, hipMemcpyAsync(host, h->staging, sizeof(float) * want, hipMemcpyDeviceToHost, h->stream));
    } else {
        HIP_TRY(h, hipMemcpyAsync(host, f.data, sizeof(float) * want, hipMemcpyDeviceToHost, h->stream));
    }
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return SPH_OK;
}

int sph_build_neighbors(SphHandle *h)
{
    if (!h) return SPH_E_INVALID;
    HIP_TRY(h, hipSetDevice(h->device));
    // pbf_lambda and delta_pos are per-particle fields of the solver that neither update_grid nor compute_all_rho touches; they live in device order
    // (pbf_arrays), which the re-sort changes: carry them through in API order -- lambda in the staging buffer, delta_pos as 3 N floats in pos_new
    // (phase 1's new positions: scratch between steps, 4 N floats).  Here and not in sph_compute_density: a sph_build_neighbors of its own re-sorts too
    // Slab handles do NOT carry: there id[] holds global ids (~id for ghosts), fewer or more than N particles are resident, and the re-sort starts with
    // a particle exchange that changes who is -- k_unsort_* / k_sort_in_* over N elements would index outside the arrays.  pbf_lambda / delta_pos of a
    // slab handle are valid from a step until the next sort; sph_download_local answers SPH_E_STATE after it
    const bool keep = h->cfg.solver == SPH_SOLVER_PBF && h->simulate_cnt > 0 && !h->slab;
    if (h->slab) h->pbf_fields = false;
    FieldLoc lambda = {}, delta_pos = {};
    float *delta_pos_api = keep ? (float *)pbf_arrays(h).pos_new : nullptr;
    int rc;
    if (keep) {
        if ((rc = locate_field(h, SPH_F_PBF_LAMBDA, FV_API, &lambda)) || (rc = locate_field(h, SPH_F_PBF_DELTA_POS, FV_API, &delta_pos))) return rc;
        launch_unsort(h, lambda, h->staging);
        launch_unsort(h, delta_pos, delta_pos_api);
    }
    if ((rc = stage_sort_and_lists(h))) return rc;
    if (keep) {
        launch_sort_in(h, h->staging, lambda);
        launch_sort_in(h, delta_pos_api, delta_pos);
    }
    if ((rc = read_scalars(h))) return rc;
    return check_overflow_all(h);
}

int sph_compute_density(SphHandle *h)
{
    if (!h) return SPH_E_INVALID;
    HIP_TRY(h, hipSetDevice(h->device));
    int rc;
    if (!h->nl_valid && (rc = sph_build_neighbors(h))) return rc;      // (one GPU: carries pbf_lambda and delta_pos through its re-sort)
    if (h->density_valid) return SPH_OK;
    if ((rc = stage_density(h))) return rc;
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return SPH_OK;
}

int sph_compute_alpha(SphHandle *h)
{
    if (!h) return SPH_E_INVALID;
    if (h->cfg.solver != SPH_SOLVER_DFSPH) return fail(h, SPH_E_STATE, "alpha needs a dfsph handle");
    return sph_compute_density(h);   // the fused sweep produces rho and alpha together
}

// The WCSPH step is a fixed launch sequence with no host decision in it, so two steps (after which the ping-pong
// buffers are back in the same roles) are captured once into a hipGraph and replayed: at 30k particles the step is
// launch-bound and replay halves it.  Eager launches remain for odd remainders, profiling and slab handles.  *k: the steps taken
static int wcsph_replay_pairs(SphHandle *h, int nsteps, int *k)
{
    if (!(h->graphs_enabled && !h->profiling && !h->slab && !h->rigid && nsteps >= 2)) return SPH_OK;
    while (nsteps - *k >= 2) {
        const int key = h->pcur | (h->vcur << 1) | (h->icur << 2);
        if (!h->wcsph_graph[key]) {
            hipGraph_t graph = nullptr;
            const int sim_cnt = h->simulate_cnt;
            if (hipStreamBeginCapture(h->stream, hipStreamCaptureModeThreadLocal) != hipSuccess) { h->graphs_enabled = false; break; }
            int rc = step_wcsph_once(h);
            if (!rc) rc = step_wcsph_once(h);
            hipError_t e = hipStreamEndCapture(h->stream, &graph);
            h->simulate_cnt = sim_cnt;             // the capture launched nothing
            if (rc || e != hipSuccess || !graph) { if (graph) (void)hipGraphDestroy(graph); h->graphs_enabled = false; (void)hipGetLastError(); break; }
            e = hipGraphInstantiate(&h->wcsph_graph[key], graph, nullptr, nullptr, 0);
            (void)hipGraphDestroy(graph);
            if (e != hipSuccess) { h->wcsph_graph[key] = nullptr; h->graphs_enabled = false; (void)hipGetLastError(); break; }
            if ((h->pcur | (h->vcur << 1) | (h->icur << 2)) != key) { h->graphs_enabled = false; break; }   // roles must return after 2 steps
        }
        HIP_TRY(h, hipGraphLaunch(h->wcsph_graph[key], h->stream));
        h->graph_launches += 1;
        h->simulate_cnt += 2;
        mark_stale(h, STALE_STEP_RAN);
        *k += 2;
    }
    return SPH_OK;
}

// (the frame: run_steps in sph_host_dfsph.h.  wcsph and pbf steps read nothing back, so their calls end with the overflow read-back)
int sph_step_wcsph(SphHandle *h, int nsteps)
{
    const StepFrame f = {SPH_SOLVER_WCSPH, "handle was not created for wcsph", true, false, TAIL_ALWAYS};
    return run_steps(h, f, nsteps, nullptr, [](SphHandle *hh, SphStepStats *) { return step_wcsph_once(hh); }, [&](int *k) { return wcsph_replay_pairs(h, nsteps, k); });
}

int sph_step_dfsph(SphHandle *h, int nsteps, SphStepStats *last)
{
    const StepFrame f = {SPH_SOLVER_DFSPH, "handle was not created for dfsph", true, false, TAIL_NONE};
    return run_steps(h, f, nsteps, last, step_dfsph_once);
}

int sph_step_pcisph(SphHandle *h, int nsteps, SphStepStats *last)
{
    const StepFrame f = {SPH_SOLVER_PCISPH, "handle was not created for pcisph", true, false, TAIL_NONE};
    return run_steps(h, f, nsteps, last, step_pcisph_once);
}

int sph_step_iisph(SphHandle *h, int nsteps, SphStepStats *last)
{
    const StepFrame f = {SPH_SOLVER_IISPH, "handle was not created for iisph", true, false, TAIL_NONE};
    return run_steps(h, f, nsteps, last, step_iisph_once);
}

int sph_step_pbf(SphHandle *h, int nsteps)       // (pbf has no rigid coupling: nothing to have released)
{
    const StepFrame f = {SPH_SOLVER_PBF, "handle was not created with solver = SPH_SOLVER_PBF", false, true, TAIL_IF_STEPPED};
    return run_steps(h, f, nsteps, nullptr, [](SphHandle *hh, SphStepStats *) { return step_pbf_once(hh); });
}

int sph_get_scalar(SphHandle *h, int which, double *out)
{
    if (!h || !out) return SPH_E_INVALID;
    switch (which) {
    case SPH_S_DELTA_TIME:
        if (h->cfg.solver != SPH_SOLVER_DFSPH && !h->step_adaptive) { *out = (double)h->dt_wcsph; return SPH_OK; }   // a launch argument: the host's value
        else { int rc = read_scalars(h); if (rc) return rc; *out = (double)h->ds_host->dt; return SPH_OK; }
    case SPH_S_SIMULATE_CNT: *out = (double)h->simulate_cnt; return SPH_OK;
    case SPH_S_PARTICLE_M: *out = (double)h->c.m; return SPH_OK;
    case SPH_S_SUPPORT_RADIUS: *out = (double)h->c.h; return SPH_OK;
    case SPH_S_GRAPH_LAUNCHES: *out = (double)h->graph_launches; return SPH_OK;
    case SPH_S_PCISPH_DELTA:
        if (h->step_adaptive) { int rc = read_scalars(h); if (rc) return rc; *out = (double)h->ds_host->pci_delta; return SPH_OK; }      // k_step_dt's
        *out = (double)h->pci_delta; return SPH_OK;
    case SPH_S_PCISPH_BETA: *out = (double)h->pci_beta; return SPH_OK;
    case SPH_S_PCISPH_MAX_INDEX: *out = (double)h->pci_max_index; return SPH_OK;
    case SPH_S_PCISPH_MAX_COUNT: *out = (double)h->pci_max_count; return SPH_OK;
    case SPH_S_PS_DELTA_TIME: { int rc = read_scalars(h); if (rc) return rc; *out = (double)h->ds_host->ps_dt; return SPH_OK; }
    case SPH_S_ARITH_RELAXED: *out = (use_relaxed(h) || h->verlet || relaxed_pressure(h) || relaxed_unstaged(h) || relaxed_pbf(h)) ? 1.0 : 0.0; return SPH_OK;
    case SPH_S_RIGID_ACTIVE: *out = rigid_binned(h) ? 1.0 : 0.0; return SPH_OK;
    case SPH_S_RIGID_MODE: *out = h->rigid ? (double)h->rigid_mode : 0.0; return SPH_OK;
    case SPH_S_PAIR_BITS: *out = h->pair_bits_read ? 1.0 : 0.0; return SPH_OK;
    case SPH_S_FLUID_CAPACITY: *out = (double)(h->slab ? h->N : h->ncap); return SPH_OK;      // (a slab handle's ncap is its slab's: sph_slab_info)
    case SPH_S_TIME: { int rc = read_scalars(h); if (rc) return rc; *out = h->ds_host->sim_time; return SPH_OK; }
    case SPH_S_ACCEL: case SPH_S_ACCEL + 1: case SPH_S_ACCEL + 2:
        if (h->frc.on) {                                            // formed on the device (k_accel_eval): by the last step, or by a set call since
            int rc = read_scalars(h); if (rc) return rc;
            for (int a = 0; a < 3; ++a) h->frc.accel[a] = h->ds_host->frc.accel[a];
        }
        *out = (double)h->frc.accel[which - SPH_S_ACCEL]; return SPH_OK;
    case SPH_S_GRAVITY_VEC: case SPH_S_GRAVITY_VEC + 1: case SPH_S_GRAVITY_VEC + 2: *out = (double)h->frc.g[which - SPH_S_GRAVITY_VEC]; return SPH_OK;
    case SPH_S_VERLET_BUILDS: { int rc = read_scalars(h); if (rc) return rc; *out = (double)h->ds_host->verlet_builds; return SPH_OK; }      // kr_split is settled by the first list build
    case SPH_P_DENSITY_THRESHOLD: *out = h->p.density_threshold; return SPH_OK;
    case SPH_P_MIN_ITERATION_DENSITY: *out = h->p.min_iteration_density; return SPH_OK;
    case SPH_P_MIN_ITERATION_DENSITY_DIVERGENCE: *out = h->p.min_iteration_density_divergence; return SPH_OK;
    case SPH_P_MAX_ITERATION_DENSITY_DIVERGENCE: *out = h->p.max_iteration_density_divergence; return SPH_OK;
    case SPH_P_DENSITY_DIVERGENCE_THRESHOLD: *out = h->p.density_divergence_threshold; return SPH_OK;
    case SPH_P_WARM_START: *out = h->p.warm_start; return SPH_OK;
    case SPH_P_ADAPTIVE_DT: *out = h->p.adaptive_dt; return SPH_OK;
    case SPH_P_MAX_DT: *out = h->p.max_dt; return SPH_OK;
    case SPH_P_MIN_DT: *out = h->p.min_dt; return SPH_OK;
    case SPH_P_VISCOSITY_C_S: *out = h->p.viscosity_c_s; return SPH_OK;
    case SPH_P_VISCOSITY_ALPHA: *out = h->p.viscosity_alpha; return SPH_OK;
    case SPH_P_VISCOSITY_EPSILON: *out = h->p.viscosity_epsilon; return SPH_OK;
    case SPH_P_TENSION_K: *out = h->p.tension_k; return SPH_OK;
    case SPH_P_STEP_ADAPTIVE_DT: *out = h->step_adaptive ? 1.0 : 0.0; return SPH_OK;
    case SPH_P_STEP_MAX_DT: *out = h->step_max_dt; return SPH_OK;
    case SPH_P_STEP_MIN_DT: *out = h->step_min_dt; return SPH_OK;
    default:
        if (h->rigid && which >= SPH_S_RIGID_CENTROID && which < SPH_S_RIGID_INERTIA_INV + 9) {
            if (which < SPH_S_RIGID_OMEGA) *out = (double)h->centroid[which - SPH_S_RIGID_CENTROID];
            else if (which < SPH_S_RIGID_VEL) *out = (double)h->rs_omega[which - SPH_S_RIGID_OMEGA];
            else if (which < SPH_S_RIGID_MASS) *out = (double)h->r_vel[which - SPH_S_RIGID_VEL];
            else if (which == SPH_S_RIGID_MASS) *out = (double)h->rs_mass;
            else *out = (double)h->inertia_inv[which - SPH_S_RIGID_INERTIA_INV];
            return SPH_OK;
        }
        if (h->rigid && which >= SPH_S_RIGID_ACC && which < SPH_S_RIGID_ALPHA + 3) {
            *out = which < SPH_S_RIGID_ALPHA ? (double)h->r_acc[which - SPH_S_RIGID_ACC] : (double)h->r_alpha[which - SPH_S_RIGID_ALPHA];
            return SPH_OK;
        }
        return fail(h, SPH_E_INVALID, "unknown scalar %d", which);
    }
}

// the solver attributes a caller of the reference edits on the solver object (SPH_P_*): validated, kept in h->p, folded into the launch constants
// and the device's loop-control block
static int set_param(SphHandle *h, int which, double value)
{
    // validated into a COPY and committed at the end: a rejected call leaves the handle -- and what sph_get_scalar reports -- as it was
    SphHandle::Params p = h->p;
    const bool dfsph = h->cfg.solver == SPH_SOLVER_DFSPH;
    auto count = [&](int *dst, int lo) -> int {
        if (!(value >= lo && value <= 100000.0) || value != std::floor(value)) return fail(h, SPH_E_INVALID, "sph_set_scalar(%d): an integer >= %d expected, got %g", which, lo, value);
        *dst = (int)value; return SPH_OK;
    };
    // the reference takes whatever the caller assigns; what is refused here is what cannot be computed with: a value that is not finite, a time step bound <= 0
    auto finite = [&](double *dst) -> int {
        if (!std::isfinite(value)) return fail(h, SPH_E_INVALID, "sph_set_scalar(%d): a finite value expected, got %g", which, value);
        *dst = value; return SPH_OK;
    };
    auto positive = [&](double *dst) -> int {
        if (!(value > 0.0) || !std::isfinite(value)) return fail(h, SPH_E_INVALID, "sph_set_scalar(%d): a finite value > 0 expected, got %g", which, value);
        *dst = value; return SPH_OK;
    };
    int rc = SPH_OK;
    if (which >= SPH_P_DENSITY_THRESHOLD && which <= SPH_P_MIN_DT && !dfsph) return fail(h, SPH_E_STATE, "sph_set_scalar(%d): a dfsph_solver attribute on a handle of another solver", which);
    if (h->cfg.solver == SPH_SOLVER_PBF && which >= SPH_P_VISCOSITY_C_S && which <= SPH_P_TENSION_K) return fail(h, SPH_E_STATE, "sph_set_scalar(%d): pbf_solver has no such attribute", which);
    switch (which) {
    case SPH_P_DENSITY_THRESHOLD: rc = finite(&p.density_threshold); break;
    case SPH_P_MIN_ITERATION_DENSITY: rc = count(&p.min_iteration_density, 0); break;
    case SPH_P_MIN_ITERATION_DENSITY_DIVERGENCE: rc = count(&p.min_iteration_density_divergence, 0); break;
    case SPH_P_MAX_ITERATION_DENSITY_DIVERGENCE: rc = count(&p.max_iteration_density_divergence, 0); break;
    case SPH_P_DENSITY_DIVERGENCE_THRESHOLD: rc = finite(&p.density_divergence_threshold); break;
    case SPH_P_WARM_START: p.warm_start = value != 0.0; break;
    case SPH_P_ADAPTIVE_DT: p.adaptive_dt = value != 0.0; break;
    case SPH_P_MAX_DT: rc = positive(&p.max_dt); break;
    case SPH_P_MIN_DT: rc = positive(&p.min_dt); break;
    case SPH_P_VISCOSITY_C_S: rc = finite(&p.viscosity_c_s); break;
    case SPH_P_VISCOSITY_ALPHA: rc = finite(&p.viscosity_alpha); break;
    case SPH_P_VISCOSITY_EPSILON: rc = finite(&p.viscosity_epsilon); break;
    case SPH_P_TENSION_K: rc = finite(&p.tension_k); break;
    default: return fail(h, SPH_E_INVALID, "unknown scalar %d", which);
    }
    if (rc) return rc;
    h->p = p;
    HIP_TRY(h, hipSetDevice(h->device));
    fold_params(h);
    if (dfsph) {          // (the mirror's other words are whatever the last read-back left: only the p_* block is written)
        loop_params(h, h->ds_host);
        HIP_TRY(h, hipMemcpyAsync(&h->ds->p_dens_thr, &h->ds_host->p_dens_thr, sizeof(DevScalars) - offsetof(DevScalars, p_dens_thr), hipMemcpyHostToDevice, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
    }
    mark_stale(h, STALE_LAUNCH_ARGS);                                // (the captured step pairs carry the old constants as launch arguments)
    return SPH_OK;
}

// SPH_P_STEP_*: the adaptive time step of wcsph / pcisph / iisph / pbf handles.  Validated before anything is touched.  Switching it on hands the
// current delta_time (and pcisph's delta) to the device, where they live from then on; switching it off takes back what the last step left there.
// Either way the captured wcsph step pairs hold or lack its two nodes and carry the bounds as launch arguments: they are dropped
static int set_step_param(SphHandle *h, int which, double value)
{
    if (h->cfg.solver == SPH_SOLVER_DFSPH) return fail(h, SPH_E_STATE, "sph_set_scalar(%d): dfsph adapts delta_time through SPH_P_ADAPTIVE_DT / SPH_P_MAX_DT / SPH_P_MIN_DT", which);
    if (h->slab) return fail(h, SPH_E_STATE, "sph_set_scalar(%d): the adaptive time step is not available on a slab handle", which);
    if (which == SPH_P_STEP_ADAPTIVE_DT) {
        if (value != 0.0 && value != 1.0) return fail(h, SPH_E_INVALID, "sph_set_scalar(%d): 0 or 1 expected, got %g", which, value);
    } else if (!(value > 0.0) || !std::isfinite(value))
        return fail(h, SPH_E_INVALID, "sph_set_scalar(%d): a finite value > 0 expected, got %g", which, value);
    HIP_TRY(h, hipSetDevice(h->device));
    if (which == SPH_P_STEP_MAX_DT) h->step_max_dt = value;
    else if (which == SPH_P_STEP_MIN_DT) h->step_min_dt = value;
    else if ((value != 0.0) != h->step_adaptive) {
        if (int rc = read_scalars(h)) return rc;
        if (value != 0.0) {
            h->ds_host->dt = h->dt_wcsph;
            h->ds_host->dt2 = h->ds_host->dt * h->ds_host->dt;
            h->ds_host->pci_delta = h->pci_delta;
            HIP_TRY(h, hipMemcpyAsync(h->ds, h->ds_host, offsetof(DevScalars, ps_dt), hipMemcpyHostToDevice, h->stream));
            HIP_TRY(h, hipMemcpyAsync(&h->ds->pci_delta, &h->ds_host->pci_delta, sizeof(float), hipMemcpyHostToDevice, h->stream));
            HIP_TRY(h, hipStreamSynchronize(h->stream));
        } else {
            if (h->ds_host->dt != h->dt_wcsph) { h->dt_wcsph = h->ds_host->dt; h->cfg.delta_time = (double)h->ds_host->dt; }      // (as write_delta_time)
            if (h->cfg.solver == SPH_SOLVER_PCISPH) h->pci_delta = h->ds_host->pci_delta;        // (SPH_S_PCISPH_BETA stays the attribute of construction, :23)
        }
        h->step_adaptive = value != 0.0;
    }
    mark_stale(h, STALE_LAUNCH_ARGS);
    return SPH_OK;
}

int sph_set_scalar(SphHandle *h, int which, double value)
{
    if (!h) return SPH_E_INVALID;
    if (which >= SPH_P_STEP_ADAPTIVE_DT && which <= SPH_P_STEP_MIN_DT) return set_step_param(h, which, value);
    if (which >= SPH_P_DENSITY_THRESHOLD && which <= SPH_P_TENSION_K) return set_param(h, which, value);      // (on slab handles too: every rank sets the same)
    if (which == SPH_S_TIME) {                                        // the handle's clock; the acceleration vector follows at once
        if (!std::isfinite(value)) return fail(h, SPH_E_INVALID, "sph_set_scalar(SPH_S_TIME): a finite value expected, got %g", value);
        HIP_TRY(h, hipSetDevice(h->device));
        HIP_TRY(h, hipMemcpyAsync(&h->ds->sim_time, &value, sizeof(double), hipMemcpyHostToDevice, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        return forcing_commit(h);
    }
    if (which != SPH_S_DELTA_TIME || !(value > 0.0)) return fail(h, SPH_E_INVALID, "sph_set_scalar: SPH_S_DELTA_TIME > 0, SPH_S_TIME or a solver attribute SPH_P_* can be written");
    HIP_TRY(h, hipSetDevice(h->device));
    return write_delta_time(h, value);                               // (on slab handles too: every rank writes the same)
}

int sph_set_gravity(SphHandle *h, const float g[3])
{
    if (!h) return SPH_E_INVALID;
    if (!g) return fail(h, SPH_E_INVALID, "sph_set_gravity: null argument");
    for (int a = 0; a < 3; ++a)
        if (!std::isfinite(g[a])) return fail(h, SPH_E_INVALID, "sph_set_gravity: finite values expected, got %g on axis %d", (double)g[a], a);
    HIP_TRY(h, hipSetDevice(h->device));
    for (int a = 0; a < 3; ++a) h->frc.g[a] = g[a];
    return forcing_commit(h);
}

int sph_set_forcing(SphHandle *h, const double amp[3], const double omega[3], const double phase[3])
{
    if (!h) return SPH_E_INVALID;
    const double *arg[3] = {amp, omega, phase};
    for (int k = 0; k < 3; ++k)
        for (int a = 0; amp && arg[k] && a < 3; ++a)
            if (!std::isfinite(arg[k][a])) return fail(h, SPH_E_INVALID, "sph_set_forcing: finite values expected, got %g (argument %d, axis %d)", arg[k][a], k, a);
    HIP_TRY(h, hipSetDevice(h->device));
    h->frc.on = 0;
    for (int a = 0; a < 3; ++a) {
        h->frc.amp[a] = amp ? amp[a] : 0.0;
        h->frc.omega[a] = (amp && omega) ? omega[a] : 0.0;
        h->frc.phase[a] = (amp && phase) ? phase[a] : 0.0;
        if (h->frc.amp[a] != 0.0) h->frc.on = 1;                      // all amplitudes zero: a = g, nothing is evaluated
    }
    return forcing_commit(h);
}

// ---- the carried scalar ----------------------------------------------------------------------------------------
int sph_scalar_enable(SphHandle *h, double diffusivity, double beta, double t_ref) { return h ? scalar_enable(h, diffusivity, beta, t_ref) : SPH_E_INVALID; }
int sph_scalar_disable(SphHandle *h) { return h ? scalar_disable(h) : SPH_E_INVALID; }
int sph_scalar_upload(SphHandle *h, const float *values, size_t n)
{
    if (!h) return SPH_E_INVALID;
    if (!values) { if (int rc = scalar_refused(h, "sph_scalar_upload", true)) return rc; return fail(h, SPH_E_INVALID, "sph_scalar_upload: null argument"); }
    return scalar_copy(h, "sph_scalar_upload", nullptr, values, n);
}
int sph_scalar_download(SphHandle *h, float *values, size_t n)
{
    if (!h) return SPH_E_INVALID;
    if (!values) { if (int rc = scalar_refused(h, "sph_scalar_download", true)) return rc; return fail(h, SPH_E_INVALID, "sph_scalar_download: null argument"); }
    return scalar_copy(h, "sph_scalar_download", values, nullptr, n);
}
int sph_scalar_set_inflow(SphHandle *h, double value) { return h ? scalar_set_inflow(h, value) : SPH_E_INVALID; }
int sph_scalar_rate(SphHandle *h, float *out, size_t n) { return h ? scalar_rate_fetch(h, out, n) : SPH_E_INVALID; }

// ---- derived per-particle fields ------------------------------------------------------------------------------
int sph_derived(SphHandle *h, int which, float *host, size_t n_floats)
{
    if (!h) return SPH_E_INVALID;
    return derived_fetch(h, which, host, n_floats);
}

// ---- run diagnostics -----------------------------------------------------------------------------------------
// On demand, between steps: the two launches into the scratch row and one blocking read.  Nothing on the handle changes -- no flag, no buffer
// role, no array a step reads -- so the steps that follow are those of a handle that never called it
int sph_diagnostics(SphHandle *h, SphDiagnostics *out)
{
    if (!h) return SPH_E_INVALID;
    if (!out) return fail(h, SPH_E_INVALID, "sph_diagnostics: null argument");
    if (int rc = diag_refused(h, "sph_diagnostics")) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (int rc = diag_scratch(h)) return rc;
    const float *rho = nullptr;                       // the densities describe the current positions only after sph_compute_density
    if (h->density_valid)
        if (int rc = diag_rho(h, &rho)) return rc;
    launch_diag(h, rho, nullptr, h->diag_row);
    HIP_TRY(h, hipGetLastError());
    static_assert(sizeof(SphDiagnostics) == sizeof(double) * kDiagSlots, "SphDiagnostics is 32 doubles");
    HIP_TRY(h, hipMemcpyAsync(out, h->diag_row, sizeof(SphDiagnostics), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return SPH_OK;
}

// every >= 1: (re)start recording into a fresh ring of `rows` rows, the counters at zero; every == 0: stop (rows is ignored; what the ring holds
// stays readable).  Validated and allocated before anything is touched.  The captured wcsph step pairs hold or lack the two nodes: dropped
int sph_diag_record(SphHandle *h, int every, int rows)
{
    if (!h) return SPH_E_INVALID;
    if (int rc = diag_refused(h, "sph_diag_record")) return rc;
    if (every < 0) return fail(h, SPH_E_INVALID, "sph_diag_record: every >= 0 expected, got %d", every);
    if (every > 0 && (rows < 1 || rows > kDiagMaxRows)) return fail(h, SPH_E_INVALID, "sph_diag_record: 1 <= rows <= %d expected, got %d", kDiagMaxRows, rows);
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (every > 0) {
        if (int rc = diag_scratch(h)) return rc;
        DevMem ring_mem;                   // (neither is zeroed: the counters are written whole, a row is written before it is read)
        double *ring = nullptr;
        ring_mem.want(&ring, kDiagSlots * (size_t)rows);
        HIP_TRY(h, ring_mem.commit(h->stream, false));
        if (!h->own.diag_ctl) {
            h->own.diag_ctl.want(&h->diag_ctl, 1);
            if (h->own.diag_ctl.commit(h->stream, false) != hipSuccess) return fail(h, SPH_E_HIP, "sph_diag_record: out of device memory");
        }
        const DiagCtl ctl{0, 0, h->simulate_cnt, every, rows, 0};
        hipError_t e = hipMemcpyAsync(h->diag_ctl, &ctl, sizeof(ctl), hipMemcpyHostToDevice, h->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
        if (e != hipSuccess) return fail(h, SPH_E_HIP, "sph_diag_record: %s", hipGetErrorString(e));
        h->own.diag_ring = std::move(ring_mem);
        h->diag_ring = ring;
        h->diag_rows = rows;
        h->diag_consumed = 0;
    }
    h->diag_every = every;
    mark_stale(h, STALE_LAUNCH_ARGS);
    return SPH_OK;
}

// the rows still in the ring, oldest first, at most max_rows of them; *total = rows recorded since recording was switched on.  What is handed out
// (and what was overwritten before it could be) is consumed: a second read returns the rows recorded since
int sph_diag_read(SphHandle *h, SphDiagnostics *out, size_t max_rows, size_t *n_rows, int64_t *total)
{
    if (!h) return SPH_E_INVALID;
    if (!n_rows || (!out && max_rows > 0)) return fail(h, SPH_E_INVALID, "sph_diag_read: null argument");
    if (int rc = diag_refused(h, "sph_diag_read")) return rc;
    *n_rows = 0;
    if (total) *total = 0;
    if (!h->diag_ring) return SPH_OK;                  // never recorded
    HIP_TRY(h, hipSetDevice(h->device));
    DiagCtl ctl;
    HIP_TRY(h, hipMemcpyAsync(&ctl, h->diag_ctl, sizeof(ctl), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    const long long rows = h->diag_rows, first = std::max(h->diag_consumed, ctl.count - rows);
    const long long k = std::min<long long>(ctl.count - first, (long long)std::min<size_t>(max_rows, (size_t)rows));
    for (long long done = 0; done < k;) {              // at most two runs of slots
        const long long slot = (first + done) % rows, run = std::min(k - done, rows - slot);
        HIP_TRY(h, hipMemcpyAsync(out + done, h->diag_ring + slot * kDiagSlots, sizeof(SphDiagnostics) * (size_t)run, hipMemcpyDeviceToHost, h->stream));
        done += run;
    }
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    h->diag_consumed = first + k;
    *n_rows = (size_t)k;
    if (total) *total = ctl.count;
    return SPH_OK;
}

const char *sph_overrides(SphHandle *h) { return h ? h->overrides.c_str() : ""; }

int sph_synchronize(SphHandle *h)
{
    if (!h) return SPH_E_INVALID;
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return SPH_OK;
}

int sph_profile_enable(SphHandle *h, int on)
{
    if (!h) return SPH_E_INVALID;
    drain_profile(h);
    h->profiling = on != 0;
    return SPH_OK;
}

int sph_profile_reset(SphHandle *h)
{
    if (!h) return SPH_E_INVALID;
    drain_profile(h);
    for (int k = 0; k < K_COUNT; ++k) { h->prof_ms[k] = 0; h->prof_n[k] = 0; }
    return SPH_OK;
}

int sph_profile_kernel_count(void) { return K_COUNT; }
const char *sph_profile_kernel_name(int kid) { return (kid >= 0 && kid < K_COUNT) ? kKernelNames[kid] : ""; }

int sph_profile_get(SphHandle *h, int kid, double *total_ms, int64_t *launches)
{
    if (!h || kid < 0 || kid >= K_COUNT) return SPH_E_INVALID;
    drain_profile(h);
    if (total_ms) *total_ms = h->prof_ms[kid];
    if (launches) *launches = h->prof_n[kid];
    return SPH_OK;
}

// Tuning aid (not part of the reference's surface): mean duration in microseconds of `reps` back-to-back launches of one DFSPH sweep
// on the handle's current state with `lds_bytes` of dynamic LDS, bracketed by one HIP event pair.  `which` and what each value leaves behind on
// the handle: include/sph_mi355x.h (0, 2, 3 and any value outside 0 .. 7, which runs 3's sort + list build, change no trajectory; 1 and 4 .. 7 are
// for throw-away handles).
int sph_tune_time(SphHandle *h, int which, unsigned lds_bytes, int reps, double *avg_us)
{
    if (!h || !avg_us || reps < 1) return SPH_E_INVALID;
    if (h->cfg.solver != SPH_SOLVER_DFSPH || h->slab) return fail(h, SPH_E_STATE, "sph_tune_time needs a single-GPU dfsph handle");
    HIP_TRY(h, hipSetDevice(h->device));
    int rc;
    if (!h->nl_valid && (rc = stage_sort_and_lists(h))) return rc;
    if (!h->density_valid && (rc = stage_density(h))) return rc;
    const unsigned saved = h->sweep_lds;
    h->sweep_lds = lds_bytes;
    h->tune_all = true;                    // repeated launches on one state: every tile computes (no change propagation)
    hipEvent_t a, b;
    HIP_TRY(h, hipEventCreate(&a));
    HIP_TRY(h, hipEventCreate(&b));
    HIP_TRY(h, hipEventRecord(a, h->stream));
    for (int k = 0; k < reps; ++k) {
        if (which == 0) launch_div_residual(h, GATE_NONE);
        else if (which == 1) launch_correct<CORR_DIV>(h, K_D_DIV_CORRECT, h->drho, h->V[h->vcur], GATE_NONE);
        else if (which == 2) launch_dens_residual(h, GATE_NONE);
        else if (which == 4) {      // a sweep followed by the single-workgroup reduction of its block partials, as in the solver loops
            launch_div_residual(h, GATE_NONE);
            hipLaunchKernelGGL(k_finalize_mean, dim3(1), dim3(kFinBlock), 0, h->stream, h->psum, h->pcnt, h->nblocks, h->ds, (int)FIN_PLAIN, (int)FINP_ALL, (double *)nullptr, partial_group(h), partial_count(h));
        } else if (which == 5) {    // the reduction alone
            hipLaunchKernelGGL(k_finalize_mean, dim3(1), dim3(kFinBlock), 0, h->stream, h->psum, h->pcnt, h->nblocks, h->ds, (int)FIN_PLAIN, (int)FINP_ALL, (double *)nullptr, partial_group(h), partial_count(h));
        } else if (which == 6) {    // two different sweeps alternating (residual, correct), no reduction between them
            launch_div_residual(h, GATE_NONE);
            launch_correct<CORR_DIV>(h, K_D_DIV_CORRECT, h->drho, h->V[h->vcur], GATE_NONE);
        } else if (which == 7) {    // the same with the reduction after the residual: one solver iteration
            launch_div_residual(h, GATE_NONE);
            hipLaunchKernelGGL(k_finalize_mean, dim3(1), dim3(kFinBlock), 0, h->stream, h->psum, h->pcnt, h->nblocks, h->ds, (int)FIN_PLAIN, (int)FINP_ALL, (double *)nullptr, partial_group(h), partial_count(h));
            launch_correct<CORR_DIV>(h, K_D_DIV_CORRECT, h->drho, h->V[h->vcur], GATE_NONE);
        }
        else if ((rc = stage_sort_and_lists(h))) break;
    }
    HIP_TRY(h, hipEventRecord(b, h->stream));
    HIP_TRY(h, hipEventSynchronize(b));
    float ms = 0.f;
    HIP_TRY(h, hipEventElapsedTime(&ms, a, b));
    (void)hipEventDestroy(a); (void)hipEventDestroy(b);
    h->sweep_lds = saved;
    h->tune_all = false;
    if (which == 3) mark_stale(h, STALE_DENSITY);
    *avg_us = (double)ms * 1000.0 / reps;
    return SPH_OK;
}

int sph_selftest_math(int device, int op, const float *a, const float *b, float *out, size_t n)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(nullptr, SPH_E_NO_DEVICE, "no HIP device available");
    if (device < 0 || device >= ndev || !a || !b || !out) return fail(nullptr, SPH_E_INVALID, "bad argument");
    if (hipSetDevice(device) != hipSuccess) return fail(nullptr, SPH_E_HIP, "hipSetDevice failed");
    float *da = nullptr, *db = nullptr, *dout = nullptr;
    DevMem mem;                            // (the self-tests' scratch: not zeroed, on the null stream, gone with the call)
    mem.want(&da, n); mem.want(&db, n); mem.want(&dout, n);
    int rc = SPH_OK;
    if (mem.commit(nullptr, false) != hipSuccess) rc = fail(nullptr, SPH_E_HIP, "hipMalloc failed");
    if (!rc) {
        (void)hipMemcpy(da, a, n * 4, hipMemcpyHostToDevice);
        (void)hipMemcpy(db, b, n * 4, hipMemcpyHostToDevice);
        Consts c;
        memset(&c, 0, sizeof(c));
        c.h = 0.1f;
        const float pi_f = (float)3.141592653589793;
        const float h3 = c.h * (c.h * c.h);
        c.kw = 8.0f / (pi_f * h3);
        c.rh = 1.0f / c.h;
        const float kg = 48.0f / (pi_f * h3);
        c.kg6 = kg * 6.0f; c.neg_kg6 = -kg * 6.0f;
        hipLaunchKernelGGL(k_selftest, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, c, op, da, db, dout, n);
        if (hipDeviceSynchronize() != hipSuccess) rc = fail(nullptr, SPH_E_HIP, "selftest kernel failed");
        else (void)hipMemcpy(out, dout, n * 4, hipMemcpyDeviceToHost);
    }
    return rc;
}

int sph_selftest_wave(int device, int op, const double *in, double *out, size_t n)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(nullptr, SPH_E_NO_DEVICE, "no HIP device available");
    if (device < 0 || device >= ndev || !in || !out || n == 0 || n % 256 != 0 || op < 0 || op > 4) return fail(nullptr, SPH_E_INVALID, "bad argument (n must be a multiple of 256)");
    if (hipSetDevice(device) != hipSuccess) return fail(nullptr, SPH_E_HIP, "hipSetDevice failed");
    double *din = nullptr, *dout = nullptr;
    DevMem mem;
    mem.want(&din, n); mem.want(&dout, n);
    int rc = SPH_OK;
    if (mem.commit(nullptr, false) != hipSuccess) rc = fail(nullptr, SPH_E_HIP, "hipMalloc failed");
    if (!rc) {
        (void)hipMemcpy(din, in, n * 8, hipMemcpyHostToDevice);
        hipLaunchKernelGGL(k_selftest_wave, dim3((unsigned)(n / 256)), dim3(256), 0, 0, op, din, dout);
        if (hipDeviceSynchronize() != hipSuccess) rc = fail(nullptr, SPH_E_HIP, "selftest kernel failed");
        else (void)hipMemcpy(out, dout, n * 8, hipMemcpyDeviceToHost);
    }
    return rc;
}

int sph_selftest_stage(SphHandle *h, int layout, int check, int empty_idle, int use_pre, int not_staged, const uint32_t *runs, int nruns,
                       const float *A, const float *B, const float *S, const unsigned char *changed, size_t n_src, float *out, int *verdict)
{
    int ndev = 0;
    const int device = h ? h->device : 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(h, SPH_E_NO_DEVICE, "no HIP device available");
    if (layout < 0 || layout > 7 || check < 0 || check > 2 || nruns < 0 || nruns > kStageMaxCells || (nruns && !runs) ||
        !A || !B || !S || !changed || n_src == 0 || !out || !verdict)
        return fail(h, SPH_E_INVALID, "bad argument");
    // the plan as k_build_nl writes it: (first, local base | count << 16) per run, particles | runs << 16 for the workgroup
    std::vector<uint2> plan(kStageMaxCells, make_uint2(0u, 0u));
    size_t nst = 0;
    for (int r = 0; r < nruns; ++r) {
        const uint32_t first = runs[2 * r], n = runs[2 * r + 1];
        if (n > 0xffffu || (size_t)first + n > n_src || nst + n > (size_t)kStageCapMax) return fail(h, SPH_E_INVALID, "a run leaves the source arrays or the staged set the capacity");
        plan[r] = make_uint2(first, (uint32_t)nst | (n << 16));
        nst += n;
    }
    const int cnt = not_staged ? -1 : (int)nst | (nruns << 16);
    if (hipSetDevice(device) != hipSuccess) return fail(h, SPH_E_HIP, "hipSetDevice failed");
    const size_t out_bytes = (size_t)6 * kStageCapMax * sizeof(float);
    uint2 *d_runs = nullptr; int *d_cnt = nullptr; float4 *d_A = nullptr, *d_B = nullptr; float *d_S = nullptr, *d_out = nullptr; unsigned char *d_ch = nullptr;
    DevMem mem;
    mem.want(&d_runs, plan.size()); mem.want(&d_cnt, 2); mem.want(&d_A, n_src); mem.want(&d_B, n_src); mem.want(&d_S, n_src); mem.want(&d_ch, n_src);
    mem.want(&d_out, out_bytes / sizeof(float));
    int rc = SPH_OK;
    if (mem.commit(nullptr, false) != hipSuccess) rc = fail(h, SPH_E_HIP, "hipMalloc failed");
    if (!rc) {
        const int head[2] = {cnt, -1};                         // [1]: the verdict
        (void)hipMemcpy(d_runs, plan.data(), plan.size() * sizeof(uint2), hipMemcpyHostToDevice);
        (void)hipMemcpy(d_cnt, head, sizeof(head), hipMemcpyHostToDevice);
        (void)hipMemcpy(d_A, A, n_src * 16, hipMemcpyHostToDevice);
        (void)hipMemcpy(d_B, B, n_src * 16, hipMemcpyHostToDevice);
        (void)hipMemcpy(d_S, S, n_src * 4, hipMemcpyHostToDevice);
        (void)hipMemcpy(d_ch, changed, n_src, hipMemcpyHostToDevice);
        (void)hipMemset(d_out, 0, out_bytes);
        const size_t lds = (size_t)kStageCapMax * StagePV<>::kBytes;      // the largest layout
        auto launch = [&](auto empty) {
            constexpr StageVerdict EMPTY = decltype(empty)::value;
            if (check == 0) hipLaunchKernelGGL((k_selftest_stage<kCheckNone, EMPTY>), dim3(1), dim3(kBlock), lds, 0, layout, use_pre, d_runs, d_cnt, d_A, d_B, d_S, d_ch, d_out, d_cnt + 1);
            else if (check == 1) hipLaunchKernelGGL((k_selftest_stage<kCheckWith, EMPTY>), dim3(1), dim3(kBlock), lds, 0, layout, use_pre, d_runs, d_cnt, d_A, d_B, d_S, d_ch, d_out, d_cnt + 1);
            else hipLaunchKernelGGL((k_selftest_stage<kCheckFirst, EMPTY>), dim3(1), dim3(kBlock), lds, 0, layout, use_pre, d_runs, d_cnt, d_A, d_B, d_S, d_ch, d_out, d_cnt + 1);
        };
        if (empty_idle) launch(std::integral_constant<StageVerdict, kStagedIdle>{});
        else launch(std::integral_constant<StageVerdict, kStaged>{});
        if (hipDeviceSynchronize() != hipSuccess) rc = fail(h, SPH_E_HIP, "selftest kernel failed");
        else {
            (void)hipMemcpy(out, d_out, out_bytes, hipMemcpyDeviceToHost);
            (void)hipMemcpy(verdict, d_cnt + 1, sizeof(int), hipMemcpyDeviceToHost);
        }
    }
    return rc;
}

int sph_selftest_walk(SphHandle *h, int walk, int src, int rigid, const uint32_t *lists, const int *counts, uint32_t run_first, uint32_t run_n,
                      const float *A, const float *B, const float *C, const float *S, size_t n_src, const float *RP, size_t n_rig, uint32_t *out)
{
    int ndev = 0;
    const int device = h ? h->device : 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(h, SPH_E_NO_DEVICE, "no HIP device available");
    constexpr int NP = kWalkTestParticles, ROWS = kWalkTestRows, PITCH = kWalkTestPitch;
    const bool lds = walk >= 2, half = walk == 3;
    if (walk < 0 || walk > 3 || src < 0 || src > (lds ? 8 : 4) || (rigid && (half || (!lds && src == 0))) || !lists || !counts || !A || !B || !C || !S ||
        !RP || n_src == 0 || n_rig == 0 || !out || run_n == 0 || run_n > (uint32_t)kWalkTestCap || (size_t)run_first + run_n > n_src)
        return fail(h, SPH_E_INVALID, "bad argument");
    // the lists as k_build_nl lays them out (nl_index; 16-bit: entry 2q in the low, 2q + 1 in the high half of word q of a group, NlWriter), one
    // zeroed spare tile behind them.  Every entry a walk can fetch must be a valid index, the slots past a count and the spare group included
    std::vector<uint32_t> nl((size_t)(NP / 64 + 1) * PITCH * 64, 0u);
    for (int i = 0; i < NP; ++i) {
        if (counts[i] < 0 || counts[i] > ROWS) return fail(h, SPH_E_INVALID, "a count leaves 0 .. 24");
        for (int k = 0; k < (half ? ROWS : PITCH); ++k) {
            const uint32_t j = lists[(size_t)i * PITCH + k];
            const bool rg = (j & kRigidTag) != 0;
            if (rg ? (!rigid || (j & ~kRigidTag) >= n_rig) : j >= (lds ? (size_t)run_n : n_src)) return fail(h, SPH_E_INVALID, "a list entry leaves its array");
            if (half) nl[nl_index(i, 4 * (k >> 3) + ((k & 7) >> 1), PITCH)] |= j << (16 * (k & 1));
            else nl[nl_index(i, k, PITCH)] = j;
        }
    }
    std::vector<uint2> plan(kStageMaxCells, make_uint2(0u, 0u));
    plan[0] = make_uint2(run_first, run_n << 16);
    const int head = (int)run_n | (1 << 16);
    const int nthreads = walk == 1 ? 4 * NP : NP;
    if (hipSetDevice(device) != hipSuccess) return fail(h, SPH_E_HIP, "hipSetDevice failed");
    uint2 *d_runs = nullptr; int *d_head = nullptr, *d_cnt = nullptr; float4 *d_A = nullptr, *d_B = nullptr, *d_C = nullptr, *d_RP = nullptr; float *d_S = nullptr;
    uint32_t *d_nl = nullptr, *d_out = nullptr;
    DevMem mem;
    mem.want(&d_runs, plan.size()); mem.want(&d_head, 1); mem.want(&d_cnt, NP); mem.want(&d_A, n_src); mem.want(&d_B, n_src); mem.want(&d_C, n_src); mem.want(&d_S, n_src);
    mem.want(&d_RP, n_rig); mem.want(&d_nl, nl.size()); mem.want(&d_out, (size_t)nthreads * 4);
    int rc = SPH_OK;
    if (mem.commit(nullptr, false) != hipSuccess) rc = fail(h, SPH_E_HIP, "hipMalloc failed");
    if (!rc) {
        (void)hipMemcpy(d_runs, plan.data(), plan.size() * sizeof(uint2), hipMemcpyHostToDevice);
        (void)hipMemcpy(d_head, &head, sizeof(int), hipMemcpyHostToDevice);
        (void)hipMemcpy(d_cnt, counts, NP * sizeof(int), hipMemcpyHostToDevice);
        (void)hipMemcpy(d_A, A, n_src * 16, hipMemcpyHostToDevice);
        (void)hipMemcpy(d_B, B, n_src * 16, hipMemcpyHostToDevice);
        (void)hipMemcpy(d_C, C, n_src * 16, hipMemcpyHostToDevice);
        (void)hipMemcpy(d_S, S, n_src * 4, hipMemcpyHostToDevice);
        (void)hipMemcpy(d_RP, RP, n_rig * 16, hipMemcpyHostToDevice);
        (void)hipMemcpy(d_nl, nl.data(), nl.size() * 4, hipMemcpyHostToDevice);
        (void)hipMemset(d_out, 0, (size_t)nthreads * 16);
        RigidView rv{};
        rv.RP = d_RP;
        const size_t smem = (size_t)kWalkTestCap * 32;            // the largest set: StageUpdateP
        const dim3 grid((unsigned)(nthreads / kBlock)), block(kBlock);
        auto launch = [&](auto rg) {
            constexpr bool RG = decltype(rg)::value;
            if (walk == 0) hipLaunchKernelGGL((k_selftest_walk<0, RG>), grid, block, smem, 0, src, d_runs, d_head, d_A, d_B, d_C, d_S, rv, d_nl, d_cnt, d_out);
            else if (walk == 1) hipLaunchKernelGGL((k_selftest_walk<1, RG>), grid, block, smem, 0, src, d_runs, d_head, d_A, d_B, d_C, d_S, rv, d_nl, d_cnt, d_out);
            else if (walk == 2) hipLaunchKernelGGL((k_selftest_walk<2, RG>), grid, block, smem, 0, src, d_runs, d_head, d_A, d_B, d_C, d_S, rv, d_nl, d_cnt, d_out);
        };
        if (walk == 3) hipLaunchKernelGGL((k_selftest_walk<3, false>), grid, block, smem, 0, src, d_runs, d_head, d_A, d_B, d_C, d_S, rv, d_nl, d_cnt, d_out);
        else if (rigid) launch(std::true_type{});
        else launch(std::false_type{});
        if (hipDeviceSynchronize() != hipSuccess) rc = fail(h, SPH_E_HIP, "selftest kernel failed");
        else (void)hipMemcpy(out, d_out, (size_t)nthreads * 16, hipMemcpyDeviceToHost);
    }
    return rc;
}

// walk_list16 with the pair-bit stream, on one workgroup of kWalkTestParticles threads: lists (NP x 24 entries < NP), counts (0 .. 24), words (NP x 3: the
// word of every group of eight, read when write == 0 and returned when write != 0), verdicts (NP x 24: what body k records when write != 0); seen
// (NP x 24) and calls (NP) are what the bodies report (k_selftest_walk_bits)
int sph_selftest_walk_bits(SphHandle *h, int write, const uint32_t *lists, const int *counts, uint32_t *words, const int *verdicts, uint32_t *seen, int *calls)
{
    int ndev = 0;
    const int device = h ? h->device : 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(nullptr, SPH_E_NO_DEVICE, "no HIP device available");
    constexpr int NP = kWalkTestParticles, ROWS = kWalkTestRows, PITCH = kWalkTestPitch, GROUPS = ROWS / 8;
    if (device < 0 || device >= ndev || !lists || !counts || !words || !verdicts || !seen || !calls) return fail(nullptr, SPH_E_INVALID, "bad argument");
    std::vector<uint32_t> nl((size_t)(NP / 64 + 1) * PITCH * 64, 0u), bits(nl.size() / 4, 0u);
    std::vector<float4> A(NP);
    for (int i = 0; i < NP; ++i) {
        A[i] = make_float4((float)i, 0.f, 0.f, 0.f);
        if (counts[i] < 0 || counts[i] > ROWS) return fail(nullptr, SPH_E_INVALID, "a count leaves 0 .. 24");
        for (int k = 0; k < ROWS; ++k) {
            const uint32_t j = lists[(size_t)i * ROWS + k];
            if (j >= (uint32_t)NP) return fail(nullptr, SPH_E_INVALID, "a list entry leaves its array");
            nl[nl_index(i, 4 * (k >> 3) + ((k & 7) >> 1), PITCH)] |= j << (16 * (k & 1));
        }
        for (int g = 0; g < GROUPS; ++g) bits[(nl_index(i, 0, PITCH) >> 2) + (size_t)g * 64] = write ? 0xffffffffu : words[(size_t)i * GROUPS + g];
    }
    if (hipSetDevice(device) != hipSuccess) return fail(nullptr, SPH_E_HIP, "hipSetDevice failed");
    float4 *d_A = nullptr; uint32_t *d_nl = nullptr, *d_bits = nullptr, *d_seen = nullptr; int *d_cnt = nullptr, *d_verdict = nullptr, *d_calls = nullptr;
    DevMem mem;
    mem.want(&d_A, NP); mem.want(&d_nl, nl.size()); mem.want(&d_bits, bits.size()); mem.want(&d_seen, (size_t)NP * ROWS); mem.want(&d_cnt, NP);
    mem.want(&d_verdict, (size_t)NP * ROWS); mem.want(&d_calls, NP);
    int rc = SPH_OK;
    if (mem.commit(nullptr, false) != hipSuccess) rc = fail(nullptr, SPH_E_HIP, "hipMalloc failed");
    if (!rc) {
        (void)hipMemcpy(d_A, A.data(), NP * 16, hipMemcpyHostToDevice);
        (void)hipMemcpy(d_nl, nl.data(), nl.size() * 4, hipMemcpyHostToDevice);
        (void)hipMemcpy(d_bits, bits.data(), bits.size() * 4, hipMemcpyHostToDevice);
        (void)hipMemcpy(d_cnt, counts, NP * 4, hipMemcpyHostToDevice);
        (void)hipMemcpy(d_verdict, verdicts, (size_t)NP * ROWS * 4, hipMemcpyHostToDevice);
        (void)hipMemset(d_seen, 0xff, (size_t)NP * ROWS * 4);
        hipLaunchKernelGGL(k_selftest_walk_bits, dim3(1), dim3(kBlock), 0, 0, write, d_A, d_nl, d_cnt, d_bits, d_verdict, d_seen, d_calls);
        if (hipDeviceSynchronize() != hipSuccess) rc = fail(nullptr, SPH_E_HIP, "selftest kernel failed");
        else {
            (void)hipMemcpy(seen, d_seen, (size_t)NP * ROWS * 4, hipMemcpyDeviceToHost);
            (void)hipMemcpy(calls, d_calls, NP * 4, hipMemcpyDeviceToHost);
            (void)hipMemcpy(bits.data(), d_bits, bits.size() * 4, hipMemcpyDeviceToHost);
            for (int i = 0; i < NP; ++i)
                for (int g = 0; g < GROUPS; ++g) words[(size_t)i * GROUPS + g] = bits[(nl_index(i, 0, PITCH) >> 2) + (size_t)g * 64];
        }
    }
    return rc;
}

}  // extern "C"
