// sph_pbf_kernels.h -- PBF (pbf_solver.py) on the cell-sorted arrays and per-step neighbour lists of sph_kernels.h.
//
// pbf_solver.py is stale at the surveyed commit (its fluid callbacks still index particle fields with what for_all_neighbor now passes
// as particle structs, ParticleSystem.py:468-469); it is read the way the other solvers' callbacks were updated (callback argument
// -> the struct's pos / vel / index).  update_all_pos (:66-95) races on pos and vel; the kernels follow the barrier-synchronised
// schedule (every particle's own writes, then every particle's neighbour reads, then the viscosity update), which is one legal
// execution of the reference loop and the one both CPU restatements of the tests follow: the C restatement under oracle/ (its step_pbf) and the
// independently written tests/second_restatement_pbf.py, whose docstring numbers the reading as conventions 1-6; the quad and plain
// instantiations below are held to the second one on linear and on Morton cells (tests/test_second_restatement_gpu.py).  No rigid
// coupling (the callbacks have none).
//
// Three sweeps per step:
//   k_pbf_lambda   rho (poly6), constrain, constrain_derivative, lambda           :32-52, 108-140   (the reference: five walks)
//   k_pbf_delta    delta_pos; externel_force_predict_pos; update_all_pos phase 1   :26-29, 55-64, 66-84
//   k_pbf_xsph     v_i = sum_j (vel_j - vel_i) W(|x_i - x_j|) on the NEW positions through the cell lists of the step's start; vel += c v   :86-98
//
// RX (SphConfig.arith = SPH_ARITH_RELAXED, relaxed_pbf() in sph_host_rigid.h): the tolerance-grade pair bodies.  Same pairs, lists, cell walk and
// buffers; only the pair arithmetic changes.  r2 = fma(z,z, fma(y,y, fma(x,x, 1e-30))); poly6 is a polynomial in r2 -- tp = max(1 - r2 / h^2, 0),
// W = kpoly tp^3, no root, no divide; the spiky gradient is one scalar times x_ij -- rinv = v_rsq_f32(r2), r = r2 rinv, ts = max(1 - r / h, 0),
// grad W = K ts^2 rinv x_ij with K = -45 / (pi h^4).  Every constant factor of a sum is taken out of it and applied once per particle (PbfConsts.rx_*,
// folded in f64 on the host): the sweeps add tp^3, ts^2 rinv x_ij and (ts^2 rinv)^2 r2, and s_corr = -k (W / w_corr)^4 is rx_sc tp^12.
// A coincident pair (x_ij = 0 exactly; r2 is its floor, the scalar s = ts^2 rinv is 1e15, finite) contributes, as in the reference:
//   tp^3 = 1 to the poly6 sums (rho, the wall's rb, s_corr, xsph's W = kpoly: poly6 has no gate at q = 0);
//   s x_ij = 0 to the three vector sums of k_pbf_lambda and k_pbf_delta -- the reference's q > 0 gate gives the same 0, so they carry no gate;
//   0 to the SCALAR sum of squared gradients of k_pbf_lambda (sum, sb): pbf_sq_rx selects it on x_ij == 0.  Ungated the term is s^2 r2 = 1,
//   after the epilogue (K / rho0)^2 -- the limit r -> 0+, the largest term a pair can give, where the reference's gate gives 0.
// Any pair with x_ij != 0 takes the ungated term, bit for bit what it was before the select existed.  k_pbf_xsph decides membership by r2 <= r2_cut
// (Consts: the f32 image of r <= h) and never takes a root.  What stays exact: the per-particle epilogues that set the discrete outcomes --
// the constraint and its max, lambda's `con == 0` branch and divide, the prediction, vel = (pp - pos) / dt, the clamp planes, vel += c v.  The wall
// walk of k_pbf_delta is kept (the regrouping lambda_i G_i + T_i through k_pbf_lambda was not built).  tests/test_pbf_relaxed_gpu.py holds the RX
// instantiations to 4 x the f32 oracle's own error against the f64 oracle; RX = false is the exact code as it was before the argument
// existed (same registers: profiles/r09/pbf_relaxed/kernel_resources.txt; same bits: tests/test_pbf_gpu.py).
#pragma once
#include "sph_kernels.h"

namespace sph {

struct PbfConsts {
    float kpoly;      // 315 / (64 pi h^3)                      solver_base.py:128
    float pih4;       // pi * h^4                               solver_base.py:120
    float w_corr;     // poly_kernel(s_corr_factor * kernel_h)  pbf_solver.py:148
    float neg_k;      // -k (tension)                           :151
    float c_visc;     // c                                      :92
    float eps;        // epsilon                                :17
    float lo[3], hi[3];   // clamp walls at particle_radius     :74-81
    // the RX pair bodies (folded in f64, pbf_consts)
    float rx_rh2;         // 1 / h^2
    float rx_mk;          // m kpoly: rho = 0.001 + rx_mk sum tp^3
    float rx_kg;          // -45 / (pi h^4): k_pbf_delta's sums, divided by rho0 once as in the exact epilogue
    float rx_kg_rho0;     // -45 / (pi h^4 rho0): the sums of k_pbf_lambda
    float rx_sc;          // -k (kpoly / w_corr)^4: s_corr = rx_sc tp^12
    float rx_ck;          // c kpoly: vel += rx_ck sum (vel_j - vel_i) tp^3
};

// the RX pair: squared distance with its floor, the poly6 base tp and the spiky scalar s = ts^2 / r (see the header)
struct PbfPairRx { float r2, tp, s; };
__device__ __forceinline__ float pbf_r2_rx(float dx, float dy, float dz) { return __builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, __builtin_fmaf(dx, dx, 1e-30f))); }
__device__ __forceinline__ float pbf_tp_rx(const PbfConsts &k, float r2) { return __builtin_fmaxf(__builtin_fmaf(-r2, k.rx_rh2, 1.0f), 0.0f); }
__device__ __forceinline__ PbfPairRx pbf_pair_rx(const Consts &c, const PbfConsts &k, float dx, float dy, float dz)
{
    PbfPairRx o;
    o.r2 = pbf_r2_rx(dx, dy, dz);
    const float rinv = __builtin_amdgcn_rsqf(o.r2), r = o.r2 * rinv;
    o.tp = pbf_tp_rx(k, o.r2);
    const float ts = __builtin_fmaxf(__builtin_fmaf(-r, c.rh, 1.0f), 0.0f);
    o.s = (ts * ts) * rinv;
    return o;
}

// the pair's term of k_pbf_lambda's sum of squared gradients: (ts^2 / r)^2 r2, and 0 for a coincident pair (the reference's q > 0 gate)
__device__ __forceinline__ float pbf_sq_rx(const PbfPairRx &p, float dx, float dy, float dz)
{
    const bool apart = __builtin_fmaxf(__builtin_fmaxf(__builtin_fabsf(dx), __builtin_fabsf(dy)), __builtin_fabsf(dz)) > 0.0f;
    return apart ? p.s * p.s : 0.0f;
}

__device__ __forceinline__ float pow3f(float a) { return a * (a * a); }
__device__ __forceinline__ float poly_w(const Consts &c, const PbfConsts &k, float r)       // solver_base.py:123-129
{
    const float q = div_by_h(c, r);
    const float q2 = q * q;
    const float w = k.kpoly * pow3f(1.0f - q2);
    return q <= 1.0f ? w : 0.0f;
}
__device__ __forceinline__ F3 spiky_grad(const Consts &c, const PbfConsts &k, float dx, float dy, float dz, float r)   // solver_base.py:114-121
{
    const float q = div_by_h(c, r);
    const float t = 1.0f - q;
    const float a = -(45.0f * (t * t));
    const float den = k.pih4 * r;
    const bool in = q <= 1.0f && q > 0.0f;
    F3 o;
    o.x = in ? (a * dx) / den : 0.0f; o.y = in ? (a * dy) / den : 0.0f; o.z = in ? (a * dz) / den : 0.0f;
    return o;
}

// QSUM (x-slab handles under RX, one lane per particle): the additions of the quad walk.  walk_list_quad forms every entry's terms in ZEROED
// accumulators and then adds them in list order; under RX the pair bodies accumulate with fma, so a QUAD handle rounds fma(a, b, 0) and then the
// sum where the plain walk rounds fma(a, b, acc) once -- other bits.  A slab handle runs one lane per particle whatever the scene's size, and must
// give what the one-GPU handle of the same scene gives: where that handle walks quad-wide (pbf_qsum(), sph_host_dfsph.h) the slabs take this
// walk.  The exact bodies round every product and sum separately: QUAD and plain agree there, and QSUM is never instantiated.
// (a functor, not a lambda in the sweep: the kernels' own closures keep their places, and the instantiations without QSUM stay the code they were)
template <int N, class Body>
struct PbfQuadSum {
    float (&acc)[N];
    Body &body;
    __device__ __forceinline__ void operator()(const float4 pj) const
    {
        float save[N];
#pragma unroll
        for (int n = 0; n < N; ++n) { save[n] = acc[n]; acc[n] = 0.0f; }
        body(pj);
#pragma unroll
        for (int n = 0; n < N; ++n) acc[n] = save[n] + acc[n];
    }
};
template <int N, class Body> __device__ __forceinline__ PbfQuadSum<N, Body> pbf_quad_sum(float (&acc)[N], Body &body) { return PbfQuadSum<N, Body>{acc, body}; }

// rho, constrain, constrain_derivative, lambda.  Pout = (pos, lambda) for the gather of k_pbf_delta.
// QUAD (both list sweeps): four lanes per particle, small scenes (walk_list_quad, sph_kernels.h)
template <bool QUAD, bool RX = false, bool QSUM = false>
__global__ __launch_bounds__(kBlock) void k_pbf_lambda(Consts c, PbfConsts k, const float4 *__restrict__ P, const float4 *__restrict__ WP,
                                                       const uint32_t *__restrict__ nl, const uint32_t *__restrict__ nlb,
                                                       const int *__restrict__ cnt, float *__restrict__ rho_out, float *__restrict__ lambda_out,
                                                       float4 *__restrict__ Pout, int rho_only)
{
    SPH_SWEEP_PROLOGUE_M(QUAD)
    float fa[5] = {RX ? 0.f : 0.001f, 0.f, 0.f, 0.f, 0.f};        // rho starts at 0.001, solver_base.py:44 (RX: added in the epilogue)
    float &rho = fa[0], &cx = fa[1], &cy = fa[2], &cz = fa[3], &sum = fa[4];
    auto pair = [&](const float4 pj) {
        const float dx = pi.x - pj.x, dy = pi.y - pj.y, dz = pi.z - pj.z;
        if constexpr (RX) {
            const PbfPairRx p = pbf_pair_rx(c, k, dx, dy, dz);
            rho = __builtin_fmaf(p.tp * p.tp, p.tp, rho);
            cx = __builtin_fmaf(p.s, dx, cx); cy = __builtin_fmaf(p.s, dy, cy); cz = __builtin_fmaf(p.s, dz, cz);
            sum = __builtin_fmaf(pbf_sq_rx(p, dx, dy, dz), p.r2, sum);
            return;
        }
        const float r = norm3(dx, dy, dz);
        rho += c.m * poly_w(c, k, r);                              // :169-170
        const F3 g = spiky_grad(c, k, dx, dy, dz, r);
        const float gx = g.x / c.rho0, gy = g.y / c.rho0, gz = g.z / c.rho0;
        cx += gx; cy += gy; cz += gz;                              // :116-117
        sum += (gx * gx + gy * gy) + gz * gz;                      // :133-134
    };
    if (QUAD) sweep_quad<false>(SrcP{P}, nlp, kf, q, fa, pair);
    else if constexpr (QSUM) sweep_list<false>(SrcP{P}, nlp, kf, pbf_quad_sum(fa, pair));
    else sweep_list<false>(SrcP{P}, nlp, kf, pair);
    float wa[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    float &rb = wa[0], &bx = wa[1], &by = wa[2], &bz = wa[3], &sb = wa[4];
    auto wall = [&](const float4 pj) {
        const float dx = pi.x - pj.x, dy = pi.y - pj.y, dz = pi.z - pj.z;
        if constexpr (RX) {
            const PbfPairRx p = pbf_pair_rx(c, k, dx, dy, dz);
            rb = __builtin_fmaf(pj.w * (p.tp * p.tp), p.tp, rb);
            bx = __builtin_fmaf(p.s, dx, bx); by = __builtin_fmaf(p.s, dy, by); bz = __builtin_fmaf(p.s, dz, bz);
            sb = __builtin_fmaf(pbf_sq_rx(p, dx, dy, dz), p.r2, sb);
            return;
        }
        const float r = norm3(dx, dy, dz);
        rb += pj.w * poly_w(c, k, r);                              // :173-176
        const F3 g = spiky_grad(c, k, dx, dy, dz, r);
        const float gx = g.x / c.rho0, gy = g.y / c.rho0, gz = g.z / c.rho0;
        bx += gx; by += gy; bz += gz;                              // :120-122
        sb += (gx * gx + gy * gy) + gz * gz;                       // :139-140
    };
    if (QUAD) sweep_quad<false>(SrcP{WP}, nlbp, kb, q, wa, wall);
    else if constexpr (QSUM) sweep_list<false>(SrcP{WP}, nlbp, kb, pbf_quad_sum(wa, wall));
    else sweep_list<false>(SrcP{WP}, nlbp, kb, wall);
    if (!owner) return;
    if constexpr (RX) {                                            // the constant factors of the sums, once
        rho = __builtin_fmaf(k.rx_mk, rho, 0.001f); rb *= k.kpoly;
        cx *= k.rx_kg_rho0; cy *= k.rx_kg_rho0; cz *= k.rx_kg_rho0; bx *= k.rx_kg_rho0; by *= k.rx_kg_rho0; bz *= k.rx_kg_rho0;
        sum *= k.rx_kg_rho0 * k.rx_kg_rho0; sb *= k.rx_kg_rho0 * k.rx_kg_rho0;
    }
    const float rho_i = c.boundary_handle ? rho + rb * c.rho0 : rho;
    if (rho_only) { rho_out[i] = rho_i; return; }                  // compute_all_rho alone (solver_base.py:36-50 with :166-174): pbf_lambda keeps its values
    const float con = rmax(rho_i / c.rho0 - 1.0f, 0.0f);          // :127-128
    float dxs = cx, dys = cy, dzs = cz;
    if (c.boundary_handle) { dxs = cx + bx; dys = cy + by; dzs = cz + bz; }   // :112
    const float cdcd = (dxs * dxs + dys * dys) + dzs * dzs;
    const float tot = c.boundary_handle ? (cdcd + sum) + sb : cdcd + sum;     // :48 / :50
    const float lam = con == 0.0f ? 0.0f : -con / (tot + k.eps);  // :39-52
    rho_out[i] = rho_i;
    lambda_out[i] = lam;
    Pout[i] = make_float4(pi.x, pi.y, pi.z, lam);
}

// delta_pos, the prediction and phase 1 of update_all_pos.  PL = (pos, lambda); writes Pn = new position, Vn = phase-1 velocity.
template <bool QUAD, bool RX = false, bool QSUM = false>
__global__ __launch_bounds__(kBlock) void k_pbf_delta(Consts c, PbfConsts k, StepDt step, const float4 *__restrict__ PL, const float4 *__restrict__ V,
                                                      const float4 *__restrict__ WP, const uint32_t *__restrict__ nl,
                                                      const uint32_t *__restrict__ nlb, const int *__restrict__ cnt,
                                                      float4 *__restrict__ dpos_out, float4 *__restrict__ Pn, float4 *__restrict__ Vn)
{
    const float dt = step_dt(step);
    if (blockIdx.x == 0 && threadIdx.x == 0) clock_advance(c.clock, dt);      // once per step: its dt joins the handle's clock
    const float4 *P = PL;
    SPH_SWEEP_PROLOGUE_M(QUAD)
    const float li = pi.w;
    float fa[3] = {0.f, 0.f, 0.f};
    float &ax = fa[0], &ay = fa[1], &az = fa[2];
    auto pair = [&](const float4 pj) {
        const float dx = pi.x - pj.x, dy = pi.y - pj.y, dz = pi.z - pj.z;
        if constexpr (RX) {
            const PbfPairRx p = pbf_pair_rx(c, k, dx, dy, dz);
            float t12 = (p.tp * p.tp) * p.tp; t12 *= t12; t12 *= t12;
            const float f = __builtin_fmaf(k.rx_sc, t12, li + pj.w) * p.s;
            ax = __builtin_fmaf(f, dx, ax); ay = __builtin_fmaf(f, dy, ay); az = __builtin_fmaf(f, dz, az);
            return;
        }
        const float r = norm3(dx, dy, dz);
        float sc = poly_w(c, k, r) / k.w_corr;                     // :148
        sc *= sc; sc *= sc; sc *= k.neg_k;                         // :149-151
        const F3 g = spiky_grad(c, k, dx, dy, dz, r);
        const float f = (li + pj.w) + sc;                          // :153
        ax += f * g.x; ay += f * g.y; az += f * g.z;
    };
    if (QUAD) sweep_quad<false>(SrcP{PL}, nlp, kf, q, fa, pair);
    else if constexpr (QSUM) sweep_list<false>(SrcP{PL}, nlp, kf, pbf_quad_sum(fa, pair));
    else sweep_list<false>(SrcP{PL}, nlp, kf, pair);
    float wa[3] = {0.f, 0.f, 0.f};
    float &bx = wa[0], &by = wa[1], &bz = wa[2];
    auto wall = [&](const float4 pj) {
        const float dx = pi.x - pj.x, dy = pi.y - pj.y, dz = pi.z - pj.z;
        if constexpr (RX) {
            const PbfPairRx p = pbf_pair_rx(c, k, dx, dy, dz);
            float t12 = (p.tp * p.tp) * p.tp; t12 *= t12; t12 *= t12;
            const float f = __builtin_fmaf(k.rx_sc, t12, li) * p.s;
            bx = __builtin_fmaf(f, dx, bx); by = __builtin_fmaf(f, dy, by); bz = __builtin_fmaf(f, dz, bz);
            return;
        }
        const float r = norm3(dx, dy, dz);
        float sc = poly_w(c, k, r) / k.w_corr;
        sc *= sc; sc *= sc; sc *= k.neg_k;
        const F3 g = spiky_grad(c, k, dx, dy, dz, r);
        const float f = li + sc;                                   // :164
        bx += f * g.x; by += f * g.y; bz += f * g.z;
    };
    if (QUAD) sweep_quad<false>(SrcP{WP}, nlbp, kb, q, wa, wall);
    else if constexpr (QSUM) sweep_list<false>(SrcP{WP}, nlbp, kb, pbf_quad_sum(wa, wall));
    else sweep_list<false>(SrcP{WP}, nlbp, kb, wall);
    if (!owner) return;
    if constexpr (RX) { ax *= k.rx_kg; ay *= k.rx_kg; az *= k.rx_kg; bx *= k.rx_kg; by *= k.rx_kg; bz *= k.rx_kg; }
    float dp[3];
    if (c.boundary_handle) { dp[0] = (ax + bx) / c.rho0; dp[1] = (ay + by) / c.rho0; dp[2] = (az + bz) / c.rho0; }   // :62
    else { dp[0] = ax / c.rho0; dp[1] = ay / c.rho0; dp[2] = az / c.rho0; }                                          // :64
    const float4 vi = V[i];
    const float acc[3] = {c.accel[0], c.accel[1], c.accel[2]};     // reset(), solver_base.py:131-133: the handle's vector (DevScalars.frc.accel)
    const float pos[3] = {pi.x, pi.y, pi.z};
    float vel[3] = {vi.x, vi.y, vi.z}, pp[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        vel[a] += dt * acc[a];                                     // :28
        pp[a] = pos[a] + dt * vel[a];                              // :29
        pp[a] += dp[a];                                            // :69
        vel[a] = (pp[a] - pos[a]) / dt;                            // :70
        if (!c.boundary_handle) {                                  // :73-81
            if (pp[a] <= k.lo[a]) { pp[a] = k.lo[a]; vel[a] *= 0.5f; }
            if (pp[a] >= k.hi[a]) { pp[a] = k.hi[a]; vel[a] *= 0.5f; }
        }
    }
    dpos_out[i] = make_float4(dp[0], dp[1], dp[2], 0.f);
    Pn[i] = make_float4(pp[0], pp[1], pp[2], 0.f);
    Vn[i] = make_float4(vel[0], vel[1], vel[2], 0.f);
}

// phases 2 and 3 of update_all_pos: the 27-cell walk of for_all_neighbor over the cell lists of the step's start (belong_grid of the OLD
// position), distances and kernel on the NEW positions.  Writes the final state: Pfin = new position, Vfin = vel + c * v.
// QUAD (small scenes): the four lanes of a quad serve one particle; lane q evaluates candidate j0 + q of every batch of four of a cell and
// all four add the four terms in candidate order (quad_bcast, sph_kernels.h) -- a candidate that is skipped contributes +0, which leaves
// the running sums (never -0) unchanged: the same additions in the same order as the one-lane walk.
//
// SLAB (x-slab handles, one lane per particle): a ghost (cnt < 0, k_build_nl's ghost bit) does not walk -- half of its 27 cells are not resident --
// and copies what its owner sent after k_pbf_delta (slab_exchange_field mode 4: Pn, Vn) into Pfin / Vfin, so that every resident slot of the
// final arrays holds defined values.  Nothing downstream depends on them: the next particle exchange decides "last step's ghost: dies" from the
// sign of id[] alone, in k_classify_count and k_classify_write alike (classify_slot returns before it reads P), the dead slot takes no part in
// the sort, and the owner sends the ghost's successor.  An owned particle of an edge column finds its ghost neighbours' refreshed Pn / Vn through
// the same cell lists as on one GPU, in the same (cell, id) order.  The one-GPU kernels are the instantiations SLAB = false of the same body.
template <bool QUAD, bool RX, bool SLAB>
__device__ __forceinline__ void pbf_xsph_body(const Consts &c, const PbfConsts &k, const float4 *__restrict__ Pold, const float4 *__restrict__ Pn,
                                              const float4 *__restrict__ Vn, const int *__restrict__ cell_start, const int *__restrict__ cnt,
                                              float4 *__restrict__ Pfin, float4 *__restrict__ Vfin)
{
    const int blk = xcd_block(blockIdx.x, gridDim.x);
    const int q = QUAD ? (int)(threadIdx.x & 3) : 0;
    const int i = QUAD ? blk * (kBlock / 4) + (int)(threadIdx.x >> 2) : blk * kBlock + (int)threadIdx.x;
    if (i >= c.n) return;                                          // (a quad leaves together)
    const float4 po = Pold[i], pi = Pn[i], vi = Vn[i];
    if constexpr (SLAB) {
        if (cnt[i] < 0) {                                          // a ghost: the owner's values, no walk
            Pfin[i] = make_float4(pi.x, pi.y, pi.z, 0.f);
            Vfin[i] = make_float4(vi.x, vi.y, vi.z, 0.f);
            return;
        }
    }
    int cx, cy, cz;
    cell_id_of(c, po.x, po.y, po.z, cx, cy, cz);                   // belong_grid, set by update_grid at the step's start
    float ax = 0.f, ay = 0.f, az = 0.f;
    auto term = [&](int j, float &tx, float &ty, float &tz) {      // (vel_j - vel_i) W, or nothing
        const float4 pj = Pn[j];
        const float ex = pi.x - pj.x, ey = pi.y - pj.y, ez = pi.z - pj.z;
        if constexpr (RX) {                                        // membership and W from r2 alone; rx_ck in the epilogue
            const float r2 = pbf_r2_rx(ex, ey, ez);
            if (r2 > c.r2_cut) return;
            const float4 vj = Vn[j];
            const float tp = pbf_tp_rx(k, r2), w = (tp * tp) * tp;
            tx = (vj.x - vi.x) * w; ty = (vj.y - vi.y) * w; tz = (vj.z - vi.z) * w;
            return;
        }
        const float r = norm3(ex, ey, ez);
        if (r > c.h) return;                                       // :466
        const float4 vj = Vn[j];
        const float w = poly_w(c, k, r);                           // pbf_solver.py:98
        tx = (vj.x - vi.x) * w; ty = (vj.y - vi.y) * w; tz = (vj.z - vi.z) * w;
    };
    for (int dx = -1; dx <= 1; ++dx)
        for (int dy = -1; dy <= 1; ++dy)
            for (int dz = -1; dz <= 1; ++dz) {
                const int x = cx + dx, y = cy + dy, z = cz + dz;
                if (x >= c.gx || y >= c.gy || z >= c.gz || x < 0 || y < 0 || z < 0) continue;          // ParticleSystem.py:453-456
                const int slot = cell_slot_xyz(c, x, y, z, x + y * c.sy + z * c.sz);
                if (slot < 0) continue;
                const int a = cell_start[slot], b = cell_start[slot + 1];
                if (QUAD) {
                    for (int j0 = a; j0 < b; j0 += 4) {
                        const int j = j0 + q;
                        float tx = 0.f, ty = 0.f, tz = 0.f;
                        if (j < b && j != i) term(j, tx, ty, tz);  // :461
                        ax += quad_bcast<0>(tx); ax += quad_bcast<1>(tx); ax += quad_bcast<2>(tx); ax += quad_bcast<3>(tx);
                        ay += quad_bcast<0>(ty); ay += quad_bcast<1>(ty); ay += quad_bcast<2>(ty); ay += quad_bcast<3>(ty);
                        az += quad_bcast<0>(tz); az += quad_bcast<1>(tz); az += quad_bcast<2>(tz); az += quad_bcast<3>(tz);
                    }
                } else {
                    for (int j = a; j < b; ++j) {
                        if (j == i) continue;                      // :461
                        float tx = 0.f, ty = 0.f, tz = 0.f;
                        if constexpr (RX) {
                            term(j, tx, ty, tz);
                            ax += tx; ay += ty; az += tz;
                            continue;
                        }
                        const float4 pj = Pn[j];
                        const float ex = pi.x - pj.x, ey = pi.y - pj.y, ez = pi.z - pj.z;
                        const float r = norm3(ex, ey, ez);
                        if (r > c.h) continue;                     // :466
                        const float4 vj = Vn[j];
                        const float w = poly_w(c, k, r);           // pbf_solver.py:98
                        tx = (vj.x - vi.x) * w; ty = (vj.y - vi.y) * w; tz = (vj.z - vi.z) * w;
                        ax += tx; ay += ty; az += tz;
                    }
                }
            }
    if (q != 0) return;
    Pfin[i] = make_float4(pi.x, pi.y, pi.z, 0.f);
    const float cv = RX ? k.rx_ck : k.c_visc;
    Vfin[i] = make_float4(vi.x + cv * ax, vi.y + cv * ay, vi.z + cv * az, 0.f);   // :92 / :94
}
template <bool QUAD, bool RX = false>
__global__ __launch_bounds__(kBlock) void k_pbf_xsph(Consts c, PbfConsts k, const float4 *__restrict__ Pold, const float4 *__restrict__ Pn,
                                                     const float4 *__restrict__ Vn, const int *__restrict__ cell_start,
                                                     float4 *__restrict__ Pfin, float4 *__restrict__ Vfin)
{
    pbf_xsph_body<QUAD, RX, false>(c, k, Pold, Pn, Vn, cell_start, nullptr, Pfin, Vfin);
}
template <bool RX>
__global__ __launch_bounds__(kBlock) void k_pbf_xsph_slab(Consts c, PbfConsts k, const float4 *__restrict__ Pold, const float4 *__restrict__ Pn,
                                                          const float4 *__restrict__ Vn, const int *__restrict__ cell_start, const int *__restrict__ cnt,
                                                          float4 *__restrict__ Pfin, float4 *__restrict__ Vfin)
{
    pbf_xsph_body<false, RX, true>(c, k, Pold, Pn, Vn, cell_start, cnt, Pfin, Vfin);
}

}  // namespace sph
