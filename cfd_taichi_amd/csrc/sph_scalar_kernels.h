// sph_scalar_kernels.h -- one carried scalar T per particle (a temperature, a dye concentration) on the device: it diffuses
// (Brookshaw's Laplacian over the lists the step has anyway) and, with beta != 0, lifts (a Boussinesq kick along the step's acceleration vector).
// T is kept by particle id (API order), so the sort and every existing kernel stay as they are.  k_scalar_pack puts (x, y, z, T) of every particle
// into one float4 array in device order, so that the sweep has one operand per neighbour; k_scalar_rate is the sweep, modelled on k_derived (no
// second operand: the staged instantiation gathers nothing from memory); k_scalar_advance is the step's epilogue; k_scalar_unsort brings the rate to
// API order; k_scalar_compact renumbers T behind sph_remove_in_box.
//
// The arithmetic of the sweep, once: f32, unfused.  Per FLUID entry j of particle i's fluid list, in list order: d = x_i - x_j,
// r2 = (dx dx + dy dy) + dz dz, r = sqrt_rn(r2); r > h contributes nothing (Verlet lists hold such pairs); q = div_by_h(r);
// g = q <= 0.5 ? (3 (q q) - 2 q) : -((1 - q) (1 - q)); f = (g r) / (r2 + eta2), one IEEE-rounded quotient; acc += (T_i - T_j) f.  A tagged rigid
// entry adds nothing (the body is insulated) and the wall lists are not walked (so are the walls).  No self term; acc starts at +0 and takes at most
// one term per entry (the quad walk's condition).  rate_i = kq acc, with eta2 = 0.01 h^2 and kq = 12 D (m / rho0) kw / h formed by the host in f64.
// No density is read: one shape on every solver, and the pair term is antisymmetric bit for bit.
#pragma once
#include "sph_kernels.h"

namespace sph {

struct ScalarConsts {
    float eta2, kq;       // the sweep
    float beta, t_ref;    // the kick: s = -(beta (T - t_ref)), applied only when beta != 0
};

// XT[s] = (P[s].xyz, T[id[s]]) in device order
__global__ __launch_bounds__(kBlock) void k_scalar_pack(int n, const float4 *__restrict__ P, const int *__restrict__ id, const float *__restrict__ T,
                                                        float4 *__restrict__ XT)
{
    const int s = blockIdx.x * kBlock + threadIdx.x;
    if (s >= n) return;
    const float4 p = P[s];
    XT[s] = make_float4(p.x, p.y, p.z, T[id[s]]);
}

// (the prologue names its operand array P: here it is XT, so pi = (x_i, T_i))
template <bool RIGID, int SWEEP>
__global__ __launch_bounds__(kBlock) void k_scalar_rate(Consts c, ScalarConsts k, const float4 *__restrict__ P, const uint32_t *__restrict__ nl,
                                                        const int *__restrict__ cnt, RigidView rv, const uint2 *__restrict__ stage_src,
                                                        const int *__restrict__ stage_cnt, float *__restrict__ rate)
{
    constexpr bool STAGED = SWEEP == SWEEP_STAGED, QUAD = SWEEP == SWEEP_QUAD;
    extern __shared__ float4 s_operand[];
    const uint32_t *const nlb = nullptr;                     // the wall lists are not walked
    SPH_SWEEP_PROLOGUE_M(QUAD)
    (void)nlbp; (void)kb;
    const SrcA mem{P};
    const StageF4<> lds{s_operand, P};
    const bool staged = STAGED && stage_operands(lds, StagePlan{stage_src, stage_cnt, blk}) != kNotStaged;
    float fa[1] = {0.f};
    auto pair = [&](const float4 pj, const float4, const uint32_t j) {
        if (RIGID && (j & kRigidTag)) return;                // a coupled body's sample: insulated
        const float dx = pi.x - pj.x, dy = pi.y - pj.y, dz = pi.z - pj.z;
        const float r2 = (dx * dx + dy * dy) + dz * dz;
        const float r = sqrt_rn(r2);
        if (r > c.h) return;                                 // a skin entry of a Verlet list
        const float q = div_by_h(c, r);
        const float t = 1.0f - q;
        const float g = q <= 0.5f ? (3.0f * (q * q) - 2.0f * q) : -(t * t);
        const float f = div_shared(g * r, recip_prepare(r2 + k.eta2));
        fa[0] += (pi.w - pj.w) * f;
    };
    if (QUAD) sweep_quad<RIGID>(mem, nlp, kf, q, fa, pair, rv);
    else if (staged && (RIGID ? stage_lists16(stage_cnt, blk) : c.nl16 != 0)) walk_list16(lds, nlp, kf, pair);
    else if (staged) walk_staged<RIGID>(lds, nlp, kf, pair, rv);
    else sweep_list<RIGID>(mem, nlp, kf, pair, rv);
    if (!owner) return;                                      // (no lane past c.n is an owner)
    rate[i] = k.kq * fa[0];
}

// The step's epilogue, one thread per particle in device order, with dt as the step left it.  beta != 0: V.xyz += (dt s) a with s = -(beta (T - t_ref))
// from T^n and a = the step's acceleration vector; .w is kept.  Then T[id] = T + dt rate.  beta == 0: V is not touched.
__global__ __launch_bounds__(kBlock) void k_scalar_advance(int n, ScalarConsts k, StepDt step, const DevScalars *__restrict__ ds, const int *__restrict__ id,
                                                           const float *__restrict__ rate, float *__restrict__ T, float4 *__restrict__ V)
{
    const int s = blockIdx.x * kBlock + threadIdx.x;
    if (s >= n) return;
    const float dt = step_dt(step);
    const int o = id[s];
    const float t = T[o];
    if (k.beta != 0.0f) {
        const float b = dt * -(k.beta * (t - k.t_ref));
        float4 v = V[s];
        v.x += b * ds->frc.accel[0]; v.y += b * ds->frc.accel[1]; v.z += b * ds->frc.accel[2];
        V[s] = v;
    }
    T[o] = t + dt * rate[s];
}

// dst[id[s]] = src[s]: the rate in API order
__global__ __launch_bounds__(kBlock) void k_scalar_unsort(int n, const float *__restrict__ src, const int *__restrict__ id, float *__restrict__ dst)
{
    const int s = blockIdx.x * kBlock + threadIdx.x;
    if (s >= n) return;
    dst[id[s]] = src[s];
}

// sph_remove_in_box: the survivors' values under their new ids, by the renumbering k_remove_compact applies (scan_id: removed ids below an id).
// Into a second array: a survivor's new id is another particle's old one.
template <class Pred>
__global__ __launch_bounds__(kBlock) void k_scalar_compact(int n, Pred gone, const float4 *__restrict__ P, const int *__restrict__ id,
                                                           const int *__restrict__ scan_id, const float *__restrict__ T, float *__restrict__ out)
{
    const int s = blockIdx.x * kBlock + threadIdx.x;
    if (s >= n) return;
    if (gone(s, P[s])) return;
    const int o = id[s];
    out[o - scan_id[o]] = T[o];
}

// T[first .. first + m) = value
__global__ __launch_bounds__(kBlock) void k_scalar_fill(int first, int m, float value, float *__restrict__ T)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i < m) T[first + i] = value;
}

}  // namespace sph
