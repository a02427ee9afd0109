// sph_derived_kernels.h -- derived per-particle fields of the fluid on the device: the plain SPH estimates of the velocity
// gradient (and with it vorticity and divergence), of the free-surface normal and of the kernel cover, in one pair sweep over the lists the handle
// already has.  k_derived_pack puts (vel, rho) of every solver into one float4 array, so that the sweep has one shape; k_derived is the sweep,
// modelled on k_dfsph_ext (positions staged, (vel, rho) gathered through the staged source index); k_unsort_planes brings one quantity to API order.
//
// The arithmetic, once: f32, unfused, KF<false> on every handle (the sweep is not part of a step).  Per fluid entry j of particle i's list, in list
// order: d = x_i - x_j, r = norm3(d); r > h contributes nothing (Verlet lists hold such pairs); vol = rho_j > 0 ? m / rho_j : 0; g = grad_in(d, r),
// w = w_in(r); G_ab += (vol (v_j,a - v_i,a)) g_b; F_b += vol g_b; F_c += vol w.  A tagged rigid entry: F_b += V_r g_b, F_c += V_r w.  Per wall entry:
// B_b += V_b g_b, B_c += V_b w.  No self term.  Every accumulator takes at most one term per entry (the quad walk's condition).
#pragma once
#include "sph_kernels.h"

namespace sph {

// the planes of the result, plane k of particle i at out[k * stride + i] (device order)
enum { DV_VELGRAD = 0, DV_VORTICITY = 9, DV_DIVERGENCE = 12, DV_NORMAL = 13, DV_COVER = 16, kDerivedPlanes = 17 };

__global__ __launch_bounds__(kBlock) void k_derived_pack(int n, const float4 *__restrict__ V, const float *__restrict__ rho, float4 *__restrict__ VR)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const float4 v = V[i];
    VR[i] = make_float4(v.x, v.y, v.z, rho[i]);
}

template <bool RIGID, int SWEEP>
__global__ __launch_bounds__(kBlock) void k_derived(Consts c, const float4 *__restrict__ P, const float4 *__restrict__ VR, const float4 *__restrict__ WP,
                                                    const uint32_t *__restrict__ nl, const uint32_t *__restrict__ nlb, const int *__restrict__ cnt,
                                                    RigidView rv, const uint2 *__restrict__ stage_src, const int *__restrict__ stage_cnt,
                                                    float *__restrict__ out)
{
    constexpr bool STAGED = SWEEP == SWEEP_STAGED, QUAD = SWEEP == SWEEP_QUAD;
    using K = KF<false>;
    extern __shared__ float4 s_operand[];
    SPH_SWEEP_PROLOGUE_M(QUAD)
    uint32_t *s_src = StageF4Src::second(s_operand, c.stage_cap);      // (vel, rho) needs 16 B: gathered from memory
    const SrcAB mem{P, VR};
    const StageF4Src lay{{s_operand, P}, s_src};
    const StageF4Src::Gather lds = lay.gather(VR);
    const bool staged = STAGED && stage_operands(lay, StagePlan{stage_src, stage_cnt, blk}) != kNotStaged;
    const float4 vi = VR[ii];
    float fa[13] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};      // G (row a, column b), F_x, F_y, F_z, F_c
    auto pair = [&](const float4 pj, const float4 vj, const uint32_t j) {
        const float dx = pi.x - pj.x, dy = pi.y - pj.y, dz = pi.z - pj.z;
        const float r = K::norm3(dx, dy, dz);
        if (r > c.h) return;                                 // a skin entry of a Verlet list
        const F3 g = K::grad_in(c, dx, dy, dz, r);
        const float w = K::w_in(c, r);
        if (RIGID && (j & kRigidTag)) {                      // a coupled body's sample: (x, y, z, V_r); nothing goes to G
            fa[9] += pj.w * g.x; fa[10] += pj.w * g.y; fa[11] += pj.w * g.z;
            fa[12] += pj.w * w;
            return;
        }
        const float vol = vj.w > 0.f ? c.m / vj.w : 0.f;
        const float sx = vol * (vj.x - vi.x), sy = vol * (vj.y - vi.y), sz = vol * (vj.z - vi.z);
        fa[0] += sx * g.x; fa[1] += sx * g.y; fa[2] += sx * g.z;
        fa[3] += sy * g.x; fa[4] += sy * g.y; fa[5] += sy * g.z;
        fa[6] += sz * g.x; fa[7] += sz * g.y; fa[8] += sz * g.z;
        fa[9] += vol * g.x; fa[10] += vol * g.y; fa[11] += vol * g.z;
        fa[12] += vol * w;
    };
    if (QUAD) sweep_quad<RIGID>(mem, nlp, kf, q, fa, pair, rv);
    else if (staged && (RIGID ? stage_lists16(stage_cnt, blk) : c.nl16 != 0)) walk_list16(lds, nlp, kf, pair);
    else if (staged) walk_staged<RIGID>(lds, nlp, kf, pair, rv);
    else sweep_list<RIGID>(mem, nlp, kf, pair, rv);
    float wa[4] = {0.f, 0.f, 0.f, 0.f};                      // B_x, B_y, B_z, B_c
    auto wall = [&](const float4 pj) {                       // pj = (x, y, z, V_b)
        const float dx = pi.x - pj.x, dy = pi.y - pj.y, dz = pi.z - pj.z;
        const float r = K::norm3(dx, dy, dz);
        if (r > c.h) return;
        const F3 g = K::grad_in(c, dx, dy, dz, r);
        wa[0] += pj.w * g.x; wa[1] += pj.w * g.y; wa[2] += pj.w * g.z;
        wa[3] += pj.w * K::w_in(c, r);
    };
    if (QUAD) sweep_quad<false>(SrcP{WP}, nlbp, kb, q, wa, wall);
    else sweep_list<false>(SrcP{WP}, nlbp, kb, wall);
    if (!owner) return;                                      // (no lane past c.n is an owner)
    float *o = out + i;
    const size_t st = (size_t)c.stride;
#pragma unroll
    for (int k = 0; k < 9; ++k) o[(DV_VELGRAD + k) * st] = fa[k];
    o[(DV_VORTICITY + 0) * st] = fa[7] - fa[5];              // G_zy - G_yz
    o[(DV_VORTICITY + 1) * st] = fa[2] - fa[6];              // G_xz - G_zx
    o[(DV_VORTICITY + 2) * st] = fa[3] - fa[1];              // G_yx - G_xy
    o[DV_DIVERGENCE * st] = (fa[0] + fa[4]) + fa[8];
    o[(DV_NORMAL + 0) * st] = -(c.h * (fa[9] + wa[0]));
    o[(DV_NORMAL + 1) * st] = -(c.h * (fa[10] + wa[1]));
    o[(DV_NORMAL + 2) * st] = -(c.h * (fa[11] + wa[2]));
    o[DV_COVER * st] = fa[12] + wa[3];
}

// planes first .. first + width - 1 of the result in API order: dst[id * width + a]
__global__ __launch_bounds__(kBlock) void k_unsort_planes(int n, const float *__restrict__ src, size_t stride, int first, int width, const int *__restrict__ id,
                                                          float *__restrict__ dst)
{
    const int s = blockIdx.x * kBlock + threadIdx.x;
    if (s >= n) return;
    const size_t o = (size_t)id[s] * width;
    for (int a = 0; a < width; ++a) dst[o + a] = src[(size_t)(first + a) * stride + s];
}

}  // namespace sph
