// sph_wall_load_kernels.h -- loads on walls and static geometry: what the fluid presses on selected wall groups with.
//
// A measured wall sample is a body sample that never moves and that the fluid already feels: the measured set M -- (x, y, z, V_b) of the selected
// groups' samples in the wall set's sorted order -- is handed to k_build_rnl (its lists) and to k_rigid_force / k_rigid_force_p<MODE> (the pair
// formulas; sph_rigid_kernels.h, sph_pressure_kernels.h) as a body's samples are.  There is no second copy of a pair formula here.  This file holds
// what a body does on the host or not at all: the zeroing of the per-sample totals at the head of a step, the per-group reduction behind it, and
// the way of the per-sample forces from sorted order into a group's own sample order.
//
// The reduction follows the arithmetic contract of sph_diag_kernels.h: every f32 operand is widened to f64 first, products and the sums inside a
// term are f64, terms are summed in f64 in a fixed order -- thread-strided, the wave butterfly, the waves through LDS in wave order, the partial
// rows in index order.  No atomics: the same state gives the same bits.  It is segmented by group: one launch pair serves every selected group
// (blockIdx.y = the group's place in the selection).
#pragma once
#include "sph_device.h"

namespace sph {

constexpr int kWlParts = 64;             // workgroups of k_wl_partials per group at most: grid-stride above 16 384 samples of a group
constexpr int kWlSums = 6;               // f64 sums of a partial row: force (3), torque (3)
constexpr int kWlRow = 8;                // doubles of a partial row (two unused: rows stay 64-byte aligned)
constexpr int kWlAcc = 8;                // doubles a group accumulates across steps: impulse (3), angular impulse about the origin (3), seconds, unused
constexpr int kWlMaxGroups = 1024;       // selected groups of a handle at most (blockIdx.y of the reduction)

// the measured set on the device (memory of the feature's own; the host side is sph_host_wall_load.h)
struct WlView {
    int nm, ng;                  // samples of M, selected groups
    const float4 *MP;            // [nm + 64] (x, y, z, V_b), sorted order
    const float *force;          // [3 nm] the step's running per-sample totals, sorted order
    const int *perm;             // [nm] the entries of M group by group (selection order), inside a group in sorted order
    const int *seg;              // [ng + 1] where a group's entries start in perm
};

__device__ __forceinline__ int wl_parts_of(int count) { return min(kWlParts, max(1, (count + kBlock - 1) / kBlock)); }

// head of every step: the samples' totals start at zero (rigid_solver.py:38 does it for a body at the end of its step)
__global__ __launch_bounds__(kBlock) void k_wl_zero(int n3, float *__restrict__ force)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i < n3) force[i] = 0.0f;
}

// First stage: workgroup (p, g) sums the entries p kBlock + t, + parts kBlock, ... of group g: f_b and (x_b - c) x f_b, about the point c.
// A workgroup beyond the group's parts leaves at once; k_wl_final reads only the rows that were written.
__global__ __launch_bounds__(kBlock) void k_wl_partials(WlView v, double cx, double cy, double cz, double *__restrict__ part)
{
    __shared__ double s_sum[kBlock / 64][kWlSums];
    const int g = blockIdx.y, first = v.seg[g], count = v.seg[g + 1] - first, parts = wl_parts_of(count);
    if ((int)blockIdx.x >= parts) return;
    double s[kWlSums];
#pragma unroll
    for (int k = 0; k < kWlSums; ++k) s[k] = 0.0;
    for (int i = blockIdx.x * kBlock + threadIdx.x; i < count; i += parts * kBlock) {
        const int e = v.perm[first + i];
        const float4 p = v.MP[e];
        const double fx = (double)v.force[3 * e], fy = (double)v.force[3 * e + 1], fz = (double)v.force[3 * e + 2];
        const double rx = (double)p.x - cx, ry = (double)p.y - cy, rz = (double)p.z - cz;
        s[0] += fx; s[1] += fy; s[2] += fz;
        s[3] += ry * fz - rz * fy; s[4] += rz * fx - rx * fz; s[5] += rx * fy - ry * fx;
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int k = 0; k < kWlSums; ++k) s[k] = wave_sum(s[k]);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < kWlSums; ++k) s_sum[wave][k] = s[k];
    }
    __syncthreads();
    if (threadIdx.x < kWlSums) {         // the waves in wave order, one thread per column
        double a = s_sum[0][threadIdx.x];
        for (int w = 1; w < kBlock / 64; ++w) a += s_sum[w][threadIdx.x];
        part[((size_t)g * kWlParts + blockIdx.x) * kWlRow + threadIdx.x] = a;
    }
}

// Second stage, one workgroup per group: the partial rows in index order into load[g] = (force, torque about c).  acc != null (the end of a
// step; c = the origin): impulse += dt F, angular impulse += dt torque, seconds += dt, with the dt the step used (StepDt, as k_diag_final).
// acc == null: a read on demand, nothing accumulates.
__global__ __launch_bounds__(kBlock) void k_wl_final(WlView v, StepDt dt, const double *__restrict__ part, double *__restrict__ load, double *__restrict__ acc)
{
    const int g = blockIdx.x, t = threadIdx.x;
    if (t > kWlSums) return;
    const double d = acc ? (double)step_dt(dt) : 0.0;
    if (t == kWlSums) {
        if (acc) acc[(size_t)g * kWlAcc + 6] += d;
        return;
    }
    const int parts = wl_parts_of(v.seg[g + 1] - v.seg[g]);
    const double *row = part + (size_t)g * kWlParts * kWlRow + t;
    double a = row[0];
    for (int k = 1; k < parts; ++k) a += row[(size_t)k * kWlRow];
    load[(size_t)g * kWlRow + t] = a;
    if (acc) acc[(size_t)g * kWlAcc + t] += d * a;
}

// the step's per-sample forces of one selected group, from sorted order into the group's own sample order (for the box: the order of the wall
// downloads).  slot[e]: the group's place in the selection, local[e]: the sample's index inside its group
__global__ __launch_bounds__(kBlock) void k_wl_unsort(int nm, int which, const int *__restrict__ slot, const int *__restrict__ local,
                                                      const float *__restrict__ force, float *__restrict__ out)
{
    const int e = blockIdx.x * kBlock + threadIdx.x;
    if (e >= nm || slot[e] != which) return;
    const int o = local[e];
    out[3 * o] = force[3 * e]; out[3 * o + 1] = force[3 * e + 1]; out[3 * o + 2] = force[3 * e + 2];
}

}  // namespace sph
