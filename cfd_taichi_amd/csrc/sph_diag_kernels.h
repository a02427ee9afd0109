// sph_diag_kernels.h -- run diagnostics of the fluid on the device: the SphDiagnostics row of include/sph_mi355x.h in two
// launches.  k_diag_partials streams positions, velocities, ids (and densities) once, at most kDiagParts workgroups, one partial row each;
// k_diag_final, one workgroup, folds the partial rows in index order, scales, and writes the finished row -- into a scratch row
// (sph_diagnostics) or into the next slot of a ring (sph_diag_record), where it also advances the device-resident counters.
//
// The arithmetic contract, once: every f32 operand is widened to f64 first; products and the three-term sums inside a term are f64; terms are
// summed in f64 in a fixed order -- thread-strided, then the wave butterfly (wave_sum), then the waves through LDS in wave order, then the
// workgroups' partial rows in index order.  No atomics, nothing depends on which workgroup finishes first: the same state in the same slot order
// gives the same bits.  Scaling by m, 1/2, 1/n happens once, at the end, in f64.  Maxima, minima, the id and n are exact.
#pragma once
#include "sph_device.h"

namespace sph {

constexpr int kDiagParts = 256;          // workgroups of k_diag_partials at most: grid-stride above 65 536 particles
constexpr int kDiagSums = 12;            // f64 sums of a partial row: v (3), x cross v (3), |v|^2, a.x, x (3), rho
// a partial row, as doubles (the f32 extrema and the id widen exactly): the sums, then
enum { DP_VMAX = kDiagSums, DP_VID, DP_MIN, DP_MAX = DP_MIN + 3, DP_RHO_MIN = DP_MAX + 3, DP_RHO_MAX, DP_USED, kDiagPartStride = 24 };
static_assert(DP_USED <= kDiagPartStride, "partial row");
constexpr int kDiagSlots = 32;           // doubles of an SphDiagnostics row

// Recording (sph_diag_record): what the device keeps between steps.  The host writes the block when recording is switched on and reads it in
// sph_diag_read; in between only k_diag_final's thread 0 writes it, once per step, so that a replayed graph needs nothing from the host.
struct DiagCtl {
    long long count;     // rows recorded since recording was switched on: the next row goes to ring slot count % rows
    long long since;     // solver steps since then: step `since + 1` is due when it is a multiple of `every`
    int step;            // the handle's step counter (SPH_S_SIMULATE_CNT) before the step that is ending
    int every, rows, pad;
};
__device__ __forceinline__ bool diag_due(const DiagCtl *ctl) { return !ctl || (ctl->since + 1) % ctl->every == 0; }

__device__ __forceinline__ float wave_min(float v) { return -wave_max(-v); }            // (exact: negation only flips the sign bit)
__device__ __forceinline__ int wave_min(int v) { return -wave_max(-v); }                // ids are >= 0

// ctl != null: a recorded step -- every workgroup leaves at once unless the step is due.  rho == null: the row carries no densities.
__global__ __launch_bounds__(kBlock) void k_diag_partials(int n, const float4 *__restrict__ P, const float4 *__restrict__ V, const int *__restrict__ id,
                                                          const float *__restrict__ rho, const DevScalars *__restrict__ ds,
                                                          const DiagCtl *__restrict__ ctl, double *__restrict__ part)
{
    if (!diag_due(ctl)) return;
    __shared__ double s_sum[kBlock / 64][kDiagSums];
    __shared__ float s_ext[kBlock / 64][9];
    __shared__ int s_id[kBlock / 64];
    const double ax = (double)ds->frc.accel[0], ay = (double)ds->frc.accel[1], az = (double)ds->frc.accel[2];
    double s[kDiagSums];
#pragma unroll
    for (int k = 0; k < kDiagSums; ++k) s[k] = 0.0;
    float vmax = -1.0f, lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY}, rlo = INFINITY, rhi = -INFINITY;
    int vid = 0x7fffffff;
    // One wave per SIMD at most, so it is the loads in flight that hide the memory latency: four trips' operands are requested in one batch (a
    // clamped index keeps the loads branch-free), then added in trip order -- the order of the plain grid-stride loop
    constexpr int kTrips = 4;
    const int first = blockIdx.x * kBlock + threadIdx.x, stride = gridDim.x * kBlock;
    for (int i0 = first; i0 < n; i0 += kTrips * stride) {
        float4 pb[kTrips], vb[kTrips];
        int ib[kTrips];
        float rb[kTrips];
#pragma unroll
        for (int u = 0; u < kTrips; ++u) {
            const int i = min(i0 + u * stride, n - 1);
            pb[u] = P[i]; vb[u] = V[i]; ib[u] = id[i];
            rb[u] = rho ? rho[i] : 0.0f;
        }
#pragma unroll
        for (int u = 0; u < kTrips; ++u) {
            if (i0 + u * stride >= n) break;
            const float4 p = pb[u], v = vb[u];
            const int pid = ib[u];
            const double x = (double)p.x, y = (double)p.y, z = (double)p.z, vx = (double)v.x, vy = (double)v.y, vz = (double)v.z;
            s[0] += vx; s[1] += vy; s[2] += vz;
            s[3] += y * vz - z * vy; s[4] += z * vx - x * vz; s[5] += x * vy - y * vx;
            s[6] += (vx * vx + vy * vy) + vz * vz;
            s[7] += (ax * x + ay * y) + az * z;
            s[8] += x; s[9] += y; s[10] += z;
            const float sp = sqrtf((v.x * v.x + v.y * v.y) + v.z * v.z);         // k_step_vmax's expression
            if (sp > vmax || (sp == vmax && pid < vid)) { vmax = sp; vid = pid; }
            lo[0] = fminf(lo[0], p.x); lo[1] = fminf(lo[1], p.y); lo[2] = fminf(lo[2], p.z);
            hi[0] = fmaxf(hi[0], p.x); hi[1] = fmaxf(hi[1], p.y); hi[2] = fmaxf(hi[2], p.z);
            if (rho) {
                s[11] += (double)rb[u];
                rlo = fminf(rlo, rb[u]); rhi = fmaxf(rhi, rb[u]);
            }
        }
    }
    // the wave: sums by the butterfly, the extrema likewise; the id is the lowest among the lanes that hold the wave's largest speed
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int k = 0; k < kDiagSums; ++k) s[k] = wave_sum(s[k]);
    const float wv = wave_max(vmax);
    const int wid = wave_min(vmax == wv ? vid : 0x7fffffff);
    float e[8] = {lo[0], lo[1], lo[2], hi[0], hi[1], hi[2], rlo, rhi};
#pragma unroll
    for (int k = 0; k < 8; ++k) e[k] = (k < 3 || k == 6) ? wave_min(e[k]) : wave_max(e[k]);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < kDiagSums; ++k) s_sum[wave][k] = s[k];
#pragma unroll
        for (int k = 0; k < 8; ++k) s_ext[wave][k] = e[k];
        s_ext[wave][8] = wv;
        s_id[wave] = wid;
    }
    __syncthreads();
    // the workgroup: the waves in wave order, one thread per column of the partial row
    double *row = part + (size_t)blockIdx.x * kDiagPartStride;
    const int t = threadIdx.x;
    if (t < kDiagSums) {
        double a = s_sum[0][t];
        for (int w = 1; w < kBlock / 64; ++w) a += s_sum[w][t];
        row[t] = a;
    } else if (t < kDiagSums + 8) {
        const int k = t - kDiagSums;
        const bool is_min = k < 3 || k == 6;
        float a = s_ext[0][k];
        for (int w = 1; w < kBlock / 64; ++w) a = is_min ? fminf(a, s_ext[w][k]) : fmaxf(a, s_ext[w][k]);
        row[DP_MIN + k] = (double)a;
    } else if (t == kDiagSums + 8) {
        float a = s_ext[0][8];
        int b = s_id[0];
        for (int w = 1; w < kBlock / 64; ++w) {
            const float c = s_ext[w][8];
            if (c > a || (c == a && s_id[w] < b)) { a = c; b = s_id[w]; }
        }
        row[DP_VMAX] = (double)a;
        row[DP_VID] = (double)b;
    }
}

struct DiagFinal {
    int n, nparts;
    double m;            // the particle mass, f64
    StepDt dt;           // the time step the step used: the host's value, or DevScalars.dt (dfsph; the adaptive time step)
    int step;            // on demand: SPH_S_SIMULATE_CNT (a recorded row takes DiagCtl's)
    int have_rho;
};
// out: the scratch row (ctl == null) or the ring's first row
__global__ __launch_bounds__(kBlock) void k_diag_final(DiagFinal f, const DevScalars *__restrict__ ds, DiagCtl *__restrict__ ctl, const double *__restrict__ part,
                                                       double *__restrict__ out)
{
    __shared__ double s_part[kDiagParts * kDiagPartStride];
    __shared__ double s_res[kDiagPartStride];
    const bool due = diag_due(ctl);
    long long count = 0, since = 0;
    int step = f.step, rows = 1;
    if (ctl) { count = ctl->count; since = ctl->since; step = ctl->step + 1; rows = ctl->rows; }
    if (due && (int)threadIdx.x < f.nparts) {      // one thread per partial row: all of a row's loads are in flight at once, one memory latency in all
        const double2 *src = (const double2 *)(part + (size_t)threadIdx.x * kDiagPartStride);
        double2 r[kDiagPartStride / 2];
#pragma unroll
        for (int k = 0; k < kDiagPartStride / 2; ++k) r[k] = src[k];
        double2 *dst = (double2 *)(s_part + threadIdx.x * kDiagPartStride);
#pragma unroll
        for (int k = 0; k < kDiagPartStride / 2; ++k) dst[k] = r[k];
    }
    __syncthreads();                      // (every thread has read ctl before thread 0 writes it)
    if (due) {
        const int t = threadIdx.x;
        if (t < kDiagSums) {              // the partial rows in index order
            double a = s_part[t];
#pragma unroll 16
            for (int k = 1; k < f.nparts; ++k) a += s_part[k * kDiagPartStride + t];
            s_res[t] = a;
        } else if (t >= DP_MIN && t < DP_USED) {
            const int k = t - DP_MIN;
            const bool is_min = k < 3 || k == 6;
            double a = s_part[t];
            for (int q = 1; q < f.nparts; ++q) { const double c = s_part[q * kDiagPartStride + t]; a = is_min ? fmin(a, c) : fmax(a, c); }
            s_res[t] = a;
        } else if (t == DP_VMAX) {
            double a = s_part[DP_VMAX], b = s_part[DP_VID];
            for (int q = 1; q < f.nparts; ++q) {
                const double c = s_part[q * kDiagPartStride + DP_VMAX], d = s_part[q * kDiagPartStride + DP_VID];
                if (c > a || (c == a && d < b)) { a = c; b = d; }
            }
            s_res[DP_VMAX] = a; s_res[DP_VID] = b;
        }
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    if (due) {
        double *row = out + (size_t)(count % rows) * kDiagSlots;
        const double nd = (double)f.n, nan = __longlong_as_double(0x7ff8000000000000ll);
        row[0] = ds->sim_time;
        row[1] = (double)step_dt(f.dt);
        row[2] = (double)step;
        row[3] = nd;
        row[4] = nd * f.m;
        for (int a = 0; a < 6; ++a) row[5 + a] = f.m * s_res[a];
        row[11] = 0.5 * f.m * s_res[6];
        row[12] = -f.m * s_res[7];
        for (int a = 0; a < 3; ++a) row[13 + a] = s_res[8 + a] / nd;
        row[16] = s_res[DP_VMAX];
        row[17] = s_res[DP_VID];
        for (int a = 0; a < 6; ++a) row[18 + a] = s_res[DP_MIN + a];
        row[24] = f.have_rho ? s_res[DP_RHO_MIN] : nan;
        row[25] = f.have_rho ? s_res[DP_RHO_MAX] : nan;
        row[26] = f.have_rho ? s_res[11] / nd : nan;
        for (int a = 27; a < kDiagSlots; ++a) row[a] = 0.0;
    }
    if (ctl) {
        ctl->since = since + 1;
        ctl->step = step;
        if (due) ctl->count = count + 1;
    }
}

}  // namespace sph
