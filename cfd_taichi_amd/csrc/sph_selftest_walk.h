// sph_selftest_walk.h -- self-test of the list walks (sph_selftest_walk): one workgroup stages a one-run plan through stage_operands, then
// every thread walks a list the caller supplies through one of the four walks and one operand source, and reports what its bodies saw.
//   walk 0 sweep_list, 1 sweep_quad, 2 walk_staged, 3 walk_list16
//   src  walks 0 / 1 (memory):  0 SrcP, 1 SrcA, 2 SrcAB, 3 SrcAS, 4 SrcABC
//        walks 2 / 3 (LDS):     0 / 1 StageF4 plain / scaled, 2 / 3 StagePS, 4 / 5 StagePV, 6 StageF4S, 7 StageF4Src + gathered B,
//                               8 StageUpdateP (A, B gathered through the source index, C.xyz staged)
// Per thread: out[0] = body calls, out[1] = h, the order-sensitive hash h = h * 0x9E3779B1 + word over, per call in order, the bits of every
// operand the body received (a tagged entry: the position operand only) and then the rigid flag; the quad walk instead: out[2], out[3] = the
// bits of two accumulators that start at 0.001 and 0 and take a.x and a.y of every call.
#pragma once
#include "sph_pressure_kernels.h"

namespace sph {

constexpr int kWalkTestRows = 24, kWalkTestPitch = kWalkTestRows + 4;     // + the spare group every tile keeps
constexpr int kWalkTestParticles = kBlock, kWalkTestCap = 512;

struct WalkSeen {
    uint32_t h = 0u; int calls = 0;
    __device__ __forceinline__ void word(uint32_t w) { h = h * 0x9E3779B1u + w; }
    __device__ __forceinline__ void f4(const float4 v) { word(__float_as_uint(v.x)); word(__float_as_uint(v.y)); word(__float_as_uint(v.z)); word(__float_as_uint(v.w)); }
};
struct WalkHashBody {
    WalkSeen *st;
    __device__ __forceinline__ void operator()(const float4 a) const { ++st->calls; st->f4(a); st->word(0u); }
    __device__ __forceinline__ void operator()(const float4 a, const float4 b, const uint32_t j) const
    {
        const bool rg = (j & kRigidTag) != 0;
        ++st->calls; st->f4(a);
        if (!rg) st->f4(b);
        st->word(rg ? 1u : 0u);
    }
    __device__ __forceinline__ void operator()(const float4 a, const float s, const uint32_t j) const
    {
        const bool rg = (j & kRigidTag) != 0;
        ++st->calls; st->f4(a);
        if (!rg) st->word(__float_as_uint(s));
        st->word(rg ? 1u : 0u);
    }
    __device__ __forceinline__ void operator()(const float4 a, const float4 b, const float4 cc, const uint32_t j) const
    {
        const bool rg = (j & kRigidTag) != 0;
        ++st->calls; st->f4(a);
        if (!rg) { st->f4(b); st->f4(cc); }
        st->word(rg ? 1u : 0u);
    }
};
struct WalkSumBody {
    float *acc;
    __device__ __forceinline__ void add(const float4 a) const { acc[0] += a.x; acc[1] += a.y; }
    __device__ __forceinline__ void operator()(const float4 a) const { add(a); }
    __device__ __forceinline__ void operator()(const float4 a, const float4, const uint32_t) const { add(a); }
    __device__ __forceinline__ void operator()(const float4 a, const float, const uint32_t) const { add(a); }
    __device__ __forceinline__ void operator()(const float4 a, const float4, const float4, const uint32_t) const { add(a); }
};

template <int WALK, bool RIGID>
__global__ __launch_bounds__(kBlock) void k_selftest_walk(int src, const uint2 *__restrict__ runs, const int *__restrict__ plan_cnt,
                                                          const float4 *__restrict__ A, const float4 *__restrict__ B, const float4 *__restrict__ C,
                                                          const float *__restrict__ S, RigidView rv, const uint32_t *__restrict__ nl,
                                                          const int *__restrict__ cnt, uint32_t *__restrict__ out)
{
    extern __shared__ float4 s_operand[];
    constexpr bool QUAD = WALK == 1;
    constexpr int cap = kWalkTestCap;
    const int t = (int)(blockIdx.x * kBlock + threadIdx.x);
    const int i = QUAD ? t >> 2 : t, q = QUAD ? (t & 3) : 0;
    const uint32_t *nlp = nl + nl_index(i, 0, kWalkTestPitch);
    const int kf = cnt[i];
    WalkSeen st;
    float acc[2] = {0.001f, 0.f};
    auto run = [&](const auto &s) {
        if constexpr (WALK == 0) sweep_list<RIGID>(s, nlp, kf, WalkHashBody{&st}, rv);
        else if constexpr (WALK == 1) sweep_quad<RIGID>(s, nlp, kf, q, acc, WalkSumBody{acc}, rv);
        else if constexpr (WALK == 2) walk_staged<RIGID>(s, nlp, kf, WalkHashBody{&st}, rv);
        else walk_list16(s, nlp, kf, WalkHashBody{&st});
    };
    if constexpr (WALK < 2) {
        switch (src) {
        case 0: if constexpr (!RIGID) run(SrcP{A}); break;
        case 1: run(SrcA{A}); break;
        case 2: run(SrcAB{A, B}); break;
        case 3: run(SrcAS{A, S}); break;
        default: run(SrcABC{A, B, C}); break;
        }
    } else {
        const StagePlan plan{runs, plan_cnt, 0};
        auto staged = [&](const auto &lay) { stage_operands(lay, plan); run(lay); };
        switch (src) {
        case 0: staged(StageF4<false>{s_operand, A}); break;
        case 1: staged(StageF4<true>{s_operand, A}); break;
        case 2: staged(StagePS<false>{s_operand, A, S}); break;
        case 3: staged(StagePS<true>{s_operand, A, S}); break;
        case 4: staged(StagePV<false>{s_operand, StagePV<>::second(s_operand, cap), A, B, nullptr}); break;
        case 5: staged(StagePV<true>{s_operand, StagePV<>::second(s_operand, cap), A, B, nullptr}); break;
        case 6: staged(StageF4S{s_operand, StageF4S::second(s_operand, cap), A, S}); break;
        case 7: {
            const StageF4Src lay{{s_operand, A}, StageF4Src::second(s_operand, cap)};
            stage_operands(lay, plan);
            run(lay.gather(B));
            break;
        }
        default: {                                           // the set k_ii_update_p stages by hand, filled the way it fills it
            uint32_t *s_src = StageF4Src::second(s_operand, cap);
            float *s_ex = reinterpret_cast<float *>(s_src + cap), *s_ey = s_ex + cap, *s_ez = s_ey + cap;
            const int nst = stage_expand(runs, plan_cnt, 0, s_src);
            for (int e = threadIdx.x; e < nst; e += kBlock) {
                const uint32_t j = s_src[e];
                const float4 ev = C[j];
                s_operand[e] = A[j];
                s_ex[e] = ev.x; s_ey[e] = ev.y; s_ez[e] = ev.z;
            }
            __syncthreads();
            run(StageUpdateP{s_operand, s_src, s_ex, s_ey, s_ez, B});
            break;
        }
        }
    }
    out[4 * t + 0] = (uint32_t)st.calls; out[4 * t + 1] = st.h;
    out[4 * t + 2] = __float_as_uint(acc[0]); out[4 * t + 3] = __float_as_uint(acc[1]);
}

// sph_selftest_walk_bits: walk_list16 with a bits stream on one workgroup.  Every thread walks its 16-bit list (entries = indices into A, A[j].x = j)
// and reports, per body call in order, seen[k] = entry | (field & 0xff) << 16 (the field sign-extended as the body received it), and its call count.
//   write == 0 (kBitsRead): the fields come from the caller's words;  write == 1 (kBitsWrite): body k records verdict[k] and the words the walk stored come back
__global__ __launch_bounds__(kBlock) void k_selftest_walk_bits(int write, const float4 *__restrict__ A, const uint32_t *__restrict__ nl, const int *__restrict__ cnt,
                                                               uint32_t *__restrict__ bits, const int *__restrict__ verdict, uint32_t *__restrict__ seen,
                                                               int *__restrict__ calls)
{
    const int i = (int)threadIdx.x;
    const uint32_t *nlp = nl + nl_index(i, 0, kWalkTestPitch);
    uint32_t *bp = bits + (nl_index(i, 0, kWalkTestPitch) >> 2);
    const int kf = cnt[i];
    int n = 0;
    uint32_t *mine = seen + (size_t)i * kWalkTestRows;
    const int *want = verdict + (size_t)i * kWalkTestRows;
    const SrcA src{A};
    if (write) walk_list16<kBitsWrite>(src, nlp, kf, [&](const float4 a, const float4, const auto f) { if (n < kWalkTestRows) { mine[n] = (uint32_t)a.x; f.root(want[n]); } ++n; }, bp);
    else walk_list16<kBitsRead>(src, nlp, kf, [&](const float4 a, const float4, const auto f) { if (n < kWalkTestRows) mine[n] = (uint32_t)a.x | ((uint32_t)f.root() & 0xffu) << 16; ++n; }, (const uint32_t *)bp);
    calls[i] = n;
}

}  // namespace sph
