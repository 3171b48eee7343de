// hope_gae_kernel.h -- the device side of PPO's advantage block (include/hope_env.h "PPO's advantage block"; rule: hope_gae_core.h).
// Single-wave blocks, no LDS, no private arrays, no scratch; every store is a vector store.
//
//   k_gae_scan<V>   grid ceil(rows / 64), one lane per row.  The lane walks its row backwards (ga_step), writes adv and v_target and
//                   keeps the row's two sums; the wave then runs the chunk's aligned tree with cross-lane moves (lane i takes in lane
//                   i + h, h = 1 .. 32; lanes past `rows` hold +0.0) and lane 0 writes the chunk's partials to part[2][chunks].  A row
//                   is 4 T contiguous bytes, so over the loop a wave covers 256 T contiguous bytes of every tensor.  V = 4: T % 4 == 0
//                   and 16-byte aligned bases -- four time steps per load and store (float4); V = 1: any T, 4-byte alignment.
//                   part == nullptr: no sums are wanted, the tree is skipped.
//   k_gae_merge     one wave.  The aligned binary tree over the chunk partials, level by level and in place (as k_obsnorm_merge: at
//                   level h lane t adds partial i + h into partial i for i = t 2h, (t + 64) 2h, ...; a partial without a partner is
//                   not touched), a block barrier between levels.  Lane 0 writes sums = {s0, s1, count}.
//   k_adv_apply     one lane per element: reads the three sums, out = (adv - m) / (s + 1e-5f).  out may be adv itself (every lane
//                   reads its element before it writes it and touches no other).
#pragma once
#include "hope_gae_core.h"

namespace hope {

// x of lane + h (the own value past the wave's end: those lanes' results are never used)
__device__ __forceinline__ double ga_down(double x, int h) { return __shfl_down(x, (unsigned)h, 64); }

// the chunk's aligned tree over the wave's 64 values: lane 0 ends with the chunk's sum (ga_chunk_tree's order)
__device__ __forceinline__ double ga_wave_tree(double x) {
#pragma unroll
    for (int h = 1; h < GA_CHUNK; h *= 2) x += ga_down(x, h);
    return x;
}
// the aligned tree with pass-through over K planes of nk chunk partials (plane k at part + k nk), level by level and in place, by one
// wave with a block barrier behind every level (ga_merge_tree's order); plane k's sum ends in part[k nk]
template <int K>
__device__ __forceinline__ void ga_merge_wave(double* part, long long nk, int lane) {
    for (long long h = 1; h < nk; h *= 2) {                       // level: h = 2^l
        for (long long i = (long long)lane * 2 * h; i + h < nk; i += 128 * h) {
#pragma unroll
            for (int k = 0; k < K; k++) part[k * nk + i] += part[k * nk + i + h];
        }
        __syncthreads();
    }
}

template <int V>
__global__ __launch_bounds__(64) void k_gae_scan(const float* __restrict__ reward, const float* __restrict__ done, const float* __restrict__ value,
                                                 const float* __restrict__ v_last, const float* __restrict__ value_target, int rows, int T, double gamma,
                                                 double lam, float* __restrict__ adv, float* __restrict__ v_target, long long chunks,
                                                 double* __restrict__ part) {
    const long long i = (long long)blockIdx.x * GA_CHUNK + threadIdx.x;
    double gae = 0.0, s0 = 0.0, s1 = 0.0;
    if (i < rows) {
        const size_t b = (size_t)i * (size_t)T;
        float nv = v_last[i];
        if (V == 4) {
            const float4* r4 = (const float4*)(reward + b);
            const float4* d4 = (const float4*)(done + b);
            const float4* v4 = (const float4*)(value + b);
            const float4* t4 = (const float4*)(value_target + b);
            float4* a4 = (float4*)(adv + b);
            float4* o4 = (float4*)(v_target + b);
            for (int q = T / 4 - 1; q >= 0; q--) {
                const float4 r = r4[q], d = d4[q], v = v4[q], vt = t4[q];
                float4 a, o;
                a.w = ga_step(r.w, d.w, v.w, nv, gamma, lam, gae, s0, s1, nullptr);
                a.z = ga_step(r.z, d.z, v.z, v.w, gamma, lam, gae, s0, s1, nullptr);
                a.y = ga_step(r.y, d.y, v.y, v.z, gamma, lam, gae, s0, s1, nullptr);
                a.x = ga_step(r.x, d.x, v.x, v.y, gamma, lam, gae, s0, s1, nullptr);
                nv = v.x;
                o.w = a.w + vt.w; o.z = a.z + vt.z; o.y = a.y + vt.y; o.x = a.x + vt.x;
                a4[q] = a;
                o4[q] = o;
            }
        } else {
            for (int t = T - 1; t >= 0; t--) {
                const float v = value[b + t];
                const float a = ga_step(reward[b + t], done[b + t], v, nv, gamma, lam, gae, s0, s1, nullptr);
                adv[b + t] = a;
                v_target[b + t] = a + value_target[b + t];
                nv = v;
            }
        }
    }
    if (!part) return;                                            // (uniform: a kernel argument)
    s0 = ga_wave_tree(s0);
    s1 = ga_wave_tree(s1);
    if (threadIdx.x == 0 && (long long)blockIdx.x < chunks) {
        part[blockIdx.x] = s0;
        part[chunks + blockIdx.x] = s1;
    }
}

__global__ __launch_bounds__(64) void k_gae_merge(long long nk, double count, double* part, double* __restrict__ sums) {
    const int lane = threadIdx.x;
    ga_merge_wave<2>(part, nk, lane);
    if (lane == 0) {
        sums[0] = part[0];
        sums[1] = part[nk];
        sums[2] = count;
    }
}

__global__ __launch_bounds__(64) void k_adv_apply(const float* adv, long long count, const double* __restrict__ sums, float* out) {
    const long long e = (long long)blockIdx.x * 64 + threadIdx.x;
    if (e >= count) return;
    const GaMeanStd ms = ga_mean_std(sums[0], sums[1], sums[2]);
    out[e] = ga_apply(adv[e], ms);
}

}  // namespace hope
