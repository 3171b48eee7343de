// hope_ring_kernel.h -- the device side of the transition ring (include/hope_env.h "the transition ring"; rule: hope_ring_core.h).
// Single-wave blocks, no LDS, no private arrays, no scratch; every store is a vector store.
//
//   k_ring_before<V>  a wave takes whole scenes, RB_SCENES consecutive ones per block: 171 floats in, 171 floats out at column t.
//                     V = 4: one pass, a lane moves one piece -- lanes 0..29 a float4 of the lidar row (480 B rows: 16-byte aligned
//                     whenever the base is), lanes 30..50 a float2 of the mask row (168 B rows), lanes 51..55 a float of the target
//                     row (20 B rows), lane 56 the action pair, lane 57 the log_prob pair; needs the lidar bases 16-byte and the
//                     mask / action / log_prob bases 8-byte aligned.  V = 1: three passes of 4-byte words (rg_before_word), any base.
//   k_ring_after      grid ceil(n / 64), one lane per scene: the two column stores; with `part` (the tally is wanted) the chunk's done
//                     and success counts by ballot and popcount, the chunk's aligned tree over (double)reward with cross-lane moves
//                     (ga_wave_tree; lanes past n hold +0.0), and lane 0 writes the chunk's partials part[chunk], cnt[2 chunk + {0, 1}].
//   k_ring_tally      one wave: the aligned tree over the reward partials, level by level in place (ga_merge_wave), integer sums of
//                     the counts; lane 0 adds all three into the running totals.
//   k_ring_sample     one wave per batch item: every lane forms the item's pick (s, t, tn, newest: wave-uniform), then the lanes
//                     stream the item's 2 x 167 + 4 floats (rg_sample_word) and lanes 0..2 write idx[b].
#pragma once
#include "hope_gae_kernel.h"
#include "hope_ring_core.h"

namespace hope {

constexpr int RB_SCENES = 4;                                      // scenes per block of k_ring_before

template <int V>
__global__ __launch_bounds__(64) void k_ring_before(hope_ring_t R, int t, const float* __restrict__ lidar, const float* __restrict__ target,
                                                    const float* __restrict__ mask, const float* __restrict__ action, const float* __restrict__ log_prob) {
    const int lane = threadIdx.x;
    const long long i0 = (long long)blockIdx.x * RB_SCENES;
#pragma unroll
    for (int q = 0; q < RB_SCENES; q++) {
        const long long i = i0 + q;
        if (i >= R.n) return;                                     // (uniform)
        const size_t cell = (size_t)i * (size_t)R.T + (size_t)t;
        if (V == 4) {
            if (lane < 30) {
                ((float4*)(R.lidar + cell * RG_LIDAR))[lane] = ((const float4*)(lidar + (size_t)i * RG_LIDAR))[lane];
            } else if (lane < 51) {
                ((float2*)(R.action_mask + cell * RG_MASK))[lane - 30] = ((const float2*)(mask + (size_t)i * RG_MASK))[lane - 30];
            } else if (lane < 56) {
                R.target[cell * RG_TARGET + (lane - 51)] = target[(size_t)i * RG_TARGET + (lane - 51)];
            } else if (lane == 56) {
                *(float2*)(R.action + cell * RG_PAIR) = *(const float2*)(action + (size_t)i * RG_PAIR);
            } else if (lane == 57) {
                *(float2*)(R.log_prob + cell * RG_PAIR) = *(const float2*)(log_prob + (size_t)i * RG_PAIR);
            }
        } else {
            for (int e = lane; e < RG_ROW; e += 64) rg_before_word(R, (size_t)i, cell, lidar, target, mask, action, log_prob, e);
        }
    }
}

__global__ __launch_bounds__(64) void k_ring_after(hope_ring_t R, int t, const void* __restrict__ reward, int reward_f64, const uint8_t* __restrict__ done,
                                                   const int32_t* __restrict__ status, long long chunks, double* __restrict__ part, int32_t* __restrict__ cnt) {
    const long long i = (long long)blockIdx.x * GA_CHUNK + threadIdx.x;
    const bool in = i < R.n;
    double r = 0.0;
    bool dn = false, ok = false;
    if (in) {
        const size_t cell = (size_t)i * (size_t)R.T + (size_t)t;
        const uint8_t d = done[i];
        R.reward[cell] = rg_reward_f32(reward, reward_f64, i);
        R.done[cell] = (float)d;
        if (part) {
            r = rg_reward(reward, reward_f64, i);
            dn = d != 0;
            ok = status[i] == RG_SUCCESS;
        }
    }
    if (!part) return;                                            // (uniform: a kernel argument)
    const int n_done = __popcll(__ballot(dn)), n_ok = __popcll(__ballot(ok));
    r = ga_wave_tree(r);
    if (threadIdx.x == 0 && (long long)blockIdx.x < chunks) {
        part[blockIdx.x] = r;
        *(int2*)(cnt + 2 * (size_t)blockIdx.x) = make_int2(n_done, n_ok);
    }
}

__global__ __launch_bounds__(64) void k_ring_tally(long long nk, double* part, const int32_t* __restrict__ cnt, long long* __restrict__ counts,
                                                   double* __restrict__ reward_sum) {
    const int lane = threadIdx.x;
    long long ep = 0, su = 0;
    for (long long k = lane; k < nk; k += 64) {
        const int2 c = *(const int2*)(cnt + 2 * k);
        ep += c.x;
        su += c.y;
    }
#pragma unroll
    for (int h = 1; h < 64; h *= 2) {                             // integers: any order gives the sum
        ep += __shfl_down(ep, (unsigned)h, 64);
        su += __shfl_down(su, (unsigned)h, 64);
    }
    ga_merge_wave<1>(part, nk, lane);
    if (lane == 0) {
        counts[0] += ep;
        counts[1] += su;
        reward_sum[0] += part[0];
    }
}

__global__ __launch_bounds__(64) void k_ring_sample(hope_ring_t R, int head, int size, const int32_t* __restrict__ s, const int32_t* __restrict__ j,
                                                    unsigned long long seed, unsigned long long counter, const float* __restrict__ last_lidar,
                                                    const float* __restrict__ last_target, const float* __restrict__ last_mask, hope_ring_batch_t O) {
    const long long b = blockIdx.x;
    const int lane = threadIdx.x;
    const RgPick p = rg_pick(R.n, R.T, head, size, s, j, seed, counter, b);      // the same for every lane
    for (int e = lane; e < RG_ITEM; e += 64) rg_sample_word(R, last_lidar, last_target, last_mask, O, (size_t)b, p, e);
    if (lane < 3) O.idx[3 * b + lane] = rg_idx_word(p, lane);
}

}  // namespace hope
