// hope_ppo_kernel.h -- the device side of PPO's minibatch (include/hope_env.h "PPO's minibatch"; rule: hope_ppo_core.h).
// Single-wave blocks, no LDS, no private arrays, no scratch; every store is a vector store.
//
//   k_ppo_gather<V>  one wave per batch item: every lane reads index[b] (wave-uniform), then the lanes move the row.  V = 4: one pass,
//                    a lane moves one piece (k_ring_before<4>'s split) -- lanes 0..29 a float4 of the lidar row (480 B rows: 16-byte
//                    aligned whenever the base is), lanes 30..50 a float2 of the mask row (168 B rows), lanes 51..55 a float of the
//                    target row, lane 56 the action pair, lane 57 the summed log-probability, lanes 58 / 59 adv / v_target, lane 60
//                    idx; needs the lidar bases (ring and out) 16-byte and the mask / action bases and the ring's log_prob 8-byte
//                    aligned.  V = 1: three passes of 4-byte words (pb_gather_word), any base.  A refused row stores zeros through
//                    the same lanes.
//   k_ppo_loss       grid ceil(mb / 64), one lane per item (pb_item): stores g_raw and g_value, then the wave runs the chunk's four
//                    aligned trees with cross-lane moves (ga_wave_tree; lanes past mb hold +0.0) and lane 0 writes the chunk's
//                    partials to part[4][chunks].  vec2: raw, action and g_raw are 8-byte aligned and move as float2.
//   k_ppo_merge      one wave: the four merge trees level by level and in place (ga_merge_wave<4>); lane 0 writes losses[2] and
//                    g_log_std[2].
#pragma once
#include "hope_gae_kernel.h"
#include "hope_ppo_core.h"

namespace hope {

template <int V>
__global__ __launch_bounds__(64) void k_ppo_gather(hope_ring_t R, const float* __restrict__ adv, const float* __restrict__ v_target,
                                                   const int64_t* __restrict__ index, hope_ppo_batch_t O) {
    const size_t b = blockIdx.x;
    const int lane = threadIdx.x;
    const int64_t r = index[b];                                 // the same for every lane
    const bool ok = pb_row_ok(r, R.n, R.T);
    if (V == 4) {
        const size_t s = (size_t)(ok ? r : 0);
        if (lane < 30) {
            ((float4*)(O.lidar + b * RG_LIDAR))[lane] = ok ? ((const float4*)(R.lidar + s * RG_LIDAR))[lane] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        } else if (lane < 51) {
            ((float2*)(O.mask + b * RG_MASK))[lane - 30] = ok ? ((const float2*)(R.action_mask + s * RG_MASK))[lane - 30] : make_float2(0.0f, 0.0f);
        } else if (lane < 56) {
            O.target[b * RG_TARGET + (lane - 51)] = ok ? R.target[s * RG_TARGET + (lane - 51)] : 0.0f;
        } else if (lane == 56) {
            *(float2*)(O.action + b * RG_PAIR) = ok ? *(const float2*)(R.action + s * RG_PAIR) : make_float2(0.0f, 0.0f);
        } else if (lane == 57) {
            const float2 p = ok ? *(const float2*)(R.log_prob + s * RG_PAIR) : make_float2(0.0f, 0.0f);
            O.old_lp[b] = p.x + p.y;
        } else if (lane < 61) {
            pb_gather_word(R, adv, v_target, O, b, r, ok, PB_COPY + 1 + (lane - 58));
        }
    } else {
        for (int e = lane; e < PB_ITEM; e += 64) pb_gather_word(R, adv, v_target, O, b, r, ok, e);
    }
}

__global__ __launch_bounds__(64) void k_ppo_loss(const float* __restrict__ raw, const float* __restrict__ log_std, const float* __restrict__ value,
                                                 const float* __restrict__ action, const float* __restrict__ old_lp, const float* __restrict__ adv,
                                                 const float* __restrict__ v_target, int mb, double clip, int vec2, float* __restrict__ g_raw,
                                                 float* __restrict__ g_value, long long chunks, double* __restrict__ part) {
    const long long i = (long long)blockIdx.x * PB_CHUNK + threadIdx.x;
    double t0 = 0.0, t1 = 0.0, t2 = 0.0, t3 = 0.0;
    if (i < mb) {
        float2 rw, x;
        if (vec2) {                                               // (uniform: a kernel argument)
            rw = ((const float2*)raw)[i];
            x = ((const float2*)action)[i];
        } else {
            rw = make_float2(raw[2 * i], raw[2 * i + 1]);
            x = make_float2(action[2 * i], action[2 * i + 1]);
        }
        const PbItem o = pb_item(rw.x, rw.y, (double)log_std[0], (double)log_std[1], value[i], x.x, x.y, old_lp[i], adv[i], v_target[i], clip, (double)mb);
        if (vec2) {
            ((float2*)g_raw)[i] = make_float2(o.g0, o.g1);
        } else {
            g_raw[2 * i] = o.g0;
            g_raw[2 * i + 1] = o.g1;
        }
        g_value[i] = o.gv;
        t0 = o.actor; t1 = o.critic; t2 = o.ls0; t3 = o.ls1;
    }
    t0 = ga_wave_tree(t0);
    t1 = ga_wave_tree(t1);
    t2 = ga_wave_tree(t2);
    t3 = ga_wave_tree(t3);
    if (threadIdx.x == 0 && (long long)blockIdx.x < chunks) {
        part[blockIdx.x] = t0;
        part[chunks + blockIdx.x] = t1;
        part[2 * chunks + blockIdx.x] = t2;
        part[3 * chunks + blockIdx.x] = t3;
    }
}

__global__ __launch_bounds__(64) void k_ppo_merge(long long nk, double mb, double* part, float* __restrict__ losses, float* __restrict__ g_log_std) {
    const int lane = threadIdx.x;
    ga_merge_wave<PB_SUMS>(part, nk, lane);
    if (lane == 0) {
        losses[0] = pb_loss_out(part[0], mb);
        losses[1] = pb_loss_out(part[nk], mb);
        g_log_std[0] = (float)part[2 * nk];
        g_log_std[1] = (float)part[3 * nk];
    }
}

}  // namespace hope
