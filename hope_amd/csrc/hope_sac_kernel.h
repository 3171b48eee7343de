// hope_sac_kernel.h -- the device side of SAC's update (include/hope_env.h "SAC's update"; rule: hope_sac_core.h).
// Single-wave blocks, grid ceil(B / 64), one lane per item; no LDS, no private arrays, no scratch; every store is a vector store.
// vec2: the [B][2] arrays of the call are 8-byte aligned and move as float2, otherwise as two 4-byte words; the results do not
// depend on that.  log_std and log_alpha are read by every lane (wave-uniform addresses).
//
//   k_sac_sample     su_draw: stores action and lp.
//   k_sac_critic     su_critic: stores q_target, g_q1, g_q2, then the wave runs the chunk's two aligned trees with cross-lane moves
//                    (ga_wave_tree; lanes past B hold +0.0) and lane 0 writes the chunk's partials to part[2][chunks].
//   k_sac_seed       su_seed: stores s1 and s2.
//   k_sac_policy     su_policy: stores g_raw, then the chunk's four trees; lane 0 writes part[4][chunks].
//   k_sac_merge<K>   one wave: the K merge trees level by level and in place (ga_merge_wave<K>).  K = 2: lane 0 writes the critic call's
//                    losses[2]; K = 4: the policy call's losses[2], g_log_std[2] and g_log_alpha (float64).
#pragma once
#include "hope_gae_kernel.h"
#include "hope_sac_core.h"

namespace hope {

__device__ __forceinline__ float2 su_pair(const float* __restrict__ p, long long i, int vec2) {
    return vec2 ? ((const float2*)p)[i] : make_float2(p[2 * i], p[2 * i + 1]);
}
__device__ __forceinline__ void su_put_pair(float* __restrict__ p, long long i, int vec2, float x, float y) {
    if (vec2) {
        ((float2*)p)[i] = make_float2(x, y);
    } else {
        p[2 * i] = x;
        p[2 * i + 1] = y;
    }
}

__global__ __launch_bounds__(64) void k_sac_sample(const float* __restrict__ raw, const float* __restrict__ log_std, const float* __restrict__ eps, int batch,
                                                   int vec2, float* __restrict__ action, float* __restrict__ lp) {
    const long long i = (long long)blockIdx.x * SU_CHUNK + threadIdx.x;
    if (i >= batch) return;
    const SuStd s = su_std(log_std[0], log_std[1]);
    const float2 rw = su_pair(raw, i, vec2), ep = su_pair(eps, i, vec2);       // (vec2 is uniform: a kernel argument)
    const SuDraw w = su_draw(rw.x, rw.y, s, ep.x, ep.y);
    su_put_pair(action, i, vec2, (float)w.a0, (float)w.a1);
    lp[i] = (float)w.lp;
}

__global__ __launch_bounds__(64) void k_sac_critic(const float* __restrict__ q1, const float* __restrict__ q2, const float* __restrict__ qt1,
                                                   const float* __restrict__ qt2, const float* __restrict__ next_lp, const float* __restrict__ reward,
                                                   const float* __restrict__ done, const double* __restrict__ log_alpha, double gamma, int batch,
                                                   float* __restrict__ q_target, float* __restrict__ g_q1, float* __restrict__ g_q2, long long chunks,
                                                   double* __restrict__ part) {
    const long long i = (long long)blockIdx.x * SU_CHUNK + threadIdx.x;
    double t0 = 0.0, t1 = 0.0;
    if (i < batch) {
        const double alpha = su_alpha(su_alpha64(log_alpha[0]));
        const SuCritic o = su_critic(q1[i], q2[i], qt1[i], qt2[i], next_lp[i], reward[i], done[i], alpha, gamma, (double)batch);
        q_target[i] = o.y;
        g_q1[i] = o.g1;
        g_q2[i] = o.g2;
        t0 = o.t1; t1 = o.t2;
    }
    t0 = ga_wave_tree(t0);
    t1 = ga_wave_tree(t1);
    if (threadIdx.x == 0 && (long long)blockIdx.x < chunks) {
        part[blockIdx.x] = t0;
        part[chunks + blockIdx.x] = t1;
    }
}

__global__ __launch_bounds__(64) void k_sac_seed(const float* __restrict__ q1, const float* __restrict__ q2, int batch, float* __restrict__ s1,
                                                 float* __restrict__ s2) {
    const long long i = (long long)blockIdx.x * SU_CHUNK + threadIdx.x;
    if (i >= batch) return;
    const SuSeed o = su_seed(q1[i], q2[i], (double)batch);
    s1[i] = o.s1;
    s2[i] = o.s2;
}

__global__ __launch_bounds__(64) void k_sac_policy(const float* __restrict__ raw, const float* __restrict__ log_std, const float* __restrict__ eps,
                                                   const float* __restrict__ q1, const float* __restrict__ q2, const float* __restrict__ g_action,
                                                   const double* __restrict__ log_alpha, double target_entropy, int batch, int vec2,
                                                   float* __restrict__ g_raw, long long chunks, double* __restrict__ part) {
    const long long i = (long long)blockIdx.x * SU_CHUNK + threadIdx.x;
    double t0 = 0.0, t1 = 0.0, t2 = 0.0, t3 = 0.0;
    if (i < batch) {
        const SuStd s = su_std(log_std[0], log_std[1]);
        const double alpha = su_alpha(su_alpha64(log_alpha[0]));
        const float2 rw = su_pair(raw, i, vec2), ep = su_pair(eps, i, vec2), G = su_pair(g_action, i, vec2);
        const SuPolicy o = su_policy(rw.x, rw.y, s, ep.x, ep.y, q1[i], q2[i], G.x, G.y, alpha, target_entropy, (double)batch);
        su_put_pair(g_raw, i, vec2, o.g0, o.g1);
        t0 = o.actor; t1 = o.entropy; t2 = o.ls0; t3 = o.ls1;
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

template <int K>
__global__ __launch_bounds__(64) void k_sac_merge(long long nk, double n, double* part, const double* __restrict__ log_alpha, float* __restrict__ losses,
                                                  float* __restrict__ g_log_std, double* __restrict__ g_log_alpha) {
    const int lane = threadIdx.x;
    ga_merge_wave<K>(part, nk, lane);
    if (lane != 0) return;
    losses[0] = su_mean_out(part[0], n);
    if (K == SU_CRITIC_SUMS) {
        losses[1] = su_mean_out(part[nk], n);
    } else {
        const double ga = su_log_alpha_out(su_alpha64(log_alpha[0]), part[nk], n);
        losses[1] = (float)ga;
        g_log_alpha[0] = ga;
        g_log_std[0] = (float)part[2 * nk];
        g_log_std[1] = (float)part[3 * nk];
    }
}

}  // namespace hope
