/*
 * hope_sac_core.h -- SAC's update around the network forwards: the sampled action, the Q target and the losses' gradients, one source
 * for host and device.
 *
 * BatchedSAC.update (the reference's SACAgent.update, src/model/agent/sac_agent.py:250-337) runs seven network forwards; everything
 * between them is arithmetic on [B][1] and [B][2] tensors.  This header pins that arithmetic to ONE rule, so that the kernels
 * (hope_sac_kernel.h) and the host twins su_sample_host / su_critic_host / su_seed_host / su_policy_host give the same bits whatever
 * the launch geometry: plain IEEE + - * /, ch_exp for every exponential, contraction off on both compilers.  float64 throughout on
 * the float32 inputs; every output is rounded to float32 once, except g_log_alpha, which is float64.  Finite inputs are the contract.
 *
 * Common    B items, d = 0, 1:  ls_d = log_std[d];  sd_d = exp(ls_d);  var_d = exp(2 ls_d);  h = 0.5 ln 2 pi
 *           clamp1(x) = x < -1 ? -1 : (x > 1 ? 1 : x)                                         (pb_clamp1)
 *           alpha64 = exp(log_alpha), log_alpha a float64 scalar read where the other inputs live (no host synchronisation)
 *           alpha   = (double)(float)alpha64: the torch path casts the detached temperature to the reward's dtype
 * Sample    (_sample_action without autograd)  inputs raw [B][2] (the actor's output before its clamp), log_std [2], eps [B][2]:
 *             mean_d = clamp1(raw_d);   z_d = mean_d + sd_d eps_d;   a_d = clamp1(z_d);   e_d = a_d - mean_d
 *             lp     = ((-(e_0 e_0) / (2 var_0) - ls_0) - h) + ((-(e_1 e_1) / (2 var_1) - ls_1) - h)
 *           Outputs: action [B][2] = a, lp [B].
 * Critic    inputs q1, q2 [B] (the critics at the stored action), qt1, qt2 [B] (the target critics at the sampled next action),
 *           next_lp [B], reward, done [B], gamma, log_alpha:
 *             y = reward + ((1 - done) gamma) ((qt1 < qt2 ? qt1 : qt2) - alpha next_lp)
 *           Outputs: q_target = (float)y, g_q1 = (2 (q1 - y)) / B, g_q2 = (2 (q2 - y)) / B (the differences use the unrounded y),
 *           losses = {(sum (q1 - y)^2) / B, (sum (q2 - y)^2) / B}.
 * Seed      the gradient of the actor loss at the two critic outputs, torch's rule for the elementwise min (as pb_item): the whole
 *           gradient to the smaller argument, half to each on a tie:
 *             (w1, w2) = q1 < q2 ? (1, 0) : (q1 > q2 ? (0, 1) : (1/2, 1/2));   s1 = -w1 / B;   s2 = -w2 / B
 * Policy    inputs raw, log_std, eps, q1, q2 [B] (the critics at the sampled action), G [B][2] (what autograd returns at the sampled
 *           action for the seeds), log_alpha, target_entropy.  mean, z, a, e, lp as in Sample; the clamp passes its gradient on the
 *           closed interval, bounds included:  ca_d = [-1 <= z_d <= 1],  cm_d = [-1 <= raw_d <= 1].  With k = alpha / B and
 *           t_d = k (e_d / var_d):
 *             dz_d        = ca_d ? G_d - t_d : 0
 *             g_raw[b][d] = cm_d ? dz_d + t_d : 0
 *             log_std term_d = (dz_d sd_d) eps_d + k ((e_d e_d) / var_d - 1)
 *             actor term  = alpha lp - (q1 < q2 ? q1 : q2);   entropy term = -lp - target_entropy
 *           Outputs: g_raw [B][2], g_log_std[d] = sum_b log_std term_d, losses[0] = (sum actor terms) / B,
 *           g_log_alpha = alpha64 ((sum entropy terms) / B) in float64, losses[1] = (float)g_log_alpha (the value of the temperature
 *           loss).
 * Sums      ONE arithmetic order, that of hope_gae_core.h's sums: every item contributes its term, SU_CHUNK = 64 consecutive items
 *           (items past B count as +0.0) combine in the aligned binary tree (ga_chunk_tree / ga_wave_tree), the chunk partials in
 *           the aligned tree with pass-through (ga_merge_tree / ga_merge_wave).
 */
#pragma once
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "hope_env.h"
#include "hope_math.h"
#include "hope_chooser_core.h"
#include "hope_gae_core.h"
#include "hope_ppo_core.h"

#define SU_CHUNK GA_CHUNK                              /* items per chunk partial: one wave */
#define SU_CRITIC_SUMS 2                               /* planes of the critic call's partials: the two squared errors */
#define SU_POLICY_SUMS 4                               /* of the policy call's: actor, entropy, log_std 0, log_std 1 */
#define SU_SUMS 4                                      /* planes the partials have room for */

HM_FN int64_t su_chunks(int64_t batch) { return (batch + SU_CHUNK - 1) / SU_CHUNK; }
HM_FN double su_alpha64(double log_alpha) { return ch_exp(log_alpha); }
HM_FN double su_alpha(double alpha64) { return (double)(float)alpha64; }

/* what log_std gives every item */
struct SuStd { double ls0, ls1, sd0, sd1, var0, var1; };
HM_FN SuStd su_std(float l0, float l1) {
    SuStd s;
    s.ls0 = (double)l0; s.ls1 = (double)l1;
    s.sd0 = ch_exp(s.ls0); s.sd1 = ch_exp(s.ls1);
    s.var0 = ch_exp(2.0 * s.ls0); s.var1 = ch_exp(2.0 * s.ls1);
    return s;
}

/* the reparameterised sample of one item */
struct SuDraw { double z0, z1, a0, a1, e0, e1, lp; };
HM_FN SuDraw su_draw(float raw0, float raw1, const SuStd& s, float eps0, float eps1) {
    const double m0 = pb_clamp1((double)raw0), m1 = pb_clamp1((double)raw1);
    SuDraw o;
    o.z0 = m0 + s.sd0 * (double)eps0; o.z1 = m1 + s.sd1 * (double)eps1;
    o.a0 = pb_clamp1(o.z0); o.a1 = pb_clamp1(o.z1);
    o.e0 = o.a0 - m0; o.e1 = o.a1 - m1;
    o.lp = ((-(o.e0 * o.e0) / (2.0 * s.var0) - s.ls0) - CH_HALF_LN_2PI) + ((-(o.e1 * o.e1) / (2.0 * s.var1) - s.ls1) - CH_HALF_LN_2PI);
    return o;
}

/* the critic call of one item: its three words and its two terms */
struct SuCritic { float y, g1, g2; double t1, t2; };
HM_FN SuCritic su_critic(float q1, float q2, float qt1, float qt2, float next_lp, float reward, float done, double alpha, double gamma, double n) {
    const double mn = qt1 < qt2 ? (double)qt1 : (double)qt2;
    const double y = (double)reward + ((1.0 - (double)done) * gamma) * (mn - alpha * (double)next_lp);
    const double d1 = (double)q1 - y, d2 = (double)q2 - y;
    SuCritic o;
    o.y = (float)y;
    o.g1 = (float)((2.0 * d1) / n);
    o.g2 = (float)((2.0 * d2) / n);
    o.t1 = d1 * d1;
    o.t2 = d2 * d2;
    return o;
}

/* the seeds of one item */
struct SuSeed { float s1, s2; };
HM_FN SuSeed su_seed(float q1, float q2, double n) {
    const double w1 = q1 < q2 ? 1.0 : (q1 > q2 ? 0.0 : 0.5), w2 = 1.0 - w1;
    SuSeed o;
    o.s1 = (float)(-w1 / n);
    o.s2 = (float)(-w2 / n);
    return o;
}

/* the policy call of one item: its two gradient words and its four terms */
struct SuPolicy { float g0, g1; double actor, entropy, ls0, ls1; };
HM_FN SuPolicy su_policy(float raw0, float raw1, const SuStd& s, float eps0, float eps1, float q1, float q2, float G0, float G1, double alpha,
                         double target_entropy, double n) {
    const SuDraw w = su_draw(raw0, raw1, s, eps0, eps1);
    const double k = alpha / n;
    const double t0 = k * (w.e0 / s.var0), t1 = k * (w.e1 / s.var1);
    const double dz0 = (w.z0 >= -1.0 && w.z0 <= 1.0) ? (double)G0 - t0 : 0.0;
    const double dz1 = (w.z1 >= -1.0 && w.z1 <= 1.0) ? (double)G1 - t1 : 0.0;
    SuPolicy o;
    o.g0 = (raw0 >= -1.0f && raw0 <= 1.0f) ? (float)(dz0 + t0) : 0.0f;
    o.g1 = (raw1 >= -1.0f && raw1 <= 1.0f) ? (float)(dz1 + t1) : 0.0f;
    o.ls0 = (dz0 * s.sd0) * (double)eps0 + k * ((w.e0 * w.e0) / s.var0 - 1.0);
    o.ls1 = (dz1 * s.sd1) * (double)eps1 + k * ((w.e1 * w.e1) / s.var1 - 1.0);
    o.actor = alpha * w.lp - (q1 < q2 ? (double)q1 : (double)q2);
    o.entropy = -w.lp - target_entropy;
    return o;
}
/* the results from the merged sums */
HM_FN float su_mean_out(double sum, double n) { return (float)(sum / n); }
HM_FN double su_log_alpha_out(double alpha64, double sum, double n) { return alpha64 * (sum / n); }

/* a float64 scalar at any address */
static inline double su_load64(const double* p) { double x; memcpy(&x, p, sizeof x); return x; }
static inline void su_store64(double* p, double x) { memcpy(p, &x, sizeof x); }

/* The host twins (no alignment requirements, no upper bound on batch).  They return HOPE_OK, HOPE_EINVAL or HOPE_ENOMEM;
 * hope_sac_*_host forward to them. */
static inline int su_sample_host(const float* raw, const float* log_std, const float* eps, int64_t batch, float* action, float* lp) {
    if (!raw || !log_std || !eps || !action || !lp || batch < 1) return HOPE_EINVAL;
    const SuStd s = su_std(log_std[0], log_std[1]);
    for (int64_t i = 0; i < batch; i++) {
        const SuDraw w = su_draw(raw[2 * i], raw[2 * i + 1], s, eps[2 * i], eps[2 * i + 1]);
        action[2 * i] = (float)w.a0; action[2 * i + 1] = (float)w.a1;
        lp[i] = (float)w.lp;
    }
    return HOPE_OK;
}
static inline int su_critic_host(const float* q1, const float* q2, const float* qt1, const float* qt2, const float* next_lp, const float* reward,
                                 const float* done, const double* log_alpha, double gamma, int64_t batch, float* q_target, float* g_q1, float* g_q2,
                                 float* losses) {
    if (!q1 || !q2 || !qt1 || !qt2 || !next_lp || !reward || !done || !log_alpha || !q_target || !g_q1 || !g_q2 || !losses || batch < 1 || !ga_finite(gamma))
        return HOPE_EINVAL;
    const int64_t nk = su_chunks(batch);
    double* part = (double*)malloc((size_t)nk * SU_CRITIC_SUMS * sizeof(double));       /* [SU_CRITIC_SUMS][nk] */
    if (!part) return HOPE_ENOMEM;
    const double alpha = su_alpha(su_alpha64(su_load64(log_alpha))), n = (double)batch;
    for (int64_t k = 0; k < nk; k++) {
        double c[SU_CRITIC_SUMS][SU_CHUNK];
        for (int l = 0; l < SU_CHUNK; l++) {
            const int64_t i = k * SU_CHUNK + l;
            c[0][l] = c[1][l] = 0.0;
            if (i >= batch) continue;
            const SuCritic o = su_critic(q1[i], q2[i], qt1[i], qt2[i], next_lp[i], reward[i], done[i], alpha, gamma, n);
            q_target[i] = o.y; g_q1[i] = o.g1; g_q2[i] = o.g2;
            c[0][l] = o.t1; c[1][l] = o.t2;
        }
        for (int q = 0; q < SU_CRITIC_SUMS; q++) { ga_chunk_tree(c[q]); part[q * nk + k] = c[q][0]; }
    }
    for (int q = 0; q < SU_CRITIC_SUMS; q++) ga_merge_tree(part + q * nk, nk);
    losses[0] = su_mean_out(part[0], n);
    losses[1] = su_mean_out(part[nk], n);
    free(part);
    return HOPE_OK;
}
static inline int su_seed_host(const float* q1, const float* q2, int64_t batch, float* s1, float* s2) {
    if (!q1 || !q2 || !s1 || !s2 || batch < 1) return HOPE_EINVAL;
    for (int64_t i = 0; i < batch; i++) {
        const SuSeed o = su_seed(q1[i], q2[i], (double)batch);
        s1[i] = o.s1; s2[i] = o.s2;
    }
    return HOPE_OK;
}
static inline int su_policy_host(const float* raw, const float* log_std, const float* eps, const float* q1, const float* q2, const float* g_action,
                                 const double* log_alpha, double target_entropy, int64_t batch, float* g_raw, float* g_log_std, double* g_log_alpha,
                                 float* losses) {
    if (!raw || !log_std || !eps || !q1 || !q2 || !g_action || !log_alpha || !g_raw || !g_log_std || !g_log_alpha || !losses || batch < 1 ||
        !ga_finite(target_entropy))
        return HOPE_EINVAL;
    const int64_t nk = su_chunks(batch);
    double* part = (double*)malloc((size_t)nk * SU_POLICY_SUMS * sizeof(double));       /* [SU_POLICY_SUMS][nk] */
    if (!part) return HOPE_ENOMEM;
    const SuStd s = su_std(log_std[0], log_std[1]);
    const double alpha64 = su_alpha64(su_load64(log_alpha)), alpha = su_alpha(alpha64), n = (double)batch;
    for (int64_t k = 0; k < nk; k++) {
        double c[SU_POLICY_SUMS][SU_CHUNK];
        for (int l = 0; l < SU_CHUNK; l++) {
            const int64_t i = k * SU_CHUNK + l;
            c[0][l] = c[1][l] = c[2][l] = c[3][l] = 0.0;
            if (i >= batch) continue;
            const SuPolicy o = su_policy(raw[2 * i], raw[2 * i + 1], s, eps[2 * i], eps[2 * i + 1], q1[i], q2[i], g_action[2 * i], g_action[2 * i + 1], alpha,
                                         target_entropy, n);
            g_raw[2 * i] = o.g0; g_raw[2 * i + 1] = o.g1;
            c[0][l] = o.actor; c[1][l] = o.entropy; c[2][l] = o.ls0; c[3][l] = o.ls1;
        }
        for (int q = 0; q < SU_POLICY_SUMS; q++) { ga_chunk_tree(c[q]); part[q * nk + k] = c[q][0]; }
    }
    for (int q = 0; q < SU_POLICY_SUMS; q++) ga_merge_tree(part + q * nk, nk);
    const double ga = su_log_alpha_out(alpha64, part[nk], n);
    losses[0] = su_mean_out(part[0], n);
    losses[1] = (float)ga;
    su_store64(g_log_alpha, ga);
    g_log_std[0] = (float)part[2 * nk];
    g_log_std[1] = (float)part[3 * nk];
    free(part);
    return HOPE_OK;
}
