/*
 * hope_ppo_core.h -- PPO's minibatch: the gather by permutation, the clipped loss and its gradients, one source for host and device.
 *
 * The inner loop of BatchedPPO.update (the reference's PPO.update, src/model/agent/ppo_agent.py:278-336) draws a minibatch by index,
 * runs the two networks and differentiates the clipped surrogate and the critic's squared error.  This header pins everything
 * around the two forwards to ONE rule, so that the kernels (hope_ppo_kernel.h) and the host twins pb_gather_host / pb_loss_host give
 * the same bits whatever the launch geometry: plain IEEE + - * /, hm_exp, contraction off on both compilers.  Finite inputs are
 * the contract.
 *
 * Gather    item b takes the flat transition r = index[b] (int64) of the ring (hope_ring_t) viewed as [n T] rows, r = scene T +
 *           column -- what obs[k].reshape(n T, ...)[index] reads:
 *             lidar (120), target (5), action_mask (42), action (2)   word for word
 *             old_lp[b]   = log_prob[r][0] + log_prob[r][1]           one float32 addition: .sum(1) of a pair
 *             adv[b]      = adv_in[r];  v_target[b] = v_target_in[r]  (two float32 [n T] arrays)
 *             idx[b]      = (int32)r
 *           An r outside 0 .. n T - 1 reads nothing: the item's outputs are +0.0 and idx[b] = -1 (flagged, not clamped: the ring's
 *           convention).
 * Loss      float64 throughout, every output rounded to float32 once; exponent arguments are screened as the chooser's (ch_exp).
 *           Inputs: raw [mb][2] (the actor's output before its clamp), log_std ls [2], value [mb], the gathered action x, old_lp,
 *           adv a, v_target, and clip.  Per item (pb_item), d = 0, 1:
 *             mean_d  = raw_d < -1 ? -1 : (raw_d > 1 ? 1 : raw_d)
 *             var_d   = exp(2 ls_d);   e_d = x_d - mean_d
 *             lp      = ((-(e_0 e_0) / (2 var_0) - ls_0) - h) + ((-(e_1 e_1) / (2 var_1) - ls_1) - h),   h = 0.5 ln 2 pi
 *             ratio   = exp(lp - old_lp);   lo = 1 - clip;   hi = 1 + clip
 *             u       = ratio a;   c = (ratio < lo ? lo : (ratio > hi ? hi : ratio)) a
 *             actor term  = -(u < c ? u : c);   critic term = (value - v_target)^2
 *           and torch's autograd rules for them: clamp passes the gradient where lo <= x <= hi, bounds included; the elementwise min
 *           gives the whole gradient to the smaller argument and half to each on a tie:
 *             (w_u, w_c) = u < c ? (1, 0) : (u > c ? (0, 1) : (1/2, 1/2))
 *             dmin    = a (w_u + w_c [lo <= ratio <= hi])              d min / d ratio
 *             k       = -(dmin ratio) / mb                             d loss / d lp
 *             g_raw[b][d]  = [-1 <= raw_d <= 1] ? k (e_d / var_d) : 0
 *             g_value[b]   = (2 (value - v_target)) / mb
 *             log_std term_d = k ((e_d e_d) / var_d - 1)
 *           Outputs: g_raw [mb][2], g_value [mb], g_log_std[d] = sum_b log_std term_d, losses = {(sum actor terms) / mb,
 *           (sum critic terms) / mb}.
 *           The four sums have ONE arithmetic order, that of hope_gae_core.h's sums: every item contributes its term, PB_CHUNK = 64
 *           consecutive items (items past mb count as +0.0) combine in the aligned binary tree (ga_chunk_tree / ga_wave_tree), the
 *           chunk partials in the aligned tree with pass-through (ga_merge_tree / ga_merge_wave).
 */
#pragma once
#include <stdint.h>
#include <stdlib.h>

#include "hope_env.h"
#include "hope_math.h"
#include "hope_chooser_core.h"
#include "hope_gae_core.h"
#include "hope_ring_core.h"

#define PB_CHUNK GA_CHUNK                              /* items per chunk partial: one wave */
#define PB_SUMS 4                                      /* planes of the partials: actor, critic, log_std 0, log_std 1 */
#define PB_COPY (RG_OBS + RG_PAIR)                     /* 169 floats of an item that are copied: lidar, target, mask, action */
#define PB_ITEM (PB_COPY + 4)                          /* + old_lp, adv, v_target, idx */

HM_FN int64_t pb_chunks(int64_t mb) { return (mb + PB_CHUNK - 1) / PB_CHUNK; }
HM_FN bool pb_row_ok(int64_t r, int n, int T) { return r >= 0 && r < (int64_t)n * (int64_t)T; }

/* word e (0 .. PB_ITEM - 1) of item b, from row r of the ring (ok: r is in range) */
HM_FN void pb_gather_word(const hope_ring_t& R, const float* adv, const float* v_target, const hope_ppo_batch_t& O, size_t b, int64_t r, bool ok, int e) {
    const size_t s = (size_t)(ok ? r : 0);
    if (e < RG_LIDAR) O.lidar[b * RG_LIDAR + e] = ok ? R.lidar[s * RG_LIDAR + e] : 0.0f;
    else if (e < RG_LIDAR + RG_TARGET) O.target[b * RG_TARGET + (e - RG_LIDAR)] = ok ? R.target[s * RG_TARGET + (e - RG_LIDAR)] : 0.0f;
    else if (e < RG_OBS) O.mask[b * RG_MASK + (e - RG_LIDAR - RG_TARGET)] = ok ? R.action_mask[s * RG_MASK + (e - RG_LIDAR - RG_TARGET)] : 0.0f;
    else if (e < PB_COPY) O.action[b * RG_PAIR + (e - RG_OBS)] = ok ? R.action[s * RG_PAIR + (e - RG_OBS)] : 0.0f;
    else if (e == PB_COPY) O.old_lp[b] = ok ? R.log_prob[s * RG_PAIR] + R.log_prob[s * RG_PAIR + 1] : 0.0f;
    else if (e == PB_COPY + 1) O.adv[b] = ok ? adv[s] : 0.0f;
    else if (e == PB_COPY + 2) O.v_target[b] = ok ? v_target[s] : 0.0f;
    else O.idx[b] = ok ? (int32_t)r : -1;
}

/* what one item gives: its three gradient words and its four terms */
struct PbItem { float g0, g1, gv; double actor, critic, ls0, ls1; };
HM_FN double pb_clamp1(double x) { return x < -1.0 ? -1.0 : (x > 1.0 ? 1.0 : x); }
HM_FN PbItem pb_item(float raw0, float raw1, double ls0, double ls1, float value, float x0, float x1, float old_lp, float adv, float v_target, double clip,
                     double mb) {
    const double var0 = ch_exp(2.0 * ls0), var1 = ch_exp(2.0 * ls1);
    const double e0 = (double)x0 - pb_clamp1((double)raw0), e1 = (double)x1 - pb_clamp1((double)raw1);
    const double lp = ((-(e0 * e0) / (2.0 * var0) - ls0) - CH_HALF_LN_2PI) + ((-(e1 * e1) / (2.0 * var1) - ls1) - CH_HALF_LN_2PI);
    const double ratio = ch_exp(lp - (double)old_lp);
    const double lo = 1.0 - clip, hi = 1.0 + clip, a = (double)adv;
    const double u = ratio * a;
    const double c = (ratio < lo ? lo : (ratio > hi ? hi : ratio)) * a;
    const double wu = u < c ? 1.0 : (u > c ? 0.0 : 0.5), wc = 1.0 - wu;
    const double in = (ratio >= lo && ratio <= hi) ? 1.0 : 0.0;
    const double dmin = a * (wu + wc * in);
    const double k = -(dmin * ratio) / mb;
    const double dv = (double)value - (double)v_target;
    PbItem o;
    o.g0 = (raw0 >= -1.0f && raw0 <= 1.0f) ? (float)(k * (e0 / var0)) : 0.0f;
    o.g1 = (raw1 >= -1.0f && raw1 <= 1.0f) ? (float)(k * (e1 / var1)) : 0.0f;
    o.gv = (float)((2.0 * dv) / mb);
    o.actor = -(u < c ? u : c);
    o.critic = dv * dv;
    o.ls0 = k * ((e0 * e0) / var0 - 1.0);
    o.ls1 = k * ((e1 * e1) / var1 - 1.0);
    return o;
}
/* the four results from the merged sums: losses[2], g_log_std[2] */
HM_FN float pb_loss_out(double sum, double mb) { return (float)(sum / mb); }

static inline bool pb_batch_ok(const hope_ppo_batch_t* O) {
    return O && O->lidar && O->target && O->mask && O->action && O->old_lp && O->adv && O->v_target && O->idx;
}
HM_FN bool pb_clip_ok(double clip) { return clip >= 0.0 && ga_finite(clip); }              /* false for NaN */

/* The host twins (no alignment requirements, no upper bound on n, T, batch or mb).  They return HOPE_OK, HOPE_EINVAL or HOPE_ENOMEM;
 * hope_ppo_gather_host / hope_ppo_loss_host forward to them. */
static inline int pb_gather_host(const hope_ring_t* R, const float* adv, const float* v_target, const int64_t* index, int64_t batch,
                                 const hope_ppo_batch_t* O) {
    if (!rg_ring_ok(R) || !pb_batch_ok(O) || !adv || !v_target || !index || batch < 1) return HOPE_EINVAL;
    for (int64_t b = 0; b < batch; b++) {
        const int64_t r = index[b];
        const bool ok = pb_row_ok(r, R->n, R->T);
        for (int e = 0; e < PB_ITEM; e++) pb_gather_word(*R, adv, v_target, *O, (size_t)b, r, ok, e);
    }
    return HOPE_OK;
}
static inline int pb_loss_host(const float* raw, const float* log_std, const float* value, const hope_ppo_batch_t* B, int64_t mb, double clip, float* g_raw,
                               float* g_log_std, float* g_value, float* losses) {
    if (!raw || !log_std || !value || !B || !B->action || !B->old_lp || !B->adv || !B->v_target || !g_raw || !g_log_std || !g_value || !losses || mb < 1 ||
        !pb_clip_ok(clip))
        return HOPE_EINVAL;
    const int64_t nk = pb_chunks(mb);
    double* part = (double*)malloc((size_t)nk * PB_SUMS * sizeof(double));       /* [PB_SUMS][nk] */
    if (!part) return HOPE_ENOMEM;
    const double ls0 = (double)log_std[0], ls1 = (double)log_std[1], n = (double)mb;
    for (int64_t k = 0; k < nk; k++) {
        double c[PB_SUMS][PB_CHUNK];
        for (int l = 0; l < PB_CHUNK; l++) {
            const int64_t i = k * PB_CHUNK + l;
            c[0][l] = c[1][l] = c[2][l] = c[3][l] = 0.0;
            if (i >= mb) continue;
            const PbItem o = pb_item(raw[2 * i], raw[2 * i + 1], ls0, ls1, value[i], B->action[2 * i], B->action[2 * i + 1], B->old_lp[i], B->adv[i],
                                     B->v_target[i], clip, n);
            g_raw[2 * i] = o.g0; g_raw[2 * i + 1] = o.g1; g_value[i] = o.gv;
            c[0][l] = o.actor; c[1][l] = o.critic; c[2][l] = o.ls0; c[3][l] = o.ls1;
        }
        for (int q = 0; q < PB_SUMS; q++) { ga_chunk_tree(c[q]); part[q * nk + k] = c[q][0]; }
    }
    for (int q = 0; q < PB_SUMS; q++) ga_merge_tree(part + q * nk, nk);
    losses[0] = pb_loss_out(part[0], n);
    losses[1] = pb_loss_out(part[nk], n);
    g_log_std[0] = (float)part[2 * nk];
    g_log_std[1] = (float)part[3 * nk];
    free(part);
    return HOPE_OK;
}
