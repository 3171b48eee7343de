/*
 * hope_ring_core.h -- the transition ring of the trainers, one source for host and device.
 *
 * rollout.TransitionRing (the batched ReplayMemory of the reference, src/model/replay_memory.py:6-49) keeps what every scene saw, did
 * and got for the last T steps, and HopeRollout tallies episodes, successes and rewards behind it.  This header pins the push of a
 * column, the tally of the same step and the draw of a SAC batch to ONE rule, so that the kernels (hope_ring_kernel.h) and the host
 * twins rg_before_host / rg_after_host / rg_sample_host give the same bits whatever the launch geometry.
 *
 * Layout (hope_ring_t, all float32, contiguous, caller-owned): lidar [n][T][120], target [n][T][5], action_mask [n][T][42],
 * action [n][T][2], log_prob [n][T][2], reward [n][T], done [n][T].
 *
 * Columns   col(head, size, T, j) = (head - size + j) mod T, non-negative, 0 <= j < size: age j = 0 is the oldest column
 *           (TransitionRing.columns).
 * Push      before half at column t: lidar, target, mask, action, log_prob of every scene, word for word, into [i][t].
 *           after half at column t:  reward[i][t] = (float)reward_in[i] (float32, or float64 rounded to nearest as copy_ does),
 *                                    done[i][t] = (float)done_in[i] (uint8).
 * Tally     counts[0] += #{done_in != 0}, counts[1] += #{status == 2} (int64, exact); reward_sum += step_sum, where step_sum adds
 *           (double)reward_in[i] -- the input, before the rounding to float32 -- in the order of hope_gae_core.h's sums: 64-row
 *           chunks (rows past n count +0.0) in the aligned binary tree, the chunk partials in the aligned tree with pass-through.
 * Sample    batch item b reads the scene s and the age j from the caller's int32 arrays, or draws them:
 *             x_d = mix64(mix64(mix64(seed) ^ counter) ^ (2 b + d)),  d = 0: scene, d = 1: age  (ch_mix64, the chooser's finaliser)
 *             index = (uint32)(((x_d >> 32) * range) >> 32)            integers only; < range; bias at most range / 2^32
 *           t = col(j), newest = (j == size - 1), tn = col(min(j + 1, size - 1));
 *             obs_*  = ring[s][t];  next_* = newest ? last_*[s] : ring[s][tn];  action, reward, done = ring[s][t];
 *             idx[b] = {s, t, newest ? -1 : tn}.
 *           A supplied s outside 0..n-1 or j outside 0..size-1 reads nothing: the item's outputs are +0.0 and idx[b] = {-1, -1, -1}
 *           (flagged, not clamped).
 */
#pragma once
#include <stdint.h>
#include <stdlib.h>

#include "hope_env.h"
#include "hope_math.h"
#include "hope_chooser_core.h"
#include "hope_gae_core.h"

#define RG_LIDAR 120
#define RG_TARGET 5
#define RG_MASK 42
#define RG_PAIR 2                                      /* action, log_prob */
#define RG_OBS (RG_LIDAR + RG_TARGET + RG_MASK)        /* 167 floats of one observation */
#define RG_ROW (RG_OBS + 2 * RG_PAIR)                  /* 171 floats of a before half */
#define RG_ITEM (2 * RG_OBS + RG_PAIR + 2)             /* 338 floats of a batch item */
#define RG_SUCCESS 2                                   /* Status.ARRIVED */

HM_FN int rg_col(int head, int size, int T, int j) {
    const int c = (head - size + j) % T;               /* |head - size + j| < 2 T: no overflow */
    return c < 0 ? c + T : c;
}
HM_FN uint32_t rg_draw(uint64_t seed, uint64_t counter, uint64_t b, int d, uint32_t range) {
    const uint64_t x = ch_mix64(ch_mix64(ch_mix64(seed) ^ counter) ^ (2 * b + (uint64_t)d));
    return (uint32_t)(((x >> 32) * (uint64_t)range) >> 32);
}
HM_FN double rg_reward(const void* reward, int f64, int64_t i) { return f64 ? ((const double*)reward)[i] : (double)((const float*)reward)[i]; }
HM_FN float rg_reward_f32(const void* reward, int f64, int64_t i) { return f64 ? (float)((const double*)reward)[i] : ((const float*)reward)[i]; }

/* where word e (0 .. RG_ROW - 1) of a scene's before half comes from and goes to */
HM_FN void rg_before_word(const hope_ring_t& R, size_t i, size_t cell, const float* lidar, const float* target, const float* mask, const float* action,
                          const float* log_prob, int e) {
    if (e < RG_LIDAR) R.lidar[cell * RG_LIDAR + e] = lidar[i * RG_LIDAR + e];
    else if (e < RG_LIDAR + RG_TARGET) R.target[cell * RG_TARGET + (e - RG_LIDAR)] = target[i * RG_TARGET + (e - RG_LIDAR)];
    else if (e < RG_OBS) R.action_mask[cell * RG_MASK + (e - RG_LIDAR - RG_TARGET)] = mask[i * RG_MASK + (e - RG_LIDAR - RG_TARGET)];
    else if (e < RG_OBS + RG_PAIR) R.action[cell * RG_PAIR + (e - RG_OBS)] = action[i * RG_PAIR + (e - RG_OBS)];
    else R.log_prob[cell * RG_PAIR + (e - RG_OBS - RG_PAIR)] = log_prob[i * RG_PAIR + (e - RG_OBS - RG_PAIR)];
}

/* what a batch item reads: ok = false for a supplied index out of range (then s = t = tn = -1) */
struct RgPick { int s, t, tn; bool newest, ok; };
HM_FN RgPick rg_pick(int n, int T, int head, int size, const int32_t* s_in, const int32_t* j_in, uint64_t seed, uint64_t counter, int64_t b) {
    const int64_t s = s_in ? (int64_t)s_in[b] : (int64_t)rg_draw(seed, counter, (uint64_t)b, 0, (uint32_t)n);
    const int64_t j = j_in ? (int64_t)j_in[b] : (int64_t)rg_draw(seed, counter, (uint64_t)b, 1, (uint32_t)size);
    RgPick p;
    p.ok = s >= 0 && s < n && j >= 0 && j < size;
    p.newest = p.ok && j == size - 1;
    p.s = p.ok ? (int)s : -1;
    p.t = p.ok ? rg_col(head, size, T, (int)j) : -1;
    p.tn = p.ok ? rg_col(head, size, T, (int)(j + 1 < size ? j + 1 : size - 1)) : -1;
    return p;
}
/* word e (0 .. RG_ITEM - 1) of batch item b: obs (167), next_obs (167), action (2), reward, done */
HM_FN void rg_sample_word(const hope_ring_t& R, const float* last_lidar, const float* last_target, const float* last_mask, const hope_ring_batch_t& O,
                          size_t b, RgPick p, int e) {
    const size_t s = (size_t)(p.ok ? p.s : 0), cell = s * (size_t)R.T + (size_t)(p.ok ? p.t : 0);
    if (e < 2 * RG_OBS) {
        const bool nx = e >= RG_OBS, last = nx && p.newest;
        const int k = nx ? e - RG_OBS : e;
        const size_t from = last ? s : (nx ? s * (size_t)R.T + (size_t)(p.ok ? p.tn : 0) : cell);
        if (k < RG_LIDAR)
            (nx ? O.next_lidar : O.obs_lidar)[b * RG_LIDAR + k] = p.ok ? (last ? last_lidar : R.lidar)[from * RG_LIDAR + k] : 0.0f;
        else if (k < RG_LIDAR + RG_TARGET)
            (nx ? O.next_target : O.obs_target)[b * RG_TARGET + (k - RG_LIDAR)] = p.ok ? (last ? last_target : R.target)[from * RG_TARGET + (k - RG_LIDAR)] : 0.0f;
        else
            (nx ? O.next_mask : O.obs_mask)[b * RG_MASK + (k - RG_LIDAR - RG_TARGET)] =
                p.ok ? (last ? last_mask : R.action_mask)[from * RG_MASK + (k - RG_LIDAR - RG_TARGET)] : 0.0f;
    } else if (e < 2 * RG_OBS + RG_PAIR) {
        O.action[b * RG_PAIR + (e - 2 * RG_OBS)] = p.ok ? R.action[cell * RG_PAIR + (e - 2 * RG_OBS)] : 0.0f;
    } else if (e == 2 * RG_OBS + RG_PAIR) {
        O.reward[b] = p.ok ? R.reward[cell] : 0.0f;
    } else {
        O.done[b] = p.ok ? R.done[cell] : 0.0f;
    }
}
/* word e (0 .. 2) of idx[b] */
HM_FN int32_t rg_idx_word(RgPick p, int e) { return e == 0 ? p.s : (e == 1 ? p.t : (p.newest ? -1 : p.tn)); }

static inline bool rg_ring_ok(const hope_ring_t* R) {
    return R && R->lidar && R->target && R->action_mask && R->action && R->log_prob && R->reward && R->done && R->n >= 1 && R->T >= 1;
}
static inline bool rg_batch_ok(const hope_ring_batch_t* O) {
    return O && O->obs_lidar && O->obs_target && O->obs_mask && O->next_lidar && O->next_target && O->next_mask && O->action && O->reward && O->done && O->idx;
}

/* The host twins (no alignment requirements, no upper bound on n, T or batch).  They return HOPE_OK, HOPE_EINVAL or HOPE_ENOMEM;
 * hope_ring_*_host forward to them. */
static inline int rg_before_host(const hope_ring_t* R, int t, const float* lidar, const float* target, const float* mask, const float* action,
                                 const float* log_prob) {
    if (!rg_ring_ok(R) || !lidar || !target || !mask || !action || !log_prob || t < 0 || t >= R->T) return HOPE_EINVAL;
    for (int64_t i = 0; i < R->n; i++)
        for (int e = 0; e < RG_ROW; e++) rg_before_word(*R, (size_t)i, (size_t)i * (size_t)R->T + (size_t)t, lidar, target, mask, action, log_prob, e);
    return HOPE_OK;
}
static inline int rg_after_host(const hope_ring_t* R, int t, const void* reward, int reward_f64, const uint8_t* done, const int32_t* status, int64_t* counts,
                                double* reward_sum) {
    const bool tally = status || counts || reward_sum;
    if (!rg_ring_ok(R) || !reward || !done || t < 0 || t >= R->T || (tally && (!status || !counts || !reward_sum))) return HOPE_EINVAL;
    const int64_t n = R->n, nk = ga_chunks(n);
    double* part = nullptr;
    if (tally && !(part = (double*)malloc((size_t)nk * sizeof(double)))) return HOPE_ENOMEM;
    int64_t episodes = 0, successes = 0;
    for (int64_t k = 0; k < nk; k++) {
        double c[GA_CHUNK];
        for (int l = 0; l < GA_CHUNK; l++) {
            const int64_t i = k * GA_CHUNK + l;
            c[l] = 0.0;
            if (i >= n) continue;
            const size_t cell = (size_t)i * (size_t)R->T + (size_t)t;
            R->reward[cell] = rg_reward_f32(reward, reward_f64, i);
            R->done[cell] = (float)done[i];
            if (!tally) continue;
            c[l] = rg_reward(reward, reward_f64, i);
            episodes += done[i] != 0;
            successes += status[i] == RG_SUCCESS;
        }
        if (!tally) continue;
        ga_chunk_tree(c);
        part[k] = c[0];
    }
    if (!tally) return HOPE_OK;
    ga_merge_tree(part, nk);
    counts[0] += episodes;
    counts[1] += successes;
    reward_sum[0] += part[0];
    free(part);
    return HOPE_OK;
}
static inline int rg_sample_host(const hope_ring_t* R, int head, int size, int64_t batch, const int32_t* s, const int32_t* j, uint64_t seed, uint64_t counter,
                                 const float* last_lidar, const float* last_target, const float* last_mask, const hope_ring_batch_t* O) {
    if (!rg_ring_ok(R) || !rg_batch_ok(O) || !last_lidar || !last_target || !last_mask || (s != nullptr) != (j != nullptr) || head < 0 || head >= R->T ||
        size < 1 || size > R->T || batch < 1)
        return HOPE_EINVAL;
    for (int64_t b = 0; b < batch; b++) {
        const RgPick p = rg_pick(R->n, R->T, head, size, s, j, seed, counter, b);
        for (int e = 0; e < RG_ITEM; e++) rg_sample_word(*R, last_lidar, last_target, last_mask, *O, (size_t)b, p, e);
        for (int e = 0; e < 3; e++) O->idx[3 * b + e] = rg_idx_word(p, e);
    }
    return HOPE_OK;
}
