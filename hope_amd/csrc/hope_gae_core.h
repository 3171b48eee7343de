/*
 * hope_gae_core.h -- PPO's advantage block over [rows][T] float32 tensors, one source for host and device.
 *
 * agent_glue.batched_gae and BatchedPPO.advantages (the reference's PPO.update, src/model/agent/ppo_agent.py:255-273) compute the
 * generalised advantage estimate along T for every scene, the critic's regression target and the advantages' normalisation by their
 * global mean and unbiased standard deviation.  This header pins that block to ONE arithmetic order, so that the kernels
 * (hope_gae_kernel.h) and the host twins ga_host / ga_normalize_host give the same bits whatever the launch geometry: plain IEEE
 * + - * / sqrt, contraction off on both compilers.  Finite inputs are the contract.
 *
 * 1. scan   every row on its own, t = T-1 .. 0, gae = 0 before the first step (ga_step):
 *             nv    = t == T-1 ? v_last[i] : value[i][t+1]
 *             d     = (double)done                                    (0 / 1, as TransitionRing stores it)
 *             delta = (double)(float)(((double)r + (gamma * (1.0 - d)) * (double)nv) - (double)v)
 *             gae   = delta + ((gamma * lam) * gae) * (1.0 - d)
 *             adv[i][t] = (float)gae;   v_target[i][t] = adv[i][t] + value_target[i][t]   (float32)
 *           -- batched_gae operation for operation; no next_value tensor is built.
 * 2. sums   s0 = sum (double)adv, s1 = sum (double)adv * (double)adv over the float32 adv just written:
 *             row    a row adds its own terms in scan order (t descending), from +0.0;
 *             chunk  GA_CHUNK = 64 consecutive rows (rows past `rows` count as +0.0) combine in an aligned binary tree: row i takes
 *                    in row i + h for h = 1, 2, .. 32 where i % 2h == 0;
 *             tree   the chunk partials combine in the aligned binary tree of the observation normalisation (hope_obsnorm_core.h):
 *                    at level h = 1, 2, 4, .. partial i (a multiple of 2h) takes in partial i + h if that one exists, otherwise it
 *                    passes through untouched.
 *           sums = {s0, s1, (double)(rows * T)}: plain sums, so that ranks can add theirs.
 * 3. apply  agents._global_mean_std's formula and the line after it (ga_mean_std, ga_apply):
 *             n = sums[2];  mean = s0 / n;  var = (s1 - n * mean * mean) / max(n - 1, 1)
 *             m = (float)mean;  s = (float)sqrt(max(var, 0));  out = (adv - m) / (s + 1e-5f)   (float32)
 *           A single element has var = 0, so out = 0.
 */
#pragma once
#include <stdint.h>
#include <stdlib.h>

#include "hope_env.h"
#include "hope_math.h"

#define GA_CHUNK 64                                    /* rows per chunk partial: one wave */
#define GA_EPS 1e-5f

/* one time step of one row: gae and the row's two running sums move on; returns adv */
HM_FN float ga_step(float r, float done, float v, float nv, double gamma, double lam, double& gae, double& s0, double& s1, float* delta_out) {
    const double d = (double)done;
    const double x = ((double)r + (gamma * (1.0 - d)) * (double)nv) - (double)v;
    const float df = (float)x;
    if (delta_out) *delta_out = df;
    gae = (double)df + ((gamma * lam) * gae) * (1.0 - d);
    const float a = (float)gae;
    s0 += (double)a;
    s1 += (double)a * (double)a;
    return a;
}
HM_FN bool ga_finite(double x) { return fabs(x) <= 1.7976931348623157e308; }       /* false for NaN and +-inf */
HM_FN int64_t ga_chunks(int64_t rows) { return (rows + GA_CHUNK - 1) / GA_CHUNK; }

struct GaMeanStd { float m, s; };
HM_FN GaMeanStd ga_mean_std(double s0, double s1, double n) {
    const double mean = s0 / n;
    const double nm1 = n - 1.0;
    const double var = (s1 - n * mean * mean) / (nm1 > 1.0 ? nm1 : 1.0);
    GaMeanStd r;
    r.m = (float)mean;
    r.s = (float)sqrt(var > 0.0 ? var : 0.0);
    return r;
}
HM_FN float ga_apply(float a, GaMeanStd ms) { return (a - ms.m) / (ms.s + GA_EPS); }

/* The two trees of step 2 on the host, in place (hope_ring_core.h sums a step's rewards in the same order):
 * ga_chunk_tree: the aligned binary tree over one chunk's GA_CHUNK values, the sum ends in c[0];
 * ga_merge_tree: the aligned binary tree with pass-through over nk chunk partials, the sum ends in p[0]. */
static inline void ga_chunk_tree(double* c) {
    for (int h = 1; h < GA_CHUNK; h *= 2)
        for (int l = 0; l + h < GA_CHUNK; l += 2 * h) c[l] += c[l + h];
}
static inline void ga_merge_tree(double* p, int64_t nk) {
    for (int64_t h = 1; h < nk; h *= 2)                /* level: h = 2^l */
        for (int64_t i = 0; i + h < nk; i += 2 * h) p[i] += p[i + h];
}

/* The host twins (layouts as hope_env_gae / hope_env_adv_normalize; no alignment requirements, no upper bound on rows or T).
 * ga_host: delta_out [rows][T] (may be NULL) takes batched_gae's float32 delta; sums_out (may be NULL) the three doubles.  Returns
 * HOPE_OK, HOPE_EINVAL or HOPE_ENOMEM; hope_gae_host forwards to it. */
static inline int ga_normalize_host(const float* adv, int64_t count, const double* sums, float* out, float* mean_std_out) {
    if (!sums || count < 0 || (count > 0 && (!adv || !out))) return HOPE_EINVAL;
    const GaMeanStd ms = ga_mean_std(sums[0], sums[1], sums[2]);
    if (mean_std_out) { mean_std_out[0] = ms.m; mean_std_out[1] = ms.s; }
    for (int64_t e = 0; e < count; e++) out[e] = ga_apply(adv[e], ms);
    return HOPE_OK;
}
static inline int ga_host(const float* reward, const float* done, const float* value, const float* v_last, const float* value_target, int64_t rows,
                          int64_t T, double gamma, double lam, uint32_t flags, float* adv, float* v_target, double* sums_out, float* delta_out) {
    if (!reward || !done || !value || !v_last || !value_target || !adv || !v_target || rows < 1 || T < 1 || !ga_finite(gamma) || !ga_finite(lam) ||
        (flags & ~(uint32_t)(HOPE_GAE_SUMS | HOPE_GAE_NORMALIZE)))
        return HOPE_EINVAL;
    const bool want_sums = flags & (HOPE_GAE_SUMS | HOPE_GAE_NORMALIZE);
    const int64_t nk = ga_chunks(rows);
    double* part = nullptr;                            /* [2][nk] */
    if (want_sums && !(part = (double*)malloc((size_t)nk * 2 * sizeof(double)))) return HOPE_ENOMEM;
    for (int64_t k = 0; k < nk; k++) {
        double c0[GA_CHUNK], c1[GA_CHUNK];
        for (int l = 0; l < GA_CHUNK; l++) {
            const int64_t i = k * GA_CHUNK + l;
            double gae = 0.0, s0 = 0.0, s1 = 0.0;
            if (i < rows) {
                const size_t b = (size_t)i * (size_t)T;
                float nv = v_last[i];
                for (int64_t t = T - 1; t >= 0; t--) {
                    const float v = value[b + t];
                    const float a = ga_step(reward[b + t], done[b + t], v, nv, gamma, lam, gae, s0, s1, delta_out ? delta_out + b + t : nullptr);
                    adv[b + t] = a;
                    v_target[b + t] = a + value_target[b + t];
                    nv = v;
                }
            }
            c0[l] = s0; c1[l] = s1;
        }
        if (!want_sums) continue;
        ga_chunk_tree(c0);
        ga_chunk_tree(c1);
        part[k] = c0[0]; part[nk + k] = c1[0];
    }
    if (!want_sums) return HOPE_OK;
    ga_merge_tree(part, nk);
    ga_merge_tree(part + nk, nk);
    const double sums[3] = {part[0], part[nk], (double)(rows * T)};
    free(part);
    if (sums_out) { sums_out[0] = sums[0]; sums_out[1] = sums[1]; sums_out[2] = sums[2]; }
    if (flags & HOPE_GAE_NORMALIZE) return ga_normalize_host(adv, rows * T, sums, adv, nullptr);
    return HOPE_OK;
}
