/*
 * hope_obsnorm_core.h -- running normalisation of the 'lidar' and 'target' observations, one source for host and device.
 *
 * The reference's StateNorm (src/model/state_norm.py:25-47) keeps a running mean / S / std per observation column and feeds
 * (x - mean) / (std + 1e-8) to the networks; agent_glue.BatchedStateNorm is its batched torch form (a parallel merge of the same
 * recurrence, statistics in float64).  This header pins that merge to ONE arithmetic order, so that the kernels
 * (hope_obsnorm_kernel.h) and the host twin on_host / hope_obsnorm_host give the same bits whatever the launch geometry: float64
 * throughout, plain IEEE + - * / sqrt, contraction off on both compilers.
 *
 * State: mean[125], S[125], std[125] (float64; columns 0 .. 119 lidar, 120 .. 124 target) and the integer n_state, which lives on
 * the host -- every call's row count is known there -- and reaches a kernel as an argument.
 *
 * update over `rows` observations (float32 or float64, converted to float64 exactly):
 *   first sample   n_state == 0: row 0 becomes mean AND std, S stays 0, n_state = 1 (state_norm.py:26-31, as BatchedStateNorm
 *                  keeps it); the rest works on rows 1 onwards.
 *   chunks         the remaining m rows are cut into chunks of ON_CHUNK = 64 consecutive rows (the last may be shorter): a function
 *                  of m alone.  Per chunk and column, in row order:  s = sum x;  mean_c = s / count;  M2_c = sum (x - mean_c) *
 *                  (x - mean_c).
 *   on_merge       of partials a and b:  n = na + nb;  d = mb - ma;  mean = ma + d * (nb / n);  S = Sa + Sb + d * d * (na * nb / n)
 *                  -- evaluated left to right as written; the counts are doubles and exact.
 *   tree           chunk partials merge in a fixed aligned binary tree: at level l = 0, 1, ... partial i (a multiple of 2^(l+1))
 *                  absorbs partial i + 2^l if that one exists, otherwise it passes through untouched (no arithmetic).
 *   final          the root is merged into the running (n_state, mean, S), the running state being operand a;  std = sqrt(S / n);
 *                  n_state += m.
 * A one-row call is the Welford step in its merge form: mean + d * (1 / n), S + 0 + d * d * (n_state * 1 / n).
 *
 * normalize:  out = (float)((x - mean[c]) / (std[c] + 1e-8)): float64, a true division, rounded once -- the bits of
 * BatchedStateNorm.normalize(...).float() for the same statistics.  A NaN comes out as the one quiet NaN 0x7FC00000 (which payload
 * an operation hands on is the one thing the two sides do not share).
 */
#pragma once
#include <stdint.h>
#include <stdlib.h>

#include "hope_env.h"
#include "hope_math.h"

#define ON_NL HOPE_OBSNORM_LIDAR                       /* 120 lidar columns */
#define ON_NT HOPE_OBSNORM_TARGET                      /* 5 target columns */
#define ON_NC HOPE_OBSNORM_COLS                        /* 125 */
#define ON_CHUNK 64                                    /* rows per chunk partial */
#define ON_EPS 1e-8

struct OnPart { double n, mean, S; };                  /* count (exact in a double), mean, sum of centred squares */

HM_FN OnPart on_merge(OnPart a, OnPart b) {
    OnPart r;
    r.n = a.n + b.n;
    const double d = b.mean - a.mean;
    r.mean = a.mean + d * (b.n / r.n);
    r.S = a.S + b.S + d * d * (a.n * b.n / r.n);
    return r;
}
HM_FN float on_apply(double x, double mean, double std) {
    const float y = (float)((x - mean) / (std + ON_EPS));
    return y == y ? y : __builtin_bit_cast(float, 0x7FC00000u);
}
/* element (row, c) of the observation: lidar [rows][120] and target [rows][5] are separate arrays */
template <class T>
HM_FN double on_load(const T* lidar, const T* target, size_t row, int c) {
    return c < ON_NL ? (double)lidar[row * ON_NL + (size_t)c] : (double)target[row * ON_NT + (size_t)(c - ON_NL)];
}
/* the partial of rows r0 .. r0 + count - 1 of column c: two passes in row order */
template <class T>
HM_FN OnPart on_chunk(const T* lidar, const T* target, size_t r0, int count, int c) {
    double s = 0.0;
#pragma unroll 8                                       /* (several loads in flight; the additions keep their order) */
    for (int r = 0; r < count; r++) s += on_load(lidar, target, r0 + (size_t)r, c);
    OnPart p;
    p.n = (double)count;
    p.mean = s / p.n;
    p.S = 0.0;
#pragma unroll 8
    for (int r = 0; r < count; r++) {
        const double e = on_load(lidar, target, r0 + (size_t)r, c) - p.mean;
        p.S += e * e;
    }
    return p;
}
HM_FN int64_t on_chunks(int64_t m) { return (m + ON_CHUNK - 1) / ON_CHUNK; }

/* the caller-owned state of the host twin is hope_obsnorm_state (hope_env.h) */
template <class T>
static inline int on_host_t(hope_obsnorm_state* st, const T* lidar, const T* target, int64_t rows, uint32_t flags, float* out_lidar, float* out_target) {
    if (flags & HOPE_OBSNORM_UPDATE) {
        int64_t start = 0;
        if (st->n_state == 0) {
            for (int c = 0; c < ON_NC; c++) { st->mean[c] = st->std[c] = on_load(lidar, target, 0, c); st->S[c] = 0.0; }
            st->n_state = 1;
            start = 1;
        }
        const int64_t m = rows - start, nk = on_chunks(m);
        if (m > 0) {
            OnPart* part = (OnPart*)malloc((size_t)nk * sizeof(OnPart));
            if (!part) return HOPE_ENOMEM;
            for (int c = 0; c < ON_NC; c++) {
                for (int64_t k = 0; k < nk; k++) {
                    const int64_t left = m - k * ON_CHUNK;
                    part[k] = on_chunk(lidar, target, (size_t)(start + k * ON_CHUNK), (int)(left < ON_CHUNK ? left : ON_CHUNK), c);
                }
                for (int64_t h = 1; h < nk; h *= 2)                 /* level l: h = 2^l */
                    for (int64_t i = 0; i + h < nk; i += 2 * h) part[i] = on_merge(part[i], part[i + h]);
                OnPart run;
                run.n = (double)st->n_state; run.mean = st->mean[c]; run.S = st->S[c];
                run = on_merge(run, part[0]);
                st->mean[c] = run.mean; st->S[c] = run.S; st->std[c] = sqrt(run.S / run.n);
            }
            free(part);
            st->n_state += m;
        }
    }
    if (flags & HOPE_OBSNORM_NORMALIZE) {
        for (int64_t r = 0; r < rows; r++) {
            for (int c = 0; c < ON_NL; c++) out_lidar[(size_t)r * ON_NL + c] = on_apply((double)lidar[(size_t)r * ON_NL + c], st->mean[c], st->std[c]);
            for (int c = 0; c < ON_NT; c++)
                out_target[(size_t)r * ON_NT + c] = on_apply((double)target[(size_t)r * ON_NT + c], st->mean[ON_NL + c], st->std[ON_NL + c]);
        }
    }
    return HOPE_OK;
}

/* The host twin (layouts as hope_env_obsnorm; no alignment requirements, no upper bound on rows).  Returns HOPE_OK, HOPE_EINVAL or
 * HOPE_ENOMEM; hope_obsnorm_host forwards to it. */
static inline int on_host(hope_obsnorm_state* st, const void* lidar, const void* target, int64_t rows, int in_f64, uint32_t flags, float* out_lidar,
                          float* out_target) {
    if (!st || !lidar || !target || rows < 1 || st->n_state < 0 || !(flags & (HOPE_OBSNORM_UPDATE | HOPE_OBSNORM_NORMALIZE)) ||
        (flags & ~(uint32_t)(HOPE_OBSNORM_UPDATE | HOPE_OBSNORM_NORMALIZE)) || ((flags & HOPE_OBSNORM_NORMALIZE) && (!out_lidar || !out_target)))
        return HOPE_EINVAL;
    return in_f64 ? on_host_t(st, (const double*)lidar, (const double*)target, rows, flags, out_lidar, out_target)
                  : on_host_t(st, (const float*)lidar, (const float*)target, rows, flags, out_lidar, out_target);
}
