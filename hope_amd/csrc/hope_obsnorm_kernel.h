// hope_obsnorm_kernel.h -- the device side of the observation normalisation (include/hope_env.h "normalisation of the observations";
// rule: hope_obsnorm_core.h).  T = the observation's type (float or double).  Single-wave blocks, no LDS, no private arrays, no
// scratch; every store is a vector store.
//
//   k_obsnorm_partial<T>  grid (chunks, 2): one wave per 64-row chunk and column half, lane = column (block y = 1 takes columns
//                         64 .. 124: 61 lanes).  on_chunk walks the chunk's rows twice -- sum, then centred squares -- and in both a
//                         wave's load is one row's 64 consecutive words (the second pass re-reads L2).  Writes count, mean_c, M2_c to
//                         part[column][3][stride] at index `chunk`: one column's partials of one kind are contiguous.
//   k_obsnorm_merge<T>    125 blocks, one per column.  The aligned binary tree of the rule, level by level and in place over the
//                         column's partials: at level l lane t merges partial i + 2^l into partial i for i = t 2^(l+1), (t + 64)
//                         2^(l+1), ...; a partial without a partner is not touched.  The levels are separated by a block barrier (the
//                         column's partials are written and read by this one wave only).  Lane 0 then merges the root into the running
//                         state -- or, for the first sample, into (1, row 0, 0) -- and writes mean, S, std of its column.  n_state is
//                         an argument: no kernel reads a count that another block is writing.
//   k_obsnorm_apply<T>    one lane per element of lidar [rows][120] followed by target [rows][5]: coalesced reads and float32 writes;
//                         mean and std of the column come from the 3 x 125 state block (cache resident).
#pragma once
#include "hope_obsnorm_core.h"

namespace hope {

template <class T>
__global__ __launch_bounds__(64) void k_obsnorm_partial(const T* __restrict__ lidar, const T* __restrict__ target, long long start, long long m,
                                                        long long stride, double* __restrict__ part) {
    const int c = blockIdx.y * 64 + threadIdx.x;
    const long long k = blockIdx.x;
    const long long left = m - k * ON_CHUNK;
    if (c >= ON_NC || left <= 0 || k >= stride) return;
    const OnPart p = on_chunk(lidar, target, (size_t)(start + k * ON_CHUNK), (int)(left < ON_CHUNK ? left : ON_CHUNK), c);
    double* q = part + (size_t)c * 3 * (size_t)stride + (size_t)k;
    q[0] = p.n;
    q[stride] = p.mean;
    q[2 * stride] = p.S;
}

template <class T>
__global__ __launch_bounds__(64) void k_obsnorm_merge(const T* __restrict__ lidar, const T* __restrict__ target, int first, long long n_state,
                                                      long long nk, long long stride, double* part, double* __restrict__ state) {
    const int c = blockIdx.x;
    const int lane = threadIdx.x;
    if (c >= ON_NC || nk > stride) return;
    double* pn = part + (size_t)c * 3 * (size_t)stride;
    double* pm = pn + stride;
    double* pS = pm + stride;
    for (long long h = 1; h < nk; h *= 2) {                       // level l: h = 2^l
        for (long long i = (long long)lane * 2 * h; i + h < nk; i += 128 * h) {
            OnPart a, b;
            a.n = pn[i]; a.mean = pm[i]; a.S = pS[i];
            b.n = pn[i + h]; b.mean = pm[i + h]; b.S = pS[i + h];
            const OnPart r = on_merge(a, b);
            pn[i] = r.n; pm[i] = r.mean; pS[i] = r.S;
        }
        __syncthreads();
    }
    if (lane == 0) {
        OnPart run;
        double sd;
        if (first) {
            run.n = 1.0; run.mean = on_load(lidar, target, 0, c); run.S = 0.0;
            sd = run.mean;
        } else {
            run.n = (double)n_state; run.mean = state[c]; run.S = state[ON_NC + c];
            sd = state[2 * ON_NC + c];
        }
        if (nk > 0) {
            OnPart root;
            root.n = pn[0]; root.mean = pm[0]; root.S = pS[0];
            run = on_merge(run, root);
            sd = sqrt(run.S / run.n);
        }
        state[c] = run.mean;
        state[ON_NC + c] = run.S;
        state[2 * ON_NC + c] = sd;
    }
}

template <class T>
__global__ __launch_bounds__(64) void k_obsnorm_apply(const T* __restrict__ lidar, const T* __restrict__ target, long long rows,
                                                      const double* __restrict__ state, float* __restrict__ out_lidar, float* __restrict__ out_target) {
    const size_t e = (size_t)blockIdx.x * 64 + threadIdx.x;
    const size_t nl = (size_t)rows * ON_NL, nt = (size_t)rows * ON_NT;
    if (e < nl) {
        const int c = (int)(e % ON_NL);
        out_lidar[e] = on_apply((double)lidar[e], state[c], state[2 * ON_NC + c]);
    } else if (e - nl < nt) {
        const size_t j = e - nl;
        const int c = ON_NL + (int)(j % ON_NT);
        out_target[j] = on_apply((double)target[j], state[c], state[2 * ON_NC + c]);
    }
}

}  // namespace hope
