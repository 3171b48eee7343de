// hope_chooser_kernel.h -- the device side of the masked action choice (include/hope_env.h "masked choice of the discrete action").
//
//   k_choose<T>   one lane per scene, one wave per block; T = the mask's type (the handle's observation type).  The 64 mask rows of a
//                 wave are ONE contiguous block of 64 x 42 words: the wave loads it coalesced, 16 bytes per lane and instruction
//                 (lane i takes pieces i, i + 64, ...; word by word when the base is not 16-byte aligned), converts to float64 and
//                 stores it into LDS with a row pitch of CH_PITCH = 43 doubles (22 016 B per block).  A lane then walks its own row
//                 -- ch_scene of hope_chooser_core.h, the source the host twin compiles -- without bank conflicts, overwrites
//                 mask_k with e_k (the draw's second pass reads it back) and, when probs is wanted, with e_k / S, which the wave
//                 stores as it loaded the mask: coalesced, out of LDS.  A lane reading its row straight from global memory would
//                 touch 64 different lines per load, 42 times over.  The last block of a batch is partly filled: the cooperative
//                 load / store stop at the batch's last word and lanes past the batch compute and write nothing.
//                 The action table is read through uniform addresses (scalar loads).  No private arrays, no scratch; every store is
//                 a vector store, an action row one 8- or 16-byte store.
#pragma once
#include "hope_chooser_core.h"

namespace hope {

template <class T>
__global__ __launch_bounds__(64) void k_choose(int n, const double* __restrict__ A, const void* __restrict__ mean, const void* __restrict__ log_std,
                                               int ls_stride, int in_f64, const T* __restrict__ mask, const double2* __restrict__ planned,
                                               const uint8_t* __restrict__ executing, const double* __restrict__ u, uint64_t seed, uint64_t counter,
                                               void* __restrict__ action, int act_f64, float2* action_f32, int* __restrict__ idx,
                                               float2* __restrict__ log_prob, double* __restrict__ probs) {
    __shared__ double rows[64 * CH_PITCH];
    constexpr int V = 16 / (int)sizeof(T);                        // words per 16-byte piece
    struct alignas(16) Piece { T w[V]; };
    const int lane = threadIdx.x;
    const int s0 = blockIdx.x * 64;
    const int s = s0 + lane;
    const int n_rows = n - s0 < 64 ? n - s0 : 64;
    const int words = n_rows * CH_NA;                             // of this block: <= 2688
    const T* src = mask + (size_t)s0 * CH_NA;
    if (((uintptr_t)src & 15) == 0) {
        const int pieces = words / V;
        for (int p = lane; p < pieces; p += 64) {
            const Piece q = ((const Piece*)src)[p];
#pragma unroll
            for (int j = 0; j < V; j++) {
                const int w = p * V + j;
                rows[(w / CH_NA) * CH_PITCH + w % CH_NA] = (double)q.w[j];
            }
        }
        for (int w = pieces * V + lane; w < words; w += 64) rows[(w / CH_NA) * CH_PITCH + w % CH_NA] = (double)src[w];
    } else {
        for (int w = lane; w < words; w += 64) rows[(w / CH_NA) * CH_PITCH + w % CH_NA] = (double)src[w];
    }
    __syncthreads();
    if (s < n) {
        double m0, m1, ls0, ls1;
        const size_t l = (size_t)s * (size_t)ls_stride;
        if (in_f64) {
            const double2 m = ((const double2*)mean)[s];
            m0 = m.x; m1 = m.y; ls0 = ((const double*)log_std)[l]; ls1 = ((const double*)log_std)[l + 1];
        } else {
            const float2 m = ((const float2*)mean)[s];
            m0 = m.x; m1 = m.y; ls0 = ((const float*)log_std)[l]; ls1 = ((const float*)log_std)[l + 1];
        }
        const bool ex = executing && executing[s];
        double p0 = 0.0, p1 = 0.0;
        if (ex) { const double2 p = planned[s]; p0 = p.x; p1 = p.y; }
        const double uu = u ? u[s] : ch_uniform(seed, counter, (uint64_t)s);
        const ChOut o = ch_scene(A, m0, m1, ls0, ls1, rows + lane * CH_PITCH, ex, p0, p1, uu, probs != nullptr);
        if (act_f64) ((double2*)action)[s] = make_double2((double)o.a0, (double)o.a1);
        else ((float2*)action)[s] = make_float2(o.a0, o.a1);
        if (action_f32 && (void*)action_f32 != action) action_f32[s] = make_float2(o.a0, o.a1);
        if (idx) idx[s] = o.idx;
        if (log_prob) log_prob[s] = make_float2(o.lp0, o.lp1);
    }
    if (probs) {
        __syncthreads();
        double* dst = probs + (size_t)s0 * CH_NA;
        for (int w = lane; w < words; w += 64) dst[w] = rows[(w / CH_NA) * CH_PITCH + w % CH_NA];
    }
}

}  // namespace hope
