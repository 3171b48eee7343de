// hope_imgenc_kernel.h -- HopeNet's image encoder on gfx950 (rule: hope_imgenc_core.h).  Included behind
// hope_policy_kernel.h, whose accumulator helpers (pk_acc, pk_row, pk_fill, pk_gemm) the head reuses.
//
// k_imgenc_pack   the 14 tensors -> the handle's packed buffer (IE_OFF_*): the convolution tensors as torch holds them, the three
//                 Linear weights [k][out], so that the head's B operand (lane l: W[k0 + (l >> 5)][n0 + (l & 31)]) is two coalesced rows.
// k_imgenc_conv   a workgroup of 512 lanes per image.  The 12 288 bytes go to LDS as float32 pixels in a [3][66][66] tile with a zero
//                 border; a lane per pooled output pixel (two of block 1's 1 024 per lane) walks its 4 x 4 x CIN patch an input channel
//                 at a time (two ds_read_b64 per row) and feeds the 3x3 chains of the 2x2 window and the 1x1 shortcuts of every output
//                 channel, then max, act and the average (ie_block_pixel, the twin's function).  Block 1 goes to a bordered [4][34][34] tile, block 2 reads it: pixel
//                 t & 255, channels 4 (t >> 8) .. + 3 per lane, stored to the features coalesced.  The 464 convolution weights are
//                 read from a uniform base at uniform offsets: scalar loads, scalar operands of v_fma_f32 / v_pk_fma_f32.  LDS 70 768 B
//                 (dynamic): two workgroups per CU.
// k_imgenc_head   a workgroup of four waves owns 32 images.  fc1 on v_mfma_f32_32x32x2_f32: wave w owns columns 64 w .. 64 w + 63 as
//                 two 32 x 32 accumulator tiles that start at the bias and take 1 024 steps, k ascending -- the core's chain.  A: the
//                 features in K-chunks of 128 through two LDS buffers (row stride 129, odd), the next chunk's global loads in flight
//                 while the current one is multiplied; B: from the packed weights (L2), eight steps ahead.  act on the accumulators,
//                 h to LDS (stride 257), then output_mean -> pc_tanh -> re_embed_img.1 with wave w owning columns 32 w .. 32 w + 31.
//                 Rows of the last tile past `batch` are computed from zeros and stored nowhere.  LDS 49 536 B.
#pragma once
#include <hip/hip_runtime.h>

#include "hope_imgenc_core.h"
#include "hope_policy_kernel.h"

namespace hope {

constexpr int IK_CONV_THREADS = 512;
constexpr size_t IK_CONV_LDS = (size_t)(IE_TILE0 + IE_TILE1) * sizeof(float);
constexpr int IK_TILE = 32;                              // images of a head workgroup
constexpr int IK_THREADS = 256;
constexpr int IK_KC = 128;                               // k of a staged chunk of the features
constexpr int IK_LDA = IK_KC + 1;
constexpr int IK_LDH = IE_HID + 1;
constexpr int IK_LDR = IE_E + 1;
constexpr int IK_U = 8;                                  // matrix steps whose B operands are requested together
static_assert(2 * IK_TILE * IK_LDA >= IK_TILE * IK_LDH, "h reuses the two chunk buffers");

struct IkPtrs { const float* t[IE_NPARAM]; };

__global__ __launch_bounds__(256) void k_imgenc_pack(IkPtrs P, float* __restrict__ packed) {
    const IeLayout L = ie_layout();
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < IE_TOTAL; i += gridDim.x * blockDim.x) {
        const float* src = P.t[0];
        int off = 0, n = 0, kin = 0;
#pragma unroll
        for (int j = 1; j < IE_NPARAM; ++j) {
            const bool in = i >= L.off[j];
            src = in ? P.t[j] : src;
            off = in ? L.off[j] : off;
            n = in ? L.n_out[j] : n;
            kin = in ? L.k_in[j] : kin;
        }
        const int r = i - off;
        long at = r;
        if (kin) {
            const int k = r / n, o = r - k * n;
            at = (long)o * kin + k;
        }
        packed[i] = src[at];
    }
}

template <int ACT>
__global__ __launch_bounds__(IK_CONV_THREADS) void k_imgenc_conv(const float* __restrict__ wp, const uint8_t* __restrict__ img, float* __restrict__ feat) {
    extern __shared__ __attribute__((aligned(16))) float ik_conv_lds[];
    float* const t0 = ik_conv_lds;
    float* const t1 = ik_conv_lds + IE_TILE0;
    const int tid = threadIdx.x;
    const long long b = blockIdx.x;

    // ---- the borders of both tiles: zero
    for (int i = tid; i < IE_C0 * 4 * IE_LD0 + IE_C1 * 4 * IE_LD1; i += IK_CONV_THREADS) {
        const bool first = i < IE_C0 * 4 * IE_LD0;
        const int j = first ? i : i - IE_C0 * 4 * IE_LD0, ld = first ? IE_LD0 : IE_LD1;
        const int c = j / (4 * ld), e = j - c * 4 * ld, side = e / ld, q = e - side * ld;      // side 0 top, 1 bottom, 2 left, 3 right
        const int y = side == 0 ? 0 : side == 1 ? ld - 1 : q, x = side == 2 ? 0 : side == 3 ? ld - 1 : q;
        (first ? t0 : t1)[(c * ld + y) * ld + x] = 0.0f;
    }
    // ---- the image: 3 072 words of four pixels, coalesced
    const uint32_t* const src = (const uint32_t*)(img + b * IE_IMG);
    for (int i = tid; i < IE_IMG / 4; i += IK_CONV_THREADS) {
        const uint32_t w = src[i];
        const int c = i >> 10, y = (i >> 4) & 63, x = (i & 15) * 4;
        float* const d = t0 + (c * IE_LD0 + y + 1) * IE_LD0 + x + 1;
        d[0] = ie_pixel((uint8_t)(w & 255u));
        d[1] = ie_pixel((uint8_t)((w >> 8) & 255u));
        d[2] = ie_pixel((uint8_t)((w >> 16) & 255u));
        d[3] = ie_pixel((uint8_t)(w >> 24));
    }
    __syncthreads();
    // ---- block 1: 32 x 32 pooled pixels, two per lane
#pragma unroll 1
    for (int q = tid; q < (IE_S0 / 2) * (IE_S0 / 2); q += IK_CONV_THREADS) {
        const int y = q >> 5, x = q & 31;
        ie_block_pixel<IE_C0, IE_C1, ACT>(t0 + 2 * y * IE_LD0 + 2 * x, IE_LD0, IE_LD0 * IE_LD0, wp + IE_OFF_CONV1_W, wp + IE_OFF_CONV1_B, wp + IE_OFF_SHORT1_W,
                                          wp + IE_OFF_SHORT1_B, t1 + (y + 1) * IE_LD1 + x + 1, IE_LD1 * IE_LD1);
    }
    __syncthreads();
    // ---- block 2: 16 x 16 pooled pixels, the eight channels over two lanes (waves 0 .. 3: channels 0 .. 3, waves 4 .. 7: 4 .. 7)
    {
        const int q = tid & 255, y = q >> 4, x = q & 15;
        const int c0 = __builtin_amdgcn_readfirstlane(tid >> 8) * (IE_C2 / 2);
        ie_block_pixel<IE_C1, IE_C2 / 2, ACT>(t1 + 2 * y * IE_LD1 + 2 * x, IE_LD1, IE_LD1 * IE_LD1, wp + IE_OFF_CONV2_W + c0 * IE_C1 * 9, wp + IE_OFF_CONV2_B + c0,
                                              wp + IE_OFF_SHORT2_W + c0 * IE_C1, wp + IE_OFF_SHORT2_B + c0, feat + b * IE_FEAT + c0 * 256 + q, 256);
    }
}

template <int ACT>
__global__ __launch_bounds__(IK_THREADS) void k_imgenc_head(const float* __restrict__ wp, const float* __restrict__ feat, long long batch, float* __restrict__ token) {
    __shared__ float bufA[2 * IK_TILE * IK_LDA];          // the two chunk buffers; h [32][257] behind fc1
    __shared__ float bufR[IK_TILE * IK_LDR];              // tanh(e) [32][129]
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, lr = lane & 31, lk = lane >> 5;
    const long long s0 = (long long)blockIdx.x * IK_TILE;
    const int rows = (int)(batch - s0 < IK_TILE ? batch - s0 : IK_TILE);          // images of this tile, >= 1

    // this lane's 16 elements of a chunk: element j is row (tid >> 7) + 2 j, k = tid & 127
    const int gk = tid & (IK_KC - 1), gr = tid >> 7;
    float g[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int r = gr + 2 * j;
        g[j] = r < rows ? feat[(s0 + r) * IE_FEAT + gk] : 0.0f;
    }
#pragma unroll
    for (int j = 0; j < 16; ++j) bufA[(gr + 2 * j) * IK_LDA + gk] = g[j];
    __syncthreads();

    // ---- fc1: 1 024 steps into two tiles
    const int col = wave * 64 + lr;
    pk_acc acc[2];
#pragma unroll
    for (int i = 0; i < 16; ++i) { acc[0][i] = wp[IE_OFF_FC1_B + col]; acc[1][i] = wp[IE_OFF_FC1_B + col + 32]; }
    const float* const w = wp + IE_OFF_FC1_W + lk * IE_HID + col;             // step s: w[2 s * 256], w[2 s * 256 + 32]
    float b0[IK_U], b1[IK_U];
#pragma unroll
    for (int u = 0; u < IK_U; ++u) { b0[u] = w[(long)(2 * u) * IE_HID]; b1[u] = w[(long)(2 * u) * IE_HID + 32]; }
    constexpr int CHUNKS = IE_FEAT / IK_KC, STEPS = IK_KC / 2;
#pragma unroll 1
    for (int c = 0; c < CHUNKS; ++c) {
        const float* const a = bufA + (c & 1) * IK_TILE * IK_LDA + lr * IK_LDA + lk;
        if (c + 1 < CHUNKS) {
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const int r = gr + 2 * j;
                g[j] = r < rows ? feat[(s0 + r) * IE_FEAT + (c + 1) * IK_KC + gk] : 0.0f;
            }
        }
#pragma unroll 1
        for (int t0 = 0; t0 < STEPS; t0 += IK_U) {
            const int gs = c * STEPS + t0;
            const int sn = gs + IK_U < IE_FEAT / 2 ? gs + IK_U : gs;              // the last round asks for its own operands again: in range, unused
            float n0[IK_U], n1[IK_U];
#pragma unroll
            for (int u = 0; u < IK_U; ++u) { n0[u] = w[(long)(2 * (sn + u)) * IE_HID]; n1[u] = w[(long)(2 * (sn + u)) * IE_HID + 32]; }
#pragma unroll
            for (int u = 0; u < IK_U; ++u) {
                const float av = a[2 * (t0 + u)];
                acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b0[u], acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b1[u], acc[1], 0, 0, 0);
            }
#pragma unroll
            for (int u = 0; u < IK_U; ++u) { b0[u] = n0[u]; b1[u] = n1[u]; }
        }
        if (c + 1 < CHUNKS) {                                 // the other buffer was last read before the previous barrier
            float* const d = bufA + ((c + 1) & 1) * IK_TILE * IK_LDA;
#pragma unroll
            for (int j = 0; j < 16; ++j) d[(gr + 2 * j) * IK_LDA + gk] = g[j];
        }
        __syncthreads();
    }
    // ---- h = act(fc1) to LDS (every wave is past the barrier behind the last chunk's reads)
    float* const bufH = bufA;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) bufH[pk_row(i, lane) * IK_LDH + col + 32 * t] = ie_act<ACT>(acc[t][i]);
    __syncthreads();
    // ---- e = output_mean(h), r = tanh(e), tok = re_embed_img.1(r): wave w owns columns 32 w .. 32 w + 31
    const int c1 = wave * 32 + lr;
    pk_acc e[1];
    pk_fill<1>(e, wp[IE_OFF_MEAN_B + c1]);
    pk_gemm<1, 8>(e, bufH + lr * IK_LDH + lk, 0, wp + IE_OFF_MEAN_W + lk * IE_E + c1, IE_E, IE_HID / 2);
#pragma unroll
    for (int i = 0; i < 16; ++i) bufR[pk_row(i, lane) * IK_LDR + c1] = pc_tanh(e[0][i]);
    __syncthreads();
    pk_fill<1>(e, wp[IE_OFF_RE_B + c1]);
    pk_gemm<1, 8>(e, bufR + lr * IK_LDR + lk, 0, wp + IE_OFF_RE_W + lk * IE_E + c1, IE_E, IE_E / 2);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int r = pk_row(i, lane);
        if (r < rows) token[(s0 + r) * IE_E + c1] = e[0][i];
    }
}

}  // namespace hope
