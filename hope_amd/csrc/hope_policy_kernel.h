// hope_policy_kernel.h -- the fused inference forward of HopeNet on gfx950 (rule: hope_policy_core.h).
//
// k_policy_pack     torch's [out][in] tensors -> the handle's packed buffer, every tensor stored [k][out] (k padded to even with zero
//                   rows), so that the forward's B operand (lane l: W[k = k0 + (l >> 5)][n0 + (l & 31)]) is two coalesced 128-byte rows.
// k_policy_forward  a workgroup of four waves owns 32 scenes = T blocks of 32 rows (row = token * 32 + scene).  Every Linear runs on
//                   v_mfma_f32_32x32x2_f32: A = 32 rows x 2 k from LDS, B = 2 k x 32 outputs from the packed weights (L2), the 32 x 32
//                   accumulator tile starts at the bias and takes the steps k ascending -- the core's chain.  Wave w owns output
//                   columns 32 w .. 32 w + 31 of a 128-wide layer for all T row blocks (one B load feeds T matrix steps); in the qkv
//                   stage of head h waves 0, 1, 2 own q, k, v of that head.  The token matrix never leaves the workgroup: it sits in
//                   the accumulator registers (the residual stream) and in LDS (the next layer's A operand); per head q, k, v and the
//                   attention output are four [T * 32][32] LDS tiles, and to_out accumulates head by head in registers, which is the
//                   chain's k order.  LayerNorm (a lane per row), the softmax block (a lane per scene and query token) and every tanh
//                   are the core's float64 functions on the VALU.  Only [batch][out_dim] is written.
//                   LDS: A = T * 32 rows x 129, B = 4 tiles x T * 32 rows x 33 floats: 100 224 B (T = 3), 133 632 B (T = 4).
//                   Rows of the last tile past `batch` are computed from zeros and stored nowhere.
#pragma once
#include <hip/hip_runtime.h>

#include "hope_policy_core.h"

namespace hope {

constexpr int PK_TILE = 32;                              // scenes of a workgroup
constexpr int PK_THREADS = 256;
constexpr int PK_LDA = PC_E + 1;                         // row stride of the token matrix in LDS: odd, ds_read_b32 of 32 rows hits 32 banks
constexpr int PK_LDH = PC_DH + 1;                        // of a per-head tile
constexpr int PK_IN_LIDAR = 0, PK_LD_LIDAR = PC_LIDAR + 1;                       // the inputs' tiles in buffer B, odd strides, zero-padded k
constexpr int PK_IN_TARGET = PK_IN_LIDAR + PK_TILE * PK_LD_LIDAR, PK_LD_TARGET = PC_TARGET + 2;
constexpr int PK_IN_MASK = PK_IN_TARGET + PK_TILE * PK_LD_TARGET, PK_LD_MASK = PC_MASK + 1;

constexpr int pk_lds_a(int T) { return T * PK_TILE * PK_LDA; }
constexpr int pk_lds_b(int T) { return 4 * T * PK_TILE * PK_LDH; }
constexpr size_t pk_lds_bytes(int T) { return (size_t)(pk_lds_a(T) + pk_lds_b(T)) * sizeof(float); }

typedef float pk_acc __attribute__((ext_vector_type(16)));

struct PkPtrs { const float* t[PC_NPARAM]; };

__global__ __launch_bounds__(256) void k_policy_pack(PkPtrs P, PcLayout L, float* __restrict__ packed) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < L.total; i += gridDim.x * blockDim.x) {
        int s = 0;
#pragma unroll 1
        for (int j = 1; j < PC_NPARAM; ++j) s = i >= L.off[j] ? j : s;
        const int r = i - L.off[s], n = L.n_out[s], k = r / n, o = r - k * n;
        float v = 0.0f;
        if (k < L.k_in[s]) v = P.t[s][(long)o * L.k_in[s] + k];
        packed[i] = v;                                   // (the alignment gap behind a tensor: k >= k_pad >= k_in, zero)
    }
}

// acc[r] (r < R: row blocks, `a_blk` floats apart) take `nsteps` matrix steps.  a: this lane's first A element (row l & 31, k = l >> 5),
// w: its first B element (k = l >> 5, column n0 + (l & 31)), `ldw` floats between two k.  The B operands of the next U steps are
// requested before the current U steps run.
template <int R, int U>
__device__ __forceinline__ void pk_gemm(pk_acc (&acc)[R], const float* a, int a_blk, const float* __restrict__ w, int ldw, int nsteps) {
    float b[U];
#pragma unroll
    for (int u = 0; u < U; ++u) b[u] = w[(long)(2 * u) * ldw];
    for (int s0 = 0; s0 < nsteps; s0 += U) {
        const int sn = s0 + U < nsteps ? s0 + U : s0;    // the last round asks for its own operands again: in range, unused
        float bn[U];
#pragma unroll
        for (int u = 0; u < U; ++u) bn[u] = w[(long)(2 * (sn + u)) * ldw];
#pragma unroll
        for (int u = 0; u < U; ++u) {
#pragma unroll
            for (int r = 0; r < R; ++r) acc[r] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[r * a_blk + 2 * (s0 + u)], b[u], acc[r], 0, 0, 0);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) b[u] = bn[u];
    }
}

// element i of a lane's accumulator tile is row (i & 3) + 8 (i >> 2) + 4 (l >> 5), column l & 31
__device__ __forceinline__ int pk_row(int i, int lane) { return (i & 3) + 8 * (i >> 2) + 4 * (lane >> 5); }

template <int R>
__device__ __forceinline__ void pk_fill(pk_acc (&acc)[R], float v) {
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[r][i] = v;
}

// the tiles to LDS: dst + (r * 32 + row) * ld + column
template <int R>
__device__ __forceinline__ void pk_store(const pk_acc (&acc)[R], float* dst, int ld, int col, int lane) {
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int i = 0; i < 16; ++i) dst[(r * PK_TILE + pk_row(i, lane)) * ld + col] = acc[r][i];
}

template <int T>
__global__ __launch_bounds__(256) void k_policy_forward(const float* __restrict__ wp, PcLayout L, const float* __restrict__ lidar, const float* __restrict__ target,
                                                        const float* __restrict__ mask, const float* __restrict__ img, long long batch, int out_dim, int tanh_out,
                                                        float* __restrict__ out) {
    extern __shared__ float pk_lds[];
    float* const bufA = pk_lds;
    float* const bufB = pk_lds + pk_lds_a(T);
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, lr = lane & 31, lk = lane >> 5;
    const long long s0 = (long long)blockIdx.x * PK_TILE;
    const int rows = (int)(batch - s0 < PK_TILE ? batch - s0 : PK_TILE);          // scenes of this tile, >= 1
    const int n0 = wave * 32, col = n0 + lr;

    // ---- the inputs to LDS (flat, coalesced; 4-byte loads: no alignment beyond the element's), zero beyond `rows` and in the k padding
    for (int i = tid; i < PK_TILE * PK_LD_LIDAR; i += PK_THREADS) {
        const int s = i / PK_LD_LIDAR, k = i - s * PK_LD_LIDAR;
        bufB[PK_IN_LIDAR + i] = (s < rows && k < PC_LIDAR) ? lidar[(s0 + s) * PC_LIDAR + k] : 0.0f;
    }
    for (int i = tid; i < PK_TILE * PK_LD_TARGET; i += PK_THREADS) {
        const int s = i / PK_LD_TARGET, k = i - s * PK_LD_TARGET;
        bufB[PK_IN_TARGET + i] = (s < rows && k < PC_TARGET) ? target[(s0 + s) * PC_TARGET + k] : 0.0f;
    }
    for (int i = tid; i < PK_TILE * PK_LD_MASK; i += PK_THREADS) {
        const int s = i / PK_LD_MASK, k = i - s * PK_LD_MASK;
        bufB[PK_IN_MASK + i] = (s < rows && k < PC_MASK) ? mask[(s0 + s) * PC_MASK + k] : 0.0f;
    }
    __syncthreads();

    pk_acc x[T], acc[T];                                  // x: the residual stream, acc: the running layer; tile t = token t, this wave's 32 columns
    // ---- embedding layer 1: h = tanh(W1 in + b1) per token, to buffer A
    {
        pk_acc e[1];
        pk_fill<1>(e, wp[L.off[PC_LIDAR_W1 + 1] + col]);
        pk_gemm<1, 4>(e, bufB + PK_IN_LIDAR + lr * PK_LD_LIDAR + lk, 0, wp + L.off[PC_LIDAR_W1] + lk * PC_E + col, PC_E, 60);
        acc[0] = e[0];
        pk_fill<1>(e, wp[L.off[PC_TARGET_W1 + 1] + col]);
        pk_gemm<1, 3>(e, bufB + PK_IN_TARGET + lr * PK_LD_TARGET + lk, 0, wp + L.off[PC_TARGET_W1] + lk * PC_E + col, PC_E, 3);
        acc[1] = e[0];
        pk_fill<1>(e, wp[L.off[PC_MASK_W1 + 1] + col]);
        pk_gemm<1, 7>(e, bufB + PK_IN_MASK + lr * PK_LD_MASK + lk, 0, wp + L.off[PC_MASK_W1] + lk * PC_E + col, PC_E, 21);
        acc[2] = e[0];
#pragma unroll
        for (int t = 0; t < 3; ++t)
#pragma unroll
            for (int i = 0; i < 16; ++i) bufA[(t * PK_TILE + pk_row(i, lane)) * PK_LDA + col] = pc_tanh(acc[t][i]);
    }
    __syncthreads();
    // ---- embedding layer 2: the tokens, in registers; the image token as given
#pragma unroll
    for (int t = 0; t < 3; ++t) {
        pk_acc e[1];
        pk_fill<1>(e, wp[L.off[4 * t + 3] + col]);
        pk_gemm<1, 8>(e, bufA + (t * PK_TILE + lr) * PK_LDA + lk, 0, wp + L.off[4 * t + 2] + lk * PC_E + col, PC_E, PC_E / 2);
        x[t] = e[0];
    }
    if (T == 4) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int s = pk_row(i, lane);
            x[T - 1][i] = s < rows ? img[(s0 + s) * PC_E + col] : 0.0f;
        }
    }
    __syncthreads();                                      // layer 1's output has been read
    pk_store<T>(x, bufA, PK_LDA, col, lane);
    __syncthreads();
    if (tid < T * PK_TILE) pc_ln_row(bufA + tid * PK_LDA, wp + L.off[PC_LN1_G], wp + L.off[PC_LN1_B], bufA + tid * PK_LDA);
    __syncthreads();

    // ---- attention, head by head: qkv of the head (waves 0 .. 2), softmax block, to_out's next 32 k
    float* const tq = bufB;                               // four [T * 32][33] tiles: q, k, v, o
    float* const to = bufB + 3 * T * PK_TILE * PK_LDH;
    pk_fill<T>(acc, wp[L.off[PC_OUT_B] + col]);
#pragma unroll 1
    for (int h = 0; h < PC_HEADS; ++h) {
        if (wave < 3) {
            pk_acc q[T];
            pk_fill<T>(q, 0.0f);
            pk_gemm<T, 8>(q, bufA + lr * PK_LDA + lk, PK_TILE * PK_LDA, wp + L.off[PC_QKV_W] + lk * PC_QKV + wave * PC_INNER + h * PC_DH + lr, PC_QKV, PC_E / 2);
            pk_store<T>(q, tq + wave * T * PK_TILE * PK_LDH, PK_LDH, lr, lane);
        }
        __syncthreads();
        if (tid < T * PK_TILE)                            // tid = query token * 32 + scene: the row of the tiles
            pc_attend<T>(tq + tid * PK_LDH, tq + (T * PK_TILE + (tid & 31)) * PK_LDH, PK_TILE * PK_LDH, tq + (2 * T * PK_TILE + (tid & 31)) * PK_LDH,
                         PK_TILE * PK_LDH, to + tid * PK_LDH);
        __syncthreads();
        pk_gemm<T, 8>(acc, to + lr * PK_LDH + lk, PK_TILE * PK_LDH, wp + L.off[PC_OUT_W] + (h * PC_DH + lk) * PC_E + col, PC_E, PC_DH / 2);
    }
#pragma unroll
    for (int t = 0; t < T; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) x[t][i] = x[t][i] + acc[t][i];
    pk_store<T>(x, bufA, PK_LDA, col, lane);              // (the normalised tokens were last read before the loop's last barrier)
    __syncthreads();
    if (tid < T * PK_TILE) pc_ln_row(bufA + tid * PK_LDA, wp + L.off[PC_LN2_G], wp + L.off[PC_LN2_B], bufA + tid * PK_LDA);
    __syncthreads();

    // ---- the token MLP
    pk_fill<T>(acc, wp[L.off[PC_FF1_B] + col]);
    pk_gemm<T, 8>(acc, bufA + lr * PK_LDA + lk, PK_TILE * PK_LDA, wp + L.off[PC_FF1_W] + lk * PC_E + col, PC_E, PC_E / 2);
#pragma unroll
    for (int t = 0; t < T; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) bufB[(t * PK_TILE + pk_row(i, lane)) * PK_LDA + col] = pc_tanh(acc[t][i]);
    __syncthreads();
    pk_fill<T>(acc, wp[L.off[PC_FF2_B] + col]);
    pk_gemm<T, 8>(acc, bufB + lr * PK_LDA + lk, PK_TILE * PK_LDA, wp + L.off[PC_FF2_W] + lk * PC_E + col, PC_E, PC_E / 2);
#pragma unroll
    for (int t = 0; t < T; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) x[t][i] = x[t][i] + acc[t][i];
    pk_store<T>(x, bufA, PK_LDA, col, lane);              // (every wave is past the barrier behind its own reads of buffer A)
    __syncthreads();

    // ---- the head: 32 scenes x (T * 128) -> 128, tanh, -> out_dim
    {
        pk_acc e[1];
        pk_fill<1>(e, wp[L.off[PC_HEAD1_B] + col]);
#pragma unroll 1
        for (int t = 0; t < T; ++t)
            pk_gemm<1, 8>(e, bufA + (t * PK_TILE + lr) * PK_LDA + lk, 0, wp + L.off[PC_HEAD1_W] + (t * PC_E + lk) * PC_E + col, PC_E, PC_E / 2);
#pragma unroll
        for (int i = 0; i < 16; ++i) bufB[pk_row(i, lane) * PK_LDA + col] = pc_tanh(e[0][i]);
    }
    __syncthreads();
    if (tid < PK_TILE * out_dim) {
        const int s = tid / out_dim, o = tid - s * out_dim;
        const float r = pc_chain(wp[L.off[PC_HEAD2_B] + o], bufB + s * PK_LDA, 1, wp + L.off[PC_HEAD2_W] + o, out_dim, PC_E);
        if (s < rows) out[(s0 + s) * out_dim + o] = tanh_out ? pc_tanh(r) : r;
    }
}

}  // namespace hope
