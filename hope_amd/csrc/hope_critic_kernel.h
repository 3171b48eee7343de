// hope_critic_kernel.h -- the fused inference forward of up to HOPE_CRITIC_SLOTS critic HopeNets on gfx950 (rule: hope_critic_core.h;
// DESIGN.md 5o).  Built from the pieces of hope_policy_kernel.h (pk_gemm, pk_fill, pk_store, pk_row) with a plan of its own.
//
// k_critic_pack     torch's [out][in] tensors -> slot `slot` of the handle's packed buffer, every tensor stored [k][out] (k padded to
//                   even with zero rows), as k_policy_pack does for the policy's 27: here up to 31, the four of the action embedding
//                   empty in a layout without the action token.
// k_critic_forward  blockIdx.x: a tile of 32 scenes, blockIdx.y: the i-th net of the call -- parameter slot slots[i], image token
//                   img[i][batch][128], output out[i][batch]; lidar, target, mask and action are the same for every net.  A workgroup
//                   of four waves owns 32 scenes = T blocks of 32 rows (row = token * 32 + scene), T = 3 + has_img + has_action; every
//                   Linear runs on v_mfma_f32_32x32x2_f32 with the accumulator starting at the bias and k ascending, wave w owning output
//                   columns 32 w .. 32 w + 31; LayerNorm, the softmax block and every tanh are the core's float64 functions on the VALU.
//                   Ownership and order are k_policy_forward's; the LDS plan is not, because T = 5 does not fit that one:
//                     A   the token matrix, T * 32 rows x 129 floats.  The token MLP runs in place: ff1 from A into registers, barrier,
//                         tanh into A, barrier, ff2 from A.
//                     B   THREE per-head tiles q, k, v of T * 32 rows x 33 floats.  The attention output goes onto the q tile: in
//                         pc_attend lane `tid` reads q row `tid` into registers before it writes o row `tid`, and no other lane touches
//                         that row; one more barrier per head keeps the next head's q behind to_out's reads of o.
//                         The inputs (lidar, target, mask, action: 5 568 floats) and the head's hidden tile (4 128) are staged in B.
//                   LDS: (T * 32 * 129 + 3 * T * 32 * 33) * 4 B = 87 552 B (T = 3), 116 736 B (T = 4), 145 920 B (T = 5) of 163 840.
//                   Rows of the last tile past `batch` are computed from zeros and stored nowhere.
#pragma once
#include <hip/hip_runtime.h>

#include "hope_critic_core.h"
#include "hope_policy_kernel.h"

namespace hope {

constexpr int CK_IN_ACTION = PK_IN_MASK + PK_TILE * PK_LD_MASK, CK_LD_ACTION = CC_ACTION + 1;   // behind the policy kernel's input tiles
constexpr int CK_IN_END = CK_IN_ACTION + PK_TILE * CK_LD_ACTION;

constexpr int ck_lds_a(int T) { return T * PK_TILE * PK_LDA; }
constexpr int ck_lds_b(int T) { return 3 * T * PK_TILE * PK_LDH; }
constexpr size_t ck_lds_bytes(int T) { return (size_t)(ck_lds_a(T) + ck_lds_b(T)) * sizeof(float); }
static_assert(CK_IN_END <= ck_lds_b(3) && PK_TILE * PK_LDA <= ck_lds_b(3), "the inputs and the head's hidden tile are staged in buffer B");
static_assert(ck_lds_bytes(5) <= 163840, "a workgroup's LDS");

struct CkPtrs { const float* t[CC_NPARAM]; };
struct CkSlots { int s[HOPE_CRITIC_SLOTS]; };

__global__ __launch_bounds__(256) void k_critic_pack(CkPtrs P, CcLayout L, float* __restrict__ packed, int slot) {
    float* const dst = packed + (long)slot * L.total;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < L.total; i += gridDim.x * blockDim.x) {
        int s = 0;
#pragma unroll 1
        for (int j = 1; j < CC_NPARAM; ++j) s = i >= L.off[j] ? j : s;      // (the empty action tensors are the last and start at L.total: never chosen)
        const int r = i - L.off[s], n = L.n_out[s], k = r / n, o = r - k * n;
        float v = 0.0f;
        if (k < L.k_in[s]) v = P.t[s][(long)o * L.k_in[s] + k];
        dst[i] = v;                                      // (the alignment gap behind a tensor: k >= k_pad >= k_in, zero)
    }
}

template <int T>
__global__ __launch_bounds__(256) void k_critic_forward(const float* __restrict__ packed, CcLayout L, CkSlots slots, int has_img, int has_action,
                                                        const float* __restrict__ lidar, const float* __restrict__ target, const float* __restrict__ mask,
                                                        const float* __restrict__ img, const float* __restrict__ action, long long batch,
                                                        float* __restrict__ out) {
    extern __shared__ float ck_lds[];
    float* const bufA = ck_lds;
    float* const bufB = ck_lds + ck_lds_a(T);
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, lr = lane & 31, lk = lane >> 5;
    const long long s0 = (long long)blockIdx.x * PK_TILE;
    const int rows = (int)(batch - s0 < PK_TILE ? batch - s0 : PK_TILE);          // scenes of this tile, >= 1
    const int n0 = wave * 32, col = n0 + lr;
    const float* __restrict__ const wp = packed + (long)slots.s[blockIdx.y] * L.total;
    if (has_img) img += (long long)blockIdx.y * batch * PC_E;
    out += (long long)blockIdx.y * batch;

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
    if (has_action && tid < PK_TILE * CK_LD_ACTION) {
        const int s = tid / CK_LD_ACTION, k = tid - s * CK_LD_ACTION;
        bufB[CK_IN_ACTION + tid] = (s < rows && k < CC_ACTION) ? action[(s0 + s) * CC_ACTION + k] : 0.0f;
    }
    __syncthreads();

    pk_acc x[T], acc[T];                                  // x: the residual stream, acc: the running layer; tile t = token t, this wave's 32 columns
    // ---- embedding layer 1: h = tanh(W1 in + b1) per token, to buffer A (the action's in the last token's block)
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
        if (T > 3 && has_action) {
            pk_fill<1>(e, wp[L.off[CC_ACTION_B1] + col]);
            pk_gemm<1, 1>(e, bufB + CK_IN_ACTION + lr * CK_LD_ACTION + lk, 0, wp + L.off[CC_ACTION_W1] + lk * PC_E + col, PC_E, 1);
#pragma unroll
            for (int i = 0; i < 16; ++i) bufA[((T - 1) * PK_TILE + pk_row(i, lane)) * PK_LDA + col] = pc_tanh(e[0][i]);
        }
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
    if (T > 3 && has_img) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int s = pk_row(i, lane);
            x[T > 3 ? 3 : 0][i] = s < rows ? img[(s0 + s) * PC_E + col] : 0.0f;
        }
    }
    if (T > 3 && has_action) {
        pk_acc e[1];
        pk_fill<1>(e, wp[L.off[CC_ACTION_B2] + col]);
        pk_gemm<1, 8>(e, bufA + ((T - 1) * PK_TILE + lr) * PK_LDA + lk, 0, wp + L.off[CC_ACTION_W2] + lk * PC_E + col, PC_E, PC_E / 2);
        x[T - 1] = e[0];
    }
    __syncthreads();                                      // layer 1's output has been read
    pk_store<T>(x, bufA, PK_LDA, col, lane);
    __syncthreads();
    if (tid < T * PK_TILE) pc_ln_row(bufA + tid * PK_LDA, wp + L.off[PC_LN1_G], wp + L.off[PC_LN1_B], bufA + tid * PK_LDA);
    __syncthreads();

    // ---- attention, head by head: qkv of the head (waves 0 .. 2), softmax block (o onto q), to_out's next 32 k
    float* const tq = bufB;                               // three [T * 32][33] tiles: q (then o), k, v
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
        if (tid < T * PK_TILE)                            // tid = query token * 32 + scene: the row of the tiles; q row tid is in registers before o row tid is written
            pc_attend<T>(tq + tid * PK_LDH, tq + (T * PK_TILE + (tid & 31)) * PK_LDH, PK_TILE * PK_LDH, tq + (2 * T * PK_TILE + (tid & 31)) * PK_LDH,
                         PK_TILE * PK_LDH, tq + tid * PK_LDH);
        __syncthreads();
        pk_gemm<T, 8>(acc, tq + lr * PK_LDH + lk, PK_TILE * PK_LDH, wp + L.off[PC_OUT_W] + (h * PC_DH + lk) * PC_E + col, PC_E, PC_DH / 2);
        __syncthreads();                                  // o has been read: the next head's q may take its place
    }
#pragma unroll
    for (int t = 0; t < T; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) x[t][i] = x[t][i] + acc[t][i];
    pk_store<T>(x, bufA, PK_LDA, col, lane);              // (the normalised tokens were last read before the loop's last barriers)
    __syncthreads();
    if (tid < T * PK_TILE) pc_ln_row(bufA + tid * PK_LDA, wp + L.off[PC_LN2_G], wp + L.off[PC_LN2_B], bufA + tid * PK_LDA);
    __syncthreads();

    // ---- the token MLP, in place in buffer A
    pk_fill<T>(acc, wp[L.off[PC_FF1_B] + col]);
    pk_gemm<T, 8>(acc, bufA + lr * PK_LDA + lk, PK_TILE * PK_LDA, wp + L.off[PC_FF1_W] + lk * PC_E + col, PC_E, PC_E / 2);
    __syncthreads();                                      // every wave has read the normalised tokens
#pragma unroll
    for (int t = 0; t < T; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) bufA[(t * PK_TILE + pk_row(i, lane)) * PK_LDA + col] = pc_tanh(acc[t][i]);
    __syncthreads();
    pk_fill<T>(acc, wp[L.off[PC_FF2_B] + col]);
    pk_gemm<T, 8>(acc, bufA + lr * PK_LDA + lk, PK_TILE * PK_LDA, wp + L.off[PC_FF2_W] + lk * PC_E + col, PC_E, PC_E / 2);
#pragma unroll
    for (int t = 0; t < T; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) x[t][i] = x[t][i] + acc[t][i];
    __syncthreads();                                      // every wave has read ff1's output
    pk_store<T>(x, bufA, PK_LDA, col, lane);
    __syncthreads();

    // ---- the head: 32 scenes x (T * 128) -> 128, tanh, -> 1
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
    if (tid < rows) out[s0 + tid] = pc_chain(wp[L.off[PC_HEAD2_B]], bufB + tid * PK_LDA, 1, wp + L.off[PC_HEAD2_W], 1, PC_E);
}

}  // namespace hope
