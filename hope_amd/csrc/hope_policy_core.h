/*
 * hope_policy_core.h -- the inference forward of HopeNet (hope_amd/policy.py; the reference's MultiObsEmbedding with its attention
 * trunk, src/model/network.py:34-187, src/model/attention.py:7-94) in ONE arithmetic order, one source for the fused kernel
 * (hope_policy_kernel.h) and the host twin pc_forward_host.
 *
 * Shape, fixed at compile time: embed 128, two-layer embedding MLPs with tanh, one pre-norm encoder layer (8 heads x 32, bias-free
 * fused qkv, a 128-wide token MLP with tanh), a (T x 128) -> 128 -> out_dim head with tanh between.  T = 3 tokens (lidar 120, target 5,
 * action mask 42) or T = 4: the fourth token arrives ready-made as [B][128] (torch keeps the image encoder's convolutions and
 * computes re_embed_img(embed_img(img))).  out_dim 1 or 2, the output tanh on or off.  view_embed is not added (the reference never
 * adds it).
 *
 * The rule.  float32 values throughout; two kinds of operation:
 *   chain      every Linear output is ONE accumulator that starts at its bias (+0.0f for to_qkv) and runs
 *                acc = fmaf(x[k], W[o][k], acc)        k = 0, 1, ... over the whole fan-in, ascending, no split,
 *              which is what the f32-input MFMA computes (k ascending across and inside its steps) and what v_fma_f32 computes.  The
 *              matrix instruction consumes two k per step, so an ODD fan-in (the target's 5) ends with one more term
 *              fmaf(+0.0f, +0.0f, acc): it changes nothing but a -0.0f sum, which becomes +0.0f.  (pc_chain)
 *   float64    everything else takes the float32 values to float64, computes there with IEEE + - * / sqrt and hm_exp / hm_tanh
 *              (hope_math.h) in the order written below, and rounds to float32 ONCE per stored value.
 *
 *   tanh       pc_tanh(x) = (float)hm_tanh((double)x)
 *   LayerNorm  torch's: biased variance, eps 1e-5.  Over the 128 values of a row, all sums in index order:
 *                mean = (x_0 + x_1 + ... + x_127) / 128;  d_i = x_i - mean;  var = (d_0 d_0 + d_1 d_1 + ...) / 128
 *                r = 1 / sqrt(var + 1e-5);   y_i = (float)(((d_i r) g_i) + b_i)                                          (pc_ln_row)
 *   attention  per scene and head, tokens i, j < T, q_i, k_j, v_j the head's 32 columns of the qkv output:
 *                dot_ij = chain from +0.0f over d = 0 .. 31 of q_i[d] k_j[d]                       (float32, no bias, even fan-in)
 *                s_ij   = (float)((double)dot_ij * 32^-0.5),  32^-0.5 = 0.17677669529663687 (the float64 nearest)
 *                m_i    = max_j s_ij;   e_ij = hm_exp((double)s_ij - (double)m_i);   z_i = e_i0 + e_i1 + ... (j ascending)
 *                p_ij   = (float)(e_ij / z_i)
 *                o_i[d] = chain from +0.0f over j = 0 .. T-1 of p_ij v_j[d]                        (no padding term)       (pc_attend)
 *   residual   x + y is one float32 addition.
 *
 * Forward of one scene:
 *   token_t  = chain_2(tanh(chain_1(in_t)))  for lidar, target, mask;  token_3 = the image token as given
 *   a        = to_out(concat_h o^h) ;  x1 = x + a          (to_out's chain runs over the 256 attention outputs, head-major)
 *   f        = ff2(tanh(ff1(LN2(x1)))) ;  x2 = x1 + f
 *   hid      = tanh(head1(x2 flattened token-major)) ;  out = head2(hid), then pc_tanh if tanh_out
 * Finite inputs are the contract.  A row's result depends on that row only.
 */
#pragma once
#include <stdint.h>
#include <math.h>

#include "hope_env.h"
#include "hope_math.h"

#define PC_E 128                                        /* embed width, mlp_dim, hidden_dim */
#define PC_HEADS 8
#define PC_DH 32
#define PC_INNER 256                                    /* heads x dim_head */
#define PC_QKV 768
#define PC_LIDAR 120
#define PC_TARGET 5
#define PC_MASK 42
#define PC_NPARAM 27                                    /* tensors of hope_policy_params_t */
#define PC_SCALE 0.17677669529663687                    /* 32^-0.5 */
#define PC_LN_EPS 1e-5

/* the order of hope_policy_params_t's fields */
enum { PC_LIDAR_W1 = 0, PC_TARGET_W1 = 4, PC_MASK_W1 = 8, PC_LN1_G = 12, PC_LN1_B, PC_QKV_W, PC_OUT_W, PC_OUT_B, PC_LN2_G, PC_LN2_B,
       PC_FF1_W, PC_FF1_B, PC_FF2_W, PC_FF2_B, PC_HEAD1_W, PC_HEAD1_B, PC_HEAD2_W, PC_HEAD2_B };

/* tensor i as torch holds it: [n_out][k_in] (a vector: k_in = 1) */
struct PcLayout {
    int n_out[PC_NPARAM], k_in[PC_NPARAM], k_pad[PC_NPARAM], off[PC_NPARAM];   /* off: floats into the packed buffer, tensor i stored [k_pad][n_out] */
    int total;
};

HM_FN bool pc_shape_ok(int n_tokens, int out_dim, int tanh_out) {
    return (n_tokens == 3 || n_tokens == 4) && (out_dim == 1 || out_dim == 2) && (tanh_out == 0 || tanh_out == 1);
}

HM_FN PcLayout pc_layout(int n_tokens, int out_dim) {
    PcLayout L;
    const int fan[3] = {PC_LIDAR, PC_TARGET, PC_MASK};
    for (int t = 0; t < 3; ++t) {
        const int i = 4 * t;
        L.n_out[i] = PC_E; L.k_in[i] = fan[t];
        L.n_out[i + 1] = PC_E; L.k_in[i + 1] = 1;
        L.n_out[i + 2] = PC_E; L.k_in[i + 2] = PC_E;
        L.n_out[i + 3] = PC_E; L.k_in[i + 3] = 1;
    }
    for (int i = PC_LN1_G; i < PC_NPARAM; ++i) { L.n_out[i] = PC_E; L.k_in[i] = 1; }
    L.n_out[PC_QKV_W] = PC_QKV; L.k_in[PC_QKV_W] = PC_E;
    L.k_in[PC_OUT_W] = PC_INNER;
    L.k_in[PC_FF1_W] = PC_E; L.k_in[PC_FF2_W] = PC_E;
    L.k_in[PC_HEAD1_W] = n_tokens * PC_E;
    L.n_out[PC_HEAD2_W] = out_dim; L.k_in[PC_HEAD2_W] = PC_E;
    L.n_out[PC_HEAD2_B] = out_dim;
    int off = 0;
    for (int i = 0; i < PC_NPARAM; ++i) {
        L.k_pad[i] = L.k_in[i] == 1 ? 1 : ((L.k_in[i] + 1) & ~1);
        L.off[i] = off;
        off += L.k_pad[i] * L.n_out[i];
        off = (off + 3) & ~3;
    }
    L.total = off;
    return L;
}

HM_FN float pc_tanh(float x) { return (float)hm_tanh((double)x); }

/* acc = fmaf(x[k xs], w[k ws], acc), k ascending; an odd fan-in ends with the matrix step's zero term */
HM_FN float pc_chain(float acc, const float* x, int xs, const float* w, int ws, int K) {
    for (int k = 0; k < K; ++k) acc = fmaf(x[(long)k * xs], w[(long)k * ws], acc);
    if (K & 1) acc = fmaf(0.0f, 0.0f, acc);
    return acc;
}

/* LayerNorm of one row of 128; y may be x */
HM_FN void pc_ln_row(const float* x, const float* g, const float* b, float* y) {
    double sum = 0.0;
    for (int i = 0; i < PC_E; ++i) sum = sum + (double)x[i];
    const double mean = sum / (double)PC_E;
    double sq = 0.0;
    for (int i = 0; i < PC_E; ++i) {
        const double d = (double)x[i] - mean;
        sq = sq + d * d;
    }
    const double r = 1.0 / sqrt(sq / (double)PC_E + PC_LN_EPS);
    for (int i = 0; i < PC_E; ++i) {
        const double d = (double)x[i] - mean;
        y[i] = (float)(((d * r) * (double)g[i]) + (double)b[i]);
    }
}

/* one query token of one head: q [32]; token j's key at k + j ks, value at v + j vs (32 each); o [32] */
template <int T>
HM_FN void pc_attend(const float* q, const float* k, int ks, const float* v, int vs, float* o) {
    float qv[PC_DH], s[T], p[T];
#pragma unroll
    for (int d = 0; d < PC_DH; ++d) qv[d] = q[d];
#pragma unroll
    for (int j = 0; j < T; ++j) {
        float dot = 0.0f;
#pragma unroll
        for (int d = 0; d < PC_DH; ++d) dot = fmaf(qv[d], k[j * ks + d], dot);
        s[j] = (float)((double)dot * PC_SCALE);
    }
    float m = s[0];
#pragma unroll
    for (int j = 1; j < T; ++j) m = s[j] > m ? s[j] : m;
    double e[T], z = 0.0;
#pragma unroll
    for (int j = 0; j < T; ++j) {
        e[j] = hm_exp((double)s[j] - (double)m);
        z = z + e[j];
    }
#pragma unroll
    for (int j = 0; j < T; ++j) p[j] = (float)(e[j] / z);
#pragma unroll
    for (int d = 0; d < PC_DH; ++d) {
        float acc = 0.0f;
#pragma unroll
        for (int j = 0; j < T; ++j) acc = fmaf(p[j], v[j * vs + d], acc);
        o[d] = acc;
    }
}

/* ---- the host twin: one scene at a time over torch's [out][in] tensors ---- */
static inline bool pc_params_ok(const hope_policy_params_t* P) {
    if (!P) return false;
    const float* const* t = (const float* const*)P;
    for (int i = 0; i < PC_NPARAM; ++i)
        if (!t[i]) return false;
    return true;
}

/* y[o] = chain(b[o], x, W[o]) for a torch Linear W [n_out][K] */
static inline void pc_linear(const float* W, const float* b, int n_out, int K, const float* x, float* y) {
    for (int o = 0; o < n_out; ++o) y[o] = pc_chain(b ? b[o] : 0.0f, x, 1, W + (long)o * K, 1, K);
}

template <int T>
static inline void pc_forward_row(const hope_policy_params_t* P, int out_dim, int tanh_out, const float* lidar, const float* target, const float* mask,
                                  const float* img, float* out) {
    const float* const* w = (const float* const*)P;
    const float* in[3] = {lidar, target, mask};
    const int fan[3] = {PC_LIDAR, PC_TARGET, PC_MASK};
    float x[T][PC_E], xn[T][PC_E], h[PC_E], qkv[T][PC_QKV], att[T][PC_INNER], y[PC_E];
    for (int t = 0; t < 3; ++t) {
        pc_linear(w[4 * t], w[4 * t + 1], PC_E, fan[t], in[t], h);
        for (int c = 0; c < PC_E; ++c) h[c] = pc_tanh(h[c]);
        pc_linear(w[4 * t + 2], w[4 * t + 3], PC_E, PC_E, h, x[t]);
    }
    if (T == 4)
        for (int c = 0; c < PC_E; ++c) x[T - 1][c] = img[c];
    for (int t = 0; t < T; ++t) {
        pc_ln_row(x[t], P->ln1_g, P->ln1_b, xn[t]);
        pc_linear(P->qkv_w, nullptr, PC_QKV, PC_E, xn[t], qkv[t]);
    }
    for (int hd = 0; hd < PC_HEADS; ++hd)
        for (int i = 0; i < T; ++i)
            pc_attend<T>(&qkv[i][hd * PC_DH], &qkv[0][PC_INNER + hd * PC_DH], PC_QKV, &qkv[0][2 * PC_INNER + hd * PC_DH], PC_QKV, &att[i][hd * PC_DH]);
    for (int t = 0; t < T; ++t) {
        pc_linear(P->out_w, P->out_b, PC_E, PC_INNER, att[t], y);
        for (int c = 0; c < PC_E; ++c) x[t][c] = x[t][c] + y[c];
        pc_ln_row(x[t], P->ln2_g, P->ln2_b, xn[t]);
        pc_linear(P->ff1_w, P->ff1_b, PC_E, PC_E, xn[t], h);
        for (int c = 0; c < PC_E; ++c) h[c] = pc_tanh(h[c]);
        pc_linear(P->ff2_w, P->ff2_b, PC_E, PC_E, h, y);
        for (int c = 0; c < PC_E; ++c) x[t][c] = x[t][c] + y[c];
    }
    pc_linear(P->head1_w, P->head1_b, PC_E, T * PC_E, &x[0][0], h);
    for (int c = 0; c < PC_E; ++c) h[c] = pc_tanh(h[c]);
    for (int o = 0; o < out_dim; ++o) {
        const float r = pc_chain(P->head2_b[o], h, 1, P->head2_w + (long)o * PC_E, 1, PC_E);
        out[o] = tanh_out ? pc_tanh(r) : r;
    }
}

static inline int pc_forward_host(const hope_policy_params_t* P, int n_tokens, int out_dim, int tanh_out, const float* lidar, const float* target,
                                  const float* mask, const float* img, int64_t batch, float* out) {
    if (!pc_params_ok(P) || !pc_shape_ok(n_tokens, out_dim, tanh_out) || !lidar || !target || !mask || !out || batch < 1) return HOPE_EINVAL;
    if ((n_tokens == 4) != (img != nullptr)) return HOPE_EINVAL;
    for (int64_t b = 0; b < batch; ++b) {
        const float *l = lidar + b * PC_LIDAR, *t = target + b * PC_TARGET, *m = mask + b * PC_MASK;
        if (n_tokens == 4) pc_forward_row<4>(P, out_dim, tanh_out, l, t, m, img + b * PC_E, out + b * out_dim);
        else pc_forward_row<3>(P, out_dim, tanh_out, l, t, m, nullptr, out + b * out_dim);
    }
    return HOPE_OK;
}
