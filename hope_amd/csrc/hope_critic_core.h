/*
 * hope_critic_core.h -- the inference forward of a critic HopeNet (hope_amd/policy.py HopeNet with output_size 1 and SacCritic; the
 * reference's MultiObsEmbedding under SACCriticAdapter, src/model/agent/sac_agent.py:15-30) in ONE arithmetic order, one source for
 * the fused kernel (hope_critic_kernel.h) and the host twin cc_forward_host.
 *
 * The rule is hope_policy_core.h's, extended to T = 3 + has_img + has_action tokens, T in {3, 4, 5}:
 *   token order  that of HopeNet.tokens: lidar, target, mask, [the image token as given, [B][128]], [action]
 *   action       token = chain_2(tanh(chain_1(action))): embed_action.0 is [128][2] (even fan-in: one matrix step, no zero term),
 *                embed_action.2 is [128][128]
 *   head         head1 is [128][T * 128], token-major; out_dim = 1, no output tanh
 * and everything else as it stands there: every Linear one k-ascending float32 fmaf chain from its bias (pc_chain), LayerNorm,
 * softmax and tanh float64 rounded once (pc_ln_row, pc_attend<T>, pc_tanh), a residual one float32 addition.  For has_action = 0 the
 * operations are those of pc_forward_row with out_dim 1 and tanh_out 0, so the words are the same.
 * Finite inputs are the contract.  A row's result depends on that row only.
 */
#pragma once
#include "hope_policy_core.h"

#define CC_ACTION 2                                     /* fan-in of embed_action.0 */
#define CC_NPARAM 31                                    /* tensors of hope_critic_params_t */

/* the order of hope_critic_params_t's fields: hope_policy_params_t's (PC_*), then the action embedding */
enum { CC_ACTION_W1 = PC_NPARAM, CC_ACTION_B1, CC_ACTION_W2, CC_ACTION_B2 };

/* tensor i as torch holds it: [n_out][k_in] (a vector: k_in = 1); without an action token the four action tensors are empty */
struct CcLayout {
    int n_out[CC_NPARAM], k_in[CC_NPARAM], k_pad[CC_NPARAM], off[CC_NPARAM];   /* off: floats into a slot, tensor i stored [k_pad][n_out] */
    int total;                                                                  /* floats of a slot, a multiple of 4 */
};

HM_FN bool cc_shape_ok(int has_img, int has_action) { return (has_img == 0 || has_img == 1) && (has_action == 0 || has_action == 1); }
HM_FN int cc_tokens(int has_img, int has_action) { return 3 + has_img + has_action; }

HM_FN CcLayout cc_layout(int has_img, int has_action) {
    const PcLayout P = pc_layout(cc_tokens(has_img, has_action), 1);
    CcLayout L;
    for (int i = 0; i < PC_NPARAM; ++i) { L.n_out[i] = P.n_out[i]; L.k_in[i] = P.k_in[i]; }
    for (int i = PC_NPARAM; i < CC_NPARAM; ++i) { L.n_out[i] = has_action ? PC_E : 0; L.k_in[i] = 1; }
    L.k_in[CC_ACTION_W1] = CC_ACTION; L.k_in[CC_ACTION_W2] = PC_E;
    int off = 0;
    for (int i = 0; i < CC_NPARAM; ++i) {
        L.k_pad[i] = L.k_in[i] == 1 ? 1 : ((L.k_in[i] + 1) & ~1);
        L.off[i] = off;
        off += L.k_pad[i] * L.n_out[i];
        off = (off + 3) & ~3;
    }
    L.total = off;
    return L;
}

/* ---- the host twin: one scene at a time over torch's [out][in] tensors ---- */
static inline bool cc_params_ok(const hope_critic_params_t* P, int has_action) {
    if (!P) return false;
    const float* const* t = (const float* const*)P;
    for (int i = 0; i < CC_NPARAM; ++i)
        if ((t[i] != nullptr) != (i < PC_NPARAM || has_action)) return false;      /* the action tensors NULL exactly without the token */
    return true;
}

template <int T>
static inline void cc_forward_row(const hope_critic_params_t* P, int has_img, int has_action, const float* lidar, const float* target, const float* mask,
                                  const float* img, const float* action, float* out) {
    const float* const* w = (const float* const*)P;
    const float* in[3] = {lidar, target, mask};
    const int fan[3] = {PC_LIDAR, PC_TARGET, PC_MASK};
    float x[T][PC_E], xn[T][PC_E], h[PC_E], qkv[T][PC_QKV], att[T][PC_INNER], y[PC_E];
    for (int t = 0; t < 3; ++t) {
        pc_linear(w[4 * t], w[4 * t + 1], PC_E, fan[t], in[t], h);
        for (int c = 0; c < PC_E; ++c) h[c] = pc_tanh(h[c]);
        pc_linear(w[4 * t + 2], w[4 * t + 3], PC_E, PC_E, h, x[t]);
    }
    if (has_img)
        for (int c = 0; c < PC_E; ++c) x[T > 3 ? 3 : 0][c] = img[c];               /* (has_img: T > 3) */
    if (has_action) {
        pc_linear(w[CC_ACTION_W1], w[CC_ACTION_B1], PC_E, CC_ACTION, action, h);
        for (int c = 0; c < PC_E; ++c) h[c] = pc_tanh(h[c]);
        pc_linear(w[CC_ACTION_W2], w[CC_ACTION_B2], PC_E, PC_E, h, x[T - 1]);
    }
    for (int t = 0; t < T; ++t) {
        pc_ln_row(x[t], w[PC_LN1_G], w[PC_LN1_B], xn[t]);
        pc_linear(w[PC_QKV_W], nullptr, PC_QKV, PC_E, xn[t], qkv[t]);
    }
    for (int hd = 0; hd < PC_HEADS; ++hd)
        for (int i = 0; i < T; ++i)
            pc_attend<T>(&qkv[i][hd * PC_DH], &qkv[0][PC_INNER + hd * PC_DH], PC_QKV, &qkv[0][2 * PC_INNER + hd * PC_DH], PC_QKV, &att[i][hd * PC_DH]);
    for (int t = 0; t < T; ++t) {
        pc_linear(w[PC_OUT_W], w[PC_OUT_B], PC_E, PC_INNER, att[t], y);
        for (int c = 0; c < PC_E; ++c) x[t][c] = x[t][c] + y[c];
        pc_ln_row(x[t], w[PC_LN2_G], w[PC_LN2_B], xn[t]);
        pc_linear(w[PC_FF1_W], w[PC_FF1_B], PC_E, PC_E, xn[t], h);
        for (int c = 0; c < PC_E; ++c) h[c] = pc_tanh(h[c]);
        pc_linear(w[PC_FF2_W], w[PC_FF2_B], PC_E, PC_E, h, y);
        for (int c = 0; c < PC_E; ++c) x[t][c] = x[t][c] + y[c];
    }
    pc_linear(w[PC_HEAD1_W], w[PC_HEAD1_B], PC_E, T * PC_E, &x[0][0], h);
    for (int c = 0; c < PC_E; ++c) h[c] = pc_tanh(h[c]);
    out[0] = pc_chain(w[PC_HEAD2_B][0], h, 1, w[PC_HEAD2_W], 1, PC_E);
}

static inline int cc_forward_host(const hope_critic_params_t* P, int has_img, int has_action, const float* lidar, const float* target, const float* mask,
                                  const float* img, const float* action, int64_t batch, float* out) {
    if (!cc_shape_ok(has_img, has_action) || !cc_params_ok(P, has_action) || !lidar || !target || !mask || !out || batch < 1) return HOPE_EINVAL;
    if ((has_img != 0) != (img != nullptr) || (has_action != 0) != (action != nullptr)) return HOPE_EINVAL;
    const int T = cc_tokens(has_img, has_action);
    for (int64_t b = 0; b < batch; ++b) {
        const float *l = lidar + b * PC_LIDAR, *t = target + b * PC_TARGET, *m = mask + b * PC_MASK;
        const float *i = has_img ? img + b * PC_E : nullptr, *a = has_action ? action + b * CC_ACTION : nullptr;
        if (T == 3) cc_forward_row<3>(P, has_img, has_action, l, t, m, i, a, out + b);
        else if (T == 4) cc_forward_row<4>(P, has_img, has_action, l, t, m, i, a, out + b);
        else cc_forward_row<5>(P, has_img, has_action, l, t, m, i, a, out + b);
    }
    return HOPE_OK;
}
