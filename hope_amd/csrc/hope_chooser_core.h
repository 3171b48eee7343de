/*
 * hope_chooser_core.h -- the masked choice of one of the 42 discrete actions, one source for host and device.
 *
 * The reference's ActionMask.choose_action (src/model/action_mask.py:199-227) weighs the Gaussian policy head's density at the 42
 * discrete actions with the action mask and draws one of them; the agent then casts, clamps, lets the path replay override the row
 * (parking_agent.py:80-99) and evaluates the log-probability of what it took (ppo_agent.py:137-140).  k_choose
 * (hope_chooser_kernel.h) and the host twin ch_host / hope_chooser_host compile this header: float64 throughout, hm_exp of
 * hope_math.h and plain IEEE operations in a fixed order, contraction off on both compilers -- both give the same bits.
 *
 * Action table A[42][2] (float64, numpy's own bits of tables.discrete_actions() / [VALID_STEER[1], 1]): rows 0 .. 20 are the 21
 * steers at speed A[0][1], rows 21 .. 41 the SAME 21 steers at speed A[21][1] (ch_table_ok checks exactly that), so a scene needs
 * 21 steer terms and 2 speed terms, not 84.
 *
 * Per scene, with sd_d = exp(log_std_d):
 *   term(a, d) = clip(-0.5 z^2 - (log_std_d + 0.5 ln 2pi), -10, 10),  z = (a - mean_d) / sd_d       (action_mask.py:217-222)
 *   e_k        = exp(term(A[k][0], 0) + term(A[k][1], 1)) * mask_k
 *   S          = e_0 + e_1 + ... + e_41 (in this order);  cum_k the running sums;  t = u * S
 *   k*         = the first k with e_k > 0 and cum_k > t; if rounding at the top leaves none, the last k with e_k > 0
 * which is np.random.choice(p = e / S): cdf, then searchsorted on the right.  log_std + 0.5 ln 2pi stands for the reference's
 * log(sqrt(2 pi) std): no logarithm is needed, and the clip is continuous, so the last bit decides nothing.
 *
 * Degenerate rows.  A row is unusable when S is not positive or not finite (an all-zero mask of an inactive slot), or when a mean or
 * log_std of the row is not finite (a NaN or an infinity from the policy).  The reference -- and torch.multinomial, with a
 * device-side assertion -- would crash on it; here
 *   1. the row is redone with every mask_k = 1                                      -> idx has HOPE_CHOOSE_NOMASK (64) set
 *   2. if S is still unusable, or the policy's numbers are not finite, k* = CH_FALLBACK = 10 (steer 0, forwards); probs is 1 at
 *      that index and 0 elsewhere                                                   -> idx has HOPE_CHOOSE_NOMASK | HOPE_CHOOSE_FIXED
 * idx & 63 is always a legal index, nothing is read out of range, nothing asserts.  The log-probability of a row with a
 * non-finite mean is what the formula gives (-inf, or NaN -- always the one quiet NaN 0x7FC00000): the flag is the signal.
 *
 * Action: a_d = clamp((float)A[k*][d], -1, 1); an executing scene takes (float)planned_d instead (agents.act's order of cast, clamp
 * and torch.where).  Log-probability: gaussian_log_prob in float64 on that float32 action, rounded to float32 once.
 *
 * Without a supplied u the draw is counter-based: the top 53 bits of ch_mix64(ch_mix64(ch_mix64(seed) ^ counter) ^ scene), times
 * 2^-53 -- ch_mix64 is the splitmix64 finaliser (hope_dev.h's mix64, hope_env.hip's hmix64).  It depends on (seed, counter, scene
 * index) alone: not on the launch geometry, not on how a batch is split.
 *
 * Exponent arguments are screened (ch_exp): hm_exp converts rint(x log2 e) to int, which is defined for |x| <= 700 only.
 */
#pragma once
#include <stdint.h>

#include "hope_env.h"
#include "hope_math.h"

#define CH_NA HOPE_N_ACTION
#define CH_NS 21                                       /* steers; the speed takes two values */
#define CH_PITCH 43                                    /* row pitch in LDS: odd, so 64 lanes walking their rows hit 64 banks */
#define CH_HALF_LN_2PI 0.9189385332046727              /* 0.5 * log(2 pi) */
#define CH_FALLBACK 10                                 /* A[10] = [0, 1]: straight ahead */

HM_FN bool ch_finite(double x) { return fabs(x) <= 1.7976931348623157e308; }       /* false for NaN and +-inf */
HM_FN double ch_exp(double x) {
    if (!(x == x)) return x;
    if (x > 700.0) return __builtin_inf();
    if (x < -700.0) return 0.0;
    return hm_exp(x);
}
HM_FN double ch_clip(double lp) { return lp < -10.0 ? -10.0 : (lp > 10.0 ? 10.0 : lp); }    /* NaN stays NaN, as torch.clamp */
HM_FN double ch_term(double a, double mean, double sd, double log_std) {
    const double z = (a - mean) / sd;
    return ch_clip(-0.5 * (z * z) - (log_std + CH_HALF_LN_2PI));
}
HM_FN uint64_t ch_mix64(uint64_t z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
HM_FN double ch_uniform(uint64_t seed, uint64_t counter, uint64_t scene) {
    const uint64_t x = ch_mix64(ch_mix64(ch_mix64(seed) ^ counter) ^ scene);
    return (double)(x >> 11) * 0x1p-53;                              /* 2^-53: [0, 1) */
}
HM_FN float ch_clamp1(float a) { return a < -1.0f ? -1.0f : (a > 1.0f ? 1.0f : a); }
/* one NaN for every NaN: which payload and sign an operation hands on is the one thing the two sides do not share */
HM_FN float ch_canon(float x) { return x == x ? x : __builtin_bit_cast(float, 0x7FC00000u); }

/* the layout the 23-term evaluation relies on */
static inline bool ch_table_ok(const double* A) {
    for (int k = 0; k < CH_NA; k++) {
        if (!ch_finite(A[2 * k]) || !ch_finite(A[2 * k + 1])) return false;
        if (A[2 * k + 1] != A[k < CH_NS ? 1 : 2 * CH_NS + 1]) return false;
        if (k >= CH_NS && A[2 * k] != A[2 * (k - CH_NS)]) return false;
    }
    return true;
}

/* e_k into row[0 .. 41] (row holds the mask on entry; ones: every mask_k = 1); returns S */
HM_FN double ch_fill(const double* A, double m0, double m1, double ls0, double ls1, double sd0, double sd1, double* row, bool ones) {
    const double cf = ch_term(A[1], m1, sd1, ls1), cb = ch_term(A[2 * CH_NS + 1], m1, sd1, ls1);
    for (int k = 0; k < CH_NS; k++) {
        const double c0 = ch_term(A[2 * k], m0, sd0, ls0);
        const double mf = ones ? 1.0 : row[k], mb = ones ? 1.0 : row[k + CH_NS];
        row[k] = ch_exp(c0 + cf) * mf;
        row[k + CH_NS] = ch_exp(c0 + cb) * mb;
    }
    double S = 0.0;
    for (int k = 0; k < CH_NA; k++) S += row[k];
    return S;
}

struct ChOut {
    int idx;                 /* k* | HOPE_CHOOSE_* flags */
    float a0, a1;            /* the action taken */
    float lp0, lp1;          /* its log-probability per dimension */
};

/* One scene.  row: 42 doubles of scratch that hold the mask on entry (LDS on the device, a local array on the host) and, with
 * want_probs, e_k / S on return.  ex: the scene replays a planned action (p0, p1). */
HM_FN ChOut ch_scene(const double* A, double m0, double m1, double ls0, double ls1, double* row, bool ex, double p0, double p1, double u,
                     bool want_probs) {
    ChOut o;
    const bool in_ok = ch_finite(m0) && ch_finite(m1) && ch_finite(ls0) && ch_finite(ls1);
    const double sd0 = ch_exp(ls0), sd1 = ch_exp(ls1);
    int flags = 0;
    double S = 0.0;
    bool ok = false;
    if (in_ok) {
        S = ch_fill(A, m0, m1, ls0, ls1, sd0, sd1, row, false);
        ok = S > 0.0 && ch_finite(S);
    }
    if (!ok) {
        flags = HOPE_CHOOSE_NOMASK;
        if (in_ok) {
            S = ch_fill(A, m0, m1, ls0, ls1, sd0, sd1, row, true);
            ok = S > 0.0 && ch_finite(S);
        }
    }
    int kk = CH_FALLBACK;
    if (ok) {
        const double t = u * S;
        double cum = 0.0;
        int pick = -1, last = 0;
        for (int k = 0; k < CH_NA; k++) {
            const double e = row[k];
            cum += e;
            if (e > 0.0) {
                last = k;
                if (pick < 0 && cum > t) pick = k;
            }
        }
        kk = pick >= 0 ? pick : last;
        if (want_probs)
            for (int k = 0; k < CH_NA; k++) row[k] = row[k] / S;
    } else {
        flags |= HOPE_CHOOSE_FIXED;
        if (want_probs)
            for (int k = 0; k < CH_NA; k++) row[k] = k == CH_FALLBACK ? 1.0 : 0.0;
    }
    o.idx = kk | flags;
    o.a0 = ch_clamp1((float)A[2 * kk]);
    o.a1 = ch_clamp1((float)A[2 * kk + 1]);
    if (ex) { o.a0 = (float)p0; o.a1 = (float)p1; }
    const double d0 = (double)o.a0 - m0, d1 = (double)o.a1 - m1;
    o.lp0 = ch_canon((float)(-(d0 * d0) / (2.0 * ch_exp(2.0 * ls0)) - ls0 - CH_HALF_LN_2PI));
    o.lp1 = ch_canon((float)(-(d1 * d1) / (2.0 * ch_exp(2.0 * ls1)) - ls1 - CH_HALF_LN_2PI));
    return o;
}

/* The host twin: the same choice over host arrays (layouts as hope_env_choose).  scene0: index of row 0 in the counter-based draw,
 * so that a batch may be split.  Returns HOPE_OK or HOPE_EINVAL; hope_chooser_host forwards to it. */
static inline int ch_host(int n, const double* A, const void* mean, const void* log_std, int ls_stride, int in_f64, const void* mask, int mask_f64,
                          const double* planned, const uint8_t* executing, const double* u, uint64_t seed, uint64_t counter, uint64_t scene0,
                          void* action, int action_f64, float* action_f32, int32_t* idx, float* log_prob, double* probs) {
    if (n <= 0 || !A || !mean || !log_std || !mask || !action || (ls_stride != 0 && ls_stride != 2) || (planned != nullptr) != (executing != nullptr) ||
        !ch_table_ok(A))
        return HOPE_EINVAL;
    for (int s = 0; s < n; s++) {
        const size_t i = (size_t)s, l = i * (size_t)ls_stride;
        double m0, m1, ls0, ls1, row[CH_NA];
        if (in_f64) { const double* q = (const double*)mean; m0 = q[2 * i]; m1 = q[2 * i + 1]; q = (const double*)log_std; ls0 = q[l]; ls1 = q[l + 1]; }
        else { const float* q = (const float*)mean; m0 = q[2 * i]; m1 = q[2 * i + 1]; q = (const float*)log_std; ls0 = q[l]; ls1 = q[l + 1]; }
        for (int k = 0; k < CH_NA; k++) row[k] = mask_f64 ? ((const double*)mask)[i * CH_NA + k] : (double)((const float*)mask)[i * CH_NA + k];
        const bool ex = executing && executing[i];
        const double uu = u ? u[i] : ch_uniform(seed, counter, scene0 + i);
        const ChOut o = ch_scene(A, m0, m1, ls0, ls1, row, ex, planned ? planned[2 * i] : 0.0, planned ? planned[2 * i + 1] : 0.0, uu, probs != nullptr);
        if (action_f64) { ((double*)action)[2 * i] = (double)o.a0; ((double*)action)[2 * i + 1] = (double)o.a1; }
        else { ((float*)action)[2 * i] = o.a0; ((float*)action)[2 * i + 1] = o.a1; }
        if (action_f32) { action_f32[2 * i] = o.a0; action_f32[2 * i + 1] = o.a1; }
        if (idx) idx[i] = o.idx;
        if (log_prob) { log_prob[2 * i] = o.lp0; log_prob[2 * i + 1] = o.lp1; }
        if (probs) for (int k = 0; k < CH_NA; k++) probs[i * CH_NA + k] = row[k];
    }
    return HOPE_OK;
}
