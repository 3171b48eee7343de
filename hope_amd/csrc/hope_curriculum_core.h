/*
 * hope_curriculum_core.h -- the arithmetic of the map curriculum, one source for host and device.
 *
 * The reference picks every new episode's scene with two choosers (src/train/train_HOPE_sac.py:23-97): SceneChoose (scene type:
 * Normal / Complex / Extrem / dlp) and DlpCaseChoose (the Dragon-Lake case).  Here a finished scene draws `list[key % n]` inside the
 * step kernel, so the curriculum is a WEIGHTED draw list of fixed length CW_LIST_LEN in which bucket b owns ~p_b * CW_LIST_LEN
 * positions.  This header holds everything that decides those lists: the window rule, the probabilities, the apportionment of the
 * positions and the entry of a position.  k_curriculum_weights / k_curriculum_fill (hope_curriculum_kernel.h) and the host twin
 * hope_curriculum_lists_host compile it; only + - * / floor and compares are used and contraction is off on both compilers
 * (-ffp-contract=off), so both give the same lists bit for bit.
 *
 * Buckets: 0 / 1 / 2 lots of level Normal / Complex / Extrem, 3 "dlp" as a scene type (every Dragon-Lake episode), 4 + c Dragon-Lake
 * case c.  Groups of a draw list (one list per size class): 0 / 1 / 2 the labelled lots of that level, 3 the UNLABELLED pool entries,
 * 4 + c case c.  A class list keeps, per kind (labelled lots, unlabelled lots, cases), the share that kind has in the uniform base
 * list: this library fixes which scene slots are Dragon-Lake slots (the large-tile class: launch lists, LDS size), so q_3 cannot
 * move scenes between classes -- it is reported and otherwise unused.
 *
 * Phases: the functions named cw_*_phase take (lane, n_lanes) and touch the entries lane, lane + n_lanes, ...; the caller puts a
 * barrier between two phases (the host calls them with (0, 1)).  Sums run sequentially in index order on every lane, so their
 * rounding does not depend on the lane count.
 */
#pragma once
#include <stdint.h>

#include "hope_env.h"
#include "hope_math.h"

#define CW_LIST_LEN HOPE_CURRICULUM_LIST_LEN
#define CW_MAX_GROUPS 254                              /* 4 + n_cases: a bucket id fits a byte, 255 = unlabelled */
#define CW_UNLABELLED 255

HM_FN double cw_clip(double x, double lo, double hi) { return x < lo ? lo : (x > hi ? hi : x); }

/* the running window of one bucket: (n, s) += (dn, ds); beyond W both are scaled back to n = W */
HM_FN void cw_fold(double* n, double* s, double dn, double ds, double W) {
    double nn = *n + dn, ss = *s + ds;
    if (nn > W) { ss = ss * (W / nn); nn = W; }
    *n = nn; *s = ss;
}

/* SceneChoose: pw = _choose_case_worst_perform's p; q = the long-run type frequencies of choose_case, the water-filling
 * q_t = max(worst_share * pw_t, h) with sum q = 1 (closed form over the sorted values).  A type that never finished an episode has
 * success rate 0 (the reference divides 0 by 0 there).  Uniform before type_horizon episodes. */
HM_FN void cw_type_probs(const double* wn, const double* ws, const hope_curriculum_params* P, uint64_t type_episodes, double* pw, double* q) {
    double fail[4], sum = 0.0;
    for (int t = 0; t < 4; t++) {
        const double rate = wn[t] > 0.0 ? ws[t] / wn[t] : 0.0;
        fail[t] = cw_clip(P->target[t] - rate, P->type_fail_min, 1.0);
        sum = sum + fail[t];
    }
    for (int t = 0; t < 4; t++) pw[t] = fail[t] / sum;
    if ((int64_t)type_episodes < P->type_horizon) { for (int t = 0; t < 4; t++) q[t] = 0.25; return; }
    double a[4];
    for (int t = 0; t < 4; t++) a[t] = P->worst_share * pw[t];
    double srt[4] = {a[0], a[1], a[2], a[3]};                  /* ascending */
    for (int i = 1; i < 4; i++) for (int j = i; j > 0 && srt[j] < srt[j - 1]; j--) { const double tmp = srt[j]; srt[j] = srt[j - 1]; srt[j - 1] = tmp; }
    double h = 0.25;
    double top = 0.0;                                          /* sum of the values above the water level */
    for (int k = 4; k >= 1; k--) {                             /* the k smallest are lifted to h */
        h = (1.0 - top) / (double)k;
        if (h >= srt[k - 1]) break;
        top = top + srt[k - 1];
    }
    for (int t = 0; t < 4; t++) q[t] = a[t] > h ? a[t] : h;
}

/* DlpCaseChoose.choose_case: the clipped failure rate of one case */
HM_FN double cw_case_fail(double n, double s, const hope_curriculum_params* P) {
    const double rate = n <= 1.0 ? 0.0 : s / n;
    return cw_clip(1.0 - rate, P->case_fail_min, 1.0);
}

/* what a class list is made of */
struct CwClass {
    int32_t cnt[4];          /* entries of group 0 .. 3 (labelled lots by level, unlabelled lots) in `sorted`, in that order */
    int32_t n_cases;         /* Dragon-Lake cases in this class's list (all of them or none) */
};
HM_FN int cw_n_base(const CwClass& c) { return c.cnt[0] + c.cnt[1] + c.cnt[2] + c.cnt[3] + c.n_cases; }
HM_FN bool cw_has_entries(const CwClass& c, int g) { return g < 4 ? c.cnt[g] > 0 : c.n_cases > 0; }

/* working arrays of one class (CW_MAX_GROUPS entries each, prefix one more) */
struct CwWork {
    double* w;               /* weight of every group, sum 1 */
    double* r;               /* remainder of w * L, -1 for a group that cannot take a remainder position */
    int32_t* f;              /* floor(w * L), at least 1 for a group with entries */
    int32_t* pos;            /* positions */
    int32_t* prefix;         /* [G + 1] */
};

/* phase 1: case failure rates into w[4 + c] */
HM_FN void cw_case_fail_phase(const double* wn, const double* ws, int n_cases, const hope_curriculum_params* P, double* w, int lane, int nl) {
    for (int c = lane; c < n_cases; c += nl) w[4 + c] = cw_case_fail(wn[4 + c], ws[4 + c], P);
}
/* phase 2: case probabilities p_c (prob[4 + c]) from the failure rates in w[4 + c]; uniform before case_horizon Dragon-Lake episodes */
HM_FN void cw_case_prob_phase(int n_cases, const hope_curriculum_params* P, uint64_t dlp_episodes, const double* w, double* prob, int lane, int nl) {
    if (n_cases <= 0) return;
    double sum = 0.0;
    for (int c = 0; c < n_cases; c++) sum = sum + w[4 + c];
    const double u = 1.0 / (double)n_cases;
    const bool uniform = (int64_t)dlp_episodes < P->case_horizon;
    for (int c = lane; c < n_cases; c += nl)
        prob[4 + c] = uniform ? u : P->case_uniform * u + (1.0 - P->case_uniform) * (w[4 + c] / sum);
}
/* phase 3: group weights of a class from q (prob[0 .. 3]) and p_c (prob[4 + c]); then x = w * L, floor, remainder */
HM_FN void cw_weight_phase(const CwClass& cl, int G, const double* prob, const CwWork& k, int lane, int nl) {
    const double nb = (double)cw_n_base(cl);
    const int n_lev = cl.cnt[0] + cl.cnt[1] + cl.cnt[2];
    double qs = 0.0;
    for (int l = 0; l < 3; l++) if (cl.cnt[l] > 0) qs = qs + prob[l];
    const double share_lev = (double)n_lev / nb, share_unl = (double)cl.cnt[3] / nb, share_case = (double)cl.n_cases / nb;
    for (int g = lane; g < G; g += nl) {
        double w;
        if (g < 3) w = cl.cnt[g] > 0 ? share_lev * (prob[g] / qs) : 0.0;
        else if (g == 3) w = share_unl;
        else w = cl.n_cases > 0 ? share_case * prob[g] : 0.0;
        const double x = w * (double)CW_LIST_LEN;
        double fl = floor(x);
        double rem = x - fl;
        if (!cw_has_entries(cl, g)) { fl = 0.0; rem = -1.0; }
        else if (fl < 1.0) { fl = 1.0; rem = -1.0; }               /* every group with entries owns a position */
        k.w[g] = w; k.f[g] = (int32_t)fl; k.r[g] = rem;
    }
}
/* phase 4: largest remainder, ties to the lower group: group g gets one of the R left-over positions iff fewer than R groups
 * rank before it */
HM_FN void cw_remainder_phase(int G, const CwWork& k, int lane, int nl) {
    int64_t sum = 0;
    for (int g = 0; g < G; g++) sum += k.f[g];
    const int64_t R = (int64_t)CW_LIST_LEN - sum;
    for (int g = lane; g < G; g += nl) {
        int inc = 0;
        const double rg = k.r[g];
        if (R > 0 && rg >= 0.0) {
            int rank = 0;
            for (int o = 0; o < G; o++) { const double ro = k.r[o]; if (ro > rg || (ro == rg && o < g)) rank++; }
            inc = rank < R ? 1 : 0;
        }
        k.pos[g] = k.f[g] + inc;
    }
}
/* phase 5 (one lane): whatever is still missing or too much goes to / comes from the largest group (only when minimum positions
 * were handed out or the weights did not sum to 1 within G ulps), then the prefix sum */
HM_FN void cw_prefix_phase(int G, const CwWork& k) {
    int64_t sum = 0;
    for (int g = 0; g < G; g++) sum += k.pos[g];
    while (sum != (int64_t)CW_LIST_LEN) {
        int big = 0;
        for (int g = 1; g < G; g++) if (k.pos[g] > k.pos[big]) big = g;
        if (sum < (int64_t)CW_LIST_LEN) { k.pos[big] += (int32_t)((int64_t)CW_LIST_LEN - sum); sum = CW_LIST_LEN; }
        else {
            const int64_t over = sum - (int64_t)CW_LIST_LEN, room = (int64_t)k.pos[big] - 1;
            const int64_t take = over < room ? over : room;
            if (take <= 0) break;                              /* (every group at its minimum: cannot happen for G <= L) */
            k.pos[big] -= (int32_t)take; sum -= take;
        }
    }
    k.prefix[0] = 0;
    for (int g = 0; g < G; g++) k.prefix[g + 1] = k.prefix[g] + k.pos[g];
}

/* the entry at position pos of a class list: the group by binary search in the prefix, then that group's entries in turn.
 * sorted: the class's pool entries ordered by group (0, 1, 2, unlabelled); a case group is its own single entry -2 - c */
HM_FN int32_t cw_entry(const CwClass& cl, int G, const int32_t* prefix, const int32_t* sorted, int32_t pos) {
    int lo = 0, hi = G;                                        /* prefix[lo] <= pos < prefix[hi] */
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (prefix[mid] <= pos) lo = mid; else hi = mid; }
    const int g = lo;
    if (g >= 4) return -2 - (g - 4);
    int off = 0;
    for (int o = 0; o < g; o++) off += cl.cnt[o];
    return sorted[off + (pos - prefix[g]) % cl.cnt[g]];
}
