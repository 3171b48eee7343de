/*
 * hope_evaltrack_core.h -- the per-episode bookkeeping of an evaluation run, one source for host and device.
 *
 * The reference's eval() (src/evaluation/eval_utils.py:35-57) keeps, per episode: the stuck detector (:46-47 -- when obs['target']
 * did not change since the previous step the action is replaced by a uniform draw from the PHYSICAL action box, which the wrapper
 * clips to [-1, 1]), the step count, the summed reward, the path length (sum of the rear-axle displacements, :52-53) and the final
 * status; a batched evaluator adds the alive mask (finished slots are frozen) and hides the stale Reeds-Shepp words of frozen slots
 * from the planner.  k_eval_begin / k_eval_override / k_eval_track (hope_evaltrack_kernel.h) and the host twins et_begin_host /
 * et_override_host / et_track_host compile this header: float64 throughout, hm_hypot of hope_math.h and plain IEEE operations in a
 * fixed order, contraction off on both compilers, no libm -- both give the same bits.
 *
 * State of a scene: ET_WORDS = 10 eight-byte words, stored as planes ([j][stride], j = 0 .. 9) so that a wave reads and writes whole
 * lines:
 *   planes 0-4  last_target as double (a float32 observation widens exactly: == decides what torch's == decides)
 *   planes 5-6  last_xy
 *   plane  7    the summed reward
 *   plane  8    the path length
 *   plane  9    packed: bits 0-31 steps, bits 32-39 status, bit 40 alive, bit 41 stuck
 * A NaN that is stored is always stored as the one quiet NaN 0x7FF8000000000000 (et_canon): which payload and sign an operation
 * hands on is the one thing the two compilers do not share.
 *
 * begin(target, pose):  last_target = target, last_xy = pose[:2], sums and steps 0, status 1, alive 1, stuck 1 -- the reference's
 *                       first comparison is obs['target'] with itself (:39, :46), so every episode's first action is the random one.
 * override(actions):    active_out = alive; a scene with `stuck` set -- alive or not, as the torch loop does row for row -- has its
 *                       action row replaced by a_d = clamp(lo_d + span_d * u_d, -1, 1) cast once to the action type, span_d = hi_d -
 *                       lo_d formed once on the host (evaluate.py's `self._lo + self._span * rand`).  Other rows are not touched.
 *                       Without a supplied u the draw is counter-based: u_d = the top 53 bits of
 *                       mix64(mix64(mix64(seed ^ ET_TAG) ^ counter) ^ (2 * scene + d)) times 2^-53 -- the chooser's construction
 *                       (hope_chooser_core.h) under a fixed tag, so the two streams differ under one seed.  It depends on (seed,
 *                       counter, scene, d) alone: not on the launch geometry, not on how a batch is split.
 * track(...):           after the env step, per scene with live = alive:
 *                         1. live: steps += 1, total += (double)reward, path += hm_hypot(x - last_x, y - last_y)
 *                         2. last_xy = (x, y)
 *                         3. fin = live && done; fin: status = the env's status
 *                         4. stuck = all_k((double)target_k == last_target_k)          (a NaN target is never stuck)
 *                         5. last_target = target
 *                         6. keep = live && !fin
 *                         7. word_out = rs_word with byte 6 (the found flag) zeroed unless keep
 *                         8. done_out = fin
 *                         9. alive = keep
 */
#pragma once
#include <stdint.h>

#include "hope_env.h"
#include "hope_math.h"

#define ET_WORDS HOPE_EVAL_STATE_WORDS
#define ET_TAG 0x4556414C54524B31ull                   /* "EVALTRK1": keeps the stream apart from the chooser's under the same seed */
#define ET_QNAN 0x7FF8000000000000ull
#define ET_ALIVE (1ull << 40)
#define ET_STUCK (1ull << 41)
#define ET_FOUND_BYTE (0xFFull << 48)                  /* byte 6 of an rs_word row */

/* scalar members and no loops over them: every access has a static address, so the state stays in registers on the device */
struct EtState {
    double t0, t1, t2, t3, t4;   /* last_target */
    double lx, ly;               /* last_xy */
    double total, path;
    uint64_t w;
};
struct EtObs {
    double t0, t1, t2, t3, t4;   /* target, widened */
    double x, y;                 /* pose[:2] */
};
struct EtBox {
    double lo0, span0, lo1, span1;   /* steer, speed: lo and hi - lo */
};

HM_FN double et_bits_to_double(uint64_t u) { return __builtin_bit_cast(double, u); }
HM_FN uint64_t et_double_to_bits(double d) { return __builtin_bit_cast(uint64_t, d); }
HM_FN double et_canon(double x) { return x == x ? x : et_bits_to_double(ET_QNAN); }
HM_FN float et_canon32(float x) { return x == x ? x : __builtin_bit_cast(float, 0x7FC00000u); }
HM_FN bool et_finite(double x) { return fabs(x) <= 1.7976931348623157e308; }       /* false for NaN and +-inf */
HM_FN uint64_t et_mix64(uint64_t z) {                  /* the splitmix64 finaliser (hope_chooser_core.h's ch_mix64) */
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
HM_FN uint64_t et_key(uint64_t seed, uint64_t counter) { return et_mix64(et_mix64(seed ^ ET_TAG) ^ counter); }
HM_FN double et_uniform(uint64_t key, uint64_t scene, int d) {
    const uint64_t x = et_mix64(key ^ (2 * scene + (uint64_t)d));
    return (double)(x >> 11) * 0x1p-53;                /* 2^-53: [0, 1) */
}
HM_FN double et_clamp1(double a) { return a < -1.0 ? -1.0 : (a > 1.0 ? 1.0 : a); }     /* NaN stays NaN, as torch.clamp */
HM_FN double et_random_action(double lo, double span, double u) { return et_canon(et_clamp1(lo + span * u)); }
HM_FN bool et_box_ok(const double* box) { return box && et_finite(box[0]) && et_finite(box[1]) && et_finite(box[2]) && et_finite(box[3]); }
HM_FN EtBox et_box(const double* box) {                /* box: steer lo, steer hi, speed lo, speed hi */
    EtBox b;
    b.lo0 = box[0]; b.span0 = box[1] - box[0]; b.lo1 = box[2]; b.span1 = box[3] - box[2];
    return b;
}

HM_FN void et_begin_scene(EtState& st, const EtObs& o) {
    st.t0 = et_canon(o.t0); st.t1 = et_canon(o.t1); st.t2 = et_canon(o.t2); st.t3 = et_canon(o.t3); st.t4 = et_canon(o.t4);
    st.lx = et_canon(o.x); st.ly = et_canon(o.y);
    st.total = 0.0; st.path = 0.0;
    st.w = (1ull << 32) | ET_ALIVE | ET_STUCK;
}

/* One scene after the env step.  Returns the word the planner sees; *fin_out = the episode ended in this step. */
HM_FN uint64_t et_track_scene(EtState& st, const EtObs& o, double reward, int status, bool done, uint64_t word, bool* fin_out) {
    const bool live = (st.w & ET_ALIVE) != 0;
    uint32_t steps = (uint32_t)st.w;
    uint64_t stat = (st.w >> 32) & 0xFFull;
    if (live) {
        steps += 1u;
        st.total = et_canon(st.total + reward);
        st.path = et_canon(st.path + hm_hypot(o.x - st.lx, o.y - st.ly));
    }
    st.lx = et_canon(o.x); st.ly = et_canon(o.y);
    const bool fin = live && done;
    if (fin) stat = (uint64_t)(uint32_t)status & 0xFFull;
    const bool stuck = o.t0 == st.t0 && o.t1 == st.t1 && o.t2 == st.t2 && o.t3 == st.t3 && o.t4 == st.t4;
    st.t0 = et_canon(o.t0); st.t1 = et_canon(o.t1); st.t2 = et_canon(o.t2); st.t3 = et_canon(o.t3); st.t4 = et_canon(o.t4);
    const bool keep = live && !fin;
    st.w = (uint64_t)steps | (stat << 32) | (keep ? ET_ALIVE : 0ull) | (stuck ? ET_STUCK : 0ull);
    *fin_out = fin;
    return keep ? word : (word & ~ET_FOUND_BYTE);
}

/* float32 [4] of a scene: status, steps, (float)total, (float)path */
HM_FN void et_record(uint64_t w, double total, double path, float* r0, float* r1, float* r2, float* r3) {
    *r0 = (float)(uint32_t)((w >> 32) & 0xFFull);
    *r1 = (float)(uint32_t)w;
    *r2 = et_canon32((float)total);
    *r3 = et_canon32((float)path);
}

/* ---- the host twins: the same three operations over host arrays.  state: ET_WORDS planes, `stride` words apart, of which words
 * 0 .. n-1 are this call's scenes (stride >= n: a sub-batch of a larger block passes the block's stride and a pointer to its first
 * scene's word of plane 0).  Return HOPE_OK or HOPE_EINVAL; the hope_eval_*_host entry points forward to them. ---- */
static inline EtObs et_load_obs_host(const void* target, int obs_f64, const double* pose, size_t i) {
    EtObs o;
    if (obs_f64) { const double* q = (const double*)target + i * 5; o.t0 = q[0]; o.t1 = q[1]; o.t2 = q[2]; o.t3 = q[3]; o.t4 = q[4]; }
    else { const float* q = (const float*)target + i * 5; o.t0 = q[0]; o.t1 = q[1]; o.t2 = q[2]; o.t3 = q[3]; o.t4 = q[4]; }
    o.x = pose[i * 3]; o.y = pose[i * 3 + 1];
    return o;
}
static inline void et_store_host(uint64_t* sw, size_t S, size_t i, const EtState& st) {
    sw[i] = et_double_to_bits(st.t0); sw[S + i] = et_double_to_bits(st.t1); sw[2 * S + i] = et_double_to_bits(st.t2);
    sw[3 * S + i] = et_double_to_bits(st.t3); sw[4 * S + i] = et_double_to_bits(st.t4);
    sw[5 * S + i] = et_double_to_bits(st.lx); sw[6 * S + i] = et_double_to_bits(st.ly);
    sw[7 * S + i] = et_double_to_bits(st.total); sw[8 * S + i] = et_double_to_bits(st.path);
    sw[9 * S + i] = st.w;
}

static inline int et_begin_host(int64_t n, int64_t stride, void* state, const void* target, int obs_f64, const double* pose) {
    if (n <= 0 || stride < n || !state || !target || !pose) return HOPE_EINVAL;
    uint64_t* sw = (uint64_t*)state;
    for (int64_t s = 0; s < n; s++) {
        EtState st;
        et_begin_scene(st, et_load_obs_host(target, obs_f64, pose, (size_t)s));
        et_store_host(sw, (size_t)stride, (size_t)s, st);
    }
    return HOPE_OK;
}

static inline int et_override_host(int64_t n, int64_t stride, const void* state, const double* box, void* actions_inout, int action_is_f64,
                                   const double* u, uint64_t seed, uint64_t counter, uint64_t scene0, uint8_t* active_out) {
    if (n <= 0 || stride < n || !state || !actions_inout || !active_out || !et_box_ok(box)) return HOPE_EINVAL;
    const uint64_t* sw = (const uint64_t*)state + 9 * (size_t)stride;
    const EtBox b = et_box(box);
    const uint64_t key = et_key(seed, counter);
    for (int64_t s = 0; s < n; s++) {
        const size_t i = (size_t)s;
        const uint64_t w = sw[i];
        active_out[i] = (w & ET_ALIVE) ? 1 : 0;
        if (!(w & ET_STUCK)) continue;
        const double u0 = u ? u[2 * i] : et_uniform(key, scene0 + i, 0), u1 = u ? u[2 * i + 1] : et_uniform(key, scene0 + i, 1);
        const double a0 = et_random_action(b.lo0, b.span0, u0), a1 = et_random_action(b.lo1, b.span1, u1);
        if (action_is_f64) { ((double*)actions_inout)[2 * i] = a0; ((double*)actions_inout)[2 * i + 1] = a1; }
        else { ((float*)actions_inout)[2 * i] = et_canon32((float)a0); ((float*)actions_inout)[2 * i + 1] = et_canon32((float)a1); }
    }
    return HOPE_OK;
}

static inline int et_track_host(int64_t n, int64_t stride, void* state, const void* target, int obs_f64, const double* pose, const void* reward,
                                const int32_t* status, const uint8_t* done, const int8_t* rs_word, int8_t* word_out, uint8_t* done_out) {
    if (n <= 0 || stride < n || !state || !target || !pose || !reward || !status || !done || !rs_word || !word_out || !done_out) return HOPE_EINVAL;
    uint64_t* sw = (uint64_t*)state;
    const size_t S = (size_t)stride;
    for (int64_t s = 0; s < n; s++) {
        const size_t i = (size_t)s;
        EtState st;
        st.t0 = et_bits_to_double(sw[i]); st.t1 = et_bits_to_double(sw[S + i]); st.t2 = et_bits_to_double(sw[2 * S + i]);
        st.t3 = et_bits_to_double(sw[3 * S + i]); st.t4 = et_bits_to_double(sw[4 * S + i]);
        st.lx = et_bits_to_double(sw[5 * S + i]); st.ly = et_bits_to_double(sw[6 * S + i]);
        st.total = et_bits_to_double(sw[7 * S + i]); st.path = et_bits_to_double(sw[8 * S + i]);
        st.w = sw[9 * S + i];
        const double r = obs_f64 ? ((const double*)reward)[i] : (double)((const float*)reward)[i];
        uint64_t word;
        __builtin_memcpy(&word, rs_word + i * 8, 8);
        bool fin;
        word = et_track_scene(st, et_load_obs_host(target, obs_f64, pose, i), r, status[i], done[i] != 0, word, &fin);
        et_store_host(sw, S, i, st);
        __builtin_memcpy(word_out + i * 8, &word, 8);
        done_out[i] = fin ? 1 : 0;
    }
    return HOPE_OK;
}
