/*
 * hope_planner_core.h -- replay of a found Reeds-Shepp path as unit actions, one source for host and device.
 *
 * The reference's RsPlanner (src/model/agent/parking_agent.py:2-47) turns a path into a LIST of actions [steer, signed fraction of a
 * full step] and pops one per env step; ParkingAgent (:49-95) adopts a new path only while none is being replayed and drops the
 * path at episode end.  Here nothing is expanded into a list: a scene keeps the five segment lengths in steps and a cursor, and the
 * next action is computed when it is popped.  k_plan (hope_planner_kernel.h) and the host twin pl_step_host /
 * hope_planner_step_host compile this header; only / - compares and int <-> double conversions are used (no libm, contraction off
 * on both compilers), so both give the same bits.
 *
 * Segment i < n_seg of type L / S / R (rs_word[i] = 1 / 0 / 2):
 *   steer = +1 / 0 / -1;  x = (double)length / step_ratio (ONE IEEE division);  ax = |x|;
 *   k     = ax > 1 ? ceil(ax) - 1 : 0 unit actions [steer, sign(x)], then
 *   rem   = ax > 1 ? sign(x) * (ax - k) : x, one action [steer, rem] kept iff ax != 1 and |rem| > 1e-3.
 * ax - k is exact, and so is the reference's repeated `-= 1` (:29-37): the two agree bit for bit.  A segment whose x is not finite
 * contributes nothing; k is clamped to 2^31 - 1.  No cap on the number of actions.
 *
 * State of a scene: PL_WORDS = 6 eight-byte words, stored as planes ([j][n_scenes], j = 0 .. 5) so that a wave reads and writes
 * whole lines: words 0 .. 4 the five x (0.0 for an unused or non-finite segment), word 5 packed --
 *   bits 0-9   segment type codes, two bits each (0 S, 1 L, 2 R)
 *   bits 10-12 cursor: the segment the next action comes from
 *   bit  13    busy
 *   bits 32-63 actions already emitted from that segment
 * An idle scene's six words are all zero; a zeroed block is "every scene idle".
 *
 * One planner step per scene, in the order HopeRollout._plan runs the torch class:
 *   1. done          -> the path is cleared (ParkingAgent.reset)
 *   2. found word    -> adopted if the scene is idle, or always with HOPE_PLAN_FORCED; a word without actions leaves it idle
 *   3. a busy scene  -> pops its next action; after the last one it is idle again (get_action :43-47)
 */
#pragma once
#include <stdint.h>

#include "hope_env.h"
#include "hope_math.h"

#define PL_WORDS HOPE_PLAN_STATE_WORDS
#define PL_BUSY (1ull << 13)
#define PL_KEEP_MIN 1e-3                               /* parking_agent.py:26, :32, :38 */

/* scalar members and no loops over them: every access has a static address, so the state stays in registers on the device */
struct PlState {
    double x0, x1, x2, x3, x4;
    uint64_t w;
};
struct PlLen {
    double l0, l1, l2, l3, l4;
};

struct PlSeg {
    uint32_t k;              /* unit actions */
    uint32_t cnt;            /* k + (remainder kept) */
    double unit;             /* sign(x) */
    double rem;
};

HM_FN double pl_bits_to_double(uint64_t u) { return __builtin_bit_cast(double, u); }
HM_FN uint64_t pl_double_to_bits(double d) { return __builtin_bit_cast(uint64_t, d); }
HM_FN bool pl_finite(double x) { return fabs(x) <= 1.7976931348623157e308; }       /* false for NaN and +-inf */
/* ceil of a finite ax >= 0 without libm: from 2^52 on every double is an integer */
HM_FN double pl_ceil(double ax) {
    if (ax >= 4503599627370496.0) return ax;
    const double t = (double)(int64_t)ax;
    return t < ax ? t + 1.0 : t;
}

HM_FN PlSeg pl_segment(double x) {
    PlSeg s;
    const double ax = fabs(x);
    s.unit = x > 0.0 ? 1.0 : (x < 0.0 ? -1.0 : 0.0);
    if (!pl_finite(x)) { s.k = 0; s.cnt = 0; s.rem = 0.0; return s; }
    const double kd = ax > 1.0 ? pl_ceil(ax) - 1.0 : 0.0;
    s.rem = ax > 1.0 ? s.unit * (ax - kd) : x;
    const bool keep = ax != 1.0 && fabs(s.rem) > PL_KEEP_MIN;
    s.k = kd > 2147483647.0 ? 2147483647u : (uint32_t)kd;
    s.cnt = s.k + (keep ? 1u : 0u);
    return s;
}

HM_FN void pl_clear(PlState& st) {
    st.x0 = 0.0; st.x1 = 0.0; st.x2 = 0.0; st.x3 = 0.0; st.x4 = 0.0;
    st.w = 0;
}

/* the first segment after `after` that holds an action, 5 if none */
HM_FN int pl_next_segment(const PlState& st, int after) {
    int next = 5;
    if (4 > after && pl_segment(st.x4).cnt > 0) next = 4;
    if (3 > after && pl_segment(st.x3).cnt > 0) next = 3;
    if (2 > after && pl_segment(st.x2).cnt > 0) next = 2;
    if (1 > after && pl_segment(st.x1).cnt > 0) next = 1;
    if (0 > after && pl_segment(st.x0).cnt > 0) next = 0;
    return next;
}

/* segment i of a word: its length in steps (0.0 when unused or not finite); its type code is or-ed into *w */
HM_FN double pl_adopt_segment(uint64_t word, int i, int n_seg, double len, double step_ratio, uint64_t* w) {
    const int t = (int)(int8_t)(word >> (8 * i));
    const bool used = i < n_seg && t >= 0;
    double x = used ? len / step_ratio : 0.0;
    if (!pl_finite(x)) x = 0.0;
    if (used && (t == HOPE_RS_L || t == HOPE_RS_R)) *w |= (uint64_t)t << (2 * i);
    return x;
}

/* RsPlanner.set_rs_path: word = the eight bytes of rs_word[s] (little endian: byte i = segment type i, byte 5 = n_seg) */
HM_FN void pl_adopt(PlState& st, uint64_t word, const PlLen& len, double step_ratio) {
    int n_seg = (int)(int8_t)(word >> 40);
    n_seg = n_seg < 0 ? 0 : (n_seg > 5 ? 5 : n_seg);
    uint64_t w = 0;
    st.x0 = pl_adopt_segment(word, 0, n_seg, len.l0, step_ratio, &w);
    st.x1 = pl_adopt_segment(word, 1, n_seg, len.l1, step_ratio, &w);
    st.x2 = pl_adopt_segment(word, 2, n_seg, len.l2, step_ratio, &w);
    st.x3 = pl_adopt_segment(word, 3, n_seg, len.l3, step_ratio, &w);
    st.x4 = pl_adopt_segment(word, 4, n_seg, len.l4, step_ratio, &w);
    const int c = pl_next_segment(st, -1);
    if (c >= 5) { pl_clear(st); return; }
    st.w = w | ((uint64_t)c << 10) | PL_BUSY;
}

/* RsPlanner.get_action of a busy scene */
HM_FN void pl_pop(PlState& st, double* out0, double* out1) {
    const int c = (int)((st.w >> 10) & 7);
    uint32_t e = (uint32_t)(st.w >> 32);
    double x = st.x0;
    x = c == 1 ? st.x1 : x;
    x = c == 2 ? st.x2 : x;
    x = c == 3 ? st.x3 : x;
    x = c == 4 ? st.x4 : x;
    const PlSeg s = pl_segment(x);
    const int code = (int)((st.w >> (2 * c)) & 3);
    *out0 = code == HOPE_RS_L ? 1.0 : (code == HOPE_RS_R ? -1.0 : 0.0);
    *out1 = e < s.k ? s.unit : s.rem;
    e++;
    int cn = c;
    if (e >= s.cnt) { e = 0; cn = pl_next_segment(st, c); }
    if (cn >= 5) { pl_clear(st); return; }
    st.w = (st.w & 0x3FFull) | ((uint64_t)cn << 10) | PL_BUSY | ((uint64_t)e << 32);
}

/* One planner step of one scene.  load_len() -> PlLen fetches the scene's segment lengths; it is called only when a word is
 * adopted.  Returns true when the state changed.  With HOPE_PLAN_NO_POP nothing is popped (planned = 0, executing = 0). */
template <class LoadLen>
HM_FN bool pl_step_scene(PlState& st, uint64_t word, bool done, int flags, double step_ratio, LoadLen load_len, double* planned0, double* planned1,
                         int* executing) {
    bool dirty = false;
    if (done && st.w != 0) { pl_clear(st); dirty = true; }
    const bool found = (int8_t)(word >> 48) > 0;
    if (found && (!(st.w & PL_BUSY) || (flags & HOPE_PLAN_FORCED))) {
        const PlLen len = load_len();
        dirty = dirty || st.w != 0;
        pl_adopt(st, word, len, step_ratio);
        dirty = dirty || st.w != 0;
    }
    *planned0 = 0.0; *planned1 = 0.0; *executing = 0;
    if (!(flags & HOPE_PLAN_NO_POP) && (st.w & PL_BUSY)) {
        pl_pop(st, planned0, planned1);
        *executing = 1;
        dirty = true;
    }
    return dirty;
}

/* The host twin: the same step over host arrays (layouts as hope_env_planner_step; state: PL_WORDS planes of n words).  Returns
 * HOPE_OK or HOPE_EINVAL; hope_planner_step_host forwards to it. */
static inline int pl_step_host(int n, double step_ratio, void* state, const int8_t* rs_word, const void* rs_lengths, int lengths_f64,
                               const uint8_t* done, int flags, double* planned_out, uint8_t* executing_out, void* actions_inout, int action_is_f64) {
    if (n <= 0 || !state || !rs_word || !rs_lengths || !(step_ratio > 0.0) || !pl_finite(step_ratio)) return HOPE_EINVAL;
    uint64_t* sw = (uint64_t*)state;
    const size_t N = (size_t)n;
    for (int s = 0; s < n; s++) {
        PlState st;
        st.x0 = pl_bits_to_double(sw[s]); st.x1 = pl_bits_to_double(sw[N + s]); st.x2 = pl_bits_to_double(sw[2 * N + s]);
        st.x3 = pl_bits_to_double(sw[3 * N + s]); st.x4 = pl_bits_to_double(sw[4 * N + s]);
        st.w = sw[5 * N + s];
        uint64_t word;
        __builtin_memcpy(&word, rs_word + (size_t)s * 8, 8);
        double p0, p1;
        int ex;
        const bool dirty = pl_step_scene(st, word, done && done[s], flags, step_ratio,
                                         [&]() {
                                             PlLen l;
                                             if (lengths_f64) { const double* q = (const double*)rs_lengths + (size_t)s * 5; l.l0 = q[0]; l.l1 = q[1]; l.l2 = q[2]; l.l3 = q[3]; l.l4 = q[4]; }
                                             else { const float* q = (const float*)rs_lengths + (size_t)s * 5; l.l0 = q[0]; l.l1 = q[1]; l.l2 = q[2]; l.l3 = q[3]; l.l4 = q[4]; }
                                             return l;
                                         },
                                         &p0, &p1, &ex);
        if (dirty) {
            sw[s] = pl_double_to_bits(st.x0); sw[N + s] = pl_double_to_bits(st.x1); sw[2 * N + s] = pl_double_to_bits(st.x2);
            sw[3 * N + s] = pl_double_to_bits(st.x3); sw[4 * N + s] = pl_double_to_bits(st.x4);
            sw[5 * N + s] = st.w;
        }
        if (flags & HOPE_PLAN_NO_POP) continue;
        if (planned_out) { planned_out[(size_t)s * 2] = p0; planned_out[(size_t)s * 2 + 1] = p1; }
        if (executing_out) executing_out[s] = (uint8_t)ex;
        if (actions_inout && ex) {
            if (action_is_f64) { ((double*)actions_inout)[(size_t)s * 2] = p0; ((double*)actions_inout)[(size_t)s * 2 + 1] = p1; }
            else { ((float*)actions_inout)[(size_t)s * 2] = (float)p0; ((float*)actions_inout)[(size_t)s * 2 + 1] = (float)p1; }
        }
    }
    return HOPE_OK;
}
