// hope_planner_kernel.h -- the device side of the path replay (include/hope_env.h "replay of found Reeds-Shepp paths").
//
//   k_plan        one lane per scene, behind a step on the caller's stream: runs pl_step_scene of hope_planner_core.h -- the source
//                 the host twin compiles.  Per scene it reads rs_word (one 8-byte load), done (1 B) and the packed state word; the
//                 five x only of a busy scene, rs_lengths only when a word is adopted.  It writes planned (16 B), executing (1 B), the
//                 action row of an executing scene and the state of a scene whose state changed.  No LDS, no scratch; launch-bound
//                 (~150 B per scene at most).
//   k_plan_reset  clears the path of the scenes with mask[s] != 0.
#pragma once
#include "hope_planner_core.h"

namespace hope {

__global__ __launch_bounds__(64) void k_plan(int n, const uint64_t* __restrict__ rs_word, const void* __restrict__ rs_lengths, int len_f64,
                                             const uint8_t* __restrict__ done, int flags, double step_ratio, uint64_t* __restrict__ state,
                                             double2* __restrict__ planned, uint8_t* __restrict__ executing, void* __restrict__ actions, int act_f64) {
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (s >= n) return;
    const size_t N = (size_t)n;
    PlState st;
    st.w = state[5 * N + s];
    st.x0 = 0.0; st.x1 = 0.0; st.x2 = 0.0; st.x3 = 0.0; st.x4 = 0.0;
    if (st.w != 0) {                                              // (an idle scene's words are all zero)
        st.x0 = pl_bits_to_double(state[s]); st.x1 = pl_bits_to_double(state[N + s]); st.x2 = pl_bits_to_double(state[2 * N + s]);
        st.x3 = pl_bits_to_double(state[3 * N + s]); st.x4 = pl_bits_to_double(state[4 * N + s]);
    }
    const uint64_t word = rs_word[s];
    const bool d = done && done[s];
    double p0, p1;
    int ex;
    const bool dirty = pl_step_scene(st, word, d, flags, step_ratio,
                                     [&]() {
                                         PlLen l;
                                         if (len_f64) { const double* q = (const double*)rs_lengths + (size_t)s * 5; l.l0 = q[0]; l.l1 = q[1]; l.l2 = q[2]; l.l3 = q[3]; l.l4 = q[4]; }
                                         else { const float* q = (const float*)rs_lengths + (size_t)s * 5; l.l0 = q[0]; l.l1 = q[1]; l.l2 = q[2]; l.l3 = q[3]; l.l4 = q[4]; }
                                         return l;
                                     },
                                     &p0, &p1, &ex);
    if (dirty) {
        state[s] = pl_double_to_bits(st.x0); state[N + s] = pl_double_to_bits(st.x1); state[2 * N + s] = pl_double_to_bits(st.x2);
        state[3 * N + s] = pl_double_to_bits(st.x3); state[4 * N + s] = pl_double_to_bits(st.x4);
        state[5 * N + s] = st.w;
    }
    if (flags & HOPE_PLAN_NO_POP) return;
    if (planned) planned[s] = make_double2(p0, p1);
    if (executing) executing[s] = (uint8_t)ex;
    if (actions && ex) {
        if (act_f64) ((double2*)actions)[s] = make_double2(p0, p1);
        else ((float2*)actions)[s] = make_float2((float)p0, (float)p1);
    }
}

__global__ __launch_bounds__(64) void k_plan_reset(int n, const uint8_t* __restrict__ mask, uint64_t* __restrict__ state) {
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (s >= n || !mask[s]) return;
    const size_t N = (size_t)n;
    if (state[5 * N + s] == 0) return;
    for (int j = 0; j < PL_WORDS; j++) state[j * N + s] = 0;
}

}  // namespace hope
