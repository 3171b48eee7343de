// hope_evaltrack_kernel.h -- the device side of the evaluation bookkeeping (include/hope_env.h "bookkeeping of an evaluation run";
// rule: hope_evaltrack_core.h).  T = the observation's type (float or double).  One lane per scene, single-wave blocks, no LDS, no
// private arrays, no scratch, no atomics; every store is a vector store.  The state planes are n-strided: a wave's load or store of
// one plane is 64 consecutive words.  About 80 B of state and 70 B of inputs per scene: launch-bound.
//
//   k_eval_begin<T>     writes the ten planes of every scene from (target, pose).
//   k_eval_override     reads the packed plane alone; writes active_out (1 B) and the action row of a stuck scene (8 / 16 B).
//   k_eval_track<T>     reads and writes the ten planes; the word copy is one 8-byte load and one 8-byte store per lane.
//   k_eval_records      float32 [n][4] (status, steps, total, path) as one 16-byte store per lane.
#pragma once
#include "hope_evaltrack_core.h"

namespace hope {

template <class T>
__device__ __forceinline__ EtObs et_load_obs(const T* __restrict__ target, const double* __restrict__ pose, size_t s) {
    EtObs o;
    const T* q = target + s * 5;
    o.t0 = (double)q[0]; o.t1 = (double)q[1]; o.t2 = (double)q[2]; o.t3 = (double)q[3]; o.t4 = (double)q[4];
    o.x = pose[s * 3]; o.y = pose[s * 3 + 1];
    return o;
}

__device__ __forceinline__ void et_store(uint64_t* __restrict__ state, size_t N, size_t s, const EtState& st) {
    state[s] = et_double_to_bits(st.t0); state[N + s] = et_double_to_bits(st.t1); state[2 * N + s] = et_double_to_bits(st.t2);
    state[3 * N + s] = et_double_to_bits(st.t3); state[4 * N + s] = et_double_to_bits(st.t4);
    state[5 * N + s] = et_double_to_bits(st.lx); state[6 * N + s] = et_double_to_bits(st.ly);
    state[7 * N + s] = et_double_to_bits(st.total); state[8 * N + s] = et_double_to_bits(st.path);
    state[9 * N + s] = st.w;
}

template <class T>
__global__ __launch_bounds__(64) void k_eval_begin(int n, const T* __restrict__ target, const double* __restrict__ pose, uint64_t* __restrict__ state) {
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (s >= n) return;
    EtState st;
    et_begin_scene(st, et_load_obs(target, pose, (size_t)s));
    et_store(state, (size_t)n, (size_t)s, st);
}

__global__ __launch_bounds__(64) void k_eval_override(int n, const uint64_t* __restrict__ state, EtBox box, void* __restrict__ actions, int act_f64,
                                                      const double* __restrict__ u, uint64_t seed, uint64_t counter, uint8_t* __restrict__ active) {
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (s >= n) return;
    const uint64_t w = state[9 * (size_t)n + s];
    active[s] = (w & ET_ALIVE) ? 1 : 0;
    if (!(w & ET_STUCK)) return;
    double u0, u1;
    if (u) { u0 = u[2 * (size_t)s]; u1 = u[2 * (size_t)s + 1]; }
    else { const uint64_t key = et_key(seed, counter); u0 = et_uniform(key, (uint64_t)s, 0); u1 = et_uniform(key, (uint64_t)s, 1); }
    const double a0 = et_random_action(box.lo0, box.span0, u0), a1 = et_random_action(box.lo1, box.span1, u1);
    if (act_f64) ((double2*)actions)[s] = make_double2(a0, a1);
    else ((float2*)actions)[s] = make_float2(et_canon32((float)a0), et_canon32((float)a1));
}

template <class T>
__global__ __launch_bounds__(64) void k_eval_track(int n, const T* __restrict__ target, const double* __restrict__ pose, const T* __restrict__ reward,
                                                   const int32_t* __restrict__ status, const uint8_t* __restrict__ done,
                                                   const uint64_t* rs_word, uint64_t* __restrict__ state, uint64_t* word_out,
                                                   uint8_t* __restrict__ done_out) {
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (s >= n) return;
    const size_t N = (size_t)n;
    EtState st;
    st.t0 = et_bits_to_double(state[s]); st.t1 = et_bits_to_double(state[N + s]); st.t2 = et_bits_to_double(state[2 * N + s]);
    st.t3 = et_bits_to_double(state[3 * N + s]); st.t4 = et_bits_to_double(state[4 * N + s]);
    st.lx = et_bits_to_double(state[5 * N + s]); st.ly = et_bits_to_double(state[6 * N + s]);
    st.total = et_bits_to_double(state[7 * N + s]); st.path = et_bits_to_double(state[8 * N + s]);
    st.w = state[9 * N + s];
    bool fin;
    const uint64_t word = et_track_scene(st, et_load_obs(target, pose, (size_t)s), (double)reward[s], status[s], done[s] != 0, rs_word[s], &fin);
    et_store(state, N, (size_t)s, st);
    word_out[s] = word;
    done_out[s] = fin ? 1 : 0;
}

__global__ __launch_bounds__(64) void k_eval_records(int n, const uint64_t* __restrict__ state, float4* __restrict__ rec) {
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (s >= n) return;
    const size_t N = (size_t)n;
    float4 r;
    et_record(state[9 * N + s], et_bits_to_double(state[7 * N + s]), et_bits_to_double(state[8 * N + s]), &r.x, &r.y, &r.z, &r.w);
    rec[s] = r;
}

}  // namespace hope
