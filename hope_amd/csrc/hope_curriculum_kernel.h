// hope_curriculum_kernel.h -- the device side of the map curriculum (include/hope_env.h "curriculum for new-map draws").
//
//   k_curriculum_tally    one lane per scene, behind a step on the caller's stream: a finished scene adds its outcome to the bucket
//                         of the map it ran on (plain vector atomics: ~0.5 - 1 % of the lanes finish per step) and notes the bucket of
//                         the map it holds now IF it drew one since the bucket was noted (its episode counter moved: a finished scene
//                         that restarts on the same map keeps its bucket, whatever pool set is resident by then).  Reads done (1 B)
//                         per scene; status, scene_bucket, the two counters and cur_pool for the lanes that finished.
//   k_curriculum_weights  ONE wave: folds the counters into the windows, computes q / p_c and apportions the positions of both
//                         class lists (<= 254 groups, everything in LDS).  Runs the phases of hope_curriculum_core.h with a barrier
//                         between them -- the source the host twin compiles.
//   k_curriculum_fill     grid-stride over the positions of one class list (blockIdx.y): the group by binary search in the
//                         prefix (LDS), then the group's entries in turn; coalesced 4-byte stores.
// The step kernels are untouched: they keep reading pool_cls / pool_cls_n from StepCold, whose pointers the host swaps.
#pragma once
#include "hope_curriculum_core.h"

namespace hope {

// (CwDev, the device state of the curriculum: hope_internal.h)

// lab: labels of the pool set the step drew from ([n_lab], values 0 / 1 / 2 / 255).  done == nullptr: only note the buckets, of
// the scenes with mask[i] != 0 (behind hope_env_redraw) or of all (mask == nullptr).  episode: the handle's redraw counters;
// noted_ep: their value when scene_bucket[i] was noted.
__global__ __launch_bounds__(256) void k_curriculum_tally(int n, const int32_t* __restrict__ status, const uint8_t* __restrict__ done,
                                                           const uint8_t* __restrict__ mask, const int32_t* __restrict__ cur_pool, const uint8_t* __restrict__ lab, int n_lab,
                                                           int n_cases, uint8_t* __restrict__ scene_bucket, const uint32_t* __restrict__ episode,
                                                           uint32_t* __restrict__ noted_ep, CwDev d) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int nb = 4 + n_cases;
    if (done) {
        if (!done[i]) return;
        const int b = scene_bucket[i];
        const bool ok = status[i] == HOPE_STATUS_ARRIVED;
        const int idx = b < nb ? b : nb;                          // (255: unlabelled)
        atomicAdd(&d.episodes[idx], 1ull);
        if (ok) atomicAdd(&d.successes[idx], 1ull);
        if (b >= 4 && b < nb) {                                   // a Dragon-Lake case: also "dlp" as a scene type
            atomicAdd(&d.episodes[3], 1ull);
            if (ok) atomicAdd(&d.successes[3], 1ull);
        }
    } else if (mask && !mask[i]) return;
    const uint32_t ep = episode[i];
    if (done && ep == noted_ep[i]) return;                        // no new map since the bucket was noted
    noted_ep[i] = ep;
    const int j = cur_pool[i];
    int now = CW_UNLABELLED;
    if (j >= 0) { if (lab && j < n_lab) now = lab[j]; }
    else if (j <= -2 && -2 - j < n_cases) now = 4 + (-2 - j);
    scene_bucket[i] = (uint8_t)now;
}

// hope_env_set_scenes while the curriculum is on: the uploaded maps are unlabelled
__global__ void k_curriculum_forget(int n, const int32_t* __restrict__ ids, uint8_t* __restrict__ scene_bucket, const uint32_t* __restrict__ episode,
                                    uint32_t* __restrict__ noted_ep) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const int s = ids[k];
    scene_bucket[s] = CW_UNLABELLED;
    noted_ep[s] = episode[s];
}

struct CwJob {
    hope_curriculum_params P;
    CwClass cls[2];
    int n_cases;
    int fold;                        // 1: fold the counters since the last update into the windows first
    int32_t* prefix;                 // [2][CW_MAX_GROUPS + 1] out
};

__global__ __launch_bounds__(64) void k_curriculum_weights(CwJob job, CwDev d) {
    __shared__ double s_n[CW_MAX_GROUPS], s_s[CW_MAX_GROUPS], s_prob[CW_MAX_GROUPS], s_w[CW_MAX_GROUPS], s_r[CW_MAX_GROUPS];
    __shared__ int32_t s_f[CW_MAX_GROUPS], s_pos[CW_MAX_GROUPS], s_prefix[CW_MAX_GROUPS + 1];
    __shared__ unsigned long long s_eps[4];
    const int lane = threadIdx.x, nl = blockDim.x;
    const int nb = 4 + job.n_cases, G = nb;
    for (int b = lane; b < nb; b += nl) {
        double n = d.win_n[b], s = d.win_s[b];
        const unsigned long long e = d.episodes[b];
        if (job.fold) {
            // a tally enqueued behind the update may be adding while this reads: the two counters of a bucket are separate atomics,
            // so a success may be visible before its episode.  Never fold more successes than episodes; the rest waits for the next update.
            const unsigned long long de = e - d.folded_e[b], ds_seen = d.successes[b] - d.folded_s[b];
            const unsigned long long dsu = ds_seen < de ? ds_seen : de;
            const double dn = (double)de, ds = (double)dsu;
            cw_fold(&n, &s, dn, ds, b < 4 ? job.P.type_window : job.P.case_window);
            d.folded_e[b] = e; d.folded_s[b] = d.folded_s[b] + dsu;
            d.win_n[b] = n; d.win_s[b] = s;
        }
        s_n[b] = n; s_s[b] = s;
        if (b < 4) s_eps[b] = job.fold ? e : d.folded_e[b];       // the horizons look at what has been folded
    }
    __syncthreads();
    const unsigned long long type_eps = s_eps[0] + s_eps[1] + s_eps[2] + s_eps[3], dlp_eps = s_eps[3];
    if (lane == 0) {
        double pw[4], q[4];
        cw_type_probs(s_n, s_s, &job.P, type_eps, pw, q);
        for (int t = 0; t < 4; t++) { s_prob[t] = q[t]; d.pw[t] = pw[t]; }
    }
    cw_case_fail_phase(s_n, s_s, job.n_cases, &job.P, s_w, lane, nl);
    __syncthreads();
    cw_case_prob_phase(job.n_cases, &job.P, dlp_eps, s_w, s_prob, lane, nl);
    __syncthreads();
    for (int b = lane; b < nb; b += nl) d.prob[b] = s_prob[b];
    const CwWork k = {s_w, s_r, s_f, s_pos, s_prefix};
    for (int c = 0; c < 2; c++) {
        __syncthreads();
        if (cw_n_base(job.cls[c]) <= 0) {                         // (uniform over the whole block: a kernel argument)
            for (int g = lane; g <= G; g += nl) job.prefix[c * (CW_MAX_GROUPS + 1) + g] = 0;
            continue;
        }
        cw_weight_phase(job.cls[c], G, s_prob, k, lane, nl);
        __syncthreads();
        cw_remainder_phase(G, k, lane, nl);
        __syncthreads();
        if (lane == 0) cw_prefix_phase(G, k);
        __syncthreads();
        for (int g = lane; g <= G; g += nl) job.prefix[c * (CW_MAX_GROUPS + 1) + g] = s_prefix[g];
    }
}

struct CwFill {
    CwClass cls[2];
    int G;
    const int32_t* prefix;           // [2][CW_MAX_GROUPS + 1]
    const int32_t* sorted[2];        // the class's pool entries ordered by group
    int32_t* out[2];                 // [CW_LIST_LEN]
};

__global__ __launch_bounds__(256) void k_curriculum_fill(CwFill f) {
    __shared__ int32_t s_prefix[CW_MAX_GROUPS + 1];
    const int c = blockIdx.y;
    if (cw_n_base(f.cls[c]) <= 0) return;
    for (int g = threadIdx.x; g <= f.G; g += blockDim.x) s_prefix[g] = f.prefix[c * (CW_MAX_GROUPS + 1) + g];
    __syncthreads();
    int32_t* out = f.out[c];
    for (int pos = blockIdx.x * blockDim.x + threadIdx.x; pos < CW_LIST_LEN; pos += gridDim.x * blockDim.x)
        out[pos] = cw_entry(f.cls[c], f.G, s_prefix, f.sorted[c], pos);
}

}  // namespace hope
