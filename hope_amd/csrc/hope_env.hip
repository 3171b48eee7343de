// hope_env.hip -- host side of the C ABI (include/hope_env.h) + the fused step kernel instantiation: create / destroy, step launcher,
// scene pool, curriculum, debug.  (The handle and the entry prologue: hope_handle.h; planner, chooser, normalisation, evaluation: hope_agent.hip.)
// gfx950 only; no CPU fallback: every entry point fails with HOPE_ENODEV/HOPE_EHIP when no device works.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <chrono>
#include <string>
#include <vector>

#include "hope_dev.h"
#include "hope_handle.h"
#include "hope_step_kernel.h"
#include "hope_obs_pair.h"
#include "hope_motion_pair.h"
#include "hope_scenegen_kernel.h"
#include "hope_curriculum_kernel.h"
#include "hope_maplevel_kernel.h"

using namespace hope;

static thread_local std::string g_err;
int hope::fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

#include <mutex>
#include <unordered_set>
static std::mutex g_live_m;
static std::unordered_set<const void*> g_live;
bool hope::is_live(const void* h) {
    std::lock_guard<std::mutex> lk(g_live_m);
    return h && g_live.count(h) != 0;
}

static hipEvent_t get_event(hope_env* h) {
    if (!h->free_events.empty()) { hipEvent_t e = h->free_events.back(); h->free_events.pop_back(); return e; }
    hipEvent_t e;
    if (hipEventCreate(&e) != hipSuccess) return nullptr;
    return e;
}
struct EventTimer : LaunchTimer {
    hope_env* h;
    hipEvent_t a = nullptr, b = nullptr;
    int kind = 0;
    bool failed = false, skip = false;
    explicit EventTimer(hope_env* h_) : h(h_) {}
    void begin(int k, hipStream_t s) override {
        kind = k;
        skip = !((h->profile_mask >> k) & 1u);
        if (skip) return;
        a = get_event(h); b = get_event(h);
        if (!a || !b || hipEventRecord(a, s) != hipSuccess) failed = true;
    }
    void end(hipStream_t s) override {
        if (skip) return;
        if (failed || hipEventRecord(b, s) != hipSuccess) { failed = true; return; }
        h->pending.push_back({a, b, kind, h->step_seq});
    }
};

static int drain_events(hope_env* h) {
    // per launch: duration; per (call, kernel): the union of its launches' intervals (with HOPE_F_OVERLAP the launches of the
    // two tile classes run concurrently on two streams; event times are compared through hipEventElapsedTime)
    for (size_t i = 0; i < h->pending.size(); i++) {
        auto& p = h->pending[i];
        float ms = 0;
        hipError_t e = hipEventSynchronize(p.b);
        if (e == hipSuccess) e = hipEventElapsedTime(&ms, p.a, p.b);
        if (e != hipSuccess) return fail(HOPE_EHIP, std::string("event timing: ") + hipGetErrorString(e));
        h->ms[p.kind] += ms;
        h->launches[p.kind] += 1;
    }
    for (size_t i = 0; i < h->pending.size(); i++) {
        auto& p = h->pending[i];
        if (!p.a) continue;                                   // already merged into an earlier launch of its call
        // intervals of this (call, kernel) relative to p.a: merge (at most a handful per call)
        std::vector<std::pair<float, float>> iv;
        for (size_t j = i; j < h->pending.size(); j++) {
            auto& q = h->pending[j];
            if (!q.a || q.kind != p.kind || q.seq != p.seq) continue;
            float t0 = 0, t1 = 0;
            hipError_t e = hipSuccess;
            if (j != i) { hipEventSynchronize(q.b); e = hipEventElapsedTime(&t0, p.a, q.a); }
            if (e == hipSuccess) e = hipEventElapsedTime(&t1, p.a, q.b);
            if (e != hipSuccess) { t0 = 0; t1 = 0; }          // (a later event recorded "before" the reference: negative times are fine)
            iv.push_back({t0, t1});
            if (j != i) { h->free_events.push_back(q.a); h->free_events.push_back(q.b); q.a = nullptr; }
        }
        std::sort(iv.begin(), iv.end());
        double total = 0, lo = iv[0].first, hi = iv[0].second;
        for (size_t k = 1; k < iv.size(); k++) {
            if (iv[k].first <= hi) hi = std::max<double>(hi, iv[k].second);
            else { total += hi - lo; lo = iv[k].first; hi = iv[k].second; }
        }
        total += hi - lo;
        h->union_ms[p.kind] += total;
        h->union_calls[p.kind] += 1;
        h->free_events.push_back(p.a);
        h->free_events.push_back(p.b);
        p.a = nullptr;
    }
    h->pending.clear();
    return HOPE_OK;
}

// ------------------------------------------------------------------------------------------------
// scene upload kernels
// ------------------------------------------------------------------------------------------------
namespace {

// one thread per uploaded scene: constants, derived dest box, episode state reset
__global__ void k_set_scene_consts(int n, const int32_t* ids, const double* start, const double* dest,
                                   const double* bbox, const int32_t* nob, double* scene_c, double* state,
                                   int32_t* tstep, int32_t* n_obst, double* traj, int32_t* traj_len, int32_t* traj_valid,
                                   int32_t* layer_valid) {
    int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    int s = ids ? ids[k] : k;
    double* c = scene_c + (size_t)s * SC_WORDS;
    fill_scene_consts(c, start + 3 * k, dest + 3 * k, bbox + 4 * k);
    if (!state) return;                                           // (pool entries: constants only)
    double* st = state + (size_t)s * ST_WORDS;
    st[0] = start[3 * k]; st[1] = start[3 * k + 1]; st[2] = start[3 * k + 2]; st[3] = 0.0;
    tstep[s] = 0;
    n_obst[s] = nob[k];
    if (traj) {                                                   // vehicle.reset: trajectory = [start]  vehicle.py:132-133
        double* tr = traj + (size_t)s * BEV_TRAJ_LEN * 3;
        tr[0] = st[0]; tr[1] = st[1]; tr[2] = st[2];
        traj_len[s] = 1;
        traj_valid[s] = 0;
        layer_valid[s] = 0;                                           // a new map: the static image layer is rebuilt
    }
}

// hope_env_create's hardware-queue measurement: one wave that idles for `ticks` of the 100 MHz real-time counter
// and reports when it ran (stamps[0] = first, stamps[1] = last reading of the counter, which all queues share): two spins on streams of
// DIFFERENT hardware queues overlap in time, two on the same queue cannot -- decided on the GPU's own clock, not the host's
__global__ void k_spin(long long ticks, long long* stamps) {
    const long long t0 = (long long)wall_clock64();
    long long t1 = t0;
    while (t1 - t0 < ticks) { __builtin_amdgcn_s_sleep(16); t1 = (long long)wall_clock64(); }
    if (stamps && threadIdx.x == 0) { stamps[0] = t0; stamps[1] = t1; }
}

__global__ void k_debug_math(int fn, int n, const double* a, const double* b, double* out) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double x = a[i], y = b ? b[i] : 0.0, r;
    switch (fn) {
        case 0: r = hm_sin(x); break;
        case 1: r = hm_cos(x); break;
        case 2: r = hm_tan(x); break;
        case 3: r = hm_atan2(x, y); break;
        case 4: r = hm_asin(x); break;
        case 5: r = hm_acos(x); break;
        case 6: r = hm_hypot(x, y); break;
        case 7: r = hm_fmod(x, y); break;
        case 8: r = hm_tanh(x); break;
        case 9: r = hm_exp(x); break;
        case 10: r = sqrt(x); break;
        case 12: r = div_by_20(x); break;                  // k_kinematics' division by MINI_ITER (hope_step_kernel.h)
        case 13: r = mask_fraction((int)x); break;         // the action mask's k / n_iter (hope_step_kernel.h)
        default: r = x / y; break;
    }
    out[i] = r;
}

// hope_debug_geom: the geometry primitives of hope_dev.h / hope_step_kernel.h on packed test cases, called the way the step kernels
// call them.  One 64-lane wave per block.  REC doubles per case in; int32 (fn 0-5, 9) or float64 (fn 6-8) out.  fn 1, 2, 4: the 64
// lanes hold 64 cases and take the ONE work area xl one lane at a time (the loop of k_env_step's multi-sub-step pass); fn 5, 6: one
// case per block; fn 7: the lanes clip CLIP_COLS cases at a time in the column layout (the loop of k_post).
constexpr int DEBUG_GEOM_FNS = 10, DEBUG_GEOM_MAX_OBST = 32;
__host__ __device__ inline int debug_geom_rec(int fn, int n_obst) {
    return fn <= 2 ? 6 : (fn == 3 || fn == 4 || fn == 9) ? 8 : (fn == 5 ? 4 + 8 * n_obst : (fn == 8 ? 4 : 16));
}
template <int FN>
__global__ __launch_bounds__(64) void k_debug_geom(int n, int n_obst, const double* in, void* out) {
    __shared__ double xl[ROBUST_LDS_WORDS];
    const int lane = threadIdx.x;
    int32_t* oi = (int32_t*)out;
    double* od = (double*)out;
    if (FN == 5) {                                              // detect_collision by the whole wave: block = case
        __shared__ double tile[8 * DEBUG_GEOM_MAX_OBST];
        __shared__ int list[DEBUG_GEOM_MAX_OBST];
        const int c = blockIdx.x;
        if (c >= n || n_obst > DEBUG_GEOM_MAX_OBST) return;
        const double* v = in + (size_t)c * debug_geom_rec(5, n_obst);
        for (int i = lane; i < 8 * n_obst; i += WAVE) tile[i] = v[4 + i];
        for (int i = lane; i < n_obst; i += WAVE) list[i] = i;
        __syncthreads();
        unsigned und = 0;
        const bool hit = detect_collision(v[0], v[1], v[2], v[3], tile, list, n_obst, xl, lane, &und);
        if (lane == 0) { oi[2 * c] = hit; oi[2 * c + 1] = (int32_t)und; }
        return;
    }
    if (FN == 6) {                                              // the one-lane clip: block = case, operands in LDS as in overlap_area
        __shared__ double sh[64];
        __shared__ double dbox[8];
        const int c = blockIdx.x;
        if (c >= n) return;
        const double* v = in + (size_t)c * 16;
        if (lane < 8) dbox[lane] = v[8 + lane];
        __syncthreads();
        if (lane == 0) {
#pragma unroll
            for (int i = 0; i < 4; i++) { sh[i] = v[2 * i]; sh[16 + i] = v[2 * i + 1]; }
            od[c] = quad_intersection_area_lane0(dbox, sh);
        }
        return;
    }
    const int i = blockIdx.x * WAVE + lane;
    const bool live = i < n;
    const double* v = in + (size_t)(live ? i : 0) * debug_geom_rec(FN, 0);
    if (FN == 7) {                                              // the column clip, CLIP_COLS lanes at a time (k_post's loop)
        __shared__ double clip_lds[32 * CLIP_COLS];
        double area = 0.0;
        unsigned long long cm = __ballot(live);
        while (cm) {
            const int rank = __popcll(cm & ((1ull << lane) - 1));
            const bool mine = live && ((cm >> lane) & 1) && rank < CLIP_COLS;
            if (mine) {
                double* sh = clip_lds + rank;
#pragma unroll
                for (int k = 0; k < 4; k++) { sh[k * CLIP_COLS] = v[2 * k]; sh[(8 + k) * CLIP_COLS] = v[2 * k + 1]; }
                area = quad_intersection_area_private(v + 8, sh);
            }
            unsigned long long served = 0;
            {
                unsigned long long t_ = cm;
                for (int k = 0; k < CLIP_COLS && t_; k++) { served |= t_ & (~t_ + 1); t_ &= t_ - 1; }
            }
            cm &= ~served;
            __syncthreads();
        }
        if (live) od[i] = area;
        return;
    }
    if (FN == 1 || FN == 2 || FN == 4) {                        // one lane at a time in the shared work area
        int r = 0;
        unsigned long long um = __ballot(live);
        while (um) {
            const int l = __ffsll((long long)um) - 1;
            um &= um - 1;
            if (lane == l) {
                if (FN == 1) r = orient_exact_lds(v[0], v[1], v[2], v[3], v[4], v[5], xl + 12);
                if (FN == 2) r = orient_robust_lds(v[0], v[1], v[2], v[3], v[4], v[5], xl + 12);
                if (FN == 4) r = hull_edge_intersect_robust(v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], xl);
            }
        }
        if (live) oi[i] = r;
        return;
    }
    if (!live) return;
    if (FN == 0) oi[i] = orient_filter(v[0], v[1], v[2], v[3], v[4], v[5]);
    if (FN == 3) oi[i] = segments_intersect_fast(v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7]);
    if (FN == 8) od[i] = origin_seg_dist(v[0], v[1], v[2], v[3]);
    if (FN == 9) oi[i] = arrival_possible(v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7]);
}

// Calibration of the memory-side traffic counters (FETCH_SIZE / WRITE_SIZE) on THIS library's access widths: a grid-stride sweep
// over a buffer far larger than the 256 MiB Infinity Cache, with a known byte count (tools/pmc_calib.py).  MODE: reads 0 = 16 B per
// lane (the obstacle tile copies; the guide's calibrated case), 1 = 8 B per lane (kin / post / table rows), 2 = 4 B per lane, 3 = one
// 8-byte word per 64-byte line (one lane per scene record); writes 4 = 16 B, 5 = 8 B, 6 = 4 B per lane (float32 observations),
// 7 = one 8-byte word per 64-byte line.
template <int MODE>
__global__ __launch_bounds__(256) void k_traffic_calib(size_t bytes, const char* src, char* dst, double* sink) {
    const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, nth = (size_t)gridDim.x * blockDim.x;
    double acc = 0.0;
    if (MODE == 0) { const double2* q = (const double2*)src; for (size_t i = tid; i < bytes / 16; i += nth) { const double2 v = q[i]; acc += v.x + v.y; } }
    if (MODE == 1) { const double* q = (const double*)src; for (size_t i = tid; i < bytes / 8; i += nth) acc += q[i]; }
    if (MODE == 2) { const float* q = (const float*)src; for (size_t i = tid; i < bytes / 4; i += nth) acc += (double)q[i]; }
    if (MODE == 3) { const double* q = (const double*)src; for (size_t i = tid; i < bytes / 64; i += nth) acc += q[8 * i]; }
    if (MODE == 4) { double2* q = (double2*)dst; for (size_t i = tid; i < bytes / 16; i += nth) q[i] = make_double2((double)i, 1.0); }
    if (MODE == 5) { double* q = (double*)dst; for (size_t i = tid; i < bytes / 8; i += nth) q[i] = (double)i; }
    if (MODE == 6) { float* q = (float*)dst; for (size_t i = tid; i < bytes / 4; i += nth) q[i] = (float)i; }
    if (MODE == 7) { double* q = (double*)dst; for (size_t i = tid; i < bytes / 64; i += nth) q[8 * i] = (double)i; }
    if (MODE < 4 && acc == 1.2345e301) sink[0] = acc;       // (keeps the loads)
}

// episode restart: pose = start, t = 0, accum = 0 for masked scenes
__global__ void k_restart(int n, const uint8_t* mask, const double* scene_c, double* state, int32_t* tstep, double* traj,
                          int32_t* traj_len, int32_t* traj_valid) {
    int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n || !mask[s]) return;
    const double* c = scene_c + (size_t)s * SC_WORDS;
    double* st = state + (size_t)s * ST_WORDS;
    st[0] = c[SC_START]; st[1] = c[SC_START + 1]; st[2] = c[SC_START + 2]; st[3] = 0.0;
    tstep[s] = 0;
    if (traj) {
        double* tr = traj + (size_t)s * BEV_TRAJ_LEN * 3;
        tr[0] = st[0]; tr[1] = st[1]; tr[2] = st[2];
        traj_len[s] = 1;
        traj_valid[s] = 0;
    }
}

// New map at episode turnover (map.reset + vehicle.reset, car_parking_base.py:127-137), without the host: a finished scene
// (mask) takes a pool entry of ITS tile class -- the dense per-class launch lists stay valid -- picked by a counter-based
// hash of (seed, scene, episodes drawn so far), copies its obstacle tile and constants and restarts.  One wave per scene.
__global__ __launch_bounds__(64) void k_redraw(int max_obst, const uint8_t* mask, uint64_t seed, const int32_t* pl0, int n0,
                                               const int32_t* pl1, int n1, const double* pverts, const double* pc,
                                               const int32_t* pnob, double* verts, double* scene_c, int32_t* n_obst,
                                               double* state, int32_t* tstep, double* traj, int32_t* traj_len,
                                               int32_t* traj_valid, int32_t* cur_pool, uint32_t* episode, float4* obb, DlpCases dlp,
                                               int32_t* overflow, const uint8_t* slot_cls, int32_t* layer_valid, float4* fverts,
                                               float4* fbox, uint8_t* eflag) {
    __shared__ double c24[SC_WORDS];
    const int s = blockIdx.x, lane = threadIdx.x;
    if (!mask[s]) return;
    const int cls = slot_cls[s] ? 1 : 0;
    const int32_t* pl = cls ? pl1 : pl0;
    const int cnt = cls ? n1 : n0;
    const uint32_t ep = episode[s];
    __syncthreads();
    double* c = scene_c + (size_t)s * SC_WORDS;
    if (cnt > 0) {
        const uint64_t key = mix64(seed ^ mix64(((uint64_t)s << 32) | ep));
        const int j = pl[(int)(key % (uint64_t)cnt)];
        int nob;
        if (j >= 0) {
            nob = pnob[j];
            const double2* src = (const double2*)(pverts + (size_t)j * max_obst * 8);
            double2* dst = (double2*)(verts + (size_t)s * max_obst * 8);
            for (int v = lane; v < 4 * nob; v += WAVE) dst[v] = src[v];
            const double fox = pc[(size_t)j * SC_WORDS + SC_BBOX], foy = pc[(size_t)j * SC_WORDS + SC_BBOX + 2];
            for (int o = lane; o < nob; o += WAVE) {
                const double* pv = pverts + ((size_t)j * max_obst + o) * 8;
                obb[(size_t)s * max_obst + o] = obstacle_box(pv);
                obstacle_f32(pv, fox, foy, fverts + ((size_t)s * max_obst + o) * 2, fbox + (size_t)s * max_obst + o,
                             eflag + (size_t)s * eflag_stride(max_obst) + o);
            }
            if (lane < SC_WORDS) c24[lane] = pc[(size_t)j * SC_WORDS + lane];
        } else                                                // a Dragon-Lake-Parking case, drawn exactly as the fused turnover draws it
            nob = draw_dlp_case(dlp, -2 - j, mix64(key ^ 0xD1B54A32D192ED03ull), max_obst, verts + (size_t)s * max_obst * 8,
                                obb + (size_t)s * max_obst, fverts + (size_t)s * max_obst * 2, fbox + (size_t)s * max_obst,
                                eflag + (size_t)s * eflag_stride(max_obst), c24, nullptr, overflow, lane);
        __syncthreads();
        if (lane < SC_WORDS) c[lane] = c24[lane];
        if (lane == 0) { n_obst[s] = nob; cur_pool[s] = j; if (layer_valid) layer_valid[s] = 0; }
    } else if (lane < SC_WORDS) c24[lane] = c[lane];
    __syncthreads();
    if (lane == 0) {
        episode[s] = ep + 1;
        double* st = state + (size_t)s * ST_WORDS;
        st[0] = c24[SC_START]; st[1] = c24[SC_START + 1]; st[2] = c24[SC_START + 2]; st[3] = 0.0;
        tstep[s] = 0;
        if (traj) {
            double* tr = traj + (size_t)s * BEV_TRAJ_LEN * 3;
            tr[0] = st[0]; tr[1] = st[1]; tr[2] = st[2];
            traj_len[s] = 1;
            traj_valid[s] = 0;
        }
    }
}

// Reeds-Shepp work queues: the flagged scenes of each tile class (blockIdx.y), compacted.  Each block scans its share
// of the class's scene list (thread = a few consecutive entries, block-wide exclusive scan) and reserves one
// contiguous range of the queue with a single atomicAdd.
// Small workgroups on purpose: the kernel runs while other streams keep every CU busy with one-wave workgroups, and a
// 1024-thread workgroup then waits for 16 free wave slots on ONE CU (measured: up to 0.4 ms of queueing).
#ifndef HOPE_COMPACT_THREADS
#define HOPE_COMPACT_THREADS 256
#endif
constexpr int COMPACT_THREADS = HOPE_COMPACT_THREADS;
// The gate itself (car_parking_base.py:293-294: t > 1, status CONTINUE, closer than RS_MAX_DIST to the dest -- of the
// finished step, from k_env_step's hand-over record) is evaluated here, and the Reeds-Shepp outputs of every scene of the
// class are cleared here, so that the chain motion -> compact -> words -> segs -> validate does not wait for k_post.
// One thread per scene: the queue is sorted by scene inside each block's 256 scenes; the blocks append in arrival order.
template <typename OT>
__global__ __launch_bounds__(COMPACT_THREADS) void k_rs_compact(const int32_t* list, int n, uint8_t* flag, const uint8_t* active,
                                                                 int32_t* out, int32_t* rs_count, const double* post,
                                                                 const double* scene_c, int8_t* rs_word, void* rs_lengths, const int32_t* n_obst,
                                                                 int32_t* surv_count, double* rs_in) {
    __shared__ int wsum[COMPACT_THREADS / WAVE];
    __shared__ int base;
    if (surv_count && blockIdx.x == 0 && threadIdx.x == 0) *surv_count = 0;    // k_rs_screen's queue of this chain (same stream, behind the last walk)
    const int i = blockIdx.x * COMPACT_THREADS + threadIdx.x;
    int s = -1;
    bool gate = false;
    if (i < n) {
        s = list[i];
        if (!active || active[s]) {
            const double* pr = post + (size_t)s * POST_WORDS;
            const double* sc = scene_c + (size_t)s * SC_WORDS;
            const int packed = __double2loint(pr[7]);
            const int status = packed & 0xff, t = packed >> 8;
            const double ddx = pr[3] - sc[SC_DEST], ddy = pr[4] - sc[SC_DEST + 1];
            gate = t > 1 && status == HOPE_STATUS_CONTINUE && sqrt(ddx * ddx + ddy * ddy) < RS_MAX_DIST;
            flag[s] = gate;
            // cleared here; k_rs_validate fills them for the scenes whose search finds a path: {NONE x 5, 0, 0, 0}
            const unsigned long long none = (unsigned char)HOPE_RS_NONE;
            *(unsigned long long*)(rs_word + 8 * (size_t)s) = none | none << 8 | none << 16 | none << 24 | none << 32;
            if (rs_lengths) {
#pragma unroll
                for (int k = 0; k < 5; k++) ((OT*)rs_lengths)[5 * (size_t)s + k] = (OT)0;
            }
        }
    }
    // exclusive scan over the block: inside the wave by ballot, across the 4 waves through LDS
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
    const unsigned long long m = __ballot(gate);
    const int before = __popcll(m & ((1ull << lane) - 1));
    if (lane == 0) wsum[wave] = __popcll(m);
    __syncthreads();
    int woff = 0, total = 0;
    for (int w = 0; w < COMPACT_THREADS / WAVE; w++) { if (w < wave) woff += wsum[w]; total += wsum[w]; }
    if (threadIdx.x == 0) base = total ? atomicAdd(rs_count, total) : 0;
    __syncthreads();
    if (gate) {
        const int qpos = base + woff + before;
        out[qpos] = rs_list_pack(s, n_obst[s]);                                     // (hope_internal.h)
        // the search's inputs by queue position (RS_IN_WORDS): the pose is the finished step's final pose (CONTINUE: also what
        // `state` holds), so nothing behind this kernel on the search stream reads `state` / `post` / the scene constants
        const double* pr = post + (size_t)s * POST_WORDS;
        const double* sc = scene_c + (size_t)s * SC_WORDS;
        double* in = rs_in + (size_t)qpos * RS_IN_WORDS;
        const double q0x = pr[3], q0y = pr[4], q0w = pr[5];
        in[0] = q0x; in[1] = q0y; in[2] = q0w;
        in[3] = sc[SC_BBOX]; in[4] = sc[SC_BBOX + 1]; in[5] = sc[SC_BBOX + 2]; in[6] = sc[SC_BBOX + 3];
        // generate_path (reeds_shepp.py:540-557): the goal in the start frame, scaled by the maximum curvature
        const double dx = sc[SC_DEST] - q0x, dy = sc[SC_DEST + 1] - q0y;
        const double PHI = sc[SC_DEST + 2] - q0w;
        const double c = hm_cos(q0w), sn = hm_sin(q0w);
        const double X = (c * dx + sn * dy) * RS_MAXC;
        const double Y = (-sn * dx + c * dy) * RS_MAXC;
        double sPHI, cPHI;                                    // hm_sincos is exactly odd / even: serves -PHI too
        hm_sincos(PHI, &sPHI, &cPHI);
        in[7] = X; in[8] = Y; in[9] = PHI; in[10] = sPHI; in[11] = cPHI;
        in[12] = X * cPHI + Y * sPHI;                         // "backwards" (:206-207, :376-377)
        in[13] = X * sPHI - Y * cPHI;
    }
}

// one block per uploaded scene: copy its obstacle tile
__global__ void k_set_scene_tiles(const int32_t* ids, const int32_t* nob, const double* verts_in, const double* bbox_in, double* verts,
                                  float4* obb, float4* fverts, float4* fbox, uint8_t* eflag, int max_obst) {
    int k = blockIdx.x;
    int s = ids ? ids[k] : k;
    const double2* src = (const double2*)(verts_in + (size_t)k * max_obst * 8);
    double2* dst = (double2*)(verts + (size_t)s * max_obst * 8);
    int nv = 4 * nob[k];
    for (int v = threadIdx.x; v < nv; v += blockDim.x) dst[v] = src[v];
    if (obb) {
        const double fox = bbox_in[4 * (size_t)k], foy = bbox_in[4 * (size_t)k + 2];          // frame origin of the float32 view
        for (int o = threadIdx.x; o < nob[k]; o += blockDim.x) {
            const double* pv = verts_in + ((size_t)k * max_obst + o) * 8;
            obb[(size_t)s * max_obst + o] = obstacle_box(pv);
            obstacle_f32(pv, fox, foy, fverts + ((size_t)s * max_obst + o) * 2, fbox + (size_t)s * max_obst + o,
                         eflag + (size_t)s * eflag_stride(max_obst) + o);
        }
    }
}

}  // namespace

// ------------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------------
template <int PART, bool FKIN = false>
static void launch_env_step(bool of64, bool af64, dim3 grid, dim3 block, size_t lds, hipStream_t sc, const StepParams& p) {
    if (of64 && af64) hipLaunchKernelGGL((k_env_step<double, double, false, PART, FKIN>), grid, block, lds, sc, p);
    else if (of64) hipLaunchKernelGGL((k_env_step<double, float, false, PART, FKIN>), grid, block, lds, sc, p);
    else if (af64) hipLaunchKernelGGL((k_env_step<float, double, false, PART, FKIN>), grid, block, lds, sc, p);
    else hipLaunchKernelGGL((k_env_step<float, float, false, PART, FKIN>), grid, block, lds, sc, p);
}

// HOPE_DEFER_RS bookkeeping: `s` waits for the chains the last step left unjoined / the host does
int hope::join_rs(hope_env_t* h, hipStream_t s) {
    if (!h->rs_pending) return HOPE_OK;
    HIPCHK(hipStreamWaitEvent(s, h->ev_chain1_done, 0));
    HIPCHK(hipStreamWaitEvent(s, h->ev_search0_done, 0));
    h->rs_pending = false;
    return HOPE_OK;
}
int hope::settle_rs(hope_env_t* h) {
    if (!h->rs_pending) return HOPE_OK;
    DeviceGuard guard(h->device);
    HIPCHK(hipEventSynchronize(h->ev_chain1_done));
    HIPCHK(hipEventSynchronize(h->ev_search0_done));
    h->rs_pending = false;
    return HOPE_OK;
}

extern "C" {

const char* hope_last_error(void) { return g_err.c_str(); }
int hope_abi_version(void) { return HOPE_ABI_VERSION; }

static int destroy_impl(hope_env_t* h);
static void cur_free(hope_env_t* h);
int hope_env_create(hope_env_t** out, int n_scenes, int max_obstacles, int device_id, uint32_t flags) {
    if (!out || n_scenes <= 0 || max_obstacles <= 0) return fail(HOPE_EINVAL, "hope_env_create: bad argument");
    if (flags & 0x20)
        return fail(HOPE_EINVAL, "hope_env_create: flag 0x20 (hipGraph replay of the step, ABI <= 6) was removed in ABI 7: it was slower than plain launches at every batch size");
    *out = nullptr;
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0)
        return fail(HOPE_ENODEV, std::string("hope_env_create: no HIP device (") + hipGetErrorString(e) +
                                     "); libhope_env has no CPU fallback");
    if (device_id < 0 || device_id >= ndev) return fail(HOPE_EINVAL, "hope_env_create: device_id out of range");
    HIPCHK(hipSetDevice(device_id));
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device_id));
    size_t lds = step_lds_bytes(max_obstacles);
    size_t lds_rs = rs_lds_bytes(max_obstacles);
    if (max_obstacles > HOPE_MAX_OBSTACLES)
        return fail(HOPE_EINVAL, "hope_env_create: max_obstacles " + std::to_string(max_obstacles) + " exceeds HOPE_MAX_OBSTACLES (" +
                                 std::to_string(HOPE_MAX_OBSTACLES) + "): the Reeds-Shepp queue entry carries the obstacle count in 8 bits");
    if (lds > 160 * 1024 || lds_rs > 160 * 1024)
        return fail(HOPE_EINVAL, "hope_env_create: max_obstacles " + std::to_string(max_obstacles) + " does not fit the 160 KiB LDS tile of the step / search kernels");
    if (n_scenes >= RS_LIST_MAX_SCENES)
        return fail(HOPE_EINVAL, "hope_env_create: more than 2^24 - 1 scenes per handle");
    hope_env* h = new (std::nothrow) hope_env();
    if (!h) return fail(HOPE_ENOMEM, "hope_env_create: host allocation failed");
    h->n = n_scenes; h->max_obst = max_obstacles; h->device = device_id; h->flags = flags;
    h->n_obst_host.assign(n_scenes, 0);
    h->slot_cls_host.assign(n_scenes, 0);
    snprintf(h->arch, sizeof(h->arch), "%s", prop.gcnArchName);
    size_t N = (size_t)n_scenes;
#define ALLOC(ptr, bytes)                                                                          \
    do {                                                                                           \
        hipError_t e2 = hipMalloc((void**)&(ptr), (bytes));                                        \
        if (e2 != hipSuccess) {                                                                    \
            destroy_impl(h);                                                                       \
            return fail(HOPE_ENOMEM, std::string("hipMalloc " #ptr ": ") + hipGetErrorString(e2)); \
        }                                                                                          \
    } while (0)
    ALLOC(h->verts, N * max_obstacles * 8 * sizeof(double));
    ALLOC(h->obb, N * max_obstacles * sizeof(float4));
    ALLOC(h->fverts, N * max_obstacles * 2 * sizeof(float4));
    ALLOC(h->fbox, N * max_obstacles * sizeof(float4));
    ALLOC(h->eflag, N * (size_t)eflag_stride(max_obstacles));
    ALLOC(h->n_obst, N * sizeof(int32_t));
    ALLOC(h->scene_c, N * SC_WORDS * sizeof(double));
    ALLOC(h->state, N * ST_WORDS * sizeof(double));
    ALLOC(h->cs, N * 2 * sizeof(double));
    ALLOC(h->tstep, N * sizeof(int32_t));
    ALLOC(h->tab, (size_t)NL * NITER * NACT * sizeof(double));
    ALLOC(h->pmax, NL * sizeof(double));
    ALLOC(h->mask_lut, MASK_LUT_BYTES);
    ALLOC(h->mask_bsc, NBEAM * sizeof(double));
    ALLOC(h->hull_base, NBEAM * sizeof(double));
    ALLOC(h->beam_ab, 2 * NBEAM * sizeof(double));
    ALLOC(h->rs_count, 2 * hope_env::MAX_CHAIN * sizeof(int32_t));
    ALLOC(h->rs_list, 2 * N * sizeof(int32_t));
    ALLOC(h->rs_in, 2 * N * RS_IN_WORDS * sizeof(double));
    ALLOC(h->rs_flag, N);
    ALLOC(h->kin, N * KIN_WORDS * sizeof(double));
    ALLOC(h->post, N * POST_WORDS * sizeof(double));
    ALLOC(h->cls_list[0], N * sizeof(int32_t));
    ALLOC(h->cls_list[1], N * sizeof(int32_t));
    ALLOC(h->rs_rec, N * rs_rec_bytes_per_scene());
    ALLOC(h->rs_surv_count, hope_env::MAX_CHAIN * sizeof(int32_t));
    ALLOC(h->rs_surv, 2 * N * sizeof(int2));
    ALLOC(h->cur_pool, N * sizeof(int32_t));
    ALLOC(h->episode, N * sizeof(uint32_t));
    ALLOC(h->pool_overflow, sizeof(int32_t));
    ALLOC(h->slot_cls, N);
    ALLOC(h->active_snap, N);
    ALLOC(h->cold_dev, hope_env::COLD_RING * sizeof(StepCold));
    if (flags & HOPE_F_IMAGE) {
        ALLOC(h->traj, N * BEV_TRAJ_LEN * 3 * sizeof(double));
        ALLOC(h->traj_len, N * sizeof(int32_t));
        ALLOC(h->traj_valid, N * sizeof(int32_t));
        ALLOC(h->layer_valid, N * sizeof(int32_t));
        ALLOC(h->bev_layer, N * (size_t)BEV_LAYER_ROWS * BEV_LAYER_STRIDE);
        ALLOC(h->bev_dyn, N * BEV_DYN_BYTES);
        ALLOC(h->bev_list, (N + 1) * sizeof(int32_t));
        ALLOC(h->bev_legacy, (N + 1) * sizeof(int32_t));
        ALLOC(h->bev_scratch, N * BEV_SCENE_INTS * sizeof(int));
    }
#undef ALLOC
    if (h->traj) {
        HIPCHK(hipMemset(h->traj, 0, N * BEV_TRAJ_LEN * 3 * sizeof(double)));
        HIPCHK(hipMemset(h->traj_len, 0, N * sizeof(int32_t)));
        HIPCHK(hipMemset(h->traj_valid, 0, N * sizeof(int32_t)));
        HIPCHK(hipMemset(h->layer_valid, 0, N * sizeof(int32_t)));
        HIPCHK(hipMemset(h->bev_dyn, 0, N * BEV_DYN_BYTES));
        HIPCHK(hipMemset(h->bev_list, 0, (N + 1) * sizeof(int32_t)));
        HIPCHK(hipMemset(h->bev_legacy, 0, (N + 1) * sizeof(int32_t)));
        HIPCHK(hipMemset(h->bev_scratch, 0, N * BEV_SCENE_INTS * sizeof(int)));
    }
    HIPCHK(hipMemset(h->n_obst, 0, N * sizeof(int32_t)));
    HIPCHK(hipMemset(h->scene_c, 0, N * SC_WORDS * sizeof(double)));
    HIPCHK(hipMemset(h->state, 0, N * ST_WORDS * sizeof(double)));
    HIPCHK(hipMemset(h->tstep, 0, N * sizeof(int32_t)));
    HIPCHK(hipMemset(h->rs_count, 0, 2 * hope_env::MAX_CHAIN * sizeof(int32_t)));
    HIPCHK(hipMemset(h->rs_flag, 0, N));
    HIPCHK(hipMemset(h->rs_surv_count, 0, hope_env::MAX_CHAIN * sizeof(int32_t)));
    HIPCHK(hipMemset(h->rs_surv, 0, 2 * N * sizeof(int2)));
    HIPCHK(hipMemset(h->rs_in, 0, 2 * N * RS_IN_WORDS * sizeof(double)));
    HIPCHK(hipMemset(h->rs_list, 0, 2 * N * sizeof(int32_t)));      // (k_rs_words / k_rs_segs read queue entries before they know the queue length)
    HIPCHK(hipMemset(h->cur_pool, 0xFF, N * sizeof(int32_t)));
    HIPCHK(hipMemset(h->episode, 0, N * sizeof(uint32_t)));
    HIPCHK(hipMemset(h->pool_overflow, 0, sizeof(int32_t)));
    HIPCHK(hipMemset(h->slot_cls, 0, N));
    HIPCHK(hipMemset(h->active_snap, 1, N));
    HIPCHK(hipHostMalloc((void**)&h->cold_host, hope_env::COLD_RING * sizeof(StepCold)));
    for (int i = 0; i < hope_env::COLD_RING; i++) HIPCHK(hipEventCreateWithFlags(&h->cold_ev[i], hipEventDisableTiming));
    memset(&h->cold_last, 0, sizeof(h->cold_last));
    HIPCHK(rs_init_tables());        // (a synchronous symbol copy: here, never inside a captured step)
    if (lds > 48 * 1024) {
        for (const void* f : {(const void*)k_env_step<float, float>, (const void*)k_env_step<float, float, true>,
                              (const void*)k_env_step<float, double>, (const void*)k_env_step<double, float>,
                              (const void*)k_env_step<double, double>,
                              (const void*)k_env_step<float, float, false, 0, true>, (const void*)k_env_step<float, double, false, 0, true>,
                              (const void*)k_env_step<double, float, false, 0, true>, (const void*)k_env_step<double, double, false, 0, true>,
                              (const void*)k_env_step<float, float, false, 1>, (const void*)k_env_step<float, double, false, 1>,
                              (const void*)k_env_step<double, float, false, 1>, (const void*)k_env_step<double, double, false, 1>,
                              (const void*)k_env_step<float, float, false, 2>, (const void*)k_env_step<float, double, false, 2>,
                              (const void*)k_env_step<double, float, false, 2>, (const void*)k_env_step<double, double, false, 2>})
            HIPCHK(hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    }
    if (flags & HOPE_F_OVERLAP) {
        HIPCHK(hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&h->ev_collect, hipEventDisableTiming));
        for (int i = 0; i < 2; i++) HIPCHK(hipEventCreateWithFlags(&h->ev_bev[i], hipEventDisableTiming));
        for (int i = 0; i < 2; i++) { HIPCHK(hipEventCreateWithFlags(&h->ev_step[i], hipEventDisableTiming)); HIPCHK(hipEventCreateWithFlags(&h->ev_segs[i], hipEventDisableTiming)); HIPCHK(hipEventCreateWithFlags(&h->ev_post[i], hipEventDisableTiming)); }
        for (hipEvent_t* e : {&h->ev_chain1_done, &h->ev_image_done, &h->ev_obs_done[0], &h->ev_obs_done[1], &h->ev_search0_done})
            HIPCHK(hipEventCreateWithFlags(e, hipEventDisableTiming));
        // Which library stream plays which role decides which roles share a HARDWARE queue (the runtime spreads streams over a few
        // queues in creation order, and launches of streams that share one serialise).  perm[role] = the created stream (1 .. 7) that
        // plays it.  Default: the two observation launches on streams that do not share a hardware queue (3 and 7; with 3 and 4 the
        // larger class's observation started only when the smaller class's was done, 180 us after its motion launch): 0.695 -> 0.675 ms
        // (profiles/r04_stream_roles.txt).  Third session, final (pipelined) structure, profiles/r04_stream_roles_pipelined.txt: the
        // deferred forms use ROLE_CHAIN, ROLE_OBS_LARGE, ROLE_SEARCH0 (+ the caller's stream) and their assignment is in the best class;
        // ROLE_OBS_SMALL matters to the JOINED form, which wants it on the 2nd stream (65 536 scenes 0.672 -> 0.660 ms, 16 384: 0.343 ->
        // 0.305), and ROLE_OBS_SUB to the second sub-chain of a single-class batch, which wants the 7th stream (on the 2nd: 0.68 -> 0.89 ms).
        // A handle with the image (HOPE_F_IMAGE) has six streams at work in a step (the image on the caller's stream, two env, two search
        // streams, the layer rebuild): other roles have to share.  Measured over 40 random assignments under the final launch structure
        // (profiles/r04_stream_roles_pipelined.txt): 65 536 scenes 1.92 -> 1.85 ms, 8 192 scenes 0.527 -> 0.445 ms with the image; the
        // same assignment costs a step WITHOUT the image 15 % (0.60 -> 0.69 ms), hence by the handle's flag, not for everyone.
        // (Stream priorities by role were measured and rejected, DESIGN.md 9a: every stream has priority 0.)
        static const int perm_plain[N_ROLES] = {0, 1, 6, 3, 2, 5, 4, 7}, perm_image[N_ROLES] = {0, 6, 2, 3, 1, 4, 5, 7};
        int perm[N_ROLES];
        for (int r = 0; r < N_ROLES; r++) perm[r] = (flags & HOPE_F_IMAGE) ? perm_image[r] : perm_plain[r];
        hipStream_t created[N_ROLES] = {};
        for (int c = 1; c < N_ROLES; c++) HIPCHK(hipStreamCreateWithPriority(&created[c], hipStreamNonBlocking, 0));
        // ---- which created streams share a hardware queue: measure, then give the roles that are busy together different queues ----
        // cls[c]: queue class of the c-th created stream (c = 0: the NULL stream, where PyTorch's default current stream lives).
        // A stream is compared with one representative of every class seen so far: <= 4 classes x 7 streams pairs.
        int cls[N_ROLES];
        for (int c = 0; c < N_ROLES; c++) cls[c] = -1;
        {
            const auto t_begin = std::chrono::steady_clock::now();
            const long long ticks = 10000;                    // 100 us at 100 MHz
            // Two spin kernels, one per stream: they OVERLAP on the GPU's clock iff the streams sit on different hardware queues.  An overlap
            // is proof of two queues; its absence may be a late second launch (a loaded host), so a pair that did not overlap is tried up to
            // three times before it counts as one queue (the host's wall clock with fixed thresholds misread pairs on a busy box).
            long long* stamps = nullptr;                      // [2][2], host-visible
            if (hipHostMalloc((void**)&stamps, 4 * sizeof(long long), hipHostMallocDefault) != hipSuccess) stamps = nullptr;
            bool ok = stamps != nullptr;
            auto pair_overlaps = [&](hipStream_t a, hipStream_t b) -> int {   // 1 / 0, -1: the measurement is not to be trusted
                for (int rep_ = 0; rep_ < 3; rep_++) {
                    hipStreamSynchronize(a); hipStreamSynchronize(b);
                    hipLaunchKernelGGL(k_spin, dim3(1), dim3(64), 0, a, ticks, stamps);
                    hipLaunchKernelGGL(k_spin, dim3(1), dim3(64), 0, b, ticks, stamps + 2);
                    if (hipStreamSynchronize(a) != hipSuccess || hipStreamSynchronize(b) != hipSuccess) return -1;
                    const long long lo = std::max(stamps[0], stamps[2]), hi = std::min(stamps[1], stamps[3]);
                    if (hi - lo > ticks / 4) return 1;        // ran side by side for > 25 us
                    if (std::max(stamps[1], stamps[3]) - std::min(stamps[0], stamps[2]) > 20 * ticks) return -1;   // > 2 ms: the GPU is shared
                }
                return 0;
            };
            hipLaunchKernelGGL(k_spin, dim3(1), dim3(64), 0, created[1], 100LL, (long long*)nullptr);      // (first launch of the kernel: module load, not measured)
            hipStreamSynchronize(created[1]);
            int rep[N_ROLES], n_cls = 0;
            for (int c = 0; c < N_ROLES && ok; c++) {
                int found = -1;
                for (int k = 0; k < n_cls && found < 0 && ok; k++) {
                    const int ov = pair_overlaps(created[rep[k]], created[c]);
                    if (ov < 0) ok = false;                   // something else is using the GPU: do not trust any of it
                    else if (ov == 0) found = k;              // serialised: the same hardware queue
                }
                if (found < 0) { rep[n_cls] = c; found = n_cls++; }
                cls[c] = found;
            }
            if (stamps) hipHostFree(stamps);
            HIPCHK(hipGetLastError());
            h->queue_check_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
            if (!ok) { for (int c = 0; c < N_ROLES; c++) cls[c] = -1; n_cls = 0; }
            h->n_queues = n_cls;
            // Assignment.  Roles busy at the same time: deferred step {caller, SEARCH0, CHAIN, OBS_LARGE}; joined step {caller, CHAIN,
            // OBS_LARGE, OBS_SMALL}; two sub-chains of one class {SEARCH0, CHAIN, OBS_LARGE, OBS_SUB}.  Greedy in that order of importance:
            // every role takes the free stream whose class collides with the fewest roles it must not share with; ties keep the hand-found
            // table (so a box that shows nothing to gain gets exactly round 4's assignment).  Not for image handles (six busy streams on
            // four queues: the measured table stays).
            if (n_cls >= 2 && !(flags & HOPE_F_IMAGE)) {
                static const int order[N_ROLES - 1] = {ROLE_SEARCH0, ROLE_CHAIN, ROLE_OBS_LARGE, ROLE_OBS_SMALL, ROLE_OBS_SUB, ROLE_IMAGE, ROLE_SPARE};
                static const int conflicts[N_ROLES][4] = {
                    /* ROLE_CALLER    */ {-1, -1, -1, -1},
                    /* ROLE_CHAIN     */ {ROLE_CALLER, ROLE_SEARCH0, -1, -1},
                    /* ROLE_IMAGE     */ {-1, -1, -1, -1},
                    /* ROLE_OBS_LARGE */ {ROLE_CALLER, ROLE_SEARCH0, ROLE_CHAIN, -1},
                    /* ROLE_OBS_SMALL */ {ROLE_CALLER, ROLE_CHAIN, ROLE_OBS_LARGE, -1},
                    /* ROLE_SEARCH0   */ {ROLE_CALLER, -1, -1, -1},
                    /* ROLE_SPARE     */ {-1, -1, -1, -1},
                    /* ROLE_OBS_SUB   */ {ROLE_SEARCH0, ROLE_CHAIN, ROLE_OBS_LARGE, -1}};
                int newperm[N_ROLES] = {0, 0, 0, 0, 0, 0, 0, 0};
                bool taken[N_ROLES] = {};
                for (const int r : order) {
                    int best = -1, best_cost = 1 << 30;
                    for (int c = 1; c < N_ROLES; c++) {
                        if (taken[c]) continue;
                        int cost = 0;
                        for (const int o : conflicts[r]) {
                            if (o < 0) continue;
                            const int oc = o == ROLE_CALLER ? cls[0] : (newperm[o] ? cls[newperm[o]] : -2);
                            if (oc == cls[c]) cost += 4;
                        }
                        if (c != perm[r]) cost += 1;          // prefer the table's stream among equals
                        if (cost < best_cost) { best_cost = cost; best = c; }
                    }
                    newperm[r] = best; taken[best] = true;
                }
                for (int r = 1; r < N_ROLES; r++) perm[r] = newperm[r];
            }
        }
        for (int r = 1; r < N_ROLES; r++) h->side[r] = created[perm[r]];
        h->queue_of_role[ROLE_CALLER] = cls[0];
        for (int r = 1; r < N_ROLES; r++) h->queue_of_role[r] = cls[perm[r]];
    }
    HIPCHK(hipDeviceSynchronize());
    { std::lock_guard<std::mutex> lk(g_live_m); g_live.insert(h); }
    *out = h;
    return HOPE_OK;
}

int hope_env_destroy(hope_env_t* h) {
    if (!h) return HOPE_OK;
    {
        std::lock_guard<std::mutex> lk(g_live_m);
        if (g_live.erase(h) == 0) return fail(HOPE_EINVAL, HOPE_NOT_LIVE("hope_env_destroy", "destroyed twice?"));
    }
    return destroy_impl(h);
}
static int destroy_impl(hope_env_t* h) {                   // (also the clean-up of a hope_env_create that failed half-way: not registered yet)
    settle_rs(h);
    DeviceGuard guard(h->device);
    drain_events(h);
    hipDeviceSynchronize();
    for (hipEvent_t e : {h->ev_collect, h->ev_bev[0], h->ev_bev[1], h->ev_fork, h->ev_step[0], h->ev_step[1], h->ev_segs[0], h->ev_segs[1], h->ev_post[0], h->ev_post[1],
                         h->ev_chain1_done, h->ev_image_done, h->ev_obs_done[0], h->ev_obs_done[1], h->ev_search0_done}) if (e) hipEventDestroy(e);
    for (hipStream_t q : h->side) if (q) hipStreamDestroy(q);
    if (h->pool_stream) hipStreamDestroy(h->pool_stream);
    for (hipEvent_t e : h->cold_ev) if (e) hipEventDestroy(e);
    if (h->cold_host) hipHostFree(h->cold_host);
    for (hipEvent_t e : {h->ev_pool_ready, h->ev_pool_copied, h->ev_last_step}) if (e) hipEventDestroy(e);
    for (void* q : {(void*)h->pstage.start, (void*)h->pstage.dest, (void*)h->pstage.bbox, (void*)h->pstage.verts, (void*)h->pstage.nobst, (void*)h->pstage.list}) if (q) hipHostFree(q);
    for (int i = 0; i < 2; i++) { if (h->gen_nobst[i]) hipHostFree(h->gen_nobst[i]); if (h->ev_gen_copied[i]) hipEventDestroy(h->ev_gen_copied[i]); }
    for (hipEvent_t e : h->free_events) hipEventDestroy(e);
    cur_free(h);
    plan_free(h);
    choose_free(h);
    onorm_free(h);
    evalt_free(h);
    gae_free(h);
    ring_free(h);
    ppo_free(h);
    sac_free(h);
    policy_free(h);
    imgenc_free(h);
    critics_free(h);
    for (auto& ps : h->pset) for (void* q : {(void*)ps.label, (void*)ps.sorted_own[0], (void*)ps.sorted_own[1]}) if (q) hipFree(q);
    void* ptrs[] = {h->obb, h->fverts, h->fbox, h->eflag, h->verts, h->n_obst, h->scene_c, h->state, h->cs, h->tstep, h->tab, h->pmax, h->mask_lut, h->mask_bsc,
                    h->hull_base, h->beam_ab, h->rs_count, h->rs_surv_count, h->rs_surv, h->rs_list, h->rs_in, h->rs_flag, h->kin, h->post, h->cls_list[0], h->cls_list[1], h->rs_rec, h->cur_pool, h->episode, h->pset[0].verts, h->pset[0].c, h->pset[0].nobst, h->pset[0].list[0], h->pset[0].list[1], h->pset[1].verts, h->pset[1].c, h->pset[1].nobst, h->pset[1].list[0], h->pset[1].list[1], h->pstage_dev, h->pool_overflow, h->slot_cls, h->active_snap, h->cold_dev, h->dlp_mem[0], h->dlp_mem[1], h->dlp_mem[2], h->dlp_mem[3], h->dlp_mem[4], h->dlp_mem[5], h->stage, h->traj, h->traj_len, h->traj_valid, h->layer_valid, h->bev_layer, h->bev_dyn, h->bev_list, h->bev_legacy, h->bev_scratch};
    for (void* q : ptrs)
        if (q) hipFree(q);
    delete h;
    return HOPE_OK;
}

int hope_debug_step_prof(uint64_t* out, int reset) {
    static unsigned long long buf[64 * 16];
    hipError_t e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpyFromSymbol(buf, HIP_SYMBOL(g_step_prof), sizeof(buf));
    for (int i = 0; i < 16; i++) { out[i] = 0; for (int sh = 0; sh < 64; sh++) out[i] += buf[sh * 16 + i]; }
    if (e == hipSuccess && reset) {
        for (auto& v : buf) v = 0;
        e = hipMemcpyToSymbol(HIP_SYMBOL(g_step_prof), buf, sizeof(buf));
    }
    return e == hipSuccess ? HOPE_OK : fail(HOPE_EHIP, std::string("hope_debug_step_prof: ") + hipGetErrorString(e));
}

int hope_debug_census(uint64_t* out, int reset) {
    // [1] [3] [7] are minima (bit patterns of non-negative doubles), the rest are counts; 64 shards
    static unsigned long long buf[64 * 16];
    if (!out) return fail(HOPE_EINVAL, "hope_debug_census: null argument");
    hipError_t e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpyFromSymbol(buf, HIP_SYMBOL(g_census), sizeof(buf));
    for (int i = 0; i < 16; i++) {
        const bool is_min = i == 1 || i == 3 || i == 7;
        out[i] = is_min ? ~0ull : 0;
        for (int sh = 0; sh < 64; sh++) out[i] = is_min ? std::min<uint64_t>(out[i], buf[sh * 16 + i]) : out[i] + buf[sh * 16 + i];
    }
    if (e == hipSuccess && reset) {
        for (int sh = 0; sh < 64; sh++) for (int i = 0; i < 16; i++) buf[sh * 16 + i] = (i == 1 || i == 3 || i == 7) ? 0x7ff0000000000000ull : 0;
        e = hipMemcpyToSymbol(HIP_SYMBOL(g_census), buf, sizeof(buf));
    }
    return e == hipSuccess ? HOPE_OK : fail(HOPE_EHIP, std::string("hope_debug_census: ") + hipGetErrorString(e));
}

int hope_debug_rs_prof(uint64_t* out, int reset) {
    hipError_t e = rs_prof_read((unsigned long long*)out, reset);
    return e == hipSuccess ? HOPE_OK : fail(HOPE_EHIP, std::string("hope_debug_rs_prof: ") + hipGetErrorString(e));
}

int hope_debug_rs_filter_stats(uint64_t* out, int reset) {
    if (!out) return fail(HOPE_EINVAL, "hope_debug_rs_filter_stats: null argument");
    hipError_t e = rs_fstat_read((unsigned long long*)out, reset);
    return e == hipSuccess ? HOPE_OK : fail(HOPE_EHIP, std::string("hope_debug_rs_filter_stats: ") + hipGetErrorString(e));
}

int hope_debug_rs_filter_dump(double* out) {
    if (!out) return fail(HOPE_EINVAL, "hope_debug_rs_filter_dump: null argument");
    hipError_t e = rs_fdump_read(out);
    return e == hipSuccess ? HOPE_OK : fail(HOPE_EHIP, std::string("hope_debug_rs_filter_dump: ") + hipGetErrorString(e));
}

int hope_debug_rs_log(int32_t* out, int cap, int32_t* n, int reset) {
    if (!out || !n || cap < 0) return fail(HOPE_EINVAL, "hope_debug_rs_log: bad argument");
    hipError_t e = rs_log_read(out, cap, n, reset);
    return e == hipSuccess ? HOPE_OK : fail(HOPE_EHIP, std::string("hope_debug_rs_log: ") + hipGetErrorString(e));
}

int hope_env_queue_check(hope_env_t* h, int32_t* queue_of_role, int32_t* n_queues, double* ms) {
    HOPE_ENTER(h, "hope_env_queue_check");
    if (queue_of_role) for (int r = 0; r < N_ROLES; r++) queue_of_role[r] = h->queue_of_role[r];
    if (n_queues) *n_queues = h->n_queues;
    if (ms) *ms = h->queue_check_ms;
    return HOPE_OK;
}

// the getters keep their return conventions (HOPE_EINVAL / ""); a pointer that is neither NULL nor a handle hope_env_create returned also leaves the message
#define NOT_LIVE(h, name) ((h) ? fail(HOPE_EINVAL, HOPE_NOT_LIVE(name, "destroyed?")) : HOPE_EINVAL)
int hope_env_num_scenes(const hope_env_t* h) { return is_live(h) ? h->n : NOT_LIVE(h, "hope_env_num_scenes"); }
int hope_env_max_obstacles(const hope_env_t* h) { return is_live(h) ? h->max_obst : NOT_LIVE(h, "hope_env_max_obstacles"); }
const char* hope_env_device_arch(const hope_env_t* h) { return is_live(h) ? h->arch : (NOT_LIVE(h, "hope_env_device_arch"), ""); }

// Count-interval table of the action mask's coarse beams (round 6; read by k_obs_pair's mask stage).  The scan value x of coarse beam i
// falls into bin b = floor((x - lo_i) scale_i), lo_i = hull_base_i - 1e-6 (x >= hull_base_i always); the MASK_LUT_NB bins reach to the
// table's maximum at that beam + 4e-9.  Per (i, b, action): cnt_lo <= #{k : tab <= x - 1e-9} and #{k : tab <= x} <= cnt_hi for EVERY x
// whose computed bin is b -- the bin's edges are widened by 1e-6 of a bin (the device evaluates b in float64: its rounding is ~1e-13 of
// a bin) and by 2e-9 m (the tie band of the coarse decision is 1e-9 m).  cnt_lo == cnt_hi: the count is known and no table entry lies
// within 1e-9 of x; otherwise the kernel looks at the float64 entries cnt_lo .. cnt_hi - 1 themselves.  tab: [NL][NITER][NACT] prefix-maxed.
//
// The kernels index the table with (int)((x - lo_i) scale_i) once that is below MASK_LUT_NB, so a table whose scale is not a finite positive
// number would send them out of bounds: tables with a value that is not finite, or with a coarse beam whose maximum does not lie above
// lo_i, are refused (HOPE_EINVAL, `err` names the beam) before anything is built from them.  dist_star: the caller's [NL][NACT][NITER].
static int build_mask_lut(const double* dist_star, const std::vector<double>& tab, const std::vector<double>& pmax, const double* hull_base,
                          std::vector<uint16_t>& lut, std::vector<double>& bsc, std::string& err) {
    // a count takes four bits of a table word (0 .. NITER), and the pair kernel keeps a table row next to its beam in 16 bits
    static_assert(NITER <= 15 && NBEAM * MASK_LUT_NB < 65536, "the mask table's packing: 4-bit counts, 16-bit row numbers");
    for (int i = 0; i < NBEAM; i++)
        if (!std::isfinite(hull_base[i])) { err = "hull_base is not finite at beam " + std::to_string(i); return HOPE_EINVAL; }
    for (int l = 0; l < NL; l++)
        for (int e = 0; e < NACT * NITER; e++)
            if (!std::isfinite(dist_star[(size_t)l * NACT * NITER + e])) {
                err = "dist_star is not finite at beam " + std::to_string(l / UPS) + " (row " + std::to_string(l) + ", action " +
                      std::to_string(e / NITER) + ")";
                return HOPE_EINVAL;
            }
    for (int i = 0; i < NBEAM; i++) {
        const double lo = hull_base[i] - 1e-6;
        const double scale = (double)MASK_LUT_NB / (pmax[UPS * i] + 4e-9 - lo);
        if (!(pmax[UPS * i] > lo) || !std::isfinite(scale) || !(scale > 0.0)) {
            err = "dist_star's maximum at beam " + std::to_string(i) + " does not lie above hull_base - 1e-6: the beam's bins have no extent";
            return HOPE_EINVAL;
        }
    }
    lut.assign((size_t)MASK_LUT_ROWS * MASK_LUT_ROW, (uint16_t)0xAAAA);       // padding lanes and the neutral last row: [10, 10]
    bsc.assign(NBEAM, 0.0);
    for (int i = 0; i < NBEAM; i++) {
        const int l = UPS * i;
        const double lo = hull_base[i] - 1e-6;
        const double scale = (double)MASK_LUT_NB / (pmax[l] + 4e-9 - lo);
        bsc[i] = scale;
        for (int b = 0; b < MASK_LUT_NB; b++) {
            const double e_lo = lo + ((double)b - 1e-6) / scale - 2e-9, e_hi = lo + ((double)b + 1.0 + 1e-6) / scale + 2e-9;
            uint16_t* row = lut.data() + ((size_t)i * MASK_LUT_NB + b) * MASK_LUT_ROW;
            for (int hl = 0; hl < NACT / 2; hl++) {
                int c[2][2];
                for (int d = 0; d < 2; d++) {
                    const int a = hl + d * (NACT / 2);
                    int cl = 0, ch = 0;
                    for (int k = 0; k < NITER; k++) {
                        const double t = tab[((size_t)l * NITER + k) * NACT + a];
                        cl += t <= e_lo; ch += t <= e_hi;
                    }
                    c[d][0] = cl; c[d][1] = ch;
                }
                row[hl] = (uint16_t)(c[0][0] | c[0][1] << 4 | c[1][0] << 8 | c[1][1] << 12);
            }
        }
    }
    return HOPE_OK;
}

// device layout of the mask table: prefix-max over k (first exceedance of a sequence == first exceedance of its running max: exact),
// transposed to [l][k][a] so that lane = action reads coalesced rows; pmax[l] = the maximum over (a, k)
static void build_mask_tab(const double* dist_star, std::vector<double>& tab, std::vector<double>& pmax) {
    tab.assign((size_t)NL * NITER * NACT, 0.0);
    pmax.assign(NL, 0.0);
    for (int l = 0; l < NL; l++) {
        double pm = -INFINITY;
        for (int a = 0; a < NACT; a++) {
            double run = -INFINITY;
            for (int k = 0; k < NITER; k++) {
                double v = dist_star[((size_t)l * NACT + a) * NITER + k];
                run = v > run ? v : run;
                tab[((size_t)l * NITER + k) * NACT + a] = run;
            }
            pm = run > pm ? run : pm;
        }
        pmax[l] = pm;
    }
}

int hope_debug_mask_lut(const double* dist_star, const double* hull_base, uint16_t* lut_out, double* scale_out) {
    if (!dist_star || !hull_base || !lut_out || !scale_out) return fail(HOPE_EINVAL, "hope_debug_mask_lut: null argument");
    std::vector<double> tab, pmax, bsc;
    std::vector<uint16_t> lut;
    std::string err;
    build_mask_tab(dist_star, tab, pmax);
    if (build_mask_lut(dist_star, tab, pmax, hull_base, lut, bsc, err) != HOPE_OK) return fail(HOPE_EINVAL, "hope_debug_mask_lut: " + err);
    memcpy(lut_out, lut.data(), MASK_LUT_BYTES);
    memcpy(scale_out, bsc.data(), NBEAM * sizeof(double));
    return HOPE_OK;
}

int hope_env_upload_tables(hope_env_t* h, const double* dist_star, const double* hull_base, const double* beam_ab) {
    HOPE_ENTER_AS(h, "hope_env_upload_tables", "null argument");
    if (!dist_star || !hull_base || !beam_ab) return fail(HOPE_EINVAL, "hope_env_upload_tables: null argument");
    HOPE_ON_DEVICE(h);
    // everything is derived, and the tables are validated, before the first copy: a refused call leaves the handle's tables as they were
    std::vector<double> tab, pmax, bsc;
    std::vector<uint16_t> lut;
    std::string err;
    build_mask_tab(dist_star, tab, pmax);
    if (build_mask_lut(dist_star, tab, pmax, hull_base, lut, bsc, err) != HOPE_OK) return fail(HOPE_EINVAL, "hope_env_upload_tables: " + err);
    HIPCHK(hipMemcpy(h->tab, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->pmax, pmax.data(), pmax.size() * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->mask_lut, lut.data(), MASK_LUT_BYTES, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->mask_bsc, bsc.data(), NBEAM * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->hull_base, hull_base, NBEAM * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->beam_ab, beam_ab, 2 * NBEAM * sizeof(double), hipMemcpyHostToDevice));
    h->have_tables = true;
    return HOPE_OK;
}

static int upload_scenes(hope_env_t* h, const int32_t* ids, int n, const double* start, const double* dest, const double* bbox,
                         const double* verts, const int32_t* n_obst, double* d_scene_c, double* d_state, int32_t* d_t,
                         int32_t* d_nobst, double* d_verts, float4* d_obb, double* d_traj, int32_t* d_traj_len, int32_t* d_traj_valid,
                         int32_t* d_layer_valid);
static int apply_pending_pool(hope_env_t* h, bool wait);
static int cur_on_swap(hope_env_t* h);

// The dense per-class scene lists of the launch chains and the per-slot class byte (host mirror; reset-time only).  A slot's class
// decides which launch chain steps it (LDS tile of 32 or max_obstacles obstacles) AND which pool entries it draws at episode
// turnover: by default the size class of the map hope_env_set_scenes gave it, or what hope_env_set_draw_class says.
static int rebuild_class_lists(hope_env_t* h) {
    std::vector<int32_t> l0, l1;
    l0.reserve(h->n); l1.reserve(h->n);
    const bool two = h->max_obst > SMALL_TILE;
    for (int i = 0; i < h->n; i++) (two && h->slot_cls_host[i] ? l1 : l0).push_back(i);
    // Two launch chains run concurrently (HOPE_F_OVERLAP): the step ends with the longer one running alone.  A scene with
    // few obstacles may run in the large-tile launches too (it only gets more LDS than it needs), so the small-tile class
    // hands scenes over until the large-tile chain holds `frac` of all scenes (HOPE_CLS1_FRAC, default below).  (The handed-over
    // slots keep their class byte: they go on drawing small lots.)
    if (two && (h->flags & HOPE_F_OVERLAP)) {
        const char* fr = getenv("HOPE_CLS1_FRAC");
        // measured (mixed scene set, 25 % large-tile scenes by themselves): 0.42 gives +1 / +4 / +4 % at 4 096 / 8 192 / 16 384
        // scenes, 0 at 32 768, -3 % at 65 536 (the moved scenes lose occupancy there and nothing is left to hide)
        const double frac = fr ? atof(fr) : (h->n < 32768 ? 0.42 : 0.0);
        const size_t want1 = (size_t)(frac * h->n);
        if (l1.size() < want1) {
            const size_t move = std::min(l0.size(), want1 - l1.size());
            l1.insert(l1.end(), l0.end() - move, l0.end());
            l0.resize(l0.size() - move);
            std::sort(l1.begin(), l1.end());
        }
    }
    h->cls_count[0] = (int)l0.size(); h->cls_count[1] = (int)l1.size();
    h->cls_list_host[0] = l0; h->cls_list_host[1] = l1;     // (host mirror: hope_env_step_plan)
    if (!l0.empty()) HIPCHK(hipMemcpy(h->cls_list[0], l0.data(), l0.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    if (!l1.empty()) HIPCHK(hipMemcpy(h->cls_list[1], l1.data(), l1.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->slot_cls, h->slot_cls_host.data(), (size_t)h->n, hipMemcpyHostToDevice));
    return HOPE_OK;
}

int hope_env_set_scenes(hope_env_t* h, const int32_t* scene_ids, int n, const double* start, const double* dest,
                        const double* bbox, const double* verts, const int32_t* n_obst) {
    HOPE_ENTER_AS(h, "hope_env_set_scenes", "null argument");
    { int rcs = settle_rs(h); if (rcs != HOPE_OK) return rcs; }
    if (n < 0 || (n > 0 && (!scene_ids || !start || !dest || !bbox || !n_obst))) return fail(HOPE_EINVAL, "hope_env_set_scenes: null argument");
    if (n == 0) return HOPE_OK;
    for (int k = 0; k < n; k++) {
        if (scene_ids[k] < 0 || scene_ids[k] >= h->n) return fail(HOPE_EINVAL, "hope_env_set_scenes: scene id out of range");
        if (n_obst[k] < 0 || n_obst[k] > h->max_obst) return fail(HOPE_EINVAL, "hope_env_set_scenes: n_obst exceeds max_obstacles");
        if (n_obst[k] > 0 && !verts) return fail(HOPE_EINVAL, "hope_env_set_scenes: verts is null");
    }
    HOPE_ON_DEVICE(h);
    {
        int rc = upload_scenes(h, scene_ids, n, start, dest, bbox, verts, n_obst, h->scene_c, h->state, h->tstep, h->n_obst,
                               h->verts, h->obb, h->traj, h->traj_len, h->traj_valid, h->layer_valid);
        if (rc != HOPE_OK) return rc;
    }
    for (int k = 0; k < n; k++) {
        h->n_obst_host[scene_ids[k]] = n_obst[k];
        h->slot_cls_host[scene_ids[k]] = (h->max_obst > SMALL_TILE && n_obst[k] > SMALL_TILE) ? 1 : 0;
    }
    { int rc = rebuild_class_lists(h); if (rc != HOPE_OK) return rc; }
    if (h->cur.on) {                                        // the curriculum: an uploaded map is unlabelled (ids: head of the staging)
        hipLaunchKernelGGL(k_curriculum_forget, dim3((n + 255) / 256), dim3(256), 0, 0, n, (const int32_t*)h->stage, h->cur.scene_bucket,
                           h->episode, h->cur.noted_ep);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipDeviceSynchronize());
    h->have_scenes = true;
    return HOPE_OK;
}

// The rarely used parameters of the step kernel (StepCold) live in device memory: when their content differs from the version
// uploaded last, the next ring slot is filled and copied on the caller's stream -- ahead of every launch of the step, whose chains
// fork from that stream.  A slot is immutable while launches may read it: it comes round again after COLD_RING changes, and its
// event (the copy that last filled it) is waited for before the pinned source is rewritten.
// the lists a draw indexes: the uniform base lists of the active pool set, or the curriculum's weighted lists of the same entries
static void draw_lists(const hope_env_t* h, const int32_t** lists, int* counts) {
    for (int c = 0; c < 2; c++) {
        const bool weighted = h->cur.on && h->cur.wactive >= 0 && h->pool_cls_n[c] > 0;
        lists[c] = weighted ? h->cur.wl[h->cur.wactive][c] : h->pool_cls[c];
        counts[c] = weighted ? CW_LIST_LEN : h->pool_cls_n[c];
    }
}
static int sync_cold(hope_env_t* h, hipStream_t s) {
    StepCold c;
    memset(&c, 0, sizeof(c));
    c.traj = h->traj; c.traj_len = h->traj_len; c.traj_valid = h->traj_valid; c.layer_valid = h->layer_valid;
    c.pool_verts = h->pool_verts; c.pool_c = h->pool_c; c.pool_nobst = h->pool_nobst;
    draw_lists(h, c.pool_cls, c.pool_cls_n);
    c.cur_pool = h->cur_pool; c.episode = h->episode; c.redraw_seed = h->redraw_seed;
    c.dlp = h->dlp; c.pool_overflow = h->pool_overflow; c.slot_cls = h->slot_cls;
    c.fverts = h->fverts; c.fbox = h->fbox; c.eflag = h->eflag;
    if (h->cold_idx >= 0 && memcmp(&c, &h->cold_last, sizeof(c)) == 0) return HOPE_OK;
    const int slot = (h->cold_idx + 1) % hope_env::COLD_RING;
    HIPCHK(hipEventSynchronize(h->cold_ev[slot]));
    memcpy(&h->cold_host[slot], &c, sizeof(c));
    HIPCHK(hipMemcpyAsync(h->cold_dev + slot, h->cold_host + slot, sizeof(c), hipMemcpyHostToDevice, s));
    HIPCHK(hipEventRecord(h->cold_ev[slot], s));
    h->cold_idx = slot;
    memcpy(&h->cold_last, &c, sizeof(c));
    return HOPE_OK;
}

// ---- the step's launch plan ----
// One chain of launches per tile class (scenes with few obstacles get a small LDS tile and therefore more resident waves):
// [k_kinematics ->] k_env_step -> k_post, and with the search k_rs_compact -> k_rs_words -> k_rs_segs -> k_rs_validate.  The chains
// share nothing but read-only data (own scene list, own queue counter, record slots filled from opposite ends), so with HOPE_F_OVERLAP
// they run concurrently from the fork to the join: every class kernel is latency-bound per wave, and at <= 16 k scenes per GPU one
// class alone cannot fill the 1024 SIMDs.  The form of the step is decided by these measured thresholds (steady ms per step):
//
// Two-launch step kernel (the motion launch, then the observation half on its own stream next to the search of the same class): from
// 16 384 scenes (+4.5 % at 65 536 scenes, +3.7 % at 131 072, 0 at 16 384, -3 % at 8 192 and below: two more launches per class) ...
constexpr int SPLIT_MIN_SCENES = 16384;
// ... and from 32 768 scenes with pipelined steps (HOPE_DEFER_RS), where the one-launch form stays the faster one: 16 384 scenes
// 0.249 vs 0.266 ms.  HOPE_SPLIT_MIN overrides both (read per call: the tests force the split at small sizes).
constexpr int SPLIT_MIN_SCENES_DEFER = 32768;
// One-launch form with the kinematics fused in (the step kernel's waves compute their scene's sub-step poses themselves): the step
// is a chain of launch latencies there, and the kinematics launch cost the critical stream ~16 us plus a launch gap.  Only where the
// GPU is far from full: the wave-per-scene form spends ~2x the vector instructions of k_kinematics' four lanes per scene (fused /
// separate: 4 096 scenes 0.152 / 0.156, 8 192 0.186 / 0.176, 16 384 0.249 / 0.222).
constexpr int FUSE_KIN_MAX_SCENES = 4096;
// A batch whose scenes all sit in ONE tile class has one chain: no second stream, and none of the two-chain forms (observation half
// on its own stream, pipelined steps).  Pipelined steps cut that class's list into two sub-chains where that was measured to pay
// (profiles/r04_single_class_chains.txt; same bits: the chains share nothing): the small-tile class from 32 768 scenes (65 536
// generated lots 0.790 -> 0.680 ms; below that the single chain in the one-launch form is the faster one), the large-tile class from
// 4 096 to 32 768 scenes (4 096 Dragon-Lake scenes 0.190 -> 0.155 ms, 16 384: 0.278 -> 0.232; 65 536: 0.698 vs 0.717, not there).
// {lo, hi} of the small-tile class, then of the large-tile class; HOPE_AUTO_CHAINS=lo0:hi0:lo1:hi1 moves them (read per call: tests).
constexpr int AUTO_SUBS_RANGE[4] = {32768, 1 << 30, 4096, 32768};

enum MotionKernel { MOTION_ONE_LAUNCH, MOTION_FUSED_KIN, MOTION_TIMING, MOTION_SPLIT, MOTION_PAIR };
enum ObsKernel { OBS_IN_STEP, OBS_SPLIT, OBS_PAIR };     // OBS_IN_STEP: the one-launch step kernel computes the observation
static_assert(MOTION_ONE_LAUNCH == HOPE_STEPPLAN_MOTION_ONE_LAUNCH && MOTION_FUSED_KIN == HOPE_STEPPLAN_MOTION_FUSED_KIN &&
              MOTION_TIMING == HOPE_STEPPLAN_MOTION_TIMING && MOTION_SPLIT == HOPE_STEPPLAN_MOTION_SPLIT && MOTION_PAIR == HOPE_STEPPLAN_MOTION_PAIR &&
              OBS_IN_STEP == HOPE_STEPPLAN_OBS_IN_STEP && OBS_SPLIT == HOPE_STEPPLAN_OBS_SPLIT && OBS_PAIR == HOPE_STEPPLAN_OBS_PAIR,
              "hope_env_step_plan reports these numbers (include/hope_env.h)");

struct StepPlan {
    struct Chain {
        int c, a, b;              // tile class and the range [a, b) of its scene list
        int tile_cap;             // LDS tile capacity of the class's launches
        Role search, kin, obs;    // streams of the search launches, of the kinematics + motion launch, of the observation + k_post
        bool on_caller;           // pipelined: this chain's env launches are on the caller's stream itself
        bool post_on_search;      // k_post heads the search stream instead of following the observation launch
        MotionKernel motion;
        ObsKernel obs_kernel;
    } chain[hope_env::MAX_CHAIN];
    int n_chain;
    bool want_rs;
    bool fork;                    // two chains on their own streams: HOPE_F_OVERLAP and n_chain == 2
    bool split;                   // two-launch step kernel
    bool pipe;                    // pipelined (deferred) step: the search streams stay unjoined (HOPE_DEFER_RS)
    bool pipe1;                   // pipelined with the one-launch step kernel
    bool fuse_kin;                // one-launch step kernel with the kinematics fused in
    bool auto_subs;               // two sub-chains of one tile class
};

// cycle accounting build (tools/step_timing.py); read once per process
static bool step_timing_build() {
    static const bool on = getenv("HOPE_STEP_TIMING") != nullptr;
    return on;
}

// What one step enqueues (no HIP calls).
static StepPlan plan_step(const hope_env_t* h, uint32_t stages, bool want_rs, bool overlap, int has_action, bool step_timing) {
    StepPlan pl = {};
    pl.want_rs = want_rs;
    const int n_cls = h->max_obst > SMALL_TILE ? 2 : 1;
    const bool obs = stages & HOPE_STAGE_OBS, defer_rs = stages & HOPE_DEFER_RS, img = stages & HOPE_STAGE_IMG;
    int subs = 1;
    if (overlap && want_rs && obs && defer_rs && !img && (h->cls_count[0] == 0) != (h->cls_count[1] == 0)) {
        int range[4] = {AUTO_SUBS_RANGE[0], AUTO_SUBS_RANGE[1], AUTO_SUBS_RANGE[2], AUTO_SUBS_RANGE[3]};
        if (const char* e = getenv("HOPE_AUTO_CHAINS")) sscanf(e, "%d:%d:%d:%d", range, range + 1, range + 2, range + 3);
        const int c1 = h->cls_count[0] == 0 ? 1 : 0, cnt = h->cls_count[c1];
        if (cnt >= range[2 * c1] && cnt <= range[2 * c1 + 1]) { subs = 2; pl.auto_subs = true; }
    }
    // chains with work, the large-tile class first (its chain is the longer one); two sub-chains only when the other class is empty
    for (int c = n_cls - 1; c >= 0; c--)
        for (int j = 0; j < subs; j++) {
            const int a = (int)((long long)h->cls_count[c] * j / subs), b = (int)((long long)h->cls_count[c] * (j + 1) / subs);
            if (b > a) {
                StepPlan::Chain& ch = pl.chain[pl.n_chain++];
                ch.c = c; ch.a = a; ch.b = b;
                ch.tile_cap = (c == 0 && n_cls == 2) ? SMALL_TILE : h->max_obst;
            }
        }
    pl.fork = overlap && pl.n_chain == 2;
    const bool two_stream_forms = pl.fork && want_rs && obs && !step_timing;
    const char* split_min = getenv("HOPE_SPLIT_MIN");
    pl.split = two_stream_forms && h->n >= (split_min ? atoi(split_min) : defer_rs ? SPLIT_MIN_SCENES_DEFER : SPLIT_MIN_SCENES);
    pl.pipe = two_stream_forms && defer_rs;
    pl.pipe1 = pl.pipe && !pl.split;
    pl.fuse_kin = h->n <= FUSE_KIN_MAX_SCENES && !pl.split && !step_timing;
    const bool of64 = h->flags & HOPE_F_OBS_F64, af64 = h->flags & HOPE_F_ACTION_F64;
    for (int i = 0; i < pl.n_chain; i++) {
        StepPlan::Chain& ch = pl.chain[i];
        // joined: the first chain on the caller's stream, the second on ROLE_CHAIN; pipelined: the search launches on ROLE_SEARCH0 /
        // ROLE_CHAIN, so that step k + 1's kinematics and motion launch do not queue behind step k's validation kernel
        ch.search = (pl.fork && i == 1) ? ROLE_CHAIN : pl.pipe ? ROLE_SEARCH0 : ROLE_CALLER;
        // pipelined: the env launches of the class with MORE scenes are on the caller's stream itself -- its kernels are the step's
        // critical cycle (kinematics -> motion -> observation -> the caller's next actions -> kinematics ...), and every hop between a
        // library stream and the caller's costs that cycle 20-30 us (two hops per step: 0.648 -> 0.60 ms).  Not with the image, which
        // runs on the caller's stream next to the observation launches; not for two sub-chains of one class (both would land on the
        // caller's stream and serialise: 0.80 vs 0.68 ms).  (With exactly equal class counts both chains take the caller's stream.)
        ch.on_caller = pl.pipe && !pl.auto_subs && !img && h->cls_count[ch.c] >= h->cls_count[1 - ch.c];
        ch.obs = !(pl.split || pl.pipe1) ? ch.search : ch.on_caller ? ROLE_CALLER : (pl.auto_subs && i == 1) ? ROLE_OBS_SUB : (Role)(ROLE_OBS_LARGE + i);
        ch.kin = pl.pipe ? ch.obs : ch.search;
        // pipelined two-launch form: k_post, whose outputs the caller's stream joins too, runs at the head of the search stream
        // instead of behind the observation launch (the search stream has slack, the env stream is the critical one).  In the
        // one-launch form k_post stays behind the step kernel (8 192 scenes 0.205 vs 0.188 ms: the search chain is the longer one)
        ch.post_on_search = pl.pipe && pl.split;
        // small-tile class, moving step: two scenes per wave (hope_motion_pair.h, hope_obs_pair.h; STAGE_ONE_SCENE: the one-scene kernels)
        const bool one_scene = stages & STAGE_ONE_SCENE;
        if (pl.split) ch.motion = (ch.c == 0 && n_cls == 2 && (stages & HOPE_STAGE_MOTION) && has_action && !one_scene) ? MOTION_PAIR : MOTION_SPLIT;
        else if (step_timing && !of64 && !af64) ch.motion = MOTION_TIMING;
        else ch.motion = pl.fuse_kin ? MOTION_FUSED_KIN : MOTION_ONE_LAUNCH;
        ch.obs_kernel = !pl.split ? OBS_IN_STEP : (ch.tile_cap == SMALL_TILE && !one_scene) ? OBS_PAIR : OBS_SPLIT;
    }
    return pl;
}

// Enqueues the launches of one step (plan_step) on the caller's stream `s` and the handle's role streams.
static int enqueue_step(hope_env_t* h, const void* actions, const uint8_t* active, uint32_t stages, const hope_step_out* out,
                        hipStream_t s, bool overlap, int has_action, LaunchTimer* tm) {
    StepParams p;
    memset(&p, 0, sizeof(p));
    p.n = h->n; p.max_obst = h->max_obst; p.stages = stages; p.has_action = has_action;
    p.hflags = h->traj ? STEP_HF_TRAJ : 0;
    p.verts = h->verts; p.obb = h->obb; p.eflag = h->eflag; p.n_obst = h->n_obst; p.scene_c = h->scene_c; p.state = h->state; p.cs = h->cs; p.tstep = h->tstep;
    p.active = active; p.active_out = active ? h->active_snap : nullptr; p.kin = h->kin; p.actions = actions; p.post = h->post;
    p.tab = h->tab; p.pmax = h->pmax; p.mask_lut = h->mask_lut; p.mask_bsc = h->mask_bsc; p.hull_base = h->hull_base; p.beam_ab = h->beam_ab;
    p.lidar = out->lidar; p.action_mask = out->action_mask;
    p.cold = h->cold_dev + h->cold_idx;                     // (sync_cold ran on the caller's stream before any launch of this step)
    const uint8_t* active_rs = active ? h->active_snap : nullptr;   // what the Reeds-Shepp chain reads instead of the caller's mask
    const bool of64 = h->flags & HOPE_F_OBS_F64, af64 = h->flags & HOPE_F_ACTION_F64;
    const dim3 block(WAVE);
    const bool step_timing = step_timing_build();
    const bool want_rs = (stages & HOPE_STAGE_RS) && out->rs_word;
    const StepPlan pl = plan_step(h, stages, want_rs, overlap, has_action, step_timing);
    auto stream = [&](Role r) { return r == ROLE_CALLER ? s : h->side[r]; };

    if (!pl.pipe) { int rcj = join_rs(h, s); if (rcj != HOPE_OK) return rcj; }    // (a deferred step's launches follow the unjoined ones on the same streams)
    // PIPELINED steps (HOPE_DEFER_RS): each chain runs on TWO streams --
    //   env stream   : k_kinematics -> k_env_step<motion> -> k_env_step<observation> -> k_post     (what the caller's stream joins)
    //   search stream: [motion done] k_rs_compact -> k_rs_words -> k_rs_segs -> k_rs_validate      (hope_env_wait_rs / never)
    // so that step k + 1's kinematics and motion launch only wait for step k's k_rs_compact (the last reader of `state` / `post` on the
    // search stream) and -- through the caller's stream -- for its observation.  The search of step k may then read obstacle tiles
    // that step k + 1's episode turnover is rewriting: only for scenes whose episode ended in step k + 1, whose search result nobody
    // can read any more (k_rs_compact of step k + 1 clears it, after the validation kernel, on the same stream), and all reads stay
    // inside the scene's own tile slots.  The queue counter alternates between two words per chain (the motion launch of step k + 1
    // zeroes the one step k + 1 uses while step k's validation blocks are still reading theirs).
    if (want_rs) h->rs_parity ^= 1;
    if (pl.fork) {
        HIPCHK(hipEventRecord(h->ev_fork, s));
        HIPCHK(hipStreamWaitEvent(h->side[ROLE_CHAIN], h->ev_fork, 0));
        if (pl.pipe) HIPCHK(hipStreamWaitEvent(h->side[ROLE_SEARCH0], h->ev_fork, 0));
    }
    // every chain's motion launch is followed by its ev_step record: those two events cover the pool's readers (the pool upload waits
    // for them instead of a per-step record on the caller's stream)
    h->last_via_steps = false;
    for (int i = 0; i < pl.n_chain; i++) {
        const StepPlan::Chain& ch = pl.chain[i];
        const int c = ch.c;
        const hipStream_t sc = stream(ch.search), sk = stream(ch.kin), so = stream(ch.obs);
        int32_t* counter = h->rs_count + i + hope_env::MAX_CHAIN * h->rs_parity;
        if (pl.pipe && !ch.on_caller) HIPCHK(hipStreamWaitEvent(sk, h->ev_fork, 0));
        p.tile_cap = ch.tile_cap;
        p.scene_list = h->cls_list[c] + ch.a;
        p.n_list = ch.b - ch.a;
        p.rs_count_zero = want_rs ? counter : nullptr;
        if ((stages & HOPE_STAGE_MOTION) && has_action && !pl.fuse_kin) {       // this chain's sub-step poses head it
            dim3 kg((p.n_list + KIN_SCENES_PER_BLOCK - 1) / KIN_SCENES_PER_BLOCK);
            if (tm) tm->begin(HOPE_K_KINEMATICS, sk);
            if (af64) hipLaunchKernelGGL((k_kinematics<double>), kg, block, 0, sk, p.n_list, p.scene_list, h->state, actions, active, stages, h->scene_c, h->kin);
            else hipLaunchKernelGGL((k_kinematics<float>), kg, block, 0, sk, p.n_list, p.scene_list, h->state, actions, active, stages, h->scene_c, h->kin);
            if (tm) tm->end(sk);
        }
        const dim3 grid(p.n_list);
        const size_t lds = step_lds_bytes(p.tile_cap);
        // pipelined: the last step's k_rs_compact (search stream) reads `post` and `state`, which the motion launch rewrites
        if (pl.pipe) HIPCHK(hipStreamWaitEvent(sk, h->ev_segs[i], 0));
        if (tm) tm->begin(HOPE_K_STEP, sk);
        switch (ch.motion) {
        case MOTION_PAIR: hipLaunchKernelGGL(k_motion_pair, dim3((p.n_list + 1) / 2), block, MP_LDS_BYTES, sk, p); break;
        case MOTION_SPLIT: launch_env_step<1>(of64, af64, grid, block, lds, sk, p); break;
        case MOTION_TIMING: hipLaunchKernelGGL((k_env_step<float, float, true>), grid, block, lds, sk, p); break;
        case MOTION_FUSED_KIN: launch_env_step<0, true>(of64, af64, grid, block, lds, sk, p); break;
        case MOTION_ONE_LAUNCH: launch_env_step<0>(of64, af64, grid, block, lds, sk, p); break;
        }
        if (tm) tm->end(sk);
        if (pl.fork && (pl.split || pl.pipe || (stages & HOPE_STAGE_IMG))) { HIPCHK(hipEventRecord(h->ev_step[i], sk)); h->last_via_steps = true; }   // poses final
        if (pl.split && !pl.pipe) HIPCHK(hipStreamWaitEvent(so, h->ev_step[i], 0));
        auto launch_post = [&](hipStream_t sp) {                // scalar outputs, reward / target arithmetic: one lane per scene
            dim3 pg((p.n_list + WAVE - 1) / WAVE);
            if (tm) tm->begin(HOPE_K_POST, sp);
            if (of64) hipLaunchKernelGGL((k_post<double>), pg, block, 0, sp, p.n_list, p.scene_list, active, stages, h->scene_c, h->state, h->post, h->rs_flag, *out);
            else hipLaunchKernelGGL((k_post<float>), pg, block, 0, sp, p.n_list, p.scene_list, active, stages, h->scene_c, h->state, h->post, h->rs_flag, *out);
            if (tm) tm->end(sp);
        };
        if (!pl.split) launch_post(so);
        else {
            if (tm) tm->begin(HOPE_K_STEP, so);
            if (ch.obs_kernel == OBS_PAIR) {
                if (of64) hipLaunchKernelGGL((k_obs_pair<double>), dim3((p.n_list + 1) / 2), block, OP_LDS_BYTES, so, p);
                else hipLaunchKernelGGL((k_obs_pair<float>), dim3((p.n_list + 1) / 2), block, OP_LDS_BYTES, so, p);
            } else launch_env_step<2>(of64, af64, grid, block, lds, so, p);
            if (tm) tm->end(so);
            // k_post BEHIND the observation half on that stream: nothing waits for its outputs before the join, the observation is
            // the long launch (0.675 -> 0.669 ms)
            if (!ch.post_on_search) launch_post(so);
        }
        if ((pl.split || pl.pipe1) && !ch.on_caller) HIPCHK(hipEventRecord(h->ev_obs_done[i], so));
        if (!want_rs) continue;
        if (pl.pipe) HIPCHK(hipStreamWaitEvent(sc, h->ev_step[i], 0));  // the search stream starts behind this step's motion launch
        if (ch.post_on_search) {
            launch_post(sc);
            HIPCHK(hipEventRecord(h->ev_post[i], sc));
        }
        int32_t* qlist = h->rs_list + (size_t)c * h->n + ch.a;       // this chain's part of the class's queue storage
        double* rs_in = h->rs_in + ((size_t)c * h->n + ch.a) * RS_IN_WORDS;      // ... and of the search inputs, same index
        if (tm) tm->begin(HOPE_K_RS_COMPACT, sc);
        {
            const dim3 cg((p.n_list + COMPACT_THREADS - 1) / COMPACT_THREADS);
            if (of64) hipLaunchKernelGGL(k_rs_compact<double>, cg, dim3(COMPACT_THREADS), 0, sc, p.scene_list, p.n_list, h->rs_flag, active_rs, qlist,
                                         counter, (const double*)h->post, (const double*)h->scene_c, out->rs_word, out->rs_lengths, (const int32_t*)h->n_obst, h->rs_surv_count + i, rs_in);
            else hipLaunchKernelGGL(k_rs_compact<float>, cg, dim3(COMPACT_THREADS), 0, sc, p.scene_list, p.n_list, h->rs_flag, active_rs, qlist,
                                    counter, (const double*)h->post, (const double*)h->scene_c, out->rs_word, out->rs_lengths, (const int32_t*)h->n_obst, h->rs_surv_count + i, rs_in);
        }
        if (tm) tm->end(sc);
        // pipelined steps: the next step's motion launch rewrites `state` / `post` (and, on an episode turnover, the scene constants),
        // which k_post and k_rs_compact are the last to read -- k_rs_words / k_rs_segs work from k_rs_compact's rows (RS_IN_WORDS)
        if (pl.pipe) HIPCHK(hipEventRecord(h->ev_segs[i], sc));
        RsParams r;
        r.n = h->n; r.max_obst = h->max_obst; r.obs_f64 = of64;
        r.prio_front = 0;
        r.tile_cap = p.tile_cap;
        r.max_queue = p.n_list;
        r.slot_base = (c == 0) ? ch.a : h->n - 1 - ch.a;    // the two classes fill the record storage from both ends
        r.slot_dir = (c == 0) ? 1 : -1;
        r.verts = h->verts; r.obb = h->obb; r.n_obst = h->n_obst; r.scene_c = h->scene_c; r.state = h->state;
        r.fverts = h->fverts; r.fbox = h->fbox; r.eflag = h->eflag;
        r.rs_count = counter; r.rs_list = qlist; r.rs_in = rs_in;
        r.rs_rec = h->rs_rec;
        r.surv_count = h->rs_surv_count + i;
        r.surv_list = h->rs_surv + (size_t)c * h->n + ch.a;
        r.rs_word = out->rs_word; r.rs_lengths = out->rs_lengths;
        HIPCHK(launch_rs_search(r, sc, tm));
    }
    HIPCHK(hipGetLastError());
    if (stages & HOPE_STAGE_IMG) {
        BevParams b;
        b.n = h->n; b.max_obst = h->max_obst; b.verts = h->verts; b.n_obst = h->n_obst; b.scene_c = h->scene_c;
        b.state = h->state; b.traj = h->traj; b.traj_len = h->traj_len; b.traj_valid = h->traj_valid; b.scratch = h->bev_scratch; b.img = out->img;
        b.layer = h->bev_layer; b.layer_valid = h->layer_valid; b.rebuild = h->bev_list; b.dyn = h->bev_dyn;
        b.legacy_list = h->bev_legacy;
        // with auto-reset every scene shows its NEW episode's first observation, like lidar / action_mask / target
        b.active = active;
        b.debug = 0;
        if (const char* e_ = getenv("HOPE_BEV_DEBUG")) b.debug |= atoi(e_);   // (profiling switches, hope_bev.hip: 16 no block cache, 64 no image stores, ...)
        if (getenv("HOPE_BEV_LEGACY")) b.debug |= 32;          // (tests) the per-tile raster of the moving boxes instead of the trajectory layer
        if (pl.fork) {
            // the image depends on the step kernels only (pose, trajectory ring), not on the Reeds-Shepp search: render it on
            // ROLE_IMAGE while the two chains run k_rs_words / k_rs_validate.  Pipelined steps: both chains run on library streams and
            // the caller's stream is idle during the step: the image, which the caller waits for anyway, goes there, and the static-layer
            // rebuild goes to ROLE_IMAGE
            const hipStream_t si = pl.pipe ? s : h->side[ROLE_IMAGE];
            HIPCHK(hipStreamWaitEvent(si, h->ev_step[0], 0));
            HIPCHK(hipStreamWaitEvent(si, h->ev_step[1], 0));
            if (pl.pipe) HIPCHK(launch_bev_image(b, si, tm, h->side[ROLE_IMAGE], h->ev_bev[0], h->ev_bev[1]));
            else HIPCHK(launch_bev_image(b, si, tm));
            HIPCHK(hipEventRecord(h->ev_image_done, si));
        } else HIPCHK(launch_bev_image(b, s, tm));           // (no fork: every launch of the step is on the caller's stream)
    }
    if (!pl.fork) return HOPE_OK;
    HIPCHK(hipEventRecord(h->ev_chain1_done, h->side[ROLE_CHAIN]));
    if (pl.pipe) {                                          // the search streams stay unjoined: hope_env_wait_rs / the next step
        HIPCHK(hipEventRecord(h->ev_search0_done, h->side[ROLE_SEARCH0]));
        h->rs_pending = true;
    } else HIPCHK(hipStreamWaitEvent(s, h->ev_chain1_done, 0));
    if (stages & HOPE_STAGE_IMG) HIPCHK(hipStreamWaitEvent(s, h->ev_image_done, 0));
    if (pl.split || pl.pipe1) {
        // Round 6: every event the caller's stream waits for or records is a packet in ITS queue, in front of the next step's
        // kinematics -- the head of the step's critical cycle: three waits + two records made a 50 us hole behind the observation
        // launch (profiles/r05_step_timeline_pipelined.txt).  With one chain on the caller's stream the OTHER chain's observation
        // stream -- it has slack -- waits for the two k_post launches and records ONE event for the caller.
        const StepPlan::Chain* ch = pl.chain;
        if (ch[0].on_caller != ch[1].on_caller) {
            const hipStream_t so = stream(ch[ch[0].on_caller ? 1 : 0].obs);
            for (int i = 0; i < 2; i++) if (ch[i].post_on_search) HIPCHK(hipStreamWaitEvent(so, h->ev_post[i], 0));
            HIPCHK(hipEventRecord(h->ev_collect, so));
            HIPCHK(hipStreamWaitEvent(s, h->ev_collect, 0));
        } else for (int i = 0; i < 2; i++) {
            if (!ch[i].on_caller) HIPCHK(hipStreamWaitEvent(s, h->ev_obs_done[i], 0));
            if (ch[i].post_on_search) HIPCHK(hipStreamWaitEvent(s, h->ev_post[i], 0));
        }
    }
    return HOPE_OK;
}

// A scene draws its next map from the pool entries of ITS tile class (the dense per-class launch lists are fixed between
// hope_env_set_scenes calls).  A resident class without entries would silently keep its maps: refuse instead.
static int check_pool_classes(hope_env_t* h, const char* who) {
    bool resident[2] = {false, false};
    for (int i = 0; i < h->n; i++) resident[h->slot_cls_host[i] ? 1 : 0] = true;
    for (int c = 0; c < 2; c++)
        if (resident[c] && h->pool_cls_n[c] == 0)
            return fail(HOPE_ESTATE, std::string(who) + ": scene slots of the " + (c ? "large" : "small (<= 32 obstacles)") +
                                     " size class are resident but the pool holds no map of that size class (a slot draws from its own class: "
                                     "hope_env_set_pool / hope_env_set_dlp_cases / hope_env_set_draw_class)");
    return HOPE_OK;
}

static int launch_step(hope_env_t* h, const void* actions, const uint8_t* active, uint32_t stages,
                       const hope_step_out* out, void* stream, int has_action) {
    if (!out) return fail(HOPE_EINVAL, "hope_env_step: null argument");
    if (!h->have_tables) return fail(HOPE_ESTATE, "hope_env_step: hope_env_upload_tables has not been called");
    if (!h->have_scenes) return fail(HOPE_ESTATE, "hope_env_step: hope_env_set_scenes has not been called");
    if (has_action && !actions) return fail(HOPE_EINVAL, "hope_env_step: actions is null");
    if (stages & HOPE_STAGE_RS) stages |= HOPE_STAGE_REWARD;       // the RS gate needs the status
    if (stages & HOPE_AUTO_REDRAW) {
        if (!(stages & HOPE_AUTO_RESET)) return fail(HOPE_EINVAL, "hope_env_step: HOPE_AUTO_REDRAW needs HOPE_AUTO_RESET");
        if (h->pool_n <= 0 && h->dlp.n_cases <= 0) return fail(HOPE_ESTATE, "hope_env_step: HOPE_AUTO_REDRAW without a scene pool (hope_env_set_pool / hope_env_set_dlp_cases)");
        int rc0 = check_pool_classes(h, "hope_env_step");
        if (rc0 != HOPE_OK) return rc0;
    }
    if (stages & HOPE_STAGE_IMG) {
        if (!h->traj) return fail(HOPE_ESTATE, "hope_env_step: HOPE_STAGE_IMG needs a handle created with HOPE_F_IMAGE");
        if (!out->img) return fail(HOPE_EINVAL, "hope_env_step: HOPE_STAGE_IMG without out->img");
    }
    HOPE_ON_DEVICE(h);
    hipStream_t s = (hipStream_t)stream;
    const bool prof = h->flags & HOPE_F_PROFILE;
    h->step_seq++;
    { int rcp = apply_pending_pool(h, false); if (rcp != HOPE_OK) return rcp; }    // a relaxed commit whose upload has finished takes over here
    if (h->pool_wait_pending) {                             // a pool committed since the last launch: its upload orders before this step
        HIPCHK(hipStreamWaitEvent(s, h->ev_pool_ready, 0));
        h->pool_wait_pending = false;
    }
    { int rcc = sync_cold(h, s); if (rcc != HOPE_OK) return rcc; }
    h->draw_set = h->pactive;
    struct LastStep {                                       // (the next pool upload must not overwrite a set this step still reads)
        hope_env_t* h; hipStream_t s;
        ~LastStep() { if (h->pactive >= 0 && h->ev_last_step && !h->last_via_steps) hipEventRecord(h->ev_last_step, s); }
    } last_step{h, s};
    if (prof && h->pending.size() > 4096) { int rc = drain_events(h); if (rc) return rc; }
    EventTimer timer(h);
    LaunchTimer* tm = prof ? &timer : nullptr;
    int rc = enqueue_step(h, actions, active, stages, out, s, (h->flags & HOPE_F_OVERLAP) != 0, has_action, tm);
    if (rc != HOPE_OK) return rc;
    if (timer.failed) return fail(HOPE_EHIP, "hipEventRecord failed");
    return HOPE_OK;
}


// Shared by set_scenes and set_pool: stage the host arrays and write constants / tiles for entries ids[0..n)
static int upload_scenes(hope_env_t* h, const int32_t* ids, int n, const double* start, const double* dest, const double* bbox,
                         const double* verts, const int32_t* n_obst, double* d_scene_c, double* d_state, int32_t* d_t,
                         int32_t* d_nobst, double* d_verts, float4* d_obb, double* d_traj, int32_t* d_traj_len, int32_t* d_traj_valid,
                         int32_t* d_layer_valid) {
    size_t tile = (size_t)h->max_obst * 8 * sizeof(double);
    size_t o_ids = 0, o_nob = o_ids + sizeof(int32_t) * n, o_start = (o_nob + sizeof(int32_t) * n + 15) & ~(size_t)15;
    size_t o_dest = o_start + 24 * (size_t)n, o_bbox = o_dest + 24 * (size_t)n, o_verts = (o_bbox + 32 * (size_t)n + 15) & ~(size_t)15;
    size_t need = o_verts + tile * n;
    if (need > h->stage_bytes) {
        if (h->stage) hipFree(h->stage);
        h->stage = nullptr; h->stage_bytes = 0;
        hipError_t e2 = hipMalloc(&h->stage, need);
        if (e2 != hipSuccess) return fail(HOPE_ENOMEM, std::string("hipMalloc stage: ") + hipGetErrorString(e2));
        h->stage_bytes = need;
    }
    char* sp = (char*)h->stage;
    HIPCHK(hipMemcpy(sp + o_ids, ids, sizeof(int32_t) * n, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(sp + o_nob, n_obst, sizeof(int32_t) * n, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(sp + o_start, start, 24 * (size_t)n, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(sp + o_dest, dest, 24 * (size_t)n, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(sp + o_bbox, bbox, 32 * (size_t)n, hipMemcpyHostToDevice));
    if (verts) HIPCHK(hipMemcpy(sp + o_verts, verts, tile * n, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_set_scene_consts, dim3((n + 127) / 128), dim3(128), 0, 0, n, (const int32_t*)(sp + o_ids),
                       (const double*)(sp + o_start), (const double*)(sp + o_dest), (const double*)(sp + o_bbox),
                       (const int32_t*)(sp + o_nob), d_scene_c, d_state, d_t, d_nobst, d_traj, d_traj_len, d_traj_valid, d_layer_valid);
    if (verts)
        hipLaunchKernelGGL(k_set_scene_tiles, dim3(n), dim3(128), 0, 0, (const int32_t*)(sp + o_ids),
                           (const int32_t*)(sp + o_nob), (const double*)(sp + o_verts), (const double*)(sp + o_bbox), d_verts, d_obb,
                           h->fverts, h->fbox, h->eflag, h->max_obst);
    HIPCHK(hipGetLastError());
    HIPCHK(hipDeviceSynchronize());
    return HOPE_OK;
}

// ---- scene pool: pinned staging -> asynchronous upload into the set the kernels are not reading -> swap by stream order ----
// pool identity (hope_env_pool_generation): a hash chain over what was uploaded, so that equal histories give equal values across
// processes and different pools differ (a counter said "1" for any first pool)
static uint64_t hmix64(uint64_t z) {                        // splitmix64 finaliser (host twin of hope_dev.h's mix64)
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static uint64_t fold64(uint64_t a, uint64_t b) { return hmix64(a ^ hmix64(b + 0x9E3779B97F4A7C15ull)); }
// (one multiply per 8 bytes: hope_env_commit_pool hashes ~0.8 MB on the thread that enqueues the steps -- ~0.1 ms per commit; the
// splitmix chain above cost 0.7 ms, more than a 65 536-scene step)
static uint64_t hash_bytes(uint64_t hsh, const void* p, size_t bytes) {
    const unsigned char* q = (const unsigned char*)p;
    size_t i = 0;
    for (; i + 8 <= bytes; i += 8) { uint64_t w; memcpy(&w, q + i, 8); hsh = (hsh ^ w) * 0x100000001B3ull; hsh ^= hsh >> 29; }
    uint64_t w = 0;
    if (i < bytes) { memcpy(&w, q + i, bytes - i); hsh = (hsh ^ w) * 0x100000001B3ull; }
    return fold64(hsh, bytes);
}
static void bump_pool_generation(hope_env_t* h, uint64_t content) {
    h->pool_generation = fold64(h->pool_generation, content);
    if (h->pool_generation == 0) h->pool_generation = 1;   // 0 is reserved: "no pool" / "skip the check"
}

static int pool_init_streams(hope_env_t* h) {
    if (h->pool_stream) return HOPE_OK;
    HIPCHK(hipStreamCreateWithFlags(&h->pool_stream, hipStreamNonBlocking));
    HIPCHK(hipEventCreateWithFlags(&h->ev_pool_ready, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&h->ev_pool_copied, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&h->ev_last_step, hipEventDisableTiming));
    return HOPE_OK;
}

// draw lists of the two size classes into pinned staging: complete pool scenes by their obstacle count, and -- in the large class
// -- the device-drawn Dragon-Lake cases as -2 - case (-1 is "the map hope_env_set_scenes uploaded")
static void build_pool_lists(hope_env_t* h, const int32_t* n_obst, int n_pool, std::vector<int32_t>& l0, std::vector<int32_t>& l1) {
    const bool two = h->max_obst > SMALL_TILE;
    for (int k = 0; k < n_pool; k++) (two && n_obst[k] > SMALL_TILE ? l1 : l0).push_back(k);
    for (int c = 0; c < h->dlp.n_cases; c++) (two ? l1 : l0).push_back(-2 - c);
}

static int pool_set_reserve(hope_env_t* h, hope_env::PoolSet& ps, int n_pool, int n_list) {
    if (n_pool > ps.cap) {
        for (void* q : {(void*)ps.verts, (void*)ps.c, (void*)ps.nobst, (void*)ps.label}) if (q) hipFree(q);
        ps.verts = ps.c = nullptr; ps.nobst = nullptr; ps.label = nullptr; ps.cap = 0;
        const size_t P = (size_t)n_pool;
        hipError_t e_ = hipMalloc((void**)&ps.verts, P * h->max_obst * 8 * sizeof(double));
        if (e_ == hipSuccess) e_ = hipMalloc((void**)&ps.c, P * SC_WORDS * sizeof(double));
        if (e_ == hipSuccess) e_ = hipMalloc((void**)&ps.nobst, P * sizeof(int32_t));
        if (e_ == hipSuccess) e_ = hipMalloc((void**)&ps.label, P);
        if (e_ != hipSuccess) return fail(HOPE_ENOMEM, std::string("hipMalloc pool: ") + hipGetErrorString(e_));
        ps.cap = n_pool;
    }
    if (n_list > ps.list_cap) {
        for (int c = 0; c < 2; c++) { if (ps.list[c]) hipFree(ps.list[c]); ps.list[c] = nullptr; }
        for (int c = 0; c < 2; c++) {
            hipError_t e_ = hipMalloc((void**)&ps.list[c], (size_t)n_list * sizeof(int32_t));
            if (e_ != hipSuccess) return fail(HOPE_ENOMEM, std::string("hipMalloc pool lists: ") + hipGetErrorString(e_));
        }
        ps.list_cap = n_list;
    }
    return HOPE_OK;
}

int hope_env_pool_staging(hope_env_t* h, int n_pool, double** start, double** dest, double** bbox, double** verts, int32_t** n_obst) {
    HOPE_ENTER_AS(h, "hope_env_pool_staging", "bad argument");
    if (n_pool <= 0 || !start || !dest || !bbox || !verts || !n_obst) return fail(HOPE_EINVAL, "hope_env_pool_staging: bad argument");
    HOPE_ON_DEVICE(h);
    int rc = pool_init_streams(h);
    if (rc != HOPE_OK) return rc;
    if (h->pstage.busy) { HIPCHK(hipEventSynchronize(h->ev_pool_copied)); h->pstage.busy = false; }   // the previous upload still reads it
    if (n_pool > h->pstage.cap) {
        for (void* q : {(void*)h->pstage.start, (void*)h->pstage.dest, (void*)h->pstage.bbox, (void*)h->pstage.verts, (void*)h->pstage.nobst, (void*)h->pstage.list})
            if (q) hipHostFree(q);
        h->pstage = hope_env::PoolStage{};
        const size_t P = (size_t)n_pool;
        hipError_t e_ = hipHostMalloc((void**)&h->pstage.start, P * 24);
        if (e_ == hipSuccess) e_ = hipHostMalloc((void**)&h->pstage.dest, P * 24);
        if (e_ == hipSuccess) e_ = hipHostMalloc((void**)&h->pstage.bbox, P * 32);
        if (e_ == hipSuccess) e_ = hipHostMalloc((void**)&h->pstage.verts, P * h->max_obst * 8 * sizeof(double));
        if (e_ == hipSuccess) e_ = hipHostMalloc((void**)&h->pstage.nobst, P * sizeof(int32_t));
        if (e_ == hipSuccess) e_ = hipHostMalloc((void**)&h->pstage.list, (P + 4096) * sizeof(int32_t));
        if (e_ != hipSuccess) return fail(HOPE_ENOMEM, std::string("hipHostMalloc pool staging: ") + hipGetErrorString(e_));
        h->pstage.cap = n_pool;
    }
    h->pstage.staged = true;
    *start = h->pstage.start; *dest = h->pstage.dest; *bbox = h->pstage.bbox; *verts = h->pstage.verts; *n_obst = h->pstage.nobst;
    return HOPE_OK;
}

int hope_env_pool_staging_ready(hope_env_t* h) {
    HOPE_ENTER(h, "hope_env_pool_staging_ready");
    if (!h->pstage.busy) return 1;
    HOPE_ON_DEVICE(h);
    const hipError_t e = hipEventQuery(h->ev_pool_copied);
    if (e == hipSuccess) { h->pstage.busy = false; return 1; }
    if (e == hipErrorNotReady) return 0;
    return fail(HOPE_EHIP, std::string("hipEventQuery: ") + hipGetErrorString(e));
}

static int effective_generation(hope_env_t* h, uint64_t* generation);
int hope_env_pool_generation(hope_env_t* h, uint64_t* generation) {
    HOPE_ENTER_AS(h, "hope_env_pool_generation", "null argument");
    if (!generation) return fail(HOPE_EINVAL, "hope_env_pool_generation: null argument");
    { DeviceGuard guard(h->device); int rcp = apply_pending_pool(h, true); if (rcp != HOPE_OK) return rcp; }
    return effective_generation(h, generation);
}

// the host copy of a generated pool's obstacle counts (hope_env_generate_pool), once its kernel and copy have finished
static int settle_gen_nobst(hope_env_t* h) {
    const int g = h->gen_host_set;
    if (g < 0) return HOPE_OK;
    HIPCHK(hipEventSynchronize(h->ev_gen_copied[g]));
    h->pool_nobst_host.assign(h->gen_nobst[g], h->gen_nobst[g] + h->gen_nobst_n[g]);
    h->gen_host_set = -1;
    return HOPE_OK;
}

// the swap of hope_env_commit_pool_relaxed, once its upload is complete (wait: block until it is)
static int apply_pending_pool(hope_env_t* h, bool wait) {
    if (!h->pend.on) return HOPE_OK;
    if (wait) HIPCHK(hipEventSynchronize(h->ev_pool_ready));
    else {
        const hipError_t e = hipEventQuery(h->ev_pool_ready);
        if (e == hipErrorNotReady) return HOPE_OK;
        if (e != hipSuccess) return fail(HOPE_EHIP, std::string("hipEventQuery: ") + hipGetErrorString(e));
    }
    hope_env::PoolSet& ps = h->pset[h->pend.set];
    h->pool_verts = ps.verts; h->pool_c = ps.c; h->pool_nobst = ps.nobst;
    h->pool_cls[0] = ps.list[0]; h->pool_cls[1] = ps.list[1];
    h->pool_cls_n[0] = h->pend.cls_n[0]; h->pool_cls_n[1] = h->pend.cls_n[1];
    h->pool_n = h->pend.n_pool;
    h->pool_nobst_host.swap(h->pend.nobst_host);
    h->pactive = h->pend.set;
    h->pend.on = false;
    bump_pool_generation(h, h->pend.content);
    h->gen_host_set = h->pend.generated ? h->pend.set : -1; // (a generated pool: its counts are fetched when somebody asks)
    return cur_on_swap(h);
}

static int commit_pool_impl(hope_env_t* h, int n_pool, bool relaxed);
int hope_env_commit_pool(hope_env_t* h, int n_pool, void* stream) {
    (void)stream;
    HOPE_ENTER_AS(h, "hope_env_commit_pool", "bad argument");
    return commit_pool_impl(h, n_pool, false);
}
int hope_env_commit_pool_relaxed(hope_env_t* h, int n_pool) {
    HOPE_ENTER_AS(h, "hope_env_commit_pool_relaxed", "bad argument");
    return commit_pool_impl(h, n_pool, true);
}

static int commit_pool_impl(hope_env_t* h, int n_pool, bool relaxed) {
    // (no join of an unjoined Reeds-Shepp chain here: only the motion launches read the pool, and ev_last_step covers them)
    if (n_pool <= 0) return fail(HOPE_EINVAL, "hope_env_commit_pool: bad argument");
    if (n_pool > h->pstage.cap) return fail(HOPE_ESTATE, "hope_env_commit_pool: more entries than hope_env_pool_staging provided");
    for (int k = 0; k < n_pool; k++)
        if (h->pstage.nobst[k] < 0 || h->pstage.nobst[k] > h->max_obst) return fail(HOPE_EINVAL, "hope_env_commit_pool: n_obst exceeds max_obstacles");
    HOPE_ON_DEVICE(h);
    std::vector<int32_t> l0, l1;
    build_pool_lists(h, h->pstage.nobst, n_pool, l0, l1);
    if ((int)(l0.size() + l1.size()) > h->pstage.cap + 4096) return fail(HOPE_EINVAL, "hope_env_commit_pool: too many Dragon-Lake cases for the list staging");
    { int rcp = apply_pending_pool(h, true); if (rcp != HOPE_OK) return rcp; }     // (a relaxed swap still in flight: it comes first)
    const int t = h->pactive < 0 ? 0 : 1 - h->pactive;
    hope_env::PoolSet& ps = h->pset[t];
    // two commits without a hope_env_pool_staging call in between: the previous upload may still be reading the pinned arrays
    if (h->pstage.busy) { HIPCHK(hipEventSynchronize(h->ev_pool_copied)); h->pstage.busy = false; }
    int rc = pool_set_reserve(h, ps, n_pool, (int)std::max(l0.size(), l1.size()) + 1);
    if (rc != HOPE_OK) return rc;
    if (3 * 32 * n_pool / 8 > h->pstage_dev_cap) {           // start | dest | bbox: 24 + 24 + 32 bytes per entry
        if (h->pstage_dev) hipFree(h->pstage_dev);
        h->pstage_dev = nullptr; h->pstage_dev_cap = 0;
        hipError_t e_ = hipMalloc((void**)&h->pstage_dev, (size_t)n_pool * 80);
        if (e_ != hipSuccess) return fail(HOPE_ENOMEM, std::string("hipMalloc pool staging: ") + hipGetErrorString(e_));
        h->pstage_dev_cap = 12 * n_pool;
    }
    hipStream_t us = h->pool_stream;
    // the target set was the active one until the previous swap: steps enqueued before that swap may still be reading it
    if (h->pactive >= 0) {
        HIPCHK(hipStreamWaitEvent(us, h->ev_last_step, 0));
        if (h->last_via_steps) for (int i = 0; i < 2; i++) HIPCHK(hipStreamWaitEvent(us, h->ev_step[i], 0));   // (the motion launches of the last step)
    }
    const size_t P = (size_t)n_pool;
    char* dv = (char*)h->pstage_dev;
    {   // only the used prefix of every entry's obstacle tile travels (a 2-D copy: one row per entry): generated lots hold ~7 obstacles of
        // the 128 slots, and the full 67 MB of an 8 192-entry pool took ~1 ms on the hardware queue the upload stream shares with one of
        // the step's streams -- the step enqueued right after a commit took 1.52 ms instead of 0.49, now 0.65 (tools/commit_cost.py; the
        // excess scaled with the pool size; moving k_set_scene_consts off the upload stream did not change it).  The tail of a row
        // keeps the previous generation's bytes; nothing reads beyond n_obst.
        int maxn = 1;
        for (int k = 0; k < n_pool; k++) maxn = std::max(maxn, (int)h->pstage.nobst[k]);
        const size_t pitch = (size_t)h->max_obst * 8 * sizeof(double), width = (size_t)maxn * 8 * sizeof(double);
        if (2 * width <= pitch) HIPCHK(hipMemcpy2DAsync(ps.verts, pitch, h->pstage.verts, pitch, width, P, hipMemcpyHostToDevice, us));
        else HIPCHK(hipMemcpyAsync(ps.verts, h->pstage.verts, P * pitch, hipMemcpyHostToDevice, us));
    }
    HIPCHK(hipMemcpyAsync(ps.nobst, h->pstage.nobst, P * sizeof(int32_t), hipMemcpyHostToDevice, us));
    HIPCHK(hipMemcpyAsync(dv, h->pstage.start, P * 24, hipMemcpyHostToDevice, us));
    HIPCHK(hipMemcpyAsync(dv + P * 24, h->pstage.dest, P * 24, hipMemcpyHostToDevice, us));
    HIPCHK(hipMemcpyAsync(dv + P * 48, h->pstage.bbox, P * 32, hipMemcpyHostToDevice, us));
    memcpy(h->pstage.list, l0.data(), l0.size() * sizeof(int32_t));
    memcpy(h->pstage.list + l0.size(), l1.data(), l1.size() * sizeof(int32_t));
    if (!l0.empty()) HIPCHK(hipMemcpyAsync(ps.list[0], h->pstage.list, l0.size() * sizeof(int32_t), hipMemcpyHostToDevice, us));
    if (!l1.empty()) HIPCHK(hipMemcpyAsync(ps.list[1], h->pstage.list + l0.size(), l1.size() * sizeof(int32_t), hipMemcpyHostToDevice, us));
    HIPCHK(hipEventRecord(h->ev_pool_copied, us));          // the pinned staging may be refilled once this has passed
    {
        const int nc = h->dlp.n_cases, two = h->max_obst > SMALL_TILE;
        ps.n_pool = n_pool; ps.npool_cls[0] = (int)l0.size() - (two ? 0 : nc); ps.npool_cls[1] = (int)l1.size() - (two ? nc : 0);
        ps.lab_kind = 0; ps.lab_host.clear();
    }
    h->pstage.busy = true;
    h->pstage.staged = false;
    hipLaunchKernelGGL(k_set_scene_consts, dim3((n_pool + 127) / 128), dim3(128), 0, us, n_pool, (const int32_t*)nullptr,
                       (const double*)dv, (const double*)(dv + P * 24), (const double*)(dv + P * 48), (const int32_t*)nullptr, ps.c,
                       (double*)nullptr, (int32_t*)nullptr, (int32_t*)nullptr, (double*)nullptr, (int32_t*)nullptr, (int32_t*)nullptr, (int32_t*)nullptr);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(h->ev_pool_ready, us));
    uint64_t content;
    {   // identity of the new pool: every scalar of every entry and two vertex words of each
        uint64_t c = hash_bytes(0x706f6f6cull, h->pstage.start, P * 24);
        c = hash_bytes(c, h->pstage.dest, P * 24);
        c = hash_bytes(c, h->pstage.bbox, P * 32);
        c = hash_bytes(c, h->pstage.nobst, P * sizeof(int32_t));
        const size_t tile_words = (size_t)h->max_obst * 8;
        for (size_t k = 0; k < P; k++) {                     // two vertex words of every entry (the whole tile array is 67 MB per 8 192 lots)
            const size_t nw = (size_t)h->pstage.nobst[k] * 8;
            if (nw == 0) continue;
            uint64_t b0, b1;
            memcpy(&b0, h->pstage.verts + k * tile_words + (k * 7) % nw, 8);
            memcpy(&b1, h->pstage.verts + k * tile_words + nw - 1, 8);
            c = (c ^ b0) * 0x100000001B3ull; c = (c ^ b1) * 0x100000001B3ull; c ^= c >> 29;
        }
        content = c;
    }
    if (relaxed && h->pactive >= 0) {
        // the swap waits for the upload, not the steps for the swap: apply_pending_pool (launch_step / hope_env_redraw / the next commit)
        h->pend.on = true; h->pend.set = t; h->pend.n_pool = n_pool;
        h->pend.cls_n[0] = (int)l0.size(); h->pend.cls_n[1] = (int)l1.size(); h->pend.content = content;
        h->pend.nobst_host.assign(h->pstage.nobst, h->pstage.nobst + n_pool);
        h->pend.generated = false;
        return HOPE_OK;
    }
    // swap: every launch enqueued from now on reads the new set, after waiting (on its own stream) for the upload
    h->pool_verts = ps.verts; h->pool_c = ps.c; h->pool_nobst = ps.nobst;
    h->pool_cls[0] = ps.list[0]; h->pool_cls[1] = ps.list[1];
    h->pool_cls_n[0] = (int)l0.size(); h->pool_cls_n[1] = (int)l1.size();
    h->pool_n = n_pool;
    h->pool_nobst_host.assign(h->pstage.nobst, h->pstage.nobst + n_pool);
    h->gen_host_set = -1;
    h->pactive = t;
    h->pool_wait_pending = true;
    bump_pool_generation(h, content);
    return cur_on_swap(h);
}

int hope_env_set_pool(hope_env_t* h, int n_pool, const double* start, const double* dest, const double* bbox,
                      const double* verts, const int32_t* n_obst) {
    HOPE_ENTER_AS(h, "hope_env_set_pool", "bad argument");
    { int rcs = settle_rs(h); if (rcs != HOPE_OK) return rcs; }
    if (n_pool <= 0 || !start || !dest || !bbox || !verts || !n_obst) return fail(HOPE_EINVAL, "hope_env_set_pool: bad argument");
    for (int k = 0; k < n_pool; k++)
        if (n_obst[k] < 0 || n_obst[k] > h->max_obst) return fail(HOPE_EINVAL, "hope_env_set_pool: n_obst exceeds max_obstacles");
    double *ps, *pd, *pb, *pv;
    int32_t* pn;
    int rc = hope_env_pool_staging(h, n_pool, &ps, &pd, &pb, &pv, &pn);
    if (rc != HOPE_OK) return rc;
    const size_t P = (size_t)n_pool;
    memcpy(ps, start, P * 24); memcpy(pd, dest, P * 24); memcpy(pb, bbox, P * 32);
    memcpy(pv, verts, P * h->max_obst * 8 * sizeof(double)); memcpy(pn, n_obst, P * sizeof(int32_t));
    rc = hope_env_commit_pool(h, n_pool, nullptr);
    if (rc != HOPE_OK) return rc;
    DeviceGuard guard(h->device);
    HIPCHK(hipStreamSynchronize(h->pool_stream));           // the synchronous form: the caller's arrays are free on return anyway
    return HOPE_OK;
}

// ---- lots generated on the device (k_scenegen, hope_scenegen_kernel.h) ---------------------------------------------------------
int hope_scenegen_generate_device(int device_id, int level, int bay_mode, int n, uint64_t seed, int64_t first_index, int max_obstacles,
                                  double* start, double* dest, double* bbox, double* verts, int32_t* n_obst, int32_t* case_id, void* stream) {
    if (level < 0 || level > 2 || n < 0) return fail(HOPE_EINVAL, "hope_scenegen_generate_device: bad argument");
    if (max_obstacles < SG_MAX_RINGS + 1) return fail(HOPE_EINVAL, "hope_scenegen_generate_device: max_obstacles < 18 (a generated lot holds up to 17 obstacles)");
    if (n == 0) return HOPE_OK;
    if (!start || !dest || !bbox || !verts || !n_obst) return fail(HOPE_EINVAL, "hope_scenegen_generate_device: null output buffer");
    HOPE_ON_DEVICE_AS(device_id, HOPE_ENODEV, "hope_scenegen_generate_device: ");
    SgJob job{};
    for (int l = 0; l < 4; l++) job.off[l] = l > level ? n : 0;
    for (int l = 0; l < 3; l++) job.seed[l] = seed;
    job.first_index = first_index; job.bay_mode = bay_mode;
    hipLaunchKernelGGL(k_scenegen, dim3((n + SG_BLOCK - 1) / SG_BLOCK), dim3(SG_BLOCK), 0, (hipStream_t)stream, job, max_obstacles, start, dest,
                       bbox, verts, n_obst, case_id, (double*)nullptr);
    HIPCHK(hipGetLastError());
    return HOPE_OK;
}

// ---- map difficulty labels on the device (k_map_level, hope_maplevel_kernel.h) --------------------------------------------------
int hope_map_level_device(int device_id, int n, int max_obstacles, const double* start, const double* dest, const double* verts,
                          const int32_t* n_obst, uint8_t* level, int32_t* detail, void* stream) {
    if (n <= 0) return fail(HOPE_EINVAL, "hope_map_level_device: n <= 0");
    if (max_obstacles <= 0 || max_obstacles > HOPE_MAX_OBSTACLES) return fail(HOPE_EINVAL, "hope_map_level_device: max_obstacles out of range (1 .. 255)");
    if (!level) return fail(HOPE_EINVAL, "hope_map_level_device: null level buffer");
    if (!start || !dest || !verts || !n_obst) return fail(HOPE_EINVAL, "hope_map_level_device: null input buffer");
    HOPE_ON_DEVICE_AS(device_id, HOPE_ENODEV, "hope_map_level_device: ");
    hipLaunchKernelGGL(k_map_level, dim3(n), dim3(WAVE), 0, (hipStream_t)stream, n, max_obstacles, start, 3, dest, 3, verts, n_obst,
                       (const uint8_t*)nullptr, level, detail);
    HIPCHK(hipGetLastError());
    return HOPE_OK;
}

int hope_env_map_level(hope_env_t* h, const uint8_t* active, uint8_t* level, int32_t* detail, void* stream) {
    HOPE_ENTER(h, "hope_env_map_level");
    if (!level) return fail(HOPE_EINVAL, "hope_env_map_level: null level buffer");
    if (!h->have_scenes) return fail(HOPE_ESTATE, "hope_env_map_level: hope_env_set_scenes has not been called");
    HOPE_ON_DEVICE(h);
    { int rcs = join_rs(h, (hipStream_t)stream); if (rcs != HOPE_OK) return rcs; }   // ordered like every entry that reads the handle's state
    hipLaunchKernelGGL(k_map_level, dim3(h->n), dim3(WAVE), 0, (hipStream_t)stream, h->n, h->max_obst, (const double*)(h->scene_c + SC_START),
                       (int)SC_WORDS, (const double*)(h->scene_c + SC_DEST), (int)SC_WORDS, (const double*)h->verts, (const int32_t*)h->n_obst, active,
                       level, detail);
    HIPCHK(hipGetLastError());
    return HOPE_OK;
}

int hope_env_generate_pool(hope_env_t* h, int n_pool, const int32_t* n_per_level, uint64_t seed, int64_t first_index, int relaxed) {
    HOPE_ENTER_AS(h, "hope_env_generate_pool", "bad argument");
    if (n_pool <= 0 || !n_per_level) return fail(HOPE_EINVAL, "hope_env_generate_pool: bad argument");
    {
        int64_t sum = 0;
        for (int l = 0; l < 3; l++) {
            if (n_per_level[l] < 0) return fail(HOPE_EINVAL, "hope_env_generate_pool: negative lot count");
            sum += n_per_level[l];
        }
        if (sum != n_pool) return fail(HOPE_EINVAL, "hope_env_generate_pool: n_per_level does not sum to n_pool");
    }
    if (h->max_obst < SG_MAX_RINGS + 1) return fail(HOPE_EINVAL, "hope_env_generate_pool: max_obstacles < 18 (a generated lot holds up to 17 obstacles)");
    if (h->pstage.staged) return fail(HOPE_ESTATE, "hope_env_generate_pool: a hope_env_pool_staging fill has not been committed (hope_env_commit_pool first)");
    HOPE_ON_DEVICE(h);
    int rc = pool_init_streams(h);
    if (rc != HOPE_OK) return rc;
    { int rcp = apply_pending_pool(h, true); if (rcp != HOPE_OK) return rcp; }     // (a relaxed swap still in flight: it comes first)
    const bool two = h->max_obst > SMALL_TILE;
    const int n_cases = h->dlp.n_cases;
    const int n_l0 = two ? n_pool : n_pool + n_cases, n_l1 = two ? n_cases : 0;
    const int t = h->pactive < 0 ? 0 : 1 - h->pactive;
    hope_env::PoolSet& ps = h->pset[t];
    rc = pool_set_reserve(h, ps, n_pool, std::max(n_l0, n_l1) + 1);
    if (rc != HOPE_OK) return rc;
    // (set t is not the active one, so nobody is waiting for gen_nobst[t]; an earlier copy into it is ordered before this one on us)
    if (!h->ev_gen_copied[t]) HIPCHK(hipEventCreateWithFlags(&h->ev_gen_copied[t], hipEventDisableTiming));
    if (n_pool > h->gen_nobst_cap[t]) {
        if (h->gen_nobst[t]) { HIPCHK(hipEventSynchronize(h->ev_gen_copied[t])); hipHostFree(h->gen_nobst[t]); }   // (a larger pool than before: rare)
        h->gen_nobst[t] = nullptr; h->gen_nobst_cap[t] = 0;
        hipError_t e_ = hipHostMalloc((void**)&h->gen_nobst[t], (size_t)n_pool * sizeof(int32_t));
        if (e_ != hipSuccess) return fail(HOPE_ENOMEM, std::string("hipHostMalloc generated n_obst: ") + hipGetErrorString(e_));
        h->gen_nobst_cap[t] = n_pool;
    }
    hipStream_t us = h->pool_stream;
    // the target set was the active one until the previous swap: steps enqueued before that swap may still be reading it
    if (h->pactive >= 0) {
        HIPCHK(hipStreamWaitEvent(us, h->ev_last_step, 0));
        if (h->last_via_steps) for (int i = 0; i < 2; i++) HIPCHK(hipStreamWaitEvent(us, h->ev_step[i], 0));   // (the motion launches of the last step)
    }
    SgJob job{};
    job.off[0] = 0;
    for (int l = 0; l < 3; l++) {
        job.off[l + 1] = job.off[l] + n_per_level[l];
        job.seed[l] = seed * 1000003ull + (uint64_t)l;          // PoolRefresher._fill's convention: level l draws from seed * 1000003 + l
    }
    job.first_index = first_index; job.bay_mode = -1;
    hipLaunchKernelGGL(k_scenegen, dim3((n_pool + SG_BLOCK - 1) / SG_BLOCK), dim3(SG_BLOCK), 0, us, job, h->max_obst, (double*)nullptr, (double*)nullptr,
                       (double*)nullptr, ps.verts, ps.nobst, (int32_t*)nullptr, ps.c);
    hipLaunchKernelGGL(k_pool_lists_generated, dim3((n_pool + n_cases + 255) / 256), dim3(256), 0, us, n_pool, n_cases, two ? 1 : 0, ps.list[0], ps.list[1]);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(h->gen_nobst[t], ps.nobst, (size_t)n_pool * sizeof(int32_t), hipMemcpyDeviceToHost, us));
    HIPCHK(hipEventRecord(h->ev_gen_copied[t], us));
    HIPCHK(hipEventRecord(h->ev_pool_ready, us));
    h->gen_nobst_n[t] = n_pool;
    ps.n_pool = n_pool; ps.npool_cls[0] = n_pool; ps.npool_cls[1] = 0;
    ps.lab_kind = 1; ps.lab_host.clear();
    for (int l = 0; l < 3; l++) ps.gen_counts[l] = n_per_level[l];
    // identity of the new pool: a pure function of the arguments (the lots are a pure function of them)
    uint64_t content = 0x67656e706f6f6cull;
    content = fold64(content, (uint64_t)(uint32_t)n_pool);
    for (int l = 0; l < 3; l++) content = fold64(content, (uint64_t)(uint32_t)n_per_level[l]);
    content = fold64(content, seed);
    content = fold64(content, (uint64_t)first_index);
    if (relaxed && h->pactive >= 0) {
        h->pend.on = true; h->pend.set = t; h->pend.n_pool = n_pool;
        h->pend.cls_n[0] = n_l0; h->pend.cls_n[1] = n_l1; h->pend.content = content;
        h->pend.nobst_host.clear(); h->pend.generated = true;  // (pool_nobst_host: settle_gen_nobst, after the swap has been applied)
        return HOPE_OK;
    }
    h->pool_verts = ps.verts; h->pool_c = ps.c; h->pool_nobst = ps.nobst;
    h->pool_cls[0] = ps.list[0]; h->pool_cls[1] = ps.list[1];
    h->pool_cls_n[0] = n_l0; h->pool_cls_n[1] = n_l1;
    h->pool_n = n_pool;
    h->pactive = t;
    h->gen_host_set = t;
    h->pool_wait_pending = true;
    bump_pool_generation(h, content);
    return cur_on_swap(h);
}

// the class lists of the ACTIVE set after the Dragon-Lake cases changed (rare; host-synchronous)
static int refresh_pool_lists_sync(hope_env_t* h) {
    int rc = pool_init_streams(h);
    if (rc != HOPE_OK) return rc;
    HIPCHK(hipDeviceSynchronize());
    { int rcg = settle_gen_nobst(h); if (rcg != HOPE_OK) return rcg; }
    std::vector<int32_t> l0, l1;
    build_pool_lists(h, h->pool_nobst_host.data(), h->pool_n, l0, l1);
    if (h->pactive < 0) h->pactive = 0;
    hope_env::PoolSet& ps = h->pset[h->pactive];
    rc = pool_set_reserve(h, ps, std::max(h->pool_n, ps.cap), (int)std::max(l0.size(), l1.size()) + 1);
    if (rc != HOPE_OK) return rc;
    if (!l0.empty()) HIPCHK(hipMemcpy(ps.list[0], l0.data(), l0.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    if (!l1.empty()) HIPCHK(hipMemcpy(ps.list[1], l1.data(), l1.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    h->pool_cls[0] = ps.list[0]; h->pool_cls[1] = ps.list[1];
    h->pool_cls_n[0] = (int)l0.size(); h->pool_cls_n[1] = (int)l1.size();
    {
        const int nc = h->dlp.n_cases, two = h->max_obst > SMALL_TILE;
        ps.n_pool = h->pool_n; ps.npool_cls[0] = (int)l0.size() - (two ? 0 : nc); ps.npool_cls[1] = (int)l1.size() - (two ? nc : 0);
    }
    return HOPE_OK;
}

int hope_env_set_dlp_cases(hope_env_t* h, int n_cases, const double* dest, const int32_t* cand_off, const double* cand,
                           const int32_t* case_set, int n_sets, const int32_t* set_off, const double* set_verts) {
    HOPE_ENTER_AS(h, "hope_env_set_dlp_cases", "bad argument");
    { int rcs = settle_rs(h); if (rcs != HOPE_OK) return rcs; }
    if (n_cases < 0 || (n_cases > 0 && (!dest || !cand_off || !cand || !case_set || n_sets <= 0 || !set_off || !set_verts)))
        return fail(HOPE_EINVAL, "hope_env_set_dlp_cases: bad argument");
    if (h->cur.on) return fail(HOPE_ESTATE, "hope_env_set_dlp_cases: the curriculum is on and its buckets are sized by the cases (hope_env_curriculum_disable first)");
    for (int c = 0; c < n_cases; c++) {
        if (cand_off[c + 1] <= cand_off[c]) return fail(HOPE_EINVAL, "hope_env_set_dlp_cases: a case without start candidates");
        if (case_set[c] < 0 || case_set[c] >= n_sets) return fail(HOPE_EINVAL, "hope_env_set_dlp_cases: case_set out of range");
    }
    HOPE_ON_DEVICE(h);
    // a relaxed commit still pending takes over FIRST: its class lists were built with the old cases, and refresh_pool_lists_sync
    // below rebuilds the lists of the set that is active when it runs
    { int rcp = apply_pending_pool(h, true); if (rcp != HOPE_OK) return rcp; }
    HIPCHK(hipDeviceSynchronize());
    for (void*& q : h->dlp_mem) { if (q) hipFree(q); q = nullptr; }
    h->dlp = DlpCases{};
    if (n_cases > 0) {
        const size_t nc = (size_t)cand_off[n_cases], nv = (size_t)set_off[n_sets];
        const void* src[6] = {dest, cand_off, cand, case_set, set_off, set_verts};
        const size_t bytes[6] = {sizeof(double) * 3 * n_cases, sizeof(int32_t) * (n_cases + 1), sizeof(double) * 3 * nc,
                                 sizeof(int32_t) * n_cases, sizeof(int32_t) * (n_sets + 1), sizeof(double) * 8 * nv};
        for (int i = 0; i < 6; i++) {
            hipError_t e_ = hipMalloc(&h->dlp_mem[i], bytes[i]);
            if (e_ != hipSuccess) return fail(HOPE_ENOMEM, std::string("hipMalloc dlp cases: ") + hipGetErrorString(e_));
            HIPCHK(hipMemcpy(h->dlp_mem[i], src[i], bytes[i], hipMemcpyHostToDevice));
        }
        h->dlp.n_cases = n_cases;
        h->dlp.dest = (const double*)h->dlp_mem[0]; h->dlp.cand_off = (const int32_t*)h->dlp_mem[1];
        h->dlp.cand = (const double*)h->dlp_mem[2]; h->dlp.case_set = (const int32_t*)h->dlp_mem[3];
        h->dlp.set_off = (const int32_t*)h->dlp_mem[4]; h->dlp.set_verts = (const double*)h->dlp_mem[5];
        uint64_t c = 0x646c70ull;
        for (int i = 0; i < 6; i++) c = hash_bytes(c, src[i], bytes[i]);
        bump_pool_generation(h, c);
    } else bump_pool_generation(h, 0x6e6f646c70ull);        // the cases were removed
    return refresh_pool_lists_sync(h);
}

int hope_env_set_draw_class(hope_env_t* h, const int32_t* scene_ids, int n, const uint8_t* cls) {
    HOPE_ENTER_AS(h, "hope_env_set_draw_class", "null argument");
    { int rcs = settle_rs(h); if (rcs != HOPE_OK) return rcs; }
    if (n < 0 || (n > 0 && (!scene_ids || !cls))) return fail(HOPE_EINVAL, "hope_env_set_draw_class: null argument");
    if (!h->have_scenes) return fail(HOPE_ESTATE, "hope_env_set_draw_class: hope_env_set_scenes has not been called");
    HOPE_ON_DEVICE(h);
    HIPCHK(hipDeviceSynchronize());
    // the obstacle counts as they are NOW: device-side draws (HOPE_AUTO_REDRAW, hope_env_redraw) change them behind the host copy
    HIPCHK(hipMemcpy(h->n_obst_host.data(), h->n_obst, (size_t)h->n * sizeof(int32_t), hipMemcpyDeviceToHost));
    for (int k = 0; k < n; k++) {
        if (scene_ids[k] < 0 || scene_ids[k] >= h->n) return fail(HOPE_EINVAL, "hope_env_set_draw_class: scene id out of range");
        if (!cls[k] && h->n_obst_host[scene_ids[k]] > SMALL_TILE)
            return fail(HOPE_EINVAL, "hope_env_set_draw_class: a scene with more than 32 obstacles cannot join the small class");
    }
    for (int k = 0; k < n; k++) h->slot_cls_host[scene_ids[k]] = (cls[k] && h->max_obst > SMALL_TILE) ? 1 : 0;
    int rc = rebuild_class_lists(h);
    if (rc != HOPE_OK) return rc;
    HIPCHK(hipDeviceSynchronize());
    return HOPE_OK;
}

int hope_env_pool_overflow(hope_env_t* h, int32_t* count) {
    HOPE_ENTER_AS(h, "hope_env_pool_overflow", "null argument");
    { int rcs = settle_rs(h); if (rcs != HOPE_OK) return rcs; }
    if (!count) return fail(HOPE_EINVAL, "hope_env_pool_overflow: null argument");
    HOPE_ON_DEVICE(h);
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(count, h->pool_overflow, sizeof(int32_t), hipMemcpyDeviceToHost));
    return HOPE_OK;
}

// the maps the scenes hold NOW (after device-side draws they exist on the device only): host-synchronous
int hope_env_download_scenes(hope_env_t* h, const int32_t* scene_ids, int n, double* start, double* dest, double* bbox, double* verts,
                             int32_t* n_obst) {
    HOPE_ENTER_AS(h, "hope_env_download_scenes", "bad argument");
    { int rcs = settle_rs(h); if (rcs != HOPE_OK) return rcs; }
    if (n < 0 || (n > 0 && !scene_ids)) return fail(HOPE_EINVAL, "hope_env_download_scenes: bad argument");
    HOPE_ON_DEVICE(h);
    HIPCHK(hipDeviceSynchronize());
    const size_t tile = (size_t)h->max_obst * 8;
    std::vector<double> c(SC_WORDS);
    for (int k = 0; k < n; k++) {
        const int s_ = scene_ids[k];
        if (s_ < 0 || s_ >= h->n) return fail(HOPE_EINVAL, "hope_env_download_scenes: scene id out of range");
        HIPCHK(hipMemcpy(c.data(), h->scene_c + (size_t)s_ * SC_WORDS, SC_WORDS * sizeof(double), hipMemcpyDeviceToHost));
        for (int i = 0; i < 3; i++) { if (start) start[3 * (size_t)k + i] = c[SC_START + i]; if (dest) dest[3 * (size_t)k + i] = c[SC_DEST + i]; }
        for (int i = 0; i < 4; i++) if (bbox) bbox[4 * (size_t)k + i] = c[SC_BBOX + i];
        if (verts) HIPCHK(hipMemcpy(verts + (size_t)k * tile, h->verts + (size_t)s_ * tile, tile * sizeof(double), hipMemcpyDeviceToHost));
        if (n_obst) HIPCHK(hipMemcpy(n_obst + k, h->n_obst + s_, sizeof(int32_t), hipMemcpyDeviceToHost));
    }
    return HOPE_OK;
}

int hope_env_set_redraw_seed(hope_env_t* h, uint64_t seed) {
    HOPE_ENTER(h, "hope_env_set_redraw_seed");
    h->redraw_seed = seed;
    return HOPE_OK;
}

int hope_env_redraw(hope_env_t* h, const uint8_t* mask, uint64_t seed, void* stream) {
    HOPE_ENTER_AS(h, "hope_env_redraw", "null argument");
    { DeviceGuard g0(h->device); int rcs = join_rs(h, (hipStream_t)stream); if (rcs != HOPE_OK) return rcs; }
    if (!mask) return fail(HOPE_EINVAL, "hope_env_redraw: null argument");
    if (!h->have_scenes) return fail(HOPE_ESTATE, "hope_env_redraw: hope_env_set_scenes has not been called");
    if (h->pool_n <= 0 && h->dlp.n_cases <= 0) return fail(HOPE_ESTATE, "hope_env_redraw: no scene pool (hope_env_set_pool / hope_env_set_dlp_cases)");
    int rc0 = check_pool_classes(h, "hope_env_redraw");
    if (rc0 != HOPE_OK) return rc0;
    HOPE_ON_DEVICE(h);
    { int rcp = apply_pending_pool(h, false); if (rcp != HOPE_OK) return rcp; }
    if (h->pool_wait_pending) { HIPCHK(hipStreamWaitEvent((hipStream_t)stream, h->ev_pool_ready, 0)); h->pool_wait_pending = false; }
    const int32_t* dl[2]; int dn[2];
    draw_lists(h, dl, dn);
    h->draw_set = h->pactive;
    hipLaunchKernelGGL(k_redraw, dim3(h->n), dim3(WAVE), 0, (hipStream_t)stream, h->max_obst, mask, seed, dl[0],
                       dn[0], dl[1], dn[1], h->pool_verts, h->pool_c, h->pool_nobst, h->verts,
                       h->scene_c, h->n_obst, h->state, h->tstep, h->traj, h->traj_len, h->traj_valid, h->cur_pool, h->episode, h->obb,
                       h->dlp, h->pool_overflow, h->slot_cls, h->layer_valid, h->fverts, h->fbox, h->eflag);
    HIPCHK(hipGetLastError());
    if (h->cur.on && h->pactive >= 0) {                     // the curriculum notes the buckets of the maps just drawn
        const hope_env::PoolSet& ps = h->pset[h->pactive];
        hipLaunchKernelGGL(k_curriculum_tally, dim3((h->n + 255) / 256), dim3(256), 0, (hipStream_t)stream, h->n, (const int32_t*)nullptr,
                           (const uint8_t*)nullptr, mask, h->cur_pool, ps.label, ps.n_pool, h->cur.n_cases, h->cur.scene_bucket, h->episode, h->cur.noted_ep, h->cur.dev);
        HIPCHK(hipGetLastError());
    }
    if (h->pactive >= 0 && h->ev_last_step) HIPCHK(hipEventRecord(h->ev_last_step, (hipStream_t)stream));
    return HOPE_OK;
}

// Snapshot / restore of the map each scene holds after device-side draws.  A draw is a pure function of (seed, scene, episode
// counter) and of the pool / case lists, so a map is restored by repeating its draw: the counters go back by one and k_redraw runs
// for the scenes that held a drawn map.  Pose / t / accumulator are restored separately (hope_env_upload_state, afterwards).
int hope_env_download_pool_state(hope_env_t* h, int32_t* pool_index, uint32_t* episode) {
    HOPE_ENTER(h, "hope_env_download_pool_state");
    { int rcs = settle_rs(h); if (rcs != HOPE_OK) return rcs; }
    HOPE_ON_DEVICE(h);
    { int rcp = apply_pending_pool(h, true); if (rcp != HOPE_OK) return rcp; }     // the snapshot belongs to the pool the next step draws from
    HIPCHK(hipDeviceSynchronize());
    if (pool_index) HIPCHK(hipMemcpy(pool_index, h->cur_pool, (size_t)h->n * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (episode) HIPCHK(hipMemcpy(episode, h->episode, (size_t)h->n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return HOPE_OK;
}

int hope_env_restore_maps(hope_env_t* h, const uint8_t* drawn /* host [N]: the scene held a drawn map */, const uint32_t* episode, uint64_t seed,
                          uint64_t pool_generation) {
    HOPE_ENTER_AS(h, "hope_env_restore_maps", "null argument");
    { int rcs = settle_rs(h); if (rcs != HOPE_OK) return rcs; }
    if (!drawn || !episode) return fail(HOPE_EINVAL, "hope_env_restore_maps: null argument");
    { DeviceGuard guard0(h->device); int rcp = apply_pending_pool(h, true); if (rcp != HOPE_OK) return rcp; }   // (compare generations after a pending swap)
    if (h->pool_n <= 0 && h->dlp.n_cases <= 0) return fail(HOPE_ESTATE, "hope_env_restore_maps: no scene pool");
    uint64_t gen_now = 0;
    if (pool_generation != 0) { int rcg = effective_generation(h, &gen_now); if (rcg != HOPE_OK) return rcg; }
    if (pool_generation != 0 && pool_generation != gen_now)
        return fail(HOPE_ESTATE, "hope_env_restore_maps: the scene pool or the curriculum's draw lists have been replaced since the snapshot (pool generation " +
                                 std::to_string(gen_now) + " now, " + std::to_string(pool_generation) + " in the snapshot): repeating the draws "
                                 "would give other maps -- snapshot refreshed runs with hope_env_download_scenes / hope_env_set_scenes");
    HOPE_ON_DEVICE(h);
    HIPCHK(hipDeviceSynchronize());
    std::vector<uint32_t> ep(episode, episode + h->n);
    for (int i = 0; i < h->n; i++) if (drawn[i]) { if (ep[i] == 0) return fail(HOPE_EINVAL, "hope_env_restore_maps: a drawn scene with episode counter 0"); ep[i] -= 1; }
    HIPCHK(hipMemcpy(h->episode, ep.data(), (size_t)h->n * sizeof(uint32_t), hipMemcpyHostToDevice));
    uint8_t* dmask = nullptr;
    HIPCHK(hipMalloc((void**)&dmask, (size_t)h->n));
    hipError_t e = hipMemcpy(dmask, drawn, (size_t)h->n, hipMemcpyHostToDevice);
    int rc = e == hipSuccess ? hope_env_redraw(h, dmask, seed, nullptr) : fail(HOPE_EHIP, "hipMemcpy mask");
    hipDeviceSynchronize();
    hipFree(dmask);
    return rc;
}

int hope_env_download_pool_index(hope_env_t* h, int32_t* out) {
    HOPE_ENTER_AS(h, "hope_env_download_pool_index", "null argument");
    { int rcs = settle_rs(h); if (rcs != HOPE_OK) return rcs; }
    if (!out) return fail(HOPE_EINVAL, "hope_env_download_pool_index: null argument");
    HOPE_ON_DEVICE(h);
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(out, h->cur_pool, (size_t)h->n * sizeof(int32_t), hipMemcpyDeviceToHost));
    return HOPE_OK;
}

// ---- curriculum for new-map draws (include/hope_env.h; kernels: hope_curriculum_kernel.h, arithmetic: hope_curriculum_core.h) ----
// The weighted lists live in two buffers like the pool sets: a rebuild fills the buffer the kernels are not reading on the pool
// stream and publishes it through draw_lists / sync_cold; the next step waits for it in stream order (pool_wait_pending).
static const hope_curriculum_params CW_DEFAULTS = {{0.95, 0.95, 0.9, 0.99}, 250.0, 10.0, 0.01, 0.005, 0.5, 0.2, 200, 500};

static void cur_free(hope_env_t* h) {
    hope_env::Curriculum& cu = h->cur;
    for (void* q : {cu.mem, (void*)cu.scene_bucket, (void*)cu.noted_ep, (void*)cu.wl[0][0], (void*)cu.prefix[0]}) if (q) hipFree(q);
    if (cu.ev_order) hipEventDestroy(cu.ev_order);
    cu = hope_env::Curriculum{};
}

// what the class lists of pool set t are made of, and the order of their pool entries
static void cur_set_groups(const hope_env_t* h, int t, CwClass cls[2], const int32_t* sorted[2]) {
    const hope_env::PoolSet& ps = h->pset[t];
    const bool two = h->max_obst > SMALL_TILE;
    for (int c = 0; c < 2; c++) {
        cls[c] = CwClass{};
        cls[c].n_cases = c == (two ? 1 : 0) ? h->dlp.n_cases : 0;
        sorted[c] = ps.list[c];
        if (ps.lab_kind == 0) cls[c].cnt[3] = ps.npool_cls[c];
        else if (ps.lab_kind == 1) { if (c == 0) for (int l = 0; l < 3; l++) cls[c].cnt[l] = ps.gen_counts[l]; }
        else {
            sorted[c] = ps.sorted_own[c];
            // (counted again from the labels: cheap, and the only place that needs them)
        }
    }
    if (ps.lab_kind == 2) {
        for (int k = 0; k < ps.n_pool; k++) {
            const int c = two && h->pool_nobst_host[k] > SMALL_TILE ? 1 : 0;
            const int b = ps.lab_host[k];
            cls[c].cnt[b < 3 ? b : 3]++;
        }
    }
}

// the device label table of set t (tally) on stream s
static int cur_write_labels(hope_env_t* h, int t, hipStream_t s) {
    hope_env::PoolSet& ps = h->pset[t];
    if (ps.n_pool <= 0 || !ps.label) return HOPE_OK;
    if (ps.lab_kind == 1) {
        size_t off = 0;
        for (int l = 0; l < 3; l++) { if (ps.gen_counts[l] > 0) HIPCHK(hipMemsetAsync(ps.label + off, l, (size_t)ps.gen_counts[l], s)); off += (size_t)ps.gen_counts[l]; }
    } else if (ps.lab_kind == 2) HIPCHK(hipMemcpyAsync(ps.label, ps.lab_host.data(), (size_t)ps.n_pool, hipMemcpyHostToDevice, s));
    else HIPCHK(hipMemsetAsync(ps.label, CW_UNLABELLED, (size_t)ps.n_pool, s));
    return HOPE_OK;
}

// weights + fill for the ACTIVE pool set into the buffer the kernels are not reading, on the pool stream; published at once
static int cur_build_lists(hope_env_t* h, bool fold, hipStream_t after) {
    hope_env::Curriculum& cu = h->cur;
    int rc = pool_init_streams(h);
    if (rc != HOPE_OK) return rc;
    hipStream_t us = h->pool_stream;
    if (fold) {                                              // the tallies enqueued so far come first
        HIPCHK(hipEventRecord(cu.ev_order, after));
        HIPCHK(hipStreamWaitEvent(us, cu.ev_order, 0));
    }
    // the target buffer was the active one until the previous swap: steps enqueued before that swap may still be reading it
    if (h->pactive >= 0) {
        HIPCHK(hipStreamWaitEvent(us, h->ev_last_step, 0));
        if (h->last_via_steps) for (int i = 0; i < 2; i++) HIPCHK(hipStreamWaitEvent(us, h->ev_step[i], 0));
    }
    const int w = cu.wactive < 0 ? 0 : 1 - cu.wactive;
    CwJob job{};
    CwFill fl{};
    job.P = cu.P; job.n_cases = cu.n_cases; job.fold = fold ? 1 : 0; job.prefix = cu.prefix[w];
    cur_set_groups(h, h->pactive, job.cls, fl.sorted);
    for (int c = 0; c < 2; c++) { fl.cls[c] = job.cls[c]; fl.out[c] = cu.wl[w][c]; cu.cls[c] = job.cls[c]; }
    fl.G = cu.nb; fl.prefix = cu.prefix[w];
    hipLaunchKernelGGL(k_curriculum_weights, dim3(1), dim3(64), 0, us, job, cu.dev);
    hipLaunchKernelGGL(k_curriculum_fill, dim3(256, 2), dim3(256), 0, us, fl);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(h->ev_pool_ready, us));
    cu.wactive = w;
    h->pool_wait_pending = true;
    return HOPE_OK;
}

// a pool set has just become the active one: its labels and weighted lists, before anything draws from it
static int cur_on_swap(hope_env_t* h) {
    if (!h->cur.on) return HOPE_OK;
    int rc = pool_init_streams(h);
    if (rc != HOPE_OK) return rc;
    for (int c = 0; c < 2; c++)
        if (h->pool_cls_n[c] > CW_LIST_LEN) return fail(HOPE_EINVAL, "curriculum: a draw list longer than HOPE_CURRICULUM_LIST_LEN entries");
    rc = cur_write_labels(h, h->pactive, h->pool_stream);
    if (rc != HOPE_OK) return rc;
    return cur_build_lists(h, false, nullptr);
}

static int cur_init_scene_buckets(hope_env_t* h, hipStream_t s) {
    const hope_env::PoolSet& ps = h->pset[h->pactive];
    hipLaunchKernelGGL(k_curriculum_tally, dim3((h->n + 255) / 256), dim3(256), 0, s, h->n, (const int32_t*)nullptr, (const uint8_t*)nullptr,
                       (const uint8_t*)nullptr, h->cur_pool, ps.label, ps.n_pool, h->cur.n_cases, h->cur.scene_bucket, h->episode, h->cur.noted_ep, h->cur.dev);
    HIPCHK(hipGetLastError());
    return HOPE_OK;
}

static void cur_layout(hope_env::Curriculum& cu) {
    const size_t nb = (size_t)cu.nb;
    char* p = (char*)cu.mem;
    cu.dev.episodes = (unsigned long long*)p; p += (nb + 1) * 8;
    cu.dev.successes = (unsigned long long*)p; p += (nb + 1) * 8;
    cu.dev.folded_e = (unsigned long long*)p; p += nb * 8;
    cu.dev.folded_s = (unsigned long long*)p; p += nb * 8;
    cu.dev.win_n = (double*)p; p += nb * 8;
    cu.dev.win_s = (double*)p; p += nb * 8;
    cu.dev.prob = (double*)p; p += nb * 8;
    cu.dev.pw = (double*)p;
}
static size_t cur_mem_bytes(int nb) { return ((size_t)nb * 7 + 2 + 4) * 8; }

int hope_env_curriculum_enable(hope_env_t* h, const hope_curriculum_params* params) {
    HOPE_ENTER(h, "hope_env_curriculum_enable");
    { int rcs = settle_rs(h); if (rcs != HOPE_OK) return rcs; }
    const hope_curriculum_params P = params ? *params : CW_DEFAULTS;
    if (!(P.type_window > 0.0) || !(P.case_window > 0.0) || !(P.type_fail_min > 0.0) || !(P.case_fail_min > 0.0) ||
        !(P.worst_share >= 0.0 && P.worst_share <= 1.0) || !(P.case_uniform >= 0.0 && P.case_uniform <= 1.0))
        return fail(HOPE_EINVAL, "hope_env_curriculum_enable: windows and failure floors must be positive, shares in [0, 1]");
    HOPE_ON_DEVICE(h);
    { int rcp = apply_pending_pool(h, true); if (rcp != HOPE_OK) return rcp; }
    if ((h->pool_n <= 0 && h->dlp.n_cases <= 0) || h->pactive < 0)
        return fail(HOPE_ESTATE, "hope_env_curriculum_enable: no scene pool and no Dragon-Lake cases (hope_env_set_pool / hope_env_generate_pool / hope_env_set_dlp_cases first)");
    if (4 + h->dlp.n_cases > CW_MAX_GROUPS) return fail(HOPE_EINVAL, "hope_env_curriculum_enable: more than 250 Dragon-Lake cases (a bucket id is one byte)");
    for (int c = 0; c < 2; c++)
        if (h->pool_cls_n[c] > CW_LIST_LEN) return fail(HOPE_EINVAL, "hope_env_curriculum_enable: a draw list longer than HOPE_CURRICULUM_LIST_LEN entries");
    HIPCHK(hipDeviceSynchronize());
    { int rcg = settle_gen_nobst(h); if (rcg != HOPE_OK) return rcg; }
    cur_free(h);
    hope_env::Curriculum& cu = h->cur;
    cu.P = P; cu.n_cases = h->dlp.n_cases; cu.nb = 4 + cu.n_cases;
    hipError_t e_ = hipMalloc(&cu.mem, cur_mem_bytes(cu.nb));
    if (e_ == hipSuccess) e_ = hipMalloc((void**)&cu.scene_bucket, (size_t)h->n);
    if (e_ == hipSuccess) e_ = hipMalloc((void**)&cu.noted_ep, (size_t)h->n * sizeof(uint32_t));
    if (e_ == hipSuccess) e_ = hipMalloc((void**)&cu.wl[0][0], (size_t)4 * CW_LIST_LEN * sizeof(int32_t));
    if (e_ == hipSuccess) e_ = hipMalloc((void**)&cu.prefix[0], (size_t)4 * (CW_MAX_GROUPS + 1) * sizeof(int32_t));
    if (e_ == hipSuccess) e_ = hipEventCreateWithFlags(&cu.ev_order, hipEventDisableTiming);
    if (e_ != hipSuccess) { cur_free(h); return fail(HOPE_ENOMEM, std::string("hope_env_curriculum_enable: ") + hipGetErrorString(e_)); }
    cu.wl[0][1] = cu.wl[0][0] + CW_LIST_LEN; cu.wl[1][0] = cu.wl[0][0] + 2 * (size_t)CW_LIST_LEN; cu.wl[1][1] = cu.wl[0][0] + 3 * (size_t)CW_LIST_LEN;
    cu.prefix[1] = cu.prefix[0] + 2 * (CW_MAX_GROUPS + 1);
    cur_layout(cu);
    HIPCHK(hipMemset(cu.mem, 0, cur_mem_bytes(cu.nb)));
    HIPCHK(hipMemset(cu.scene_bucket, CW_UNLABELLED, (size_t)h->n));
    HIPCHK(hipMemset(cu.noted_ep, 0, (size_t)h->n * sizeof(uint32_t)));
    HIPCHK(hipMemset(cu.wl[0][0], 0xFF, (size_t)4 * CW_LIST_LEN * sizeof(int32_t)));
    HIPCHK(hipMemset(cu.prefix[0], 0, (size_t)4 * (CW_MAX_GROUPS + 1) * sizeof(int32_t)));
    cu.on = true;
    int rc = cur_on_swap(h);
    if (rc == HOPE_OK) rc = cur_init_scene_buckets(h, h->pool_stream);
    if (rc != HOPE_OK) { cur_free(h); return rc; }
    HIPCHK(hipDeviceSynchronize());
    return HOPE_OK;
}

int hope_env_curriculum_disable(hope_env_t* h) {
    HOPE_ENTER(h, "hope_env_curriculum_disable");
    { int rcs = settle_rs(h); if (rcs != HOPE_OK) return rcs; }
    HOPE_ON_DEVICE(h);
    HIPCHK(hipDeviceSynchronize());                         // steps in flight read the weighted lists
    cur_free(h);
    return HOPE_OK;
}

int hope_env_set_pool_buckets(hope_env_t* h, int n_pool, const uint8_t* bucket) {
    HOPE_ENTER_AS(h, "hope_env_set_pool_buckets", "null argument");
    { int rcs = settle_rs(h); if (rcs != HOPE_OK) return rcs; }
    if (!bucket) return fail(HOPE_EINVAL, "hope_env_set_pool_buckets: null argument");
    HOPE_ON_DEVICE(h);
    { int rcp = apply_pending_pool(h, true); if (rcp != HOPE_OK) return rcp; }
    if (h->pool_n <= 0 || h->pactive < 0) return fail(HOPE_ESTATE, "hope_env_set_pool_buckets: no scene pool");
    if (n_pool != h->pool_n)
        return fail(HOPE_EINVAL, "hope_env_set_pool_buckets: " + std::to_string(n_pool) + " labels for a resident pool of " + std::to_string(h->pool_n) + " entries");
    for (int k = 0; k < n_pool; k++)
        if (bucket[k] > 2 && bucket[k] != CW_UNLABELLED)
            return fail(HOPE_EINVAL, "hope_env_set_pool_buckets: bucket id " + std::to_string((int)bucket[k]) + " of entry " + std::to_string(k) + " is out of range (0, 1, 2 or 255)");
    HIPCHK(hipDeviceSynchronize());
    { int rcg = settle_gen_nobst(h); if (rcg != HOPE_OK) return rcg; }
    hope_env::PoolSet& ps = h->pset[h->pactive];
    // the class lists' pool entries ordered by label (stable): what a weighted list cycles through per group
    const bool two = h->max_obst > SMALL_TILE;
    std::vector<int32_t> srt[2];
    for (int g = 0; g < 4; g++)
        for (int k = 0; k < n_pool; k++) {
            const int b = bucket[k] < 3 ? bucket[k] : 3;
            if (b == g) srt[two && h->pool_nobst_host[k] > SMALL_TILE ? 1 : 0].push_back(k);
        }
    if (n_pool > ps.sorted_own_cap) {
        for (int c = 0; c < 2; c++) { if (ps.sorted_own[c]) hipFree(ps.sorted_own[c]); ps.sorted_own[c] = nullptr; }
        ps.sorted_own_cap = 0;
        for (int c = 0; c < 2; c++) {
            hipError_t e_ = hipMalloc((void**)&ps.sorted_own[c], (size_t)n_pool * sizeof(int32_t));
            if (e_ != hipSuccess) return fail(HOPE_ENOMEM, std::string("hipMalloc pool labels: ") + hipGetErrorString(e_));
        }
        ps.sorted_own_cap = n_pool;
    }
    for (int c = 0; c < 2; c++)
        if (!srt[c].empty()) HIPCHK(hipMemcpy(ps.sorted_own[c], srt[c].data(), srt[c].size() * sizeof(int32_t), hipMemcpyHostToDevice));
    ps.lab_host.assign(bucket, bucket + n_pool);
    ps.lab_kind = 2;
    if (h->cur.on) {
        int rc = cur_on_swap(h);
        if (rc == HOPE_OK) rc = cur_init_scene_buckets(h, h->pool_stream);
        if (rc != HOPE_OK) return rc;
        HIPCHK(hipDeviceSynchronize());
    }
    return HOPE_OK;
}

int hope_env_curriculum_tally(hope_env_t* h, const int32_t* status, const uint8_t* done, void* stream) {
    HOPE_ENTER_AS(h, "hope_env_curriculum_tally", "null argument");
    if (!status || !done) return fail(HOPE_EINVAL, "hope_env_curriculum_tally: null argument");
    if (!h->cur.on) return fail(HOPE_ESTATE, "hope_env_curriculum_tally: the curriculum is off (hope_env_curriculum_enable first)");
    HOPE_ON_DEVICE(h);
    // the labels of the set the step just drew from: a relaxed commit may have swapped sets at that step, never after it
    const int t = h->draw_set >= 0 ? h->draw_set : h->pactive;
    const hope_env::PoolSet& ps = h->pset[t];
    hipLaunchKernelGGL(k_curriculum_tally, dim3((h->n + 255) / 256), dim3(256), 0, (hipStream_t)stream, h->n, status, done, (const uint8_t*)nullptr,
                       h->cur_pool,
                       ps.label, ps.n_pool, h->cur.n_cases, h->cur.scene_bucket, h->episode, h->cur.noted_ep, h->cur.dev);
    HIPCHK(hipGetLastError());
    // the tally reads the label table of set t: a later swap that rewrites that table on the pool stream waits for this event
    if (h->pactive >= 0 && h->ev_last_step) HIPCHK(hipEventRecord(h->ev_last_step, (hipStream_t)stream));
    return HOPE_OK;
}

int hope_env_curriculum_update(hope_env_t* h, void* stream) {
    HOPE_ENTER(h, "hope_env_curriculum_update");
    if (!h->cur.on) return fail(HOPE_ESTATE, "hope_env_curriculum_update: the curriculum is off (hope_env_curriculum_enable first)");
    HOPE_ON_DEVICE(h);
    { int rcp = apply_pending_pool(h, false); if (rcp != HOPE_OK) return rcp; }   // (lists are built for the set the next step draws from)
    int rc = cur_build_lists(h, true, (hipStream_t)stream);
    if (rc == HOPE_OK) h->cur.updates++;
    return rc;
}

int hope_env_curriculum_state(hope_env_t* h, int32_t* n_buckets, uint64_t* episodes, uint64_t* successes, double* win_n, double* win_s,
                              double* prob, double* pw, uint64_t* misc) {
    HOPE_ENTER(h, "hope_env_curriculum_state");
    { int rcs = settle_rs(h); if (rcs != HOPE_OK) return rcs; }
    const hope_env::Curriculum& cu = h->cur;
    if (n_buckets) *n_buckets = cu.on ? cu.nb : 4 + h->dlp.n_cases;
    if (!cu.on) {
        if (episodes || successes || win_n || win_s || prob || pw) return fail(HOPE_ESTATE, "hope_env_curriculum_state: the curriculum is off");
        if (misc) misc[0] = misc[1] = misc[2] = misc[3] = 0;
        return HOPE_OK;
    }
    HOPE_ON_DEVICE(h);
    HIPCHK(hipDeviceSynchronize());
    const size_t nb = (size_t)cu.nb;
    std::vector<uint64_t> e(nb + 1), s(nb + 1);
    HIPCHK(hipMemcpy(e.data(), cu.dev.episodes, (nb + 1) * 8, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(s.data(), cu.dev.successes, (nb + 1) * 8, hipMemcpyDeviceToHost));
    if (episodes) memcpy(episodes, e.data(), nb * 8);
    if (successes) memcpy(successes, s.data(), nb * 8);
    if (win_n) HIPCHK(hipMemcpy(win_n, cu.dev.win_n, nb * 8, hipMemcpyDeviceToHost));
    if (win_s) HIPCHK(hipMemcpy(win_s, cu.dev.win_s, nb * 8, hipMemcpyDeviceToHost));
    if (prob) HIPCHK(hipMemcpy(prob, cu.dev.prob, nb * 8, hipMemcpyDeviceToHost));
    if (pw) HIPCHK(hipMemcpy(pw, cu.dev.pw, 4 * 8, hipMemcpyDeviceToHost));
    if (misc) { misc[0] = cu.updates; misc[1] = e[nb]; misc[2] = s[nb]; misc[3] = 1; }
    return HOPE_OK;
}

int hope_env_curriculum_set_windows(hope_env_t* h, int n_buckets, const double* win_n, const double* win_s, const uint64_t* episodes,
                                    const uint64_t* successes) {
    HOPE_ENTER_AS(h, "hope_env_curriculum_set_windows", "null argument");
    { int rcs = settle_rs(h); if (rcs != HOPE_OK) return rcs; }
    if (!win_n || !win_s || !episodes || !successes) return fail(HOPE_EINVAL, "hope_env_curriculum_set_windows: null argument");
    hope_env::Curriculum& cu = h->cur;
    if (!cu.on) return fail(HOPE_ESTATE, "hope_env_curriculum_set_windows: the curriculum is off (hope_env_curriculum_enable first)");
    if (n_buckets != cu.nb) return fail(HOPE_EINVAL, "hope_env_curriculum_set_windows: " + std::to_string(n_buckets) + " buckets given, the handle has " + std::to_string(cu.nb));
    for (int b = 0; b < n_buckets; b++)
        if (!(win_n[b] >= 0.0) || !(win_s[b] >= 0.0) || win_s[b] > win_n[b] || successes[b] > episodes[b])
            return fail(HOPE_EINVAL, "hope_env_curriculum_set_windows: bucket " + std::to_string(b) + " needs 0 <= s <= n");
    HOPE_ON_DEVICE(h);
    { int rcp = apply_pending_pool(h, true); if (rcp != HOPE_OK) return rcp; }
    HIPCHK(hipDeviceSynchronize());
    const size_t nb = (size_t)cu.nb;
    HIPCHK(hipMemcpy(cu.dev.win_n, win_n, nb * 8, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(cu.dev.win_s, win_s, nb * 8, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(cu.dev.episodes, episodes, nb * 8, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(cu.dev.successes, successes, nb * 8, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(cu.dev.folded_e, episodes, nb * 8, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(cu.dev.folded_s, successes, nb * 8, hipMemcpyHostToDevice));
    int rc = cur_build_lists(h, false, nullptr);
    if (rc != HOPE_OK) return rc;
    HIPCHK(hipDeviceSynchronize());
    return HOPE_OK;
}

int hope_env_curriculum_download_lists(hope_env_t* h, int32_t* list0, int32_t* list1, int32_t* positions) {
    HOPE_ENTER(h, "hope_env_curriculum_download_lists");
    { int rcs = settle_rs(h); if (rcs != HOPE_OK) return rcs; }
    const hope_env::Curriculum& cu = h->cur;
    if (!cu.on || cu.wactive < 0) return fail(HOPE_ESTATE, "hope_env_curriculum_download_lists: the curriculum is off");
    HOPE_ON_DEVICE(h);
    { int rcp = apply_pending_pool(h, true); if (rcp != HOPE_OK) return rcp; }
    HIPCHK(hipDeviceSynchronize());
    int32_t* out[2] = {list0, list1};
    for (int c = 0; c < 2; c++)
        if (out[c] && h->pool_cls_n[c] > 0) HIPCHK(hipMemcpy(out[c], cu.wl[cu.wactive][c], (size_t)CW_LIST_LEN * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (positions) {
        std::vector<int32_t> pf(2 * (CW_MAX_GROUPS + 1));
        HIPCHK(hipMemcpy(pf.data(), cu.prefix[cu.wactive], pf.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
        for (int c = 0; c < 2; c++)
            for (int g = 0; g < cu.nb; g++) positions[c * cu.nb + g] = pf[c * (CW_MAX_GROUPS + 1) + g + 1] - pf[c * (CW_MAX_GROUPS + 1) + g];
    }
    return HOPE_OK;
}

// the identity of what a draw can return: the pool's hash chain and, with the curriculum on, what the applied weighted lists are made
// of (they are a pure function of the groups' entries and positions)
static int effective_generation(hope_env_t* h, uint64_t* generation) {
    *generation = h->pool_generation;
    const hope_env::Curriculum& cu = h->cur;
    if (!cu.on || cu.wactive < 0 || h->pactive < 0) return HOPE_OK;
    HOPE_ON_DEVICE(h);
    HIPCHK(hipStreamSynchronize(h->pool_stream));
    std::vector<int32_t> pf(2 * (CW_MAX_GROUPS + 1));
    HIPCHK(hipMemcpy(pf.data(), cu.prefix[cu.wactive], pf.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    uint64_t c = hash_bytes(0x637572726963ull, pf.data(), pf.size() * sizeof(int32_t));
    c = hash_bytes(c, cu.cls, sizeof(cu.cls));
    const hope_env::PoolSet& ps = h->pset[h->pactive];
    if (ps.lab_kind == 2) c = hash_bytes(c, ps.lab_host.data(), ps.lab_host.size());
    uint64_t g = fold64(h->pool_generation, c);
    *generation = g ? g : 1;
    return HOPE_OK;
}

int hope_curriculum_fold_host(double* n, double* s, double dn, double ds, double window) {
    if (!n || !s || !(window > 0.0)) return fail(HOPE_EINVAL, "hope_curriculum_fold_host: bad argument");
    cw_fold(n, s, dn, ds, window);
    return HOPE_OK;
}

int hope_curriculum_lists_host(const hope_curriculum_params* params, int n_pool, const int32_t* n_obst, const uint8_t* bucket, int n_cases,
                               int max_obstacles, const uint64_t* episodes, const double* win_n, const double* win_s, int32_t* list0,
                               int32_t* list1, double* prob, double* pw, int32_t* positions) {
    if (n_pool < 0 || n_cases < 0 || (n_pool > 0 && !n_obst) || !episodes || !win_n || !win_s || max_obstacles <= 0)
        return fail(HOPE_EINVAL, "hope_curriculum_lists_host: bad argument");
    if (4 + n_cases > CW_MAX_GROUPS) return fail(HOPE_EINVAL, "hope_curriculum_lists_host: more than 250 Dragon-Lake cases");
    if (n_pool + n_cases <= 0) return fail(HOPE_EINVAL, "hope_curriculum_lists_host: nothing to draw from");
    if (n_pool + n_cases > CW_LIST_LEN) return fail(HOPE_EINVAL, "hope_curriculum_lists_host: a draw list longer than HOPE_CURRICULUM_LIST_LEN entries");
    const hope_curriculum_params P = params ? *params : CW_DEFAULTS;
    const int G = 4 + n_cases;
    const bool two = max_obstacles > SMALL_TILE;
    CwClass cls[2] = {};
    std::vector<int32_t> srt[2];
    for (int k = 0; k < n_pool; k++)
        if (bucket && bucket[k] > 2 && bucket[k] != CW_UNLABELLED) return fail(HOPE_EINVAL, "hope_curriculum_lists_host: bucket id out of range (0, 1, 2 or 255)");
    for (int g = 0; g < 4; g++)
        for (int k = 0; k < n_pool; k++) {
            const int b = bucket && bucket[k] < 3 ? bucket[k] : 3;
            if (b != g) continue;
            const int c = two && n_obst[k] > SMALL_TILE ? 1 : 0;
            srt[c].push_back(k); cls[c].cnt[g]++;
        }
    cls[two ? 1 : 0].n_cases = n_cases;
    std::vector<double> pr(G, 0.0), w(G), r(G);
    std::vector<int32_t> f(G), pos(G), prefix(G + 1);
    double pw4[4], q[4];
    cw_type_probs(win_n, win_s, &P, episodes[0] + episodes[1] + episodes[2] + episodes[3], pw4, q);
    for (int t = 0; t < 4; t++) pr[t] = q[t];
    cw_case_fail_phase(win_n, win_s, n_cases, &P, w.data(), 0, 1);
    cw_case_prob_phase(n_cases, &P, episodes[3], w.data(), pr.data(), 0, 1);
    if (prob) memcpy(prob, pr.data(), (size_t)G * 8);
    if (pw) memcpy(pw, pw4, 32);
    int32_t* out[2] = {list0, list1};
    const CwWork k = {w.data(), r.data(), f.data(), pos.data(), prefix.data()};
    for (int c = 0; c < 2; c++) {
        if (cw_n_base(cls[c]) <= 0) { if (positions) for (int g = 0; g < G; g++) positions[c * G + g] = 0; continue; }
        cw_weight_phase(cls[c], G, pr.data(), k, 0, 1);
        cw_remainder_phase(G, k, 0, 1);
        cw_prefix_phase(G, k);
        if (positions) for (int g = 0; g < G; g++) positions[c * G + g] = pos[g];
        if (out[c]) for (int p = 0; p < CW_LIST_LEN; p++) out[c][p] = cw_entry(cls[c], G, prefix.data(), srt[c].data(), p);
    }
    return HOPE_OK;
}

int hope_env_restart(hope_env_t* h, const uint8_t* mask, void* stream) {
    HOPE_ENTER_AS(h, "hope_env_restart", "null argument");
    { DeviceGuard g0(h->device); int rcs = join_rs(h, (hipStream_t)stream); if (rcs != HOPE_OK) return rcs; }
    if (!mask) return fail(HOPE_EINVAL, "hope_env_restart: null argument");
    if (!h->have_scenes) return fail(HOPE_ESTATE, "hope_env_restart: hope_env_set_scenes has not been called");
    HOPE_ON_DEVICE(h);
    hipLaunchKernelGGL(k_restart, dim3((h->n + 255) / 256), dim3(256), 0, (hipStream_t)stream, h->n, mask, h->scene_c,
                       h->state, h->tstep, h->traj, h->traj_len, h->traj_valid);
    HIPCHK(hipGetLastError());
    return HOPE_OK;
}

// HOPE_F_PROFILE: drains the recorded event pairs, then copies (and clears) one pair of per-kernel accumulators
static int profile_read(hope_env_t* h, double* acc_ms, int64_t* acc_n, double* ms, int64_t* counts, int reset) {
    HOPE_ON_DEVICE(h);
    int rc = drain_events(h);
    if (rc) return rc;
    for (int k = 0; k < HOPE_N_KERNELS; k++) {
        if (ms) ms[k] = acc_ms[k];
        if (counts) counts[k] = acc_n[k];
        if (reset) { acc_ms[k] = 0; acc_n[k] = 0; }
    }
    return HOPE_OK;
}

int hope_env_kernel_ms(hope_env_t* h, double* ms, int64_t* launches, int reset) {
    HOPE_ENTER(h, "hope_env_kernel_ms");
    if (!(h->flags & HOPE_F_PROFILE)) return fail(HOPE_ESTATE, "hope_env_kernel_ms: handle was not created with HOPE_F_PROFILE");
    return profile_read(h, h->ms, h->launches, ms, launches, reset);
}

int hope_env_kernel_union_ms(hope_env_t* h, double* ms, int64_t* calls, int reset) {
    HOPE_ENTER(h, "hope_env_kernel_union_ms");
    if (!(h->flags & HOPE_F_PROFILE)) return fail(HOPE_ESTATE, "hope_env_kernel_union_ms: handle was not created with HOPE_F_PROFILE");
    return profile_read(h, h->union_ms, h->union_calls, ms, calls, reset);
}

int hope_env_profile_kernels(hope_env_t* h, uint32_t kernel_mask) {
    HOPE_ENTER(h, "hope_env_profile_kernels");
    if (!(h->flags & HOPE_F_PROFILE)) return fail(HOPE_ESTATE, "hope_env_profile_kernels: handle was not created with HOPE_F_PROFILE");
    h->profile_mask = kernel_mask;
    return HOPE_OK;
}

int hope_env_step(hope_env_t* h, const void* actions, const uint8_t* active, uint32_t stages,
                  const hope_step_out* out, void* stream) {
    HOPE_ENTER_AS(h, "hope_env_step", "null argument");
    return launch_step(h, actions, active, stages, out, stream, 1);
}

// Test hook: the plan the next hope_env_step / hope_env_reset_obs with these stages would enqueue (launch_step's stage rule, then
// plan_step with enqueue_step's arguments; the search as with out->rs_word given).  No HIP call, no state change.
int hope_env_step_plan(hope_env_t* h, uint32_t stages, int has_action, int32_t* out, int cap) {
    HOPE_ENTER(h, "hope_env_step_plan");
    if (!out || cap < 0) return fail(HOPE_EINVAL, "hope_env_step_plan: null argument");
    if (!h->have_scenes) return fail(HOPE_ESTATE, "hope_env_step_plan: hope_env_set_scenes has not been called");
    if (!has_action) stages &= ~HOPE_STAGE_MOTION;
    if (stages & HOPE_STAGE_RS) stages |= HOPE_STAGE_REWARD;
    const StepPlan pl = plan_step(h, stages, (stages & HOPE_STAGE_RS) != 0, (h->flags & HOPE_F_OVERLAP) != 0, has_action ? 1 : 0, step_timing_build());
    long long need = HOPE_STEPPLAN_HEAD;
    for (int i = 0; i < pl.n_chain; i++) need += HOPE_STEPPLAN_CHAIN_HEAD + (pl.chain[i].b - pl.chain[i].a);
    if (need > cap) return fail(HOPE_EINVAL, "hope_env_step_plan: cap is too small: " + std::to_string(need) + " words are needed");
    int32_t* w = out;
    *w++ = (int32_t)need;
    *w++ = (pl.split ? HOPE_STEPPLAN_SPLIT : 0) | (pl.pipe ? HOPE_STEPPLAN_PIPE : 0) | (pl.fuse_kin ? HOPE_STEPPLAN_FUSE_KIN : 0) | (pl.auto_subs ? HOPE_STEPPLAN_AUTO_SUBS : 0);
    *w++ = pl.n_chain;
    for (int i = 0; i < pl.n_chain; i++) {
        const StepPlan::Chain& ch = pl.chain[i];
        *w++ = ch.c; *w++ = ch.tile_cap; *w++ = (int32_t)ch.motion; *w++ = (int32_t)ch.obs_kernel; *w++ = ch.b - ch.a;
        const std::vector<int32_t>& l = h->cls_list_host[ch.c];
        for (int j = ch.a; j < ch.b; j++) *w++ = l[j];
    }
    return HOPE_OK;
}

int hope_env_wait_rs(hope_env_t* h, void* stream) {
    HOPE_ENTER(h, "hope_env_wait_rs");
    HOPE_ON_DEVICE(h);
    return join_rs(h, (hipStream_t)stream);
}

int hope_env_last_step(hope_env_t* h, uint64_t* step) {
    HOPE_ENTER_AS(h, "hope_env_last_step", "null argument");
    if (!step) return fail(HOPE_EINVAL, "hope_env_last_step: null argument");
    *step = h->step_seq;
    return HOPE_OK;
}

int hope_env_wait_rs_step(hope_env_t* h, uint64_t step, void* stream) {
    HOPE_ENTER(h, "hope_env_wait_rs_step");
    if (step == 0 || step > h->step_seq) return fail(HOPE_EINVAL, "hope_env_wait_rs_step: no such step (hope_env_last_step)");
    if (step != h->step_seq)
        return fail(HOPE_ESTATE, "hope_env_wait_rs_step: step " + std::to_string(step) + " is not the last one (" + std::to_string(h->step_seq) +
                                 "): a later hope_env_step / hope_env_reset_obs has replaced its Reeds-Shepp outputs -- wait before enqueuing the next step");
    HOPE_ON_DEVICE(h);
    return join_rs(h, (hipStream_t)stream);
}

int hope_env_download_n_obst(hope_env_t* h, int32_t* n_obst) {
    HOPE_ENTER_AS(h, "hope_env_download_n_obst", "null argument");
    { int rcs = settle_rs(h); if (rcs != HOPE_OK) return rcs; }
    if (!n_obst) return fail(HOPE_EINVAL, "hope_env_download_n_obst: null argument");
    HOPE_ON_DEVICE(h);
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(n_obst, h->n_obst, (size_t)h->n * sizeof(int32_t), hipMemcpyDeviceToHost));
    return HOPE_OK;
}

int hope_env_reset_obs(hope_env_t* h, const uint8_t* active, uint32_t stages, const hope_step_out* out, void* stream) {
    HOPE_ENTER_AS(h, "hope_env_reset_obs", "null argument");
    return launch_step(h, nullptr, active, stages & ~HOPE_STAGE_MOTION, out, stream, 0);
}

int hope_debug_math(int fn, int n, const double* a, const double* b, double* out, void* stream) {
    if (n < 0 || !a || !out) return fail(HOPE_EINVAL, "hope_debug_math: bad argument");
    if (n == 0) return HOPE_OK;
    hipLaunchKernelGGL(k_debug_math, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, fn, n, a, b, out);
    HIPCHK(hipGetLastError());
    return HOPE_OK;
}

int hope_debug_geom(int fn, int n, int n_obst, const double* in, void* out, void* stream) {
    if (n < 0 || !in || !out) return fail(HOPE_EINVAL, "hope_debug_geom: bad argument");
    if (fn < 0 || fn >= DEBUG_GEOM_FNS) return fail(HOPE_EINVAL, "hope_debug_geom: unknown fn " + std::to_string(fn));
    if (fn == 5 && (n_obst < 0 || n_obst > DEBUG_GEOM_MAX_OBST))
        return fail(HOPE_EINVAL, "hope_debug_geom: n_obst " + std::to_string(n_obst) + " outside 0.." + std::to_string(DEBUG_GEOM_MAX_OBST));
    if (n == 0) return HOPE_OK;
    const dim3 g(fn == 5 || fn == 6 ? n : (n + WAVE - 1) / WAVE), b(WAVE);
    hipStream_t s = (hipStream_t)stream;
    switch (fn) {
        case 0: hipLaunchKernelGGL((k_debug_geom<0>), g, b, 0, s, n, n_obst, in, out); break;
        case 1: hipLaunchKernelGGL((k_debug_geom<1>), g, b, 0, s, n, n_obst, in, out); break;
        case 2: hipLaunchKernelGGL((k_debug_geom<2>), g, b, 0, s, n, n_obst, in, out); break;
        case 3: hipLaunchKernelGGL((k_debug_geom<3>), g, b, 0, s, n, n_obst, in, out); break;
        case 4: hipLaunchKernelGGL((k_debug_geom<4>), g, b, 0, s, n, n_obst, in, out); break;
        case 5: hipLaunchKernelGGL((k_debug_geom<5>), g, b, 0, s, n, n_obst, in, out); break;
        case 6: hipLaunchKernelGGL((k_debug_geom<6>), g, b, 0, s, n, n_obst, in, out); break;
        case 7: hipLaunchKernelGGL((k_debug_geom<7>), g, b, 0, s, n, n_obst, in, out); break;
        case 8: hipLaunchKernelGGL((k_debug_geom<8>), g, b, 0, s, n, n_obst, in, out); break;
        default: hipLaunchKernelGGL((k_debug_geom<9>), g, b, 0, s, n, n_obst, in, out); break;
    }
    HIPCHK(hipGetLastError());
    return HOPE_OK;
}

int hope_debug_traffic(int mode, size_t bytes, void* buf, void* stream) {
    if (mode < 0 || mode > 7 || !buf || bytes < 4096) return fail(HOPE_EINVAL, "hope_debug_traffic: bad argument");
    const dim3 g(256 * 32), b(256);
    hipStream_t s = (hipStream_t)stream;
    char* q = (char*)buf;
    double* sink = (double*)buf;
    switch (mode) {
        case 0: hipLaunchKernelGGL((k_traffic_calib<0>), g, b, 0, s, bytes, q, q, sink); break;
        case 1: hipLaunchKernelGGL((k_traffic_calib<1>), g, b, 0, s, bytes, q, q, sink); break;
        case 2: hipLaunchKernelGGL((k_traffic_calib<2>), g, b, 0, s, bytes, q, q, sink); break;
        case 3: hipLaunchKernelGGL((k_traffic_calib<3>), g, b, 0, s, bytes, q, q, sink); break;
        case 4: hipLaunchKernelGGL((k_traffic_calib<4>), g, b, 0, s, bytes, q, q, sink); break;
        case 5: hipLaunchKernelGGL((k_traffic_calib<5>), g, b, 0, s, bytes, q, q, sink); break;
        case 6: hipLaunchKernelGGL((k_traffic_calib<6>), g, b, 0, s, bytes, q, q, sink); break;
        default: hipLaunchKernelGGL((k_traffic_calib<7>), g, b, 0, s, bytes, q, q, sink); break;
    }
    HIPCHK(hipGetLastError());
    return HOPE_OK;
}

int hope_env_download_state(hope_env_t* h, double* pose, int32_t* t, double* accum) {
    HOPE_ENTER(h, "hope_env_download_state");
    { int rcs = settle_rs(h); if (rcs != HOPE_OK) return rcs; }
    HOPE_ON_DEVICE(h);
    HIPCHK(hipDeviceSynchronize());
    std::vector<double> st((size_t)h->n * ST_WORDS);
    HIPCHK(hipMemcpy(st.data(), h->state, st.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (int i = 0; i < h->n; i++) {
        if (pose) { pose[3 * i] = st[4 * (size_t)i]; pose[3 * i + 1] = st[4 * (size_t)i + 1]; pose[3 * i + 2] = st[4 * (size_t)i + 2]; }
        if (accum) accum[i] = st[4 * (size_t)i + 3];
    }
    if (t) HIPCHK(hipMemcpy(t, h->tstep, (size_t)h->n * sizeof(int32_t), hipMemcpyDeviceToHost));
    return HOPE_OK;
}

int hope_env_upload_state(hope_env_t* h, const double* pose, const int32_t* t, const double* accum) {
    HOPE_ENTER(h, "hope_env_upload_state");
    { int rcs = settle_rs(h); if (rcs != HOPE_OK) return rcs; }
    HOPE_ON_DEVICE(h);
    HIPCHK(hipDeviceSynchronize());
    std::vector<double> st((size_t)h->n * ST_WORDS);
    HIPCHK(hipMemcpy(st.data(), h->state, st.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (int i = 0; i < h->n; i++) {
        if (pose) { st[4 * (size_t)i] = pose[3 * i]; st[4 * (size_t)i + 1] = pose[3 * i + 1]; st[4 * (size_t)i + 2] = pose[3 * i + 2]; }
        if (accum) st[4 * (size_t)i + 3] = accum[i];
    }
    HIPCHK(hipMemcpy(h->state, st.data(), st.size() * sizeof(double), hipMemcpyHostToDevice));
    if (t) HIPCHK(hipMemcpy(h->tstep, t, (size_t)h->n * sizeof(int32_t), hipMemcpyHostToDevice));
    return HOPE_OK;
}

}  // extern "C"
