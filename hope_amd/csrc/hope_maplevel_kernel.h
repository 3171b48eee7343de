// hope_maplevel_kernel.h -- k_map_level: the difficulty label of every scene's map on the device, one wavefront per scene.
//
// The wave runs ml_classify of hope_maplevel_core.h -- the source hope_map_level_host compiles -- with MlWaveOps scanning the
// obstacles; every value that steers the control flow is wave-uniform after its reduction, so all 64 lanes take the same path.
// Lane mapping:
//   prepare   lanes stride over the obstacles (o = lane, lane + 64, ...): each loads its ring (64 B) once and writes the ring's
//             distance to the four probe points (mid-points of the dest box's edges) into LDS, dcache[probe][o].
//   nearest   lanes stride over dcache[probe]: per-lane strict `<` in ascending index order, then a 6-step butterfly on
//             (distance, index) where the lower index wins equal distances -- the serial loop's answer whatever the lane count.
//   ring_box  lane = 16 r + 4 i + j takes term (i, j) of ring_ring_distance(ring found[r], dest box): one edge pair for the crossing
//             test and two point-segment distances; min over the 16 lanes of a group (xor 8, 4, 2, 1), crossing by ballot.
//   rectangle the hull and smallest rectangle of the 5 or 9 points run on lane 0 in 64 doubles of LDS (dynamic indices, no scratch).
//   meets     lanes stride over the obstacles against the free rectangle; ballot per 64 obstacles: popcount (detail record) or
//             early out at the first hit.
// A minimum over doubles does not depend on the order, the argmin carries its tie rule, the count is a sum of integers: the
// results equal the serial core's bit for bit.  LDS: 4 x 256 + 64 doubles = 8 704 B per one-wave block.
#pragma once
#include "hope_dev.h"
#include "hope_maplevel_core.h"

namespace hope {

constexpr int ML_CACHE = 256;                                  // obstacles per scene the distance cache holds (HOPE_MAX_OBSTACLES + 1)

struct MlWaveOps {
    const double* tile;      // [n][4][2] of this scene
    int n;
    int lane;
    double* dcache;          // LDS [4][ML_CACHE]
    double* w;               // LDS [ML_WORK_WORDS]

    __device__ __forceinline__ void prepare(const double* px, const double* py) {
        for (int o = lane; o < n; o += WAVE) {
            const MlRing r = ml_load_ring(tile + 8 * (size_t)o);
#pragma unroll
            for (int k = 0; k < 4; k++) dcache[k * ML_CACHE + o] = ml_point_ring(px[k], py[k], r);
        }
        __syncthreads();
    }
    __device__ __forceinline__ int nearest(int k, int s0, int s1, int s2) const {
        double bd = ML_LENGTH / 2;
        int bi = ML_NONE;
        for (int o = lane; o < n; o += WAVE) {
            const double d = dcache[k * ML_CACHE + o];
            if (o != s0 && o != s1 && o != s2 && d < bd) { bd = d; bi = o; }
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const double od = __shfl_xor(bd, off);
            const int oi = __shfl_xor(bi, off);
            if (od < bd || (od == bd && oi < bi)) { bd = od; bi = oi; }
        }
        bi = __builtin_amdgcn_readfirstlane(bi);
        return bi == ML_NONE ? -1 : bi;
    }
    __device__ __forceinline__ void ring_box(const int32_t* found, const MlRing& box, double* dist) const {
        const int r = lane >> 4, i = (lane >> 2) & 3, j = lane & 3;
        const int f = r == 0 ? found[0] : (r == 1 ? found[1] : (r == 2 ? found[2] : found[3]));
        double t = INFINITY;
        bool cross = false;
        if (f >= 0) t = ml_pair_term(ml_load_ring(tile + 8 * (size_t)f), box, i, j, &cross);
#pragma unroll
        for (int off = 8; off >= 1; off >>= 1) {
            const double o = __shfl_xor(t, off);
            if (o < t) t = o;
        }
        const unsigned long long cb = __ballot(cross);
#pragma unroll
        for (int k = 0; k < 4; k++) dist[k] = ((cb >> (16 * k)) & 0xffffull) ? 0.0 : readlane_d(t, 16 * k);
    }
    __device__ __forceinline__ double* work() const { return w; }
    __device__ __forceinline__ bool leader() const { return lane == 0; }
    __device__ __forceinline__ void sync() const { __syncthreads(); }
    __device__ __forceinline__ int meets(const MlRing& rect, int sa, int sb, bool all) const {
        int cnt = 0;
        for (int base = 0; base < n; base += WAVE) {
            const int o = base + lane;
            bool hit = false;
            if (o < n && o != sa && o != sb) hit = ml_poly_meets_ring(rect, ml_load_ring(tile + 8 * (size_t)o));
            cnt += __popcll(__ballot(hit));
            if (!all && cnt) break;
        }
        return cnt;
    }
};

// Scene k: start / dest at start[k * start_stride], dest[k * dest_stride] (x, y, heading: stride 3 for packed arrays, SC_WORDS for
// the handle's constant records), obstacles verts[k][max_obst][4][2] of which n_obst[k] (clamped to [0, max_obst]) are valid.
// active != null: scenes with active[k] == 0 keep level[k] / detail[k].  detail [n][8] may be null.
__global__ __launch_bounds__(WAVE) void k_map_level(int n, int max_obst, const double* __restrict__ start, int start_stride,
                                                    const double* __restrict__ dest, int dest_stride, const double* __restrict__ verts,
                                                    const int32_t* __restrict__ n_obst, const uint8_t* __restrict__ active,
                                                    uint8_t* __restrict__ level, int32_t* __restrict__ detail) {
    __shared__ double dcache[4 * ML_CACHE];
    __shared__ double work[ML_WORK_WORDS];
    const int k = blockIdx.x;
    if (k >= n) return;
    if (active && active[k] == 0) return;
    int no = n_obst[k];
    no = no < 0 ? 0 : (no > max_obst ? max_obst : no);
    no = no > ML_CACHE ? ML_CACHE : no;
    no = __builtin_amdgcn_readfirstlane(no);
    MlWaveOps ops;
    ops.tile = verts + (size_t)k * max_obst * 8;
    ops.n = no;
    ops.lane = threadIdx.x;
    ops.dcache = dcache;
    ops.w = work;
    const double* st = start + (size_t)k * start_stride;
    const double* de = dest + (size_t)k * dest_stride;
    MlDetail D;
    const int lv = ml_classify(ops, st[0], st[1], st[2], de[0], de[1], de[2], no, detail != nullptr, D);
    if (threadIdx.x == 0) {
        level[k] = (uint8_t)lv;
        if (detail) {
            int32_t* d = detail + (size_t)k * ML_DETAIL_WORDS;
            d[0] = D.found[0]; d[1] = D.found[1]; d[2] = D.found[2]; d[3] = D.found[3];
            d[4] = D.branch; d[5] = D.far; d[6] = D.count; d[7] = 0;
        }
    }
}

}  // namespace hope
