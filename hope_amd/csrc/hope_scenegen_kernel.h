// hope_scenegen_kernel.h -- k_scenegen: Normal / Complex / Extrem lots drawn on the device, one lane per lot.
//
// The lane runs sg_generate_lot of hope_scenegen_core.h -- the source the host twin hope_scenegen_generate_det compiles -- so the
// lots are the twin's bit for bit.  Attempts of a lot run one after the other on that lot's own random stream (acceptance is 0.63
// .. 0.93 per attempt, at most a handful of attempts per lot), so a wave's time is that of its slowest lane's few attempts.
//
// Ring list of the attempt in flight: SG_MAX_RINGS x 8 doubles per lane in LDS, word-major / lane-minor: word w of ring o of lane
// l at ring_lds[(o * 8 + w) * SG_BLOCK + l].  A wave's 64-bit access then touches 64 consecutive doubles whatever ring each lane
// is at (the ring index moves the address by a multiple of SG_BLOCK * 8 = 512 bytes, two whole 256-byte bank rows), so the two
// 32-lane halves of a ds_read_b64 / the 16-lane groups of a ds_write_b64 are conflict-free by construction, also when lanes have
// diverged to different rings.  Rings are indexed at run time (the count varies), so registers would mean scratch: there is none.
// One wave per block: 17 * 64 * 64 B = 69 632 B of LDS, two blocks per CU next to the step kernels' tiles.
#pragma once
#include "hope_scenegen_core.h"

namespace hope {

constexpr int SG_BLOCK = 64;

// which lots a launch draws: lot k of the launch is lot first_index + (k - off[l]) of (seed[l], level l) for off[l] <= k < off[l + 1]
struct SgJob {
    int off[4];
    uint64_t seed[3];
    int64_t first_index;
    int bay_mode;
};

// Outputs.  verts [n][max_obst][8] (rows beyond n_obst untouched) and n_obst [n] always.  pool_c != null: the pool's constant
// records [n][SC_WORDS] through fill_scene_consts (what k_set_scene_consts writes for an uploaded pool); else start [n][3], dest
// [n][3], bbox [n][4] in the hope_env_set_scenes layout.  case_id [n] may be null.
__global__ __launch_bounds__(SG_BLOCK) void k_scenegen(SgJob job, int max_obst, double* __restrict__ start, double* __restrict__ dest,
                                                       double* __restrict__ bbox, double* __restrict__ verts, int32_t* __restrict__ n_obst,
                                                       int32_t* __restrict__ case_id, double* __restrict__ pool_c) {
    __shared__ double ring_lds[SG_MAX_RINGS * 8 * SG_BLOCK];
    const int k = blockIdx.x * SG_BLOCK + threadIdx.x;
    if (k >= job.off[3]) return;
    const int level = k >= job.off[2] ? 2 : (k >= job.off[1] ? 1 : 0);
    const SgRings R = {ring_lds + threadIdx.x, SG_BLOCK};
    double st[3], de[3], bb[4];
    int cid;
    const int off = level == 2 ? job.off[2] : (level == 1 ? job.off[1] : job.off[0]);
    const uint64_t seed = level == 2 ? job.seed[2] : (level == 1 ? job.seed[1] : job.seed[0]);
    const int nr = sg_generate_lot(level, job.bay_mode, seed, job.first_index + (k - off), R, st, de, bb, &cid);
    double* v = verts + (size_t)k * max_obst * 8;
    for (int o = 0; o < nr; o++) {
        const SgQuad q = sg_get(R, o);
        double* row = v + 8 * o;
#pragma unroll
        for (int c = 0; c < 4; c++) { row[2 * c] = q.x[c]; row[2 * c + 1] = q.y[c]; }
    }
    n_obst[k] = nr;
    if (case_id) case_id[k] = cid;
    if (pool_c) fill_scene_consts(pool_c + (size_t)k * SC_WORDS, st, de, bb);
    else {
        for (int i = 0; i < 3; i++) { start[3 * (size_t)k + i] = st[i]; dest[3 * (size_t)k + i] = de[i]; }
        for (int i = 0; i < 4; i++) bbox[4 * (size_t)k + i] = bb[i];
    }
}


// the class lists of a generated pool: every generated lot holds at most 17 obstacles, i.e. belongs to the small-tile class, so the
// lists do not depend on the lots: entries 0 .. n_pool - 1 in the small class; the Dragon-Lake cases (-2 - case) in the large class,
// or behind the lots when the handle has one class only (build_pool_lists' rule)
__global__ void k_pool_lists_generated(int n_pool, int n_cases, int two, int32_t* list0, int32_t* list1) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n_pool) list0[k] = k;
    else if (k < n_pool + n_cases) {
        const int c = k - n_pool;
        if (two) list1[c] = -2 - c; else list0[k] = -2 - c;
    }
}

}  // namespace hope
