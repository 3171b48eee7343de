// hope_optim_kernel.h -- the optimiser block on the device (rule: hope_optim_core.h).  Included by hope_agent.hip only.
//
// k_optim<MODE>   one launch over up to OP_CAP tensors.  The table (OkTable: the entries, the groups' hyper-parameters, tau) travels
//                 as the kernel's argument, 3 288 bytes of the 4 KiB an argument block may hold, so nothing is staged through memory
//                 that a later call could overwrite and nothing about a call outlives its enqueue.  A workgroup of 256 lanes owns one
//                 chunk of OP_CHUNK = 1 024 elements of one tensor: it finds the tensor by a binary search over the entries' first-chunk
//                 numbers -- blockIdx.x against argument words, uniform, on scalar loads.  Where every pointer of the entry is 16-byte
//                 aligned (OK_VEC, float32 only) a lane takes four consecutive elements with 16-byte loads and stores; a lane whose
//                 four would cross the tensor's end, and every lane of an entry that is not so aligned or is float64, goes element by
//                 element at a stride of 256 (coalesced 4- or 8-byte accesses).  No LDS, no scratch, no atomics; a word is read and
//                 written by one lane only.
#pragma once
#include <hip/hip_runtime.h>

#include "hope_optim_core.h"

namespace hope {

constexpr int OK_THREADS = 256;
constexpr uint32_t OK_F64 = 1u, OK_VEC = 2u;           // OkEntry::meta bits; the group index sits above them (meta >> 2)

struct OkEntry {
    void* p;                                           // ADAM: parameter   POLYAK: target
    const void* g;                                     // ADAM: gradient    POLYAK: the current net's tensor
    void* m;                                           // ADAM: exp_avg
    void* v;                                           // ADAM: exp_avg_sq
    uint32_t numel, first, meta, pad;                  // first: the launch's chunk number of the tensor's first chunk
};
struct OkTable {
    hope_optim_group_t group[HOPE_OPTIM_MAX_GROUPS];
    double tau, omt;
    int32_t n, pad;
    OkEntry e[OP_CAP];
};
static_assert(sizeof(OkEntry) == 48 && sizeof(OkTable) == 216 + 48 * OP_CAP && sizeof(OkTable) <= 3584, "the table must leave room in the 4 KiB argument block");

template <int MODE, class T>
__device__ __forceinline__ void ok_one(const OkEntry& E, const hope_optim_group_t& G, double tau, double omt, size_t i) {
    if (MODE == OP_ADAM) {
        T* p = (T*)E.p + i; T* m = (T*)E.m + i; T* v = (T*)E.v + i;
        T pv = *p, mv = *m, vv = *v;
        op_adam(pv, ((const T*)E.g)[i], mv, vv, G);
        *p = pv; *m = mv; *v = vv;
    } else {
        T* t = (T*)E.p + i;
        *t = op_polyak(*t, ((const T*)E.g)[i], tau, omt);
    }
}

template <int MODE>
__global__ __launch_bounds__(OK_THREADS) void k_optim(const OkTable tab) {
    const uint32_t chunk = blockIdx.x;
    int lo = 0, hi = tab.n - 1;                        // the last entry whose first chunk is <= chunk
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (tab.e[mid].first <= chunk) lo = mid; else hi = mid - 1;
    }
    const OkEntry E = tab.e[lo];
    const hope_optim_group_t G = tab.group[MODE == OP_ADAM ? (E.meta >> 2) : 0];
    const double tau = tab.tau, omt = tab.omt;
    const size_t base = (size_t)(chunk - E.first) * OP_CHUNK;
    const size_t numel = E.numel;
    const int tid = threadIdx.x;
    if (E.meta & OK_F64) {
#pragma unroll
        for (int j = 0; j < OP_CHUNK / OK_THREADS; ++j) {
            const size_t i = base + (size_t)(j * OK_THREADS + tid);
            if (i < numel) ok_one<MODE, double>(E, G, tau, omt, i);
        }
        return;
    }
    if (E.meta & OK_VEC) {
        const size_t i = base + 4 * (size_t)tid;
        if (i + 4 <= numel) {
            if (MODE == OP_ADAM) {
                float4 p = *(const float4*)((const float*)E.p + i), m = *(const float4*)((const float*)E.m + i), v = *(const float4*)((const float*)E.v + i);
                const float4 g = *(const float4*)((const float*)E.g + i);
                op_adam(p.x, g.x, m.x, v.x, G);
                op_adam(p.y, g.y, m.y, v.y, G);
                op_adam(p.z, g.z, m.z, v.z, G);
                op_adam(p.w, g.w, m.w, v.w, G);
                *(float4*)((float*)E.p + i) = p;
                *(float4*)((float*)E.m + i) = m;
                *(float4*)((float*)E.v + i) = v;
            } else {
                float4 t = *(const float4*)((const float*)E.p + i);
                const float4 c = *(const float4*)((const float*)E.g + i);
                t.x = op_polyak(t.x, c.x, tau, omt);
                t.y = op_polyak(t.y, c.y, tau, omt);
                t.z = op_polyak(t.z, c.z, tau, omt);
                t.w = op_polyak(t.w, c.w, tau, omt);
                *(float4*)((float*)E.p + i) = t;
            }
        } else {
            for (size_t k = i; k < numel; ++k) ok_one<MODE, float>(E, G, tau, omt, k);       // at most three: the tensor's tail
        }
        return;
    }
#pragma unroll
    for (int j = 0; j < OP_CHUNK / OK_THREADS; ++j) {
        const size_t i = base + (size_t)(j * OK_THREADS + tid);
        if (i < numel) ok_one<MODE, float>(E, G, tau, omt, i);
    }
}

}  // namespace hope
