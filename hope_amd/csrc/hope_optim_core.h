/*
 * hope_optim_core.h -- the optimiser block of an update over many tensors at once, one source for host and device: Adam's step
 * (torch.optim.Adam without amsgrad, weight decay or maximize) and the Polyak average of a target network (agents._soft_update).
 *
 * torch runs either as a chain of multi-tensor launches whose vectorised paths contract and reorder, so its bits cannot be restated.
 * This header pins the block to ONE arithmetic, so that the kernel (hope_optim_kernel.h) and the host twins op_adam_host /
 * op_polyak_host give the same bits whatever the launch geometry: plain IEEE + - * / sqrt in double, contraction off on both
 * compilers (no fused multiply-add anywhere: every product below is rounded to double before the sum that takes it), each stored
 * word rounded to its type once.  Double sqrt and / are correctly rounded on both sides.  NaN and infinity propagate as IEEE gives
 * them; there is no special case.
 *
 * The hyper-parameters of a group arrive as doubles, computed once per group on the host from lr, (beta1, beta2), eps and the step
 * count t >= 1 (hope_optim_group_t):
 *     c1 = 1 - beta1     b2 = beta2     c2 = 1 - beta2     step_size = lr / (1 - beta1^t)     bc2s = sqrt(1 - beta2^t)     eps
 * Per element of a float32 entry (op_adam), f32() the one rounding of a stored word:
 *     m' = f32( m + c1 * (g - m) )
 *     v' = f32( b2 * v + (c2 * g) * g )
 *     p' = f32( p - step_size * ( m' / ( sqrt(v') / bc2s + eps ) ) )          m', v' read back as the stored float32
 * which is torch's single-tensor order (lerp; mul, addcmul; sqrt, div, add; addcdiv) with every intermediate a double.
 * Polyak (op_polyak), omt = 1 - tau computed once on the host:
 *     t' = f32( omt * t + tau * p )
 * A float64 entry (SAC's log_alpha) runs the same expressions and stores the doubles.
 */
#pragma once
#include <stdint.h>

#include "hope_env.h"
#include "hope_math.h"

#define OP_CHUNK HOPE_OPTIM_CHUNK                      /* elements a workgroup owns */
#define OP_CAP HOPE_OPTIM_CAP                          /* entries per launch */

template <class T>
HM_FN void op_adam(T& p, T g, T& m, T& v, const hope_optim_group_t& G) {
    const double gd = (double)g, md = (double)m, vd = (double)v;
    const double dm = gd - md;
    const double cm = G.c1 * dm;
    const T m2 = (T)(md + cm);
    const double bv = G.b2 * vd;
    const double cg = G.c2 * gd;
    const double gg = cg * gd;
    const T v2 = (T)(bv + gg);
    const double root = sqrt((double)v2);
    const double den = root / G.bc2s + G.eps;
    const double quot = (double)m2 / den;
    const double move = G.step_size * quot;
    p = (T)((double)p - move);
    m = m2;
    v = v2;
}

template <class T>
HM_FN T op_polyak(T t, T p, double tau, double omt) {
    const double a = omt * (double)t;
    const double b = tau * (double)p;
    return (T)(a + b);
}

HM_FN bool op_finite(double x) { return fabs(x) <= 1.7976931348623157e308; }       /* false for NaN and +-inf */

/* What a call refuses, before anything is launched or written.  op_check returns HOPE_OK, or HOPE_EINVAL with `bad` filled in:
 * index = the entry (OP_BAD_ENTRY), the group (OP_BAD_GROUP) or nothing (OP_BAD_CALL) the text is about. */
enum { OP_BAD_CALL = 0, OP_BAD_ENTRY = 1, OP_BAD_GROUP = 2 };
struct OpBad { int kind; long long index; const char* what; };
enum { OP_ADAM = 0, OP_POLYAK = 1 };

static inline int op_refuse(OpBad* bad, int kind, long long index, const char* what) {
    if (bad) { bad->kind = kind; bad->index = index; bad->what = what; }
    return HOPE_EINVAL;
}

/* mode OP_ADAM: groups / n_groups are checked, tau is not used; OP_POLYAK: tau is checked, an entry's p (the target) and g (the
 * current net's tensor) must be there, its m, v and group are not looked at. */
static inline int op_check(int mode, const hope_optim_entry_t* e, int64_t n, const hope_optim_group_t* g, int n_groups, double tau, OpBad* bad) {
    if (!e) return op_refuse(bad, OP_BAD_CALL, 0, "null entry table");
    if (n < 1) return op_refuse(bad, OP_BAD_CALL, 0, "n_entries < 1");
    if (mode == OP_ADAM) {
        if (!g) return op_refuse(bad, OP_BAD_CALL, 0, "null group table");
        if (n_groups < 1 || n_groups > HOPE_OPTIM_MAX_GROUPS) return op_refuse(bad, OP_BAD_CALL, 0, "n_groups must be 1 .. 4");
        for (int k = 0; k < n_groups; k++) {
            if (!op_finite(g[k].c1) || !op_finite(g[k].b2) || !op_finite(g[k].c2) || !op_finite(g[k].step_size) || !op_finite(g[k].bc2s) || !op_finite(g[k].eps))
                return op_refuse(bad, OP_BAD_GROUP, k, "a hyper-parameter is not finite");
            if (g[k].eps < 0.0) return op_refuse(bad, OP_BAD_GROUP, k, "eps < 0");
            if (g[k].bc2s <= 0.0) return op_refuse(bad, OP_BAD_GROUP, k, "bc2s <= 0");
        }
    } else if (!(tau >= 0.0 && tau <= 1.0)) {
        return op_refuse(bad, OP_BAD_CALL, 0, "tau must be in [0, 1]");
    }
    int64_t total = 0;
    for (int64_t i = 0; i < n; i++) {
        const bool adam = mode == OP_ADAM;
        if (!e[i].p || !e[i].g || (adam && (!e[i].m || !e[i].v))) return op_refuse(bad, OP_BAD_ENTRY, i, "null pointer");
        if (e[i].dtype != HOPE_OPTIM_F32 && e[i].dtype != HOPE_OPTIM_F64) return op_refuse(bad, OP_BAD_ENTRY, i, "dtype is neither HOPE_OPTIM_F32 nor HOPE_OPTIM_F64");
        if (e[i].numel < 1) return op_refuse(bad, OP_BAD_ENTRY, i, "numel < 1");
        if (e[i].numel > ((int64_t)1 << 31) || (total += e[i].numel) > ((int64_t)1 << 31)) return op_refuse(bad, OP_BAD_ENTRY, i, "more than 2^31 elements in one call");
        const uintptr_t am = e[i].dtype == HOPE_OPTIM_F64 ? 7 : 3;
        uintptr_t bits = (uintptr_t)e[i].p | (uintptr_t)e[i].g;
        if (adam) bits |= (uintptr_t)e[i].m | (uintptr_t)e[i].v;
        if (bits & am) return op_refuse(bad, OP_BAD_ENTRY, i, "a pointer is not aligned to its element");
        if (adam && (e[i].group < 0 || e[i].group >= n_groups)) return op_refuse(bad, OP_BAD_ENTRY, i, "group index out of range");
    }
    return HOPE_OK;
}

/* The host twins (no alignment requirement beyond the element's, which op_check asks of both sides alike). */
template <class T>
static inline void op_adam_entry_host(const hope_optim_entry_t& e, const hope_optim_group_t& G) {
    T* p = (T*)e.p; const T* g = (const T*)e.g; T* m = (T*)e.m; T* v = (T*)e.v;
    for (int64_t i = 0; i < e.numel; i++) op_adam(p[i], g[i], m[i], v[i], G);
}
static inline int op_adam_host(const hope_optim_entry_t* e, int64_t n, const hope_optim_group_t* g, int n_groups, OpBad* bad) {
    const int rc = op_check(OP_ADAM, e, n, g, n_groups, 0.0, bad);
    if (rc != HOPE_OK) return rc;
    for (int64_t i = 0; i < n; i++) {
        if (e[i].dtype == HOPE_OPTIM_F64) op_adam_entry_host<double>(e[i], g[e[i].group]);
        else op_adam_entry_host<float>(e[i], g[e[i].group]);
    }
    return HOPE_OK;
}
static inline int op_polyak_host(const hope_optim_entry_t* e, int64_t n, double tau, OpBad* bad) {
    const int rc = op_check(OP_POLYAK, e, n, nullptr, 0, tau, bad);
    if (rc != HOPE_OK) return rc;
    const double omt = 1.0 - tau;
    for (int64_t i = 0; i < n; i++) {
        if (e[i].dtype == HOPE_OPTIM_F64) {
            double* t = (double*)e[i].p; const double* p = (const double*)e[i].g;
            for (int64_t k = 0; k < e[i].numel; k++) t[k] = op_polyak(t[k], p[k], tau, omt);
        } else {
            float* t = (float*)e[i].p; const float* p = (const float*)e[i].g;
            for (int64_t k = 0; k < e[i].numel; k++) t[k] = op_polyak(t[k], p[k], tau, omt);
        }
    }
    return HOPE_OK;
}
