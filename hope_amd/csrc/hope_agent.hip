// hope_agent.hip -- the policy-side features of the C ABI (include/hope_env.h): replay of found Reeds-Shepp paths, masked choice of the
// action, normalisation of the observations, bookkeeping of an evaluation run, PPO's advantage block, the transition ring, PPO's minibatch, SAC's update, the optimiser block -- and their host twins.  They share nothing with the
// step path (hope_env.hip) but the handle (hope_handle.h); their kernels are instantiated here and nowhere else.
#include <hip/hip_runtime.h>

#include <string.h>

#include <string>

#include "hope_handle.h"
#include "hope_planner_kernel.h"
#include "hope_chooser_kernel.h"
#include "hope_obsnorm_kernel.h"
#include "hope_evaltrack_kernel.h"
#include "hope_gae_kernel.h"
#include "hope_ring_kernel.h"
#include "hope_ppo_kernel.h"
#include "hope_sac_kernel.h"
#include "hope_optim_kernel.h"

using namespace hope;

#define PLANNER_ON(h, name) HOPE_NEED((h)->plan.on, name, "the planner is off (hope_env_planner_enable first)")
#define CHOOSER_ON(h, name) HOPE_NEED((h)->choose.on, name, "the chooser is off (hope_env_chooser_enable first)")
#define OBSNORM_ON(h, name) HOPE_NEED((h)->onorm.on, name, "the normalisation is off (hope_env_obsnorm_enable first)")
#define EVAL_ON(h, name) HOPE_NEED((h)->evalt.on, name, "the evaluation tracker is off (hope_env_eval_enable first)")
#define GAE_ON(h, name) HOPE_NEED((h)->gae.on, name, "the advantage block is off (hope_env_gae_enable first)")
#define RING_ON(h, name) HOPE_NEED((h)->ring.on, name, "the transition ring is off (hope_env_ring_enable first)")
#define PPO_ON(h, name) HOPE_NEED((h)->ppo.on, name, "the minibatch is off (hope_env_ppo_enable first)")
#define SAC_ON(h, name) HOPE_NEED((h)->sac.on, name, "the SAC update is off (hope_env_sac_enable first)")

// What every hope_env_*_enable does with a feature's device buffer: allocate it if absent, fill it (from `src`, or with zeros) and
// wait.  On any failure the buffer is freed and *buf is null; the caller then puts the feature's struct back to "off" (*_free).
template <class T>
static int device_buffer(const char* who, T** buf, size_t bytes, const void* src = nullptr) {
    hipError_t e_ = hipSuccess;
    if (!*buf && (e_ = hipMalloc((void**)buf, bytes)) != hipSuccess) {
        *buf = nullptr;
        return fail(HOPE_ENOMEM, std::string(who) + ": " + hipGetErrorString(e_));
    }
    e_ = src ? hipMemcpy(*buf, src, bytes, hipMemcpyHostToDevice) : hipMemset(*buf, 0, bytes);
    if (e_ == hipSuccess) e_ = hipDeviceSynchronize();
    if (e_ == hipSuccess) return HOPE_OK;
    hipFree(*buf);
    *buf = nullptr;
    return fail(HOPE_EHIP, std::string(who) + ": " + hipGetErrorString(e_));
}

// hope_env_*_disable: nothing in flight reads the feature's memory any more, then it goes
static int feature_disable(hope_env_t* h, void (*free_fn)(hope_env_t*)) {
    HOPE_ON_DEVICE(h);
    HIPCHK(hipDeviceSynchronize());
    free_fn(h);
    return HOPE_OK;
}

// the state block of a feature ([words][n] 64-bit words) to the host
static int download_words(hope_env_t* h, const uint64_t* state, int words, void* state_out) {
    HOPE_ON_DEVICE(h);
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(state_out, state, (size_t)words * h->n * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return HOPE_OK;
}

void hope::plan_free(hope_env_t* h) {
    if (h->plan.state) hipFree(h->plan.state);
    h->plan = hope_env::Planner{};
}
void hope::choose_free(hope_env_t* h) {
    if (h->choose.actions) hipFree(h->choose.actions);
    h->choose = hope_env::Chooser{};
}
void hope::onorm_free(hope_env_t* h) {
    if (h->onorm.state) hipFree(h->onorm.state);
    if (h->onorm.part) hipFree(h->onorm.part);
    h->onorm = hope_env::ObsNorm{};
}
void hope::evalt_free(hope_env_t* h) {
    if (h->evalt.state) hipFree(h->evalt.state);
    h->evalt = hope_env::EvalTrack{};
}

void hope::gae_free(hope_env_t* h) {
    if (h->gae.part) hipFree(h->gae.part);
    if (h->gae.sums) hipFree(h->gae.sums);
    h->gae = hope_env::Gae{};
}

void hope::ring_free(hope_env_t* h) {
    if (h->ring.part) hipFree(h->ring.part);
    if (h->ring.cnt) hipFree(h->ring.cnt);
    h->ring = hope_env::Ring{};
}

void hope::ppo_free(hope_env_t* h) {
    if (h->ppo.part) hipFree(h->ppo.part);
    h->ppo = hope_env::Ppo{};
}

void hope::sac_free(hope_env_t* h) {
    if (h->sac.part) hipFree(h->sac.part);
    h->sac = hope_env::Sac{};
}

// the ring descriptor of a hope_env_ring_* call `name`: every tensor there and aligned to its element, n and T in range
#define RING_ARG(h, R, name)                                                                                                                  \
    do {                                                                                                                                      \
        if (!(R)) return fail(HOPE_EINVAL, name ": null ring");                                                                               \
        if (!rg_ring_ok_ptrs(R)) return fail(HOPE_EINVAL, name ": null tensor in the ring");                                                  \
        if (ring_bits(R) & 3) return fail(HOPE_EINVAL, name ": misaligned buffer (the ring's float32 tensors 4 bytes)");                      \
        if ((R)->n < 1 || (R)->n > (h)->n) return fail(HOPE_EINVAL, name ": the ring's n must be 1 .. the handle's scenes");                  \
        if ((R)->T < 1 || (R)->T > HOPE_RING_MAX_T) return fail(HOPE_EINVAL, name ": the ring's T must be 1 .. " + std::to_string(HOPE_RING_MAX_T)); \
    } while (0)
static bool rg_ring_ok_ptrs(const hope_ring_t* R) { return R->lidar && R->target && R->action_mask && R->action && R->log_prob && R->reward && R->done; }
static uintptr_t ring_bits(const hope_ring_t* R) {
    return (uintptr_t)R->lidar | (uintptr_t)R->target | (uintptr_t)R->action_mask | (uintptr_t)R->action | (uintptr_t)R->log_prob | (uintptr_t)R->reward |
           (uintptr_t)R->done;
}

template <class T>
static void onorm_launch(hope_env_t* h, const T* lidar, const T* target, int rows, uint32_t flags, float* out_lidar, float* out_target, hipStream_t st) {
    hope_env::ObsNorm& o = h->onorm;
    if (flags & HOPE_OBSNORM_UPDATE) {
        const int first = o.n_state == 0 ? 1 : 0;
        const long long m = (long long)rows - first, nk = on_chunks(m);      // nk <= stride: rows <= N
        if (nk > 0)
            hipLaunchKernelGGL(k_obsnorm_partial<T>, dim3((unsigned)nk, 2), dim3(64), 0, st, lidar, target, (long long)first, m, o.stride, o.part);
        hipLaunchKernelGGL(k_obsnorm_merge<T>, dim3(ON_NC), dim3(64), 0, st, lidar, target, first, (long long)o.n_state, nk, o.stride, o.part, o.state);
        o.n_state += rows;
    }
    if (flags & HOPE_OBSNORM_NORMALIZE) {
        const size_t total = (size_t)rows * ON_NC;
        hipLaunchKernelGGL(k_obsnorm_apply<T>, dim3((unsigned)((total + 63) / 64)), dim3(64), 0, st, lidar, target, (long long)rows, (const double*)o.state,
                           out_lidar, out_target);
    }
}

extern "C" {

// ---- replay of found Reeds-Shepp paths (include/hope_env.h; kernel: hope_planner_kernel.h, rule: hope_planner_core.h) ----
int hope_env_planner_enable(hope_env_t* h, double step_ratio) {
    HOPE_ENTER(h, "hope_env_planner_enable");
    if (step_ratio != step_ratio || !pl_finite(step_ratio)) return fail(HOPE_EINVAL, "hope_env_planner_enable: step_ratio is not finite");
    HOPE_ON_DEVICE(h);
    HIPCHK(hipDeviceSynchronize());                         // planner steps in flight read the state
    const int rc = device_buffer("hope_env_planner_enable", &h->plan.state, (size_t)PL_WORDS * h->n * sizeof(uint64_t));
    if (rc != HOPE_OK) { plan_free(h); return rc; }
    h->plan.step_ratio = step_ratio > 0.0 ? step_ratio : HOPE_PLAN_STEP_RATIO;
    h->plan.on = true;
    return HOPE_OK;
}

int hope_env_planner_disable(hope_env_t* h) {
    HOPE_ENTER(h, "hope_env_planner_disable");
    return feature_disable(h, plan_free);
}

int hope_env_planner_reset(hope_env_t* h, const uint8_t* mask, void* stream) {
    HOPE_ENTER(h, "hope_env_planner_reset");
    PLANNER_ON(h, "hope_env_planner_reset");
    HOPE_ON_DEVICE(h);
    if (!mask) {
        HIPCHK(hipMemsetAsync(h->plan.state, 0, (size_t)PL_WORDS * h->n * sizeof(uint64_t), (hipStream_t)stream));
        return HOPE_OK;
    }
    hipLaunchKernelGGL(k_plan_reset, dim3((h->n + 63) / 64), dim3(64), 0, (hipStream_t)stream, h->n, mask, h->plan.state);
    HIPCHK(hipGetLastError());
    return HOPE_OK;
}

int hope_env_planner_step(hope_env_t* h, const int8_t* rs_word, const void* rs_lengths, const uint8_t* done, int forced, uint64_t step,
                          double* planned_out, uint8_t* executing_out, void* actions_inout, int action_is_f64, void* stream) {
    HOPE_ENTER(h, "hope_env_planner_step");
    PLANNER_ON(h, "hope_env_planner_step");
    if (!rs_word || !rs_lengths) return fail(HOPE_EINVAL, "hope_env_planner_step: null rs_word / rs_lengths");
    if (forced & ~(HOPE_PLAN_FORCED | HOPE_PLAN_NO_POP)) return fail(HOPE_EINVAL, "hope_env_planner_step: unknown bit in `forced`");
    const bool lf64 = h->flags & HOPE_F_OBS_F64;
    if (((uintptr_t)rs_word & 7) || ((uintptr_t)rs_lengths & (lf64 ? 7 : 3)) || ((uintptr_t)planned_out & 15) ||
        ((uintptr_t)actions_inout & (action_is_f64 ? 15 : 7)))
        return fail(HOPE_EINVAL, "hope_env_planner_step: misaligned buffer (rs_word 8, planned_out 16, actions 8 / 16 bytes)");
    if (step != 0) {                                        // hope_env_wait_rs_step, before anything is touched
        if (step > h->step_seq) return fail(HOPE_EINVAL, "hope_env_planner_step: no such step (hope_env_last_step)");
        if (step != h->step_seq)
            return fail(HOPE_ESTATE, "hope_env_planner_step: step " + std::to_string(step) + " is not the last one (" + std::to_string(h->step_seq) +
                                     "): a later hope_env_step / hope_env_reset_obs has replaced its Reeds-Shepp outputs -- plan before enqueuing the next step");
    }
    HOPE_ON_DEVICE(h);
    if (step != 0) { int rcs = join_rs(h, (hipStream_t)stream); if (rcs != HOPE_OK) return rcs; }
    hipLaunchKernelGGL(k_plan, dim3((h->n + 63) / 64), dim3(64), 0, (hipStream_t)stream, h->n, (const uint64_t*)rs_word, rs_lengths, lf64 ? 1 : 0, done,
                       forced, h->plan.step_ratio, h->plan.state, (double2*)planned_out, executing_out, actions_inout, action_is_f64 ? 1 : 0);
    HIPCHK(hipGetLastError());
    return HOPE_OK;
}

int hope_planner_step_host(int n, double step_ratio, void* state, const int8_t* rs_word, const void* rs_lengths, int lengths_f64,
                           const uint8_t* done, int forced, double* planned_out, uint8_t* executing_out, void* actions_inout, int action_is_f64) {
    if (forced & ~(HOPE_PLAN_FORCED | HOPE_PLAN_NO_POP)) return fail(HOPE_EINVAL, "hope_planner_step_host: unknown bit in `forced`");
    const int rc = pl_step_host(n, step_ratio > 0.0 ? step_ratio : (step_ratio == 0.0 ? HOPE_PLAN_STEP_RATIO : step_ratio), state, rs_word, rs_lengths, lengths_f64,
                                done, forced, planned_out, executing_out, actions_inout, action_is_f64);
    if (rc != HOPE_OK) return fail(rc, "hope_planner_step_host: bad argument (n <= 0, a null state / rs_word / rs_lengths, or a step_ratio that is not positive and finite)");
    return HOPE_OK;
}

int hope_env_planner_download_state(hope_env_t* h, void* state_out) {
    HOPE_ENTER_AS(h, "hope_env_planner_download_state", "null argument");
    if (!state_out) return fail(HOPE_EINVAL, "hope_env_planner_download_state: null argument");
    PLANNER_ON(h, "hope_env_planner_download_state");
    return download_words(h, h->plan.state, PL_WORDS, state_out);
}

// ---- masked choice of the discrete action (include/hope_env.h; kernel: hope_chooser_kernel.h, rule: hope_chooser_core.h) ----
int hope_env_chooser_enable(hope_env_t* h, const double* actions) {
    HOPE_ENTER(h, "hope_env_chooser_enable");
    if (!actions) return fail(HOPE_EINVAL, "hope_env_chooser_enable: null action table");
    if (!ch_table_ok(actions))
        return fail(HOPE_EINVAL, "hope_env_chooser_enable: the action table must be finite, rows 0..20 at one speed and rows 21..41 the same steers at another");
    HOPE_ON_DEVICE(h);
    HIPCHK(hipDeviceSynchronize());                         // choices in flight read the table
    const int rc = device_buffer("hope_env_chooser_enable", &h->choose.actions, (size_t)CH_NA * 2 * sizeof(double), actions);
    if (rc != HOPE_OK) { choose_free(h); return rc; }
    h->choose.on = true;
    return HOPE_OK;
}

int hope_env_chooser_disable(hope_env_t* h) {
    HOPE_ENTER(h, "hope_env_chooser_disable");
    return feature_disable(h, choose_free);
}

int hope_env_choose(hope_env_t* h, const void* mean, const void* log_std, int log_std_row_stride, int in_f64, const void* mask, const double* planned,
                    const uint8_t* executing, const double* u, uint64_t seed, uint64_t counter, void* action, float* action_f32, int32_t* idx,
                    float* log_prob, double* probs, void* stream) {
    HOPE_ENTER(h, "hope_env_choose");
    CHOOSER_ON(h, "hope_env_choose");
    if (!mean || !log_std || !mask || !action) return fail(HOPE_EINVAL, "hope_env_choose: null mean / log_std / mask / action");
    if ((planned != nullptr) != (executing != nullptr)) return fail(HOPE_EINVAL, "hope_env_choose: planned and executing go together");
    if (log_std_row_stride != 0 && log_std_row_stride != 2) return fail(HOPE_EINVAL, "hope_env_choose: log_std_row_stride is 0 (one row for all) or 2");
    const bool mf64 = h->flags & HOPE_F_OBS_F64, af64 = h->flags & HOPE_F_ACTION_F64;
    if (((uintptr_t)mean & (in_f64 ? 15 : 7)) || ((uintptr_t)log_std & (in_f64 ? 7 : 3)) || ((uintptr_t)mask & (mf64 ? 7 : 3)) || ((uintptr_t)planned & 15) ||
        ((uintptr_t)u & 7) || ((uintptr_t)action & (af64 ? 15 : 7)) || ((uintptr_t)action_f32 & 7) || ((uintptr_t)idx & 3) || ((uintptr_t)log_prob & 7) ||
        ((uintptr_t)probs & 7))
        return fail(HOPE_EINVAL, "hope_env_choose: misaligned buffer (mean and action rows 8 / 16, planned 16, action_f32 and log_prob 8 bytes, the others their element)");
    HOPE_ON_DEVICE(h);
    const dim3 grid((h->n + 63) / 64), block(64);
    if (mf64)
        hipLaunchKernelGGL(k_choose<double>, grid, block, 0, (hipStream_t)stream, h->n, (const double*)h->choose.actions, mean, log_std, log_std_row_stride,
                           in_f64 ? 1 : 0, (const double*)mask, (const double2*)planned, executing, u, seed, counter, action, af64 ? 1 : 0, (float2*)action_f32,
                           (int*)idx, (float2*)log_prob, probs);
    else
        hipLaunchKernelGGL(k_choose<float>, grid, block, 0, (hipStream_t)stream, h->n, (const double*)h->choose.actions, mean, log_std, log_std_row_stride,
                           in_f64 ? 1 : 0, (const float*)mask, (const double2*)planned, executing, u, seed, counter, action, af64 ? 1 : 0, (float2*)action_f32,
                           (int*)idx, (float2*)log_prob, probs);
    HIPCHK(hipGetLastError());
    return HOPE_OK;
}

int hope_chooser_host(int n, const double* actions, const void* mean, const void* log_std, int log_std_row_stride, int in_f64, const void* mask, int mask_f64,
                      const double* planned, const uint8_t* executing, const double* u, uint64_t seed, uint64_t counter, uint64_t scene0, void* action,
                      int action_f64, float* action_f32, int32_t* idx, float* log_prob, double* probs) {
    const int rc = ch_host(n, actions, mean, log_std, log_std_row_stride, in_f64, mask, mask_f64, planned, executing, u, seed, counter, scene0, action, action_f64,
                           action_f32, idx, log_prob, probs);
    if (rc != HOPE_OK)
        return fail(rc, "hope_chooser_host: bad argument (n <= 0, a null actions / mean / log_std / mask / action, planned without executing or the reverse, a stride other than 0 / 2, or an action table that is not 21 steers x 2 speeds)");
    return HOPE_OK;
}

// ---- normalisation of the observations (include/hope_env.h; kernels: hope_obsnorm_kernel.h, rule: hope_obsnorm_core.h) ----
int hope_env_obsnorm_enable(hope_env_t* h) {
    HOPE_ENTER(h, "hope_env_obsnorm_enable");
    if (h->onorm.on) return HOPE_OK;
    HOPE_ON_DEVICE(h);
    const long long stride = (h->n + ON_CHUNK - 1) / ON_CHUNK;
    const size_t sbytes = (size_t)3 * ON_NC * sizeof(double);
    int rc = device_buffer("hope_env_obsnorm_enable", &h->onorm.state, sbytes);
    if (rc == HOPE_OK) rc = device_buffer("hope_env_obsnorm_enable", &h->onorm.part, sbytes * (size_t)stride);
    if (rc != HOPE_OK) { onorm_free(h); return rc; }
    h->onorm.stride = stride; h->onorm.n_state = 0; h->onorm.on = true;
    return HOPE_OK;
}

int hope_env_obsnorm_disable(hope_env_t* h) {
    HOPE_ENTER(h, "hope_env_obsnorm_disable");
    return feature_disable(h, onorm_free);
}

int hope_env_obsnorm_set(hope_env_t* h, int64_t n_state, const double* mean, const double* S, const double* std_) {
    HOPE_ENTER(h, "hope_env_obsnorm_set");
    OBSNORM_ON(h, "hope_env_obsnorm_set");
    if (!mean || !S || !std_ || n_state < 0) return fail(HOPE_EINVAL, "hope_env_obsnorm_set: null mean / S / std or a negative n_state");
    HOPE_ON_DEVICE(h);
    HIPCHK(hipDeviceSynchronize());                         // calls in flight read and write the statistics
    const size_t b = (size_t)ON_NC * sizeof(double);
    HIPCHK(hipMemcpy(h->onorm.state, mean, b, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->onorm.state + ON_NC, S, b, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->onorm.state + 2 * ON_NC, std_, b, hipMemcpyHostToDevice));
    HIPCHK(hipDeviceSynchronize());
    h->onorm.n_state = n_state;
    return HOPE_OK;
}

int hope_env_obsnorm_get(hope_env_t* h, int64_t* n_state, double* mean, double* S, double* std_) {
    HOPE_ENTER(h, "hope_env_obsnorm_get");
    OBSNORM_ON(h, "hope_env_obsnorm_get");
    if (n_state) *n_state = h->onorm.n_state;
    if (!mean && !S && !std_) return HOPE_OK;
    HOPE_ON_DEVICE(h);
    HIPCHK(hipDeviceSynchronize());
    const size_t b = (size_t)ON_NC * sizeof(double);
    if (mean) HIPCHK(hipMemcpy(mean, h->onorm.state, b, hipMemcpyDeviceToHost));
    if (S) HIPCHK(hipMemcpy(S, h->onorm.state + ON_NC, b, hipMemcpyDeviceToHost));
    if (std_) HIPCHK(hipMemcpy(std_, h->onorm.state + 2 * ON_NC, b, hipMemcpyDeviceToHost));
    return HOPE_OK;
}

int hope_env_obsnorm(hope_env_t* h, const void* lidar, const void* target, int rows, int in_f64, uint32_t flags, float* out_lidar, float* out_target,
                     void* stream) {
    HOPE_ENTER(h, "hope_env_obsnorm");
    OBSNORM_ON(h, "hope_env_obsnorm");
    if (!lidar || !target) return fail(HOPE_EINVAL, "hope_env_obsnorm: null lidar / target");
    if (rows < 1 || rows > h->n) return fail(HOPE_EINVAL, "hope_env_obsnorm: rows must be 1 .. the handle's scenes");
    if (!(flags & (HOPE_OBSNORM_UPDATE | HOPE_OBSNORM_NORMALIZE)) || (flags & ~(uint32_t)(HOPE_OBSNORM_UPDATE | HOPE_OBSNORM_NORMALIZE)))
        return fail(HOPE_EINVAL, "hope_env_obsnorm: flags are HOPE_OBSNORM_UPDATE | HOPE_OBSNORM_NORMALIZE, at least one");
    const bool norm = flags & HOPE_OBSNORM_NORMALIZE;
    if (norm && (!out_lidar || !out_target)) return fail(HOPE_EINVAL, "hope_env_obsnorm: HOPE_OBSNORM_NORMALIZE needs out_lidar and out_target");
    const uintptr_t am = in_f64 ? 7 : 3;
    if (((uintptr_t)lidar & am) || ((uintptr_t)target & am) || (norm && (((uintptr_t)out_lidar & 3) || ((uintptr_t)out_target & 3))))
        return fail(HOPE_EINVAL, "hope_env_obsnorm: misaligned buffer (each aligned to its element)");
    if ((size_t)rows * ON_NC > (size_t)0x7FFFFFFF * 64) return fail(HOPE_EINVAL, "hope_env_obsnorm: too many rows for one launch");
    HOPE_ON_DEVICE(h);
    if (in_f64) onorm_launch(h, (const double*)lidar, (const double*)target, rows, flags, out_lidar, out_target, (hipStream_t)stream);
    else onorm_launch(h, (const float*)lidar, (const float*)target, rows, flags, out_lidar, out_target, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return HOPE_OK;
}

int hope_obsnorm_host(hope_obsnorm_state* state, const void* lidar, const void* target, int64_t rows, int in_f64, uint32_t flags, float* out_lidar,
                      float* out_target) {
    const int rc = on_host(state, lidar, target, rows, in_f64, flags, out_lidar, out_target);
    if (rc == HOPE_ENOMEM) return fail(rc, "hope_obsnorm_host: out of memory for the chunk partials");
    if (rc != HOPE_OK)
        return fail(rc, "hope_obsnorm_host: bad argument (a null state / lidar / target, rows < 1, a negative n_state, no or an unknown flag, or NORMALIZE without both outputs)");
    return HOPE_OK;
}

// ---- bookkeeping of an evaluation run (include/hope_env.h; kernels: hope_evaltrack_kernel.h, rule: hope_evaltrack_core.h) ----
int hope_env_eval_enable(hope_env_t* h, const double* box) {
    HOPE_ENTER(h, "hope_env_eval_enable");
    if (!et_box_ok(box)) return fail(HOPE_EINVAL, "hope_env_eval_enable: the action box is null or not finite (steer lo, steer hi, speed lo, speed hi)");
    HOPE_ON_DEVICE(h);
    HIPCHK(hipDeviceSynchronize());                         // calls in flight read the box as it was
    if (!h->evalt.state) {                                  // (enabled again while on: the new box, the state as it is)
        const int rc = device_buffer("hope_env_eval_enable", &h->evalt.state, (size_t)ET_WORDS * h->n * sizeof(uint64_t));
        if (rc != HOPE_OK) { evalt_free(h); return rc; }
    }
    h->evalt.box = et_box(box);
    h->evalt.on = true;
    return HOPE_OK;
}

int hope_env_eval_disable(hope_env_t* h) {
    HOPE_ENTER(h, "hope_env_eval_disable");
    return feature_disable(h, evalt_free);
}

int hope_env_eval_begin(hope_env_t* h, const void* target, const double* pose, void* stream) {
    HOPE_ENTER(h, "hope_env_eval_begin");
    EVAL_ON(h, "hope_env_eval_begin");
    if (!target || !pose) return fail(HOPE_EINVAL, "hope_env_eval_begin: null target / pose");
    const bool of64 = h->flags & HOPE_F_OBS_F64;
    if (((uintptr_t)target & (of64 ? 7 : 3)) || ((uintptr_t)pose & 7)) return fail(HOPE_EINVAL, "hope_env_eval_begin: misaligned buffer (each aligned to its element)");
    HOPE_ON_DEVICE(h);
    const dim3 grid((h->n + 63) / 64), block(64);
    if (of64) hipLaunchKernelGGL(k_eval_begin<double>, grid, block, 0, (hipStream_t)stream, h->n, (const double*)target, pose, h->evalt.state);
    else hipLaunchKernelGGL(k_eval_begin<float>, grid, block, 0, (hipStream_t)stream, h->n, (const float*)target, pose, h->evalt.state);
    HIPCHK(hipGetLastError());
    return HOPE_OK;
}

int hope_env_eval_override(hope_env_t* h, void* actions_inout, int action_is_f64, const double* u, uint64_t seed, uint64_t counter, uint8_t* active_out,
                           void* stream) {
    HOPE_ENTER(h, "hope_env_eval_override");
    EVAL_ON(h, "hope_env_eval_override");
    if (!actions_inout || !active_out) return fail(HOPE_EINVAL, "hope_env_eval_override: null actions / active_out");
    if (((uintptr_t)actions_inout & (action_is_f64 ? 15 : 7)) || ((uintptr_t)u & 7))
        return fail(HOPE_EINVAL, "hope_env_eval_override: misaligned buffer (actions 8 / 16 bytes, u 8 bytes)");
    HOPE_ON_DEVICE(h);
    hipLaunchKernelGGL(k_eval_override, dim3((h->n + 63) / 64), dim3(64), 0, (hipStream_t)stream, h->n, (const uint64_t*)h->evalt.state, h->evalt.box,
                       actions_inout, action_is_f64 ? 1 : 0, u, seed, counter, active_out);
    HIPCHK(hipGetLastError());
    return HOPE_OK;
}

int hope_env_eval_track(hope_env_t* h, const void* target, const double* pose, const void* reward, const int32_t* status, const uint8_t* done,
                        const int8_t* rs_word, int8_t* word_out, uint8_t* done_out, void* stream) {
    HOPE_ENTER(h, "hope_env_eval_track");
    EVAL_ON(h, "hope_env_eval_track");
    if (!target || !pose || !reward || !status || !done || !rs_word || !word_out || !done_out)
        return fail(HOPE_EINVAL, "hope_env_eval_track: null target / pose / reward / status / done / rs_word / word_out / done_out");
    const bool of64 = h->flags & HOPE_F_OBS_F64;
    const uintptr_t om = of64 ? 7 : 3;
    if (((uintptr_t)target & om) || ((uintptr_t)reward & om) || ((uintptr_t)pose & 7) || ((uintptr_t)status & 3) || ((uintptr_t)rs_word & 7) ||
        ((uintptr_t)word_out & 7))
        return fail(HOPE_EINVAL, "hope_env_eval_track: misaligned buffer (rs_word and word_out 8 bytes, the others their element)");
    HOPE_ON_DEVICE(h);
    const dim3 grid((h->n + 63) / 64), block(64);
    if (of64)
        hipLaunchKernelGGL(k_eval_track<double>, grid, block, 0, (hipStream_t)stream, h->n, (const double*)target, pose, (const double*)reward, status, done,
                           (const uint64_t*)rs_word, h->evalt.state, (uint64_t*)word_out, done_out);
    else
        hipLaunchKernelGGL(k_eval_track<float>, grid, block, 0, (hipStream_t)stream, h->n, (const float*)target, pose, (const float*)reward, status, done,
                           (const uint64_t*)rs_word, h->evalt.state, (uint64_t*)word_out, done_out);
    HIPCHK(hipGetLastError());
    return HOPE_OK;
}

int hope_env_eval_records(hope_env_t* h, float* rec_out, void* stream) {
    HOPE_ENTER(h, "hope_env_eval_records");
    EVAL_ON(h, "hope_env_eval_records");
    if (!rec_out) return fail(HOPE_EINVAL, "hope_env_eval_records: null rec_out");
    if ((uintptr_t)rec_out & 15) return fail(HOPE_EINVAL, "hope_env_eval_records: misaligned buffer (rec_out 16 bytes)");
    HOPE_ON_DEVICE(h);
    hipLaunchKernelGGL(k_eval_records, dim3((h->n + 63) / 64), dim3(64), 0, (hipStream_t)stream, h->n, (const uint64_t*)h->evalt.state, (float4*)rec_out);
    HIPCHK(hipGetLastError());
    return HOPE_OK;
}

int hope_env_eval_download_state(hope_env_t* h, void* state_out) {
    HOPE_ENTER_AS(h, "hope_env_eval_download_state", "null argument");
    if (!state_out) return fail(HOPE_EINVAL, "hope_env_eval_download_state: null argument");
    EVAL_ON(h, "hope_env_eval_download_state");
    return download_words(h, h->evalt.state, ET_WORDS, state_out);
}

int hope_eval_begin_host(int64_t n, int64_t state_stride, void* state, const void* target, int obs_f64, const double* pose) {
    const int rc = et_begin_host(n, state_stride, state, target, obs_f64, pose);
    if (rc != HOPE_OK) return fail(rc, "hope_eval_begin_host: bad argument (n <= 0, state_stride < n, or a null state / target / pose)");
    return HOPE_OK;
}

int hope_eval_override_host(int64_t n, int64_t state_stride, const void* state, const double* box, void* actions_inout, int action_is_f64, const double* u,
                            uint64_t seed, uint64_t counter, uint64_t scene0, uint8_t* active_out) {
    const int rc = et_override_host(n, state_stride, state, box, actions_inout, action_is_f64, u, seed, counter, scene0, active_out);
    if (rc != HOPE_OK)
        return fail(rc, "hope_eval_override_host: bad argument (n <= 0, state_stride < n, a null state / actions / active_out, or a box that is null or not finite)");
    return HOPE_OK;
}

int hope_eval_track_host(int64_t n, int64_t state_stride, void* state, const void* target, int obs_f64, const double* pose, const void* reward,
                         const int32_t* status, const uint8_t* done, const int8_t* rs_word, int8_t* word_out, uint8_t* done_out) {
    const int rc = et_track_host(n, state_stride, state, target, obs_f64, pose, reward, status, done, rs_word, word_out, done_out);
    if (rc != HOPE_OK)
        return fail(rc, "hope_eval_track_host: bad argument (n <= 0, state_stride < n, or a null state / target / pose / reward / status / done / rs_word / word_out / done_out)");
    return HOPE_OK;
}

// ---- PPO's advantage block (include/hope_env.h; kernels: hope_gae_kernel.h, rule: hope_gae_core.h) ----
int hope_env_gae_enable(hope_env_t* h) {
    HOPE_ENTER(h, "hope_env_gae_enable");
    if (h->gae.on) return HOPE_OK;
    HOPE_ON_DEVICE(h);
    int rc = device_buffer("hope_env_gae_enable", &h->gae.part, (size_t)2 * (size_t)ga_chunks(h->n) * sizeof(double));
    if (rc == HOPE_OK) rc = device_buffer("hope_env_gae_enable", &h->gae.sums, 3 * sizeof(double));
    if (rc != HOPE_OK) { gae_free(h); return rc; }
    h->gae.on = true;
    return HOPE_OK;
}

int hope_env_gae_disable(hope_env_t* h) {
    HOPE_ENTER(h, "hope_env_gae_disable");
    return feature_disable(h, gae_free);
}

int hope_env_gae(hope_env_t* h, const float* reward, const float* done, const float* value, const float* v_last, const float* value_target, int rows, int T,
                 double gamma, double lam, uint32_t flags, float* adv, float* v_target, double* sums, void* stream) {
    HOPE_ENTER(h, "hope_env_gae");
    GAE_ON(h, "hope_env_gae");
    if (!reward || !done || !value || !v_last || !value_target || !adv || !v_target)
        return fail(HOPE_EINVAL, "hope_env_gae: null reward / done / value / v_last / value_target / adv / v_target");
    if (rows < 1 || rows > h->n) return fail(HOPE_EINVAL, "hope_env_gae: rows must be 1 .. the handle's scenes");
    if (T < 1 || T > HOPE_GAE_MAX_T) return fail(HOPE_EINVAL, "hope_env_gae: T must be 1 .. " + std::to_string(HOPE_GAE_MAX_T));
    if (flags & ~(uint32_t)(HOPE_GAE_SUMS | HOPE_GAE_NORMALIZE)) return fail(HOPE_EINVAL, "hope_env_gae: flags are HOPE_GAE_SUMS | HOPE_GAE_NORMALIZE");
    if (!ga_finite(gamma) || !ga_finite(lam)) return fail(HOPE_EINVAL, "hope_env_gae: gamma / lam is not finite");
    const uintptr_t all = (uintptr_t)reward | (uintptr_t)done | (uintptr_t)value | (uintptr_t)value_target | (uintptr_t)adv | (uintptr_t)v_target;
    if ((all & 3) || ((uintptr_t)v_last & 3) || ((uintptr_t)sums & 7))
        return fail(HOPE_EINVAL, "hope_env_gae: misaligned buffer (float32 tensors 4 bytes, sums 8 bytes)");
    HOPE_ON_DEVICE(h);
    const bool want_sums = flags & (HOPE_GAE_SUMS | HOPE_GAE_NORMALIZE);
    const long long nk = ga_chunks(rows);                         // <= the partials' room: rows <= N
    double* part = want_sums ? h->gae.part : nullptr;
    double* s = sums ? sums : h->gae.sums;
    const dim3 grid((unsigned)nk), block(64);
    if (T % 4 == 0 && !(all & 15))
        hipLaunchKernelGGL(k_gae_scan<4>, grid, block, 0, (hipStream_t)stream, reward, done, value, v_last, value_target, rows, T, gamma, lam, adv, v_target, nk,
                           part);
    else
        hipLaunchKernelGGL(k_gae_scan<1>, grid, block, 0, (hipStream_t)stream, reward, done, value, v_last, value_target, rows, T, gamma, lam, adv, v_target, nk,
                           part);
    const long long count = (long long)rows * T;
    if (want_sums) hipLaunchKernelGGL(k_gae_merge, dim3(1), block, 0, (hipStream_t)stream, nk, (double)count, part, s);
    if (flags & HOPE_GAE_NORMALIZE)
        hipLaunchKernelGGL(k_adv_apply, dim3((unsigned)((count + 63) / 64)), block, 0, (hipStream_t)stream, (const float*)adv, count, (const double*)s, adv);
    HIPCHK(hipGetLastError());
    return HOPE_OK;
}

int hope_env_adv_normalize(hope_env_t* h, const float* adv, int64_t count, const double* sums, float* out, void* stream) {
    HOPE_ENTER(h, "hope_env_adv_normalize");
    GAE_ON(h, "hope_env_adv_normalize");
    if (!adv || !out) return fail(HOPE_EINVAL, "hope_env_adv_normalize: null adv / out");
    if (count < 1 || count > (int64_t)h->n * HOPE_GAE_MAX_T) return fail(HOPE_EINVAL, "hope_env_adv_normalize: count must be 1 .. the handle's scenes x " + std::to_string(HOPE_GAE_MAX_T));
    if (((uintptr_t)adv & 3) || ((uintptr_t)out & 3) || ((uintptr_t)sums & 7))
        return fail(HOPE_EINVAL, "hope_env_adv_normalize: misaligned buffer (adv and out 4 bytes, sums 8 bytes)");
    HOPE_ON_DEVICE(h);
    hipLaunchKernelGGL(k_adv_apply, dim3((unsigned)((count + 63) / 64)), dim3(64), 0, (hipStream_t)stream, adv, (long long)count,
                       sums ? sums : (const double*)h->gae.sums, out);
    HIPCHK(hipGetLastError());
    return HOPE_OK;
}

int hope_gae_host(const float* reward, const float* done, const float* value, const float* v_last, const float* value_target, int64_t rows, int64_t T,
                  double gamma, double lam, uint32_t flags, float* adv, float* v_target, double* sums, float* delta) {
    const int rc = ga_host(reward, done, value, v_last, value_target, rows, T, gamma, lam, flags, adv, v_target, sums, delta);
    if (rc == HOPE_ENOMEM) return fail(rc, "hope_gae_host: out of memory for the chunk partials");
    if (rc != HOPE_OK)
        return fail(rc, "hope_gae_host: bad argument (a null reward / done / value / v_last / value_target / adv / v_target, rows or T < 1, an unknown flag, or a gamma / lam that is not finite)");
    return HOPE_OK;
}

int hope_adv_normalize_host(const float* adv, int64_t count, const double* sums, float* out, float* mean_std) {
    const int rc = ga_normalize_host(adv, count, sums, out, mean_std);
    if (rc != HOPE_OK) return fail(rc, "hope_adv_normalize_host: bad argument (null sums, a negative count, or a null adv / out with count > 0)");
    return HOPE_OK;
}

// ---- the transition ring (include/hope_env.h; kernels: hope_ring_kernel.h, rule: hope_ring_core.h) ----
int hope_env_ring_enable(hope_env_t* h) {
    HOPE_ENTER(h, "hope_env_ring_enable");
    if (h->ring.on) return HOPE_OK;
    HOPE_ON_DEVICE(h);
    const size_t nk = (size_t)ga_chunks(h->n);
    int rc = device_buffer("hope_env_ring_enable", &h->ring.part, nk * sizeof(double));
    if (rc == HOPE_OK) rc = device_buffer("hope_env_ring_enable", &h->ring.cnt, nk * 2 * sizeof(int32_t));
    if (rc != HOPE_OK) { ring_free(h); return rc; }
    h->ring.on = true;
    return HOPE_OK;
}

int hope_env_ring_disable(hope_env_t* h) {
    HOPE_ENTER(h, "hope_env_ring_disable");
    return feature_disable(h, ring_free);
}

int hope_env_ring_before(hope_env_t* h, const hope_ring_t* ring, int t, const float* lidar, const float* target, const float* mask, const float* action,
                         const float* log_prob, void* stream) {
    HOPE_ENTER(h, "hope_env_ring_before");
    RING_ON(h, "hope_env_ring_before");
    RING_ARG(h, ring, "hope_env_ring_before");
    if (t < 0 || t >= ring->T) return fail(HOPE_EINVAL, "hope_env_ring_before: t must be 0 .. T - 1");
    if (!lidar || !target || !mask || !action || !log_prob) return fail(HOPE_EINVAL, "hope_env_ring_before: null lidar / target / mask / action / log_prob");
    const uintptr_t in = (uintptr_t)lidar | (uintptr_t)target | (uintptr_t)mask | (uintptr_t)action | (uintptr_t)log_prob;
    if (in & 3) return fail(HOPE_EINVAL, "hope_env_ring_before: misaligned buffer (float32 tensors 4 bytes)");
    HOPE_ON_DEVICE(h);
    const uintptr_t a16 = (uintptr_t)lidar | (uintptr_t)ring->lidar;
    const uintptr_t a8 = (uintptr_t)mask | (uintptr_t)action | (uintptr_t)log_prob | (uintptr_t)ring->action_mask | (uintptr_t)ring->action | (uintptr_t)ring->log_prob;
    const dim3 grid((unsigned)((ring->n + RB_SCENES - 1) / RB_SCENES)), block(64);
    if (!(a16 & 15) && !(a8 & 7)) hipLaunchKernelGGL(k_ring_before<4>, grid, block, 0, (hipStream_t)stream, *ring, t, lidar, target, mask, action, log_prob);
    else hipLaunchKernelGGL(k_ring_before<1>, grid, block, 0, (hipStream_t)stream, *ring, t, lidar, target, mask, action, log_prob);
    HIPCHK(hipGetLastError());
    return HOPE_OK;
}

int hope_env_ring_after(hope_env_t* h, const hope_ring_t* ring, int t, const void* reward, int reward_f64, const uint8_t* done, const int32_t* status,
                        int64_t* counts, double* reward_sum, void* stream) {
    HOPE_ENTER(h, "hope_env_ring_after");
    RING_ON(h, "hope_env_ring_after");
    RING_ARG(h, ring, "hope_env_ring_after");
    if (t < 0 || t >= ring->T) return fail(HOPE_EINVAL, "hope_env_ring_after: t must be 0 .. T - 1");
    if (!reward || !done) return fail(HOPE_EINVAL, "hope_env_ring_after: null reward / done");
    const bool tally = status || counts || reward_sum;
    if (tally && (!status || !counts || !reward_sum)) return fail(HOPE_EINVAL, "hope_env_ring_after: status, counts and reward_sum go together");
    if (((uintptr_t)reward & (reward_f64 ? 7 : 3)) || ((uintptr_t)status & 3) || ((uintptr_t)counts & 7) || ((uintptr_t)reward_sum & 7))
        return fail(HOPE_EINVAL, "hope_env_ring_after: misaligned buffer (reward and status their element, counts and reward_sum 8 bytes)");
    HOPE_ON_DEVICE(h);
    const long long nk = ga_chunks(ring->n);                      // <= the partials' room: n <= N
    hipLaunchKernelGGL(k_ring_after, dim3((unsigned)nk), dim3(64), 0, (hipStream_t)stream, *ring, t, reward, reward_f64 ? 1 : 0, done, status, nk,
                       tally ? h->ring.part : nullptr, tally ? h->ring.cnt : nullptr);
    if (tally)
        hipLaunchKernelGGL(k_ring_tally, dim3(1), dim3(64), 0, (hipStream_t)stream, nk, h->ring.part, (const int32_t*)h->ring.cnt, (long long*)counts, reward_sum);
    HIPCHK(hipGetLastError());
    return HOPE_OK;
}

int hope_env_ring_sample(hope_env_t* h, const hope_ring_t* ring, int head, int size, int batch, const int32_t* s, const int32_t* j, uint64_t seed,
                         uint64_t counter, const float* last_lidar, const float* last_target, const float* last_mask, const hope_ring_batch_t* out, void* stream) {
    HOPE_ENTER(h, "hope_env_ring_sample");
    RING_ON(h, "hope_env_ring_sample");
    RING_ARG(h, ring, "hope_env_ring_sample");
    if (head < 0 || head >= ring->T) return fail(HOPE_EINVAL, "hope_env_ring_sample: head must be 0 .. T - 1");
    if (size < 1 || size > ring->T) return fail(HOPE_EINVAL, "hope_env_ring_sample: size must be 1 .. T");
    if (batch < 1 || batch > HOPE_RING_MAX_BATCH) return fail(HOPE_EINVAL, "hope_env_ring_sample: batch must be 1 .. " + std::to_string(HOPE_RING_MAX_BATCH));
    if ((s != nullptr) != (j != nullptr)) return fail(HOPE_EINVAL, "hope_env_ring_sample: s and j go together");
    if (!last_lidar || !last_target || !last_mask) return fail(HOPE_EINVAL, "hope_env_ring_sample: null last_lidar / last_target / last_mask");
    if (!out) return fail(HOPE_EINVAL, "hope_env_ring_sample: null out");
    if (!rg_batch_ok(out)) return fail(HOPE_EINVAL, "hope_env_ring_sample: null tensor in out");
    const uintptr_t all = (uintptr_t)s | (uintptr_t)j | (uintptr_t)last_lidar | (uintptr_t)last_target | (uintptr_t)last_mask | (uintptr_t)out->obs_lidar |
                          (uintptr_t)out->obs_target | (uintptr_t)out->obs_mask | (uintptr_t)out->next_lidar | (uintptr_t)out->next_target |
                          (uintptr_t)out->next_mask | (uintptr_t)out->action | (uintptr_t)out->reward | (uintptr_t)out->done | (uintptr_t)out->idx;
    if (all & 3) return fail(HOPE_EINVAL, "hope_env_ring_sample: misaligned buffer (every tensor 4 bytes)");
    HOPE_ON_DEVICE(h);
    hipLaunchKernelGGL(k_ring_sample, dim3((unsigned)batch), dim3(64), 0, (hipStream_t)stream, *ring, head, size, s, j, (unsigned long long)seed,
                       (unsigned long long)counter, last_lidar, last_target, last_mask, *out);
    HIPCHK(hipGetLastError());
    return HOPE_OK;
}

int hope_ring_before_host(const hope_ring_t* ring, int t, const float* lidar, const float* target, const float* mask, const float* action,
                          const float* log_prob) {
    const int rc = rg_before_host(ring, t, lidar, target, mask, action, log_prob);
    if (rc != HOPE_OK)
        return fail(rc, "hope_ring_before_host: bad argument (a null ring, tensor or input, n or T < 1, or t outside 0 .. T - 1)");
    return HOPE_OK;
}

int hope_ring_after_host(const hope_ring_t* ring, int t, const void* reward, int reward_f64, const uint8_t* done, const int32_t* status, int64_t* counts,
                         double* reward_sum) {
    const int rc = rg_after_host(ring, t, reward, reward_f64, done, status, counts, reward_sum);
    if (rc == HOPE_ENOMEM) return fail(rc, "hope_ring_after_host: out of memory for the chunk partials");
    if (rc != HOPE_OK)
        return fail(rc, "hope_ring_after_host: bad argument (a null ring, tensor, reward or done, n or T < 1, t outside 0 .. T - 1, or status / counts / reward_sum not together)");
    return HOPE_OK;
}

int hope_ring_sample_host(const hope_ring_t* ring, int head, int size, int64_t batch, const int32_t* s, const int32_t* j, uint64_t seed, uint64_t counter,
                          const float* last_lidar, const float* last_target, const float* last_mask, const hope_ring_batch_t* out) {
    const int rc = rg_sample_host(ring, head, size, batch, s, j, seed, counter, last_lidar, last_target, last_mask, out);
    if (rc != HOPE_OK)
        return fail(rc, "hope_ring_sample_host: bad argument (a null ring, tensor, last_* or out, n or T < 1, head outside 0 .. T - 1, size outside 1 .. T, batch < 1, or s without j or the reverse)");
    return HOPE_OK;
}

// ---- PPO's minibatch (include/hope_env.h; kernels: hope_ppo_kernel.h, rule: hope_ppo_core.h) ----
int hope_env_ppo_enable(hope_env_t* h, int max_batch) {
    HOPE_ENTER(h, "hope_env_ppo_enable");
    if (max_batch < 1 || max_batch > HOPE_PPO_MAX_BATCH) return fail(HOPE_EINVAL, "hope_env_ppo_enable: max_batch must be 1 .. " + std::to_string(HOPE_PPO_MAX_BATCH));
    if (h->ppo.on && max_batch <= h->ppo.max_batch) return HOPE_OK;
    HOPE_ON_DEVICE(h);
    HIPCHK(hipDeviceSynchronize());                         // loss calls in flight use the partials that a larger max_batch replaces
    ppo_free(h);
    const int rc = device_buffer("hope_env_ppo_enable", &h->ppo.part, (size_t)PB_SUMS * (size_t)pb_chunks(max_batch) * sizeof(double));
    if (rc != HOPE_OK) { ppo_free(h); return rc; }
    h->ppo.max_batch = max_batch;
    h->ppo.on = true;
    return HOPE_OK;
}

int hope_env_ppo_disable(hope_env_t* h) {
    HOPE_ENTER(h, "hope_env_ppo_disable");
    return feature_disable(h, ppo_free);
}

int hope_env_ppo_gather(hope_env_t* h, const hope_ring_t* ring, const float* adv, const float* v_target, const int64_t* index, int batch,
                        const hope_ppo_batch_t* out, void* stream) {
    HOPE_ENTER(h, "hope_env_ppo_gather");
    PPO_ON(h, "hope_env_ppo_gather");
    RING_ARG(h, ring, "hope_env_ppo_gather");
    if (!adv || !v_target || !index) return fail(HOPE_EINVAL, "hope_env_ppo_gather: null adv / v_target / index");
    if (batch < 1 || batch > h->ppo.max_batch) return fail(HOPE_EINVAL, "hope_env_ppo_gather: batch must be 1 .. max_batch (" + std::to_string(h->ppo.max_batch) + ")");
    if (!out) return fail(HOPE_EINVAL, "hope_env_ppo_gather: null out");
    if (!pb_batch_ok(out)) return fail(HOPE_EINVAL, "hope_env_ppo_gather: null tensor in out");
    const uintptr_t all = (uintptr_t)adv | (uintptr_t)v_target | (uintptr_t)out->lidar | (uintptr_t)out->target | (uintptr_t)out->mask | (uintptr_t)out->action |
                          (uintptr_t)out->old_lp | (uintptr_t)out->adv | (uintptr_t)out->v_target | (uintptr_t)out->idx;
    if ((all & 3) || ((uintptr_t)index & 7)) return fail(HOPE_EINVAL, "hope_env_ppo_gather: misaligned buffer (index 8 bytes, every other tensor 4)");
    HOPE_ON_DEVICE(h);
    const uintptr_t a16 = (uintptr_t)ring->lidar | (uintptr_t)out->lidar;
    const uintptr_t a8 = (uintptr_t)ring->action_mask | (uintptr_t)ring->action | (uintptr_t)ring->log_prob | (uintptr_t)out->mask | (uintptr_t)out->action;
    const dim3 grid((unsigned)batch), block(64);
    if (!(a16 & 15) && !(a8 & 7)) hipLaunchKernelGGL(k_ppo_gather<4>, grid, block, 0, (hipStream_t)stream, *ring, adv, v_target, index, *out);
    else hipLaunchKernelGGL(k_ppo_gather<1>, grid, block, 0, (hipStream_t)stream, *ring, adv, v_target, index, *out);
    HIPCHK(hipGetLastError());
    return HOPE_OK;
}

int hope_env_ppo_loss(hope_env_t* h, const float* raw, const float* log_std, const float* value, const hope_ppo_batch_t* batch, int mb, double clip,
                      float* g_raw, float* g_log_std, float* g_value, float* losses, void* stream) {
    HOPE_ENTER(h, "hope_env_ppo_loss");
    PPO_ON(h, "hope_env_ppo_loss");
    if (!raw || !log_std || !value || !g_raw || !g_log_std || !g_value || !losses)
        return fail(HOPE_EINVAL, "hope_env_ppo_loss: null raw / log_std / value / g_raw / g_log_std / g_value / losses");
    if (!batch) return fail(HOPE_EINVAL, "hope_env_ppo_loss: null batch");
    if (!batch->action || !batch->old_lp || !batch->adv || !batch->v_target) return fail(HOPE_EINVAL, "hope_env_ppo_loss: null tensor in batch (action / old_lp / adv / v_target)");
    if (mb < 1 || mb > h->ppo.max_batch) return fail(HOPE_EINVAL, "hope_env_ppo_loss: mb must be 1 .. max_batch (" + std::to_string(h->ppo.max_batch) + ")");
    if (!pb_clip_ok(clip)) return fail(HOPE_EINVAL, "hope_env_ppo_loss: clip must be finite and >= 0");
    const uintptr_t pair = (uintptr_t)raw | (uintptr_t)batch->action | (uintptr_t)g_raw;
    const uintptr_t all = pair | (uintptr_t)log_std | (uintptr_t)value | (uintptr_t)batch->old_lp | (uintptr_t)batch->adv | (uintptr_t)batch->v_target |
                          (uintptr_t)g_log_std | (uintptr_t)g_value | (uintptr_t)losses;
    if (all & 3) return fail(HOPE_EINVAL, "hope_env_ppo_loss: misaligned buffer (every tensor 4 bytes)");
    HOPE_ON_DEVICE(h);
    const long long nk = pb_chunks(mb);                           // <= the partials' room: mb <= max_batch
    hipLaunchKernelGGL(k_ppo_loss, dim3((unsigned)nk), dim3(64), 0, (hipStream_t)stream, raw, log_std, value, (const float*)batch->action,
                       (const float*)batch->old_lp, (const float*)batch->adv, (const float*)batch->v_target, mb, clip, (pair & 7) ? 0 : 1, g_raw, g_value, nk,
                       h->ppo.part);
    hipLaunchKernelGGL(k_ppo_merge, dim3(1), dim3(64), 0, (hipStream_t)stream, nk, (double)mb, h->ppo.part, losses, g_log_std);
    HIPCHK(hipGetLastError());
    return HOPE_OK;
}

int hope_ppo_gather_host(const hope_ring_t* ring, const float* adv, const float* v_target, const int64_t* index, int64_t batch, const hope_ppo_batch_t* out) {
    const int rc = pb_gather_host(ring, adv, v_target, index, batch, out);
    if (rc != HOPE_OK)
        return fail(rc, "hope_ppo_gather_host: bad argument (a null ring, tensor, adv, v_target, index or out, n or T < 1, or batch < 1)");
    return HOPE_OK;
}

int hope_ppo_loss_host(const float* raw, const float* log_std, const float* value, const hope_ppo_batch_t* batch, int64_t mb, double clip, float* g_raw,
                       float* g_log_std, float* g_value, float* losses) {
    const int rc = pb_loss_host(raw, log_std, value, batch, mb, clip, g_raw, g_log_std, g_value, losses);
    if (rc == HOPE_ENOMEM) return fail(rc, "hope_ppo_loss_host: out of memory for the chunk partials");
    if (rc != HOPE_OK)
        return fail(rc, "hope_ppo_loss_host: bad argument (a null raw / log_std / value / batch / output, a null action / old_lp / adv / v_target in batch, mb < 1, or a clip that is negative or not finite)");
    return HOPE_OK;
}

// ---- SAC's update (include/hope_env.h; kernels: hope_sac_kernel.h, rule: hope_sac_core.h) ----
int hope_env_sac_enable(hope_env_t* h, int max_batch) {
    HOPE_ENTER(h, "hope_env_sac_enable");
    if (max_batch < 1 || max_batch > HOPE_SAC_MAX_BATCH) return fail(HOPE_EINVAL, "hope_env_sac_enable: max_batch must be 1 .. " + std::to_string(HOPE_SAC_MAX_BATCH));
    if (h->sac.on && max_batch <= h->sac.max_batch) return HOPE_OK;
    HOPE_ON_DEVICE(h);
    HIPCHK(hipDeviceSynchronize());                         // calls in flight use the partials that a larger max_batch replaces
    sac_free(h);
    const int rc = device_buffer("hope_env_sac_enable", &h->sac.part, (size_t)SU_SUMS * (size_t)su_chunks(max_batch) * sizeof(double));
    if (rc != HOPE_OK) { sac_free(h); return rc; }
    h->sac.max_batch = max_batch;
    h->sac.on = true;
    return HOPE_OK;
}

int hope_env_sac_disable(hope_env_t* h) {
    HOPE_ENTER(h, "hope_env_sac_disable");
    return feature_disable(h, sac_free);
}

// the batch of a hope_env_sac_* call `name`: 1 .. max_batch
#define SAC_BATCH(h, batch, name)                                                                                                           \
    do {                                                                                                                                    \
        if ((batch) < 1 || (batch) > (h)->sac.max_batch)                                                                                    \
            return fail(HOPE_EINVAL, std::string(name) + ": batch must be 1 .. max_batch (" + std::to_string((h)->sac.max_batch) + ")");  \
    } while (0)

int hope_env_sac_sample(hope_env_t* h, const float* raw, const float* log_std, const float* eps, int batch, float* action, float* lp, void* stream) {
    HOPE_ENTER(h, "hope_env_sac_sample");
    SAC_ON(h, "hope_env_sac_sample");
    if (!raw || !log_std || !eps || !action || !lp) return fail(HOPE_EINVAL, "hope_env_sac_sample: null raw / log_std / eps / action / lp");
    SAC_BATCH(h, batch, "hope_env_sac_sample");
    const uintptr_t pair = (uintptr_t)raw | (uintptr_t)eps | (uintptr_t)action;
    if ((pair | (uintptr_t)log_std | (uintptr_t)lp) & 3) return fail(HOPE_EINVAL, "hope_env_sac_sample: misaligned buffer (every tensor 4 bytes)");
    HOPE_ON_DEVICE(h);
    hipLaunchKernelGGL(k_sac_sample, dim3((unsigned)su_chunks(batch)), dim3(64), 0, (hipStream_t)stream, raw, log_std, eps, batch, (pair & 7) ? 0 : 1, action, lp);
    HIPCHK(hipGetLastError());
    return HOPE_OK;
}

int hope_env_sac_critic(hope_env_t* h, const float* q1, const float* q2, const float* qt1, const float* qt2, const float* next_lp, const float* reward,
                        const float* done, const double* log_alpha, double gamma, int batch, float* q_target, float* g_q1, float* g_q2, float* losses,
                        void* stream) {
    HOPE_ENTER(h, "hope_env_sac_critic");
    SAC_ON(h, "hope_env_sac_critic");
    if (!q1 || !q2 || !qt1 || !qt2 || !next_lp || !reward || !done || !log_alpha || !q_target || !g_q1 || !g_q2 || !losses)
        return fail(HOPE_EINVAL, "hope_env_sac_critic: null q1 / q2 / qt1 / qt2 / next_lp / reward / done / log_alpha / q_target / g_q1 / g_q2 / losses");
    SAC_BATCH(h, batch, "hope_env_sac_critic");
    if (!ga_finite(gamma)) return fail(HOPE_EINVAL, "hope_env_sac_critic: gamma must be finite");
    const uintptr_t all = (uintptr_t)q1 | (uintptr_t)q2 | (uintptr_t)qt1 | (uintptr_t)qt2 | (uintptr_t)next_lp | (uintptr_t)reward | (uintptr_t)done |
                          (uintptr_t)q_target | (uintptr_t)g_q1 | (uintptr_t)g_q2 | (uintptr_t)losses;
    if ((all & 3) || ((uintptr_t)log_alpha & 7)) return fail(HOPE_EINVAL, "hope_env_sac_critic: misaligned buffer (log_alpha 8 bytes, every other tensor 4)");
    HOPE_ON_DEVICE(h);
    const long long nk = su_chunks(batch);                        // <= the partials' room: batch <= max_batch
    hipLaunchKernelGGL(k_sac_critic, dim3((unsigned)nk), dim3(64), 0, (hipStream_t)stream, q1, q2, qt1, qt2, next_lp, reward, done, log_alpha, gamma, batch,
                       q_target, g_q1, g_q2, nk, h->sac.part);
    hipLaunchKernelGGL(k_sac_merge<SU_CRITIC_SUMS>, dim3(1), dim3(64), 0, (hipStream_t)stream, nk, (double)batch, h->sac.part, log_alpha, losses,
                       (float*)nullptr, (double*)nullptr);
    HIPCHK(hipGetLastError());
    return HOPE_OK;
}

int hope_env_sac_seed(hope_env_t* h, const float* q1, const float* q2, int batch, float* s1, float* s2, void* stream) {
    HOPE_ENTER(h, "hope_env_sac_seed");
    SAC_ON(h, "hope_env_sac_seed");
    if (!q1 || !q2 || !s1 || !s2) return fail(HOPE_EINVAL, "hope_env_sac_seed: null q1 / q2 / s1 / s2");
    SAC_BATCH(h, batch, "hope_env_sac_seed");
    if (((uintptr_t)q1 | (uintptr_t)q2 | (uintptr_t)s1 | (uintptr_t)s2) & 3) return fail(HOPE_EINVAL, "hope_env_sac_seed: misaligned buffer (every tensor 4 bytes)");
    HOPE_ON_DEVICE(h);
    hipLaunchKernelGGL(k_sac_seed, dim3((unsigned)su_chunks(batch)), dim3(64), 0, (hipStream_t)stream, q1, q2, batch, s1, s2);
    HIPCHK(hipGetLastError());
    return HOPE_OK;
}

int hope_env_sac_policy(hope_env_t* h, const float* raw, const float* log_std, const float* eps, const float* q1, const float* q2, const float* g_action,
                        const double* log_alpha, double target_entropy, int batch, float* g_raw, float* g_log_std, double* g_log_alpha, float* losses,
                        void* stream) {
    HOPE_ENTER(h, "hope_env_sac_policy");
    SAC_ON(h, "hope_env_sac_policy");
    if (!raw || !log_std || !eps || !q1 || !q2 || !g_action || !log_alpha || !g_raw || !g_log_std || !g_log_alpha || !losses)
        return fail(HOPE_EINVAL, "hope_env_sac_policy: null raw / log_std / eps / q1 / q2 / g_action / log_alpha / g_raw / g_log_std / g_log_alpha / losses");
    SAC_BATCH(h, batch, "hope_env_sac_policy");
    if (!ga_finite(target_entropy)) return fail(HOPE_EINVAL, "hope_env_sac_policy: target_entropy must be finite");
    const uintptr_t pair = (uintptr_t)raw | (uintptr_t)eps | (uintptr_t)g_action | (uintptr_t)g_raw;
    const uintptr_t all = pair | (uintptr_t)log_std | (uintptr_t)q1 | (uintptr_t)q2 | (uintptr_t)g_log_std | (uintptr_t)losses;
    if ((all & 3) || (((uintptr_t)log_alpha | (uintptr_t)g_log_alpha) & 7))
        return fail(HOPE_EINVAL, "hope_env_sac_policy: misaligned buffer (log_alpha and g_log_alpha 8 bytes, every other tensor 4)");
    HOPE_ON_DEVICE(h);
    const long long nk = su_chunks(batch);                        // <= the partials' room: batch <= max_batch
    hipLaunchKernelGGL(k_sac_policy, dim3((unsigned)nk), dim3(64), 0, (hipStream_t)stream, raw, log_std, eps, q1, q2, g_action, log_alpha, target_entropy, batch,
                       (pair & 7) ? 0 : 1, g_raw, nk, h->sac.part);
    hipLaunchKernelGGL(k_sac_merge<SU_POLICY_SUMS>, dim3(1), dim3(64), 0, (hipStream_t)stream, nk, (double)batch, h->sac.part, log_alpha, losses, g_log_std,
                       g_log_alpha);
    HIPCHK(hipGetLastError());
    return HOPE_OK;
}

int hope_sac_sample_host(const float* raw, const float* log_std, const float* eps, int64_t batch, float* action, float* lp) {
    const int rc = su_sample_host(raw, log_std, eps, batch, action, lp);
    if (rc != HOPE_OK) return fail(rc, "hope_sac_sample_host: bad argument (a null raw / log_std / eps / action / lp, or batch < 1)");
    return HOPE_OK;
}

int hope_sac_critic_host(const float* q1, const float* q2, const float* qt1, const float* qt2, const float* next_lp, const float* reward, const float* done,
                         const double* log_alpha, double gamma, int64_t batch, float* q_target, float* g_q1, float* g_q2, float* losses) {
    const int rc = su_critic_host(q1, q2, qt1, qt2, next_lp, reward, done, log_alpha, gamma, batch, q_target, g_q1, g_q2, losses);
    if (rc == HOPE_ENOMEM) return fail(rc, "hope_sac_critic_host: out of memory for the chunk partials");
    if (rc != HOPE_OK) return fail(rc, "hope_sac_critic_host: bad argument (a null input or output, batch < 1, or a gamma that is not finite)");
    return HOPE_OK;
}

int hope_sac_seed_host(const float* q1, const float* q2, int64_t batch, float* s1, float* s2) {
    const int rc = su_seed_host(q1, q2, batch, s1, s2);
    if (rc != HOPE_OK) return fail(rc, "hope_sac_seed_host: bad argument (a null q1 / q2 / s1 / s2, or batch < 1)");
    return HOPE_OK;
}

int hope_sac_policy_host(const float* raw, const float* log_std, const float* eps, const float* q1, const float* q2, const float* g_action,
                         const double* log_alpha, double target_entropy, int64_t batch, float* g_raw, float* g_log_std, double* g_log_alpha, float* losses) {
    const int rc = su_policy_host(raw, log_std, eps, q1, q2, g_action, log_alpha, target_entropy, batch, g_raw, g_log_std, g_log_alpha, losses);
    if (rc == HOPE_ENOMEM) return fail(rc, "hope_sac_policy_host: out of memory for the chunk partials");
    if (rc != HOPE_OK) return fail(rc, "hope_sac_policy_host: bad argument (a null input or output, batch < 1, or a target_entropy that is not finite)");
    return HOPE_OK;
}

}  // extern "C"

// ---- the optimiser block (include/hope_env.h; kernel: hope_optim_kernel.h, rule: hope_optim_core.h) ----
static int optim_refused(const char* name, int rc, const OpBad& bad) {
    std::string where = bad.kind == OP_BAD_ENTRY ? "entry " + std::to_string(bad.index) + ": " : bad.kind == OP_BAD_GROUP ? "group " + std::to_string(bad.index) + ": " : "";
    return fail(rc, std::string(name) + ": " + where + bad.what);
}

// the checked entries as launches of k_optim<MODE>: OP_CAP entries at a time, each table built on the stack and handed over by value
template <int MODE>
static int optim_launch(const hope_optim_entry_t* e, int n, const hope_optim_group_t* g, int n_groups, double tau, hipStream_t st) {
    OkTable tab;
    for (int at = 0; at < n; at += OP_CAP) {
        memset(&tab, 0, sizeof(tab));
        for (int k = 0; k < n_groups; k++) tab.group[k] = g[k];
        tab.tau = tau;
        tab.omt = 1.0 - tau;
        tab.n = n - at < OP_CAP ? n - at : OP_CAP;
        uint32_t chunks = 0;
        for (int i = 0; i < tab.n; i++) {
            const hope_optim_entry_t& s = e[at + i];
            OkEntry& d = tab.e[i];
            d.p = s.p; d.g = s.g;
            uintptr_t bits = (uintptr_t)s.p | (uintptr_t)s.g;
            if (MODE == OP_ADAM) { d.m = s.m; d.v = s.v; bits |= (uintptr_t)s.m | (uintptr_t)s.v; }
            d.numel = (uint32_t)s.numel;
            d.first = chunks;
            d.meta = s.dtype == HOPE_OPTIM_F64 ? OK_F64 : (bits & 15) ? 0u : OK_VEC;
            if (MODE == OP_ADAM) d.meta |= (uint32_t)s.group << 2;
            chunks += (uint32_t)((s.numel + OP_CHUNK - 1) / OP_CHUNK);       // <= 2^21 + n in all: the call's elements are <= 2^31
        }
        hipLaunchKernelGGL(k_optim<MODE>, dim3(chunks), dim3(OK_THREADS), 0, st, tab);
        HIPCHK(hipGetLastError());
    }
    return HOPE_OK;
}

extern "C" {

int hope_env_optim_adam(hope_env_t* h, const hope_optim_entry_t* entries, int n_entries, const hope_optim_group_t* groups, int n_groups, void* stream) {
    HOPE_ENTER(h, "hope_env_optim_adam");
    OpBad bad;
    const int rc = op_check(OP_ADAM, entries, n_entries, groups, n_groups, 0.0, &bad);
    if (rc != HOPE_OK) return optim_refused("hope_env_optim_adam", rc, bad);
    HOPE_ON_DEVICE(h);
    return optim_launch<OP_ADAM>(entries, n_entries, groups, n_groups, 0.0, (hipStream_t)stream);
}

int hope_env_optim_polyak(hope_env_t* h, const hope_optim_entry_t* entries, int n_entries, double tau, void* stream) {
    HOPE_ENTER(h, "hope_env_optim_polyak");
    OpBad bad;
    const int rc = op_check(OP_POLYAK, entries, n_entries, nullptr, 0, tau, &bad);
    if (rc != HOPE_OK) return optim_refused("hope_env_optim_polyak", rc, bad);
    HOPE_ON_DEVICE(h);
    return optim_launch<OP_POLYAK>(entries, n_entries, nullptr, 0, tau, (hipStream_t)stream);
}

int hope_optim_adam_host(const hope_optim_entry_t* entries, int n_entries, const hope_optim_group_t* groups, int n_groups) {
    OpBad bad;
    const int rc = op_adam_host(entries, n_entries, groups, n_groups, &bad);
    if (rc != HOPE_OK) return optim_refused("hope_optim_adam_host", rc, bad);
    return HOPE_OK;
}

int hope_optim_polyak_host(const hope_optim_entry_t* entries, int n_entries, double tau) {
    OpBad bad;
    const int rc = op_polyak_host(entries, n_entries, tau, &bad);
    if (rc != HOPE_OK) return optim_refused("hope_optim_polyak_host", rc, bad);
    return HOPE_OK;
}

}  // extern "C"
