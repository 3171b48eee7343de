// hope_policy.hip -- the policy's inference forward of the C ABI (include/hope_env.h "the policy's inference forward"): the packed
// parameter buffer of the handle, k_policy_pack / k_policy_forward (hope_policy_kernel.h) and the host twin (hope_policy_core.h);
// and the image encoder's ("the image encoder's inference forward"): k_imgenc_pack / k_imgenc_conv / k_imgenc_head
// (hope_imgenc_kernel.h) and its twin (hope_imgenc_core.h); and the critics' ("the critics' inference forward"): the handle's parameter
// slots, k_critic_pack / k_critic_forward (hope_critic_kernel.h) and their twin (hope_critic_core.h).  The three features share no state.
// Shares nothing with the other features but the handle (hope_handle.h); its kernels are instantiated here and nowhere else.
#include <hip/hip_runtime.h>

#include <string>

#include "hope_handle.h"
#include "hope_policy_kernel.h"
#include "hope_imgenc_kernel.h"
#include "hope_critic_kernel.h"

using namespace hope;

static_assert(sizeof(hope_policy_params_t) == PC_NPARAM * sizeof(const float*), "hope_policy_params_t is PC_NPARAM pointers, in pc_layout's order");

void hope::policy_free(hope_env_t* h) {
    if (h->policy.packed) hipFree(h->policy.packed);
    h->policy = hope_env::Policy{};
}

static_assert(sizeof(hope_imgenc_params_t) == IE_NPARAM * sizeof(const float*), "hope_imgenc_params_t is IE_NPARAM pointers, in IE_OFF_*'s order");

void hope::imgenc_free(hope_env_t* h) {
    if (h->imgenc.packed) hipFree(h->imgenc.packed);
    if (h->imgenc.feat) hipFree(h->imgenc.feat);
    h->imgenc = hope_env::ImgEnc{};
}

static_assert(sizeof(hope_critic_params_t) == CC_NPARAM * sizeof(const float*), "hope_critic_params_t is CC_NPARAM pointers, in cc_layout's order");

void hope::critics_free(hope_env_t* h) {
    if (h->critics.packed) hipFree(h->critics.packed);
    h->critics = hope_env::Critics{};
}

template <int T>
static int critic_launch(hope_env_t* h, const CcLayout& L, const CkSlots& slots, int n, const float* lidar, const float* target, const float* mask,
                         const float* img, const float* action, int batch, float* out, hipStream_t st) {
    static bool lds_set[64] = {};                              // per device: the kernel's dynamic LDS is above the default limit
    if (h->device >= 0 && h->device < 64 && !lds_set[h->device]) {
        HIPCHK(hipFuncSetAttribute((const void*)k_critic_forward<T>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ck_lds_bytes(T)));
        lds_set[h->device] = true;
    }
    hipLaunchKernelGGL(k_critic_forward<T>, dim3((unsigned)((batch + PK_TILE - 1) / PK_TILE), (unsigned)n), dim3(PK_THREADS), ck_lds_bytes(T), st,
                       (const float*)h->critics.packed, L, slots, h->critics.has_img, h->critics.has_action, lidar, target, mask, img, action, (long long)batch, out);
    HIPCHK(hipGetLastError());
    return HOPE_OK;
}

template <int ACT>
static int imgenc_launch(hope_env_t* h, const uint8_t* img, long long batch, float* token, float* feat, hipStream_t st, int stages = 3) {
    static bool lds_set[64] = {};                              // per device: the conv kernel's dynamic LDS is above the default limit
    if (h->device >= 0 && h->device < 64 && !lds_set[h->device]) {
        HIPCHK(hipFuncSetAttribute((const void*)k_imgenc_conv<ACT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)IK_CONV_LDS));
        lds_set[h->device] = true;
    }
    if (stages & 1) {
        hipLaunchKernelGGL(k_imgenc_conv<ACT>, dim3((unsigned)batch), dim3(IK_CONV_THREADS), IK_CONV_LDS, st, (const float*)h->imgenc.packed, img, feat);
        HIPCHK(hipGetLastError());
    }
    if (!(stages & 2)) return HOPE_OK;
    hipLaunchKernelGGL(k_imgenc_head<ACT>, dim3((unsigned)((batch + IK_TILE - 1) / IK_TILE)), dim3(IK_THREADS), 0, st, (const float*)h->imgenc.packed,
                       (const float*)feat, batch, token);
    HIPCHK(hipGetLastError());
    return HOPE_OK;
}

template <int T>
static int policy_launch(hope_env_t* h, const PcLayout& L, const float* lidar, const float* target, const float* mask, const float* img, int batch, float* out,
                         hipStream_t st) {
    static bool lds_set[64] = {};                              // per device: the kernel's dynamic LDS is above the default limit
    if (h->device >= 0 && h->device < 64 && !lds_set[h->device]) {
        HIPCHK(hipFuncSetAttribute((const void*)k_policy_forward<T>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)pk_lds_bytes(T)));
        lds_set[h->device] = true;
    }
    hipLaunchKernelGGL(k_policy_forward<T>, dim3((unsigned)((batch + PK_TILE - 1) / PK_TILE)), dim3(PK_THREADS), pk_lds_bytes(T), st, (const float*)h->policy.packed,
                       L, lidar, target, mask, img, (long long)batch, h->policy.out_dim, h->policy.tanh_out, out);
    HIPCHK(hipGetLastError());
    return HOPE_OK;
}

extern "C" {

int hope_env_policy_enable(hope_env_t* h, int n_tokens, int out_dim, int tanh_out, int max_batch) {
    HOPE_ENTER(h, "hope_env_policy_enable");
    if (!pc_shape_ok(n_tokens, out_dim, tanh_out))
        return fail(HOPE_EINVAL, "hope_env_policy_enable: the shape is fixed: n_tokens 3 or 4, out_dim 1 or 2, tanh_out 0 or 1");
    if (max_batch < 1 || max_batch > HOPE_POLICY_MAX_BATCH)
        return fail(HOPE_EINVAL, "hope_env_policy_enable: max_batch must be 1 .. " + std::to_string(HOPE_POLICY_MAX_BATCH));
    hope_env::Policy& p = h->policy;
    if (p.on && p.n_tokens == n_tokens && p.out_dim == out_dim && p.tanh_out == tanh_out) {
        if (max_batch > p.max_batch) p.max_batch = max_batch;
        return HOPE_OK;
    }
    HOPE_ON_DEVICE(h);
    HIPCHK(hipDeviceSynchronize());                            // calls in flight read the buffer that another shape replaces
    policy_free(h);
    const PcLayout L = pc_layout(n_tokens, out_dim);
    hipError_t e_ = hipMalloc((void**)&p.packed, (size_t)L.total * sizeof(float));
    if (e_ != hipSuccess) {
        p.packed = nullptr;
        return fail(HOPE_ENOMEM, std::string("hope_env_policy_enable: ") + hipGetErrorString(e_));
    }
    e_ = hipMemset(p.packed, 0, (size_t)L.total * sizeof(float));
    if (e_ == hipSuccess) e_ = hipDeviceSynchronize();
    if (e_ != hipSuccess) {
        policy_free(h);
        return fail(HOPE_EHIP, std::string("hope_env_policy_enable: ") + hipGetErrorString(e_));
    }
    p.n_tokens = n_tokens; p.out_dim = out_dim; p.tanh_out = tanh_out; p.max_batch = max_batch;
    p.on = true;
    return HOPE_OK;
}

int hope_env_policy_disable(hope_env_t* h) {
    HOPE_ENTER(h, "hope_env_policy_disable");
    HOPE_ON_DEVICE(h);
    HIPCHK(hipDeviceSynchronize());
    policy_free(h);
    return HOPE_OK;
}

int hope_env_policy_load(hope_env_t* h, const hope_policy_params_t* p, void* stream) {
    HOPE_ENTER(h, "hope_env_policy_load");
    HOPE_NEED(h->policy.on, "hope_env_policy_load", "the policy forward is off (hope_env_policy_enable first)");
    if (!p) return fail(HOPE_EINVAL, "hope_env_policy_load: null parameter struct");
    PkPtrs ptrs;
    uintptr_t bits = 0;
    for (int i = 0; i < PC_NPARAM; ++i) {
        ptrs.t[i] = ((const float* const*)p)[i];
        if (!ptrs.t[i]) return fail(HOPE_EINVAL, "hope_env_policy_load: null tensor (field " + std::to_string(i) + " of hope_policy_params_t)");
        bits |= (uintptr_t)ptrs.t[i];
    }
    if (bits & 3) return fail(HOPE_EINVAL, "hope_env_policy_load: misaligned tensor (every tensor 4 bytes)");
    HOPE_ON_DEVICE(h);
    const PcLayout L = pc_layout(h->policy.n_tokens, h->policy.out_dim);
    hipLaunchKernelGGL(k_policy_pack, dim3((unsigned)((L.total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, ptrs, L, h->policy.packed);
    HIPCHK(hipGetLastError());
    h->policy.loaded = true;
    return HOPE_OK;
}

int hope_env_policy_forward(hope_env_t* h, const float* lidar, const float* target, const float* mask, const float* img_token, int batch, float* out,
                            void* stream) {
    HOPE_ENTER(h, "hope_env_policy_forward");
    HOPE_NEED(h->policy.on, "hope_env_policy_forward", "the policy forward is off (hope_env_policy_enable first)");
    HOPE_NEED(h->policy.loaded, "hope_env_policy_forward", "no parameters yet (hope_env_policy_load first)");
    if (!lidar || !target || !mask || !out) return fail(HOPE_EINVAL, "hope_env_policy_forward: null lidar / target / mask / out");
    if ((h->policy.n_tokens == 4) != (img_token != nullptr))
        return fail(HOPE_EINVAL, h->policy.n_tokens == 4 ? "hope_env_policy_forward: n_tokens is 4: the image token is missing"
                                                         : "hope_env_policy_forward: n_tokens is 3: there is no image token");
    if (batch < 1 || batch > h->policy.max_batch)
        return fail(HOPE_EINVAL, "hope_env_policy_forward: batch must be 1 .. max_batch (" + std::to_string(h->policy.max_batch) + ")");
    if (((uintptr_t)lidar | (uintptr_t)target | (uintptr_t)mask | (uintptr_t)img_token | (uintptr_t)out) & 3)
        return fail(HOPE_EINVAL, "hope_env_policy_forward: misaligned buffer (every tensor 4 bytes)");
    HOPE_ON_DEVICE(h);
    const PcLayout L = pc_layout(h->policy.n_tokens, h->policy.out_dim);
    if (h->policy.n_tokens == 4) return policy_launch<4>(h, L, lidar, target, mask, img_token, batch, out, (hipStream_t)stream);
    return policy_launch<3>(h, L, lidar, target, mask, nullptr, batch, out, (hipStream_t)stream);
}

int hope_policy_forward_host(const hope_policy_params_t* host_params, int n_tokens, int out_dim, int tanh_out, const float* lidar, const float* target,
                             const float* mask, const float* img_token, int64_t batch, float* out) {
    const int rc = pc_forward_host(host_params, n_tokens, out_dim, tanh_out, lidar, target, mask, img_token, batch, out);
    if (rc != HOPE_OK)
        return fail(rc, "hope_policy_forward_host: bad argument (a null parameter, input or output, n_tokens not 3 or 4, out_dim not 1 or 2, tanh_out not 0 or 1, "
                        "an image token that does not go with n_tokens, or batch < 1)");
    return HOPE_OK;
}

int hope_env_critic_enable(hope_env_t* h, int n_slots, int has_img, int has_action, int max_batch) {
    HOPE_ENTER(h, "hope_env_critic_enable");
    if (n_slots < 1 || n_slots > HOPE_CRITIC_SLOTS || !cc_shape_ok(has_img, has_action))
        return fail(HOPE_EINVAL, "hope_env_critic_enable: n_slots must be 1 .. " + std::to_string(HOPE_CRITIC_SLOTS) + ", has_img and has_action 0 or 1");
    if (max_batch < 1 || max_batch > HOPE_POLICY_MAX_BATCH)
        return fail(HOPE_EINVAL, "hope_env_critic_enable: max_batch must be 1 .. " + std::to_string(HOPE_POLICY_MAX_BATCH));
    hope_env::Critics& c = h->critics;
    if (c.on && c.n_slots == n_slots && c.has_img == has_img && c.has_action == has_action) {
        if (max_batch > c.max_batch) c.max_batch = max_batch;
        return HOPE_OK;
    }
    HOPE_ON_DEVICE(h);
    HIPCHK(hipDeviceSynchronize());                            // calls in flight read the buffer that another shape replaces
    critics_free(h);
    const size_t bytes = (size_t)n_slots * cc_layout(has_img, has_action).total * sizeof(float);
    hipError_t e_ = hipMalloc((void**)&c.packed, bytes);
    if (e_ != hipSuccess) {
        c.packed = nullptr;
        return fail(HOPE_ENOMEM, std::string("hope_env_critic_enable: ") + hipGetErrorString(e_));
    }
    e_ = hipMemset(c.packed, 0, bytes);
    if (e_ == hipSuccess) e_ = hipDeviceSynchronize();
    if (e_ != hipSuccess) {
        critics_free(h);
        return fail(HOPE_EHIP, std::string("hope_env_critic_enable: ") + hipGetErrorString(e_));
    }
    c.n_slots = n_slots; c.has_img = has_img; c.has_action = has_action; c.max_batch = max_batch;
    c.on = true;
    return HOPE_OK;
}

int hope_env_critic_disable(hope_env_t* h) {
    HOPE_ENTER(h, "hope_env_critic_disable");
    HOPE_ON_DEVICE(h);
    HIPCHK(hipDeviceSynchronize());
    critics_free(h);
    return HOPE_OK;
}

int hope_env_critic_load(hope_env_t* h, int slot, const hope_critic_params_t* p, void* stream) {
    HOPE_ENTER(h, "hope_env_critic_load");
    hope_env::Critics& c = h->critics;
    HOPE_NEED(c.on, "hope_env_critic_load", "the critics' forward is off (hope_env_critic_enable first)");
    if (slot < 0 || slot >= c.n_slots) return fail(HOPE_EINVAL, "hope_env_critic_load: slot must be 0 .. n_slots - 1 (" + std::to_string(c.n_slots - 1) + ")");
    if (!p) return fail(HOPE_EINVAL, "hope_env_critic_load: null parameter struct");
    CkPtrs ptrs;
    uintptr_t bits = 0;
    for (int i = 0; i < CC_NPARAM; ++i) {
        ptrs.t[i] = ((const float* const*)p)[i];
        if (i >= PC_NPARAM && !c.has_action) {
            if (ptrs.t[i]) return fail(HOPE_EINVAL, "hope_env_critic_load: has_action is 0: the action tensors must be NULL");
            continue;
        }
        if (!ptrs.t[i]) return fail(HOPE_EINVAL, "hope_env_critic_load: null tensor (field " + std::to_string(i) + " of hope_critic_params_t)");
        bits |= (uintptr_t)ptrs.t[i];
    }
    if (bits & 3) return fail(HOPE_EINVAL, "hope_env_critic_load: misaligned tensor (every tensor 4 bytes)");
    HOPE_ON_DEVICE(h);
    const CcLayout L = cc_layout(c.has_img, c.has_action);
    hipLaunchKernelGGL(k_critic_pack, dim3((unsigned)((L.total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, ptrs, L, c.packed, slot);
    HIPCHK(hipGetLastError());
    c.loaded[slot] = true;
    return HOPE_OK;
}

int hope_env_critic_forward(hope_env_t* h, const int* slots, int n, const float* lidar, const float* target, const float* mask, const float* img_token,
                            const float* action, int batch, float* out, void* stream) {
    HOPE_ENTER(h, "hope_env_critic_forward");
    const hope_env::Critics& c = h->critics;
    HOPE_NEED(c.on, "hope_env_critic_forward", "the critics' forward is off (hope_env_critic_enable first)");
    if (!slots || n < 1 || n > c.n_slots) return fail(HOPE_EINVAL, "hope_env_critic_forward: slots must name 1 .. n_slots (" + std::to_string(c.n_slots) + ") slots");
    CkSlots sl = {};
    for (int i = 0; i < n; ++i) {
        if (slots[i] < 0 || slots[i] >= c.n_slots)
            return fail(HOPE_EINVAL, "hope_env_critic_forward: slot " + std::to_string(slots[i]) + " is outside 0 .. n_slots - 1 (" + std::to_string(c.n_slots - 1) + ")");
        for (int j = 0; j < i; ++j)
            if (slots[j] == slots[i]) return fail(HOPE_EINVAL, "hope_env_critic_forward: slot " + std::to_string(slots[i]) + " is named twice");
        sl.s[i] = slots[i];
    }
    for (int i = 0; i < n; ++i)
        HOPE_NEED(c.loaded[sl.s[i]], "hope_env_critic_forward", "a slot has no parameters yet (hope_env_critic_load first)");
    if (!lidar || !target || !mask || !out) return fail(HOPE_EINVAL, "hope_env_critic_forward: null lidar / target / mask / out");
    if ((c.has_img != 0) != (img_token != nullptr))
        return fail(HOPE_EINVAL, c.has_img ? "hope_env_critic_forward: has_img is 1: the image token is missing" : "hope_env_critic_forward: has_img is 0: there is no image token");
    if ((c.has_action != 0) != (action != nullptr))
        return fail(HOPE_EINVAL, c.has_action ? "hope_env_critic_forward: has_action is 1: the action is missing" : "hope_env_critic_forward: has_action is 0: there is no action");
    if (batch < 1 || batch > c.max_batch)
        return fail(HOPE_EINVAL, "hope_env_critic_forward: batch must be 1 .. max_batch (" + std::to_string(c.max_batch) + ")");
    if (((uintptr_t)lidar | (uintptr_t)target | (uintptr_t)mask | (uintptr_t)img_token | (uintptr_t)action | (uintptr_t)out) & 3)
        return fail(HOPE_EINVAL, "hope_env_critic_forward: misaligned buffer (every tensor 4 bytes)");
    HOPE_ON_DEVICE(h);
    const CcLayout L = cc_layout(c.has_img, c.has_action);
    const hipStream_t st = (hipStream_t)stream;
    switch (cc_tokens(c.has_img, c.has_action)) {
        case 3: return critic_launch<3>(h, L, sl, n, lidar, target, mask, img_token, action, batch, out, st);
        case 4: return critic_launch<4>(h, L, sl, n, lidar, target, mask, img_token, action, batch, out, st);
        default: return critic_launch<5>(h, L, sl, n, lidar, target, mask, img_token, action, batch, out, st);
    }
}

int hope_critic_forward_host(const hope_critic_params_t* host_params, int has_img, int has_action, const float* lidar, const float* target, const float* mask,
                             const float* img_token, const float* action, int64_t batch, float* out) {
    const int rc = cc_forward_host(host_params, has_img, has_action, lidar, target, mask, img_token, action, batch, out);
    if (rc != HOPE_OK)
        return fail(rc, "hope_critic_forward_host: bad argument (a null parameter, input or output, has_img / has_action not 0 or 1, an image token, action or "
                        "action tensors that do not go with them, or batch < 1)");
    return HOPE_OK;
}

int hope_env_imgenc_enable(hope_env_t* h, int act, int max_batch) {
    HOPE_ENTER(h, "hope_env_imgenc_enable");
    if (!ie_act_ok(act)) return fail(HOPE_EINVAL, "hope_env_imgenc_enable: act must be 0 (tanh) or 1 (LeakyReLU)");
    if (max_batch < 1 || max_batch > HOPE_IMGENC_MAX_BATCH)
        return fail(HOPE_EINVAL, "hope_env_imgenc_enable: max_batch must be 1 .. " + std::to_string(HOPE_IMGENC_MAX_BATCH));
    hope_env::ImgEnc& p = h->imgenc;
    if (p.on && max_batch <= p.max_batch) {
        p.act = act;                                           // the packed words do not depend on act
        return HOPE_OK;
    }
    HOPE_ON_DEVICE(h);
    HIPCHK(hipDeviceSynchronize());                            // calls in flight use the feature buffer that a larger one replaces
    float *packed = p.packed, *feat = nullptr;
    hipError_t e_ = hipSuccess;
    if (!packed) {
        e_ = hipMalloc((void**)&packed, (size_t)IE_TOTAL * sizeof(float));
        if (e_ == hipSuccess) e_ = hipMemset(packed, 0, (size_t)IE_TOTAL * sizeof(float));
        else packed = nullptr;
    }
    if (e_ == hipSuccess) {
        e_ = hipMalloc((void**)&feat, (size_t)max_batch * IE_FEAT * sizeof(float));
        if (e_ != hipSuccess) feat = nullptr;
    }
    if (e_ == hipSuccess) e_ = hipDeviceSynchronize();
    if (e_ != hipSuccess) {                                    // the state from before the call stays
        if (feat) hipFree(feat);
        if (packed && packed != p.packed) hipFree(packed);
        return fail(e_ == hipErrorOutOfMemory ? HOPE_ENOMEM : HOPE_EHIP, std::string("hope_env_imgenc_enable: ") + hipGetErrorString(e_));
    }
    if (p.feat) hipFree(p.feat);
    p.packed = packed; p.feat = feat; p.act = act; p.max_batch = max_batch;
    p.on = true;
    return HOPE_OK;
}

int hope_env_imgenc_disable(hope_env_t* h) {
    HOPE_ENTER(h, "hope_env_imgenc_disable");
    HOPE_ON_DEVICE(h);
    HIPCHK(hipDeviceSynchronize());
    imgenc_free(h);
    return HOPE_OK;
}

int hope_env_imgenc_load(hope_env_t* h, const hope_imgenc_params_t* p, void* stream) {
    HOPE_ENTER(h, "hope_env_imgenc_load");
    HOPE_NEED(h->imgenc.on, "hope_env_imgenc_load", "the image encoder is off (hope_env_imgenc_enable first)");
    if (!p) return fail(HOPE_EINVAL, "hope_env_imgenc_load: null parameter struct");
    IkPtrs ptrs;
    uintptr_t bits = 0;
    for (int i = 0; i < IE_NPARAM; ++i) {
        ptrs.t[i] = ((const float* const*)p)[i];
        if (!ptrs.t[i]) return fail(HOPE_EINVAL, "hope_env_imgenc_load: null tensor (field " + std::to_string(i) + " of hope_imgenc_params_t)");
        bits |= (uintptr_t)ptrs.t[i];
    }
    if (bits & 3) return fail(HOPE_EINVAL, "hope_env_imgenc_load: misaligned tensor (every tensor 4 bytes)");
    HOPE_ON_DEVICE(h);
    hipLaunchKernelGGL(k_imgenc_pack, dim3((unsigned)((IE_TOTAL + 255) / 256)), dim3(256), 0, (hipStream_t)stream, ptrs, h->imgenc.packed);
    HIPCHK(hipGetLastError());
    h->imgenc.loaded = true;
    return HOPE_OK;
}

int hope_env_imgenc_forward(hope_env_t* h, const uint8_t* img, int64_t batch, float* token, float* feat_or_null, void* stream) {
    HOPE_ENTER(h, "hope_env_imgenc_forward");
    HOPE_NEED(h->imgenc.on, "hope_env_imgenc_forward", "the image encoder is off (hope_env_imgenc_enable first)");
    HOPE_NEED(h->imgenc.loaded, "hope_env_imgenc_forward", "no parameters yet (hope_env_imgenc_load first)");
    if (!img || !token) return fail(HOPE_EINVAL, "hope_env_imgenc_forward: null img / token");
    if (batch < 1 || batch > h->imgenc.max_batch)
        return fail(HOPE_EINVAL, "hope_env_imgenc_forward: batch must be 1 .. max_batch (" + std::to_string(h->imgenc.max_batch) + ")");
    if (((uintptr_t)img | (uintptr_t)token | (uintptr_t)feat_or_null) & 3)
        return fail(HOPE_EINVAL, "hope_env_imgenc_forward: misaligned buffer (img, token and feat 4 bytes)");
    HOPE_ON_DEVICE(h);
    float* const feat = feat_or_null ? feat_or_null : h->imgenc.feat;
    if (h->imgenc.act == 0) return imgenc_launch<0>(h, img, batch, token, feat, (hipStream_t)stream);
    return imgenc_launch<1>(h, img, batch, token, feat, (hipStream_t)stream);
}

int hope_debug_imgenc_stage(hope_env_t* h, int stage, const uint8_t* img, int64_t batch, float* token, float* feat, void* stream) {
    HOPE_ENTER(h, "hope_debug_imgenc_stage");
    HOPE_NEED(h->imgenc.on && h->imgenc.loaded, "hope_debug_imgenc_stage", "the image encoder is off or has no parameters yet");
    if ((stage != 0 && stage != 1) || !feat || (stage == 0 ? !img : !token) || batch < 1 || batch > h->imgenc.max_batch ||
        (((uintptr_t)img | (uintptr_t)token | (uintptr_t)feat) & 3))
        return fail(HOPE_EINVAL, "hope_debug_imgenc_stage: stage 0 (img -> feat) or 1 (feat -> token), non-null 4-byte aligned buffers, batch 1 .. max_batch");
    HOPE_ON_DEVICE(h);
    if (h->imgenc.act == 0) return imgenc_launch<0>(h, img, batch, token, feat, (hipStream_t)stream, 1 << stage);
    return imgenc_launch<1>(h, img, batch, token, feat, (hipStream_t)stream, 1 << stage);
}

int hope_imgenc_forward_host(const hope_imgenc_params_t* host_params, int act, const uint8_t* img, int64_t batch, float* token, float* feat_or_null) {
    const int rc = ie_forward_host(host_params, act, img, batch, token, feat_or_null);
    if (rc != HOPE_OK)
        return fail(rc, "hope_imgenc_forward_host: bad argument (a null parameter, image or token, act not 0 or 1, batch < 1, or img / token / feat not "
                        "aligned to 4 bytes)");
    return HOPE_OK;
}

}  // extern "C"
