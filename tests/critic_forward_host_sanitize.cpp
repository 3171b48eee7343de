// Stand-alone driver of the host twin of the critics' fused forward for sanitizer runs on the CPU (no device, no Python):
//   c++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -Iinclude -Ihope_amd/csrc tests/critic_forward_host_sanitize.cpp -o critic_forward_host_sanitize && ./critic_forward_host_sanitize
// It runs cc_forward_host (hope_critic_core.h; hope_critic_forward_host forwards to it) over heap buffers of EXACTLY each tensor's
// size -- the parameters (none at all behind the action tensors of a net without the token), the inputs and the output, so a read or
// write one element past any of them is an error -- at B = 1, 33 and 65 for the four shapes (T = 3, 4 with the image, 4 with the
// action, 5), from bases offset by one float, and checks that a row's word does not depend on the batch it is in, that without the
// action token the words are pc_forward_host's (out_dim 1, no tanh), that the output is finite, and that bad calls are refused.
// Exit code 0 = clean.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "hope_critic_core.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }
static double uni() { return (double)(rnd() >> 11) / 9007199254740992.0; }

// a heap buffer of exactly `count` floats behind `offset` floats that belong to nobody's call
struct Buf {
    std::vector<float> store;
    float* p;
    Buf(size_t count, int offset, double lo, double hi) : store(count + (size_t)offset) {
        for (float& x : store) x = (float)(lo + uni() * (hi - lo));
        p = store.data() + offset;
    }
};

#define FAIL(...) do { fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); return 1; } while (0)

int main() {
    long long calls = 0;
    for (int has_img : {0, 1})
        for (int has_action : {0, 1})
            for (int offset : {0, 1}) {
                const CcLayout L = cc_layout(has_img, has_action);
                const int T = cc_tokens(has_img, has_action);
                std::vector<Buf> w;
                w.reserve(CC_NPARAM);
                const float* ptr[CC_NPARAM];
                for (int i = 0; i < CC_NPARAM; ++i) {
                    const double s = L.k_in[i] == 1 ? 0.05 : 1.2 / sqrt((double)L.k_in[i]);
                    w.emplace_back((size_t)L.n_out[i] * L.k_in[i], offset, -s, s);
                    ptr[i] = L.n_out[i] ? w.back().p : nullptr;
                }
                for (int i : {(int)PC_LN1_G, (int)PC_LN2_G})
                    for (int c = 0; c < PC_E; ++c) w[i].p[c] += 1.0f;
                hope_critic_params_t P;
                memcpy(&P, ptr, sizeof P);
                float row0 = 0.0f;
                for (int64_t b : {(int64_t)65, (int64_t)33, (int64_t)1}) {
                    rng_state = 0x1234567ull + (uint64_t)T;
                    const size_t n = (size_t)b;
                    Buf lidar(n * PC_LIDAR, offset, -2.0, 2.0), target(n * PC_TARGET, offset, -2.0, 2.0), mask(n * PC_MASK, offset, 0.0, 1.0),
                        img(has_img ? n * PC_E : 1, offset, -2.0, 2.0), action(has_action ? n * CC_ACTION : 1, offset, -1.0, 1.0), out(n, offset, 7.0, 7.0);
                    for (size_t i = 0; i < n * PC_MASK; ++i) mask.p[i] = mask.p[i] < 0.6f ? 1.0f : 0.0f;
                    for (int k = 0; k < PC_MASK; ++k) mask.p[k] = 0.0f;                        // an all-zero row
                    if (n > 1) { lidar.p[PC_LIDAR + 3] = 10.0f; target.p[PC_TARGET + 1] = -10.0f; }
                    // row 0's inputs must be equal across batch sizes: draw them last, from a fixed state
                    rng_state = 0xABCDEFull;
                    for (int k = 0; k < PC_LIDAR; ++k) lidar.p[k] = (float)(-2.0 + 4.0 * uni());
                    for (int k = 0; k < PC_TARGET; ++k) target.p[k] = (float)(-2.0 + 4.0 * uni());
                    if (has_img) for (int k = 0; k < PC_E; ++k) img.p[k] = (float)(-2.0 + 4.0 * uni());
                    if (has_action) { action.p[0] = 1.0f; action.p[1] = -1.0f; }
                    const float *ip = has_img ? img.p : nullptr, *ap = has_action ? action.p : nullptr;
                    if (cc_forward_host(&P, has_img, has_action, lidar.p, target.p, mask.p, ip, ap, b, out.p) != HOPE_OK)
                        FAIL("cc_forward_host refused img %d action %d b %lld", has_img, has_action, (long long)b);
                    ++calls;
                    for (size_t i = 0; i < n; ++i)
                        if (!isfinite(out.p[i])) FAIL("output %zu = %g (T %d, b %lld)", i, out.p[i], T, (long long)b);
                    if (b == 65) row0 = out.p[0];
                    else if (memcmp(&row0, out.p, sizeof(float)) != 0) FAIL("row 0 depends on the batch size (T %d, b %lld)", T, (long long)b);
                    if (!has_action) {                                                         // the policy twin's words
                        hope_policy_params_t Q;
                        memcpy(&Q, ptr, sizeof Q);
                        Buf ref(n, offset, 7.0, 7.0);
                        if (pc_forward_host(&Q, T, 1, 0, lidar.p, target.p, mask.p, ip, b, ref.p) != HOPE_OK || memcmp(ref.p, out.p, n * sizeof(float)) != 0)
                            FAIL("not the policy twin's words (T %d, b %lld)", T, (long long)b);
                    }
                }
                // refused: flags out of range, an image token, action or action tensors that do not go with them, a null tensor, an empty batch
                Buf lidar(PC_LIDAR, 0, -1, 1), target(PC_TARGET, 0, -1, 1), mask(PC_MASK, 0, 0, 1), img(PC_E, 0, -1, 1), action(CC_ACTION, 0, -1, 1), out(1, 0, 7, 7);
                const float *gi = has_img ? img.p : nullptr, *bi = has_img ? nullptr : img.p;
                const float *ga = has_action ? action.p : nullptr, *ba = has_action ? nullptr : action.p;
                hope_critic_params_t Q = P, R = P;
                Q.qkv_w = nullptr;
                R.action_w2 = has_action ? nullptr : lidar.p;
                if (cc_forward_host(&P, 2, has_action, lidar.p, target.p, mask.p, gi, ga, 1, out.p) != HOPE_EINVAL ||
                    cc_forward_host(&P, has_img, -1, lidar.p, target.p, mask.p, gi, ga, 1, out.p) != HOPE_EINVAL ||
                    cc_forward_host(&P, has_img, has_action, lidar.p, target.p, mask.p, bi, ga, 1, out.p) != HOPE_EINVAL ||
                    cc_forward_host(&P, has_img, has_action, lidar.p, target.p, mask.p, gi, ba, 1, out.p) != HOPE_EINVAL ||
                    cc_forward_host(&Q, has_img, has_action, lidar.p, target.p, mask.p, gi, ga, 1, out.p) != HOPE_EINVAL ||
                    cc_forward_host(&R, has_img, has_action, lidar.p, target.p, mask.p, gi, ga, 1, out.p) != HOPE_EINVAL ||
                    cc_forward_host(nullptr, has_img, has_action, lidar.p, target.p, mask.p, gi, ga, 1, out.p) != HOPE_EINVAL ||
                    cc_forward_host(&P, has_img, has_action, nullptr, target.p, mask.p, gi, ga, 1, out.p) != HOPE_EINVAL ||
                    cc_forward_host(&P, has_img, has_action, lidar.p, target.p, mask.p, gi, ga, 0, out.p) != HOPE_EINVAL)
                    FAIL("a bad call was accepted (T %d)", T);
                if (out.p[0] != 7.0f) FAIL("a refused call wrote to out");
            }
    printf("clean: %lld calls\n", calls);
    return 0;
}
