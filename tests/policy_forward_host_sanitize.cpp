// Stand-alone driver of the host twin of the fused policy forward for sanitizer runs on the CPU (no device, no Python):
//   c++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -Iinclude -Ihope_amd/csrc tests/policy_forward_host_sanitize.cpp -o policy_forward_host_sanitize && ./policy_forward_host_sanitize
// It runs pc_forward_host (hope_policy_core.h; hope_policy_forward_host forwards to it) over heap buffers of EXACTLY each tensor's
// size -- the parameters, the inputs and the output, so a read or write one element past any of them is an error -- at B = 1, 33 and
// 65 with T = 3 and 4, actor and critic heads, from bases offset by one float, and checks that a row's words do not depend on the
// batch it is in, that the output is finite and within the tanh's range, and that the refused shapes are refused.  Exit code 0 = clean.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "hope_policy_core.h"

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
    for (int T : {3, 4})
        for (int out_dim : {2, 1})
            for (int offset : {0, 1}) {
                const int tanh_out = out_dim == 2;
                const PcLayout L = pc_layout(T, out_dim);
                std::vector<Buf> w;
                w.reserve(PC_NPARAM);
                const float* ptr[PC_NPARAM];
                for (int i = 0; i < PC_NPARAM; ++i) {
                    const double s = L.k_in[i] == 1 ? 0.05 : 1.2 / sqrt((double)L.k_in[i]);
                    w.emplace_back((size_t)L.n_out[i] * L.k_in[i], offset, -s, s);
                    ptr[i] = w.back().p;
                }
                for (int i : {(int)PC_LN1_G, (int)PC_LN2_G})
                    for (int c = 0; c < PC_E; ++c) w[i].p[c] += 1.0f;
                hope_policy_params_t P;
                memcpy(&P, ptr, sizeof P);
                std::vector<float> row0(out_dim);
                for (int64_t b : {(int64_t)65, (int64_t)33, (int64_t)1}) {
                    // the same generator state for every batch size: row 0 of each call sees the same inputs
                    rng_state = 0x1234567ull + (uint64_t)T;
                    const size_t n = (size_t)b;
                    Buf lidar(n * PC_LIDAR, offset, -2.0, 2.0), target(n * PC_TARGET, offset, -2.0, 2.0), mask(n * PC_MASK, offset, 0.0, 1.0),
                        img(T == 4 ? n * PC_E : 1, offset, -2.0, 2.0), out(n * out_dim, offset, 7.0, 7.0);
                    for (size_t i = 0; i < n * PC_MASK; ++i) mask.p[i] = mask.p[i] < 0.6f ? 1.0f : 0.0f;
                    for (int k = 0; k < PC_MASK; ++k) mask.p[k] = 0.0f;                        // an all-zero row
                    if (n > 1) { lidar.p[PC_LIDAR + 3] = 10.0f; target.p[PC_TARGET + 1] = -10.0f; }
                    // row 0's inputs must be equal across batch sizes: draw them last, from a fixed state
                    rng_state = 0xABCDEFull;
                    for (int k = 0; k < PC_LIDAR; ++k) lidar.p[k] = (float)(-2.0 + 4.0 * uni());
                    for (int k = 0; k < PC_TARGET; ++k) target.p[k] = (float)(-2.0 + 4.0 * uni());
                    if (T == 4) for (int k = 0; k < PC_E; ++k) img.p[k] = (float)(-2.0 + 4.0 * uni());
                    if (pc_forward_host(&P, T, out_dim, tanh_out, lidar.p, target.p, mask.p, T == 4 ? img.p : nullptr, b, out.p) != HOPE_OK)
                        FAIL("pc_forward_host refused T %d out_dim %d b %lld", T, out_dim, (long long)b);
                    ++calls;
                    for (size_t i = 0; i < n * out_dim; ++i)
                        if (!isfinite(out.p[i]) || (tanh_out && fabsf(out.p[i]) > 1.0f)) FAIL("output %zu = %g (T %d, b %lld)", i, out.p[i], T, (long long)b);
                    if (b == 65) memcpy(row0.data(), out.p, sizeof(float) * out_dim);
                    else if (memcmp(row0.data(), out.p, sizeof(float) * out_dim) != 0) FAIL("row 0 depends on the batch size (T %d, b %lld)", T, (long long)b);
                }
                // refused: shapes that are not compiled in, a missing or surplus image token, a null tensor, an empty batch
                Buf lidar(PC_LIDAR, 0, -1, 1), target(PC_TARGET, 0, -1, 1), mask(PC_MASK, 0, 0, 1), img(PC_E, 0, -1, 1), out(2, 0, 7, 7);
                const float* good_img = T == 4 ? img.p : nullptr;
                const float* bad_img = T == 4 ? nullptr : img.p;
                hope_policy_params_t Q = P;
                Q.qkv_w = nullptr;
                if (pc_forward_host(&P, 2, out_dim, tanh_out, lidar.p, target.p, mask.p, good_img, 1, out.p) != HOPE_EINVAL ||
                    pc_forward_host(&P, T, 3, tanh_out, lidar.p, target.p, mask.p, good_img, 1, out.p) != HOPE_EINVAL ||
                    pc_forward_host(&P, T, out_dim, 2, lidar.p, target.p, mask.p, good_img, 1, out.p) != HOPE_EINVAL ||
                    pc_forward_host(&P, T, out_dim, tanh_out, lidar.p, target.p, mask.p, bad_img, 1, out.p) != HOPE_EINVAL ||
                    pc_forward_host(&Q, T, out_dim, tanh_out, lidar.p, target.p, mask.p, good_img, 1, out.p) != HOPE_EINVAL ||
                    pc_forward_host(nullptr, T, out_dim, tanh_out, lidar.p, target.p, mask.p, good_img, 1, out.p) != HOPE_EINVAL ||
                    pc_forward_host(&P, T, out_dim, tanh_out, nullptr, target.p, mask.p, good_img, 1, out.p) != HOPE_EINVAL ||
                    pc_forward_host(&P, T, out_dim, tanh_out, lidar.p, target.p, mask.p, good_img, 0, out.p) != HOPE_EINVAL)
                    FAIL("a bad call was accepted (T %d)", T);
                if (out.p[0] != 7.0f || out.p[1] != 7.0f) FAIL("a refused call wrote to out");
            }
    printf("clean: %lld calls\n", calls);
    return 0;
}
