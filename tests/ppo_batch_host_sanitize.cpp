// Stand-alone driver of the host twins of PPO's minibatch for sanitizer runs on the CPU (no device, no Python):
//   c++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -Iinclude -Ihope_amd/csrc tests/ppo_batch_host_sanitize.cpp -o ppo_batch_host_sanitize && ./ppo_batch_host_sanitize
// It runs pb_gather_host and pb_loss_host (hope_ppo_core.h; hope_ppo_*_host forward to them) over heap buffers of EXACTLY the call's
// size -- so a read or write past the last transition, the last item or a short last chunk of 64 items is an error -- with ring and
// minibatch sizes around the chunk boundary, indices in and out of range (-1, n T, +-2^40), and checks the gather against a plain
// recomputation and the sums of the loss against a long double sum of the per-item terms.  Exit code 0 = clean.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "hope_ppo_core.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }
static double uni() { return (double)(rnd() >> 11) / 9007199254740992.0; }
static void fill(std::vector<float>& v, double lo = -2.0, double hi = 2.0) { for (float& x : v) x = (float)(lo + uni() * (hi - lo)); }

#define FAIL(...) do { fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); return 1; } while (0)

int main() {
    long long calls = 0, words = 0;
    double worst = 0.0;
    const int shapes[][2] = {{1, 1}, {3, 5}, {70, 4}, {1030, 4}};
    for (const auto& nt : shapes) {
        const int n = nt[0], T = nt[1];
        const int64_t m = (int64_t)n * T;
        std::vector<float> lidar(m * RG_LIDAR), target(m * RG_TARGET), mask(m * RG_MASK), action(m * RG_PAIR), logp(m * RG_PAIR), reward(m), done(m), adv(m), vt(m);
        for (auto* v : {&lidar, &target, &mask, &action, &logp, &reward, &done, &adv, &vt}) fill(*v);
        const hope_ring_t R = {lidar.data(), target.data(), mask.data(), action.data(), logp.data(), reward.data(), done.data(), n, T};
        for (int64_t mb : {(int64_t)1, (int64_t)2, (int64_t)63, (int64_t)64, (int64_t)65, (int64_t)129, (int64_t)4097}) {
            std::vector<int64_t> index(mb);
            for (int64_t b = 0; b < mb; b++) index[b] = (int64_t)(uni() * (double)m);
            if (mb >= 63) { index[0] = -1; index[5] = m; index[31] = (int64_t)1 << 40; index[mb - 1] = -((int64_t)1 << 40); index[1] = 0; index[2] = m - 1; }
            std::vector<float> ol(mb * RG_LIDAR, 7.f), ot(mb * RG_TARGET, 7.f), om(mb * RG_MASK, 7.f), oa(mb * RG_PAIR, 7.f), olp(mb, 7.f), oadv(mb, 7.f), ovt(mb, 7.f);
            std::vector<int32_t> idx(mb, 7);
            const hope_ppo_batch_t O = {ol.data(), ot.data(), om.data(), oa.data(), olp.data(), oadv.data(), ovt.data(), idx.data()};
            if (pb_gather_host(&R, adv.data(), vt.data(), index.data(), mb, &O) != HOPE_OK) FAIL("gather refused n %d T %d mb %lld", n, T, (long long)mb);
            calls++;
            for (int64_t b = 0; b < mb; b++) {
                const int64_t r = index[b];
                const bool ok = r >= 0 && r < m;
                if (idx[b] != (ok ? (int32_t)r : -1)) FAIL("idx of item %lld", (long long)b);
                for (int e = 0; e < RG_LIDAR; e++) if (ol[b * RG_LIDAR + e] != (ok ? lidar[r * RG_LIDAR + e] : 0.f)) FAIL("lidar of item %lld", (long long)b);
                for (int e = 0; e < RG_TARGET; e++) if (ot[b * RG_TARGET + e] != (ok ? target[r * RG_TARGET + e] : 0.f)) FAIL("target of item %lld", (long long)b);
                for (int e = 0; e < RG_MASK; e++) if (om[b * RG_MASK + e] != (ok ? mask[r * RG_MASK + e] : 0.f)) FAIL("mask of item %lld", (long long)b);
                for (int e = 0; e < RG_PAIR; e++) if (oa[b * RG_PAIR + e] != (ok ? action[r * RG_PAIR + e] : 0.f)) FAIL("action of item %lld", (long long)b);
                if (olp[b] != (ok ? logp[2 * r] + logp[2 * r + 1] : 0.f) || oadv[b] != (ok ? adv[r] : 0.f) || ovt[b] != (ok ? vt[r] : 0.f))
                    FAIL("old_lp / adv / v_target of item %lld", (long long)b);
                words += PB_ITEM;
            }
            // the loss over the gathered action, adv and v_target, with an old_lp near the new log-probability
            std::vector<float> raw(mb * 2), value(mb), g_raw(mb * 2, 7.f), g_value(mb, 7.f);
            fill(raw, -1.5, 1.5); fill(value);
            for (int64_t b = 0; b < mb; b++) olp[b] = (float)(-2.0 + uni());
            const float ls[2] = {-0.3f, 0.2f};
            float g_ls[2] = {7.f, 7.f}, losses[2] = {7.f, 7.f};
            const double clip = 0.2;
            if (pb_loss_host(raw.data(), ls, value.data(), &O, mb, clip, g_raw.data(), g_ls, g_value.data(), losses) != HOPE_OK)
                FAIL("loss refused mb %lld", (long long)mb);
            calls++;
            long double s[4] = {0, 0, 0, 0}, a[4] = {0, 0, 0, 0};
            for (int64_t b = 0; b < mb; b++) {
                const PbItem o = pb_item(raw[2 * b], raw[2 * b + 1], ls[0], ls[1], value[b], oa[2 * b], oa[2 * b + 1], olp[b], oadv[b], ovt[b], clip, (double)mb);
                if (memcmp(&o.g0, &g_raw[2 * b], 4) || memcmp(&o.g1, &g_raw[2 * b + 1], 4) || memcmp(&o.gv, &g_value[b], 4)) FAIL("gradient of item %lld", (long long)b);
                const double t[4] = {o.actor, o.critic, o.ls0, o.ls1};
                for (int q = 0; q < 4; q++) { s[q] += t[q]; a[q] += fabs(t[q]); }
            }
            const double got[4] = {losses[0], losses[1], g_ls[0], g_ls[1]};
            for (int q = 0; q < 4; q++) {
                const long double want = q < 2 ? s[q] / mb : s[q], scale = q < 2 ? a[q] / mb : a[q];
                const double bound = (double)(fabsl(want) * 6.0e-8L + scale * 1.0e-12L + 1.0e-45L);          // one float32 rounding, the tree's error
                const double err = fabs(got[q] - (double)want);
                if (!(err <= bound)) FAIL("sum %d of mb %lld: %g against %Lg", q, (long long)mb, got[q], want);
                if (bound > 0 && err / bound > worst) worst = err / bound;
            }
        }
    }
    // refusals
    const hope_ppo_batch_t none = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    float one[2] = {0.f, 0.f};
    if (pb_loss_host(one, one, one, &none, 1, 0.2, one, one, one, one) != HOPE_EINVAL) FAIL("a null batch field was accepted");
    if (pb_gather_host(nullptr, one, one, nullptr, 1, &none) != HOPE_EINVAL) FAIL("a null ring was accepted");
    printf("clean: %lld calls, %lld gathered words, worst sum error %.3f of its bound\n", calls, words, worst);
    return 0;
}
