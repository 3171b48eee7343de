// Stand-alone driver of the host twins of SAC's update for sanitizer runs on the CPU (no device, no Python):
//   c++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -Iinclude -Ihope_amd/csrc tests/sac_update_host_sanitize.cpp -o sac_update_host_sanitize && ./sac_update_host_sanitize
// It runs su_sample_host, su_critic_host, su_seed_host and su_policy_host (hope_sac_core.h; hope_sac_*_host forward to them) over
// heap buffers of EXACTLY the call's size -- so a read or write past the last item or a short last chunk of 64 items is an error --
// at batch sizes around the chunk boundary, from bases offset by one float (4-byte aligned only) and float64 scalars at odd
// addresses, and checks the per-item words against the item functions and the sums against a long double sum of the per-item terms.
// Exit code 0 = clean.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "hope_sac_core.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }
static double uni() { return (double)(rnd() >> 11) / 9007199254740992.0; }

// a heap buffer of exactly `count` floats behind `offset` floats that belong to nobody's call
struct Buf {
    std::vector<float> store;
    float* p;
    Buf(size_t count, int offset, double lo = -2.0, double hi = 2.0) : store(count + (size_t)offset) {
        for (float& x : store) x = (float)(lo + uni() * (hi - lo));
        p = store.data() + offset;
    }
};

#define FAIL(...) do { fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); return 1; } while (0)

static bool near(double got, long double want, long double scale) {
    return fabs(got - (double)want) <= (double)(fabsl(want) * 6.0e-8L + scale * 1.0e-12L + 1.0e-45L);      // one float32 rounding, the tree's error
}

int main() {
    long long calls = 0;
    const double gamma = 0.99, target_entropy = -2.0, la = log(0.01) + 0.0123;
    for (int offset : {0, 1}) {
        for (int64_t b : {(int64_t)1, (int64_t)2, (int64_t)63, (int64_t)64, (int64_t)65, (int64_t)129, (int64_t)4097}) {
            const size_t n = (size_t)b;
            Buf raw(2 * n, offset, -1.5, 1.5), ls(2, offset, -0.5, 0.3), eps(2 * n, offset, -3.0, 3.0), action(2 * n, offset), lp(n, offset);
            Buf q1(n, offset), q2(n, offset), qt1(n, offset), qt2(n, offset), nlp(n, offset), reward(n, offset), done(n, offset), y(n, offset), g1(n, offset),
                g2(n, offset), cl(2, offset), s1(n, offset), s2(n, offset), G(2 * n, offset, -1e-2, 1e-2), g_raw(2 * n, offset), g_ls(2, offset), pl(2, offset);
            for (size_t i = 0; i < n; i++) {
                done.p[i] = (i % 4 == 1) ? 1.f : 0.f;
                if (i % 3 == 2) q2.p[i] = q1.p[i];                                   // ties of the min
                if (i % 5 == 0) { raw.p[2 * i] = 1.f; eps.p[2 * i] = 0.f; }           // a sample exactly on the bound
                if (i % 5 == 1) raw.p[2 * i + 1] = -1.f;
            }
            // the two float64 scalars at addresses that are not multiples of 8
            std::vector<unsigned char> scal(2 * sizeof(double) + 3);
            double* log_alpha = (double*)(scal.data() + 1 + (offset ? 2 : 0));
            double* g_la = (double*)((unsigned char*)log_alpha + sizeof(double));
            memcpy(log_alpha, &la, sizeof la);
            if (su_sample_host(raw.p, ls.p, eps.p, b, action.p, lp.p) != HOPE_OK) FAIL("sample refused b %lld", (long long)b);
            if (su_critic_host(q1.p, q2.p, qt1.p, qt2.p, nlp.p, reward.p, done.p, log_alpha, gamma, b, y.p, g1.p, g2.p, cl.p) != HOPE_OK)
                FAIL("critic refused b %lld", (long long)b);
            if (su_seed_host(q1.p, q2.p, b, s1.p, s2.p) != HOPE_OK) FAIL("seed refused b %lld", (long long)b);
            if (su_policy_host(raw.p, ls.p, eps.p, q1.p, q2.p, G.p, log_alpha, target_entropy, b, g_raw.p, g_ls.p, g_la, pl.p) != HOPE_OK)
                FAIL("policy refused b %lld", (long long)b);
            calls += 4;
            const SuStd s = su_std(ls.p[0], ls.p[1]);
            const double alpha64 = su_alpha64(la), alpha = su_alpha(alpha64);
            long double sc[2] = {0, 0}, sp[4] = {0, 0, 0, 0}, ap[4] = {0, 0, 0, 0};
            for (size_t i = 0; i < n; i++) {
                const SuDraw w = su_draw(raw.p[2 * i], raw.p[2 * i + 1], s, eps.p[2 * i], eps.p[2 * i + 1]);
                const float a0 = (float)w.a0, a1 = (float)w.a1, l = (float)w.lp;
                if (memcmp(&a0, &action.p[2 * i], 4) || memcmp(&a1, &action.p[2 * i + 1], 4) || memcmp(&l, &lp.p[i], 4)) FAIL("sample of item %zu", i);
                if (action.p[2 * i] < -1.f || action.p[2 * i] > 1.f) FAIL("action of item %zu outside the clamp", i);
                const SuCritic c = su_critic(q1.p[i], q2.p[i], qt1.p[i], qt2.p[i], nlp.p[i], reward.p[i], done.p[i], alpha, gamma, (double)b);
                if (memcmp(&c.y, &y.p[i], 4) || memcmp(&c.g1, &g1.p[i], 4) || memcmp(&c.g2, &g2.p[i], 4)) FAIL("critic of item %zu", i);
                sc[0] += c.t1; sc[1] += c.t2;
                const SuSeed sd = su_seed(q1.p[i], q2.p[i], (double)b);
                if (memcmp(&sd.s1, &s1.p[i], 4) || memcmp(&sd.s2, &s2.p[i], 4)) FAIL("seed of item %zu", i);
                if (fabs((double)sd.s1 + (double)sd.s2 + 1.0 / (double)b) > 1e-7 / (double)b) FAIL("seeds of item %zu do not add up to -1 / B", i);
                const SuPolicy p = su_policy(raw.p[2 * i], raw.p[2 * i + 1], s, eps.p[2 * i], eps.p[2 * i + 1], q1.p[i], q2.p[i], G.p[2 * i], G.p[2 * i + 1], alpha,
                                             target_entropy, (double)b);
                if (memcmp(&p.g0, &g_raw.p[2 * i], 4) || memcmp(&p.g1, &g_raw.p[2 * i + 1], 4)) FAIL("g_raw of item %zu", i);
                if (fabsf(raw.p[2 * i]) > 1.f && g_raw.p[2 * i] != 0.f) FAIL("a raw beyond the clamp has a gradient, item %zu", i);
                const double t[4] = {p.actor, p.entropy, p.ls0, p.ls1};
                for (int q = 0; q < 4; q++) { sp[q] += t[q]; ap[q] += fabs(t[q]); }
            }
            double ga;
            memcpy(&ga, g_la, sizeof ga);
            if (!near(cl.p[0], sc[0] / b, sc[0] / b) || !near(cl.p[1], sc[1] / b, sc[1] / b)) FAIL("critic losses of b %lld", (long long)b);
            if (!near(pl.p[0], sp[0] / b, ap[0] / b) || !near(g_ls.p[0], sp[2], ap[2]) || !near(g_ls.p[1], sp[3], ap[3])) FAIL("policy sums of b %lld", (long long)b);
            if (fabs(ga - (double)(alpha64 * sp[1] / b)) > 1e-12 * (double)(alpha64 * ap[1] / b)) FAIL("g_log_alpha of b %lld", (long long)b);
            if ((float)ga != pl.p[1]) FAIL("the temperature loss of b %lld is not g_log_alpha rounded", (long long)b);
        }
    }
    // refusals
    float one[2] = {0.f, 0.f};
    double d = 0.0;
    if (su_sample_host(nullptr, one, one, 1, one, one) != HOPE_EINVAL || su_sample_host(one, one, one, 0, one, one) != HOPE_EINVAL) FAIL("sample accepted a bad call");
    if (su_critic_host(one, one, one, one, one, one, one, &d, NAN, 1, one, one, one, one) != HOPE_EINVAL) FAIL("critic accepted a NaN gamma");
    if (su_seed_host(one, nullptr, 1, one, one) != HOPE_EINVAL) FAIL("seed accepted a null q2");
    if (su_policy_host(one, one, one, one, one, one, &d, INFINITY, 1, one, one, &d, one) != HOPE_EINVAL) FAIL("policy accepted an infinite target_entropy");
    printf("clean: %lld calls\n", calls);
    return 0;
}
