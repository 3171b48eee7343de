// Stand-alone driver of the transition ring's host twins for sanitizer runs on the CPU (no device, no Python):
//   c++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -Iinclude -Ihope_amd/csrc tests/ring_host_sanitize.cpp -o ring_host_sanitize && ./ring_host_sanitize
// It runs rg_before_host, rg_after_host and rg_sample_host (hope_ring_core.h; hope_ring_*_host forward to them) over heap buffers of
// EXACTLY the call's size -- so a read or write past the last scene, the last column, a short last chunk of 64 rows or the last batch
// item is an error -- with scene counts around the chunk boundary, T of 1 up to 16, wrapped heads, float32 and float64 rewards, with and
// without the tally, supplied (also out-of-range) and drawn indices, and checks the outputs against a plain recomputation.
// Exit code 0 = clean.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "hope_ring_core.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }
static double uni() { return (double)(rnd() >> 11) / 9007199254740992.0; }
static void fill(std::vector<float>& v) { for (float& x : v) x = (float)(uni() * 4.0 - 2.0); }

#define FAIL(...) do { fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); return 1; } while (0)

int main() {
    long long calls = 0, words = 0;
    double worst_sum = 0.0;
    for (int n : {1, 2, 63, 64, 65, 127, 129, 193, 4097}) {
        for (int T : {1, 2, 5, 16}) {
            const size_t c = (size_t)n * T;
            std::vector<float> lidar(c * RG_LIDAR, 7.f), target(c * RG_TARGET, 7.f), mask(c * RG_MASK, 7.f), action(c * RG_PAIR, 7.f), logp(c * RG_PAIR, 7.f),
                reward(c, 7.f), done(c, 7.f);
            const hope_ring_t R = {lidar.data(), target.data(), mask.data(), action.data(), logp.data(), reward.data(), done.data(), n, T};
            int64_t counts[2] = {0, 0}, want_counts[2] = {0, 0};
            double rsum[1] = {0.0};
            long double exact = 0.0L, scale = 0.0L;
            int head = 0, size = 0;
            for (int step = 0; step < T + 3; step++) {
                std::vector<float> il((size_t)n * RG_LIDAR), it((size_t)n * RG_TARGET), im((size_t)n * RG_MASK), ia((size_t)n * RG_PAIR), ip((size_t)n * RG_PAIR), r32(n);
                std::vector<double> r64(n);
                std::vector<uint8_t> dn(n);
                std::vector<int32_t> st(n);
                fill(il); fill(it); fill(im); fill(ia); fill(ip);
                for (int i = 0; i < n; i++) { r64[i] = uni() * 6.0 - 3.0; r32[i] = (float)r64[i]; dn[i] = uni() < 0.3 ? (uint8_t)(1 + rnd() % 3) : 0; st[i] = (int32_t)(rnd() % 6); }
                const bool f64 = step % 2, tally = step % 3 != 2;
                if (rg_before_host(&R, head, il.data(), it.data(), im.data(), ia.data(), ip.data()) != HOPE_OK) FAIL("rg_before_host failed");
                if (rg_after_host(&R, head, f64 ? (const void*)r64.data() : (const void*)r32.data(), f64, dn.data(), tally ? st.data() : nullptr, tally ? counts : nullptr,
                                  tally ? rsum : nullptr) != HOPE_OK)
                    FAIL("rg_after_host failed");
                for (int i = 0; i < n; i++) {
                    const size_t cell = (size_t)i * T + head;
                    if (memcmp(&lidar[cell * RG_LIDAR], &il[(size_t)i * RG_LIDAR], RG_LIDAR * 4) || memcmp(&target[cell * RG_TARGET], &it[(size_t)i * RG_TARGET], RG_TARGET * 4) ||
                        memcmp(&mask[cell * RG_MASK], &im[(size_t)i * RG_MASK], RG_MASK * 4) || memcmp(&action[cell * RG_PAIR], &ia[(size_t)i * RG_PAIR], 8) ||
                        memcmp(&logp[cell * RG_PAIR], &ip[(size_t)i * RG_PAIR], 8))
                        FAIL("before half of scene %d differs (n %d, T %d)", i, n, T);
                    if (reward[cell] != r32[i] || done[cell] != (float)dn[i]) FAIL("after half of scene %d differs (n %d, T %d)", i, n, T);
                    if (tally) {
                        want_counts[0] += dn[i] != 0; want_counts[1] += st[i] == 2;
                        const long double v = f64 ? (long double)r64[i] : (long double)r32[i];
                        exact += v; scale += fabsl(v);
                    }
                }
                if (counts[0] != want_counts[0] || counts[1] != want_counts[1]) FAIL("counts differ (n %d, T %d)", n, T);
                const double rel = fabs((double)((long double)rsum[0] - exact)) / (double)(scale + 1e-300L);
                if (rel > worst_sum) worst_sum = rel;
                if (!(rel < 1e-14)) FAIL("reward_sum off by %g of the scale (n %d, T %d)", rel, n, T);
                head = (head + 1) % T; size = size + 1 < T ? size + 1 : T;
                calls += 2; words += (long long)n * (RG_ROW + 2);
                // batches from the ring as it is now
                std::vector<float> ll((size_t)n * RG_LIDAR), lt((size_t)n * RG_TARGET), lm((size_t)n * RG_MASK);
                fill(ll); fill(lt); fill(lm);
                for (int batch : {1, 32, 65}) {
                    const bool supplied = (step + batch) % 2;
                    std::vector<int32_t> s(batch), j(batch), idx((size_t)batch * 3, 7);
                    for (int b = 0; b < batch; b++) { s[b] = (int32_t)(rnd() % n); j[b] = (int32_t)(rnd() % size); }
                    j[0] = size - 1;
                    if (batch > 4) { s[1] = -1; s[2] = n; j[3] = size; j[4] = -1; }
                    std::vector<float> ol((size_t)batch * RG_LIDAR, 7.f), ot((size_t)batch * RG_TARGET, 7.f), om((size_t)batch * RG_MASK, 7.f), nl((size_t)batch * RG_LIDAR, 7.f),
                        nt((size_t)batch * RG_TARGET, 7.f), nm((size_t)batch * RG_MASK, 7.f), oa((size_t)batch * RG_PAIR, 7.f), orw(batch, 7.f), od(batch, 7.f);
                    const hope_ring_batch_t O = {ol.data(), ot.data(), om.data(), nl.data(), nt.data(), nm.data(), oa.data(), orw.data(), od.data(), idx.data()};
                    const uint64_t seed = rnd(), counter = rnd();
                    if (rg_sample_host(&R, head, size, batch, supplied ? s.data() : nullptr, supplied ? j.data() : nullptr, seed, counter, ll.data(), lt.data(), lm.data(), &O) !=
                        HOPE_OK)
                        FAIL("rg_sample_host failed");
                    for (int b = 0; b < batch; b++) {
                        const int64_t sb = supplied ? s[b] : (int64_t)rg_draw(seed, counter, (uint64_t)b, 0, (uint32_t)n);
                        const int64_t jb = supplied ? j[b] : (int64_t)rg_draw(seed, counter, (uint64_t)b, 1, (uint32_t)size);
                        if (!supplied && (sb < 0 || sb >= n || jb < 0 || jb >= size)) FAIL("a draw out of range");
                        if (sb < 0 || sb >= n || jb < 0 || jb >= size) {
                            if (idx[3 * b] != -1 || idx[3 * b + 1] != -1 || idx[3 * b + 2] != -1 || orw[b] != 0.f || od[b] != 0.f || ol[(size_t)b * RG_LIDAR] != 0.f ||
                                nm[(size_t)b * RG_MASK + RG_MASK - 1] != 0.f || oa[(size_t)b * 2 + 1] != 0.f)
                                FAIL("a refused row is not flagged");
                            continue;
                        }
                        const int t = (int)(((head - size + jb) % T + T) % T), jn = (int)(jb + 1 < size ? jb + 1 : size - 1), tn = ((head - size + jn) % T + T) % T;
                        const bool newest = jb == size - 1;
                        const size_t cell = (size_t)sb * T + t, ncell = (size_t)sb * T + tn;
                        if (idx[3 * b] != sb || idx[3 * b + 1] != t || idx[3 * b + 2] != (newest ? -1 : tn)) FAIL("idx of item %d differs", b);
                        if (memcmp(&ol[(size_t)b * RG_LIDAR], &lidar[cell * RG_LIDAR], RG_LIDAR * 4) || memcmp(&ot[(size_t)b * RG_TARGET], &target[cell * RG_TARGET], RG_TARGET * 4) ||
                            memcmp(&om[(size_t)b * RG_MASK], &mask[cell * RG_MASK], RG_MASK * 4) || memcmp(&oa[(size_t)b * 2], &action[cell * 2], 8) || orw[b] != reward[cell] ||
                            od[b] != done[cell])
                            FAIL("obs of item %d differs", b);
                        const float* wl = newest ? &ll[(size_t)sb * RG_LIDAR] : &lidar[ncell * RG_LIDAR];
                        const float* wt = newest ? &lt[(size_t)sb * RG_TARGET] : &target[ncell * RG_TARGET];
                        const float* wm = newest ? &lm[(size_t)sb * RG_MASK] : &mask[ncell * RG_MASK];
                        if (memcmp(&nl[(size_t)b * RG_LIDAR], wl, RG_LIDAR * 4) || memcmp(&nt[(size_t)b * RG_TARGET], wt, RG_TARGET * 4) || memcmp(&nm[(size_t)b * RG_MASK], wm, RG_MASK * 4))
                            FAIL("next_obs of item %d differs", b);
                    }
                    calls++; words += (long long)batch * (RG_ITEM + 3);
                }
            }
        }
    }
    // misuse
    float x[RG_LIDAR] = {0};
    int32_t i3[3];
    uint8_t d1[1] = {0};
    int32_t s1[1] = {0};
    int64_t cn[2] = {0, 0};
    double rs[1] = {0.0};
    hope_ring_t R = {x, x, x, x, x, x, x, 1, 1};
    const hope_ring_batch_t O = {x, x, x, x, x, x, x, x, x, i3};
    hope_ring_t bad = R;
    bad.done = nullptr;
    if (rg_before_host(nullptr, 0, x, x, x, x, x) != HOPE_EINVAL || rg_before_host(&bad, 0, x, x, x, x, x) != HOPE_EINVAL) return 1;
    if (rg_before_host(&R, 1, x, x, x, x, x) != HOPE_EINVAL || rg_before_host(&R, -1, x, x, x, x, x) != HOPE_EINVAL) return 1;
    if (rg_before_host(&R, 0, x, x, nullptr, x, x) != HOPE_EINVAL) return 1;
    if (rg_after_host(&R, 0, nullptr, 0, d1, nullptr, nullptr, nullptr) != HOPE_EINVAL || rg_after_host(&R, 1, x, 0, d1, nullptr, nullptr, nullptr) != HOPE_EINVAL) return 1;
    if (rg_after_host(&R, 0, x, 0, d1, s1, cn, nullptr) != HOPE_EINVAL || rg_after_host(&R, 0, x, 0, d1, nullptr, cn, rs) != HOPE_EINVAL) return 1;
    if (rg_sample_host(&R, 1, 1, 1, nullptr, nullptr, 0, 0, x, x, x, &O) != HOPE_EINVAL || rg_sample_host(&R, 0, 2, 1, nullptr, nullptr, 0, 0, x, x, x, &O) != HOPE_EINVAL) return 1;
    if (rg_sample_host(&R, 0, 0, 1, nullptr, nullptr, 0, 0, x, x, x, &O) != HOPE_EINVAL || rg_sample_host(&R, 0, 1, 0, nullptr, nullptr, 0, 0, x, x, x, &O) != HOPE_EINVAL) return 1;
    if (rg_sample_host(&R, 0, 1, 1, s1, nullptr, 0, 0, x, x, x, &O) != HOPE_EINVAL || rg_sample_host(&R, 0, 1, 1, nullptr, nullptr, 0, 0, x, x, x, nullptr) != HOPE_EINVAL) return 1;
    if (rg_sample_host(&R, 0, 1, 1, nullptr, nullptr, 0, 0, x, nullptr, x, &O) != HOPE_EINVAL) return 1;
    if (rg_sample_host(&R, 0, 1, 1, nullptr, nullptr, 0, 0, x, x, x, &O) != HOPE_OK || i3[0] != 0 || i3[2] != -1) return 1;
    if (cn[0] != 0 || rs[0] != 0.0) return 1;
    printf("ring host twins: %lld calls, %lld words, worst sum error %.3g of the scale, clean\n", calls, words, worst_sum);
    return calls >= 500 && words > 1000000 ? 0 : 1;
}
