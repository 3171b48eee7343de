// Stand-alone driver of the advantage block's host twins for sanitizer runs on the CPU (no device, no Python):
//   c++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -Iinclude -Ihope_amd/csrc tests/gae_host_sanitize.cpp -o gae_host_sanitize && ./gae_host_sanitize
// It runs ga_host and ga_normalize_host (hope_gae_core.h; hope_gae_host / hope_adv_normalize_host forward to them) over buffers of
// EXACTLY the call's size -- so a read or write past a short last chunk of 64 rows, or past column T - 1, is an error -- with every flag
// combination, row counts around the chunk boundary and the tree's pass-through nodes, T of 1 up to 17, every `done` pattern, and
// checks the outputs against a plain long-double recomputation.  Exit code 0 = clean.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "hope_gae_core.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }
static double uni() { return (double)(rnd() >> 11) / 9007199254740992.0; }

int main() {
    long long calls = 0, elems = 0;
    double worst_adv = 0.0, worst_sum = 0.0;
    const double gamma = 0.98, lam = 0.95;
    for (int rows : {1, 2, 63, 64, 65, 127, 128, 129, 193, 321, 385, 4097}) {
        for (int T : {1, 2, 5, 16, 17}) {
            for (int pattern = 0; pattern < 5; pattern++) {          // none, all, newest column, column 0, random 20 %
                const size_t n = (size_t)rows * T;
                // exact-size buffers: the sanitizer sees the first byte past the call
                std::vector<float> r(n), d(n), v(n), vt(n), vl(rows), adv(n, 7.f), tgt(n, 7.f), delta(n, 7.f), out(n, 7.f);
                for (size_t i = 0; i < n; i++) {
                    r[i] = (float)(uni() * 4.0 - 2.0); v[i] = (float)(uni() * 6.0 - 3.0); vt[i] = (float)(uni() * 6.0 - 3.0);
                    const int t = (int)(i % T);
                    d[i] = pattern == 1 || (pattern == 2 && t == T - 1) || (pattern == 3 && t == 0) || (pattern == 4 && uni() < 0.2) ? 1.f : 0.f;
                }
                for (int i = 0; i < rows; i++) vl[i] = (float)(uni() * 6.0 - 3.0);
                const uint32_t flags = (uint32_t)(calls % 4);          // 0, SUMS, NORMALIZE, both
                double sums[3] = {-1.0, -1.0, -1.0};
                const bool with_delta = calls % 3 != 0, with_sums = calls % 5 != 0;
                int rc = ga_host(r.data(), d.data(), v.data(), vl.data(), vt.data(), rows, T, gamma, lam, flags, adv.data(), tgt.data(),
                                 with_sums ? sums : nullptr, with_delta ? delta.data() : nullptr);
                if (rc != HOPE_OK) { fprintf(stderr, "ga_host returned %d\n", rc); return 1; }
                // the plain estimate, recomputed in long double
                std::vector<float> plain(n);
                long double e0 = 0.0L, e1 = 0.0L, a0 = 0.0L, a1 = 0.0L;
                {
                    std::vector<float> tg2(n);
                    rc = ga_host(r.data(), d.data(), v.data(), vl.data(), vt.data(), rows, T, gamma, lam, 0, plain.data(), tg2.data(), nullptr, nullptr);
                    if (rc != HOPE_OK || memcmp(tg2.data(), tgt.data(), n * sizeof(float)) != 0) { fprintf(stderr, "v_target depends on the flags\n"); return 1; }
                }
                for (int i = 0; i < rows; i++) {
                    long double gae = 0.0L;
                    for (int t = T - 1; t >= 0; t--) {
                        const size_t k = (size_t)i * T + t;
                        const long double nv = t == T - 1 ? vl[i] : v[k + 1];
                        const long double dl = (long double)r[k] + (long double)gamma * (1.0L - d[k]) * nv - v[k];
                        gae = dl + (long double)gamma * lam * gae * (1.0L - d[k]);
                        const double err = fabs((double)(plain[k] - gae));
                        if (err > worst_adv) worst_adv = err;
                        // float32 roundings of delta along the row: at most T of them, each half an ulp of a value below 2^4
                        if (!(err < 1e-5 * T)) { fprintf(stderr, "adv[%d][%d] off by %g\n", i, t, err); return 1; }
                        if (tgt[k] != plain[k] + vt[k]) { fprintf(stderr, "v_target[%d][%d] is not adv + value_target\n", i, t); return 1; }
                        e0 += plain[k]; e1 += (long double)plain[k] * plain[k];
                        a0 += fabsl((long double)plain[k]); a1 += (long double)plain[k] * plain[k];
                    }
                }
                if (flags && with_sums) {
                    const double err0 = fabs((double)(sums[0] - e0)), err1 = fabs((double)(sums[1] - e1));
                    const double rel = fmax(err0 / (double)(a0 + 1e-300L), err1 / (double)(a1 + 1e-300L));
                    if (rel > worst_sum) worst_sum = rel;
                    if (!(rel < 1e-14) || sums[2] != (double)n) { fprintf(stderr, "sums off by %g of the scale (rows %d, T %d)\n", rel, rows, T); return 1; }
                } else if (sums[0] != -1.0 || sums[2] != -1.0) { fprintf(stderr, "sums written without the flag\n"); return 1; }
                if (flags & HOPE_GAE_NORMALIZE) {                     // the fused call is the split call
                    double s2[3];
                    std::vector<float> a2(n), t2(n);
                    float ms[2];
                    rc = ga_host(r.data(), d.data(), v.data(), vl.data(), vt.data(), rows, T, gamma, lam, HOPE_GAE_SUMS, a2.data(), t2.data(), s2, nullptr);
                    if (rc == HOPE_OK) rc = ga_normalize_host(a2.data(), (int64_t)n, s2, out.data(), ms);
                    if (rc != HOPE_OK || memcmp(out.data(), adv.data(), n * sizeof(float)) != 0) { fprintf(stderr, "fused and split calls differ\n"); return 1; }
                    if (memcmp(a2.data(), plain.data(), n * sizeof(float)) != 0) { fprintf(stderr, "SUMS changed adv\n"); return 1; }
                    rc = ga_normalize_host(a2.data(), (int64_t)n, s2, a2.data(), nullptr);     // in place
                    if (rc != HOPE_OK || memcmp(a2.data(), adv.data(), n * sizeof(float)) != 0) { fprintf(stderr, "in-place normalisation differs\n"); return 1; }
                    if (n == 1 && (adv[0] != 0.f || ms[1] != 0.f)) { fprintf(stderr, "a single element must normalise to 0\n"); return 1; }
                } else if (memcmp(adv.data(), plain.data(), n * sizeof(float)) != 0) { fprintf(stderr, "adv depends on the flags\n"); return 1; }
                calls++; elems += (long long)n;
            }
        }
    }
    // misuse
    float x[4] = {0}, y[4], z[4];
    double s[3] = {0.0, 0.0, 1.0};
    float ms[2];
    if (ga_host(nullptr, x, x, x, x, 1, 1, gamma, lam, 0, y, z, nullptr, nullptr) != HOPE_EINVAL) return 1;
    if (ga_host(x, x, x, nullptr, x, 1, 1, gamma, lam, 0, y, z, nullptr, nullptr) != HOPE_EINVAL) return 1;
    if (ga_host(x, x, x, x, x, 1, 1, gamma, lam, 0, nullptr, z, nullptr, nullptr) != HOPE_EINVAL) return 1;
    if (ga_host(x, x, x, x, x, 0, 1, gamma, lam, 0, y, z, nullptr, nullptr) != HOPE_EINVAL) return 1;
    if (ga_host(x, x, x, x, x, 1, 0, gamma, lam, 0, y, z, nullptr, nullptr) != HOPE_EINVAL) return 1;
    if (ga_host(x, x, x, x, x, 1, 1, gamma, lam, 4, y, z, nullptr, nullptr) != HOPE_EINVAL) return 1;
    if (ga_host(x, x, x, x, x, 1, 1, NAN, lam, 0, y, z, nullptr, nullptr) != HOPE_EINVAL) return 1;
    if (ga_host(x, x, x, x, x, 1, 1, gamma, INFINITY, 0, y, z, nullptr, nullptr) != HOPE_EINVAL) return 1;
    if (ga_normalize_host(x, 1, nullptr, y, nullptr) != HOPE_EINVAL) return 1;
    if (ga_normalize_host(nullptr, 1, s, y, nullptr) != HOPE_EINVAL) return 1;
    if (ga_normalize_host(x, -1, s, y, nullptr) != HOPE_EINVAL) return 1;
    if (ga_normalize_host(nullptr, 0, s, nullptr, ms) != HOPE_OK || ms[0] != 0.f || ms[1] != 0.f) return 1;
    if (ga_host(x, x, x, x, x, 1, 1, gamma, lam, HOPE_GAE_NORMALIZE, y, z, s, nullptr) != HOPE_OK || y[0] != 0.f) return 1;
    printf("gae host twins: %lld calls, %lld elements, worst |adv - long double| %.3g, worst sum error %.3g of the scale, clean\n", calls, elems,
           worst_adv, worst_sum);
    return calls >= 300 && elems > 1000000 ? 0 : 1;
}
