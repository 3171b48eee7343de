// Stand-alone driver of the observation normalisation's host twin for sanitizer runs on the CPU (no device, no Python):
//   clang++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//           -Iinclude -Ihope_amd/csrc tests/obsnorm_host_sanitize.cpp -o obsnorm_host_sanitize && ./obsnorm_host_sanitize
// It runs on_host (hope_obsnorm_core.h; hope_obsnorm_host forwards to it) over buffers of EXACTLY the call's size -- so a read or
// write past a short last chunk of 64 rows is an error -- with both input types, every flag combination, the first sample alone and
// inside a longer call, row counts around the chunk boundary and around the tree's pass-through nodes, and checks the invariants of
// the outputs against a plain long-double recomputation.  Exit code 0 = clean.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "hope_obsnorm_core.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }
static double uni() { return (double)(rnd() >> 11) / 9007199254740992.0; }

int main() {
    long long calls = 0, rows_total = 0;
    double worst_mean = 0.0, worst_std = 0.0;
    for (int in_f64 = 0; in_f64 < 2; in_f64++) {
        for (int first_rows : {1, 2, 70}) {
            hope_obsnorm_state st;
            memset(&st, 0, sizeof(st));
            std::vector<long double> sx(ON_NC, 0.0L), sxx(ON_NC, 0.0L);
            long long n = 0;
            int pass = 0;
            for (int rows : {first_rows, 1, 2, 63, 64, 65, 127, 128, 129, 193, 321, 385, 4160, 1}) {
                // exact-size buffers: the sanitizer sees the first byte past the call
                std::vector<float> l32((size_t)rows * ON_NL), t32((size_t)rows * ON_NT), ol((size_t)rows * ON_NL), ot((size_t)rows * ON_NT);
                std::vector<double> l64((size_t)rows * ON_NL), t64((size_t)rows * ON_NT);
                for (size_t i = 0; i < l32.size(); i++) { l32[i] = (float)(uni() * 10.0); l64[i] = (double)l32[i]; }
                for (size_t i = 0; i < t32.size(); i++) { t32[i] = (float)((uni() - 0.5) * (i % ON_NT == 0 ? 60.0 : 6.0)); t64[i] = (double)t32[i]; }
                const void* lp = in_f64 ? (const void*)l64.data() : (const void*)l32.data();
                const void* tp = in_f64 ? (const void*)t64.data() : (const void*)t32.data();
                const uint32_t flags = pass % 3 == 0 ? HOPE_OBSNORM_UPDATE : (uint32_t)(HOPE_OBSNORM_UPDATE | HOPE_OBSNORM_NORMALIZE);
                const bool norm = flags & HOPE_OBSNORM_NORMALIZE;
                int rc = on_host(&st, lp, tp, rows, in_f64, flags, norm ? ol.data() : nullptr, norm ? ot.data() : nullptr);
                if (rc != HOPE_OK) { fprintf(stderr, "on_host returned %d\n", rc); return 1; }
                if (pass % 4 == 1) {                                // normalise alone: the statistics must not move
                    const hope_obsnorm_state keep = st;
                    rc = on_host(&st, lp, tp, rows, in_f64, HOPE_OBSNORM_NORMALIZE, ol.data(), ot.data());
                    if (rc != HOPE_OK || memcmp(&keep, &st, sizeof(st)) != 0) { fprintf(stderr, "normalize moved the statistics\n"); return 1; }
                }
                for (int r = 0; r < rows; r++)
                    for (int c = 0; c < ON_NC; c++) {
                        const long double x = c < ON_NL ? l64[(size_t)r * ON_NL + c] : t64[(size_t)r * ON_NT + c - ON_NL];
                        sx[c] += x; sxx[c] += x * x;
                    }
                n += rows;
                if (st.n_state != n) { fprintf(stderr, "n_state %lld, expected %lld\n", (long long)st.n_state, n); return 1; }
                if (n > 1) {
                    for (int c = 0; c < ON_NC; c++) {
                        const long double mean = sx[c] / n, var = sxx[c] / n - mean * mean;
                        const double em = fabs((double)(st.mean[c] - mean)), es = fabs((double)(st.std[c] - sqrtl(var > 0 ? var : 0)));
                        if (em > worst_mean) worst_mean = em;
                        if (es > worst_std) worst_std = es;
                        if (!(em < 1e-9) || !(es < 1e-6) || !(st.S[c] >= 0.0)) {   // (the long-double check itself is this coarse)
                            fprintf(stderr, "column %d after %lld rows: mean off by %g, std off by %g, S %g\n", c, n, em, es, st.S[c]); return 1;
                        }
                    }
                }
                if (norm)
                    for (size_t i = 0; i < ol.size(); i++) {
                        const int c = (int)(i % ON_NL);
                        if (ol[i] != on_apply(l64[i], st.mean[c], st.std[c])) { fprintf(stderr, "out_lidar[%zu] is not the rule's value\n", i); return 1; }
                    }
                calls++; rows_total += rows; pass++;
            }
        }
    }
    // misuse
    hope_obsnorm_state st;
    memset(&st, 0, sizeof(st));
    float l[ON_NL] = {0}, t[ON_NT] = {0}, ol[ON_NL], ot[ON_NT];
    if (on_host(nullptr, l, t, 1, 0, HOPE_OBSNORM_UPDATE, nullptr, nullptr) != HOPE_EINVAL) return 1;
    if (on_host(&st, nullptr, t, 1, 0, HOPE_OBSNORM_UPDATE, nullptr, nullptr) != HOPE_EINVAL) return 1;
    if (on_host(&st, l, nullptr, 1, 0, HOPE_OBSNORM_UPDATE, nullptr, nullptr) != HOPE_EINVAL) return 1;
    if (on_host(&st, l, t, 0, 0, HOPE_OBSNORM_UPDATE, nullptr, nullptr) != HOPE_EINVAL) return 1;
    if (on_host(&st, l, t, 1, 0, 0, ol, ot) != HOPE_EINVAL) return 1;
    if (on_host(&st, l, t, 1, 0, 8, ol, ot) != HOPE_EINVAL) return 1;
    if (on_host(&st, l, t, 1, 0, HOPE_OBSNORM_NORMALIZE, ol, nullptr) != HOPE_EINVAL) return 1;
    if (on_host(&st, l, t, 1, 0, HOPE_OBSNORM_NORMALIZE, nullptr, ot) != HOPE_EINVAL) return 1;
    if (st.n_state != 0) return 1;
    if (on_host(&st, l, t, 1, 0, HOPE_OBSNORM_UPDATE | HOPE_OBSNORM_NORMALIZE, ol, ot) != HOPE_OK || st.n_state != 1) return 1;
    printf("obsnorm host twin: %lld calls, %lld rows, worst |mean - long double| %.3g, |std - long double| %.3g, clean\n", calls, rows_total, worst_mean,
           worst_std);
    return calls >= 80 && rows_total > 30000 ? 0 : 1;
}
