// Stand-alone driver of the action chooser's host twin for sanitizer runs on the CPU (no device, no Python):
//   clang++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//           -Iinclude -Ihope_amd/csrc tests/chooser_host_sanitize.cpp -o chooser_host_sanitize && ./chooser_host_sanitize
// It runs ch_host (hope_chooser_core.h; hope_chooser_host forwards to it) over buffers of EXACTLY the batch's size -- so a read or
// write past a partly filled last block of 64 is an error -- with random rows and the edges of the rule: single-entry and all-zero
// masks, NaN / infinite / huge means, log_std, masks and u, executing rows with extreme planned values, every combination of input,
// mask and action type, broadcast log_std, NULL optional outputs, the counter-based draw -- and checks the invariants of the
// outputs.  Exit code 0 = clean.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "hope_chooser_core.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }
static double uni() { return (double)(rnd() >> 11) / 9007199254740992.0; }

int main() {
    double A[CH_NA * 2];
    for (int k = 0; k < CH_NA; k++) { A[2 * k] = 1.0 - 0.1 * (k % CH_NS); A[2 * k + 1] = k < CH_NS ? 1.0 : -1.0; }
    if (!ch_table_ok(A)) return 1;
    static const double edge[] = {0.0, -0.0, 1.0, -1.0, 0.05, NAN, INFINITY, -INFINITY, 1e300, -1e300, 5e-324, 700.0, -700.0, 701.0, -746.0, -5.0, -12.0, 2.0, 3e38, -3e38};
    const int n_edge = (int)(sizeof(edge) / sizeof(edge[0]));
    long long rows = 0, flagged = 0, fixed = 0;
    for (int n : {1, 63, 64, 65, 193}) {
        for (int t = 0; t < 96; t++) {
            const int in_f64 = t & 1, mask_f64 = (t >> 1) & 1, act_f64 = (t >> 2) & 1, bcast = (t >> 3) & 1, bare = t % 5 == 4, own_u = t % 3 != 0, plan = t % 4 != 3;
            // exact-size buffers: the sanitizer sees the first byte past the batch
            std::vector<double> m64((size_t)n * 2), ls64(bcast ? 2 : (size_t)n * 2), k64((size_t)n * CH_NA), planned((size_t)n * 2), u(n), a64((size_t)n * 2),
                probs((size_t)n * CH_NA);
            std::vector<float> m32((size_t)n * 2), ls32(bcast ? 2 : (size_t)n * 2), k32((size_t)n * CH_NA), a32((size_t)n * 2), af((size_t)n * 2), lp((size_t)n * 2);
            std::vector<uint8_t> ex(n);
            std::vector<int32_t> idx(n);
            for (size_t i = 0; i < m64.size(); i++) { const double v = rnd() % 6 == 0 ? edge[rnd() % n_edge] : uni() * 2.0 - 1.0; m64[i] = v; m32[i] = (float)v; }
            for (size_t i = 0; i < ls64.size(); i++) { const double v = rnd() % 6 == 0 ? edge[rnd() % n_edge] : uni() * 3.5 - 3.0; ls64[i] = v; ls32[i] = (float)v; }
            for (int s = 0; s < n; s++) {
                const int kind = (int)(rnd() % 8);                  // 0: all zero, 1: one entry, 2: with edge values, else multiples of 0.1
                const int one = (int)(rnd() % CH_NA);
                for (int k = 0; k < CH_NA; k++) {
                    double v = rnd() % 10 < 3 ? 0.0 : (double)(1 + rnd() % 10) / 10.0;
                    if (kind == 0) v = 0.0;
                    if (kind == 1) v = k == one ? 0.3 : 0.0;
                    if (kind == 2 && rnd() % 4 == 0) v = edge[rnd() % n_edge];
                    k64[(size_t)s * CH_NA + k] = v; k32[(size_t)s * CH_NA + k] = (float)v;
                }
                u[s] = rnd() % 5 == 0 ? edge[rnd() % n_edge] : uni();
                ex[s] = rnd() % 4 == 0;
                planned[(size_t)s * 2] = rnd() % 5 == 0 ? edge[rnd() % n_edge] : (double)((int)(rnd() % 3) - 1);
                planned[(size_t)s * 2 + 1] = uni() * 2.0 - 1.0;
                idx[s] = -1;
            }
            void* action = act_f64 ? (void*)a64.data() : (void*)a32.data();
            const int rc = ch_host(n, A, in_f64 ? (const void*)m64.data() : (const void*)m32.data(), in_f64 ? (const void*)ls64.data() : (const void*)ls32.data(),
                                   bcast ? 0 : 2, in_f64, mask_f64 ? (const void*)k64.data() : (const void*)k32.data(), mask_f64, plan ? planned.data() : nullptr,
                                   plan ? ex.data() : nullptr, own_u ? u.data() : nullptr, 0x1234 + t, (uint64_t)t << 40, (uint64_t)n * t, action, act_f64,
                                   bare ? nullptr : af.data(), bare ? nullptr : idx.data(), bare ? nullptr : lp.data(), bare ? nullptr : probs.data());
            if (rc != HOPE_OK) { fprintf(stderr, "ch_host returned %d\n", rc); return 1; }
            if (bare) continue;
            for (int s = 0; s < n; s++) {
                const int k = idx[s] & 63, fl = idx[s] & ~63;
                if (k >= CH_NA || (fl & ~(HOPE_CHOOSE_NOMASK | HOPE_CHOOSE_FIXED)) || ((fl & HOPE_CHOOSE_FIXED) && (!(fl & HOPE_CHOOSE_NOMASK) || k != CH_FALLBACK))) {
                    fprintf(stderr, "bad index %d of scene %d in pass %d\n", idx[s], s, t); return 1;
                }
                const bool replay = plan && ex[s];
                const double got0 = act_f64 ? a64[(size_t)s * 2] : (double)a32[(size_t)s * 2];
                if (got0 != (double)af[(size_t)s * 2] && !(got0 != got0)) { fprintf(stderr, "action and action_f32 differ\n"); return 1; }
                if (!replay && (af[(size_t)s * 2] != (float)A[2 * k] || af[(size_t)s * 2 + 1] != (float)A[2 * k + 1])) { fprintf(stderr, "action is not row k of the table\n"); return 1; }
                if (!fl) {                                          // an unflagged row takes an action that carries weight
                    const double w = mask_f64 ? k64[(size_t)s * CH_NA + k] : (double)k32[(size_t)s * CH_NA + k];
                    if (!(w > 0.0)) { fprintf(stderr, "scene %d took a masked-out action\n", s); return 1; }
                }
                double sum = 0.0;
                for (int j = 0; j < CH_NA; j++) sum += probs[(size_t)s * CH_NA + j];
                const double* pr = &probs[(size_t)s * CH_NA];
                if (!(fabs(sum - 1.0) < 1e-9) && !(sum != sum && !fl)) {           // (a NaN among positive mask entries leaves NaN in probs)
                    bool neg = false;                                              // negative mask entries: weights that do not sum to 1 in absolute value
                    for (int j = 0; j < CH_NA; j++) neg = neg || pr[j] < 0.0;
                    if (!neg) { fprintf(stderr, "probs of scene %d sum to %g\n", s, sum); return 1; }
                }
                rows++; flagged += fl != 0; fixed += (fl & HOPE_CHOOSE_FIXED) != 0;
            }
        }
    }
    // misuse
    float a2[2]; double m2[2] = {0, 0}, k42[CH_NA] = {0}; uint8_t e1 = 0;
    if (ch_host(0, A, m2, m2, 2, 1, k42, 1, nullptr, nullptr, nullptr, 0, 0, 0, a2, 0, nullptr, nullptr, nullptr, nullptr) != HOPE_EINVAL) return 1;
    if (ch_host(1, A, m2, m2, 2, 1, nullptr, 1, nullptr, nullptr, nullptr, 0, 0, 0, a2, 0, nullptr, nullptr, nullptr, nullptr) != HOPE_EINVAL) return 1;
    if (ch_host(1, A, m2, m2, 2, 1, k42, 1, nullptr, &e1, nullptr, 0, 0, 0, a2, 0, nullptr, nullptr, nullptr, nullptr) != HOPE_EINVAL) return 1;
    if (ch_host(1, A, m2, m2, 3, 1, k42, 1, nullptr, nullptr, nullptr, 0, 0, 0, a2, 0, nullptr, nullptr, nullptr, nullptr) != HOPE_EINVAL) return 1;
    A[7] = 0.5;
    if (ch_host(1, A, m2, m2, 2, 1, k42, 1, nullptr, nullptr, nullptr, 0, 0, 0, a2, 0, nullptr, nullptr, nullptr, nullptr) != HOPE_EINVAL) return 1;
    printf("chooser host twin: %lld rows checked, %lld flagged (%lld at the fixed index), clean\n", rows, flagged, fixed);
    return rows > 10000 && flagged > 1000 && fixed > 100 ? 0 : 1;
}
