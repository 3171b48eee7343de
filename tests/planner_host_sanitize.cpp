// Stand-alone driver of the planner's host twin for sanitizer runs on the CPU (no device, no Python):
//   clang++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//           -Iinclude -Ihope_amd/csrc tests/planner_host_sanitize.cpp -o planner_host_sanitize && ./planner_host_sanitize
// It steps pl_step_host (hope_planner_core.h; hope_planner_step_host forwards to it) over fixture-like inputs -- found words of one
// to five segments with lengths on the edges of the rule, non-finite and huge lengths, episode ends, forced adoption, both length
// and action types, odd scene counts, NULL optional outputs -- and checks the invariants of the state.  Exit code 0 = clean.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "hope_planner_core.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }
static double uni() { return (double)(rnd() >> 11) / 9007199254740992.0; }

int main() {
    static const double edge[] = {1.25, -1.25, 2.5, -3.75, 1.25 * (1 + 0x1p-52), 1.25 * (1 - 0x1p-52), 1.25e-3, -1.25e-3, 1.25 * (1 + 1e-3), 0.0, -0.0,
                                  INFINITY, -INFINITY, NAN, 1e300, -1e300, 5e-324, 4e9, -2.7e9};
    const int n_edge = (int)(sizeof(edge) / sizeof(edge[0]));
    long long popped = 0, checks = 0;
    for (int n : {1, 63, 193}) {
        for (int f64 = 0; f64 < 2; f64++) {
            std::vector<uint64_t> state((size_t)PL_WORDS * n, 0);
            std::vector<int8_t> word((size_t)n * 8);
            std::vector<double> l64((size_t)n * 5), planned((size_t)n * 2), a64((size_t)n * 2);
            std::vector<float> l32((size_t)n * 5), a32((size_t)n * 2);
            std::vector<uint8_t> done(n), ex(n);
            for (int t = 0; t < 400; t++) {
                for (int s = 0; s < n; s++) {
                    const int nseg = (int)(rnd() % 7) - 1;                 // -1 .. 5: out-of-range counts too
                    for (int i = 0; i < 5; i++) {
                        word[(size_t)s * 8 + i] = (int8_t)((int)(rnd() % 5) - 1);   // -1 .. 3
                        const double v = rnd() % 3 == 0 ? edge[rnd() % n_edge] : (uni() * 12.0 - 6.0);
                        l64[(size_t)s * 5 + i] = v; l32[(size_t)s * 5 + i] = (float)v;
                    }
                    word[(size_t)s * 8 + 5] = (int8_t)nseg;
                    word[(size_t)s * 8 + 6] = (int8_t)(rnd() % 4 == 0);
                    word[(size_t)s * 8 + 7] = 0;
                    done[s] = rnd() % 25 == 0;
                    a64[(size_t)s * 2] = a64[(size_t)s * 2 + 1] = 7.0; a32[(size_t)s * 2] = a32[(size_t)s * 2 + 1] = 7.0f;
                }
                const int flags = (t % 7 == 6 ? HOPE_PLAN_FORCED : 0) | (t % 11 == 10 ? HOPE_PLAN_NO_POP : 0);
                const bool a_is64 = t & 1;
                const bool bare = t % 13 == 12;                          // every optional pointer NULL
                const int rc = pl_step_host(n, 1.25, state.data(), word.data(), f64 ? (const void*)l64.data() : (const void*)l32.data(), f64,
                                            bare ? nullptr : done.data(), flags, bare ? nullptr : planned.data(), bare ? nullptr : ex.data(),
                                            bare ? nullptr : (a_is64 ? (void*)a64.data() : (void*)a32.data()), a_is64);
                if (rc != HOPE_OK) { fprintf(stderr, "pl_step_host returned %d\n", rc); return 1; }
                for (int s = 0; s < n; s++) {
                    const uint64_t w = state[(size_t)5 * n + s];
                    const bool busy = w & PL_BUSY;
                    bool zero = true;
                    for (int j = 0; j < PL_WORDS; j++) zero = zero && state[(size_t)j * n + s] == 0;
                    if (busy == zero || (!busy && w != 0) || ((w >> 10) & 7) > 4) { fprintf(stderr, "bad state of scene %d at step %d\n", s, t); return 1; }
                    checks++;
                    if (bare || (flags & HOPE_PLAN_NO_POP)) continue;
                    const double p0 = planned[(size_t)s * 2], p1 = planned[(size_t)s * 2 + 1];
                    if (ex[s] > 1 || !(p0 == 0.0 || p0 == 1.0 || p0 == -1.0) || !(fabs(p1) <= 1.0)) { fprintf(stderr, "bad action of scene %d at step %d\n", s, t); return 1; }
                    if (!ex[s] && (p0 != 0.0 || p1 != 0.0)) { fprintf(stderr, "idle row not zero\n"); return 1; }
                    const double got0 = a_is64 ? a64[(size_t)s * 2] : (double)a32[(size_t)s * 2];
                    if (ex[s] ? got0 != p0 : got0 != 7.0) { fprintf(stderr, "override wrong\n"); return 1; }
                    popped += ex[s];
                }
            }
        }
    }
    if (pl_step_host(0, 1.25, &rng_state, (const int8_t*)&rng_state, &rng_state, 1, nullptr, 0, nullptr, nullptr, nullptr, 0) != HOPE_EINVAL) return 1;
    printf("planner host twin: %lld state checks, %lld actions popped, clean\n", checks, popped);
    return popped > 1000 ? 0 : 1;
}
