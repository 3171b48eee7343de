// Stand-alone driver of the evaluation tracker's host twins for sanitizer runs on the CPU (no device, no Python):
//   clang++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//           -Iinclude -Ihope_amd/csrc tests/evaltrack_host_sanitize.cpp -o evaltrack_host_sanitize && ./evaltrack_host_sanitize
// It runs et_begin_host / et_override_host / et_track_host (hope_evaltrack_core.h; the hope_eval_*_host entry points forward to
// them) over heap buffers of EXACTLY the call's size -- so a read or write past the last scene of a plane, a row or a word is an
// error -- with both observation types, both action types, supplied and counter-based draws, whole batches and batches split at a
// row (a sub-batch addresses the middle of the state block), NaN inputs, and checks the outputs against a plain scalar replay.
// Exit code 0 = clean.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "hope_evaltrack_core.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }
static double uni() { return (double)(rnd() >> 11) / 9007199254740992.0; }

struct Ref {                    // the reference's loop for one scene
    double lt[5], lx, ly, total = 0.0, path = 0.0;
    int steps = 0, status = 1;
    bool alive = true, stuck = true;
};

template <class T>
static int run(int n, int act_f64, bool supplied, int split) {
    const double box[4] = {-0.75, 0.75, -2.5, 2.5};
    std::vector<uint64_t> state((size_t)ET_WORDS * n);
    std::vector<T> target((size_t)n * 5), reward((size_t)n);
    std::vector<double> pose((size_t)n * 3), u((size_t)n * 2), a64((size_t)n * 2);
    std::vector<float> a32((size_t)n * 2);
    std::vector<int32_t> status((size_t)n);
    std::vector<uint8_t> done((size_t)n), done_out((size_t)n), active((size_t)n);
    std::vector<int8_t> word((size_t)n * 8), word_out((size_t)n * 8);
    std::vector<Ref> ref((size_t)n);
    const int obs_f64 = sizeof(T) == 8;
    for (size_t i = 0; i < target.size(); i++) target[i] = (T)(float)(uni() * 6.0 - 3.0);
    for (size_t i = 0; i < pose.size(); i++) pose[i] = uni() * 20.0 - 10.0;
    if (et_begin_host(n, n, state.data(), target.data(), obs_f64, pose.data()) != HOPE_OK) return 1;
    for (int i = 0; i < n; i++) {
        for (int k = 0; k < 5; k++) ref[i].lt[k] = (double)target[(size_t)i * 5 + k];
        ref[i].lx = pose[(size_t)i * 3]; ref[i].ly = pose[(size_t)i * 3 + 1];
    }
    for (int t = 0; t < 12; t++) {
        // override: the whole batch, or two parts split at row `split` that address the same block
        for (size_t i = 0; i < u.size(); i++) { u[i] = uni(); a64[i] = uni() * 2.0 - 1.0; a32[i] = (float)a64[i]; }
        const std::vector<double> before64 = a64;
        const std::vector<float> before32 = a32;
        void* act = act_f64 ? (void*)a64.data() : (void*)a32.data();
        const size_t row = act_f64 ? 16 : 8;
        int rc;
        if (split > 0 && split < n) {
            rc = et_override_host(split, n, state.data(), box, act, act_f64, supplied ? u.data() : nullptr, 7, (uint64_t)t, 0, active.data());
            if (rc == HOPE_OK)
                rc = et_override_host(n - split, n, state.data() + split, box, (char*)act + row * split, act_f64, supplied ? u.data() + 2 * (size_t)split : nullptr, 7,
                                      (uint64_t)t, (uint64_t)split, active.data() + split);
        } else {
            rc = et_override_host(n, n, state.data(), box, act, act_f64, supplied ? u.data() : nullptr, 7, (uint64_t)t, 0, active.data());
        }
        if (rc != HOPE_OK) { fprintf(stderr, "et_override_host returned %d\n", rc); return 1; }
        const uint64_t key = et_key(7, (uint64_t)t);
        for (int i = 0; i < n; i++) {
            if (active[i] != (ref[i].alive ? 1 : 0)) { fprintf(stderr, "step %d scene %d: active\n", t, i); return 1; }
            for (int d = 0; d < 2; d++) {
                const double uu = supplied ? u[(size_t)i * 2 + d] : et_uniform(key, (uint64_t)i, d);
                double want = box[2 * d] + (box[2 * d + 1] - box[2 * d]) * uu;
                want = want < -1.0 ? -1.0 : (want > 1.0 ? 1.0 : want);
                const size_t j = (size_t)i * 2 + d;
                const bool ok = act_f64 ? a64[j] == (ref[i].stuck ? want : before64[j]) : a32[j] == (ref[i].stuck ? (float)want : before32[j]);
                if (!ok || !(uu >= 0.0 && uu < 1.0)) { fprintf(stderr, "step %d scene %d: action row\n", t, i); return 1; }
            }
        }
        // the env step's outputs; a few NaNs
        for (int i = 0; i < n; i++) {
            const bool same = uni() < 0.4;
            for (int k = 0; k < 5; k++) if (!same) target[(size_t)i * 5 + k] = (T)(float)(uni() * 6.0 - 3.0);
            if (i % 17 == 3 && t == 4) target[(size_t)i * 5 + 1] = (T)NAN;
            pose[(size_t)i * 3] += uni() - 0.5; pose[(size_t)i * 3 + 1] += uni() - 0.5;
            reward[i] = (T)(float)(uni() - 0.5);
            if (i % 19 == 5 && t == 3) reward[i] = (T)NAN;
            done[i] = uni() < 0.12;
            status[i] = done[i] ? 2 + (int)(rnd() % 4) : 1;
            for (int k = 0; k < 8; k++) word[(size_t)i * 8 + k] = (int8_t)(rnd() % 4) - 1;
            word[(size_t)i * 8 + 6] = (int8_t)(rnd() % 2);
        }
        if (split > 0 && split < n) {
            rc = et_track_host(split, n, state.data(), target.data(), obs_f64, pose.data(), reward.data(), status.data(), done.data(), word.data(), word_out.data(),
                               done_out.data());
            if (rc == HOPE_OK)
                rc = et_track_host(n - split, n, state.data() + split, target.data() + 5 * (size_t)split, obs_f64, pose.data() + 3 * (size_t)split,
                                   reward.data() + split, status.data() + split, done.data() + split, word.data() + 8 * (size_t)split,
                                   word_out.data() + 8 * (size_t)split, done_out.data() + split);
        } else {
            rc = et_track_host(n, n, state.data(), target.data(), obs_f64, pose.data(), reward.data(), status.data(), done.data(), word.data(), word_out.data(),
                               done_out.data());
        }
        if (rc != HOPE_OK) { fprintf(stderr, "et_track_host returned %d\n", rc); return 1; }
        for (int i = 0; i < n; i++) {
            Ref& r = ref[i];
            const double x = pose[(size_t)i * 3], y = pose[(size_t)i * 3 + 1];
            if (r.alive) {
                r.steps++;
                r.total += (double)reward[i];
                const double dx = x - r.lx, dy = y - r.ly;
                r.path += sqrt(dx * dx + dy * dy);
            }
            r.lx = x; r.ly = y;
            const bool fin = r.alive && done[i];
            if (fin) r.status = status[i];
            bool stuck = true;
            for (int k = 0; k < 5; k++) { const double v = (double)target[(size_t)i * 5 + k]; stuck = stuck && v == r.lt[k]; r.lt[k] = v; }
            r.stuck = stuck;
            r.alive = r.alive && !fin;
            const uint64_t w = state[(size_t)9 * n + i];
            const double total = et_bits_to_double(state[(size_t)7 * n + i]), path = et_bits_to_double(state[(size_t)8 * n + i]);
            const bool sums_ok = (total == r.total || (total != total && r.total != r.total && state[(size_t)7 * n + i] == ET_QNAN)) && path == r.path;
            if ((uint32_t)w != (uint32_t)r.steps || (int)((w >> 32) & 0xFF) != r.status || ((w & ET_ALIVE) != 0) != r.alive || ((w & ET_STUCK) != 0) != r.stuck ||
                !sums_ok || done_out[i] != (fin ? 1 : 0)) {
                fprintf(stderr, "step %d scene %d: state differs from the scalar replay\n", t, i); return 1;
            }
            for (int k = 0; k < 8; k++) {
                const int8_t want = (k == 6 && !r.alive) ? 0 : word[(size_t)i * 8 + k];
                if (word_out[(size_t)i * 8 + k] != want) { fprintf(stderr, "step %d scene %d: word byte %d\n", t, i, k); return 1; }
            }
            for (int j = 0; j < 9; j++) {
                const uint64_t b = state[(size_t)j * n + i];
                const double v = et_bits_to_double(b);
                if (v != v && b != ET_QNAN) { fprintf(stderr, "step %d scene %d: a NaN with a payload in plane %d\n", t, i, j); return 1; }
            }
        }
    }
    return 0;
}

int main() {
    long long runs = 0, scenes = 0;
    for (int n : {1, 2, 63, 64, 65, 130, 1000})
        for (int act_f64 = 0; act_f64 < 2; act_f64++)
            for (int supplied = 0; supplied < 2; supplied++)
                for (int split : {0, 1, n / 2, n - 1}) {
                    if (run<float>(n, act_f64, supplied != 0, split) || run<double>(n, act_f64, supplied != 0, split)) {
                        fprintf(stderr, "n %d act_f64 %d supplied %d split %d\n", n, act_f64, supplied, split);
                        return 1;
                    }
                    runs += 2; scenes += 2 * n;
                }
    // misuse: nothing is touched
    uint64_t st[ET_WORDS] = {0};
    float t[5] = {0}, r[1] = {0}, a[2] = {0};
    double p[3] = {0};
    int32_t s[1] = {1};
    uint8_t d[1] = {0}, dout[1], act[1];
    int8_t w[8] = {0}, wo[8];
    const double box[4] = {-1, 1, -1, 1}, bad[4] = {-1, INFINITY, -1, 1};
    if (et_begin_host(0, 1, st, t, 0, p) != HOPE_EINVAL || et_begin_host(2, 1, st, t, 0, p) != HOPE_EINVAL || et_begin_host(1, 1, nullptr, t, 0, p) != HOPE_EINVAL ||
        et_begin_host(1, 1, st, nullptr, 0, p) != HOPE_EINVAL || et_begin_host(1, 1, st, t, 0, nullptr) != HOPE_EINVAL) return 1;
    if (et_override_host(1, 1, st, nullptr, a, 0, nullptr, 0, 0, 0, act) != HOPE_EINVAL || et_override_host(1, 1, st, bad, a, 0, nullptr, 0, 0, 0, act) != HOPE_EINVAL ||
        et_override_host(1, 1, st, box, nullptr, 0, nullptr, 0, 0, 0, act) != HOPE_EINVAL || et_override_host(1, 1, st, box, a, 0, nullptr, 0, 0, 0, nullptr) != HOPE_EINVAL ||
        et_override_host(1, 1, nullptr, box, a, 0, nullptr, 0, 0, 0, act) != HOPE_EINVAL) return 1;
    if (et_track_host(1, 1, st, t, 0, p, r, s, d, w, wo, nullptr) != HOPE_EINVAL || et_track_host(1, 1, st, t, 0, p, r, s, d, nullptr, wo, dout) != HOPE_EINVAL ||
        et_track_host(1, 1, st, t, 0, p, nullptr, s, d, w, wo, dout) != HOPE_EINVAL || et_track_host(1, 0, st, t, 0, p, r, s, d, w, wo, dout) != HOPE_EINVAL) return 1;
    for (uint64_t v : st) if (v) return 1;
    if (et_begin_host(1, 1, st, t, 0, p) != HOPE_OK || et_override_host(1, 1, st, box, a, 0, nullptr, 0, 0, 0, act) != HOPE_OK ||
        et_track_host(1, 1, st, t, 0, p, r, s, d, w, wo, dout) != HOPE_OK || (uint32_t)st[9] != 1) return 1;
    printf("evaltrack host twins: %lld runs of 12 steps, %lld scenes, clean\n", runs, scenes);
    return runs >= 200 ? 0 : 1;
}
