// Stand-alone driver of the optimiser block's host twins for sanitizer runs on the CPU (no device, no Python):
//   c++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -Iinclude -Ihope_amd/csrc tests/optim_host_sanitize.cpp -o optim_host_sanitize && ./optim_host_sanitize
// It runs op_adam_host and op_polyak_host (hope_optim_core.h; hope_optim_adam_host / hope_optim_polyak_host forward to them) over heap
// buffers of EXACTLY an entry's size -- so a read or write past the last element is an error -- at bases 0, 4, 8 and 12 bytes past a
// 16-byte boundary, with float32 and float64 entries, two groups, more entries than one launch holds, the tensor sizes around a
// lane's four elements and a chunk of 1 024, and checks every output against a long-double recomputation.  Then the refusals.
// Exit code 0 = clean.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "hope_optim_core.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }
static double uni() { return (double)(rnd() >> 11) / 9007199254740992.0; }
static double gauss() { return sqrt(-2.0 * log(uni() + 1e-300)) * cos(6.283185307179586 * uni()); }

// an exact-size heap block of n elements of T whose first element sits `off` bytes past a 16-byte boundary: the block is malloc'ed
// with exactly off + n * sizeof(T) bytes behind an aligned start, so the sanitizer sees the first byte past the entry
template <class T>
struct Block {
    void* raw = nullptr;
    T* at = nullptr;
    size_t n = 0;
    Block(size_t n_, size_t off) : n(n_) {
        if (posix_memalign(&raw, 16, off + n * sizeof(T)) != 0) abort();
        at = (T*)((char*)raw + off);
    }
    Block(const Block&) = delete;
    Block(Block&& o) : raw(o.raw), at(o.at), n(o.n) { o.raw = nullptr; }
    ~Block() { free(raw); }
};

template <class T>
struct Tensor {
    Block<T> p, g, m, v;
    std::vector<T> p0, m0, v0;
    Tensor(size_t n, size_t off) : p(n, off), g(n, off), m(n, off), v(n, off), p0(n), m0(n), v0(n) {
        for (size_t i = 0; i < n; i++) {
            p.at[i] = p0[i] = (T)(gauss() * 0.1);
            g.at[i] = (T)(gauss() * pow(10.0, (double)((int)(rnd() % 10) - 8)));
            const bool first = n % 2 == 0;
            m.at[i] = m0[i] = first ? (T)0 : (T)(gauss() * pow(10.0, (double)((int)(rnd() % 10) - 8)));
            v.at[i] = v0[i] = first ? (T)0 : (T)(uni() * pow(10.0, (double)((int)(rnd() % 19) - 16)));
        }
    }
    hope_optim_entry_t entry(int group) const {
        hope_optim_entry_t e;
        e.p = p.at; e.g = g.at; e.m = m.at; e.v = v.at;
        e.numel = (int64_t)p.n; e.group = group; e.dtype = sizeof(T) == 8 ? HOPE_OPTIM_F64 : HOPE_OPTIM_F32;
        return e;
    }
};

static double worst = 0.0;

// |x - want| in units of the type's rounding step at `want` (half of one is the rule's own error; the long-double recomputation adds
// the double roundings of the intermediate steps: far below that for float32, and for float64 steps of the operands' size `scale`,
// which a cancelling sum leaves larger than the result's)
template <class T>
static bool near(T x, long double want, double ulps, long double scale = 0.0L) {
    if (want != want) return x != x;
    const double eps = sizeof(T) == 8 ? 2.220446049250313e-16 : 1.1920928955078125e-07;
    const double tiny = sizeof(T) == 8 ? 4.9e-324 : 1.4e-45;
    const double err = fabs((double)((long double)x - want)), unit = fmax(fmax(fabs((double)want), sizeof(T) == 8 ? fabs((double)scale) : 0.0) * eps, tiny);
    if (err / unit > worst) worst = err / unit;
    return err <= ulps * unit;
}

template <class T>
static bool check_adam(const Tensor<T>& t, const hope_optim_group_t& G) {
    for (size_t i = 0; i < t.p.n; i++) {
        const long double g = t.g.at[i];
        const long double m = (long double)t.m0[i] + (long double)G.c1 * (g - t.m0[i]);
        const long double v = (long double)G.b2 * t.v0[i] + (long double)G.c2 * g * g;
        if (!near(t.m.at[i], m, sizeof(T) == 8 ? 4.0 : 0.51, fabsl(g) + fabsl((long double)t.m0[i])) || !near(t.v.at[i], v, sizeof(T) == 8 ? 4.0 : 0.51)) { fprintf(stderr, "state of element %zu of %zu is off\n", i, t.p.n); return false; }
        // the step from the STORED m', v' (the rule reads them back)
        const long double den = sqrtl((long double)t.v.at[i]) / (long double)G.bc2s + (long double)G.eps;
        const long double p = (long double)t.p0[i] - (long double)G.step_size * ((long double)t.m.at[i] / den);
        if (!near(t.p.at[i], p, sizeof(T) == 8 ? 4.0 : 0.51, fabsl((long double)t.p0[i]) + fabsl(p))) { fprintf(stderr, "parameter %zu of %zu is off\n", i, t.p.n); return false; }
    }
    return true;
}

static hope_optim_group_t group_of(double lr, double b1, double b2, double eps, int t) {
    hope_optim_group_t G;
    G.c1 = 1.0 - b1; G.b2 = b2; G.c2 = 1.0 - b2; G.step_size = lr / (1.0 - pow(b1, t)); G.bc2s = sqrt(1.0 - pow(b2, t)); G.eps = eps;
    return G;
}

int main() {
    const size_t sizes[] = {1, 2, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 2049};
    const hope_optim_group_t groups[2] = {group_of(5e-6, 0.9, 0.999, 1e-8, 3), group_of(1e-3, 0.9, 0.999, 1e-5, 1000000)};
    long long calls = 0, elems = 0;
    OpBad bad;
    // every size at every base, float32 and float64, one entry per call
    for (size_t n : sizes)
        for (size_t off : {0, 4, 8, 12}) {
            Tensor<float> t(n, off);
            hope_optim_entry_t e = t.entry((int)(off / 4) % 2);
            if (op_adam_host(&e, 1, groups, 2, &bad) != HOPE_OK || !check_adam(t, groups[e.group])) return 1;
            Tensor<double> d(n, off & 8);
            hope_optim_entry_t e64 = d.entry(1);
            if (op_adam_host(&e64, 1, groups, 2, &bad) != HOPE_OK || !check_adam(d, groups[1])) return 1;
            calls += 2; elems += 2 * (long long)n;
        }
    // more entries than one launch holds, float32 and float64 and both groups mixed in one call
    for (int count : {HOPE_OPTIM_CAP, HOPE_OPTIM_CAP + 1, 2 * HOPE_OPTIM_CAP + 1}) {
        std::vector<Tensor<float>> f;
        std::vector<Tensor<double>> d;
        std::vector<hope_optim_entry_t> e;
        f.reserve(count); d.reserve(count);
        for (int i = 0; i < count; i++) {
            if (i % 5 == 4) { d.emplace_back(1 + i % 9, (size_t)(i % 2) * 8); e.push_back(d.back().entry(i % 2)); }
            else { f.emplace_back(1 + i % 9, (size_t)(i % 4) * 4); e.push_back(f.back().entry(i % 2)); }
        }
        if (op_adam_host(e.data(), count, groups, 2, &bad) != HOPE_OK) return 1;
        size_t fi = 0, di = 0;
        for (int i = 0; i < count; i++) {
            if (i % 5 == 4 ? !check_adam(d[di++], groups[i % 2]) : !check_adam(f[fi++], groups[i % 2])) return 1;
            elems += 1 + i % 9;
        }
        calls++;
    }
    // Polyak: every size at every base, tau at its ends and inside
    for (double tau : {0.0, 1.0, 0.005, 0.1})
        for (size_t n : sizes)
            for (size_t off : {0, 4, 8, 12}) {
                Tensor<float> t(n, off);
                Tensor<double> d(n, off & 8);
                hope_optim_entry_t e[2] = {t.entry(0), d.entry(0)};
                e[0].m = e[0].v = e[1].m = e[1].v = nullptr;                 // not looked at
                if (op_polyak_host(e, 2, tau, &bad) != HOPE_OK) return 1;
                for (size_t i = 0; i < n; i++) {
                    if (!near(t.p.at[i], (1.0L - tau) * t.p0[i] + (long double)tau * t.g.at[i], 0.51) ||
                        !near(d.p.at[i], (1.0L - tau) * d.p0[i] + (long double)tau * d.g.at[i], 4.0, fabsl((long double)d.p0[i]) + fabsl((long double)d.g.at[i]))) { fprintf(stderr, "polyak element %zu of %zu is off\n", i, n); return 1; }
                    if (tau == 0.0 && t.p.at[i] != t.p0[i]) return 1;
                    if (tau == 1.0 && t.p.at[i] != t.g.at[i]) return 1;
                }
                calls++; elems += 2 * (long long)n;
            }
    // misuse: refused with the entry named, nothing touched (the blocks are exact: a touch past them would be caught)
    Tensor<float> a(8, 0), b(8, 4);
    hope_optim_entry_t e[2] = {a.entry(0), b.entry(1)};
    auto refused = [&](int kind, long long index) { return bad.kind == kind && bad.index == index && bad.what; };
    if (op_adam_host(nullptr, 2, groups, 2, &bad) != HOPE_EINVAL || !refused(OP_BAD_CALL, 0)) return 1;
    if (op_adam_host(e, 0, groups, 2, &bad) != HOPE_EINVAL || op_adam_host(e, 2, nullptr, 2, &bad) != HOPE_EINVAL) return 1;
    if (op_adam_host(e, 2, groups, 0, &bad) != HOPE_EINVAL || op_adam_host(e, 2, groups, 5, &bad) != HOPE_EINVAL) return 1;
    if (op_adam_host(e, 2, groups, 1, &bad) != HOPE_EINVAL || !refused(OP_BAD_ENTRY, 1)) return 1;            // group 1 of 1
    hope_optim_entry_t x[2] = {e[0], e[1]};
    x[1].v = nullptr;
    if (op_adam_host(x, 2, groups, 2, &bad) != HOPE_EINVAL || !refused(OP_BAD_ENTRY, 1)) return 1;
    x[1] = e[1]; x[0].m = (char*)x[0].m + 2;
    if (op_adam_host(x, 2, groups, 2, &bad) != HOPE_EINVAL || !refused(OP_BAD_ENTRY, 0)) return 1;
    x[0] = e[0]; x[1].numel = 0;
    if (op_adam_host(x, 2, groups, 2, &bad) != HOPE_EINVAL || !refused(OP_BAD_ENTRY, 1)) return 1;
    x[1].numel = ((int64_t)1 << 31) - 7;                                                                       // 8 + 2^31 - 7 > 2^31
    if (op_adam_host(x, 2, groups, 2, &bad) != HOPE_EINVAL || !refused(OP_BAD_ENTRY, 1)) return 1;
    x[1] = e[1]; x[1].dtype = 2;
    if (op_adam_host(x, 2, groups, 2, &bad) != HOPE_EINVAL || !refused(OP_BAD_ENTRY, 1)) return 1;
    hope_optim_group_t g2[2] = {groups[0], groups[1]};
    g2[1].eps = -1e-9;
    if (op_adam_host(e, 2, g2, 2, &bad) != HOPE_EINVAL || !refused(OP_BAD_GROUP, 1)) return 1;
    g2[1] = groups[1]; g2[0].bc2s = 0.0;
    if (op_adam_host(e, 2, g2, 2, &bad) != HOPE_EINVAL || !refused(OP_BAD_GROUP, 0)) return 1;
    g2[0] = groups[0]; g2[0].step_size = NAN;
    if (op_adam_host(e, 2, g2, 2, &bad) != HOPE_EINVAL || !refused(OP_BAD_GROUP, 0)) return 1;
    for (double tau : {-0.5, 1.5, (double)NAN, (double)INFINITY})
        if (op_polyak_host(e, 2, tau, &bad) != HOPE_EINVAL || !refused(OP_BAD_CALL, 0)) return 1;
    for (size_t i = 0; i < 8; i++)
        if (a.p.at[i] != a.p0[i] || a.m.at[i] != a.m0[i] || b.v.at[i] != b.v0[i] || b.p.at[i] != b.p0[i]) { fprintf(stderr, "a refused call wrote\n"); return 1; }
    printf("optim host twins: %lld calls, %lld elements, worst error %.3f rounding steps, clean\n", calls, elems, worst);
    return calls >= 250 && elems > 100000 ? 0 : 1;
}
