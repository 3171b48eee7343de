// Stand-alone driver of the host twin of the fused image encoder for sanitizer runs on the CPU (no device, no Python):
//   c++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -Iinclude -Ihope_amd/csrc tests/img_encoder_host_sanitize.cpp -o img_encoder_host_sanitize && ./img_encoder_host_sanitize
// It runs ie_forward_host (hope_imgenc_core.h; hope_imgenc_forward_host forwards to it) over heap buffers of EXACTLY each tensor's
// size -- the 14 parameters, the images, the token and the features, so a read or write one element past any of them is an error --
// at B = 1 and 33 with both activations, with and without the feature output, and checks that an image's words do not depend on the
// batch it is in, that the outputs are finite, and that the refused calls are refused and write nothing.  Exit code 0 = clean.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "hope_imgenc_core.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }
static double uni() { return (double)(rnd() >> 11) / 9007199254740992.0; }

// a heap buffer of exactly `count` elements
template <typename T>
struct Buf {
    T* p;
    size_t n;
    explicit Buf(size_t count) : p(new T[count]), n(count) {}
    ~Buf() { delete[] p; }
    Buf(const Buf&) = delete;
    Buf& operator=(const Buf&) = delete;
};

#define FAIL(...) do { fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); return 1; } while (0)

int main() {
    const size_t count[IE_NPARAM] = {4 * 3 * 9, 4, 4 * 3, 4, 8 * 4 * 9, 8, 8 * 4, 8, (size_t)IE_HID * IE_FEAT, IE_HID, (size_t)IE_E * IE_HID, IE_E, (size_t)IE_E * IE_E, IE_E};
    const int fan[IE_NPARAM] = {27, 0, 3, 0, 36, 0, 4, 0, IE_FEAT, 0, IE_HID, 0, IE_E, 0};
    std::vector<Buf<float>*> w;
    const float* ptr[IE_NPARAM];
    for (int i = 0; i < IE_NPARAM; ++i) {
        w.push_back(new Buf<float>(count[i]));
        const double s = fan[i] ? 1.2 / sqrt((double)fan[i]) : 0.05;
        for (size_t k = 0; k < count[i]; ++k) w[i]->p[k] = (float)((2.0 * uni() - 1.0) * s);
        ptr[i] = w[i]->p;
    }
    hope_imgenc_params_t P;
    static_assert(sizeof P == sizeof ptr, "hope_imgenc_params_t is IE_NPARAM pointers");
    memcpy(&P, ptr, sizeof P);
    long long calls = 0;
    for (int act : {0, 1}) {
        std::vector<float> tok0(IE_E), feat0(IE_FEAT);
        for (int64_t b : {(int64_t)33, (int64_t)1}) {
            const size_t n = (size_t)b;
            Buf<uint8_t> img(n * IE_IMG);
            Buf<float> token(n * IE_E), feat(n * IE_FEAT), token2(n * IE_E);
            rng_state = 0xABCDEFull;                               // image 0 is the same for every batch size
            for (size_t i = 0; i < img.n; ++i) img.p[i] = (uint8_t)(rnd() >> 56);
            if (n > 2) { memset(img.p + IE_IMG, 0, IE_IMG); memset(img.p + 2 * IE_IMG, 255, IE_IMG); }
            for (size_t i = 0; i < token.n; ++i) token.p[i] = token2.p[i] = 7.0f;
            for (size_t i = 0; i < feat.n; ++i) feat.p[i] = 7.0f;
            if (ie_forward_host(&P, act, img.p, b, token.p, feat.p) != HOPE_OK || ie_forward_host(&P, act, img.p, b, token2.p, nullptr) != HOPE_OK)
                FAIL("ie_forward_host refused act %d b %lld", act, (long long)b);
            calls += 2;
            if (memcmp(token.p, token2.p, token.n * sizeof(float)) != 0) FAIL("the token depends on the feature output (act %d, b %lld)", act, (long long)b);
            for (size_t i = 0; i < token.n; ++i)
                if (!isfinite(token.p[i])) FAIL("token %zu = %g (act %d, b %lld)", i, token.p[i], act, (long long)b);
            for (size_t i = 0; i < feat.n; ++i)
                if (!isfinite(feat.p[i]) || feat.p[i] == 7.0f) FAIL("feature %zu = %g (act %d, b %lld)", i, feat.p[i], act, (long long)b);
            if (b == 33) {
                memcpy(tok0.data(), token.p, sizeof(float) * IE_E);
                memcpy(feat0.data(), feat.p, sizeof(float) * IE_FEAT);
            } else if (memcmp(tok0.data(), token.p, sizeof(float) * IE_E) != 0 || memcmp(feat0.data(), feat.p, sizeof(float) * IE_FEAT) != 0)
                FAIL("image 0 depends on the batch size (act %d)", act);
        }
    }
    // refused: an act that is not compiled in, a null tensor, struct, image or token, an empty batch, an image off by one byte
    {
        Buf<uint8_t> img(IE_IMG + 4);
        Buf<float> token(IE_E), feat(IE_FEAT);
        memset(img.p, 9, img.n);
        for (size_t i = 0; i < token.n; ++i) token.p[i] = 7.0f;
        for (size_t i = 0; i < feat.n; ++i) feat.p[i] = 7.0f;
        hope_imgenc_params_t Q = P;
        Q.fc1_b = nullptr;
        if (ie_forward_host(&P, 2, img.p, 1, token.p, feat.p) != HOPE_EINVAL || ie_forward_host(&Q, 0, img.p, 1, token.p, feat.p) != HOPE_EINVAL ||
            ie_forward_host(nullptr, 0, img.p, 1, token.p, feat.p) != HOPE_EINVAL || ie_forward_host(&P, 0, nullptr, 1, token.p, feat.p) != HOPE_EINVAL ||
            ie_forward_host(&P, 0, img.p, 1, nullptr, feat.p) != HOPE_EINVAL || ie_forward_host(&P, 0, img.p, 0, token.p, feat.p) != HOPE_EINVAL ||
            ie_forward_host(&P, 0, img.p + 1, 1, token.p, feat.p) != HOPE_EINVAL)
            FAIL("a bad call was accepted");
        for (size_t i = 0; i < token.n; ++i) if (token.p[i] != 7.0f) FAIL("a refused call wrote to the token");
        for (size_t i = 0; i < feat.n; ++i) if (feat.p[i] != 7.0f) FAIL("a refused call wrote to the features");
    }
    for (Buf<float>* b : w) delete b;
    printf("clean: %lld calls\n", calls);
    return 0;
}
