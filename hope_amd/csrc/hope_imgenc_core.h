/*
 * hope_imgenc_core.h -- the inference forward of HopeNet's image encoder (hope_amd/policy.py _ImgEncoder and re_embed_img; the
 * reference's ImgEncoder / ConvBlock, src/model/network.py:198-299) in ONE arithmetic order, one source for the kernels
 * (hope_imgenc_kernel.h) and the host twin ie_forward_host.
 *
 * Shape, fixed at compile time: img_shape (3, 64, 64), img_conv_layers [4, 8], k_img_conv 3, img_linear_layers [256], embed 128.
 *   x   = u8 image [3][64][64] * (1/255)
 *   b1  = act(maxpool2(conv3x3(x;  3->4, pad 1))) + avgpool2(conv1x1(x;  3->4))      [4][32][32]
 *   b2  = act(maxpool2(conv3x3(b1; 4->8, pad 1))) + avgpool2(conv1x1(b1; 4->8))      [8][16][16]
 *   f   = flatten(b2)                      2048, index c * 256 + y * 16 + x
 *   h   = act(fc1(f))                      2048 -> 256
 *   e   = output_mean(h)                   256 -> 128          (output_std is never used)
 *   tok = re_embed_img.1(tanh(e))          128 -> 128
 * act is tanh (0) or LeakyReLU(0.01) (1).
 *
 * The rule.  float32 values throughout; two kinds of operation, as in hope_policy_core.h:
 *   chain      every convolution output and every Linear output is ONE accumulator that starts at its bias and runs
 *                acc = fmaf(x, w, acc)
 *              over the whole fan-in, no split.  3x3 convolution: ci ascending, then ky, then kx (27 terms in block 1, 36 in block
 *              2); a tap that falls outside the image is EXECUTED with x = +0.0f (the tiles carry a zero border), not skipped.
 *              1x1 convolution: ci ascending.  fc1: k = 0 .. 2047 ascending; output_mean: 256 terms; re_embed_img.1: 128 terms
 *              (pc_chain; the three fan-ins are even, so the matrix instruction's zero term never occurs).  The convolutions run
 *              on the VALU and take no padding term for the odd 27.
 *   float64    everything else is computed in float64 and rounded to float32 once:
 *                pixel      x = (float)u8 * (1.0f / 255.0f): one float32 multiply (torch's img.to(float32) * (1.0 / 255.0))
 *                pooled     a = act(max(c00, c01, c10, c11)): the activation of the maximum of the four chains of a 2x2 window
 *                           (tanh and LeakyReLU are non-decreasing, so this is torch's maxpool(act(.)))
 *                act        tanh = pc_tanh;  leaky(x) = x > 0 ? x : x * 0.01f
 *                shortcut   s = (float)(((double)s00 + s01 + s10 + s11) * 0.25), in the order (0,0), (0,1), (1,0), (1,1)
 *                block      a + s, one float32 addition
 *                h = act(fc1 chain);  e = the output_mean chain;  r = pc_tanh(e);  tok = the re_embed_img.1 chain
 * Finite parameters are the contract.  An image's result depends on that image only.
 */
#pragma once
#include <stdint.h>
#include <math.h>

#include "hope_env.h"
#include "hope_math.h"
#include "hope_policy_core.h"

#define IE_S0 64                                        /* the image's side; 32 behind block 1, 16 behind block 2 */
#define IE_C0 3
#define IE_C1 4
#define IE_C2 8
#define IE_LD0 (IE_S0 + 2)                              /* row strides of the bordered tiles */
#define IE_LD1 (IE_S0 / 2 + 2)
#define IE_TILE0 (IE_C0 * IE_LD0 * IE_LD0)              /* floats of the bordered image, 13 068 */
#define IE_TILE1 (IE_C1 * IE_LD1 * IE_LD1)              /* of the bordered block-1 output, 4 624 */
#define IE_IMG (IE_C0 * IE_S0 * IE_S0)                  /* bytes of an image */
#define IE_FEAT 2048
#define IE_HID 256
#define IE_E 128
#define IE_NPARAM 14                                    /* tensors of hope_imgenc_params_t */

/* the order of hope_imgenc_params_t's fields */
enum { IE_CONV1_W = 0, IE_CONV1_B, IE_SHORT1_W, IE_SHORT1_B, IE_CONV2_W, IE_CONV2_B, IE_SHORT2_W, IE_SHORT2_B, IE_FC1_W, IE_FC1_B, IE_MEAN_W,
       IE_MEAN_B, IE_RE_W, IE_RE_B };

/* floats into the packed buffer: the convolution tensors as torch holds them, the three Linear weights [k][out] */
#define IE_OFF_CONV1_W 0
#define IE_OFF_CONV1_B 108
#define IE_OFF_SHORT1_W 112
#define IE_OFF_SHORT1_B 124
#define IE_OFF_CONV2_W 128
#define IE_OFF_CONV2_B 416
#define IE_OFF_SHORT2_W 424
#define IE_OFF_SHORT2_B 456
#define IE_OFF_FC1_W 464
#define IE_OFF_FC1_B (IE_OFF_FC1_W + IE_FEAT * IE_HID)
#define IE_OFF_MEAN_W (IE_OFF_FC1_B + IE_HID)
#define IE_OFF_MEAN_B (IE_OFF_MEAN_W + IE_HID * IE_E)
#define IE_OFF_RE_W (IE_OFF_MEAN_B + IE_E)
#define IE_OFF_RE_B (IE_OFF_RE_W + IE_E * IE_E)
#define IE_TOTAL (IE_OFF_RE_B + IE_E)

struct IeLayout { int off[IE_NPARAM + 1], n_out[IE_NPARAM], k_in[IE_NPARAM]; };   /* k_in 0: stored as given; else [n_out][k_in] -> [k_in][n_out] */

HM_FN IeLayout ie_layout() {
    IeLayout L = {{IE_OFF_CONV1_W, IE_OFF_CONV1_B, IE_OFF_SHORT1_W, IE_OFF_SHORT1_B, IE_OFF_CONV2_W, IE_OFF_CONV2_B, IE_OFF_SHORT2_W, IE_OFF_SHORT2_B,
                   IE_OFF_FC1_W, IE_OFF_FC1_B, IE_OFF_MEAN_W, IE_OFF_MEAN_B, IE_OFF_RE_W, IE_OFF_RE_B, IE_TOTAL},
                  {0, 0, 0, 0, 0, 0, 0, 0, IE_HID, 0, IE_E, 0, IE_E, 0},
                  {0, 0, 0, 0, 0, 0, 0, 0, IE_FEAT, 0, IE_HID, 0, IE_E, 0}};
    return L;
}

HM_FN bool ie_act_ok(int act) { return act == 0 || act == 1; }

HM_FN float ie_pixel(uint8_t u) { return (float)u * (1.0f / 255.0f); }

template <int ACT>
HM_FN float ie_act(float x) {
    if (ACT == 0) return pc_tanh(x);
    return x > 0.0f ? x : x * 0.01f;
}

HM_FN float ie_max4(float a, float b, float c, float d) {
    float m = a;
    m = b > m ? b : m;
    m = c > m ? c : m;
    m = d > m ? d : m;
    return m;
}

HM_FN float ie_avg4(float s00, float s01, float s10, float s11) { return (float)(((double)s00 + (double)s01 + (double)s10 + (double)s11) * 0.25); }

/* One pooled output pixel of a block, all COUT channels.  p: the top-left of its 4x4 input patch in a bordered tile (row stride ld,
 * channel stride cs; p is 8-byte aligned and ld even, so a patch row is two aligned pairs): rows / columns 1, 2 are the 2x2 window,
 * 0 and 3 its neighbours.  w3 [COUT][CIN][3][3], b3, w1 [COUT][CIN], b1: the block's tensors.  out[co * os] = a + s. */
template <int CIN, int COUT, int ACT>
HM_FN void ie_block_pixel(const float* p, int ld, int cs, const float* w3, const float* b3, const float* w1, const float* b1, float* out, int os) {
    float c[COUT][2][2], s[COUT][2][2];                 /* the 3x3 chains and the shortcut chains of the 2x2 window, every channel */
#pragma unroll
    for (int co = 0; co < COUT; ++co)
#pragma unroll
        for (int dy = 0; dy < 2; ++dy)
#pragma unroll
            for (int dx = 0; dx < 2; ++dx) { c[co][dy][dx] = b3[co]; s[co][dy][dx] = b1[co]; }
    /* an input channel at a time: its 16 patch values feed every chain's next 9 terms (ky, then kx) -- each chain still runs ci
     * ascending, then ky, then kx -- and its 9 COUT + COUT weights fit the scalar registers */
#pragma unroll 1
    for (int ci = 0; ci < CIN; ++ci) {
        float v[4][4];
#pragma unroll
        for (int y = 0; y < 4; ++y) {
#if defined(__HIP_DEVICE_COMPILE__)
            typedef float ie_f2 __attribute__((ext_vector_type(2)));
            const ie_f2 lo = *(const ie_f2*)(p + ci * cs + y * ld), hi = *(const ie_f2*)(p + ci * cs + y * ld + 2);
            v[y][0] = lo.x; v[y][1] = lo.y; v[y][2] = hi.x; v[y][3] = hi.y;
#else
#pragma unroll
            for (int x = 0; x < 4; ++x) v[y][x] = p[ci * cs + y * ld + x];
#endif
        }
#pragma unroll
        for (int co = 0; co < COUT; ++co)
#pragma unroll
            for (int dy = 0; dy < 2; ++dy)
#pragma unroll
                for (int dx = 0; dx < 2; ++dx) {
                    float acc = c[co][dy][dx];
#pragma unroll
                    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                        for (int kx = 0; kx < 3; ++kx) acc = fmaf(v[dy + ky][dx + kx], w3[((co * CIN + ci) * 3 + ky) * 3 + kx], acc);
                    c[co][dy][dx] = acc;
                    s[co][dy][dx] = fmaf(v[dy + 1][dx + 1], w1[co * CIN + ci], s[co][dy][dx]);
                }
    }
#pragma unroll
    for (int co = 0; co < COUT; ++co) {
        const float a = ie_act<ACT>(ie_max4(c[co][0][0], c[co][0][1], c[co][1][0], c[co][1][1]));
        out[co * os] = a + ie_avg4(s[co][0][0], s[co][0][1], s[co][1][0], s[co][1][1]);
    }
}

/* ---- the host twin: one image at a time over torch's tensors ---- */
static inline bool ie_params_ok(const hope_imgenc_params_t* P) {
    if (!P) return false;
    const float* const* t = (const float* const*)P;
    for (int i = 0; i < IE_NPARAM; ++i)
        if (!t[i]) return false;
    return true;
}

/* t0 [IE_TILE0], t1 [IE_TILE1]: the caller's bordered tiles, their borders zero (the interiors are overwritten); feat [2048] */
template <int ACT>
static inline void ie_features_row(const hope_imgenc_params_t* P, const uint8_t* img, float* t0, float* t1, float* feat) {
    for (int c = 0; c < IE_C0; ++c)
        for (int y = 0; y < IE_S0; ++y)
            for (int x = 0; x < IE_S0; ++x) t0[(c * IE_LD0 + y + 1) * IE_LD0 + x + 1] = ie_pixel(img[(c * IE_S0 + y) * IE_S0 + x]);
    for (int y = 0; y < IE_S0 / 2; ++y)
        for (int x = 0; x < IE_S0 / 2; ++x)
            ie_block_pixel<IE_C0, IE_C1, ACT>(t0 + 2 * y * IE_LD0 + 2 * x, IE_LD0, IE_LD0 * IE_LD0, P->conv1_w, P->conv1_b, P->short1_w, P->short1_b,
                                              t1 + (y + 1) * IE_LD1 + x + 1, IE_LD1 * IE_LD1);
    for (int y = 0; y < IE_S0 / 4; ++y)
        for (int x = 0; x < IE_S0 / 4; ++x)
            ie_block_pixel<IE_C1, IE_C2, ACT>(t1 + 2 * y * IE_LD1 + 2 * x, IE_LD1, IE_LD1 * IE_LD1, P->conv2_w, P->conv2_b, P->short2_w, P->short2_b,
                                              feat + y * (IE_S0 / 4) + x, (IE_S0 / 4) * (IE_S0 / 4));
}

template <int ACT>
static inline void ie_head_row(const hope_imgenc_params_t* P, const float* feat, float* tok) {
    float h[IE_HID], r[IE_E];
    for (int o = 0; o < IE_HID; ++o) h[o] = ie_act<ACT>(pc_chain(P->fc1_b[o], feat, 1, P->fc1_w + (long)o * IE_FEAT, 1, IE_FEAT));
    for (int o = 0; o < IE_E; ++o) r[o] = pc_tanh(pc_chain(P->mean_b[o], h, 1, P->mean_w + (long)o * IE_HID, 1, IE_HID));
    for (int o = 0; o < IE_E; ++o) tok[o] = pc_chain(P->re_b[o], r, 1, P->re_w + (long)o * IE_E, 1, IE_E);
}

/* img [batch][3][64][64] uint8 (4-byte aligned, as the device path asks), token [batch][128], feat [batch][2048] or null */
static inline int ie_forward_host(const hope_imgenc_params_t* P, int act, const uint8_t* img, int64_t batch, float* token, float* feat) {
    if (!ie_params_ok(P) || !ie_act_ok(act) || !img || !token || batch < 1) return HOPE_EINVAL;
    if (((uintptr_t)img | (uintptr_t)token | (uintptr_t)feat) & 3) return HOPE_EINVAL;
    float* const work = new float[IE_TILE0 + IE_TILE1 + IE_FEAT]();          /* zero: the borders */
    float *t0 = work, *t1 = work + IE_TILE0, *f = work + IE_TILE0 + IE_TILE1;
    for (int64_t b = 0; b < batch; ++b) {
        float* const fb = feat ? feat + b * IE_FEAT : f;
        if (act == 0) {
            ie_features_row<0>(P, img + b * IE_IMG, t0, t1, fb);
            ie_head_row<0>(P, fb, token + b * IE_E);
        } else {
            ie_features_row<1>(P, img + b * IE_IMG, t0, t1, fb);
            ie_head_row<1>(P, fb, token + b * IE_E);
        }
    }
    delete[] work;
    return HOPE_OK;
}
