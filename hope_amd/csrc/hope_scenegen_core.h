/*
 * hope_scenegen_core.h -- the DETERMINISTIC generator of Normal / Complex / Extrem parking lots, one source for host and device.
 *
 * hope_scenegen.cpp's generator (hope_scenegen_generate) calls glibc's sin / cos / log / sqrt, so no device kernel can reproduce
 * its bits, and its output is pinned by tests and must not change.  This header is the same recipe -- one_case of
 * hope_scenegen.cpp line for line: the same draws in the same order from the same splitmix64 stream keyed by (seed, index), the
 * same rejection rules, the same boundary-only ring predicates, the same bay / parallel choice and map-box rule -- written with
 * operations IEEE-754 defines exactly only: hm_sincos of hope_math.h, sqrt, and sg_log below.  Contraction is off on both
 * compilers (-ffp-contract=off; every fused multiply-add is an explicit fma()), so the host twin (hope_scenegen_generate_det)
 * and the kernel (k_scenegen, hope_scenegen_kernel.h) give the same bits by construction: one lane / one thread per lot, the
 * attempts of a lot tried one after the other on that lot's own stream.
 *
 * No std::vector: a lot holds at most SG_MAX_RINGS = 17 rings (back wall, two sides, 2 x 3 further parked cars, 8 obstacles
 * across the aisle).  The ring list of an attempt lives behind SgRings, a strided view: word w of ring o is base[(o * 8 + w) *
 * stride].  The host passes a local array (stride 1); the kernel passes its lane's column of an LDS array (stride = lanes per
 * block), so that the lanes of a wave read and write consecutive words whatever ring each of them is at.
 */
#pragma once
#include <stdint.h>

#include "hope_math.h"

#define SG_MAX_RINGS 17

/* ---- log ----------------------------------------------------------------------------------------------------- */
/* Natural logarithm of a positive normal double from exact operations: x = 2^e * m with m in (sqrt(1/2), sqrt(2)],
 * log(m) = 2 atanh(s), s = (m - 1) / (m + 1), |s| <= 0.1716, odd series to s^23 (truncation < 1e-18 relative); m - 1 is exact.
 * It only feeds Box-Muller (x in [1e-300, 1)), so it need not be correctly rounded: it must be the same bits on host and device.
 * Worst distance from glibc's log over (0, 1]: tests/test_scenegen_det.py, DESIGN.md. */
HM_FN double sg_log(double x) {
    uint64_t b;
    __builtin_memcpy(&b, &x, 8);
    int e = (int)((b >> 52) & 0x7FF) - 1023;
    b = (b & 0x000FFFFFFFFFFFFFull) | 0x3FF0000000000000ull;
    double m;
    __builtin_memcpy(&m, &b, 8);                                 /* [1, 2) */
    if (m > 1.4142135623730951) { m = m * 0.5; e = e + 1; }
    const double f = m - 1.0;
    const double s = f / (2.0 + f);
    const double z = s * s;
    double p = 0.08695652173913043;                    /* 2 / 23 */
    p = fma(p, z, 0.09523809523809523);                /* 2 / 21 */
    p = fma(p, z, 0.10526315789473684);
    p = fma(p, z, 0.11764705882352941);
    p = fma(p, z, 0.13333333333333333);
    p = fma(p, z, 0.15384615384615385);
    p = fma(p, z, 0.18181818181818182);
    p = fma(p, z, 0.2222222222222222);
    p = fma(p, z, 0.2857142857142857);
    p = fma(p, z, 0.4);
    p = fma(p, z, 0.6666666666666666);                 /* 2 / 3 */
    const double lm = fma(s, z * p, 2.0 * s);          /* log(m) */
    const double ed = (double)e;
    return fma(ed, 0.6931471803691238, fma(ed, 1.9082149292705877e-10, lm));   /* ln 2 in two parts: e * hi is exact */
}

/* ---- configuration (src/configs.py:13-17, 43-70; parking_map_normal.py:20-22) ------------------------------------ */
#define SG_WHEEL_BASE 2.8
#define SG_FRONT_HANG 0.96
#define SG_REAR_HANG 0.93
#define SG_WIDTH 1.94
#define SG_LENGTH (SG_WHEEL_BASE + SG_FRONT_HANG + SG_REAR_HANG)
#define SG_GAP 0.1                                     /* MIN_DIST_TO_OBST */
#define SG_P_WALL 0.5
#define SG_P_EXTRA 0.7
#define SG_N_EXTRA 3
#define SG_PI 3.14159265358979323846

struct SgLevel {
    double min_lot_len, max_lot_len, min_lot_wid, max_lot_wid, para_wall, bay_wall;
    int n_obst;
};
/* 0 Normal, 1 Complex, 2 Extrem (no bay lots at the Extrem level) */
HM_FN SgLevel sg_level(int level) {
    SgLevel L;
    if (level == 0) { L.min_lot_len = SG_LENGTH * 1.25; L.max_lot_len = SG_LENGTH * 1.25 + 0.5; L.min_lot_wid = SG_WIDTH + 0.85; L.max_lot_wid = SG_WIDTH + 1.2; L.para_wall = 4.5; L.bay_wall = 7.0; L.n_obst = 3; }
    else if (level == 1) { L.min_lot_len = SG_LENGTH + 0.9; L.max_lot_len = SG_LENGTH * 1.25; L.min_lot_wid = SG_WIDTH + 0.4; L.max_lot_wid = SG_WIDTH + 0.85; L.para_wall = 4.0; L.bay_wall = 6.0; L.n_obst = 5; }
    else { L.min_lot_len = SG_LENGTH + 0.6; L.max_lot_len = SG_LENGTH + 0.9; L.min_lot_wid = 0.0; L.max_lot_wid = 0.0; L.para_wall = 3.5; L.bay_wall = 0.0; L.n_obst = 8; }
    return L;
}

HM_FN double sg_min(double a, double b) { return b < a ? b : a; }      /* std::min / std::max */
HM_FN double sg_max(double a, double b) { return a < b ? b : a; }

/* ---- splitmix64 stream + Box-Muller ------------------------------------------------------------------------------ */
struct SgRng {
    uint64_t s;
    int have;
    double spare;
};
HM_FN uint64_t sg_next(SgRng& r) {
    uint64_t z = (r.s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
HM_FN double sg_uni(SgRng& r) { return (double)(sg_next(r) >> 11) * (1.0 / 9007199254740992.0); }          /* [0, 1) */
HM_FN double sg_normal(SgRng& r) {
    if (r.have) { r.have = 0; return r.spare; }
    double u1 = sg_uni(r);
    const double u2 = sg_uni(r);
    if (u1 < 1e-300) u1 = 1e-300;
    const double rad = sqrt(-2.0 * sg_log(u1)), a = 2.0 * SG_PI * u2;
    double sn, cs;
    hm_sincos(a, &sn, &cs);
    r.spare = rad * sn;
    r.have = 1;
    return rad * cs;
}
/* the stream of lot `index` of `seed` (hope_scenegen_generate's keying; the first output is discarded there too) */
HM_FN SgRng sg_rng(uint64_t seed, int64_t index) {
    SgRng r;
    r.s = seed * 0x9E3779B97F4A7C15ull + (uint64_t)index * 0xD1B54A32D192ED03ull + 0x8CB92BA72F3D8DD7ull;
    r.have = 0;
    r.spare = 0.0;
    sg_next(r);
    return r;
}
HM_FN double sg_clipn(SgRng& r, double mean, double sd, double lo, double hi) { return sg_min(hi, sg_max(lo, sg_normal(r) * sd + mean)); }
HM_FN double sg_uniform(SgRng& r, double lo, double hi) { return sg_uni(r) * (hi - lo) + lo; }

/* ---- rings --------------------------------------------------------------------------------------------------- */
struct SgQuad { double x[4], y[4]; };

struct SgRings {                                       /* strided view of up to SG_MAX_RINGS rings of 8 words (x0 y0 .. x3 y3) */
    double* base;
    int stride;
};
HM_FN void sg_put(const SgRings& R, int o, const SgQuad& q) {
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int k = 0; k < 4; k++) { R.base[(size_t)((o * 8 + 2 * k) * R.stride)] = q.x[k]; R.base[(size_t)((o * 8 + 2 * k + 1) * R.stride)] = q.y[k]; }
}
HM_FN SgQuad sg_get(const SgRings& R, int o) {
    SgQuad q;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int k = 0; k < 4; k++) { q.x[k] = R.base[(size_t)((o * 8 + 2 * k) * R.stride)]; q.y[k] = R.base[(size_t)((o * 8 + 2 * k + 1) * R.stride)]; }
    return q;
}

HM_FN SgQuad sg_quad(double x0, double y0, double x1, double y1, double x2, double y2, double x3, double y3) {
    SgQuad q;
    q.x[0] = x0; q.y[0] = y0; q.x[1] = x1; q.y[1] = y1; q.x[2] = x2; q.y[2] = y2; q.x[3] = x3; q.y[3] = y3;
    return q;
}
HM_FN SgQuad sg_create_box(double x, double y, double yaw) {   /* State.create_box (vehicle.py:32-36) */
    double s, c;
    hm_sincos(yaw, &s, &c);
    const double bx[4] = {-SG_REAR_HANG, SG_FRONT_HANG + SG_WHEEL_BASE, SG_FRONT_HANG + SG_WHEEL_BASE, -SG_REAR_HANG};
    const double by[4] = {-SG_WIDTH / 2, -SG_WIDTH / 2, SG_WIDTH / 2, SG_WIDTH / 2};
    SgQuad q;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int k = 0; k < 4; k++) { q.x[k] = c * bx[k] + (-s) * by[k] + x; q.y[k] = s * bx[k] + c * by[k] + y; }
    return q;
}
HM_FN double sg_cross(double ax, double ay, double bx, double by) { return ax * by - ay * bx; }
HM_FN int sg_sgn(double v) { return (v > 0) - (v < 0); }

/* LinearRing.intersects(LinearRing): any pair of boundary segments shares a point */
HM_FN bool sg_rings_intersect(const SgQuad& a, const SgQuad& b) {
    bool hit = false;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int i = 0; i < 4; i++) {
        const double p1x = a.x[i], p1y = a.y[i], p2x = a.x[(i + 1) & 3], p2y = a.y[(i + 1) & 3];
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int j = 0; j < 4; j++) {
            const double q1x = b.x[j], q1y = b.y[j], q2x = b.x[(j + 1) & 3], q2y = b.y[(j + 1) & 3];
            if (!(sg_min(p1x, p2x) <= sg_max(q1x, q2x) && sg_min(p1y, p2y) <= sg_max(q1y, q2y) &&
                  sg_min(q1x, q2x) <= sg_max(p1x, p2x) && sg_min(q1y, q2y) <= sg_max(p1y, p2y)))
                continue;
            const double d1 = sg_cross(p2x - p1x, p2y - p1y, q1x - p1x, q1y - p1y);
            const double d2 = sg_cross(p2x - p1x, p2y - p1y, q2x - p1x, q2y - p1y);
            const double d3 = sg_cross(q2x - q1x, q2y - q1y, p1x - q1x, p1y - q1y);
            const double d4 = sg_cross(q2x - q1x, q2y - q1y, p2x - q1x, p2y - q1y);
            if (sg_sgn(d1) * sg_sgn(d2) <= 0 && sg_sgn(d3) * sg_sgn(d4) <= 0) hit = true;
        }
    }
    return hit;
}
HM_FN double sg_pt_seg(double px, double py, double ax, double ay, double bx, double by) {
    const double abx = bx - ax, aby = by - ay, den = abx * abx + aby * aby;
    double t = den > 0 ? ((px - ax) * abx + (py - ay) * aby) / den : 0.0;
    t = sg_min(1.0, sg_max(0.0, t));
    const double cx = ax + t * abx, cy = ay + t * aby;
    return sqrt((px - cx) * (px - cx) + (py - cy) * (py - cy));
}
/* LinearRing.distance(LinearRing): 0 when they meet, else the closest vertex-to-edge gap */
HM_FN double sg_rings_distance(const SgQuad& a, const SgQuad& b) {
    if (sg_rings_intersect(a, b)) return 0.0;
    double d = 1e300;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int i = 0; i < 4; i++)
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int j = 0; j < 4; j++) {
            d = sg_min(d, sg_pt_seg(a.x[i], a.y[i], b.x[j], b.y[j], b.x[(j + 1) & 3], b.y[(j + 1) & 3]));
            d = sg_min(d, sg_pt_seg(b.x[i], b.y[i], a.x[j], a.y[j], a.x[(j + 1) & 3], a.y[(j + 1) & 3]));
        }
    return d;
}
HM_FN void sg_polar(SgRng& r, double ox, double oy, double a0, double a1, double r0, double r1, double* px, double* py) {
    const double ang = sg_clipn(r, (a0 + a1) / 2, (a1 - a0) / 4, a0, a1);
    const double rad = sg_clipn(r, (r0 + r1) / 2, (r1 - r0) / 4, r0, r1);
    double s, c;
    hm_sincos(ang, &s, &c);
    *px = ox + c * rad;
    *py = oy + s * rad;
}

/* what is fixed for a (level, bay) pair */
struct SgCfg {
    double half, space_hi, space_lo, wall, yaw0, pitch, yaw_lo, yaw_hi;
    int low_a, low_b, n_extra, n_far, bay;
};
HM_FN SgCfg sg_cfg(int level, bool bay) {
    const SgLevel L = sg_level(level);
    SgCfg c;
    c.bay = bay ? 1 : 0;
    c.half = bay ? 15.0 : 18.0;
    c.n_far = L.n_obst;
    if (bay) {
        c.space_hi = L.max_lot_wid - SG_WIDTH; c.space_lo = L.min_lot_wid - SG_WIDTH;
        c.wall = L.bay_wall; c.yaw0 = SG_PI / 2; c.pitch = SG_WIDTH;
        c.yaw_lo = SG_PI * 5 / 12; c.yaw_hi = SG_PI * 7 / 12;
        c.low_a = 0; c.low_b = 3;                       /* rear-right, rear-left corners touch the back wall */
        c.n_extra = SG_N_EXTRA;
    } else {
        c.space_hi = L.max_lot_len - SG_LENGTH; c.space_lo = L.min_lot_len - SG_LENGTH;
        c.wall = L.para_wall; c.yaw0 = 0.0; c.pitch = SG_LENGTH;
        c.yaw_lo = -SG_PI / 12; c.yaw_hi = SG_PI / 12;
        c.low_a = 0; c.low_b = 1;                       /* rear-right, front-right */
        c.n_extra = SG_N_EXTRA - 1;
    }
    return c;
}

HM_FN void sg_slot_pose(const SgCfg& C, SgRng& rng, double x, double* pose) {
    const double yaw = sg_clipn(rng, C.yaw0, SG_PI / 36, C.yaw_lo, C.yaw_hi);
    const SgQuad b = sg_create_box(x, 0.0, yaw);
    const double ya = b.y[0], yb = C.bay ? b.y[3] : b.y[1];          /* corners low_a, low_b */
    const double y_min = -sg_min(ya, yb) + SG_GAP;
    const double y = sg_clipn(rng, y_min + 0.4, 0.2, y_min, y_min + 0.8);
    pose[0] = x; pose[1] = y; pose[2] = yaw;
}

/* obstacle next to the slot on side `sign` (-1 left, +1 right): a wall-like quad or a parked car followed by further parked
 * cars (each kept with probability .7, appended to the ring list at *n) */
HM_FN SgQuad sg_side(const SgCfg& C, SgRng& rng, int sign, double nax, double nay, double nbx, double nby, double d_lo, double d_hi,
                     const SgRings& R, int* n) {
    if (sg_uni(rng) < SG_P_WALL) {
        const double a0 = sign < 0 ? SG_PI * 11 / 12 : -SG_PI / 12, a1 = sign < 0 ? SG_PI * 13 / 12 : SG_PI / 12;
        double pax, pay, pbx, pby;
        sg_polar(rng, nax, nay, a0, a1, d_lo, d_hi, &pax, &pay);
        sg_polar(rng, nbx, nby, a0, a1, d_lo, d_hi, &pbx, &pby);
        if (sign < 0) return sg_quad(pax, pay, pbx, pby, -C.half, 0.0, -C.half, pay);
        return sg_quad(C.half, pay, C.half, 0.0, pbx, pby, pax, pay);
    }
    double x = sign * (C.pitch + sg_uniform(rng, d_lo, d_hi));
    double pose[3];
    sg_slot_pose(C, rng, x, pose);
    const SgQuad first = sg_create_box(pose[0], pose[1], pose[2]);
    for (int k = 0; k < C.n_extra; k++) {
        x += sign * (C.pitch + SG_GAP + sg_uniform(rng, d_lo, d_hi));
        const double y = pose[1] + sg_clipn(rng, 0, 0.05, -0.1, 0.1);
        pose[0] = x; pose[1] = y; pose[2] = sg_clipn(rng, C.yaw0, SG_PI / 36, C.yaw_lo, C.yaw_hi);
        const SgQuad ring = sg_create_box(pose[0], pose[1], pose[2]);
        if (sg_uni(rng) < SG_P_EXTRA) { sg_put(R, *n, ring); *n = *n + 1; }
    }
    return first;
}

/* one rejection-sampling attempt of generate_bay_parking_case (bay) / generate_parallel_parking_case; false: rejected.
 * On success: start / dest poses and rings 0 .. *n_rings - 1 of R (back wall, left, right, further cars, across the aisle). */
HM_FN bool sg_one_case(const SgCfg& C, SgRng& rng, const SgRings& R, double* start, double* dest_out, int* n_rings) {
    const double half = C.half;
    double dest[3];
    sg_slot_pose(C, rng, 0.0, dest);
    const SgQuad dest_ring = sg_create_box(dest[0], dest[1], dest[2]);
    /* rb = p[0], rf = p[1], lf = p[2], lb = p[3] */
    bool ok = true;
    int n = 3;                                          /* 0 back wall, 1 left, 2 right; the further cars follow as they are drawn */
    sg_put(R, 0, sg_quad(half, 0.0, half, -1.0, -half, -1.0, -half, 0.0));
    const SgQuad left = C.bay ? sg_side(C, rng, -1, dest_ring.x[2], dest_ring.y[2], dest_ring.x[3], dest_ring.y[3], C.space_hi / 5 * 1, C.space_hi / 5 * 4, R, &n)
                              : sg_side(C, rng, -1, dest_ring.x[3], dest_ring.y[3], dest_ring.x[0], dest_ring.y[0], C.space_lo / 5 * 1, C.space_hi / 5 * 4, R, &n);
    sg_put(R, 1, left);
    const double gap_l = sg_rings_distance(dest_ring, left);
    const double d_lo = sg_max(C.space_lo - gap_l, 0.0) + SG_GAP, d_hi = sg_max(C.space_hi - gap_l, 0.0) + SG_GAP;
    const SgQuad right = C.bay ? sg_side(C, rng, +1, dest_ring.x[1], dest_ring.y[1], dest_ring.x[0], dest_ring.y[0], d_lo, d_hi, R, &n)
                               : sg_side(C, rng, +1, dest_ring.x[2], dest_ring.y[2], dest_ring.x[1], dest_ring.y[1], d_lo, d_hi, R, &n);
    sg_put(R, 2, right);
    const double gap_r = sg_rings_distance(dest_ring, right);
    if (gap_r + gap_l < C.space_lo || gap_r + gap_l > C.space_hi || gap_l < SG_GAP || gap_r < SG_GAP) ok = false;
    double top = -1e300;
    for (int o = 0; o < n; o++) {
        const SgQuad r = sg_get(R, o);
        if (sg_rings_intersect(r, dest_ring)) ok = false;
        for (int k = 0; k < 4; k++) top = sg_max(top, r.y[k]);
    }
    top += SG_GAP;
    const int far0 = n;
    if (sg_uni(rng) < 0.2) {                            /* only a thin wall across the aisle */
        const double y0 = C.wall + top + SG_GAP;
        sg_put(R, n, sg_quad(-half, y0, half, y0, half, y0 + 0.1, -half, y0 + 0.1));
        n++;
    } else {
        const SgQuad zone = sg_quad(-half, C.wall + top, half, C.wall + top, half, C.wall + top + 8, -half, C.wall + top + 8);
        for (int k = 0; k < C.n_far; k++) {
            const double px = sg_uniform(rng, -half + 2, half - 2), py = sg_uniform(rng, C.wall + top + 2, C.wall + top + 6), pyaw = sg_uni(rng) * SG_PI * 2;
            SgQuad ring = sg_create_box(px, py, pyaw);
            for (int v = 0; v < 4; v++) { ring.x[v] += 0.5 * sg_uni(rng); ring.y[v] += 0.5 * sg_uni(rng); }
            bool hit = sg_rings_intersect(ring, zone);
            for (int o = far0; o < n && !hit; o++) hit = sg_rings_intersect(ring, sg_get(R, o));
            if (!hit) { sg_put(R, n, ring); n++; }
        }
    }
    double sx, sy, syaw;
    for (;;) {                                          /* start pose in the aisle, clear of everything */
        sx = sg_uniform(rng, -half / 2, half / 2);
        sy = sg_uniform(rng, top + 1, C.wall + top - 1);
        syaw = sg_clipn(rng, 0, SG_PI / 6, -SG_PI / 2, SG_PI / 2);
        if (sg_uni(rng) < 0.5) syaw += SG_PI;
        const SgQuad sbox = sg_create_box(sx, sy, syaw);
        bool hit = sg_rings_intersect(dest_ring, sbox);
        for (int o = 0; o < n && !hit; o++) hit = sg_rings_intersect(sg_get(R, o), sbox);
        if (!hit) break;
    }
    if (!C.bay && hm_cos(syaw) < 0) {                   /* parallel: face the slot the way the car arrives */
        const SgQuad b = dest_ring;                     /* _flip_box_orientation (parking_map_dlp.py:117-123) */
        const double cx = 0.25 * (b.x[0] + b.x[1] + b.x[2] + b.x[3]), cy = 0.25 * (b.y[0] + b.y[1] + b.y[2] + b.y[3]);
        dest[0] = 2 * cx - dest[0]; dest[1] = 2 * cy - dest[1]; dest[2] += SG_PI;
    }
    if (!ok) return false;
    start[0] = sx; start[1] = sy; start[2] = syaw;
    dest_out[0] = dest[0]; dest_out[1] = dest[1]; dest_out[2] = dest[2];
    *n_rings = n;
    return true;
}

/* lot `index` of (seed, level): attempts until one is accepted.  bay_mode: -1 as ParkingMapNormal.reset (bay with probability
 * 1/2 for Normal / Complex), 0 parallel only, 1 bay only.  Writes start [3], dest [3], bbox [4] (floor / ceil of min / max(start,
 * dest) -/+ 10 m), the rings into R; returns the ring count, *case_id = 0 bay / 1 parallel. */
HM_FN int sg_generate_lot(int level, int bay_mode, uint64_t seed, int64_t index, const SgRings& R, double* start, double* dest,
                          double* bbox, int* case_id) {
    SgRng rng = sg_rng(seed, index);
    const bool bay = level != 2 && (bay_mode == 1 || (bay_mode < 0 && sg_uni(rng) > 0.5));
    const SgCfg C = sg_cfg(level, bay);
    int n = 0;
    while (!sg_one_case(C, rng, R, start, dest, &n)) {}
    bbox[0] = floor(sg_min(start[0], dest[0]) - 10); bbox[1] = ceil(sg_max(start[0], dest[0]) + 10);
    bbox[2] = floor(sg_min(start[1], dest[1]) - 10); bbox[3] = ceil(sg_max(start[1], dest[1]) + 10);
    *case_id = bay ? 0 : 1;
    return n;
}
