/*
 * hope_maplevel_core.h -- the difficulty label of a parking map (`get_map_level`), one source for host and device.
 *
 * A restatement of hope_amd/map_level.py (which names the reference lines: src/env/map_level.py:13-25, :27-112, :139-154) in plain
 * C++, function for function: ml_pt_seg / ml_point_ring (_pt_seg, point_ring_distance), ml_segs_meet (_segs_meet), ml_pair_term
 * (one (i, j) term of rings_cross + ring_ring_distance), ml_min_area_rect (_convex_hull + min_area_rectangle), ml_poly_meets_ring
 * (polygon_meets_ring) and ml_classify (_surrounding, _has_enough_space, _check_extrem and get_map_level itself).  Only operations
 * IEEE-754 defines exactly are used (+ - * / sqrt and compares; hope_math.h for sin / cos / hypot) and contraction is off on both
 * compilers, so the host compiler and hipcc give the same bits.  The geometry is that of map_level.py, i.e. parity-unpinned against
 * GEOS like the rest of that slice; it differs from the Python file only where Python calls the platform's cos / sin / hypot.
 *
 * The control flow lives in ml_classify<Ops> once.  What differs between a serial host loop and a wavefront is HOW a set of
 * obstacles is scanned, so that is what Ops supplies: prepare / nearest (the four nearest-obstacle searches), ring_box (the <= 4
 * ring-to-box distances), meets (how many obstacles touch the free rectangle) and work / leader / sync (the 64-double work area of
 * the hull code, written by one lane).  Every reduction an Ops performs is order-independent by construction:
 *   - a minimum over a set of doubles does not depend on the order;
 *   - the argmin of `nearest` is over (distance, index) with the LOWER INDEX winning equal distances, which is what the Python
 *     loop's strict `<` in ascending index order returns;
 *   - `meets` returns a count (all obstacles) or stops at the first hit (the label needs only count != 0).
 * MlHostOps below is the serial form; MlWaveOps (hope_maplevel_kernel.h) the wavefront's.
 *
 * Rings: the library's 4-vertex slot, x, y pairs; a triangle repeats its last vertex in slot 3.  Such a slot is read as a ring of
 * THREE vertices (nv = 3: edges 0-1, 1-2, 2-0), so the zero-length edge 2-3 never reaches ml_pt_seg / ml_segs_meet and the slot
 * answers exactly as the 3-vertex ring does in Python.
 */
#pragma once
#include <math.h>
#include <stdint.h>

#include "hope_math.h"

#if defined(__HIPCC__)
#define ML_MFN __host__ __device__ __forceinline__
#else
#define ML_MFN inline
#endif

#define ML_NORMAL 0
#define ML_COMPLEX 1
#define ML_EXTREM 2

/* which `return` fired (detail word 4) */
#define ML_B_FEW 1            /* n_obst <= 1                                                      -> Normal  */
#define ML_B_EXTREM_FAR_LEN 2 /* _check_extrem: start > 30 m away, slot shorter than the Normal one -> Extrem  */
#define ML_B_EXTREM_FAR_WID 3 /* _check_extrem: start > 30 m away, slot narrower than the Normal one -> Extrem */
#define ML_B_EXTREM_LEN 4     /* _check_extrem: slot shorter than EXTREM_PARK_LOT_LENGTH          -> Extrem  */
#define ML_B_BAY_EARLY 5      /* bay: far or narrow                                               -> Complex */
#define ML_B_BAY_FREE 6       /* bay: free rectangle clear                                        -> Normal  */
#define ML_B_BAY_BLOCKED 7    /* bay: an obstacle meets the free rectangle                        -> Complex */
#define ML_B_PAR_EARLY 8      /* parallel: far or short                                           -> Complex */
#define ML_B_PAR_FREE 9
#define ML_B_PAR_BLOCKED 10
#define ML_B_OPEN 11          /* neither a left-right nor a front-back pair                       -> Normal  */
#define ML_B_OTHER 12         /* the last return                                                  -> Complex */

#define ML_DETAIL_WORDS 8
#define ML_WORK_WORDS 64      /* 9 points, <= 18 hull points + 1, the rectangle */
#define ML_W_HULL 18
#define ML_W_RECT 56
#define ML_NONE 0x7fffffff    /* argmin index of "nothing closer than the limit" */

/* configs.py:13-17, :43-65, :74; map_level.py:11 -- evaluated as hope_amd/map_level.py evaluates them */
#define ML_WHEEL_BASE 2.8
#define ML_FRONT_HANG 0.96
#define ML_REAR_HANG 0.93
#define ML_WIDTH 1.94
#define ML_LENGTH (ML_WHEEL_BASE + ML_FRONT_HANG + ML_REAR_HANG)
#define ML_MIN_LOT_LEN_NORMAL (ML_LENGTH * 1.25)
#define ML_MIN_LOT_WID_NORMAL (ML_WIDTH + 0.85)
#define ML_EXTREM_LOT_LEN ((ML_LENGTH * 1.2) < (ML_LENGTH + 0.9) ? (ML_LENGTH * 1.2) : (ML_LENGTH + 0.9))
#define ML_MAX_DRIVE 15.0
#define ML_BAY_REACH (7.0 - 0.5)
#define ML_PAR_REACH (4.5 - 0.5)

struct MlRing { double x[4], y[4]; int nv; };
struct MlDetail { int32_t found[4]; int32_t branch, far, count; };

HM_FN double ml_sel4(double a0, double a1, double a2, double a3, int i) { return i == 0 ? a0 : (i == 1 ? a1 : (i == 2 ? a2 : a3)); }
HM_FN double ml_vx(const MlRing& r, int i) { return ml_sel4(r.x[0], r.x[1], r.x[2], r.x[3], i); }
HM_FN double ml_vy(const MlRing& r, int i) { return ml_sel4(r.y[0], r.y[1], r.y[2], r.y[3], i); }
HM_FN int ml_next(const MlRing& r, int i) { return i == r.nv - 1 ? 0 : i + 1; }

HM_FN MlRing ml_load_ring(const double* v) {
    MlRing r;
    r.x[0] = v[0]; r.y[0] = v[1]; r.x[1] = v[2]; r.y[1] = v[3]; r.x[2] = v[4]; r.y[2] = v[5]; r.x[3] = v[6]; r.y[3] = v[7];
    r.nv = (r.x[3] == r.x[2] && r.y[3] == r.y[2]) ? 3 : 4;
    return r;
}

/* _pt_seg */
HM_FN double ml_pt_seg(double px, double py, double ax, double ay, double bx, double by) {
    const double dx = bx - ax, dy = by - ay;
    const double l2 = dx * dx + dy * dy;
    if (l2 == 0.0) return hm_hypot(px - ax, py - ay);
    const double r = ((px - ax) * dx + (py - ay) * dy) / l2;
    if (r <= 0.0) return hm_hypot(px - ax, py - ay);
    if (r >= 1.0) return hm_hypot(px - bx, py - by);
    return fabs((ay - py) * dx - (ax - px) * dy) / sqrt(l2);
}

/* point_ring_distance */
HM_FN double ml_point_ring(double px, double py, const MlRing& r) {
    double m = INFINITY;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int i = 0; i < 4; i++) {
        if (i < r.nv) {
            const int j = ml_next(r, i);
            const double d = ml_pt_seg(px, py, r.x[i], r.y[i], ml_vx(r, j), ml_vy(r, j));
            if (d < m) m = d;
        }
    }
    return m;
}

HM_FN int ml_orient(double ax, double ay, double bx, double by, double cx, double cy) {
    const double d = (bx - ax) * (cy - ay) - (by - ay) * (cx - ax);
    return (d > 0 ? 1 : 0) - (d < 0 ? 1 : 0);
}
HM_FN double ml_max(double a, double b) { return a > b ? a : b; }
HM_FN double ml_min(double a, double b) { return a < b ? a : b; }

/* _segs_meet */
HM_FN bool ml_segs_meet(double p1x, double p1y, double p2x, double p2y, double q1x, double q1y, double q2x, double q2y) {
    if (ml_max(p1x, p2x) < ml_min(q1x, q2x) || ml_max(q1x, q2x) < ml_min(p1x, p2x) || ml_max(p1y, p2y) < ml_min(q1y, q2y) ||
        ml_max(q1y, q2y) < ml_min(p1y, p2y))
        return false;
    const int o1 = ml_orient(p1x, p1y, p2x, p2y, q1x, q1y), o2 = ml_orient(p1x, p1y, p2x, p2y, q2x, q2y);
    if (o1 * o2 > 0) return false;
    const int o3 = ml_orient(q1x, q1y, q2x, q2y, p1x, p1y), o4 = ml_orient(q1x, q1y, q2x, q2y, p2x, p2y);
    return o3 * o4 <= 0;
}

/* One (i, j) term of ring_ring_distance(a, b): whether edge i of a meets edge j of b (rings_cross), and the smaller of the
 * distances vertex i of a -> edge j of b and vertex i of b -> edge j of a (+inf where i or j is beyond a ring's vertex count).
 * ring_ring_distance = 0 if any term crosses, else the minimum of the 16 terms. */
HM_FN double ml_pair_term(const MlRing& a, const MlRing& b, int i, int j, bool* cross) {
    const int ia = ml_next(a, i), ja = ml_next(a, j), jb = ml_next(b, j);
    double t = INFINITY;
    *cross = false;
    if (i < a.nv && j < b.nv) {
        *cross = ml_segs_meet(ml_vx(a, i), ml_vy(a, i), ml_vx(a, ia), ml_vy(a, ia), ml_vx(b, j), ml_vy(b, j), ml_vx(b, jb), ml_vy(b, jb));
        t = ml_pt_seg(ml_vx(a, i), ml_vy(a, i), ml_vx(b, j), ml_vy(b, j), ml_vx(b, jb), ml_vy(b, jb));
    }
    if (i < b.nv && j < a.nv) {
        const double u = ml_pt_seg(ml_vx(b, i), ml_vy(b, i), ml_vx(a, j), ml_vy(a, j), ml_vx(a, ja), ml_vy(a, ja));
        if (u < t) t = u;
    }
    return t;
}

/* ring_ring_distance, serially */
HM_FN double ml_ring_ring(const MlRing& a, const MlRing& b) {
    double m = INFINITY;
    bool any = false;
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) {
            bool c;
            const double t = ml_pair_term(a, b, i, j, &c);
            any = any || c;
            if (t < m) m = t;
        }
    return any ? 0.0 : m;
}

/* _create_box: rb, rf, lf, lb */
HM_FN MlRing ml_box(double px, double py, double c, double s) {
    const double bx[4] = {-ML_REAR_HANG, ML_FRONT_HANG + ML_WHEEL_BASE, ML_FRONT_HANG + ML_WHEEL_BASE, -ML_REAR_HANG};
    const double by[4] = {-ML_WIDTH / 2, -ML_WIDTH / 2, ML_WIDTH / 2, ML_WIDTH / 2};
    MlRing r;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int k = 0; k < 4; k++) { r.x[k] = c * bx[k] - s * by[k] + px; r.y[k] = s * bx[k] + c * by[k] + py; }
    r.nv = 4;
    return r;
}

/* polygon_meets_ring: the filled convex quadrilateral `poly` against the closed curve `ring` */
HM_FN bool ml_poly_meets_ring(const MlRing& poly, const MlRing& ring) {
    bool hit = false;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int i = 0; i < 4; i++) {
        const int i2 = (i + 1) & 3;
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int j = 0; j < 4; j++) {
            if (j < ring.nv) {
                const int j2 = ml_next(ring, j);
                hit = hit || ml_segs_meet(poly.x[i], poly.y[i], poly.x[i2], poly.y[i2], ring.x[j], ring.y[j], ml_vx(ring, j2), ml_vy(ring, j2));
            }
        }
    }
    if (hit) return true;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int k = 0; k < 4; k++) {                               /* _inside_convex of every vertex (slot 3 of a triangle repeats slot 2) */
        bool ge = true, le = true;
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int i = 0; i < 4; i++) {
            const int i2 = (i + 1) & 3;
            const int o = ml_orient(poly.x[i], poly.y[i], poly.x[i2], poly.y[i2], ring.x[k], ring.y[k]);
            ge = ge && o >= 0; le = le && o <= 0;
        }
        hit = hit || ge || le;
    }
    return hit;
}

/* _convex_hull + min_area_rectangle over the n <= 9 points w[0 .. 2 n) (x, y pairs; overwritten).  The rectangle's corners go to
 * w[ML_W_RECT .. + 8).  One thread; w is ML_WORK_WORDS doubles of addressable memory (LDS on the device). */
HM_FN void ml_min_area_rect(double* w, int n) {
    for (int i = 1; i < n; i++) {                               /* sorted(set(points)): by x, then y */
        const double x = w[2 * i], y = w[2 * i + 1];
        int j = i;
        while (j > 0 && (w[2 * j - 2] > x || (w[2 * j - 2] == x && w[2 * j - 1] > y))) { w[2 * j] = w[2 * j - 2]; w[2 * j + 1] = w[2 * j - 1]; j--; }
        w[2 * j] = x; w[2 * j + 1] = y;
    }
    int m = 0;
    for (int i = 0; i < n; i++)
        if (m == 0 || w[2 * i] != w[2 * m - 2] || w[2 * i + 1] != w[2 * m - 1]) { w[2 * m] = w[2 * i]; w[2 * m + 1] = w[2 * i + 1]; m++; }
    double* h = w + ML_W_HULL;
    int hn = 0;
    if (m <= 2) {
        for (int i = 0; i < 2 * m; i++) h[i] = w[i];
        hn = m;
    } else {
        int k = 0;
        for (int i = 0; i < m; i++) {                           /* lower chain */
            const double x = w[2 * i], y = w[2 * i + 1];
            while (k >= 2 && ((h[2 * k - 2] - h[2 * k - 4]) * (y - h[2 * k - 3]) - (h[2 * k - 1] - h[2 * k - 3]) * (x - h[2 * k - 4])) <= 0) k--;
            h[2 * k] = x; h[2 * k + 1] = y; k++;
        }
        k--;                                                    /* lo[:-1] */
        const int base = k;
        for (int i = m - 1; i >= 0; i--) {                      /* upper chain */
            const double x = w[2 * i], y = w[2 * i + 1];
            while (k - base >= 2 && ((h[2 * k - 2] - h[2 * k - 4]) * (y - h[2 * k - 3]) - (h[2 * k - 1] - h[2 * k - 3]) * (x - h[2 * k - 4])) <= 0) k--;
            h[2 * k] = x; h[2 * k + 1] = y; k++;
        }
        k--;                                                    /* up[:-1] */
        hn = k;
    }
    double* out = w + ML_W_RECT;
    for (int i = 0; i < 4; i++) { out[2 * i] = h[0]; out[2 * i + 1] = h[1]; }   /* (no edge of non-zero length: Python has no answer) */
    double best = INFINITY;
    for (int e = 0; e < hn; e++) {
        const int e2 = e + 1 == hn ? 0 : e + 1;
        const double ax = h[2 * e], ay = h[2 * e + 1];
        const double ex = h[2 * e2] - ax, ey = h[2 * e2 + 1] - ay;
        const double len = hm_hypot(ex, ey);
        if (len == 0) continue;
        const double ux = ex / len, uy = ey / len;
        double s0 = 0, s1 = 0, t0 = 0, t1 = 0;
        for (int q = 0; q < hn; q++) {
            const double x = h[2 * q], y = h[2 * q + 1];
            const double s = (x - ax) * ux + (y - ay) * uy;
            const double t = (-(x - ax)) * uy + (y - ay) * ux;
            if (q == 0) { s0 = s1 = s; t0 = t1 = t; }
            else { if (s < s0) s0 = s; if (s > s1) s1 = s; if (t < t0) t0 = t; if (t > t1) t1 = t; }
        }
        const double area = (s1 - s0) * (t1 - t0);
        if (area < best) {
            best = area;
            out[0] = ax + ux * s0 - uy * t0; out[1] = ay + uy * s0 + ux * t0;
            out[2] = ax + ux * s1 - uy * t0; out[3] = ay + uy * s1 + ux * t0;
            out[4] = ax + ux * s1 - uy * t1; out[5] = ay + uy * s1 + ux * t1;
            out[6] = ax + ux * s0 - uy * t1; out[7] = ay + uy * s0 + ux * t1;
        }
    }
}

/* get_map_level.  start / dest: x, y, heading; n obstacles behind ops.  count_all: count every obstacle that meets the free rectangle
 * (the detail record) instead of stopping at the first.  Returns ML_NORMAL / ML_COMPLEX / ML_EXTREM and fills D. */
template <class Ops>
HM_FN int ml_classify(Ops& ops, double sx, double sy, double sh, double dx, double dy, double dh, int n, bool count_all, MlDetail& D) {
    D.found[0] = D.found[1] = D.found[2] = D.found[3] = -1;
    D.branch = ML_B_FEW; D.far = 0; D.count = 0;
    if (n <= 1) return ML_NORMAL;
    double c, s;
    hm_sincos(dh, &s, &c);
    const MlRing box = ml_box(dx, dy, c, s);                    /* rb, rf, lf, lb = 0, 1, 2, 3 */
    /* _surrounding: the mid-points of the left, right, front and back edge; each obstacle used at most once */
    const double px[4] = {(box.x[2] + box.x[3]) / 2, (box.x[1] + box.x[0]) / 2, (box.x[2] + box.x[1]) / 2, (box.x[3] + box.x[0]) / 2};
    const double py[4] = {(box.y[2] + box.y[3]) / 2, (box.y[1] + box.y[0]) / 2, (box.y[2] + box.y[1]) / 2, (box.y[3] + box.y[0]) / 2};
    ops.prepare(px, py);
    const int left = ops.nearest(0, -1, -1, -1);
    const int right = ops.nearest(1, left, -1, -1);
    const int front = ops.nearest(2, left, right, -1);
    const int back = ops.nearest(3, left, right, front);
    D.found[0] = left; D.found[1] = right; D.found[2] = front; D.found[3] = back;
    double dist[4];
    ops.ring_box(D.found, box, dist);                           /* ring_ring_distance(rings[k], box) where found */
    const double gap = hm_hypot(sx - dx, sy - dy);
    const bool far = gap > ML_MAX_DRIVE;
    D.far = far ? 1 : 0;
    const bool lr = left >= 0 && right >= 0, fb = front >= 0 && back >= 0;
    /* not _has_enough_space(dest, rings, width / length = ...) */
    const bool narrow = lr && dist[0] + dist[1] + ML_WIDTH < ML_MIN_LOT_WID_NORMAL;
    const bool shortn = fb && dist[2] + dist[3] + ML_LENGTH < ML_MIN_LOT_LEN_NORMAL;
    const bool shortx = fb && dist[2] + dist[3] + ML_LENGTH < ML_EXTREM_LOT_LEN;
    if (gap > 30.0) {                                           /* _check_extrem */
        if (shortn) { D.branch = ML_B_EXTREM_FAR_LEN; return ML_EXTREM; }
        if (narrow) { D.branch = ML_B_EXTREM_FAR_WID; return ML_EXTREM; }
    }
    if (shortx) { D.branch = ML_B_EXTREM_LEN; return ML_EXTREM; }
    const bool bay = lr && front < 0;
    if (bay || fb) {
        if (far || (bay ? narrow : shortn)) { D.branch = bay ? ML_B_BAY_EARLY : ML_B_PAR_EARLY; return ML_COMPLEX; }
        double* w = ops.work();
        if (bay) {
            const double a = c * 0.2, b = s * 0.2, a2 = c * ML_BAY_REACH, b2 = s * ML_BAY_REACH;
            if (ops.leader()) {
                w[0] = box.x[2] + a; w[1] = box.y[2] + b; w[2] = box.x[1] + a; w[3] = box.y[1] + b;
                w[4] = box.x[2] + a2; w[5] = box.y[2] + b2; w[6] = box.x[1] + a2; w[7] = box.y[1] + b2;
                w[8] = sx; w[9] = sy;
                ml_min_area_rect(w, 5);
            }
        } else {
            double out = dh + HM_PIO2, co, so;
            hm_sincos(out, &so, &co);
            const bool flip = co * (sx - dx) + so * (sy - dy) < 0;
            if (flip) { out = out + HM_PI; hm_sincos(out, &so, &co); }
            const double kfx = flip ? box.x[1] : box.x[2], kfy = flip ? box.y[1] : box.y[2];
            const double kbx = flip ? box.x[0] : box.x[3], kby = flip ? box.y[0] : box.y[3];
            double cs, ss;
            hm_sincos(sh, &ss, &cs);
            const MlRing sb = ml_box(sx, sy, cs, ss);
            const double a = co * 0.2, b = so * 0.2, a2 = co * ML_PAR_REACH, b2 = so * ML_PAR_REACH;
            if (ops.leader()) {
                w[0] = kfx + a; w[1] = kfy + b; w[2] = kbx + a; w[3] = kby + b;
                w[4] = kfx + a2; w[5] = kfy + b2; w[6] = kbx + a2; w[7] = kby + b2;
                w[8] = sb.x[0]; w[9] = sb.y[0]; w[10] = sb.x[1]; w[11] = sb.y[1]; w[12] = sb.x[2]; w[13] = sb.y[2]; w[14] = sb.x[3]; w[15] = sb.y[3];
                w[16] = sx; w[17] = sy;
                ml_min_area_rect(w, 9);
            }
        }
        ops.sync();
        MlRing free_rect = ml_load_ring(w + ML_W_RECT);
        free_rect.nv = 4;
        const int cnt = bay ? ops.meets(free_rect, left, right, count_all) : ops.meets(free_rect, back, front, count_all);
        D.count = cnt;
        if (bay) D.branch = cnt == 0 ? ML_B_BAY_FREE : ML_B_BAY_BLOCKED;
        else D.branch = cnt == 0 ? ML_B_PAR_FREE : ML_B_PAR_BLOCKED;
        return cnt == 0 ? ML_NORMAL : ML_COMPLEX;
    }
    if (!lr && !fb) { D.branch = ML_B_OPEN; return ML_NORMAL; }
    D.branch = ML_B_OTHER;
    return ML_COMPLEX;
}

/* the serial Ops: one thread walks the tile (verts of one scene, [n][4][2]) in index order */
struct MlHostOps {
    const double* tile;
    int n;
    double px[4], py[4];
    double w[ML_WORK_WORDS];
    ML_MFN void prepare(const double* x, const double* y) { for (int k = 0; k < 4; k++) { px[k] = x[k]; py[k] = y[k]; } }
    ML_MFN int nearest(int k, int s0, int s1, int s2) const {
        int best = -1;
        double bd = ML_LENGTH / 2;
        for (int o = 0; o < n; o++) {
            if (o == s0 || o == s1 || o == s2) continue;
            const double d = ml_point_ring(px[k], py[k], ml_load_ring(tile + 8 * (size_t)o));
            if (d < bd) { bd = d; best = o; }
        }
        return best;
    }
    ML_MFN void ring_box(const int32_t* found, const MlRing& box, double* dist) const {
        for (int k = 0; k < 4; k++) dist[k] = found[k] >= 0 ? ml_ring_ring(ml_load_ring(tile + 8 * (size_t)found[k]), box) : INFINITY;
    }
    ML_MFN double* work() { return w; }
    ML_MFN bool leader() const { return true; }
    ML_MFN void sync() const {}
    ML_MFN int meets(const MlRing& rect, int sa, int sb, bool all) const {
        int cnt = 0;
        for (int o = 0; o < n; o++) {
            if (o == sa || o == sb) continue;
            if (ml_poly_meets_ring(rect, ml_load_ring(tile + 8 * (size_t)o))) { cnt++; if (!all) break; }
        }
        return cnt;
    }
};

/* one scene on the host: level, and the detail record when detail != NULL */
HM_FN int ml_scene_host(const double* start, const double* dest, const double* tile, int n, int32_t* detail) {
    MlHostOps ops;
    ops.tile = tile; ops.n = n;
    MlDetail D;
    const int lv = ml_classify(ops, start[0], start[1], start[2], dest[0], dest[1], dest[2], n, detail != 0, D);
    if (detail) {
        detail[0] = D.found[0]; detail[1] = D.found[1]; detail[2] = D.found[2]; detail[3] = D.found[3];
        detail[4] = D.branch; detail[5] = D.far; detail[6] = D.count; detail[7] = 0;
    }
    return lv;
}
