"""Lots built against the FILTERS in front of the lidar's reference arithmetic (hope_amd/csrc/hope_step_kernel.h "---- lidar" and its
two-scenes-per-wave copy hope_amd/csrc/hope_obs_pair.h): the near list, the squared-quantity ring keep / drop, the float32 beam
span, the "wild" escape to all 120 beams, the back-face cull and its five gates, beam_may_hit, the pair queue and its drains,
the branch for an edge paired with more than 64 beams, the in-place compaction of the kept rings.  Drawn lots decide nearly all
of these on the easy side; these decide them on both sides, or on the threshold itself.  The role tests/touching_scenes.py
plays for the collision test.

Every lot is built in the EGO frame (sensor at the origin, heading along +x) and mapped to the world by a start pose: EXACT
poses (heading 0, dyadic x / y: the ego transform is exact for dyadic ego coordinates, alignments survive it) and ROUNDED poses
(headings +-pi/2, pi, random: hm_cos is not exact, so near-ties are moved by tests/exact_geometry.py's ulp_nudge and land on both
sides).  `census` restates the kernels' branch predicates in numpy on the ego coordinates AS THE ORACLE'S TRANSFORM ROUNDS THEM;
tests/test_lidar_adversarial.py asserts from it that every family populates the branch it is aimed at, before
tests/test_gpu_lidar_adversarial.py compares anything on the device.

Families (`fam`): 1 beam-aligned, 2 range ties, 3 behind / through the sensor, 4 wild edges, 5 shapes, 6 counts, 7 generic."""
import functools
import math

import numpy as np

import exact_geometry as E
from oracle import oracle as O

NBEAM, WAVE = 120, 64
PITCH = 2 * math.pi / NBEAM
LIDAR_RANGE = 10.0
LQ_ONE, LQ_PAIR = 384, 512                      # pair-queue entries of k_env_step / k_obs_pair
SMALL_TILE = 32
OFF_BEAM = (0.0, 1e-5, 2e-4, 3e-4)              # vertex off a beam direction, rad (near_beam: <= 2.1e-4)
OFF_COLLINEAR = (0.0, 1e-10, 1e-9, 1e-8)        # edge off a beam's line, m (beam_may_hit: 1e-9)
OFF_THIN = (0.0, 5e-5, 2e-4)                    # coordinate extent of a front edge, m (thin: < 1e-4)
OFF_RING = (1, 5, 20)                           # ring distance 10 (1 +- k 1e-10) (ring keep / drop margin: 1e-9 on squares)
OFF_NEAR = (1e-7, 1e-5)                         # obstacle box at 10 m +- (near list's slack: 1e-6)
OFF_BEHIND = (5e-9, 9e-9, 2e-8, 5e-7, 2e-6)     # intersection behind the sensor (reference: 1e-8, beam_may_hit: 1e-6); 9e-9: a hit the
                                                # reference still counts, as far behind as one can be -- a `back` nearer zero than that loses it
OFF_DECISIVE = (5e-7, 2e-6)                     # |sin| of the angle an edge subtends (decisive: > 1e-6)
EXACT_POSES = ((0.0, 0.0, 0.0), (8.5, -3.25, 0.0), (-40.125, 17.5, 0.0), (-2.0, 0.0, 0.0))
ZERO_Y_POSES = ((-2.0, 0.0, 0.0), (-1.5, 0.0, 0.0), (0.0, 0.0, 0.0), (8.5, 0.0, 0.0))      # y = 0: a world y = -0.0 stays one


def _cs(h):
    return float(O.math_fn(1, [h])[0]), float(O.math_fn(0, [h])[0])


def rounded_pose(rng, k):
    h = (math.pi / 2, -math.pi / 2, math.pi, rng.uniform(-math.pi, math.pi))[k % 4]
    return (float(rng.uniform(-40, 40)), float(rng.uniform(-40, 40)), float(h))


def to_world(pose, ego):
    """ego-frame points [..., 2] -> world.  Heading 0: a plain sum (exact for dyadic operands)"""
    ego = np.asarray(ego, float)
    x, y, h = pose
    if h == 0.0:
        return ego + np.array([x, y])
    c, s = math.cos(h), math.sin(h)
    return np.stack([c * ego[..., 0] - s * ego[..., 1] + x, s * ego[..., 0] + c * ego[..., 1] + y], axis=-1)


def to_ego(pose, verts):
    """world -> ego exactly as orc_lidar_observation / the kernels round it (hm_cos / hm_sin of the heading, no contraction)"""
    v = np.asarray(verts, float)
    x, y, h = pose
    a, b = _cs(h)
    x_off = -x * a - y * b
    y_off = x * b - y * a
    return np.stack([a * v[..., 0] + b * v[..., 1] + x_off, (-b) * v[..., 0] + a * v[..., 1] + y_off], axis=-1)


# ---- shapes in the ego frame --------------------------------------------------------------------------------------------------
def rot(q, ang):
    q = np.asarray(q, float)
    c, s = math.cos(ang), math.sin(ang)
    return np.stack([c * q[..., 0] - s * q[..., 1], s * q[..., 0] + c * q[..., 1]], axis=-1)


def quarter(q, k):
    """rotation by k x 90 degrees as an exact swap of coordinates"""
    q = np.asarray(q, float)
    for _ in range(k % 4):
        q = np.stack([-q[..., 1], q[..., 0]], axis=-1)
    return q


def box(x0, y0, x1, y1):
    return np.array([[x0, y0], [x1, y0], [x1, y1], [x0, y1]], float)


def corner_square(v, ang, side=1.0, jitter=0.0):
    """CCW square with its corner v towards the sensor, seen from direction `ang`"""
    e1 = np.array([math.cos(ang - math.pi / 4 + jitter), math.sin(ang - math.pi / 4 + jitter)])
    e2 = np.array([-e1[1], e1[0]])
    v = np.asarray(v, float)
    return np.array([v, v + side * e1, v + side * (e1 + e2), v + side * e2])


def ordinary(rng, k, lo=3.5, hi=9.0):
    """k convex CCW quads `lo`..`hi` metres from the sensor, no vertex placed on purpose"""
    out = []
    for _ in range(k):
        a, r, th = rng.uniform(0, 2 * math.pi), rng.uniform(lo, hi), rng.uniform(0, math.pi)
        w, h = rng.uniform(0.4, 1.2), rng.uniform(0.3, 0.8)
        q = rot(box(-w, -h, w, h) * rng.uniform(0.9, 1.1, (4, 2)), th) + r * np.array([math.cos(a), math.sin(a)])
        out.append(q)
    return out


class Lot:
    def __init__(self, fam, tag, pose, ego_quads, exact, first_world=None):
        """first_world: a quad given in WORLD coordinates, bit for bit, that becomes the lot's first obstacle"""
        self.fam, self.tag, self.pose, self.exact = fam, tag, tuple(float(v) for v in pose), exact
        self.quads = np.array([to_world(self.pose, q) for q in ego_quads], float).reshape(-1, 4, 2)
        if first_world is not None:
            self.quads = np.concatenate([np.asarray(first_world, float)[None], self.quads])
        assert np.abs(self.quads).max(initial=0) <= 128.0
        x, y, h = self.pose
        r = 20.0
        self.dest = np.array([x - r * math.cos(h + 2.5), y - r * math.sin(h + 2.5), h + 0.7])
        self.bbox = np.array([math.floor(x - 45), math.ceil(x + 45), math.floor(y - 45), math.ceil(y + 45)])

    def ego(self):
        return to_ego(self.pose, self.quads)


def _nudged(rng, q):
    return np.array(E.ulp_nudge(rng, [tuple(p) for p in q]))


def _place(rng, fam, tag, ego_quads, k, lots, exact_only=False, fill=2):
    """one lot on an exact pose and (unless exact_only) one on a rounded pose with one vertex of the first quad moved by 1-2 ulp"""
    extra = ordinary(rng, fill, 4.5, 9.0) if fill else []
    lots.append(Lot(fam, tag, EXACT_POSES[k % len(EXACT_POSES)], list(ego_quads) + extra, True))
    if not exact_only:
        lot = Lot(fam, tag, rounded_pose(rng, k), list(ego_quads) + extra, False)
        lot.quads[0] = _nudged(rng, lot.quads[0])
        lots.append(lot)


# ---- family 1: beam-aligned -----------------------------------------------------------------------------------------------------
def family_beam_aligned(rng):
    lots = []
    k = 0
    for rep in range(4):
        for beam in (0, 30, 60, 90, 7, 41, 77, 101):                    # a vertex on / next to a beam direction
            for off in OFF_BEAM:
                for sgn in ((1,) if off == 0 else (1, -1)):
                    r = (4.0, 5.5, 3.25, 6.75)[rep]
                    if beam % 30 == 0 and off == 0:
                        v = quarter(np.array([r, 0.0]), beam // 30)
                    else:
                        ang = beam * PITCH + sgn * off
                        v = r * np.array([math.cos(ang), math.sin(ang)])
                    q = corner_square(v, beam * PITCH, 1.0, jitter=0.2 * (rep - 1.5))
                    _place(rng, 1, ('vertex', off, sgn), [q], k, lots, exact_only=(beam % 30 == 0 and off == 0 and rep >= 2))
                    k += 1
    for rep in range(4):
        for axis in range(4):                                           # an edge on / next to an axis beam's line
            for off in OFF_COLLINEAR:
                for sgn in ((1,) if off == 0 else (1, -1)):
                    c = sgn * off
                    x0, x1 = (3.0, 2.5, 4.0, 1.5)[rep], (5.0, 6.5, 4.75, 8.0)[rep]
                    quads = [np.array([[x0, c], [x1, c], [x1, c + 1.0], [x0, c + 1.0]]),            # parallel, body above
                             np.array([[x0, -1.0 - c], [x1, -1.0 - c], [x1, c], [x0, c]]),          # parallel, body below
                             np.array([[x0, c], [x1, -c], [x1, 1.0], [x0, 1.0]])]                   # crossing the line at a tiny angle
                    q = quarter(quads[(rep + axis) % 3], axis)
                    _place(rng, 1, ('collinear', off, sgn), [q], k, lots, exact_only=True)
                    k += 1
    for rep in range(6):
        for ext in OFF_THIN:                                            # a front edge with a coordinate extent of ext
            for sgn in (1, -1):
                x0 = 3.0 + 0.5 * rep
                q = np.array([[x0, -0.9], [x0 + 1.0, -0.9], [x0 + 1.0, 1.13], [x0 + sgn * ext, 1.13]])
                _place(rng, 1, ('thin', ext, sgn), [quarter(q, rep)], k, lots, exact_only=True)
                k += 1
    for rep in range(6):
        for s0 in (0.0, -0.0):                                          # an end point with y = +-0 on the -x and on the +x axis
            for sx in (-1.0, 1.0):
                d = 3.0 + 0.5 * rep
                up = 1.0 if rep % 2 == 0 else -1.0
                qa = np.array([[sx * d, s0], [sx * d, 2.0 * up], [sx * (d + 1), 2.0 * up], [sx * (d + 1), s0]])
                qb = np.array([[sx * d, s0], [sx * (d - 1), 1.5 * up], [sx * (d + 0.5), 2.5 * up], [sx * (d + 1.5), 1.0 * up]])
                q = qa if rep < 3 else qb
                # The sign of a zero survives no addition with +0.0, so the WORLD quad is written directly (pose y = 0: world y is the
                # ego y, bit for bit) and the pose chosen for what the ego transform y' = (-b) x + a y + (x0 b - y0 a) does at heading
                # 0 (a = 1, b = +0.0; hm_sin(-0.0) is +0.0 too): a world x > 0 (the first two poses: 0 > x0 > -3) gives (-0.0) + (-0.0), and a pose x0 < 0 gives
                # y_off = (-0.0) - 0.0: y' = -0.0 on the +x axis.  A world x < 0 gives (+0.0) + (-0.0) = +0.0 whatever the pose, and at
                # any other heading b is not zero and an exact cancellation rounds to +0.0: NO pose delivers -0.0 on the -x axis.
                pose = ZERO_Y_POSES[rep % 2 if (sx > 0 and math.copysign(1.0, s0) < 0) else rep % 4]
                world = q.copy()
                world[:, 0] += pose[0]
                lots.append(Lot(1, ('zero_y', 'neg_x' if sx < 0 else 'pos_x', 'minus' if math.copysign(1.0, s0) < 0 else 'plus'), pose,
                                ordinary(rng, 2, 4.5, 9.0), True, first_world=world))
                k += 1
    return lots


# ---- family 2: range ties -----------------------------------------------------------------------------------------------------------
TIE_RINGS = {'edge_x10': np.array([[10.0, -1.25], [11.0, -1.25], [11.0, 1.125], [10.0, 1.125]]),
             'vertex_6_8': np.array([[6.0, 8.0], [7.5, 8.0], [7.5, 9.5], [6.0, 9.5]]),
             'foot_inside': np.array([[10.0, 5.0], [13.0, 9.0], [5.0, 15.0], [2.0, 11.0]])}


COMPUTED_TIE_BEAMS = (10, 25, 47, 71, 95, 113, 3, 58, 82, 104)


def reference_range(i, ring):
    """_fast_calc_lidar_obs (lidar_simulator.py:98-133) for beam i of the PACKAGE's beam table (hope_amd.tables: the one the device
    and, in the GPU tests, the oracle hold) on one ego ring [4][2], in Python floats: the unclipped range"""
    from hope_amd import tables as TB
    a, b = (float(v) for v in TB.all_tables()['beam_ab'][i])
    best = math.inf
    for j in range(4):
        (x1, y1), (x2, y2) = (float(v) for v in ring[j]), (float(v) for v in ring[(j + 1) % 4])
        d, e, f = y2 - y1, x1 - x2, y1 * x2 - x1 * y2
        det = a * e - b * d
        if det == 0:
            continue
        rx, ry = (b * f - 0.0 * e) / det, (0.0 * d - a * f) / det
        sx, sy = (1.0 if (i < NBEAM // 4 or i >= NBEAM // 4 * 3) else -1.0), (1.0 if i < NBEAM // 2 else -1.0)
        if sx * rx < -1e-8 or sy * ry < -1e-8 or rx > max(x1, x2) or rx < min(x1, x2) or ry > max(y1, y2) or ry < min(y1, y2):
            continue
        best = min(best, math.sqrt(rx * rx + ry * ry))
    return best


def computed_tie_ring(rng, beam):
    """A ring whose distance AS THE REFERENCE COMPUTES IT is exactly 10.0 (so it is dropped: :69 keeps `< lidar_range`) while the hit of
    `beam` on it, as _fast_calc_lidar_obs would compute it, is below 10 by an ulp or two: an edge at right angles to the beam, 10 m
    out, its end points moved about by a few ulp until both roundings fall that way.  Keeping the ring (`<=` for `<`) changes the scan."""
    ang = beam * PITCH
    u, n = np.array([math.cos(ang), math.sin(ang)]), np.array([-math.sin(ang), math.cos(ang)])
    for _ in range(4000):
        la, lb = rng.uniform(0.5, 2.0, 2)
        foot = 10.0 * u
        a, b = foot - la * n, foot + lb * n
        ring = np.array([a, b, b + 1.5 * u, a + 1.5 * u])
        for _ in range(int(rng.integers(0, 4))):
            ring[:2] = _nudged(rng, ring[:2])
        if ring_distance(ring[None])[0] == LIDAR_RANGE and reference_range(beam, ring) < LIDAR_RANGE:
            return ring
    raise AssertionError('no computed tie found')


def family_range_ties(rng):
    lots = []
    k = 0
    for beam in COMPUTED_TIE_BEAMS:                                      # (pose (0, 0, 0): the ego frame is the world, bit for bit)
        lots.append(Lot(2, ('tie', 'computed_10', beam), EXACT_POSES[0], [computed_tie_ring(rng, beam)], True))
    for name, ring in TIE_RINGS.items():
        for qk in range(4):
            _place(rng, 2, ('ring', name, 0, 0), [quarter(ring, qk)], k, lots, fill=1)                       # distance exactly 10
            k += 1
            for m in OFF_RING:
                for sgn in (1, -1):
                    _place(rng, 2, ('ring', name, m, sgn), [quarter(ring, qk) * (1.0 + sgn * m * 1e-10)], k, lots, fill=1)
                    k += 1
            for s in (0.9, 1.1):
                _place(rng, 2, ('ring', name, 'well', 1 if s > 1 else -1), [quarter(ring, qk) * s], k, lots, exact_only=True, fill=1)
                k += 1
    for rep in range(2):
        for qk in range(4):                                              # obstacle boxes at 10 m +- the near list's slack
            for off in OFF_NEAR:
                for sgn in (1, -1):
                    d = 10.0 + sgn * off
                    q = box(d, -1.0 - rep, d + 1.0 + rep, 0.75 + rep)
                    _place(rng, 2, ('near', off, sgn), [quarter(q, qk)], k, lots, exact_only=True, fill=1)
                    k += 1
            _place(rng, 2, ('near', 'diagonal', 0), [quarter(box(8.0 + rep * 0.5, 8.0, 9.5 + rep, 9.0), qk)], k, lots, exact_only=True, fill=1)
            k += 1
    for rep in range(3):
        for qk in range(4):                                              # a kept ring hit at exactly 10 m (the clip) and beyond it
            h = 1.0 + 0.5 * rep                                           # (the vertex at (9, -4 + ..) keeps the ring: 9.85 m or less)
            q = np.array([[10.0, h], [10.0, -h], [9.0, -4.0 + 0.25 * rep], [12.0, -3.0 - rep]])
            _place(rng, 2, ('hit', 'at_10', 0), [quarter(q, qk)], k, lots, exact_only=True, fill=0)
            k += 1
            q = np.array([[10.0 + 0.5 * (rep + 1), h], [10.0 + 0.5 * (rep + 1), -h], [9.0, -4.0 + 0.25 * rep], [13.0, -3.0 - rep]])
            _place(rng, 2, ('hit', 'beyond', 0), [quarter(q, qk)], k, lots, fill=0)
            k += 1
    return lots


# ---- family 3: behind and through the sensor ----------------------------------------------------------------------------------------
def family_behind_through(rng):
    lots = []
    k = 0
    for rep in range(3):
        for qk in range(4):                                              # the edge's line meets an axis beam `off` behind the sensor
            for off in OFF_BEHIND:
                up = 1.0 + 0.5 * rep
                dl = 1e-9                                                # (a slant of 2e-9 m: an axis-parallel edge loses the hit to the
                # reference's tolerance-free coordinate-box test whenever the quotient is an ulp off)
                quads = [np.array([[-off - dl, -up], [-off + dl, up], [-off - 2.0, up], [-off - 2.0, -up]]),          # the whole edge behind
                         np.array([[-off + 0.5, up], [-off - 0.5, -up], [-3.0, -up], [-3.0, up]])]          # crossing, one end in front
                for form, q in enumerate(quads):
                    _place(rng, 3, ('behind', off, form), [quarter(q, qk)], k, lots, exact_only=True, fill=1)
                    k += 1
    for rep in range(3):
        for qk in range(4):                                              # an edge through the sensor point itself: f == 0, range 0
            s = 1.0 + rep
            q = np.array([[-1.0 * s, -0.5 * s], [2.0 * s, 1.0 * s], [2.0 * s, 2.0 * s], [-1.0 * s, 1.0 * s]])
            _place(rng, 3, ('through', 0, 0), [quarter(q, qk)], k, lots, exact_only=True, fill=1)
            k += 1
    for rep in range(4):                                                 # the sensor strictly inside a ring
        for j, q in enumerate([box(-2.0, -1.5, 3.0, 1.5), box(-7.0, -6.5, 8.0, 7.5), box(-0.5, -0.25, 0.25, 0.5),
                               np.array([[-3.0, -3.0], [4.0, -2.0], [0.5, 0.5], [-2.0, 5.0]])]):
            _place(rng, 3, ('inside', j, 0), [rot(q, 0.3 * rep)], k, lots, fill=1)
            k += 1
    for rep in range(4):
        for qk in range(4):                                              # the sensor on an edge's line, and just off it
            p, q2 = np.array([2.0, 1.0]) * (1 + 0.5 * rep), np.array([4.0, 2.0]) * (1 + 0.5 * rep)
            n = np.array([-1.0, 2.0]) / math.sqrt(5.0)
            body = [q2 + np.array([1.0, -2.0]), p + np.array([1.0, -2.0])]
            _place(rng, 3, ('online', 0.0, 1), [quarter(np.array([p, q2] + body), qk)], k, lots, exact_only=True, fill=1)
            k += 1
            for s in OFF_DECISIVE:
                for sgn in (1, -1):
                    t = sgn * s * np.linalg.norm(q2)                     # |sin| of the subtended angle = offset of q2 from the line / |q2|
                    _place(rng, 3, ('online', s, sgn), [quarter(np.array([p, q2 + t * n] + body), qk)], k, lots, exact_only=True, fill=1)
                    k += 1
    return lots


# ---- family 4: wild edges -------------------------------------------------------------------------------------------------------------
def wild_long(ang, c=0.00125, half=3.0):
    """a quad one edge of which subtends > 3.13 rad at the sensor (pi - 2 c / half), its end points `half` metres away"""
    return rot(np.array([[-half, c], [half, c], [half, 1.0], [-half, 1.0]]), ang)


def wild_vertex(ang):
    """a quad with one vertex 0.05 m from the sensor: both edges at that vertex are wild"""
    return rot(np.array([[0.05, 0.0], [2.0, -0.75], [3.0, 0.25], [1.75, 1.0]]), ang)


WILD_MIX = {1: [(1, 0)], 3: [(1, 1)], 4: [(2, 1)], 8: [(2, 3), (4, 2)]}          # wild edges -> (long quads, vertex quads)


def family_wild(rng):
    """in the order (wild, wild, wild, plain, plain, wild) x: consecutive lots share a wave of the pair kernel"""
    lots = []
    k = 0
    for rep in range(10):
        for w, mixes in WILD_MIX.items():
            for n_long, n_vert in mixes:
                for exact in (True, False):
                    a0 = rng.uniform(0, 2 * math.pi)
                    quads = [wild_long(a0 + 2 * math.pi * i / max(n_long, 1) + 0.11, c=0.001 + 0.0001 * i) for i in range(n_long)]
                    quads += [wild_vertex(a0 + 0.7 + 2 * math.pi * i / max(n_vert, 1)) for i in range(n_vert)]
                    quads += ordinary(rng, int(rng.integers(2, 8)))
                    order = rng.permutation(len(quads))
                    lots.append(Lot(4, ('wild', w, n_long, n_vert), EXACT_POSES[k % 4] if exact else rounded_pose(rng, k), [quads[i] for i in order], exact))
                    k += 1
    out, plain = [], family_generic(np.random.default_rng(404), len(lots))
    for i in range(0, len(lots) - 3, 4):                                 # W W | W P | P W  (then the next four)
        out += [lots[i], lots[i + 1], lots[i + 2], plain[i], plain[i + 1], lots[i + 3]]
    for lot in out:
        lot.fam = 4
    return out


# ---- family 5: shapes -----------------------------------------------------------------------------------------------------------------
def _para(alpha, a=2.0, b=1.5):
    al = math.radians(alpha)
    return np.array([[0, 0], [a, 0], [a + b * math.cos(al), b * math.sin(al)], [b * math.cos(al), b * math.sin(al)]])


SHAPES = {'quad': np.array([[0, 0], [2.0, 0.25], [2.25, 1.5], [0.25, 1.25]]),
          'dart': np.array([[0, 0], [1.0, 0.5], [2.0, 0], [1.0, 2.0]]),
          'bowtie': np.array([[0, 0], [2.0, 0], [0, 1.5], [2.0, 1.5]]),
          'triangle': np.array([[0, 0], [2.0, 0], [1.0, 1.5], [1.0, 1.5]]),
          'collinear': np.array([[0, 0], [1.0, 0.5], [2.0, 1.0], [3.0, 1.5]]),
          'zero_edge': np.array([[0, 0], [0, 0], [2.0, 0], [1.0, 1.0]]),
          'point': np.array([[0.5, 0.5]] * 4),
          'angle_24': _para(24.0), 'angle_26': _para(26.0),
          'edge_049': box(0, 0, 0.049, 1.0), 'edge_051': box(0, 0, 0.051, 1.0)}


def family_shapes(rng):
    lots = []
    k = 0
    for rep in range(8):
        for name, q in SHAPES.items():
            for cw in (False, True):
                quads = []
                for _ in range(3):                                       # three copies around the sensor, all seen from outside
                    a, r, th = rng.uniform(0, 2 * math.pi), rng.uniform(3.0, 7.0), rng.uniform(0, 2 * math.pi)
                    c = q.mean(axis=0)
                    p = rot(q - c, th) + r * np.array([math.cos(a), math.sin(a)])
                    quads.append(p[::-1].copy() if cw else p)
                lots.append(Lot(5, ('shape', name, 'cw' if cw else 'ccw'), EXACT_POSES[k % 4] if rep % 2 else rounded_pose(rng, k), quads, rep % 2 == 1))
                k += 1
    return lots


# ---- family 6: counts -------------------------------------------------------------------------------------------------------------------
KEPT_SMALL, KEPT_LARGE = (0, 1, 15, 16, 17, 31, 32), (33, 63, 64, 65, 128)


def _small_quads(rng, k, lo, hi):
    out = []
    for i in range(k):
        a, r, th = rng.uniform(0, 2 * math.pi), rng.uniform(lo, hi), rng.uniform(0, math.pi)
        out.append(rot(box(-0.3, -0.2, 0.3, 0.2) * rng.uniform(0.8, 1.2, (4, 2)), th) + r * np.array([math.cos(a), math.sin(a)]))
    return out


def count_lot(rng, kept, cap, k):
    """`kept` rings within range, the rest of at most `cap` obstacles out of range (some still inside the near list's box), shuffled"""
    quads = _small_quads(rng, kept, 3.0, 8.5)
    n_out = min(cap - kept, int(rng.integers(3, 9)))
    out = _small_quads(rng, n_out // 2, 13.0, 30.0)
    for _ in range(n_out - n_out // 2):                                  # in the corner of the near list's box: near, not kept
        sx, sy = rng.choice([-1.0, 1.0], 2)
        out.append(box(-0.3, -0.2, 0.3, 0.2) + np.array([sx * rng.uniform(8.0, 9.0), sy * rng.uniform(8.0, 9.0)]))
    quads += out
    order = rng.permutation(len(quads))
    return Lot(6, ('kept', kept), EXACT_POSES[k % 4] if k % 2 else rounded_pose(rng, k), [quads[i] for i in order], k % 2 == 1)


def wall_lot(rng, k, rings=6):
    """`rings` nested squares of four long walls each, 2-7 m from the sensor, turned by a random angle: every wall's front edge
    spans ~27 beams or more -- no wild edge, yet more ordinary pairs than one queue holds"""
    quads = []
    a0 = rng.uniform(0.1, 0.6)
    for j in range(rings):
        d = 2.0 + 5.0 * j / max(rings - 1, 1)
        half = d * math.tan(math.radians(40.0))
        for s in range(4):
            quads.append(rot(box(d, -half, d + 0.25, half), a0 + 0.05 * j + s * math.pi / 2))
    order = rng.permutation(len(quads))
    return Lot(6, ('walls', rings), EXACT_POSES[k % 4] if k % 2 else rounded_pose(rng, k), [quads[i] for i in order], k % 2 == 1)


def family_counts(rng):
    lots = []
    k = 0
    for rep in range(8):
        for kept in KEPT_SMALL:
            lots.append(count_lot(rng, kept, SMALL_TILE, k))
            k += 1
        for kept in KEPT_LARGE:
            lots.append(count_lot(rng, kept, 128, k))
            k += 1
        lots.append(wall_lot(rng, k, 6))
        lots.append(wall_lot(rng, k + 1, 8))
        k += 2
    return lots


def lot_255(rng, kept):
    """255 obstacles, `kept` of them within range (for a handle with max_obstacles = 255)"""
    quads = _small_quads(rng, kept, 4.5, 9.0) + _small_quads(rng, 255 - kept, 12.0, 30.0)        # (clear of the hull: 3.76 m to the front)
    order = rng.permutation(255)
    return Lot(6, ('kept255', kept), rounded_pose(rng, kept), [quads[i] for i in order], False)


# ---- family 7: generic ----------------------------------------------------------------------------------------------------------------------
def family_generic(rng, n=48):
    """random convex quads at random non-aligned poses, the sensor enclosed by four thick walls of a room ~6 m across its half
    width (corners < 9 m away): every beam has a hit below the range -- the clean control, and the family of the exact ray cast"""
    lots = []
    for k in range(n):
        a0 = rng.uniform(0, 2 * math.pi)
        quads = []
        for s in range(4):
            d = rng.uniform(5.0, 6.2)
            w = box(d, -7.5, d + 1.0, 7.5) + rng.uniform(-0.2, 0.2, (4, 2))
            quads.append(rot(w, a0 + s * math.pi / 2))
        quads += ordinary(rng, int(rng.integers(2, 7)), 2.5, 5.0)
        order = rng.permutation(len(quads))
        pose = (float(rng.uniform(-40, 40)), float(rng.uniform(-40, 40)), float(rng.uniform(-math.pi, math.pi)))
        lots.append(Lot(7, ('generic',), pose, [quads[i] for i in order], False))
    return lots


FAMILIES = {1: family_beam_aligned, 2: family_range_ties, 3: family_behind_through, 4: family_wild, 5: family_shapes,
            6: family_counts, 7: family_generic}


@functools.lru_cache(maxsize=None)
def all_lots():
    """every family's lots, in family order (family 4 keeps its wave layout: it starts at an even index of the small class)"""
    lots = []
    for fam, fn in FAMILIES.items():
        lots += fn(np.random.default_rng(1000 + fam))
    return lots


def small_and_large(lots=None):
    """-> (small, large): the lots of the small-tile class (<= 32 obstacles) in order, family 4 first so that its pairs of
    consecutive lots are waves of the pair kernel, an odd number in all; and the lots of the large-tile class"""
    lots = all_lots() if lots is None else lots
    small = [l for l in lots if len(l.quads) <= SMALL_TILE]
    small = [l for l in small if l.fam == 4] + [l for l in small if l.fam != 4]
    if len(small) % 2 == 0:
        small = small[:-1]
    return small, [l for l in lots if len(l.quads) > SMALL_TILE]


def arrays(lots, max_obst=128):
    """the arrays hope_amd.ParkingBatch.set_scene_arrays and oracle.BatchOracle.set_scenes take"""
    n = len(lots)
    start, dest, bbox = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((n, 4))
    verts, nob = np.zeros((n, max_obst, 4, 2)), np.zeros(n, np.int32)
    for i, l in enumerate(lots):
        start[i], dest[i], bbox[i], nob[i] = l.pose, l.dest, l.bbox, len(l.quads)
        verts[i, :nob[i]] = l.quads
    return dict(start=start, dest=dest, bbox=bbox, verts=verts, nob=nob, nvert=np.full((n, max_obst), 4, np.int32),
                fam=np.array([l.fam for l in lots]))


# ---- the census: the kernels' branch predicates in numpy -----------------------------------------------------------------------------------
def shape_flags(quads):
    """obstacle_f32's shape flags (hope_amd/csrc/hope_dev.h) on world quads [m][4][2] -> convex [m], ccw [m]"""
    q = np.asarray(quads, float).reshape(-1, 4, 2)
    a = np.roll(q, -1, axis=1) - q
    b = np.roll(a, -1, axis=1)
    cr = a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]
    la, lb = (a ** 2).sum(-1), (b ** 2).sum(-1)
    ok = ((la >= 0.0025) & (lb >= 0.0025) & (cr * cr >= 0.1786 * la * lb)).all(axis=1)
    pos = cr > 0
    ok &= (pos == pos[:, :1]).all(axis=1)
    return ok, pos[:, 0]


def ring_decision(ego):
    """the squared-quantity ring test on ego rings [m][4][2] -> keep [m], drop [m] (neither: the exact fallback decides)"""
    a = np.asarray(ego, float).reshape(-1, 4, 2)
    b = np.roll(a, -1, axis=1)
    ax, ay, bx, by = a[..., 0], a[..., 1], b[..., 0], b[..., 1]
    ddx, ddy = bx - ax, by - ay
    len2 = ddx * ddx + ddy * ddy
    dot = (0.0 - ax) * ddx + (0.0 - ay) * ddy
    qa, qb = ax * ax + ay * ay, bx * bx + by * by
    num = ay * ddx - ax * ddy
    R2, ETA = LIDAR_RANGE * LIDAR_RANGE, 1e-9
    lo, hi = R2 * (1.0 - ETA), R2 * (1.0 + ETA)
    n2 = num * num
    line_far, line_near = n2 > hi * len2, n2 < lo * len2
    foot_in = (dot > ETA * len2) & (dot < (1.0 - ETA) * len2)
    foot_a, foot_b = dot < -ETA * len2, dot > (1.0 + ETA) * len2
    keep_c = (qa < lo) | (qb < lo) | (foot_in & line_near)
    drop_c = ~keep_c & np.where(len2 > 0.0, line_far | (foot_a & (qa > hi)) | (foot_b & (qb > hi)), qa > hi)
    return keep_c.any(axis=1), drop_c.all(axis=1)


def ring_distance(ego):
    """GEOS's point-to-segment distance of the origin from ego rings [m][4][2], as the oracle computes it -> [m]"""
    out = []
    for r in np.asarray(ego, float).reshape(-1, 4, 2):
        out.append(min(O.pt_seg_dist((0.0, 0.0), r[j], r[(j + 1) % 4]) for j in range(4)))
    return np.array(out)


def ring_distance2_exact(ring):
    return min(E.pt_seg_dist2_exact((0.0, 0.0), ring[j], ring[(j + 1) % 4]) for j in range(4))


def census(lot):
    """-> dict: what the lidar stage's filters do with this lot at its start pose"""
    ego = lot.ego()
    m = len(ego)
    c = dict(n_obst=m, n_near=0, n_kept=0, n_amb=0, pairs=0, pairs_nocull=0, wild=0, wild_vertex=0, wild_span=0, wide=0, near_beam=0,
             thin=0, undecisive=0, culled_rings=0, cull_blocked_by={}, nonconvex=0, cw=0, det0=0, first=None)
    if m == 0:
        return c
    lr = LIDAR_RANGE + 1e-6
    x, y = lot.pose[0], lot.pose[1]
    w = lot.quads
    near = ~((w[..., 0].min(1) > x + lr) | (w[..., 0].max(1) < x - lr) | (w[..., 1].min(1) > y + lr) | (w[..., 1].max(1) < y - lr))
    keep, drop = ring_decision(ego)
    amb = near & ~keep & ~drop
    kept = near & keep
    if amb.any():
        kept[amb] = ring_distance(ego[amb]) < LIDAR_RANGE
    convex, ccw = shape_flags(w)
    c.update(n_near=int(near.sum()), n_kept=int(kept.sum()), n_amb=int(amb.sum()), kept_mask=kept, amb_mask=amb)
    # the first ring is the one a family builds on purpose (families 1-3; the others shuffle)
    ab = beam_table()
    e0, e1 = ego[0], np.roll(ego[0], -1, axis=0)
    s1 = ab[:, 0, None] * e0[None, :, 0] + ab[:, 1, None] * e0[None, :, 1]
    s2 = ab[:, 0, None] * e1[None, :, 0] + ab[:, 1, None] * e1[None, :, 1]
    f1 = ab[:, 0, None] * e0[None, :, 1] - ab[:, 1, None] * e0[None, :, 0]
    f2 = ab[:, 0, None] * e1[None, :, 1] - ab[:, 1, None] * e1[None, :, 0]
    on_line = (np.abs(s1) <= 1e-9) & (np.abs(s2) <= 1e-9) & ~((f1 < -1e-6) & (f2 < -1e-6)) & ((e0 != e1).any(axis=1))[None]
    zy = e0[e0[:, 1] == 0.0]
    c['first'] = dict(near=bool(near[0]), amb=bool(amb[0]), kept=bool(kept[0]), keep_decided=bool(near[0] and keep[0]),
                      drop_decided=bool(near[0] and drop[0]), convex=bool(convex[0]), ccw=bool(ccw[0]), on_line_pairs=int(on_line.sum()),
                      zero_y_neg_x=int((zy[:, 0] < 0).sum()), zero_y_pos_x=int((zy[:, 0] > 0).sum()),
                      zero_y_minus=int(np.signbit(zy[:, 1]).sum()))
    K = ego[kept]
    if len(K) == 0:
        return c
    p1, p2 = K, np.roll(K, -1, axis=1)
    x1, y1, x2, y2 = (v.astype(np.float32) for v in (p1[..., 0], p1[..., 1], p2[..., 0], p2[..., 1]))
    with np.errstate(invalid='ignore'):
        t1 = np.where((x1 == 0) & (y1 == 0), np.float32(np.nan), np.arctan2(y1, x1)).astype(np.float32)
        t2 = np.roll(t1, -1, axis=1)
        dth = t2 - t1
        dth = np.where(dth > np.float32(3.14159265), dth - np.float32(6.28318531), dth)
        dth = np.where(dth <= np.float32(-3.14159265), dth + np.float32(6.28318531), dth)
        span = np.abs(dth)
        close = np.minimum(x1 * x1 + y1 * y1, x2 * x2 + y2 * y2) < np.float32(0.01)
        wide_span = (span > np.float32(3.13)) | np.isnan(span)
        wild = wide_span | close
        ts = np.where(dth >= 0, t1, t2)
        ts = np.where(ts < 0, ts + np.float32(6.28318531), ts)
        P, M = np.float32(6.283185307179586 / NBEAM), np.float32(2e-3)
        inv = np.float32(1.0) / P
        ilo = np.ceil((ts - M) * inv)
        ihi = np.floor((ts + span + M) * inv)
        cnt = np.nan_to_num(np.clip(ihi - ilo + 1, 0, NBEAM)).astype(int)
        cnt = np.where(wild, NBEAM, cnt)
        q1 = t1 * inv
        near_beam = np.abs(q1 - np.rint(q1)) * P <= np.float32(2.0e-4) + np.float32(1e-5)
    dx1, dy1, dx2, dy2 = p1[..., 0], p1[..., 1], p2[..., 0], p2[..., 1]
    cr = dx1 * dy2 - dx2 * dy1
    sc2 = (dx1 * dx1 + dy1 * dy1) * (dx2 * dx2 + dy2 * dy2)
    decisive = cr * cr > 1e-12 * sc2
    kccw, kconv = ccw[kept][:, None], convex[kept][:, None]
    front = decisive & ((cr > 0) != kccw)
    back = decisive & ~front
    thin = front & ((np.abs(dx2 - dx1) < 1e-4) | (np.abs(dy2 - dy1) < 1e-4))
    risky = wild | ~decisive | near_beam | thin | ~kconv
    ring_ok = ~risky.any(axis=1) & front.any(axis=1) & back.any(axis=1)
    culled = ring_ok[:, None] & back
    both = front.any(axis=1) & back.any(axis=1)
    gates = dict(wild=wild, undecisive=~decisive, near_beam=near_beam, thin=thin, nonconvex=np.broadcast_to(~kconv, wild.shape))
    blocked = {}                                                         # rings with both facings that ONE gate alone keeps from the cull
    for name, gate in gates.items():
        others = np.any([g.any(axis=1) for n2, g in gates.items() if n2 != name], axis=0)
        blocked[name] = int((gate.any(axis=1) & ~others & both).sum())
    blocked['one_facing'] = int((~risky.any(axis=1) & ~both).sum())
    if kept[0]:                                                          # (the first kept ring is then the lot's first ring)
        c['first'].update(near_beam=bool(near_beam[0].any()), thin=bool(thin[0].any()), undecisive=bool((~decisive[0]).any()),
                          wild=int(wild[0].sum()), culled=bool(ring_ok[0]), both_facings=bool(both[0]))
    d, e = p2[..., 1] - p1[..., 1], p1[..., 0] - p2[..., 0]
    det0 = (ab[:, 0, None, None] * e[None] - ab[:, 1, None, None] * d[None]) == 0
    c.update(pairs=int(np.where(culled, 0, cnt).sum()), pairs_nocull=int(cnt.sum()), wild=int(wild.sum()), wild_vertex=int(close.sum()),
             wild_span=int((wide_span & ~close).sum()), wide=int((np.where(culled, 0, cnt) > WAVE).sum()), near_beam=int(near_beam.sum()),
             thin=int(thin.sum()), undecisive=int((~decisive).sum()), culled_rings=int(ring_ok.sum()), cull_blocked_by=blocked,
             nonconvex=int((~kconv).sum()), cw=int((~kccw).sum()), det0=int(det0.any(axis=0).sum()), both_facings=int(both.sum()))
    return c


def beam_table():
    """[120][2] (sin theta, -cos theta): the table the oracle holds right now"""
    t = O.tables()
    return np.stack([t['beam_a'], t['beam_b']], axis=1)


def hull_base():
    return O.tables()['hull_base']


def oracle_scan(lot, rings=None):
    """the oracle's scan of the lot at its start pose, hull ranges added back: the clipped range per beam [120]"""
    q = lot.quads if rings is None else lot.quads[rings]
    if len(q) == 0:
        return np.full(NBEAM, LIDAR_RANGE)
    return O.lidar_observation(np.array(lot.pose), q, np.full(len(q), 4, np.int32)) + hull_base()


# ---- exact ray cast ----------------------------------------------------------------------------------------------------------------------------
def exact_ranges(ego, beams=None):
    """The exact nearest hit per beam on ego rings [m][4][2], every double (coordinates and the beam table's sin / -cos) taken as
    the rational it is.  -> range2 [120] (Fraction: the SQUARE of the range; None where no closed edge is met at t >= 0), and the
    float root.  Candidate edges are chosen in float64 with a wide margin, the hits are computed in Fraction."""
    Fr = E.Fr
    ab = beam_table()
    ego = np.asarray(ego, float).reshape(-1, 4, 2)
    p1 = ego.reshape(-1, 2)
    p2 = np.roll(ego, -1, axis=1).reshape(-1, 2)
    beams = range(NBEAM) if beams is None else beams
    r2 = [None] * NBEAM
    for i in beams:
        a, b = float(ab[i, 0]), float(ab[i, 1])
        ux, uy = -b, a                                                   # the beam's direction (cos, sin)
        s1, s2 = a * p1[:, 0] + b * p1[:, 1], a * p2[:, 0] + b * p2[:, 1]
        t1, t2 = ux * p1[:, 0] + uy * p1[:, 1], ux * p2[:, 0] + uy * p2[:, 1]
        cand = np.nonzero(~(((s1 > 1e-6) & (s2 > 1e-6)) | ((s1 < -1e-6) & (s2 < -1e-6))) & ~((t1 < -1e-6) & (t2 < -1e-6)))[0]
        A, B, UX, UY = Fr(a), Fr(b), Fr(ux), Fr(uy)
        uu = UX * UX + UY * UY
        best = None
        for j in cand:
            P, Q = E.F(p1[j]), E.F(p2[j])
            S1, S2 = A * P[0] + B * P[1], A * Q[0] + B * Q[1]
            if (S1 > 0 and S2 > 0) or (S1 < 0 and S2 < 0):
                continue
            T1, T2 = UX * P[0] + UY * P[1], UX * Q[0] + UY * Q[1]       # t |u|^2 of the end points
            if S1 == S2:                                                 # on the beam's line: the nearest point of the edge with t >= 0
                if max(T1, T2) < 0:
                    continue
                T = Fr(0) if min(T1, T2) <= 0 else min(T1, T2)
            else:
                lam = S1 / (S1 - S2)
                T = T1 + lam * (T2 - T1)
                if T < 0:
                    continue
            v = T * T / uu
            if best is None or v < best:
                best = v
        r2[i] = best
    root = np.array([math.sqrt(float(v)) if v is not None else math.inf for v in r2])
    return r2, root


def float_ranges(ego):
    """plain float64 ray cast on ego rings -> range [120] (inf: no hit), index of the edge hit [120].  A placement aid (which beams
    to look at), not a reference"""
    ab = beam_table()
    ego = np.asarray(ego, float).reshape(-1, 4, 2)
    p1, p2 = ego.reshape(-1, 2), np.roll(ego, -1, axis=1).reshape(-1, 2)
    a, b = ab[:, 0, None], ab[:, 1, None]
    s1, s2 = a * p1[None, :, 0] + b * p1[None, :, 1], a * p2[None, :, 0] + b * p2[None, :, 1]
    t1, t2 = -b * p1[None, :, 0] + a * p1[None, :, 1], -b * p2[None, :, 0] + a * p2[None, :, 1]
    with np.errstate(divide='ignore', invalid='ignore'):
        lam = s1 / (s1 - s2)
        t = t1 + lam * (t2 - t1)
    ok = (lam >= 0) & (lam <= 1) & (t >= 0)
    t = np.where(ok, t, np.inf)
    return t.min(axis=1), t.argmin(axis=1)


def vertex_beam_gap(ego):
    """smallest angle between a ring vertex and each beam direction -> [120] (rad)"""
    v = np.asarray(ego, float).reshape(-1, 2)
    ang = np.arctan2(v[:, 1], v[:, 0])
    dif = ang[None, :] - (np.arange(NBEAM) * PITCH)[:, None]
    dif = np.abs((dif + math.pi) % (2 * math.pi) - math.pi)
    return dif.min(axis=1) if len(v) else np.full(NBEAM, math.pi)
