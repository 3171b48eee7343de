"""Obstacles built to touch a vehicle hull, and scenes around them: input on which the orientation filter of the collision test
(hope_amd/csrc/hope_dev.h) cannot decide, so that the exact expansion behind it decides.  Generated lots and rollouts never
produce such input (tests/test_gpu_parity.py's tie census), these do.  Used by tests/test_gpu_exact_geometry.py; the premise
-- how many scenes really reach the robust path, and with which exact answer -- is computed here on the CPU with the numpy
mirror of the filter and exact rationals (tests/exact_geometry.py), and asserted by tests/test_touching_scenes.py.

Kind A: a diamond whose tip is a float64 point of a hull edge, moved by 0-2 ulp.  Kind B: a quad one edge of which passes
through a hull corner.  The poses come at coordinate scales of 4, 30 and 150 m: one ulp is sometimes inside and sometimes
outside the filter's error band."""
import math

import numpy as np

import exact_geometry as E
from oracle import oracle as O

CAR_XF, CAR_XR, CAR_YH = 0.96 + 2.8, -0.93, 1.94 / 2
SCALES = (4.0, 30.0, 150.0)
NUM_STEP = 10


def substep_poses(start, action):
    """the ten sub-step poses of one step from `start` with the policy action `action` in [-1, 1]^2 (None: the action-less step)"""
    if action is None:
        return np.array([start], float)
    phys = O.action_rescale(action)
    out, p = [], np.array(start, float)
    for _ in range(NUM_STEP):
        p, _ss = O.ks_step(p, phys)
        out.append(p.copy())
    return np.array(out)


def _ccw(quad):
    q = np.array(quad, float)
    x, y = q[:, 0], q[:, 1]
    return q if float(np.sum(x * np.roll(y, -1) - np.roll(x, -1) * y)) > 0 else q[::-1].copy()


def touching_obstacle(rng, box, kind=None, edge=None):
    """a quad that touches the hull `box` [4][2] from outside, up to the rounding of its own coordinates"""
    k = int(rng.integers(4)) if edge is None else int(edge)
    kind = ('A' if rng.random() < 0.75 else 'B') if kind is None else kind
    p, q, centre = box[k], box[(k + 1) % 4], box.mean(axis=0)
    if kind == 'A':
        t = rng.uniform(0.1, 0.9)
        tip = p + t * (q - p)
        e = (q - p) / np.linalg.norm(q - p)
        nrm = np.array([e[1], -e[0]])
        if np.dot(nrm, tip - centre) < 0:
            nrm = -nrm
        j = int(rng.integers(2))
        for _ in range(int(rng.integers(0, 3))):
            tip[j] = np.nextafter(tip[j], math.inf if rng.random() < 0.5 else -math.inf)
        d, w = rng.uniform(0.5, 1.0), rng.uniform(0.15, 0.4)
        return _ccw([tip, tip + 0.5 * d * nrm + w * e, tip + d * nrm, tip + 0.5 * d * nrm - w * e])
    g = (p - centre) / np.linalg.norm(p - centre)                 # the corner's diagonal, outwards
    u = np.array([g[1], -g[0]])
    l1, l2, d = rng.uniform(0.4, 1.0), rng.uniform(0.4, 1.0), rng.uniform(0.5, 1.0)
    return _ccw([p - l1 * u, p + l2 * u, p + l2 * u + d * g, p - l1 * u + d * g])


def hull_distance(poses, pts):
    """distance of points [m][2] from the hulls of poses [P][3] -> [P][m] (plain float64: a placement aid, not a reference)"""
    poses, pts = np.asarray(poses, float), np.asarray(pts, float)
    c, s = np.cos(poses[:, 2])[:, None], np.sin(poses[:, 2])[:, None]
    dx, dy = pts[None, :, 0] - poses[:, 0, None], pts[None, :, 1] - poses[:, 1, None]
    u, v = dx * c + dy * s, dy * c - dx * s
    du = np.maximum(np.maximum(CAR_XR - u, u - CAR_XF), 0)
    dv = np.maximum(np.abs(v) - CAR_YH, 0)
    return np.hypot(du, dv)


def hulls_box(poses):
    """(xmin, xmax, ymin, ymax) around the hulls of the poses"""
    b = np.concatenate([O.create_box(p) for p in poses])
    return b[:, 0].min(), b[:, 0].max(), b[:, 1].min(), b[:, 1].max()


def filler_quads(rng, poses, count):
    """up to `count` small quads, 1 cm or more off every hull of `poses`, whose box meets the box around those hulls: near
    obstacles for the step kernels' lists that the filter decides without trouble"""
    x0, x1, y0, y1 = hulls_box(poses)
    m = 6000
    h = rng.uniform(0.01, 0.03, m)
    cen = np.column_stack([rng.uniform(x0 - 0.02, x1 + 0.02, m), rng.uniform(y0 - 0.02, y1 + 0.02, m)])
    ok = hull_distance(poses, cen).min(axis=0) >= 1.6 * h + 0.01
    ok &= (cen[:, 0] - 0.9 * h < x1) & (cen[:, 0] + 0.9 * h > x0) & (cen[:, 1] - 0.9 * h < y1) & (cen[:, 1] + 0.9 * h > y0)
    out = []
    for i in np.nonzero(ok)[0][:count]:
        sq = np.array([[-1, -1], [1, -1], [1, 1], [-1, 1]], float) * h[i] * rng.uniform(0.95, 1.05, (4, 2))
        out.append(cen[i] + sq)
    return out


def far_quad(rng, centre, lo=7.0, hi=9.5):
    """a car-sized rectangle `lo`..`hi` metres from `centre`"""
    a, r, th = rng.uniform(0, 2 * np.pi), rng.uniform(lo, hi), rng.uniform(0, np.pi)
    c = np.asarray(centre[:2]) + r * np.array([np.cos(a), np.sin(a)])
    e, f = np.array([np.cos(th), np.sin(th)]), np.array([-np.sin(th), np.cos(th)])
    return np.array([c - e - 0.5 * f, c + e - 0.5 * f, c + e + 0.5 * f, c - e + 0.5 * f])


def near_count(poses, quads):
    """obstacles whose box meets the box around the hulls of the poses by more than 1e-9 m (the step kernels' near list)"""
    x0, x1, y0, y1 = hulls_box(poses)
    q = np.asarray(quads)
    e = 1e-9
    return int(((q[:, :, 0].min(1) < x1 - e) & (q[:, :, 0].max(1) > x0 + e) & (q[:, :, 1].min(1) < y1 - e) & (q[:, :, 1].max(1) > y0 + e)).sum())


def adversarial_scene(rng, scale, moving, many, dest_near=False):
    """-> start, dest, bbox, quads, action, k*: one lot with a touching obstacle at sub-step k* of the step `action` makes.
    dest_near: the dest box overlaps the start hull (by less than the arrival ratio), so that the first reward term of a new episode
    -- accumulated only if the start pose is free -- tells a collision at the start pose from none"""
    th = rng.uniform(-np.pi, np.pi)
    while many and abs(np.sin(2 * th)) < 0.3:                     # room for the fillers in the corners of the hulls' box
        th = rng.uniform(-np.pi, np.pi)
    start = np.array([rng.uniform(-scale, scale), rng.uniform(-scale, scale), th])
    action = rng.uniform(-1, 1, 2) if moving else np.zeros(2)
    poses = substep_poses(start, action)
    kstar = int(rng.integers(0, NUM_STEP))
    kind, edge = ('A' if rng.random() < 0.75 else 'B'), None
    if moving and rng.random() < 0.75:                            # mostly against the end that leads: the poses before k* stay clear of it
        lead = 1 if action[1] > 0 else 3                          # hull edge 1 is the front, 3 the rear; corner k starts edge k
        edge = lead if kind == 'A' else (lead + int(rng.integers(2))) & 3
    quads = [touching_obstacle(rng, O.create_box(poses[kstar]), kind=kind, edge=edge)]
    quads += filler_quads(rng, np.vstack([start[None], poses]), int(rng.integers(8, 12)) if many else int(rng.integers(0, 2)))
    if rng.random() < 0.5:
        quads.append(far_quad(rng, start))
    order = rng.permutation(len(quads))
    quads = [quads[i] for i in order]
    a, r = rng.uniform(0, 2 * np.pi), rng.uniform(9.0, 14.0)
    dest = np.array([start[0] + r * np.cos(a), start[1] + r * np.sin(a), rng.uniform(-np.pi, np.pi)])
    if dest_near:
        r = rng.uniform(0.6, 1.5)
        dest = np.array([start[0] + r * np.cos(a), start[1] + r * np.sin(a), start[2] + rng.uniform(-0.3, 0.3)])
    bbox = np.array([np.floor(start[0] - 30), np.ceil(start[0] + 30), np.floor(start[1] - 30), np.ceil(start[1] + 30)])
    return start, dest, bbox, quads, action, kstar


def build(n, seed, moving, max_obst=128, layout='mixed', dest_near=False):
    """n scenes of the small-tile class (<= 32 obstacles).  layout 'mixed': the first third adversarial at consecutive ids, then
    adversarial and plain generated scenes in turn; 'alternate': every other scene adversarial (a pool).  A third of the
    adversarial scenes carry 9-12 near obstacles.  -> dict of the arrays of hope_amd.scene_gen.mixed_arrays plus `action` [n][2]
    (zero in the adversarial scenes unless `moving`), `adv` [n] bool, `many` [n] bool, `kstar` [n]"""
    from hope_amd.scene_gen import mixed_arrays
    rng = np.random.default_rng(seed)
    first = n // 3 if layout == 'mixed' else 0
    adv = np.zeros(n, bool)
    adv[:first] = True
    adv[first::2] = True
    n_plain = int((~adv).sum())
    g = mixed_arrays(2 * n_plain + 64, levels=('Normal', 'Complex', 'Extrem'), seed=seed + 1, max_obst=max_obst)
    keep = np.nonzero(g[4] <= 32)[0][:n_plain]
    assert len(keep) == n_plain
    start, dest, bbox = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((n, 4))
    verts, nob = np.zeros((n, max_obst, 4, 2)), np.zeros(n, np.int32)
    for dst, src in zip((start, dest, bbox, verts, nob), g[:5]):
        dst[~adv] = src[keep]
    action = rng.uniform(-1, 1, (n, 2))
    many, kstar = np.zeros(n, bool), np.full(n, -1)
    for j, i in enumerate(np.nonzero(adv)[0]):
        many[i] = j % 3 == 2
        start[i], dest[i], bbox[i], quads, action[i], kstar[i] = adversarial_scene(rng, SCALES[(j // 3) % 3], moving, many[i], dest_near)
        nob[i] = len(quads)
        verts[i, :nob[i]] = quads
    return dict(start=start, dest=dest, bbox=bbox, verts=verts, nob=nob, nvert=np.full((n, max_obst), 4, np.int32),
                action=action, adv=adv, many=many, kstar=kstar)


def pair_table(box, quads):
    """segments_intersect_fast of the numpy mirror for (obstacle, obstacle edge j, hull edge k) -> [m][4][4]"""
    quads = np.asarray(quads, float)
    b1 = np.asarray(box, float)[None, None, :, :]
    b2 = np.roll(b1, -1, axis=-2)
    q1 = quads[:, :, None, :]
    q2 = np.roll(quads, -1, axis=-2)[:, :, None, :]
    return E.segments_fast_np(b1[..., 0], b1[..., 1], b2[..., 0], b2[..., 1], q1[..., 0], q1[..., 1], q2[..., 0], q2[..., 1])


def collision_filter_and_exact(box, quads):
    """-> (robust, hit): `robust`: the filter is sure of no pair and leaves some open (the device takes the robust path); `hit`: the
    EXACT answer of _detect_collision -- the filter's where it is sure (it may abstain but not lie: layer 2 of the tests pins
    that), exact rationals on the pairs it leaves open"""
    r = pair_table(box, quads)
    if (r == 1).any():
        return False, True
    op = np.argwhere(r == E.UNDECIDED)
    if len(op) == 0:
        return False, False
    hit = any(E.seg_intersect_exact(box[k], box[(k + 1) % 4], quads[m][j], quads[m][(j + 1) % 4]) for m, j, k in op)
    return True, hit


def census(sc, reset=False):
    """Which adversarial scenes reach "undecided, no certain hit" at a pose the reference's step visits (reset: the start pose of the
    action-less step; else the sub-step poses up to the first exact collision), and the exact answer there.
    -> robust [n] bool, answer [n] (1 exact intersection, 0 exact non-intersection at the first such pose, -1 not reached)"""
    n = len(sc['nob'])
    robust, answer = np.zeros(n, bool), np.full(n, -1)
    for i in np.nonzero(sc['adv'])[0]:
        quads = sc['verts'][i, :sc['nob'][i]]
        last = None
        for p in substep_poses(sc['start'][i], None if reset else sc['action'][i]):
            if last is None or not np.array_equal(p, last[0]):
                last = (p, collision_filter_and_exact(O.create_box(p), quads))
            rb, hit = last[1]
            if rb and not robust[i]:
                robust[i], answer[i] = True, int(hit)
            if hit:
                break
    return robust, answer


def assert_premise(sc, reset=False, tag=''):
    """the caps every scene test asserts before it compares anything: >= 25 % of the adversarial scenes on the robust path, each exact
    answer >= 10 % of those; prints the split"""
    robust, answer = census(sc, reset)
    n_adv, n_rb = int(sc['adv'].sum()), int(robust.sum())
    hit, miss = int((answer == 1).sum()), int((answer == 0).sum())
    print(f'touching scenes {tag}: adversarial {n_adv}, on the robust path {n_rb} ({100.0 * n_rb / n_adv:.1f} %), exact intersection {hit}, '
          f'exact non-intersection {miss}; with 9-12 near obstacles {int((robust & sc["many"]).sum())}')
    assert n_rb >= 0.25 * n_adv, (n_rb, n_adv)
    assert hit >= 0.10 * n_rb and miss >= 0.10 * n_rb, (hit, miss, n_rb)
    return robust, answer
