"""One-step cases with a programmed ACTION and POSE: what feeds every step (action rescale and clip, the 200-micro-step heading chain,
the ordered position sums: k_kinematics, wave_kinematics, the reader side of k_motion_pair) and what turns the step into a training
signal (k_post: the reward terms, accum_arrive_reward, the overlap area it clips itself under POST_F_NEED_UA, the target
representation), on the inputs where that code could be wrong and that random rollouts practically never produce.  Used by
tests/test_gpu_motion_reward.py; the premise -- which branch every case takes, with its margin, in exact rational arithmetic -- is
asserted on the CPU by tests/test_motion_reward_cases.py.

A case is a lot (start, dest, bbox, 0-3 quads far from the car; every cell once more with 40), an uploaded state (pose, t, accum), an
action and a `cell`.  Every case keeps its ten sub-steps (nothing is near the car) except the programmed arrival.  Cells:

  controls      steer and speed each at -1, 1, nextafter of each towards and away from 0, +-1.5, +-1e30, +-inf, +-0.0 and the smallest
                subnormal, next to an ordinary other control and next to themselves.  table(): rescaled float64; f32_cases(): the
                float32 values of the same list plus values whose float32 and float64 rescale differ in the last bit (float32 action
                buffer, with and without ACTION_RESCALE_F32); phys_cases(): ACTION_PHYSICAL float64 -- the list scaled to the valid
                range, values beyond it, the range ends +-1 ulp, and a speed of -0.0 (the rescale turns -0.0 into +0.0)
  chain         full lock at full speed both ways (largest dh), dh = 0 with speed != 0, speed 0 with steer != 0, from the start headings
                0, +-pi/2, +-pi as doubles and +-1 ulp of each, +-100 and +-1e4 (the reference never wraps the heading)
  zero          a pose with x or y (or both) equal to -0.0 and a speed of zero (either sign in phys_cases()) or not
  tiny          car at (0, 0), steer 0, heading 0 and pi (negative terms); the speed makes the displacement term speed cos STEP_LENGTH
                30, 70 and 31 subnormal ulps, values in [1, 64) 2^-1022 at which the three-operation division by 20 of k_kinematics
                (before its repair) differs from x / 20.0 -- found by div20_search(), an exact emulation -- and 2^-900
  tiny sin      steer 0, heading 600 ulp of the subnormal range and speed 1 / 20 of full: the Y term is 30 ulps although the speed is ordinary
                (|cos| of a double is never below 6e-17; |sin| has no such floor)
  time          t uploaded as 0, 1, 198, 199 (CONTINUE at t = 1, 2, 199, 200) and 200 (OUTTIME at 201)
  dnorm         |start - dest| below 10, above 10, exactly 10 (axis-aligned, so that sqrt returns 10) and its two neighbours
  fold          heading - dest heading of the current pose, of the previous pose and of both (steer 0) at 0, +-pi/2 as a double and
                +-1 ulp, +-pi and +-1 ulp, 3 pi / 2, +-(2 pi k + small) and +-1e-8 (the ill-conditioned end of acos(cos .)); the
                differences on the fold are exact (the subtraction the device performs returns the programmed double)
  overlap       the final pose beside the dest box: ratios 0.05, 0.5, 0.93 (slab bound of arrival_possible fails: k_post clips), 0.945
                (it passes: the walk computed it), 0.97 (ARRIVED instead); no overlap but within reach; centre distance 5.2 +- 1e-9
                (the quick reject of k_post), 5.08 and 5.075 (the largest at which two hulls can touch)
  accum         every overlapping case again with accum = the overlap term `bur` of a first oracle pass from accum 0, nextafter either
                side of it, and 1.5: equal, just below, just above, far above (0 is the first pass itself)
  target        dest position equal to the final pose (atan2(0, 0)); dest directly behind with rdy = +0.0 and -0.0; dest axis-aligned in
                the four directions; distances 8 + 2^-21 and 8 + 3 2^-21 (float32 ties, to even both ways); the headings of `chain`

scene_set(): the table as one batch of 4 101 scenes -- at the head of each tile chain's list a CENSUS BLOCK of six k_post waves that
hold exactly 0, 1, 16, 17, 33 and 64 clipping lanes (CLIP_COLS = 16: none, one partial round, one full round, a full and a partial
round, ...; clipping and non-clipping lanes alternate in the 17 and 33 waves), then permutations of the table; the 40-obstacle lots at
the tail.  Neither chain's length is a multiple of 16 (KIN_SCENES_PER_BLOCK)."""
import ctypes as C
import functools
from fractions import Fraction

import numpy as np

import touching_scenes as T
from oracle import oracle as O

NUM_STEP = 10
CONTINUE, ARRIVED, COLLIDED, OUTBOUND, OUTTIME = 1, 2, 3, 4, 5
PI = float(np.pi)
STEER_HI, SPEED_HI = 0.75, 2.5
STEP_LENGTH, MINI_ITER = 5e-2, 20
MID, HALF_L, HALF_W = 0.5 * (T.CAR_XF + T.CAR_XR), 0.5 * (T.CAR_XF - T.CAR_XR), T.CAR_YH
REACH = 5.2                                                     # the quick-reject radius of k_post
SUB = 5e-324                                                    # the smallest subnormal double
N_LARGE = 40
N_SCENES, CLS1_FRAC = 4101, 0.42
CENSUS = (0, 1, 16, 17, 33, 64)
SPOTS = ((0.5, -1.25), (12.375, 7.875), (-31.75, 22.125), (140.25, -87.5))


# ---- the three-operation division by 20, exactly ------------------------------------------------------------------------------
def div20_emulated(x):
    """q0 = RN(x R), r = RN(x - 20 q0), RN(q0 + r R) with R = RN(1 / 20): each operation evaluated in rational arithmetic and rounded
    once (int / int is correctly rounded in Python, subnormal results included)"""
    R, X = Fraction(0.05), Fraction(x)
    q0 = Fraction(float(X * R))
    r = Fraction(float(X - 20 * q0))
    return abs(float(q0 + r * R)) * (-1.0 if x < 0 else 1.0)


@functools.lru_cache(maxsize=None)
def div20_search(seed=3, draws=20000, keep=12):
    """-> (differing x in [1, 64) 2^-1022, how many of `draws` random x there differ, how many of `draws` in +-0.2 differ)"""
    rng = np.random.default_rng(seed)
    found, n_low, n_ord = [], 0, 0
    for m in rng.integers(1 << 52, 1 << 58, draws):
        x = float(int(m)) * SUB
        if div20_emulated(x) != x / 20.0:
            n_low += 1
            if len(found) < keep:
                found.append(x)
    for x in rng.uniform(-0.2, 0.2, draws):
        n_ord += div20_emulated(float(x)) != float(x) / 20.0
    return tuple(found), n_low, int(n_ord)


def term_of(action_speed, cos=1.0):
    """the displacement term of a rescaled speed action, as the reference evaluates it"""
    lo, hi = -SPEED_HI, SPEED_HI
    speed = np.clip(np.float64(action_speed), -1, 1) * (hi - lo) / 2 + (hi + lo) / 2
    return float(speed * np.float64(cos) * STEP_LENGTH)


def speed_action_for_term(x):
    """a rescaled speed action whose term at cos = 1 is the double x, or None (the map is 8 to 1 among the subnormals, about 1 to 1 above)"""
    up, down = np.float64(x) * 8, np.float64(x) * 8
    for _ in range(64):
        for a in (up, down):
            if term_of(a) == x:
                return float(a)
        up, down = np.nextafter(up, np.inf), np.nextafter(down, 0)
    return None


# ---- geometry ---------------------------------------------------------------------------------------------------------------
def poses_of(pose, action, physical=False):
    """[11][3]: the uploaded pose, then the ten sub-step poses"""
    phys = np.array(action, float) if physical else O.action_rescale(action)
    out, p = [np.array(pose, float)], np.array(pose, float)
    for _ in range(NUM_STEP):
        p, _ss = O.ks_step(p, phys)
        out.append(p.copy())
    return np.array(out)


def box_centre(pose):
    B = O.create_box(pose)
    return 0.5 * (B[0] + B[2])


def dest_beside(F, lat=0.0, lon=0.0, turn=0.0, centre=None):
    """dest whose box centre lies `lon` ahead and `lat` to the left of the box centre of pose F (or at `centre`), heading F's + turn"""
    u, nrm = np.array([np.cos(F[2]), np.sin(F[2])]), np.array([-np.sin(F[2]), np.cos(F[2])])
    c = box_centre(F) + lon * u + lat * nrm if centre is None else np.asarray(centre, float)
    hd = F[2] + turn
    return np.array([c[0] - MID * np.cos(hd), c[1] - MID * np.sin(hd), hd])


def slab_margin(pose, dest):
    """numpy mirror of arrival_possible (hope_step_kernel.h) -> (passes, distance of the deciding comparison from its threshold)"""
    ct, sn, cd, sd = np.cos(pose[2]), np.sin(pose[2]), np.cos(dest[2]), np.sin(dest[2])
    dx, dy = dest[0] + cd * MID - (pose[0] + ct * MID), dest[1] + sd * MID - (pose[1] + sn * MID)
    cphi, sphi = abs(ct * cd + sn * sd), abs(ct * sd - sn * cd)
    p, q = dx * ct + dy * sn, dy * ct - dx * sn
    hB, wB = HALF_L * cphi + HALF_W * sphi, HALF_L * sphi + HALF_W * cphi
    lov, wov = min(HALF_L, p + hB) - max(-HALF_L, p - hB), min(HALF_W, q + wB) - max(-HALF_W, q - wB)
    a, b = lov - (0.94 * 2 * HALF_L + 1e-6), wov - (0.94 * 2 * HALF_W + 1e-6)
    return (a >= 0 and b >= 0), (min(a, b) if a >= 0 and b >= 0 else -min(a, b) if min(a, b) < 0 else 0.0)


def centre_dist2_exact(pose, dest):
    """|centre of the hull's box - centre of the dest box|^2 as a Fraction of the boxes' doubles"""
    A, B = O.create_box(pose), O.create_box(dest)
    fx = lambda P, k: (Fraction(float(P[0, k])) + Fraction(float(P[2, k]))) / 2
    return (fx(A, 0) - fx(B, 0)) ** 2 + (fx(A, 1) - fx(B, 1)) ** 2


def far_quads(centre, count, seed):
    """`count` squares of half-size 0.4: the first at 7.5 m (the lidar sees it; the hull reaches 3.9 m + 1.25 m of travel), the rest 17-27 m away"""
    rng = np.random.default_rng(1000 + seed)
    out = []
    for i in range(count):
        r = 7.5 if i == 0 else rng.uniform(17.0, 27.0)
        a, phi = rng.uniform(0, 2 * PI), rng.uniform(0, PI / 2)
        c = np.asarray(centre[:2], float) + r * np.array([np.cos(a), np.sin(a)])
        e, f = 0.4 * np.array([np.cos(phi), np.sin(phi)]), 0.4 * np.array([-np.sin(phi), np.cos(phi)])
        out.append(np.array([c - e - f, c + e - f, c + e + f, c - e + f]))
    return out


_count = [0]


def case(cell, tag, pose, action, dest=None, start=None, t=5, accum=0.0, expect=CONTINUE, physical=False, n_obst=None, **extra):
    _count[0] += 1
    k = _count[0]
    pose = np.array(pose, float)
    if dest is None:
        a = 0.7 + 1.1 * k
        dest = np.array([pose[0] + 12.0 * np.cos(a), pose[1] + 12.0 * np.sin(a), 0.3 * k % 3.0 - 1.5])
    dest = np.array(dest, float)
    start = pose + np.array([1.5, -0.75, 0.25]) * (k % 2) if start is None else np.array(start, float)
    n_obst = k % 4 if n_obst is None else n_obst
    bbox = np.array([np.floor(pose[0] - 45), np.ceil(pose[0] + 45), np.floor(pose[1] - 45), np.ceil(pose[1] + 45)])
    return dict(cell=cell, tag=tag, pose=pose, action=np.array(action, float), dest=dest, start=start, t=int(t), accum=float(accum),
                expect=expect, physical=bool(physical), quads=far_quads(pose, n_obst, k), bbox=bbox, seed=k, **extra)


def large(c):
    """the case once more in a lot of 40 obstacles (the large-tile class)"""
    d = dict(c)
    d['quads'] = far_quads(c['pose'], N_LARGE, c['seed'])
    d['tag'] = c['tag'] + ' (40 obstacles)'
    return d


def spot(k, h=0.0):
    x, y = SPOTS[k % len(SPOTS)]
    return np.array([x, y, h])


# ---- the cells ---------------------------------------------------------------------------------------------------------------
def control_values(dt=np.float64):
    one, big = dt(1), dt(1e30)
    v = [one, np.nextafter(one, dt(0)), np.nextafter(one, dt(2)), dt(1.5), big, dt(np.inf), dt(0.0), np.nextafter(dt(0), one)]
    return [s * x for x in v for s in (dt(1), dt(-1))]


def last_bit_values(count=6, seed=5):
    """float32 actions whose rescaled speed in float32 Box arithmetic differs from the float64 arithmetic (as the float32 test of
    tests/test_gpu_parity.py draws them)"""
    rng = np.random.default_rng(seed)
    a = rng.uniform(-1.0, 1.0, 4000).astype(np.float32)
    p32 = a * np.float32(2 * SPEED_HI) / np.float32(2) + np.float32(0)
    p64 = a.astype(np.float64) * (2 * SPEED_HI) / 2 + 0.0
    idx = np.nonzero(p32.astype(np.float64) != p64)[0]
    assert len(idx) >= count
    return [a[i] for i in idx[:count]]


def control_cases(values, physical=False):
    """physical: the [-1, 1] list scaled to the valid range (steer x 0.75, speed x 2.5)"""
    ks, kp = (STEER_HI, SPEED_HI) if physical else (1.0, 1.0)
    out = []
    for i, v in enumerate(values):
        v = float(v)
        for j, (st, sp) in enumerate(((v, 0.7), (v, -1.0), (0.6, v), (-1.0, v), (v, v))):
            out.append(case('controls', f'controls {"steer" if j < 2 else "speed" if j < 4 else "both"} {v!r}', spot(i + j, 0.3 + 0.37 * j),
                            (st * ks, sp * kp), physical=physical))
    return out


START_HEADINGS = (0.0, PI / 2, -PI / 2, PI, -PI, float(np.nextafter(PI, 0)), float(np.nextafter(PI, 4)), float(np.nextafter(-PI, 0)),
                  float(np.nextafter(-PI, -4)), float(np.nextafter(PI / 2, 0)), float(np.nextafter(PI / 2, 2)), float(np.nextafter(-PI / 2, 0)),
                  float(np.nextafter(-PI / 2, -2)), 100.0, -100.0, 1e4, -1e4)
CHAIN_ACTIONS = (('full lock', (1.0, 1.0)), ('full lock', (-1.0, 1.0)), ('full lock', (1.0, -1.0)), ('full lock', (-1.0, -1.0)),
                 ('dh 0', (0.0, 0.8)), ('dh 0', (0.0, -1.0)), ('speed 0', (0.5, 0.0)), ('speed 0', (-1.0, -0.0)))


def chain_cases(physical=False):
    sc = (STEER_HI, SPEED_HI) if physical else (1.0, 1.0)
    out = []
    for i, h in enumerate(START_HEADINGS):
        for j, (name, a) in enumerate(CHAIN_ACTIONS):
            out.append(case('chain', f'chain {name} heading {h!r}', spot(i + j, h), (a[0] * sc[0], a[1] * sc[1]), physical=physical))
    return out


def zero_cases(physical=False):
    sc = (STEER_HI, SPEED_HI) if physical else (1.0, 1.0)
    out = []
    for xy in ((-0.0, 3.0), (3.0, -0.0), (-0.0, -0.0), (0.0, -0.0)):
        for h in (0.0, PI / 2, PI, -0.0):
            for sp in (0.0, -0.0, 0.6, -0.6):
                out.append(case('zero', f'zero pose {xy!r} speed {sp!r}', (xy[0], xy[1], h), (0.5 * sc[0], sp * sc[1]), physical=physical))
    return out


def tiny_cases():
    found, _n_low, _n_ord = div20_search()
    found = [x for x in found if speed_action_for_term(x) is not None][:4]
    assert len(found) >= 3
    terms = [30 * SUB, 70 * SUB, 31 * SUB, *found, 2.0 ** -900]
    out = []
    for x in terms:
        a = speed_action_for_term(x)
        assert a is not None, x
        for h in (0.0, PI):
            for sgn in (1.0, -1.0):
                out.append(case('tiny', f'tiny term {x!r} heading {h!r}', (0.0, 0.0, h), (0.0, sgn * a), term=x * sgn * (1.0 if h == 0.0 else -1.0)))
    for h in (600 * SUB, -600 * SUB, 1400 * SUB):                 # the Y term is tiny because sin(h) = h is, at an ordinary speed
        out.append(case('tiny sin', f'tiny sin heading {h!r}', (0.0, 0.0, h), (0.0, 0.4), term=float(np.float64(1.0) * h * STEP_LENGTH)))
    return out


def time_cases():
    return [case('time', f't uploaded {t}', spot(i, 0.4), (0.3, 0.7), t=t, expect=OUTTIME if t >= 200 else CONTINUE) for i, t in enumerate((0, 1, 198, 199, 200))]


def dnorm_cases():
    out = []
    for axis in (0, 1):
        dest = np.array([13.5, 7.25, 0.8])
        for name, off in (('below', 6.0), ('above', 14.0), ('exactly 10', 10.0), ('10 - 1 ulp', float(np.nextafter(10.0, 0))), ('10 + 1 ulp', float(np.nextafter(10.0, 20)))):
            start = dest.copy()
            start[axis] = dest[axis] + off
            if 'ulp' in name:
                start[axis] = np.nextafter(dest[axis] + 10.0, -np.inf if '-' in name else np.inf)
            out.append(case('dnorm', f'dnorm {name} axis {axis}', (1.5, 2.25, 0.6), (0.4, 0.9), dest=dest, start=start, dnorm=name))
    out.append(case('dnorm', 'dnorm below, oblique', (1.5, 2.25, 0.6), (0.4, 0.9), dest=(13.5, 7.25, 0.8), start=(9.0, 3.0, 0.1), dnorm='below'))
    out.append(case('dnorm', 'dnorm above, oblique', (1.5, 2.25, 0.6), (0.4, 0.9), dest=(13.5, 7.25, 0.8), start=(1.0, -3.0, 0.1), dnorm='above'))
    return out


FOLD_DELTAS = (('0', 0.0, True), ('pi/2', PI / 2, True), ('pi/2 - ulp', float(np.nextafter(PI / 2, 0)), True), ('pi/2 + ulp', float(np.nextafter(PI / 2, 2)), True),
               ('pi', PI, True), ('pi - ulp', float(np.nextafter(PI, 0)), True), ('pi + ulp', float(np.nextafter(PI, 4)), True),
               ('3 pi / 2', 3 * PI / 2, False), ('6 pi + 1e-3', 6 * PI + 1e-3, False), ('10 pi + 0.3', 10 * PI + 0.3, False), ('1e-8', 1e-8, False))


def dest_heading(h, delta, exact):
    """dest heading d with h - d == delta as the device subtracts them (exact: required, else as close as the doubles allow)"""
    d0 = h - delta
    for d in (d0, np.nextafter(d0, np.inf), np.nextafter(d0, -np.inf)):
        if h - d == delta:
            return float(d)
    assert not exact, (h, delta)
    return float(d0)


def fold_cases():
    out = []
    for which in ('current', 'previous', 'both'):
        for name, delta, exact in FOLD_DELTAS:
            for sgn in (1.0, -1.0):
                if sgn < 0 and delta == 0.0:
                    continue
                # headings in [2, 4) (mirrored for negative differences): there h - delta is a double for the deltas on the fold
                h0 = sgn * (3.0 if abs(delta) < 4 else 2.5)
                action = (0.0, 0.8) if which == 'both' else (sgn * 0.7, 0.9)
                pose = spot(len(out), h0)
                Q = poses_of(pose, action)
                h = Q[-1][2] if which == 'current' else h0
                d = dest_heading(h, sgn * delta, exact)
                c = case('fold', f'fold {which} pose, heading - dest heading = {"-" if sgn < 0 else ""}{name}', pose, action)
                c['dest'][2] = d
                c.update(fold_which=which, fold_delta=sgn * delta, fold_exact=bool(h - d == sgn * delta))
                out.append(c)
    return out


def overlap_cases():
    out = []
    W = 2 * HALF_W

    def add(tag, make, expect=CONTINUE, **kw):
        for i, (h0, action) in enumerate(((0.45, (0.2, 0.8)), (-2.1, (-0.6, -1.0)))):
            pose = spot(len(out) + i, h0)
            F = poses_of(pose, action)[-1]
            out.append(case('overlap', f'overlap {tag}', pose, action, dest=make(F), expect=expect, overlap=tag, **kw))

    for r in (0.05, 0.5, 0.93, 0.945):
        add(f'ratio {r}', lambda F, r=r: dest_beside(F, lat=(1 - r) * W), ratio=r)
    add('ratio 0.97', lambda F: dest_beside(F, lat=0.03 * W), expect=ARRIVED, ratio=0.97)
    add('none, within reach', lambda F: dest_beside(F, lat=2.5, lon=3.0, turn=0.7))
    add('turned 0.35', lambda F: dest_beside(F, lat=0.3, lon=-0.4, turn=0.35))
    for d in (REACH - 1e-9, REACH + 1e-9, 5.08, 5.075):
        diag = np.arctan2(HALF_W, HALF_L)
        add(f'centre distance {d!r}', lambda F, d=d: dest_beside(F, centre=box_centre(F) + d * np.array([np.cos(F[2] + diag), np.sin(F[2] + diag)])), reach=d)
    return out


def target_cases():
    out = []
    pose, action = np.array([5.0, 0.0, 0.0]), (0.0, 0.6)
    F = poses_of(pose, action)[-1]
    assert F[1] == 0.0 and not np.signbit(F[1]) and F[2] == 0.0
    for tag, dest in (('behind, rdy +0.0', (F[0] - 9.0, 0.0, 0.4)), ('behind, rdy -0.0', (F[0] - 9.0, -0.0, 0.4)), ('ahead', (F[0] + 9.0, 0.0, -0.4)),
                      ('left', (F[0], 9.0, 1.0)), ('right', (F[0], -9.0, 1.0)), ('float32 tie 8 + 2^-21', (F[0], 8.0 + 2.0 ** -21, 0.5)),
                      ('float32 tie 8 + 3 2^-21', (F[0], 8.0 + 3 * 2.0 ** -21, 0.5)), ('float32 tie, below', (F[0], -(8.0 + 2.0 ** -21), 0.5))):
        out.append(case('target', f'target {tag}', pose, action, dest=dest, target=tag))
    for i, (h0, action) in enumerate(((0.45, (0.2, 0.8)), (-2.1, (-0.6, -1.0)), (PI, (1.0, 1.0)))):
        pose = spot(i, h0)
        F = poses_of(pose, action)[-1]
        out.append(case('target', 'target dest position = final pose', pose, action, dest=(F[0], F[1], F[2] + 0.9), target='atan2(0, 0)'))
    return out


def _arrays(cases, max_obst=128):
    n = len(cases)
    sc = dict(start=np.zeros((n, 3)), dest=np.zeros((n, 3)), bbox=np.zeros((n, 4)), verts=np.zeros((n, max_obst, 4, 2)), nob=np.zeros(n, np.int32),
              nvert=np.full((n, max_obst), 4, np.int32), pose=np.zeros((n, 3)), t=np.zeros(n, np.int32), accum=np.zeros(n), action=np.zeros((n, 2)))
    for i, c in enumerate(cases):
        for key in ('start', 'dest', 'bbox', 'pose', 't', 'accum', 'action'):
            sc[key][i] = c[key]
        sc['nob'][i] = len(c['quads'])
        if c['quads']:
            sc['verts'][i, :len(c['quads'])] = c['quads']
    sc['expect'] = np.array([c['expect'] for c in cases], np.int32)
    sc['cell'] = np.array([c['cell'] for c in cases])
    return sc


# ---- the oracle's step from an uploaded state ------------------------------------------------------------------------------
class _Scene(C.Structure):
    _fields_ = [('n_obst', C.c_int32), ('verts', C.c_void_p), ('nvert', C.c_void_p), ('start', C.c_double * 3), ('dest', C.c_double * 3),
                ('bbox', C.c_double * 4), ('pose', C.c_double * 3), ('t', C.c_double), ('accum', C.c_double)]


class _Obs(C.Structure):
    _fields_ = [('lidar', C.c_double * O.NBEAM), ('mask', C.c_double * O.NACT), ('target', C.c_double * 5), ('reward_info', C.c_double * 5),
                ('reward', C.c_double), ('status', C.c_int32), ('done', C.c_int32), ('rs_found', C.c_int32), ('rs_nseg', C.c_int32),
                ('rs_ctypes', C.c_int32 * 5), ('rs_lengths', C.c_double * 5), ('rs_L', C.c_double), ('substeps', C.c_int32),
                ('collided_substep', C.c_int32)]


def oracle_step(sc, physical=False, action=None):
    """one oracle step of every scene from its uploaded state; physical: orc_env_step_physical (CarParking.step itself) on the
    actions as they stand, else the wrapper's step with its float64 action_rescale.  -> dict of outputs and state words"""
    n = len(sc['nob'])
    action = np.ascontiguousarray(sc['action'] if action is None else action, np.float64)
    mo = sc['verts'].shape[1]
    if not physical:
        orc = O.BatchOracle(n, mo, omp=True, track_traj=False)
        orc.set_scenes(np.arange(n), sc['start'], sc['dest'], sc['bbox'], sc['verts'], sc['nvert'], sc['nob'])
        orc.pose[:], orc.t[:], orc.accum[:] = sc['pose'], sc['t'], sc['accum']
        o = orc.step(action, with_rs=False)
        return dict(status=o['status'].copy(), done=(o['status'] != CONTINUE).astype(np.uint8), reward=o['reward'].copy(), reward_info=o['reward_info'].copy(),
                    lidar=o['lidar'].copy(), action_mask=o['mask'].copy(), target=o['target'].copy(), pose=orc.pose.copy(), t=orc.t.astype(np.int32),
                    accum=orc.accum.copy(), substeps=o['substeps'].copy())
    L = O.lib()
    out = dict(status=np.zeros(n, np.int32), done=np.zeros(n, np.uint8), reward=np.zeros(n), reward_info=np.zeros((n, 5)), lidar=np.zeros((n, O.NBEAM)),
               action_mask=np.zeros((n, O.NACT)), target=np.zeros((n, 5)), pose=np.zeros((n, 3)), t=np.zeros(n, np.int32), accum=np.zeros(n),
               substeps=np.zeros(n, np.int32))
    verts, nvert = np.ascontiguousarray(sc['verts'], np.float64), np.ascontiguousarray(sc['nvert'], np.int32)
    for i in range(n):
        s, o = _Scene(), _Obs()
        s.n_obst, s.verts, s.nvert = int(sc['nob'][i]), verts[i].ctypes.data, nvert[i].ctypes.data
        s.start[:], s.dest[:], s.bbox[:], s.pose[:] = sc['start'][i], sc['dest'][i], sc['bbox'][i], sc['pose'][i]
        s.t, s.accum = float(sc['t'][i]), float(sc['accum'][i])
        a = (C.c_double * 2)(*action[i])
        L.orc_env_step_physical(C.byref(s), a, C.byref(o), C.c_int(0))
        out['status'][i], out['done'][i], out['reward'][i], out['substeps'][i] = o.status, o.done, o.reward, o.substeps
        out['reward_info'][i], out['lidar'][i], out['action_mask'][i], out['target'][i] = o.reward_info[:], o.lidar[:], o.mask[:], o.target[:]
        out['pose'][i], out['t'][i], out['accum'][i] = s.pose[:], int(s.t), s.accum
    return out


# ---- the table ---------------------------------------------------------------------------------------------------------------
def _annotate(cases, ref):
    """what the premise and the census need of every case: the final pose, whether k_post clips it, and how clearly"""
    for i, c in enumerate(cases):
        F = ref['pose'][i]
        passes, margin = slab_margin(F, c['dest'])
        d2 = centre_dist2_exact(F, c['dest'])
        inside = d2 <= Fraction(REACH) ** 2
        c['final'] = F.copy()
        c['clip'] = bool(ref['status'][i] == CONTINUE and not passes and inside)
        c['clip_clear'] = bool(margin > 1e-3 and abs(float(d2) ** 0.5 - REACH) > 1e-3)
        c['bur'] = float(ref['accum'][i])


@functools.lru_cache(maxsize=None)
def table():
    """every case of the module docstring's cells for the rescaled float64 path, each cell once more in a 40-obstacle lot"""
    _count[0] = 0
    base = control_cases(control_values()) + chain_cases() + zero_cases() + tiny_cases() + time_cases() + dnorm_cases() + fold_cases()
    over = overlap_cases() + target_cases()
    # the accum branch: a first oracle pass from accum = 0 gives every overlapping case's `bur`
    first = oracle_step(_arrays(over))
    acc = []
    for i, c in enumerate(over):
        bur = float(first['accum'][i])
        if first['status'][i] == CONTINUE and bur > 0.0:
            for name, a in (('equal', bur), ('1 ulp above bur', float(np.nextafter(bur, 2))), ('1 ulp below bur', float(np.nextafter(bur, 0))), ('far above', 1.5)):
                d = dict(c)
                d.update(cell='accum', tag=f'accum {name}: {c["tag"]}', accum=a, accum_kind=name, first_bur=bur)
                acc.append(d)
    out = base + over + acc
    seen = set()
    for c in list(out):
        key = (c['cell'], c.get('fold_which'), c.get('accum_kind'))
        if key not in seen:
            seen.add(key)
            out.append(large(c))
    _annotate(out, oracle_step(_arrays(out)))
    return out


@functools.lru_cache(maxsize=None)
def f32_cases():
    """the float32 subset: float32 control values, the last-bit values, chain and zero actions (all float32-representable)"""
    _count[0] = 10000
    out = control_cases([float(v) for v in control_values(np.float32)] + [float(v) for v in last_bit_values()]) + chain_cases() + zero_cases()
    for c in out:                                                 # the ordinary partners (0.7, 0.6, ...) as float32 too
        c['action'] = c['action'].astype(np.float32).astype(np.float64)
    return out + [large(out[0]), large(out[-1])]


@functools.lru_cache(maxsize=None)
def phys_cases():
    """ACTION_PHYSICAL: the control list scaled to the valid range, values beyond it, the range ends +-1 ulp, chain and zero cases"""
    _count[0] = 20000
    vals = control_values()
    out = control_cases(vals, physical=True)
    ends = []
    for hi in (STEER_HI, SPEED_HI):
        ends.append([s * x for x in (hi, float(np.nextafter(hi, 0)), float(np.nextafter(hi, 4)), 1.25 * hi, 3.0) for s in (1.0, -1.0)])
    for st, sp in zip(*ends):
        out += [case('controls', f'controls physical steer {st!r}', spot(len(out), 0.3), (st, 1.7), physical=True),
                case('controls', f'controls physical speed {sp!r}', spot(len(out), -0.9), (0.4, sp), physical=True),
                case('controls', f'controls physical both {st!r} {sp!r}', spot(len(out), 2.0), (st, sp), physical=True)]
    out += chain_cases(physical=True) + zero_cases(physical=True)
    return out + [large(out[0]), large(out[-1])]


def case_arrays(cases):
    sc = _arrays(cases)
    sc['case'] = np.arange(len(cases), dtype=np.int32)
    return sc


# ---- the scene set -----------------------------------------------------------------------------------------------------------
def _census_block(tab, small, rng):
    """6 x 64 table indices: k_post wave w holds exactly CENSUS[w] clipping lanes (17 and 33: alternating with non-clipping ones)"""
    clip = [i for i in small if tab[i]['clip'] and tab[i]['clip_clear']]
    rest = [i for i in small if not tab[i]['clip'] and (tab[i]['clip_clear'] or tab[i]['expect'] != CONTINUE)]
    assert len(clip) >= 8 and len(rest) >= 64
    out = []
    for k in CENSUS:
        wave = [int(rest[int(j)]) for j in rng.integers(len(rest), size=64)]
        pos = np.arange(0, 2 * k, 2) if 2 * k <= 64 else np.round(np.linspace(0, 63, k)).astype(int) if k < 64 else np.arange(64)
        assert len(set(pos.tolist())) == k
        for p in pos:
            wave[int(p)] = int(clip[int(rng.integers(len(clip)))])
        out += wave
    return out


@functools.lru_cache(maxsize=None)
def scene_set(seed=11, max_obst=128):
    """-> dict of arrays, `case` [n] table indices; `m`: the length of the small-tile chain's list (ids 0 .. m - 1; the overlapped
    handle hands the ids above to the large-tile chain), `fused_rows`: the 4 095 rows of form (a), chosen so that the census blocks stay
    at the head of both lists there too"""
    tab = table()
    rng = np.random.default_rng(seed)
    n = N_SCENES
    m = n - int(CLS1_FRAC * n)
    small = [i for i, c in enumerate(tab) if len(c['quads']) <= 32]
    big = [i for i, c in enumerate(tab) if len(c['quads']) > 32]
    tail = big + big
    block = 64 * len(CENSUS)
    assert len(tail) < int(CLS1_FRAC * n) - block and m % 16 and (n - m) % 16 and n > 4096

    def fill(count):
        out = []
        while len(out) < count:
            out += [int(i) for i in rng.permutation(small)]
        return out[:count]

    case_ = _census_block(tab, small, rng) + fill(m - block) + _census_block(tab, small, rng) + fill(n - m - block - len(tail)) + tail
    assert len(case_) == n and m - block >= len(small) and n - m - block - len(tail) >= len(small)      # every small case in both chains
    sc = _arrays([tab[k] for k in case_], max_obst)
    sc['case'] = np.array(case_, np.int32)
    sc['clip'] = np.array([tab[k]['clip'] for k in case_])
    sc['clip_clear'] = np.array([tab[k]['clip_clear'] for k in case_])
    # form (a): 4 095 scenes whose lists begin with the census blocks too -- the small-tile list shrinks by 3 (fillers just below m go),
    # the large-tile list by 3 (fillers just above its block go)
    na = 4095
    ma = na - int(CLS1_FRAC * na)
    drop = list(range(m - (m - ma), m)) + list(range(m + block, m + block + (n - na) - (m - ma)))
    assert len(drop) == n - na and 0 <= m - ma <= n - na
    sc_rows = np.setdiff1d(np.arange(n), drop)
    return sc, m, sc_rows


def subset(sc, rows):
    return {k: v[rows] for k, v in sc.items()}


def post_wave_census(plan, clip):
    """clipping lanes per k_post wave (64 consecutive entries of a chain's list), per chain"""
    return [[int(clip[c['scenes'][w:w + 64]].sum()) for w in range(0, len(c['scenes']), 64)] for c in plan['chains']]
