"""One-step cases with a programmed sub-step event: where CarParking.step stops among its ten sub-step poses ("arrived? stop;
collided? retreat and stop", then _check_status on the pose that is left) is known BY CONSTRUCTION, so that every hand-written form
of that walk on the device (k_env_step's lane-grouped and serial walks, its PART 0 / PART 1, k_motion_pair's two halves) can be held
against the oracle on the cases where the forms could disagree.  Used by tests/test_gpu_substep_events.py; the premise -- the
oracle really stops where the table says, the margins hold, the near list has exactly the programmed length, every cell of the table
is filled -- is asserted on the CPU by tests/test_substep_events.py.

A case is a lot (start, dest, bbox, <= 32 quads; a few with 40), an uploaded state (pose, t, accum) and an action.  Kinds:
  K0  free run: no event, all ten sub-steps kept
  K1  collision first at sub-step kc (a 1 cm quad with a vertex >= 1 mm inside the hull of pose kc, >= 2 mm off every earlier hull)
  K2  arrival at sub-step ka (dest: a blend of two consecutive poses of the step extended to 16 sub-steps; no overlap ratio of the
      start pose or of poses 0..9 within 0.003 of 0.95, so nothing rests on the threshold's last bits)
  K3  both, |ka - kc| <= 1 and a few far pairs: the same sub-step goes to the arrival, kc = ka - 1 to the collision
  K4  near miss: dest shifted sideways and turned a little, best ratio of the ten poses in (0.90, 0.945) while pose kc still passes the
      device's slab bound (its overlap is computed, then the collision at kc cuts it off), accum 0 / 0.3 / 0.9 uploaded
  K5  the final pose's rear axle exactly ON an edge of the bbox (not OUTBOUND) and the edge one ulp further in (OUTBOUND), for a final
      pose 9, a retreat pose and the start pose; an arrival found at a pose outside the bbox
  K6  t uploaded as 199 and 200, crossed with a free run, a retreat, an arrival and an OUTBOUND final pose
  K7  blocked at sub-step 0, with the dest box far away and with the dest box over the start pose (a near miss)
Every kind comes with a programmed NEAR-LIST length: obstacles whose box meets the box around the start hull and the ten hulls (the
box k_kinematics records) -- every obstacle's box is at least 1 mm inside or outside of that box's edges, so that the float32 outward
rounding of the device's boxes cannot change the count."""
import functools

import numpy as np

import touching_scenes as T
from oracle import oracle as O

NUM_STEP, EXT_STEP = 10, 16
N_NEAR = (0, 1, 2, 3, 4, 5, 8, 9, 16, 17, 24, 25, 32)           # both sides of every S / pass-count boundary of the walks
N_NEAR_LARGE = 40                                               # large-tile class only (max_obst 128)
HALF_CLASSES = ('nothing to walk', '1', '2', '3-4', '5-8', '9-16', '17-24', '25-32')
CONTINUE, ARRIVED, COLLIDED, OUTBOUND, OUTTIME = 1, 2, 3, 4, 5
KINDS = ('K0', 'K1', 'K2', 'K3', 'K4', 'K5', 'K6', 'K7')
FAR_PAIRS = ((2, 7), (7, 2), (0, 9), (9, 0), (4, 8), (8, 3))    # (ka, kc) of K3 beyond |ka - kc| <= 1
ARRIVE_RATIO, RATIO_BAND, START_RATIO_MAX = 0.95, 0.003, 0.947
NEAR_MARGIN, HIT_DEPTH, HIT_CLEAR = 1e-3, 1e-3, 2e-3
MAX_ROUNDS = 400                                                # re-draws of one case before the builder gives up, loudly


def half_class(n_near):
    """index into HALF_CLASSES: the edge-slot class S (and pass count) a half of a pair wave walks with"""
    return n_near if n_near <= 2 else 3 if n_near <= 4 else 4 if n_near <= 8 else 5 + (n_near - 9) // 8


def extended_poses(pose, action, steps=EXT_STEP):
    """[1 + steps][3]: the uploaded pose, then the sub-step poses of `action` continued to `steps` sub-steps"""
    phys = O.action_rescale(action)
    out, p = [np.array(pose, float)], np.array(pose, float)
    for _ in range(steps):
        p, _ss = O.ks_step(p, phys)
        out.append(p.copy())
    return np.array(out)


def inside_depth(pose, pts):
    """how far the points [m][2] lie inside the hull of `pose` (negative: outside, then not a distance)"""
    pts = np.asarray(pts, float)
    c, s = np.cos(pose[2]), np.sin(pose[2])
    dx, dy = pts[:, 0] - pose[0], pts[:, 1] - pose[1]
    u, v = dx * c + dy * s, dy * c - dx * s
    return np.minimum(np.minimum(u - T.CAR_XR, T.CAR_XF - u), T.CAR_YH - np.abs(v))


def ratios(poses, dest):
    """|hull ∩ dest| / |dest| of every pose, as check_arrived computes it"""
    B = O.create_box(dest)
    area = O.quad_area(B)
    return np.array([O.quad_intersection_area(O.create_box(p), B) / area for p in poses])


def near_flags(box, quads, m=NEAR_MARGIN):
    """-> near, far [m] bool: the quad's box meets / misses the box (x0, x1, y0, y1) by at least m on the deciding axis"""
    x0, x1, y0, y1 = box
    q = np.asarray(quads, float).reshape(-1, 4, 2)
    qx0, qx1, qy0, qy1 = q[:, :, 0].min(1), q[:, :, 0].max(1), q[:, :, 1].min(1), q[:, :, 1].max(1)
    near = (qx0 < x1 - m) & (qx1 > x0 + m) & (qy0 < y1 - m) & (qy1 > y0 + m)
    far = (qx0 > x1 + m) | (qx1 < x0 - m) | (qy0 > y1 + m) | (qy1 < y0 - m)
    return near, far


def hit_quad(rng, Q, kc, speed):
    """a quad of half-size ~5 mm with a vertex >= 1.5 mm inside and a vertex outside the hull of pose kc (Q[kc + 1]) that stays >= 2 mm
    off the hulls of Q[0..kc] (it lies in a disc that does), or None"""
    pose = Q[kc + 1]
    c, s = np.cos(pose[2]), np.sin(pose[2])
    for _ in range(60):
        if rng.random() < 0.7:                                    # the end that leads
            lead = speed > 0
            u, v = (T.CAR_XF if lead else T.CAR_XR), rng.uniform(-0.9, 0.9) * T.CAR_YH
            inward = np.array([-1.0 if lead else 1.0, 0.0])
        else:                                                     # a side (a turning hull sweeps sideways)
            side = 1.0 if rng.random() < 0.5 else -1.0
            u, v = rng.uniform(T.CAR_XR + 0.1, T.CAR_XF - 0.1), side * T.CAR_YH
            inward = np.array([0.0, -side])
        loc = np.array([u, v]) + inward * rng.uniform(1.5e-3, 3e-3)
        V = np.array([pose[0] + c * loc[0] - s * loc[1], pose[1] + s * loc[0] + c * loc[1]])
        h, phi = rng.uniform(4.5e-3, 5.5e-3), rng.uniform(0, 2 * np.pi)
        e, f = np.array([np.cos(phi), np.sin(phi)]), np.array([-np.sin(phi), np.cos(phi)])
        cen = V - h * (e + f)
        quad = np.array([cen - h * e - h * f, cen + h * e - h * f, cen + h * e + h * f, cen - h * e + h * f])
        d = inside_depth(pose, quad)
        if d.max() < 1.5 * HIT_DEPTH or d.min() > -HIT_DEPTH:     # edges of the quad must cross the hull's
            continue
        if T.hull_distance(Q[:kc + 1], cen[None]).min() < 1.5 * h + HIT_CLEAR + 1e-3:
            continue
        return quad
    return None


def fillers(rng, Q, count, box):
    """`count` small quads, >= 1 cm off every hull of Q[0..10], whose box meets `box` by >= 1 mm (some straddle its edges), or None"""
    if count == 0:
        return []
    x0, x1, y0, y1 = box
    m = 6000
    h = rng.uniform(0.01, 0.03, m)
    cen = np.column_stack([rng.uniform(x0 - 0.02, x1 + 0.02, m), rng.uniform(y0 - 0.02, y1 + 0.02, m)])
    ok = T.hull_distance(Q[:NUM_STEP + 1], cen).min(axis=0) >= 1.6 * h + 0.01
    idx = np.nonzero(ok)[0]
    sq = np.array([[-1, -1], [1, -1], [1, 1], [-1, 1]], float)
    quads = cen[idx, None, :] + sq[None] * h[idx, None, None] * rng.uniform(0.95, 1.05, (len(idx), 4, 2))
    near, _far = near_flags(box, quads)
    quads = quads[near]
    return list(quads[:count]) if len(quads) >= count else None


def outside_quads(rng, Q, count, box):
    """`count` quads that miss `box` by >= 1 mm: small ones 1.5 mm .. 5 cm beyond one of its edges, or a car-sized one far away"""
    x0, x1, y0, y1 = box
    out = []
    while len(out) < count:
        if rng.random() < 0.6:
            h, gap = rng.uniform(0.01, 0.03), rng.uniform(1.5e-3, 0.05)
            side = int(rng.integers(4))
            cx = x0 - gap - 1.1 * h if side == 0 else x1 + gap + 1.1 * h if side == 1 else rng.uniform(x0, x1)
            cy = y0 - gap - 1.1 * h if side == 2 else y1 + gap + 1.1 * h if side == 3 else rng.uniform(y0, y1)
            q = np.array([cx, cy]) + np.array([[-1, -1], [1, -1], [1, 1], [-1, 1]], float) * h * rng.uniform(0.95, 1.05, (4, 2))
        else:
            q = T.far_quad(rng, Q[0])
        if near_flags(box, q)[1][0]:
            out.append(q)
    return out


def far_dest(rng, pose):
    a, r = rng.uniform(0, 2 * np.pi), rng.uniform(9.0, 14.0)
    return np.array([pose[0] + r * np.cos(a), pose[1] + r * np.sin(a), rng.uniform(-np.pi, np.pi)])


def arrival_dest(rng, Q, ka):
    """dest such that the first pose whose ratio exceeds 0.95 is pose ka, under the rejection rule of the module docstring, or None"""
    j = int(rng.integers(ka, min(ka + 4, EXT_STEP - 2) + 1)) + 1  # Q index of pose j
    u = rng.random()
    dest = (1 - u) * Q[j] + u * Q[j + 1]
    r = ratios(Q[:NUM_STEP + 1], dest)
    if r[0] > START_RATIO_MAX or (np.abs(r[1:] - ARRIVE_RATIO) < RATIO_BAND).any():
        return None
    over = np.nonzero(r[1:] > ARRIVE_RATIO)[0]
    return dest if len(over) and over[0] == ka else None


def slab_bound(pose, dest):
    """numpy mirror of the device's necessary condition for an arrival (arrival_possible, hope_step_kernel.h): a placement aid -- the
    device test counts with the device's own (hope_debug_geom fn 9)"""
    mid, hl, hw = 0.5 * (T.CAR_XF + T.CAR_XR), 0.5 * (T.CAR_XF - T.CAR_XR), T.CAR_YH
    ct, sn, cd, sd = np.cos(pose[2]), np.sin(pose[2]), np.cos(dest[2]), np.sin(dest[2])
    dx, dy = dest[0] + cd * mid - (pose[0] + ct * mid), dest[1] + sd * mid - (pose[1] + sn * mid)
    cphi, sphi = abs(ct * cd + sn * sd), abs(ct * sd - sn * cd)
    p, q = dx * ct + dy * sn, dy * ct - dx * sn
    hB, wB = hl * cphi + hw * sphi, hl * sphi + hw * cphi
    lov, wov = min(hl, p + hB) - max(-hl, p - hB), min(hw, q + wB) - max(-hw, q - wB)
    return lov >= 0.94 * 2 * hl + 1e-6 and wov >= 0.94 * 2 * hw + 1e-6


def near_miss_dest(rng, Q, k, passing):
    """dest beside pose k (Q index k + 1; k = -1: the start pose), shifted sideways and turned a little: the best ratio of the ten poses
    lies in (0.90, 0.945), the start pose's below 0.945, and pose `passing` (the one a collision cuts off; -1: the start pose) still
    passes the device's slab bound, so that its overlap IS computed -- or None.  (A sideways shift alone passes that bound only with
    a ratio above 0.94: the turn takes the area off the corners, which the bound does not see.)"""
    j = max(k, 0)
    u = rng.random()
    dest = (1 - u) * Q[j] + u * Q[j + 1]
    shift = rng.uniform(0.02, 0.11) * (1 if rng.random() < 0.5 else -1)
    dest[0] -= shift * np.sin(dest[2])
    dest[1] += shift * np.cos(dest[2])
    mid = 0.5 * (T.CAR_XF + T.CAR_XR)                             # the turn is about the box's centre
    cen = dest[:2] + mid * np.array([np.cos(dest[2]), np.sin(dest[2])])
    dest[2] += rng.uniform(0.02, 0.12) * (1 if rng.random() < 0.5 else -1)
    dest[:2] = cen - mid * np.array([np.cos(dest[2]), np.sin(dest[2])])
    if not slab_bound(Q[passing + 1], dest):
        return None
    r = ratios(Q[:NUM_STEP + 1], dest)
    return dest if 0.90 < r[1:].max() < 0.945 and r[0] < 0.945 else None


def make_case(rng, kind, n_near, scale, ka=-1, kc=-1, dest_mode='far', t=None, accum=0.0, edge=None, edge_ulp=False, final=None, tag=None):
    """one case, re-drawn until every requirement holds.  ka / kc: programmed arrival / collision sub-step (-1: none); dest_mode 'far',
    'arrival' (at ka), 'miss' (near miss beside pose kc - 1 / kc); edge 0..3 (xmin, xmax, ymin, ymax) with edge_ulp: the bbox edge on the
    final pose's rear axle / one ulp further in, `final` naming that pose ('walk': pose ka, an arrival outside the bbox)"""
    n_fill = n_near - (1 if kc >= 0 else 0)
    assert n_fill >= 0, (kind, n_near, kc)
    n_cap = max(32, n_near)
    for _round in range(MAX_ROUNDS):
        th = rng.uniform(-np.pi, np.pi)
        if n_fill >= 4 and abs(np.sin(2 * th)) < 0.3:             # room for the fillers in the corners of the hulls' box
            continue
        pose = np.array([rng.uniform(-scale, scale), rng.uniform(-scale, scale), th])
        action = np.array([rng.uniform(-1, 1), rng.uniform(0.4, 1.0) * (1 if rng.random() < 0.5 else -1)])
        Q = extended_poses(pose, action)
        speed = O.action_rescale(action)[1]
        if dest_mode == 'arrival':
            dest = arrival_dest(rng, Q, ka)
        elif dest_mode == 'miss':
            dest = near_miss_dest(rng, Q, kc - 1 if rng.random() < 0.5 else kc, passing=kc if kind == 'K4' else -1)
        else:
            dest = far_dest(rng, pose)
        if dest is None:
            continue
        quads = []
        if kc >= 0:
            hq = hit_quad(rng, Q, kc, speed)
            if hq is None:
                continue
            quads.append(hq)
        box = T.hulls_box(Q[:NUM_STEP + 1])
        fl = fillers(rng, Q, n_fill, box)
        if fl is None:
            continue
        quads += fl
        quads += outside_quads(rng, Q, int(rng.integers(0, min(3, n_cap - len(quads)) + 1)), box)
        quads = [T._ccw(quads[i]) for i in rng.permutation(len(quads))]
        near, far = near_flags(box, quads) if quads else (np.zeros(0, bool), np.zeros(0, bool))
        if not (near | far).all() or int(near.sum()) != n_near:
            continue
        # what the reference does, by construction
        if ka >= 0 and (kc < 0 or ka <= kc):
            substeps, fin, status = ka + 1, ka, ARRIVED
        elif kc >= 0:
            substeps, fin, status = kc, kc - 1, CONTINUE
        else:
            substeps, fin, status = NUM_STEP, NUM_STEP - 1, CONTINUE
        bbox = np.array([np.floor(pose[0] - 30), np.ceil(pose[0] + 30), np.floor(pose[1] - 30), np.ceil(pose[1] + 30)])
        if edge is not None:
            F = Q[fin + 1]
            coord = F[edge // 2]
            inward = np.inf if edge % 2 == 0 else -np.inf         # xmin / ymin move up, xmax / ymax move down
            bbox[edge] = np.nextafter(coord, inward) if edge_ulp else coord
            if edge_ulp and status != ARRIVED:
                status = OUTBOUND
        tt = int(rng.integers(1, 150)) if t is None else int(t)
        if status == CONTINUE and tt + 1 > 200:
            status = OUTTIME
        # every other lot starts elsewhere than the uploaded pose: what the reset left behind (heading, cos / sin) is then not the step's
        start = pose + (rng.uniform(-1, 1, 3) * np.array([2.0, 2.0, 0.6]) if rng.random() < 0.5 else 0.0)
        return dict(kind=kind, tag=tag or kind, ka=ka, kc=kc, n_near=n_near, start=start, pose=pose, dest=dest, bbox=bbox, quads=quads,
                    action=action, t=tt, accum=float(accum), substeps=substeps, final=fin, status=status, edge=-1 if edge is None else edge,
                    edge_ulp=bool(edge_ulp), final_name=final or '', scale=scale, rounds=_round + 1)
    raise AssertionError(f'substep_events: no draw in {MAX_ROUNDS} rounds for {kind} ka={ka} kc={kc} n_near={n_near} dest={dest_mode} edge={edge}')


def cell(c):
    """the table cell a case fills: (kind, sub-step or sub-step pair or variant, near-list length)"""
    k = c['kind']
    sub = (c['ka'], c['kc']) if k == 'K3' else c['ka'] if k == 'K2' else c['kc'] if k in ('K1', 'K4') else c['tag']
    return k, sub, c['n_near']


def required_cells():
    need = set()
    for n in N_NEAR:
        need.add(('K0', 'K0', n))
        for k in range(NUM_STEP):
            need.add(('K2', k, n))
            if n >= 1:
                need.add(('K1', k, n))
        if n >= 1:
            for pair in k3_pairs():
                need.add(('K3', pair, n))
            for far in (False, True):
                need.add(('K7', 'K7 dest ' + ('far' if far else 'over the start pose'), n))
    return need


def k3_pairs():
    near = [(ka, kc) for ka in range(NUM_STEP) for kc in range(NUM_STEP) if abs(ka - kc) <= 1]
    return tuple(near) + FAR_PAIRS


@functools.lru_cache(maxsize=None)
def table(seed=7, replicas=2):
    """the list of cases: every cell `replicas` times with different actions, lots and coordinate scales"""
    rng = np.random.default_rng(seed)
    out, count = [], [0]

    def add(kind, n_near, **kw):
        for _ in range(replicas):
            count[0] += 1
            out.append(make_case(rng, kind, n_near, T.SCALES[count[0] % 3], **kw))

    classes1 = [n for n in N_NEAR if n >= 1]
    rot = [0]

    def some_n(lo=1):                                             # the kinds that do not cross with the near-list length rotate through it
        rot[0] += 1
        return classes1[rot[0] % len(classes1)] if lo else N_NEAR[rot[0] % len(N_NEAR)]

    for n in N_NEAR:
        add('K0', n)
        for k in range(NUM_STEP):
            add('K2', n, ka=k, dest_mode='arrival')
            if n >= 1:
                add('K1', n, kc=k)
        if n >= 1:
            for ka, kc in k3_pairs():
                add('K3', n, ka=ka, kc=kc, dest_mode='arrival')
            add('K7', n, kc=0, tag='K7 dest far')
            add('K7', n, kc=0, dest_mode='miss', accum=0.3, tag='K7 dest over the start pose')
    for kc in range(NUM_STEP):
        for acc in (0.0, 0.3, 0.9):
            add('K4', some_n(), kc=kc, dest_mode='miss', accum=acc)
    for edge in range(4):
        for ulp in (False, True):
            add('K5', some_n(0), edge=edge, edge_ulp=ulp, final='pose 9', tag='K5 pose 9')
            add('K5', some_n(), kc=int(rng.integers(1, NUM_STEP)), edge=edge, edge_ulp=ulp, final='retreat', tag='K5 retreat pose')
            add('K5', some_n(), kc=0, edge=edge, edge_ulp=ulp, final='start', tag='K5 start pose')
        add('K5', some_n(0), ka=int(rng.integers(0, NUM_STEP)), dest_mode='arrival', edge=edge, edge_ulp=True, final='walk', tag='K5 arrival outside')
    for t in (199, 200):
        add('K6', some_n(0), t=t, tag='K6 free run')
        add('K6', some_n(), kc=int(rng.integers(1, NUM_STEP)), t=t, tag='K6 retreat')
        add('K6', some_n(0), ka=int(rng.integers(0, NUM_STEP)), dest_mode='arrival', t=t, tag='K6 arrival')
        add('K6', some_n(0), t=t, edge=int(rng.integers(4)), edge_ulp=True, final='pose 9', tag='K6 outbound')
    for k in (0, 3, 6, 9):                                        # the large-tile class's own: 40 near obstacles
        add('K1', N_NEAR_LARGE, kc=k, tag='K1 large')
        add('K3', N_NEAR_LARGE, ka=k, kc=k, dest_mode='arrival', tag='K3 large')
    add('K0', N_NEAR_LARGE, tag='K0 large')
    missing = required_cells() - {cell(c) for c in out}
    assert not missing, sorted(missing)[:10]
    return out


def event_substep(c):
    """the sub-step at which the walk of a case stops (NUM_STEP: it does not)"""
    return NUM_STEP if c['substeps'] == NUM_STEP and c['status'] != ARRIVED else c['ka'] if c['status'] == ARRIVED else c['kc']


def _pairing_block(tab, rng):
    """indices into the table, two per pair wave of the small-tile chain: all 64 ordered pairs of half classes, then every kind K1-K7
    in either half next to a partner with no event, an earlier event and a later event (K7 stops at sub-step 0: its "earlier" partner
    is another case that stops at sub-step 0)"""
    small = [i for i, c in enumerate(tab) if c['n_near'] <= 32]
    by_cls = {k: [i for i in small if half_class(tab[i]['n_near']) == k] for k in range(len(HALF_CLASSES))}
    pick = lambda lst: lst[int(rng.integers(len(lst)))]
    out = []
    for a in range(len(HALF_CLASSES)):
        for b in range(len(HALF_CLASSES)):
            out += [pick(by_cls[a]), pick(by_cls[b])]
    ev = {i: event_substep(tab[i]) for i in small}
    for kind in KINDS[1:]:
        mine = [i for i in small if tab[i]['kind'] == kind and (kind == 'K7' or 2 <= ev[i] <= 7)]
        for want in ('none', 'earlier', 'later'):
            for order in (0, 1):
                i = pick(mine)
                if want == 'none':
                    partners = [j for j in small if ev[j] == NUM_STEP]
                elif want == 'earlier':
                    partners = [j for j in small if (ev[j] < ev[i] or (kind == 'K7' and ev[j] == 0)) and j != i]
                else:
                    partners = [j for j in small if ev[i] < ev[j] < NUM_STEP]
                j = pick(partners)
                out += [i, j] if order == 0 else [j, i]
    assert len(out) % 2 == 0
    return out


@functools.lru_cache(maxsize=None)
def scene_set(seed=11, perms=3, max_obst=128, cls1_frac=0.42):
    """the table as one batch: a pairing block at the lowest ids (two consecutive ids share a wave of the pair kernels), then `perms`
    permutations of the small lots, then the 40-obstacle lots (the large-tile class by themselves), padded with further table cases to an
    odd count above 4 096 at which the small-tile chain -- the ids below the share `cls1_frac` that the overlapped handle hands to the
    large-tile chain -- is odd too, so that its last pair wave has an empty second half.  -> dict of arrays, `case` [n] table indices"""
    tab = table()
    rng = np.random.default_rng(seed)
    small = np.array([i for i, c in enumerate(tab) if c['n_near'] <= 32])
    large = np.array([i for i, c in enumerate(tab) if c['n_near'] > 32])
    head = _pairing_block(tab, rng) + [int(i) for _ in range(perms) for i in rng.permutation(small)]
    tail = [int(i) for _ in range(perms) for i in rng.permutation(large)]
    n = len(head) + len(tail)
    pad = []
    while n <= 4096 or n % 2 == 0 or int(cls1_frac * n) % 2 == 1:
        pad.append(int(small[int(rng.integers(len(small)))]))
        n += 1
    case = np.array(head + pad + tail, np.int32)
    assert n - int(cls1_frac * n) <= len(head) + len(pad) and len(tail) < int(cls1_frac * n)    # the small-tile chain: ids 0 .. n - int(frac n) - 1
    sc = dict(case=case, start=np.zeros((n, 3)), dest=np.zeros((n, 3)), bbox=np.zeros((n, 4)), verts=np.zeros((n, max_obst, 4, 2)),
              nob=np.zeros(n, np.int32), nvert=np.full((n, max_obst), 4, np.int32), pose=np.zeros((n, 3)), t=np.zeros(n, np.int32),
              accum=np.zeros(n), action=np.zeros((n, 2)))
    for i, k in enumerate(case):
        c = tab[k]
        for key in ('start', 'dest', 'bbox', 'pose', 't', 'accum', 'action'):
            sc[key][i] = c[key]
        sc['nob'][i] = len(c['quads'])
        if c['quads']:
            sc['verts'][i, :len(c['quads'])] = c['quads']
    for key in ('kind', 'ka', 'kc', 'n_near', 'substeps', 'final', 'status'):
        sc[key] = np.array([tab[k][key] for k in case])
    sc['event'] = np.array([event_substep(tab[k]) for k in case])
    sc['half_class'] = np.array([half_class(tab[k]['n_near']) if tab[k]['n_near'] <= 32 else -1 for k in case])
    return sc


def subset(sc, rows):
    """the scenes `rows` of a scene set as a scene set of their own"""
    return {k: v[rows] for k, v in sc.items()}
