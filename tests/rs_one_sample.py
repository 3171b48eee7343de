"""Adversarial scenes for the Reeds-Shepp validation walk (k_rs_validate_f, k_rs_validate, the split form): no RNG.

Random rollouts and the lattice of tests/rs_degenerate.py condemn a word through long runs of colliding samples, so a walk that
drops ONE sample passes them.  Three families on the obstacle-free poses of that lattice:

 (a) one-sample diamonds   a small axis-aligned diamond on the midpoint of a hull edge at a chosen sample of a tested word:
                           is_traj_valid (car_parking_base.py:452-534) is a BOUNDARY test, so the diamond collides with that
                           sample and is wholly inside (or outside) the hull 0.1 m further on.  Kept iff exactly one sample of the
                           word collides (or two adjacent ones) and the search's result changes with the diamond.
 (b) trailing pop          diamonds on the goal hull, where generate_local_course's `while px[-1] == 0.0: pop`
                           (reeds_shepp.py:500-505) removes a sample in use: the reference never tests that sample.
 (c) margins               a 0.6 m square with one edge along a hull side, at signed gaps around the float32 filter's margins.

The walk's pass schedule is restated here in plain Python (`windows`, `walk`), as tests/lidar_adversarial.py restates the lidar's
branch predicates, so that every kept case carries the place in the schedule where the kernel has to see its collision.
tests/golden/rs_one_sample.npz holds the reference's own results (tests/golden/make_golden_r2.py `rsonesample`); the cases are
rebuilt from here.
"""
import math

import numpy as np

import rs_degenerate as D
from hope_amd import tables as T
from oracle import oracle as O

MAXC = D.MAXC
STEP = 0.1 * MAXC                                # step_size * maxc (reeds_shepp.py:44; RS_STEP * MAXC in hope_rs.hip)
WAVE, WIN, TAB = 64, 128, 256                    # lanes, window of the sample queue, first-segment sample table (hope_rs.hip)
FEPS, FKAPPA, FETA_HULL = 1e-3, 2e-2, 2e-3       # margins of the float32 filter (hope_rs.hip)
H_DIAMOND = 0.02                                 # half diagonal (m)
H_POP = (0.02, 0.002)
CAR = np.asarray(T.VEHICLE_BOX, dtype=np.float64)
GAPS = (1e-9, 1e-6, 2e-4, 9e-4, 1.1e-3, 3e-3)
POSE_STRIDE = 7                                  # family (a): every 7th obstacle-free lattice pose


# ------------------------------------------------------------------------------------------------ geometry
def hull(traj):
    """car outline at every pose: [T, 4, 2] (car_parking_base.py:468-471)"""
    t = np.atleast_2d(np.asarray(traj, dtype=np.float64))
    c, s = np.cos(t[:, 2])[:, None], np.sin(t[:, 2])[:, None]
    return np.stack([c * CAR[:, 0] - s * CAR[:, 1] + t[:, :1], s * CAR[:, 0] + c * CAR[:, 1] + t[:, 1:2]], axis=-1)


def sample_hits(traj, rings):
    """is_traj_valid's edge test per sample in numpy (:477-526): True where the hull at the sample meets a ring edge.  A fast
    pre-screen; the verdicts that decide whether a case is kept come from the oracle (`oracle_hits`)."""
    hv = hull(traj)
    x1, y1 = hv[:, :, 0], hv[:, :, 1]
    x2, y2 = np.roll(x1, -1, axis=1), np.roll(y1, -1, axis=1)
    a, b, c = y2 - y1, x1 - x2, y1 * x2 - x1 * y2
    vx0, vx1, vy0, vy1 = np.minimum(x1, x2), np.maximum(x1, x2), np.minimum(y1, y2), np.maximum(y1, y2)
    bad = np.zeros(len(hv), bool)
    with np.errstate(divide='ignore', invalid='ignore'):
        for ring in rings:
            for j in range(len(ring)):
                (p1, q1), (p2, q2) = ring[j], ring[(j + 1) % len(ring)]
                d, e, f = q2 - q1, p1 - p2, q1 * p2 - p1 * q2
                det = a * e - b * d
                rx, ry = (b * f - c * e) / det, (c * d - a * f) / det
                ok = ((det != 0) & (rx <= max(p1, p2)) & (rx >= min(p1, p2)) & (rx <= vx1) & (rx >= vx0)
                      & (ry <= max(q1, q2)) & (ry >= min(q1, q2)) & (ry <= vy1) & (ry >= vy0))
                bad |= ok.any(axis=1)
    return bad


def oracle_hits(traj, rings, bbox):
    """single-sample is_traj_valid of the oracle, per sample"""
    v = np.asarray(rings, dtype=np.float64).reshape(-1, 4, 2)
    nv = np.full(len(v), 4, np.int32)
    return np.array([not O.is_traj_valid(traj[k:k + 1], v, nv, bbox) for k in range(len(traj))])


def diamond(c, h):
    return np.array([(c[0] + h, c[1]), (c[0], c[1] + h), (c[0] - h, c[1]), (c[0], c[1] - h)])


def edge_mid(pose, e):
    hv = hull(pose)[0]
    return 0.5 * (hv[e] + hv[(e + 1) % 4])


# ------------------------------------------------------------------------------------------------ the reference's course
def course(lens):
    """generate_local_course (:452-507) for the scaled lengths of a word: (pd, segment) of every sample in use, before the trailing
    pop.  Sample 0 is the start pose, segment ends are overwritten by the next segment's first sample, the last one stays."""
    pds, segs = [0.0], [0]
    ll = 0.0
    for i, l in enumerate(lens):
        d = STEP if l > 0.0 else -STEP
        pd = (-d - ll) if (i >= 1 and lens[i - 1] * l > 0) else (d - ll)
        while abs(pd) <= abs(l):
            pds.append(pd)
            segs.append(i)
            pd += d
        ll = l - pd - d
    pds.append(lens[-1])
    segs.append(len(lens) - 1)
    return pds, segs


def pop_order(keys):
    """heapdict 1.0.1 as find_rs_path uses it (:432-443): push in path order (sift-up swaps unless parent < child), popitem with a
    strict sift-down, until the stop rule.  Returns the path indices the search may test, in order."""
    pr, ids = [], []
    for i, k in enumerate(keys):
        pr.append(float(k))
        ids.append(i)
        j = len(pr) - 1
        while j:
            p = (j - 1) >> 1
            if pr[p] < pr[j]:
                break
            pr[p], pr[j], ids[p], ids[j] = pr[j], pr[p], ids[j], ids[p]
            j = p
    out, lmin = [], None
    while pr:
        top, key = ids[0], pr[0]
        if lmin is None:
            lmin = key
        if key > 1.6 * lmin and len(out) + 1 > 2:
            break
        out.append(top)
        last_p, last_i = pr.pop(), ids.pop()
        if pr:
            pr[0], ids[0] = last_p, last_i
            j, n = 0, len(pr)
            while True:
                l, r = 2 * j + 1, 2 * j + 2
                low = l if (l < n and pr[l] < pr[j]) else j
                if r < n and pr[r] < pr[low]:
                    low = r
                if low == j:
                    break
                pr[j], pr[low], ids[j], ids[low] = pr[low], pr[j], ids[low], ids[j]
                j = low
    return out


def words_of(pose, goal, depth=4):
    """the first `depth` words the search tests, in pop order: samples as the reference tests them (after its pop), the restated
    (pd, segment) labels, the number of samples in use that the pop removed"""
    a = O.rs_all_paths(pose, goal, MAXC)
    try:
        O.rs_pop_mode(True)
        tail = O.rs_all_paths(pose, goal, MAXC)
    finally:
        O.rs_pop_mode(False)
    out = []
    for pi in pop_order(a['L'])[:depth]:
        nseg = int(a['nseg'][pi])
        lens = [float(x) * MAXC for x in a['lengths'][pi, :nseg]]
        pds, segs = course(lens)
        traj = O.rs_path_samples(pose, goal, MAXC, int(pi))
        out.append(dict(pi=int(pi), types=tuple(int(t) for t in a['ctypes'][pi, :nseg]), lens=lens, pds=np.array(pds),
                        segs=np.array(segs), traj=traj, n_pop=int(tail['npts'][pi]) - len(traj),
                        restated=len(pds) == int(tail['npts'][pi]), cls=(int(a['ctypes'][pi, 0]), lens[0] > 0.0),
                        len0=abs(lens[0])))
    return out


# ------------------------------------------------------------------------------------------------ the kernels' schedule
def windows(segs, n_pop):
    """The pass schedule of a word's walk (hope_rs.hip, both validation kernels).  `segs`: segment of every sample in use, in path
    order (course()).  The generator appends chunks of at most 64 samples of one segment while fewer than 64 are queued (nq + 65
    <= 128); the final sample joins the chunk that ends the last segment; the trailing pop then takes `n_pop` samples off the end.
    While the word goes on only whole waves are tested (n = nq & ~63) and the rest is carried to the front of the next window.
    A window of n samples is tested in rounds of 64 lanes: stride = ceil(n / 64); coarse round: lane -> stride * lane; rest rounds:
    r -> r + (r if stride == 2 else r >> 1) + 1.  Returns one dict per window: `samples` (indices into the word's samples),
    `stride`, `rounds` (per round the sample of every active lane), `carried` (how many of its samples came from the last window).
    n_all <= 63 + 63 + 1 = 127 when the word ends and 64 <= n_all <= 127 before, so n <= 127 and stride is 1 or 2: the kernel's
    third stride (n > 128) cannot occur with the 128-entry window."""
    total = len(segs)
    nseg = int(segs[-1]) + 1
    counts = [int(((np.asarray(segs[1:total - 1])) == i).sum()) for i in range(nseg)]
    queue, g, i, left, finished, carried, out = [0], 1, 0, counts[0], False, 0, []
    while not finished or queue:
        while not finished and len(queue) + WAVE + 1 <= WIN:
            take = min(left, WAVE)
            queue += list(range(g, g + take))
            g += take
            left -= take
            if take < WAVE:                                   # the first value outside the segment is among the 64: segment done
                if i == nseg - 1:
                    queue.append(g)
                    g += 1
                    finished = True
                i += 1
                if i < nseg:
                    left = counts[i]
        if finished:
            assert n_pop <= len(queue), 'the pop reaches back beyond the last window'
            queue = queue[:len(queue) - n_pop]
        n_all = len(queue)
        n = n_all if finished else n_all & ~(WAVE - 1)
        stride = (n + WAVE - 1) >> 6
        assert stride <= 2
        n_coarse = n if stride <= 1 else (n + 1) >> 1
        n_rest = n - n_coarse
        rounds = [[queue[stride * lane] for lane in range(n_coarse)]]
        rnd = 1
        while (rnd - 1) * WAVE < n_rest:
            rs = [(rnd - 1) * WAVE + lane for lane in range(WAVE)]
            rounds.append([queue[r + (r if stride == 2 else r >> 1) + 1] for r in rs if r < n_rest])
            rnd += 1
        out.append(dict(samples=queue[:n], stride=stride, rounds=rounds, carried=carried))
        queue = queue[n:]
        carried = len(queue)
    assert g == total
    return out


def walk(words, hits):
    """find_rs_path's loop as the kernels run it: words in pop order, `hits[k]` the colliding samples of word k.  Returns (index of
    the found word or -1, events): per walked word the place where the walk sees its first collision -- window, stride, round, lanes,
    samples -- or None for a clean word; 'bad1' for a word skipped through the first-segment cache."""
    bad1 = {}
    events = []
    for k, w in enumerate(words):
        lim = bad1.get(w['cls'], math.inf)
        if lim > 0.0 and w['len0'] >= lim:
            events.append(dict(kind='bad1', equal=w['len0'] == lim))
            continue
        h = np.zeros(len(w['pds']), bool)
        h[:len(hits[k])] = hits[k]                            # (popped samples are never tested)
        ev = None
        for wi, win in enumerate(windows(w['segs'], w['n_pop'])):
            for ri, lanes in enumerate(win['rounds']):
                bad = [(lane, s) for lane, s in enumerate(lanes) if h[s]]
                if bad:
                    ev = dict(kind='hit', window=wi, stride=win['stride'], round=ri, lanes=[b[0] for b in bad],
                              samples=[b[1] for b in bad], carried=[b[1] in win['samples'][:win['carried']] for b in bad])
                    first = [abs(float(w['pds'][s])) for _, s in bad if w['segs'][s] == 0 and s < len(w['pds']) - 1]
                    if first:
                        v = min(lim, min(first))
                        bad1[w['cls']] = min(bad1.get(w['cls'], math.inf), v)
                        if v == 0.0:
                            for c in [(t, f) for t in (0, 1, 2) for f in (False, True)]:
                                bad1[c] = 0.0
                    break
            if ev:
                break
        events.append(ev)
        if ev is None:
            return k, events
    return -1, events


def labels(w, event):
    """schedule categories of a walk event on word w"""
    out = set()
    n = len(w['pds'])
    segs = w['segs']
    for lane, s, car in zip(event['lanes'], event['samples'], event['carried']):
        out.add(f'stride{event["stride"]}')
        out.add('coarse' if event['round'] == 0 else 'rest')
        if lane in (0, 63):
            out.add(f'{"coarse" if event["round"] == 0 else "rest"}_lane{lane}')
        if car:
            out.add('carried')
        if s == 0:
            out.add('sample0')
        elif s == n - 1:
            out.add('final')
        else:
            i = int(segs[s])
            inner = np.nonzero(segs[1:n - 1] == i)[0] + 1
            if s == inner[0]:
                out.add(f'seg{i}_first')
            if s == inner[-1]:
                out.add(f'seg{i}_last')
        if event['window'] > 0:
            out.add('later_window')
    return out


# ------------------------------------------------------------------------------------------------ lattice poses
_free = None


def free_poses():
    """the obstacle-free lattice cases that the step's gate lets through and that are neither arrived nor out of the map"""
    global _free
    if _free is None:
        cs = [c for c in D.cases() if c['variant'] == D.VARIANT_NONE and not c['gate']
              and D.gate_distance(c['pose'], c['goal']) < 10.0]
        n = len(cs)
        orc = O.BatchOracle(n, 1, track_traj=False)
        z = np.zeros((n, 1, 4, 2))
        orc.set_scenes(np.arange(n), np.array([c['pose'] for c in cs]), np.array([c['goal'] for c in cs]),
                       np.array([c['bbox'] for c in cs]), z, np.full((n, 1), 4, np.int32), np.zeros(n, np.int32))
        orc.t[:] = 1
        st = orc.reset_obs(with_rs=False)['status'].copy()
        _free = [c for c, s in zip(cs, st) if s == 1 and not reference_overflows(c['pose'], c['goal'])]
    return _free


def reference_overflows(pose, goal):
    """generate_local_course sizes its lists int(L / step) + len(lengths) + 3 (:453); a word that opens with zero-length segments
    writes past them and the reference raises IndexError while it builds the candidates (tests/test_rs_degenerate.py, `ref_error`):
    such a pose has no reference result"""
    try:
        O.rs_pop_mode(True)
        a = O.rs_all_paths(pose, goal, MAXC)
    finally:
        O.rs_pop_mode(False)
    return any(int(a['npts'][k]) > int(a['L'][k] * MAXC / STEP) + int(a['nseg'][k]) + 3 for k in range(a['n']))


def result_key(r):
    return (r['found'], r['n_tested'], tuple(int(c) for c in r['ctypes']), tuple(float(x) for x in r['lengths']))


def search(pose, goal, rings, bbox):
    v = np.asarray(rings, dtype=np.float64).reshape(-1, 4, 2)
    return O.find_rs_path(pose, goal, v, np.full(len(v), 4, np.int32), bbox)


def libm_independent(r, pose, goal, rings, bbox):
    """does the oracle's glibc build (the reference's arithmetic) return the result r of its hope_math build (the kernels')?  With the
    heading exactly reversed four words tie in length, and a hull that is exactly axis-parallel meets an edge only by bit-equality
    (tests/rs_illcond.py): which word such a search finds is libm noise, and a diamond placed on one build's word misses the
    other's.  Those placements are not kept."""
    try:
        O.use_libm(True)
        q = search(pose, goal, rings, bbox)
    finally:
        O.use_libm(False)
    return (r['found'] == q['found'] and r['n_tested'] == q['n_tested'] and np.array_equal(r['ctypes'], q['ctypes'])
            and np.array_equal(r['npts'], q['npts']) and np.abs(r['lengths'] - q['lengths']).max() < 1e-9)


def _targets(w):
    """sample indices of word w that cover the schedule: sample 0, the final sample, the first and last sample of every segment,
    and per window the first and last lane of every round and the carried samples' ends"""
    n = len(w['traj'])
    t = {0, n - 1}
    segs = w['segs']
    for i in range(int(segs[-1]) + 1):
        inner = np.nonzero(segs[1:len(segs) - 1] == i)[0] + 1
        if len(inner):
            t |= {int(inner[0]), int(inner[-1])}
    for win in windows(segs, w['n_pop']):
        for lanes in win['rounds']:
            if lanes:
                t |= {lanes[0], lanes[-1]}
        if win['carried']:
            t |= {win['samples'][0], win['samples'][win['carried'] - 1]}
    return sorted(s for s in t if s < n)


def _condemn(w, keep_clear, start_box):
    """a diamond that collides with word w, with none of the words in keep_clear and not with the car at the start"""
    n = len(w['traj'])
    for s in (n // 2, n // 3, (2 * n) // 3, n - 1, n // 4):
        for e in range(4):
            ring = diamond(edge_mid(w['traj'][s], e), H_DIAMOND)
            if D.convex_overlap(ring, start_box) or not sample_hits(w['traj'], [ring]).any():
                continue
            if any(sample_hits(o['traj'], [ring]).any() for o in keep_clear):
                continue
            return ring
    return None


def family_a():
    """one-sample diamonds.  Depth 0 on every POSE_STRIDE-th free pose, depths 1 and 2 (earlier words condemned by a diamond of
    their own) on every third of those.  Returns (cases, stats)."""
    out = []
    stats = dict(placements=0, one=0, two=0, changed=0, libm_noise=0, not_restated=0)
    poses = free_poses()[::POSE_STRIDE]
    for pk, c in enumerate(poses):
        pose, goal, bbox = c['pose'], c['goal'], c['bbox']
        ws = words_of(pose, goal, depth=40)
        if not all(w['restated'] for w in ws):
            stats['not_restated'] += 1
            continue
        start_box = D.car_box(pose)
        for depth in ((0, 1, 2) if pk % 3 == 0 else (0,)):
            if depth >= len(ws):
                break
            tw = ws[depth]
            pre = []
            for j in range(depth):
                ring = _condemn(ws[j], [tw], start_box)
                if ring is None:
                    break
                pre.append(ring)
            if len(pre) < depth:
                continue
            base = search(pose, goal, pre, bbox)
            for s in _targets(tw):
                for e in range(4):
                    ring = diamond(edge_mid(tw['traj'][s], e), H_DIAMOND)
                    if s > 0 and D.convex_overlap(ring, start_box):
                        continue
                    stats['placements'] += 1
                    rings = pre + [ring]
                    h = np.nonzero(sample_hits(tw['traj'], rings))[0]
                    if not (len(h) == 1 or (len(h) == 2 and h[1] == h[0] + 1)):
                        continue
                    ho = np.nonzero(oracle_hits(tw['traj'], rings, bbox))[0]
                    if not (len(ho) == 1 or (len(ho) == 2 and ho[1] == ho[0] + 1)):
                        continue
                    stats['one' if len(ho) == 1 else 'two'] += 1
                    r = search(pose, goal, rings, bbox)
                    if result_key(r) == result_key(base):
                        continue
                    stats['changed'] += 1
                    if not libm_independent(r, pose, goal, rings, bbox):
                        stats['libm_noise'] += 1
                        continue
                    hits = [sample_hits(w['traj'], rings) for w in ws]
                    hits[depth] = np.isin(np.arange(len(tw['traj'])), ho)
                    found, events = walk(ws, hits)
                    out.append(dict(family='a', pose=pose, goal=goal, bbox=bbox, rings=rings, depth=depth, n_hit=len(ho),
                                    target=s, edge=e, walk_found=found, events=events, words=ws, result=r,
                                    host_only=bool(s == 0)))
    return out, stats


def family_b():
    """trailing pop: diamonds of half diagonal 0.02 and 0.002 m on the four edge midpoints of the goal hull, for every free pose with
    a tested word whose last sample(s) the reference pops.  `differs`: the reference's form and the tail-only form of the oracle
    (orc_rs_pop_mode) return different results.  Returns (cases, stats)."""
    out = []
    stats = dict(poses=0, placements=0, libm_noise=0, differ=0, max_popped=0, pop_hist={})
    for c in free_poses():
        pose, goal, bbox = c['pose'], c['goal'], c['bbox']
        ws = words_of(pose, goal, depth=40)
        for w in ws:
            stats['pop_hist'][w['n_pop']] = stats['pop_hist'].get(w['n_pop'], 0) + 1
        if not any(w['n_pop'] > 0 and w['restated'] for w in ws):
            continue
        stats['poses'] += 1
        stats['max_popped'] = max(stats['max_popped'], max(w['n_pop'] for w in ws))
        for w in ws:                                          # (windows() asserts that the pop stays inside the word's last window)
            if w['restated']:
                windows(w['segs'], w['n_pop'])
        start_box = D.car_box(pose)
        for h in H_POP:
            for e in range(4):
                ring = diamond(edge_mid(goal, e), h)
                if D.convex_overlap(ring, start_box):
                    continue
                stats['placements'] += 1
                r = search(pose, goal, [ring], bbox)
                if not libm_independent(r, pose, goal, [ring], bbox):
                    stats['libm_noise'] += 1
                    continue
                try:
                    O.rs_pop_mode(True)
                    rt = search(pose, goal, [ring], bbox)
                finally:
                    O.rs_pop_mode(False)
                differs = result_key(r) != result_key(rt)
                stats['differ'] += differs
                out.append(dict(family='b', pose=pose, goal=goal, bbox=bbox, rings=[ring], h=h, edge=e, differs=differs, result=r,
                                host_only=False))
    return out, stats


# ------------------------------------------------------------------------------------------------ family (c): margins
C_YAWS = (0.0, math.pi / 2, 0.3, 0.5 * FETA_HULL, 2 * FETA_HULL)
C_SINES = (0.0, 0.5 * FKAPPA, 0.95 * FKAPPA, 1.05 * FKAPPA, 2 * FKAPPA)
SIGNED_GAPS = tuple(s * g for g in GAPS for s in (1.0, -1.0))
FRONT_GAPS = tuple(s * g for g in (1e-6, 1.2e-5, 2e-5) for s in (1.0, -1.0))
XR, XF, HW = float(CAR[0, 0]), float(CAR[1, 0]), float(CAR[2, 1])
SIDES = {'left': ((0.5 * (XF + XR), HW), (1.0, 0.0), (0.0, 1.0)), 'front': ((XF, 0.0), (0.0, 1.0), (1.0, 0.0))}   # point, along, outward


def to_world(pose, pts):
    c, s = math.cos(pose[2]), math.sin(pose[2])
    p = np.asarray(pts, dtype=np.float64)
    return np.stack([c * p[:, 0] - s * p[:, 1] + pose[0], s * p[:, 0] + c * p[:, 1] + pose[1]], axis=-1)


def beside(pose, m, t, n, gap, sine, length=D.SQUARE, back=0.0):
    """a rectangle `length` x 0.6 m beside the hull at `pose`: its near edge starts `back` behind the point m of a hull side (car
    frame; t along the side, n outwards), passes m at the signed distance `gap` outside the side (negative: inside the hull) and is
    turned against the side by asin(sine) -- positive: away from the hull in the direction t, negative: into it; the rest of the
    rectangle lies on the outer side of that edge"""
    m, t, n = np.asarray(m), np.asarray(t), np.asarray(n)
    co = math.sqrt(1.0 - sine * sine)
    u, up = co * t + sine * n, -sine * t + co * n
    v0 = m + gap * n - back * u
    return to_world(pose, [v0, v0 + length * u, v0 + length * u + D.SQUARE * up, v0 + D.SQUARE * up])


def _mid_sample(w, straight):
    """index of the middle sample of the longest straight (type 0) or curved segment of word w, or None"""
    best, arg = 0, None
    n = len(w['pds'])
    for i, ty in enumerate(w['types']):
        if (ty == 0) != straight:
            continue
        inner = np.nonzero(w['segs'][1:n - 1] == i)[0] + 1
        if len(inner) > best:
            best, arg = len(inner), int(inner[len(inner) // 2])
    return arg if arg is not None and arg < len(w['traj']) else None


WALL_CORNER_SINE = 0.0225                        # > FKAPPA (|sin| + |cos|): the angle itself is no reason to hesitate


def family_c():
    """margins of the float32 filter.  Every case names the pose it was built on (`at`) and the signed `gap` (positive: apart).
    kinds: `square` / `corner` / `box` are the sign-flip cases (the verdict on `at` is a collision iff gap < 0); `wall` and
    `corner_wall` always collide and exist for the filter's reasons to hesitate: an undecided pass is one WITHOUT a certain hit, and
    a 0.6 m square that pokes a vertex into the hull far enough for a certain crossing (> FEPS) always crosses a second time, at a
    steep angle and away from the corners -- a certain hit.  A shallow or corner crossing with nothing certain beside it needs an
    edge that passes through the whole hull, and a path whose other samples stay clear of it: both walls stand at the goal pose."""
    out = []

    def add(pose, goal, bbox, ring, **kw):
        if ring is not None and D.convex_overlap(ring, D.car_box(pose)):
            return
        out.append(dict(family='c', pose=pose, goal=goal, bbox=bbox, rings=[ring] if ring is not None else [], host_only=False, **kw))
    for gyaw in C_YAWS:
        goal = np.array([D.GOAL_XY[0], D.GOAL_XY[1], gyaw])
        bbox = D.map_box(goal)
        dx, dy = D.rotate(gyaw, -4.0, -3.0)
        bx, by = D.rotate(gyaw, -6.35, 0.0)             # (6.35: the last lattice sample of the straight run is 0.05 m before the goal)
        starts = {'behind': np.array([goal[0] + bx, goal[1] + by, gyaw]), 'oblique': np.array([goal[0] + dx, goal[1] + dy, gyaw + 0.5])}
        for sname, pose in starts.items():
            w = words_of(pose, goal, depth=1)[0]
            for straight in (True, False):
                s = _mid_sample(w, straight)
                if s is None:
                    continue
                at = w['traj'][s]
                for gap in SIGNED_GAPS:
                    for sine in C_SINES:
                        for side in (('left', 'front') if sine == 0.0 else ('left',)):
                            m, t, n = SIDES[side]
                            add(pose, goal, bbox, beside(at, m, t, n, gap, sine), kind='square', start=sname, straight=straight,
                                at=at, gap=gap, sine=sine, side=side)
                    # one vertex within FEPS of the line through a hull corner: the square's near vertex 0.5 FEPS along the side from
                    # the front left corner, before and beyond it
                    for delta in (-0.5 * FEPS, 0.5 * FEPS):
                        add(pose, goal, bbox, beside(at, (XF + delta, HW), (-1.0, 0.0), (0.0, 1.0), gap, 0.0), kind='corner',
                            start=sname, straight=straight, at=at, gap=gap, sine=0.0, side='left', delta=delta)
            if sname == 'oblique':
                # the float32 pose is worst at the front of the hull on an arc (native sine / cosine: 4e-6 x 3 m on the position and
                # x 3.9 m lever arm on the heading in the error budget): squares before the front side at every third sample of
                # the word's arcs, at gaps two orders below FEPS.  (Measured in self-check mode with FEPS = 1e-5 instead of 1e-3:
                # still no contradicted verdict, so the float32 error on these scenes stays below 1e-5 m.)
                n_s = len(w['pds'])
                for s in range(1, min(n_s - 1, len(w['traj'])), 3):
                    if w['types'][int(w['segs'][s])] == 0:
                        continue
                    for gap in FRONT_GAPS:
                        add(pose, goal, bbox, beside(w['traj'][s], (XF, 0.3), (0.0, 1.0), (1.0, 0.0), gap, 0.0), kind='front_arc',
                            start=sname, straight=False, at=w['traj'][s], gap=gap, sine=0.0, side='front')
            for gap in SIGNED_GAPS:
                # wall along the left side of the goal hull: 4 m behind its middle the near edge is outside, it passes the middle at
                # `gap` and dips into the hull at the given sine: ONE edge that crosses the left side at a shallow angle and leaves
                # through the front; every earlier sample's hull meets it the same way or not at all
                for sine in C_SINES[1:]:
                    m, t, n = SIDES['left']
                    add(pose, goal, bbox, beside(goal, m, t, n, gap, -sine, length=8.0, back=4.0), kind='wall', start=sname,
                        straight=None, at=goal, gap=gap, sine=-sine, side='left')
                # wall across the front left corner of the goal hull: the near edge runs through the corner (at `gap`) at 1.3 degrees
                # to the front side and leaves through the right side 0.044 m behind the front, ahead of every earlier sample's
                # hull: one edge, two crossings, one of them at a corner
                add(pose, goal, bbox, beside(goal, (XF, HW), (0.0, -1.0), (1.0, 0.0), gap, -WALL_CORNER_SINE, length=8.0, back=4.0),
                    kind='corner_wall', start=sname, straight=None, at=goal, gap=gap, sine=-WALL_CORNER_SINE, side='front')
        # one sample within FEPS of the map box: the goal pose (every word's last sample) at the signed gap inside the box side that
        # lies beyond it as seen from the start
        pose0 = starts['oblique']
        for gap in SIGNED_GAPS:
            for axis in (0, 1):
                hi = pose0[axis] < goal[axis]
                bb = bbox.copy()
                bb[2 * axis + hi] = goal[axis] + (10.0 if hi else -10.0)       # an integer: goal = (40, 25)
                g2, p2 = goal.copy(), pose0.copy()
                shift = (10.0 - gap) if hi else -(10.0 - gap)
                g2[axis] += shift
                p2[axis] += shift
                add(p2, g2, bb, None, kind='box', start='oblique', straight=None, at=g2, gap=gap, sine=0.0, side=None, axis=axis)
    return out


# ------------------------------------------------------------------------------------------------ packed arrays
A_KEEP_EVERY = 2                                 # family (a) is subsampled evenly: the GPU test holds every case in one handle
_cases = None


def cases():
    """(list of cases: family (a) subsampled, (b), (c); stats of (a) and (b)), computed once"""
    global _cases
    if _cases is None:
        a, sa = family_a()
        b, sb = family_b()
        _cases = (a[::A_KEEP_EVERY] + b + family_c(), dict(a=sa, b=sb, a_all=len(a)))
    return _cases


def build(max_obst=32):
    """packed arrays in pack_scenes' layout (start = the pose), t = 2 everywhere (the step's gate needs t > 1)"""
    cs, _ = cases()
    n = len(cs)
    start, dest, bbox = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((n, 4))
    verts = np.zeros((n, max_obst, 4, 2))
    n_obst = np.zeros(n, np.int32)
    for i, c in enumerate(cs):
        start[i], dest[i], bbox[i] = c['pose'], c['goal'], c['bbox']
        n_obst[i] = len(c['rings'])
        for j, r in enumerate(c['rings']):
            verts[i, j] = r
    return dict(n=n, start=start, dest=dest, bbox=bbox, verts=verts, n_obst=n_obst, nvert=np.full((n, max_obst), 4, np.int32),
                family=np.array([c['family'] for c in cs]), t=np.full(n, 2, np.int32))
