"""-m gpu: the device's exact collision path, its two polygon clips and its arrival bound against exact arithmetic.

On generated lots and rollouts the orientation FILTER decides every (hull edge, obstacle edge) pair
(test_tie_census_no_decision_of_the_geos_slice_comes_near_a_tie), so the code behind it -- orient_exact_lds, orient_robust_lds,
hull_edge_intersect_robust (hope_amd/csrc/hope_dev.h) and the one-lane-at-a-time loops around them in k_env_step / k_motion_pair
-- is reached by no other test.  Two layers:

  primitives  hope_debug_geom (include/hope_env.h) runs the shipped inline functions on packed cases, in the step kernels' calling
              pattern; they must equal the CPU oracle on every case and `fractions.Fraction` on a fixed-stride sample (the
              generators and exact predicates are those of tests/test_oracle_exact_geometry.py, tests/exact_geometry.py).
  scenes      tests/touching_scenes.py puts obstacles against the hull, at the start pose or at a sub-step of a moving step; the
              premise (scenes that reach "undecided, no certain hit", split of the exact answers) is asserted on the CPU first, then
              every launch form of the step must equal the oracle with tolerance 0.

A mismatch in the first layer names the primitive, one in the second layer only names the loop around it."""
import ctypes as C
import functools
import math
import os

import numpy as np
import pytest

import exact_geometry as E
import touching_scenes as T

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

INT_FNS = (0, 1, 2, 3, 4, 5, 9)
CONTINUE, COLLIDED = 1, 3


def geom(fn, cases, n_obst=0, n=None):
    """hope_debug_geom on the rows of `cases` -> int32 / float64 array (fn 5: [n][2])"""
    from hope_amd import _lib as L
    cases = np.ascontiguousarray(cases, np.float64)
    n = len(cases) if n is None else n
    a = torch.from_numpy(cases).cuda()
    per = 2 if fn == 5 else 1
    out = torch.full((max(n, 1) * per,), -77, dtype=torch.int32 if fn in INT_FNS else torch.float64, device='cuda')
    L.check(L.load_library().hope_debug_geom(fn, n, n_obst, C.c_void_p(a.data_ptr()), C.c_void_p(out.data_ptr()), None), 'hope_debug_geom')
    torch.cuda.synchronize()
    r = out.cpu().numpy()[:n * per]
    return r.reshape(n, 2) if fn == 5 else r


def _cs(h):
    from oracle import oracle as O
    return float(O.math_fn(1, [h])[0]), float(O.math_fn(0, [h])[0])


# ---- layer 1: orientation and segment predicates ----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def predicate_cases():
    """the segment pairs (both seeds of adversarial_segments + touching_segments), the orientation triples (the 40 k of the CPU
    test + the four orientations of every pair), the oracle's answers on all of them and the exact ones on a fixed-stride sample"""
    from oracle import oracle as O
    segs = [np.array([[*p1, *p2, *q1, *q2] for p1, p2, q1, q2 in E.adversarial_segments(np.random.default_rng(s), 50000)]) for s in (0, 1)]
    segs.append(np.array([[*p1, *p2, *q1, *q2] for p1, p2, q1, q2 in E.touching_segments(np.random.default_rng(11), 40000)]))
    S = np.concatenate(segs)
    tri = np.array([[*a, *b, *c] for a, b, c in E.orientation_triples(np.random.default_rng(5), 40000)])
    Tr = np.concatenate([tri, S[:, [0, 1, 2, 3, 4, 5]], S[:, [0, 1, 2, 3, 6, 7]], S[:, [4, 5, 6, 7, 0, 1]], S[:, [4, 5, 6, 7, 2, 3]]])
    lib = O.lib()
    lib.orc_segments_intersect.argtypes = [C.c_double] * 8
    lib.orc_orient.argtypes = [C.c_double] * 6
    seg_orc = np.array([lib.orc_segments_intersect(*r) for r in S.tolist()], np.int32)
    tri_orc = np.array([lib.orc_orient(*r) for r in Tr.tolist()], np.int32)
    seg_idx = np.arange(0, len(S), len(S) // 19000)                                  # <= 2 x 10^4 exact evaluations per function
    tri_idx = np.arange(0, len(Tr), len(Tr) // 19000)
    seg_exact = np.array([E.seg_intersect_exact(r[0:2], r[2:4], r[4:6], r[6:8]) for r in S[seg_idx]], np.int32)
    tri_exact = np.array([E.orient_exact(E.F(r[0:2]), E.F(r[2:4]), E.F(r[4:6])) for r in Tr[tri_idx]], np.int32)
    assert len(seg_idx) <= 20000 and len(tri_idx) <= 20000
    assert np.array_equal(seg_orc[seg_idx], seg_exact) and np.array_equal(tri_orc[tri_idx], tri_exact)      # (the CPU file's claim)
    return dict(S=S, Tr=Tr, seg_orc=seg_orc, tri_orc=tri_orc, seg_idx=seg_idx, tri_idx=tri_idx, seg_exact=seg_exact, tri_exact=tri_exact)


def test_orient_filter_abstains_but_never_lies():
    """fn 0: where the filter gives a sign it is the oracle's (= the exact one, on the sample); it abstains on >= 10 000 cases, the
    same ones as the numpy mirror that the scene tests' premise is computed with"""
    c = predicate_cases()
    got = geom(0, c['Tr'])
    und = got == E.UNDECIDED
    assert np.array_equal(got[~und], c['tri_orc'][~und])
    s = c['tri_idx']
    assert np.array_equal(got[s][~und[s]], c['tri_exact'][~und[s]])
    assert np.array_equal(got, E.orient_filter_np(*c['Tr'].T))
    print(f'fn 0 orient_filter: {len(got)} cases, undecided {int(und.sum())}; exact sample {len(s)}, undecided in it {int(und[s].sum())}')
    assert und.sum() >= 10000


@pytest.mark.parametrize('fn', [1, 2])
def test_orientation_expansion_is_the_exact_sign(fn):
    """fn 1 (the expansion on EVERY case, also where the filter would have decided: generic input, the 1e4 offsets) and fn 2 (filter,
    then expansion) equal the oracle everywhere and the exact sign on the sample; 64 cases per block pass through the one LDS
    work area one after the other"""
    c = predicate_cases()
    got = geom(fn, c['Tr'])
    bad = np.nonzero(got != c['tri_orc'])[0]
    assert len(bad) == 0, (fn, len(bad), bad[:5], c['Tr'][bad[:3]], got[bad[:3]], c['tri_orc'][bad[:3]])
    assert np.array_equal(got[c['tri_idx']], c['tri_exact'])
    zero = int((got == 0).sum())
    print(f'fn {fn}: {len(got)} cases, exactly collinear {zero}')
    assert zero > 10000
    for n in (1, 63, 64, 65):                                    # partly filled blocks
        assert np.array_equal(geom(fn, c['Tr'][:n]), c['tri_orc'][:n])


def test_segments_intersect_fast_abstains_but_never_lies():
    """fn 3: 0 / 1 are the oracle's answer (the exact one on the sample); the undecided cases hold both exact answers >= 1 000 times
    each, counted on the exact sample"""
    c = predicate_cases()
    got = geom(3, c['S'])
    und = got == E.UNDECIDED
    assert np.array_equal(got[~und], c['seg_orc'][~und])
    assert np.array_equal(got, E.segments_fast_np(*c['S'].T))
    s = c['seg_idx']
    assert np.array_equal(got[s][~und[s]], c['seg_exact'][~und[s]])
    n_hit, n_miss = int((c['seg_exact'][und[s]] == 1).sum()), int((c['seg_exact'][und[s]] == 0).sum())
    print(f'fn 3 segments_intersect_fast: {len(got)} pairs, undecided {int(und.sum())} (oracle: {int(c["seg_orc"][und].sum())} with a common point); '
          f'exact sample {len(s)}: undecided {int(und[s].sum())}, of them exact intersection {n_hit}, exact non-intersection {n_miss}')
    assert n_hit >= 1000 and n_miss >= 1000


# ---- layer 1: the robust hull-edge test and detect_collision ------------------------------------------------------------------------
def _pose(rng, k):
    s = T.SCALES[k % 3]
    return np.array([rng.uniform(-s, s), rng.uniform(-s, s), rng.uniform(-np.pi, np.pi)])


@functools.lru_cache(maxsize=None)
def hull_edge_cases():
    from oracle import oracle as O
    rng = np.random.default_rng(21)
    rows, boxes = [], []
    for k in range(1500):
        pose = _pose(rng, k)
        box = O.create_box(pose)
        ct, sn = _cs(pose[2])
        quads = [T.touching_obstacle(rng, box)]
        if k % 4 == 0:
            quads += T.filler_quads(rng, pose[None], 1) + [T.far_quad(rng, pose, 2.0, 5.0)]
        for q in quads:
            for j in range(4):
                rows.append([pose[0], pose[1], ct, sn, *q[j], *q[(j + 1) % 4]])
                boxes.append(box)
    return np.array(rows), np.array(boxes)


def test_hull_edge_intersect_robust_is_the_exact_predicate():
    """fn 4: edges of obstacles built to touch the hull (and some that do not), 64 per block through the one work area"""
    from oracle import oracle as O
    rows, boxes = hull_edge_cases()
    got = geom(4, rows)
    orc = np.array([any(O.segments_intersect(b[k], b[(k + 1) % 4], r[4:6], r[6:8]) for k in range(4)) for r, b in zip(rows, boxes)], np.int32)
    bad = np.nonzero(got != orc)[0]
    assert len(bad) == 0, (len(bad), bad[:5], rows[bad[:2]])
    s = np.arange(0, len(rows), 2)
    exact = np.array([E.hull_edge_intersect_exact(boxes[i], rows[i, 4:6], rows[i, 6:8]) for i in s], np.int32)
    assert np.array_equal(got[s], exact)
    b1, b2 = boxes, np.roll(boxes, -1, axis=1)
    r = E.segments_fast_np(b1[:, :, 0], b1[:, :, 1], b2[:, :, 0], b2[:, :, 1], rows[:, 4, None], rows[:, 5, None], rows[:, 6, None], rows[:, 7, None])
    und = (r == E.UNDECIDED).any(axis=1) & ~(r == 1).any(axis=1)
    n_hit, n_miss = int((exact[und[s]] == 1).sum()), int((exact[und[s]] == 0).sum())
    print(f'fn 4 hull_edge_intersect_robust: {len(rows)} edges, left open by the filter {int(und.sum())}; exact sample {len(s)}: of the open ones '
          f'exact intersection {n_hit}, exact non-intersection {n_miss}')
    assert und.sum() >= 500 and n_hit >= 100 and n_miss >= 100


@functools.lru_cache(maxsize=None)
def collision_cases():
    """(n_obst, records [c][4 + 8 n_obst], boxes, quads) per obstacle count: the touching obstacle in the first slot, in the last, and (32
    obstacles) in a slot >= 16, i.e. in detect_collision's second pass of 64 edges; every fourth case with a second touching
    obstacle; the other slots hold fillers a few centimetres off the hull and far quads"""
    from oracle import oracle as O
    rng = np.random.default_rng(22)
    out = []
    for n_obst in (1, 2, 8, 9, 32):
        recs, boxes, qs = [], [], []
        slots = ['first'] if n_obst == 1 else (['first', 'last', 'second_pass'] if n_obst == 32 else ['first', 'last'])
        for k in range(120 * len(slots)):
            pose = _pose(rng, k)
            box = O.create_box(pose)
            ct, sn = _cs(pose[2])
            where = slots[k % len(slots)]
            slot = 0 if where == 'first' else (n_obst - 1 if where == 'last' else int(rng.integers(16, 32)))
            quads = T.filler_quads(rng, pose[None], min(n_obst, 5))
            quads = (quads + [T.far_quad(rng, pose, 6.0, 9.0) for _ in range(n_obst)])[:n_obst]
            quads[slot] = T.touching_obstacle(rng, box)
            if n_obst >= 2 and (k // len(slots)) % 4 == 0:        # a second touching obstacle in the same pass of 16 obstacles
                lo = 16 * (slot // 16)
                other = [i for i in range(lo, min(lo + 16, n_obst)) if i != slot]
                quads[other[int(rng.integers(len(other)))]] = T.touching_obstacle(rng, box)
            quads = np.array(quads)
            recs.append(np.concatenate([[pose[0], pose[1], ct, sn], quads.ravel()]))
            boxes.append(box)
            qs.append(quads)
        out.append((n_obst, np.array(recs), boxes, qs))
    return out


def test_detect_collision_wave_against_oracle_and_exact():
    """fn 5: the hit flag equals the oracle and the exact answer; the counter says that the robust path ran wherever the numpy mirror
    of the filter finds "undecided, no certain hit", and counts every open lane when nothing is hit"""
    from oracle import oracle as O
    tot = dict(cases=0, robust=0, hit=0, miss=0, two=0)
    for n_obst, recs, boxes, qs in collision_cases():
        got = geom(5, recs, n_obst=n_obst)
        nv = np.full(n_obst, 4, np.int32)
        for i, (box, quads) in enumerate(zip(boxes, qs)):
            assert got[i, 0] == int(O.detect_collision(box, quads, nv)), (n_obst, i)
            robust, hit = T.collision_filter_and_exact(box, quads)
            assert got[i, 0] == int(hit), (n_obst, i)
            if i % 8 == 0:                                        # every pair on exact rationals
                assert got[i, 0] == int(E.collision_exact(box, quads)), (n_obst, i)
            lanes = int((T.pair_table(box, quads) == E.UNDECIDED).any(axis=2).sum())
            if robust:
                assert got[i, 1] > 0, (n_obst, i)
                if not hit:
                    assert got[i, 1] == lanes, (n_obst, i, got[i], lanes)
                tot['robust'] += 1
                tot['hit' if hit else 'miss'] += 1
                tot['two'] += lanes >= 2
            tot['cases'] += 1
    print('fn 5 detect_collision: cases {cases}, undecided with no certain hit {robust} (exact intersection {hit}, exact non-intersection {miss}), '
          'with two or more open lanes {two}'.format(**tot))
    assert tot['robust'] >= 0.25 * tot['cases'] and tot['hit'] >= 0.1 * tot['robust'] and tot['miss'] >= 0.1 * tot['robust'] and tot['two'] >= 100


# ---- layer 1: the clips, the ring distance, the arrival bound -------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def clip_cases():
    from hope_amd.scene_gen import mixed_arrays
    from oracle import oracle as O
    pairs = list(E.quad_pairs(np.random.default_rng(3), 3000)) + list(E.degenerate_quad_pairs(np.random.default_rng(6), 400))
    n_gen = 3000
    start, dest = mixed_arrays(300, seed=23, max_obst=128)[:2]    # the reward's own operands: hull of a pose vs dest box of a scene
    rng = np.random.default_rng(24)
    for k in range(300):
        pose = dest[k] + rng.normal(size=3) * (np.array([0.05, 0.05, 0.01]) if k % 2 else np.array([1.5, 1.0, 0.3]))
        pairs.append((O.create_box(pose), O.create_box(dest[k])))
    rows = np.array([np.concatenate([np.ravel(A), np.ravel(B)]) for A, B in pairs])
    orc = np.array([O.quad_intersection_area(A, B) for A, B in pairs])
    s = np.concatenate([np.arange(0, n_gen, 5), np.arange(n_gen, len(pairs))])
    exact = np.array([float(E.clip_area_exact(*pairs[i])) for i in s])
    return rows, orc, s, exact


@pytest.mark.parametrize('fn', [6, 7])
def test_quad_clip_equals_the_oracle_bit_for_bit(fn):
    """fn 6 (one lane, sh[64]) and fn 7 (16 lanes, 16 cases, column layout) on near-arrival, generic, parallel and degenerate pairs
    (equal quads, shared collinear edges, a vertex on an edge, containment, disjoint) and on the reward's own operands"""
    rows, orc, s, exact = clip_cases()
    got = geom(fn, rows)
    bad = np.nonzero(got != orc)[0]
    assert len(bad) == 0, (fn, len(bad), bad[:5], got[bad[:3]], orc[bad[:3]])
    worst = float(np.abs(got[s] - exact).max())
    print(f'fn {fn}: {len(rows)} quad pairs bit-equal to the oracle; worst error against the exact area on {len(s)} of them {worst:.3g} m^2')
    assert worst < 1e-12
    assert (orc == 0).sum() > 100 and (orc > 8.0).sum() > 100
    if fn == 7:
        one = geom(6, rows)
        assert np.array_equal(got, one)
        for n in (1, 15, 16, 17, 63, 65):                        # partly filled groups of 16 columns
            off = 3000 - n // 2                                   # (generated and degenerate pairs side by side)
            assert np.array_equal(geom(7, rows[off:off + n]), one[off:off + n]), n


def test_origin_seg_dist_equals_the_oracle_bit_for_bit():
    """fn 8 on the CPU test's point / segment cases, moved so that the point is the origin"""
    from oracle import oracle as O
    rows = np.array([[a[0] - p[0], a[1] - p[1], b[0] - p[0], b[1] - p[1]] for p, a, b in E.point_segment_cases(np.random.default_rng(4), 20000)])
    got = geom(8, rows)
    lib = O.lib()
    lib.orc_pt_seg_dist.argtypes = [C.c_double] * 6
    lib.orc_pt_seg_dist.restype = C.c_double
    orc = np.array([lib.orc_pt_seg_dist(0.0, 0.0, *r) for r in rows.tolist()])
    assert np.array_equal(got, orc)
    s = np.arange(0, len(rows), 2)
    exact = np.array([math.sqrt(float(E.pt_seg_dist2_exact((0.0, 0.0), rows[i, 0:2], rows[i, 2:4]))) for i in s])
    worst = float(np.abs(got[s] - exact).max())
    print(f'fn 8 origin_seg_dist: {len(rows)} cases bit-equal to the oracle; worst error against the exact distance on {len(s)} of them {worst:.3g} m')
    assert worst < 1e-13
    assert (rows[:, 0:2] == rows[:, 2:4]).all(axis=1).sum() > 1000               # degenerate segments among them


def test_arrival_possible_never_rules_out_an_arrival():
    """fn 9 is a shortcut the oracle does not have: it must be 1 wherever the overlap ratio exceeds 0.95.  Poses scattered about
    the dest boxes of generated and Dragon-Lake scenes, re-sampled until the neighbourhood of the threshold is well filled"""
    from hope_amd.scene_gen import mixed_arrays
    from oracle import oracle as O
    dest = mixed_arrays(400, seed=25, max_obst=128)[1]
    rng = np.random.default_rng(26)
    rows, ratio = [], []
    band = tight = 0
    dinfo = []
    for d in dest:
        B = O.create_box(d)
        cd, sd = _cs(d[2])
        dinfo.append((B, O.quad_area(B), 0.5 * (B[0, 0] + B[2, 0]), 0.5 * (B[0, 1] + B[2, 1]), cd, sd))
    rounds = 0
    while band < 2000 or tight < 500:
        rounds += 1
        assert rounds <= 40
        for d, (B, area, dcx, dcy, cd, sd) in zip(dest, dinfo):
            for _ in range(4):
                pose = d + rng.uniform(-1, 1, 3) * np.array([0.5, 0.5, 0.2]) * rng.random() ** 2
                r = O.quad_intersection_area(O.create_box(pose), B) / area
                ct, sn = _cs(pose[2])
                rows.append([pose[0], pose[1], ct, sn, dcx, dcy, cd, sd])
                ratio.append(r)
                band += 0.93 < r < 0.97
                tight += 0.95 < r < 0.96
    rows, ratio = np.array(rows), np.array(ratio)
    got = geom(9, rows)
    lost = np.nonzero((ratio > 0.95) & (got != 1))[0]
    assert len(lost) == 0, (len(lost), rows[lost[:3]], ratio[lost[:3]])
    print(f'fn 9 arrival_possible: {len(rows)} poses, ratio in (0.93, 0.97): {band}, in (0.95, 0.96): {tight}, ratio > 0.95: {int((ratio > 0.95).sum())}; '
          f'bound passes with ratio <= 0.95 (its slack): {int(((got == 1) & (ratio <= 0.95)).sum())}, bound rules out: {int((got == 0).sum())}')
    assert set(np.unique(got)) <= {0, 1} and (got == 0).sum() > 100


# ---- layer 2: scenes that send the step kernels through the robust path -----------------------------------------------------------------
N_SCENES, MO = 1501, 128
OUTS = ('status', 'done', 'pose', 'reward', 'reward_info')
FORMS = {'one_launch': ('1000000000', False), 'two_launch_pair_kernels': ('1', False), 'two_launch_large_tile': ('1', True)}


def _stages():
    """STAGE_ALL: without the search stage the launcher takes the one-launch form whatever HOPE_SPLIT_MIN says (the Reeds-Shepp
    outputs are not compared here)"""
    from hope_amd import _lib as L
    return L.STAGE_ALL


def _oracle(sc, n=None):
    from hope_amd import tables as TB
    from oracle import oracle as O
    n = len(sc['nob']) if n is None else n
    t = TB.all_tables()
    O.set_tables(hull_base=t['hull_base'], beam_a=t['beam_ab'][:, 0], beam_b=t['beam_ab'][:, 1], dist_star=t['dist_star'], omp=True)
    orc = O.BatchOracle(n, MO, omp=True, track_traj=False)
    orc.set_scenes(np.arange(n), sc['start'], sc['dest'], sc['bbox'], sc['verts'], sc['nvert'], sc['nob'])
    return orc


def _snapshot(orc, o):
    return dict(status=o['status'].copy(), done=(o['status'] != CONTINUE).astype(np.uint8), reward=o['reward'].copy(),
                reward_info=o['reward_info'].copy(), pose=orc.pose.copy(), t=orc.t.astype(np.int32), accum=orc.accum.copy())


@functools.lru_cache(maxsize=None)
def scene_reference(moving):
    """the scenes, their premise (asserted before anything runs on the device) and the oracle's reset observation and step, once"""
    sc = T.build(N_SCENES, 42 if moving else 41, moving, max_obst=MO)
    assert N_SCENES % 2 == 1 and sc['nob'].max() <= 32
    near = [T.near_count(np.vstack([sc['start'][i][None], T.substep_poses(sc['start'][i], sc['action'][i])]), sc['verts'][i, :sc['nob'][i]])
            for i in np.nonzero(sc['many'])[0]]
    assert min(near) >= 9 and max(near) <= 12
    census = {}
    if not moving:
        census['reset'] = T.assert_premise(sc, reset=True, tag='reset_obs, start pose touching')
    census['step'] = T.assert_premise(sc, reset=False, tag='moving step' if moving else 'zero-action step')
    orc = _oracle(sc)
    ref_reset = _snapshot(orc, orc.reset_obs(with_rs=False))
    ref_step = _snapshot(orc, orc.step(sc['action'], with_rs=False))
    return sc, census, ref_reset, ref_step


def _env(sc, form=None):
    """form None: the classes as set_scene_arrays leaves them (all small; the overlapped handle hands the last 42 % of the ids to the
    large-tile chain).  A name of FORMS: both chains non-empty with the ADVERSARIAL scenes in the chain whose kernel the form names --
    the small-tile chain (pair kernels) or, `large`, the large-tile chain -- and the plain scenes in the other, nothing handed over"""
    from hope_amd import ParkingBatch
    n = len(sc['nob'])
    large = form is not None and FORMS[form][1]
    if form is not None and FORMS[form][0] == '1':
        os.environ['HOPE_CLS1_FRAC'] = '0'
    try:
        env = ParkingBatch(n, MO, obs_dtype=torch.float64, action_dtype=torch.float64, overlap=True)
        env.set_scene_arrays(np.arange(n), sc['start'], sc['dest'], sc['bbox'], sc['verts'], sc['nob'])
        if form is not None and FORMS[form][0] == '1':
            env.set_draw_class(np.nonzero(sc['adv'] if large else ~sc['adv'])[0], 1)
    finally:
        os.environ.pop('HOPE_CLS1_FRAC', None)
    return env


KERNELS = {'one_launch': ('one_launch_fused_kin', 'in_step', None), 'two_launch_pair_kernels': ('pair', 'pair', 32),
           'two_launch_large_tile': ('split_one_scene', 'split_one_scene', MO)}


def _assert_routing(env, sc, form, has_action=True, every=True):
    """through the launch plan: the adversarial scenes (`every`: all of them, else some) are stepped by the kernels the form names"""
    plan = env.step_plan(stages=_stages(), has_action=has_action)
    motion, obs, cap = KERNELS[form]
    if not has_action and motion == 'pair':
        motion = 'split_one_scene'                                # (the action-less step has no pair motion kernel; its observation is k_obs_pair's)
    named = [c for c in plan['chains'] if (c['motion'], c['obs']) == (motion, obs) and cap in (None, c['tile_cap'])]
    ids = np.concatenate([c['scenes'] for c in named]) if named else np.zeros(0, np.int32)
    adv = np.nonzero(sc['adv'])[0]
    inside = np.isin(adv, ids)
    print(f"launch plan ({form}, {'step' if has_action else 'reset_obs'}): split {plan['split']}, fused kinematics {plan['fuse_kin']}; " +
          '; '.join(f"tile class {c['tile_class']} capacity {c['tile_cap']}: {len(c['scenes'])} scenes, motion {c['motion']}, observation {c['obs']}"
                    for c in plan['chains']) + f'; adversarial scenes in the named kernel {int(inside.sum())} of {len(adv)}')
    assert plan['split'] == (FORMS[form][0] == '1') and len(plan['chains']) == 2
    assert inside.all() if every else inside.sum() >= 0.4 * len(adv)


def _check(env, ref, tag):
    torch.cuda.synchronize()
    rows = slice(None)
    for k in OUTS:
        got, want = getattr(env, k).cpu().numpy()[rows], ref[k][rows]
        bad = np.nonzero((got != want).reshape(len(got), -1).any(axis=1))[0]
        assert len(bad) == 0, (tag, k, len(bad), bad[:8], got[bad[:3]], want[bad[:3]])
    pose, t, acc = env.download_state()
    assert np.array_equal(pose[rows], ref['pose'][rows]) and np.array_equal(t[rows], ref['t'][rows]) and np.array_equal(acc[rows], ref['accum'][rows]), tag


def _report(tag, sc, census, ref):
    robust, answer = census
    st = ref['status']
    print(f'{tag}: scenes {len(st)}, adversarial {int(sc["adv"].sum())}, on the robust path {int(robust.sum())} (exact intersection {int((answer == 1).sum())}, '
          f'exact non-intersection {int((answer == 0).sum())}); of those COLLIDED {int((st[robust] == COLLIDED).sum())}, CONTINUE {int((st[robust] == CONTINUE).sum())}')


@pytest.mark.parametrize('form', list(FORMS))
def test_start_pose_touching_reset_and_zero_action_step(form):
    """Cases 1 and 2: the action-less step's status test on a start pose that touches an obstacle, then one step with a zero action
    in the touching scenes (all ten poses are the start pose: an exact hit retreats to the start and re-tests the status, an
    exact miss takes the robust path at every sub-step)"""
    sc, census, ref_reset, ref_step = scene_reference(False)
    split, large = FORMS[form]
    os.environ['HOPE_SPLIT_MIN'] = split
    try:
        env = _env(sc, form)
        _assert_routing(env, sc, form, has_action=False)
        env.reset_obs(stages=_stages())
        _check(env, ref_reset, (form, 'reset'))
        _assert_routing(env, sc, form)
        env.step(torch.from_numpy(sc['action']).to(env.device), stages=_stages())
        _check(env, ref_step, (form, 'zero action'))
        _report(f'reset_obs ({form})', sc, census['reset'], ref_reset)
        _report(f'zero-action step ({form})', sc, census['step'], ref_step)
        rb = census['reset'][0]
        assert (ref_reset['status'][rb] == COLLIDED).sum() >= 0.1 * rb.sum() and (ref_reset['status'][rb] == CONTINUE).sum() >= 0.1 * rb.sum()
        env.close()
    finally:
        os.environ.pop('HOPE_SPLIT_MIN', None)


@pytest.mark.parametrize('form', list(FORMS))
def test_moving_step_touching_at_a_sub_step(form):
    """Case 3: random actions, the obstacle against the hull of sub-step k* (0..9); the oracle decides what the step does.  One launch,
    two launches with the pair kernels, two launches with the scenes in the large-tile class (k_env_step's motion part)"""
    sc, census, ref_reset, ref_step = scene_reference(True)
    split, large = FORMS[form]
    os.environ['HOPE_SPLIT_MIN'] = split
    try:
        env = _env(sc, form)
        env.reset_obs(stages=_stages())
        _check(env, ref_reset, (form, 'reset'))
        _assert_routing(env, sc, form)
        env.step(torch.from_numpy(sc['action']).to(env.device), stages=_stages())
        _check(env, ref_step, (form, 'moving'))
        _report(f'moving step ({form})', sc, census['step'], ref_step)
        assert len(np.unique(sc['kstar'][census['step'][0]])) == 10          # every sub-step 0..9 among the scenes on the robust path
        env.close()
    finally:
        os.environ.pop('HOPE_SPLIT_MIN', None)


def test_pair_kernels_equal_the_one_scene_kernels_on_touching_scenes():
    """Case 3, additionally: both scenes of a pair wave in the robust loop with one work area between them -- every output and the
    state equal the one-scene kernels' (STAGE_ONE_SCENE) bit for bit"""
    from hope_amd import _lib as L
    sc = scene_reference(True)[0]
    os.environ['HOPE_SPLIT_MIN'] = '1'
    try:
        envs = [_env(sc) for _ in range(2)]
        a = torch.from_numpy(sc['action']).to(envs[0].device)
        for e, extra in zip(envs, (0, L.STAGE_ONE_SCENE)):
            e.reset_obs(stages=L.STAGE_ALL | extra)
            e.step(a, stages=L.STAGE_ALL | extra)
        torch.cuda.synchronize()
        for k in ('lidar', 'action_mask', 'status', 'done', 'pose', 'reward', 'reward_info', 'target', 'rs_word', 'rs_lengths'):
            assert torch.equal(getattr(envs[0], k), getattr(envs[1], k)), k
        for u, v in zip(envs[0].download_state(), envs[1].download_state()):
            assert np.array_equal(u, v)
        for e in envs:
            e.close()
    finally:
        os.environ.pop('HOPE_SPLIT_MIN', None)


@functools.lru_cache(maxsize=None)
def pool_reference():
    """a pool in which every other lot has an obstacle against its START pose and a dest box that overlaps the start hull: the new
    episode's accumulated arrival reward is zero exactly when the start pose collides"""
    pool = T.build(600, 43, False, max_obst=MO, layout='alternate', dest_near=True)
    census = T.assert_premise(pool, reset=True, tag='pool lots, start pose touching')
    orc = _oracle(pool)
    first = _snapshot(orc, orc.reset_obs(with_rs=False))          # every lot's first observation: status, t = 1, accum
    zero = np.zeros((600, 2))
    second = _snapshot(orc, orc.step(zero, with_rs=False))
    return pool, census, first, second


@pytest.mark.parametrize('form', ['one_launch', 'two_launch_pair_kernels'])
def test_turnover_onto_a_start_pose_that_touches(form):
    """Case 4: scenes at the end of their episode draw a new lot inside the step (auto_reset, fresh); the turnover path tests the new
    start pose for a collision.  The new episode's state, and the status of its first step (zero action), equal the oracle's on the
    lots drawn"""
    pool, census, first, second = pool_reference()
    sc = scene_reference(True)[0]
    n = N_SCENES
    os.environ['HOPE_SPLIT_MIN'] = FORMS[form][0]
    try:
        env = _env(sc)
        env.set_pool(tuple(pool[k] for k in ('start', 'dest', 'bbox', 'verts', 'nob', 'nvert')))
        env.set_redraw_seed(7)
        env.reset_obs(stages=_stages())
        env.upload_state(t=np.full(n, 200, np.int32))             # every episode that goes on runs out of time in this step
        # (the slots draw from the pool's small class, so every scene keeps its class: the last 42 % of the ids are in the large-tile chain)
        _assert_routing(env, sc, form, every=form == 'one_launch')
        a = torch.from_numpy(sc['action']).to(env.device)
        env.step(a, stages=_stages(), auto_reset=True, fresh=True)
        torch.cuda.synchronize()
        assert env.done.cpu().numpy().all()
        idx = env.pool_index()
        assert (idx >= 0).all() and env.pool_overflow() == 0
        pose, t, acc = env.download_state()
        assert np.array_equal(pose, pool['start'][idx]) and (t == 1).all()
        bad = np.nonzero(acc != first['accum'][idx])[0]
        assert len(bad) == 0, (form, len(bad), bad[:8], acc[bad[:4]], first['accum'][idx][bad[:4]])
        env.step(torch.zeros((n, 2), dtype=torch.float64, device=env.device), stages=_stages())
        torch.cuda.synchronize()
        for k in OUTS:
            assert np.array_equal(getattr(env, k).cpu().numpy(), second[k][idx]), (form, k)
        pose, t, acc = env.download_state()
        assert np.array_equal(pose, second['pose'][idx]) and np.array_equal(t, second['t'][idx]) and np.array_equal(acc, second['accum'][idx])
        robust, answer = census
        drawn = np.bincount(idx, minlength=600) > 0
        rb = robust[idx]
        print(f'turnover ({form}): scenes {n}, lots drawn {int(drawn.sum())} of 600, scenes whose new start pose is on the robust path {int(rb.sum())} '
              f'(exact intersection {int((answer[idx] == 1).sum())}, exact non-intersection {int((answer[idx] == 0).sum())}); '
              f'of those with a first reward term {int((first["accum"][idx][rb] > 0).sum())}, COLLIDED at the first step {int((second["status"][idx][rb] == COLLIDED).sum())}')
        assert rb.sum() >= 0.1 * n and (first['accum'][idx][rb] > 0).sum() >= 0.1 * rb.sum() and (first['accum'][idx][rb] == 0).sum() >= 0.1 * rb.sum()
        env.close()
    finally:
        os.environ.pop('HOPE_SPLIT_MIN', None)
