"""The image oracle (oracle/hope_oracle_img.c) against the literal renderer of tests/image_program.py on the programmed lots, and the
trigger facts of every family (CPU only).  The device runs the same lots in tests/test_gpu_image_program.py."""
import math
from fractions import Fraction

import numpy as np
import pytest

import image_program as P
from hope_amd.scenes import pack_scenes
from oracle import oracle as O

STATIC = ('polygons', 'polygons_padded', 'truncation', 'outlines', 'headings')
_cache = {}


def family(name):
    if name not in _cache:
        _cache[name] = P.polygons(pad=128) if name == 'polygons_padded' else getattr(P, name)()
    return _cache[name]


def compare(scene, pose, traj, what):
    """oracle == literal on all 250 000 ids and, at a quarter-turn heading, on every uint8 of the image"""
    w = O.bev_world(scene.verts, scene.nvert, scene.start, scene.dest, scene.bbox, pose, traj)
    lit = P.literal_world(scene, pose, traj)
    assert (w == lit).all(), f'{what}: {int((w != lit).sum())} ids differ, first (y, x) {tuple(np.argwhere(w != lit)[0])}'
    if P.quarter_turns(pose[2]) is not None:
        img = O.bev_image(scene.verts, scene.nvert, scene.start, scene.dest, scene.bbox, pose, traj).transpose(1, 2, 0)
        want = P.literal_quarter_image(lit, scene.bbox, pose)
        assert (img == want).all(), f'{what}: {int((img != want).sum())} image values differ'
    return lit


@pytest.mark.parametrize('name', STATIC)
def test_oracle_world_and_quarter_image_equal_the_literal_renderer(name):
    fam = family(name)
    assert 0 < len(fam) <= 256
    for k, (s, p) in enumerate(zip(fam.scenes, fam.poses)):
        compare(s, p, [s.start], f'{name} lot {k}')


def test_polygon_facts():
    f = family('polygons').facts
    assert f['four_rows']['arrow'] >= 10 and f['four_rows']['bowtie'] >= 10, f['four_rows']
    assert f['border_pass'], 'the interior-edge quadrilateral must take the horizontal border pass'
    assert set(range(1, 21)) <= f['span_widths'], f['span_widths']
    assert f['wall'] == P.WIN
    # the padded variant puts every programmed obstacle at an index >= 128
    pad = family('polygons_padded')
    for s in pad.scenes[::16]:
        assert 128 < len(s.verts) <= 160 and P.shapes_box(s, which=range(128)) is None and P.shapes_box(s) is not None
    # a shape whose only row in a band of 16 rows is its maxy row (the `y == maxy` rule at a band seam)
    assert any(max(p[1] for p in r) % 16 == 0 and min(p[1] for p in r) < max(p[1] for p in r)
               for s in family('polygons').scenes[::16] for r in P.pixel_rings(s))
    # 70 obstacles in one band of 16 rows -> its second chunk of 64 is used; the 71st lies under the start outline and the dest box
    s = family('polygons').scenes[-1]
    rows = [(min(p[1] for p in r), max(p[1] for p in r)) for r in P.pixel_rings(s)[:70]]
    assert len(s.verts) == 71 and all(160 <= a and b <= 175 for a, b in rows)
    w = P.literal_world(s, np.array([1e4, 1e4, 0.0]), [])
    inside = np.zeros_like(w, bool)
    inside[150:191, 90:171] = True
    assert (w[inside] == 2).any() and (w[inside] == 3).any() and (w[inside] == 1).any()


def test_truncation_facts():
    f = family('truncation').facts
    for kind in ('obstacle', 'dest', 'start'):
        assert f[kind]
        for px, p in f[kind]:
            assert px == [p - 1, p, p], (kind, px, p)          # one ulp below the exact product is the pixel before


def test_outline_facts():
    f = family('outlines').facts
    assert not f['missing'], f['missing']
    assert set().union(*f['features'].values()) >= P.OUTLINE_FEATURES


def test_heading_facts():
    fam = family('headings')
    f = fam.facts
    assert len(f['quarter']) >= len(P.QUARTER_DEGREES) and len(f['general']) >= 2 * len(P.QUARTER_DEGREES) + 4
    for k in f['quarter']:
        assert P.quarter_turns(fam.poses[k][2]) is not None
    for k in f['general']:
        assert P.quarter_turns(fam.poses[k][2]) is None
    turns = {P.quarter_turns(fam.poses[k][2]) for k in f['quarter']}
    assert turns == {0, 1, 2, 3}
    # ((int)angle / 90) % 4 of the negative angles and of those beyond a full turn
    want = {0: 0, 90: 1, -90: 3, 180: 2, -180: 2, 270: 3, -270: 1, 360: 0, -360: 0, 450: 1, -450: 3, 720: 0}
    for d, t in want.items():
        assert P.quarter_turns(P.heading_of_degrees(np.float32(d))) == t, d
    # corner lots: the image holds samples outside the source -- changing surface pixel (0, 0) changes the image away from it
    ids = {'empty': 0, 'obstacle': 1, 'dest': 3, 'start': 2, 'vehicle': 4}
    seen = {k: 0 for k in ids}
    for k, what in f['corner']:
        s, p = fam.scenes[k], fam.poses[k]
        w = O.bev_world(s.verts, s.nvert, s.start, s.dest, s.bbox, p, [s.start])
        assert w[0, 0] == ids[what], (k, what, w[0, 0])
        w2 = w.copy()
        w2[0, 0] = 1 if w[0, 0] != 1 else 0
        a, b = O.bev_process(O.bev_raw(w, s.bbox, p)), O.bev_process(O.bev_raw(w2, s.bbox, p))
        seen[what] += int((a != b).any(-1).sum() >= 8)
    assert all(v >= 1 for v in seen.values()), seen


def test_observer_sweep_covers_its_box_and_the_sample_set_is_the_oracles():
    lot = P.make_lot([P.rect(100, 100, 180, 150)], (120, 190, 0.0))
    copies = P.observer_sweep(lot)
    assert len(copies) == 16 and len({tuple(c.start) for c in copies}) == 16
    seen = np.zeros((P.WIN, P.WIN), bool)
    for c in copies:
        m = P.sampled_world_pixels(c.bbox, c.start)
        assert 0.2 < m[100:151, 100:181].mean() < 0.3        # a quarter of the pixels each
        seen |= m
    assert seen[100:151, 100:181].all()
    with pytest.raises(AssertionError):
        P.observer_sweep(lot, box=(100, 100, 180, 400))      # a box the crop cannot hold is refused, not passed over
    # sampled_world_pixels is what the ORACLE observes: a single world pixel shows in the image exactly when it is in the set
    rng = np.random.default_rng(3)
    for d in (0, 90, 180, -90):
        pose = np.array([P.wr(250), P.wr(240), P.heading_of_degrees(np.float32(d))])
        m = P.sampled_world_pixels(P.BBOX, pose)
        assert m.sum() == 128 * 128
        for x, y in rng.integers(150, 350, (24, 2)):
            w = np.zeros((P.WIN, P.WIN), np.uint8)
            w[y, x] = 1
            assert O.bev_process(O.bev_raw(w, P.BBOX, pose)).any() == m[y, x], (d, x, y)


def test_floor_ceil_rule_agrees_with_exact_fractions():
    """for the sizes used the float32 quotient floors / ceils like the exact one: asserted, not assumed"""
    rings = []
    for name in STATIC:
        fam = family(name)
        for s in fam.scenes[::16] if name != 'headings' else fam.scenes:
            off = P.offsets(s.bbox)
            rings += P.pixel_rings(s) + [P.to_pixels(P.car_corners(q), off)[:-1] for q in (s.start, s.dest)]
    n = 0
    for r in rings:
        pts = r + r[:1]
        for y, terms in P.scan_rows([p[0] for p in pts], [p[1] for p in pts]):
            for k, (num, den, x1) in enumerate(terms):
                q, e = np.float32(num) / np.float32(den), Fraction(num, den)
                assert math.floor(q) == math.floor(e) and math.ceil(q) == math.ceil(e), (r, y, num, den)
                n += 1
    assert n > 5000


def test_row_spans_domain_limit_holds_for_every_obstacle_the_project_produces(dlp):
    """DESIGN.md, image section: row_spans' product (y - y1)(x2 - x1) and its float32 quotient are exact while an obstacle is at most
    4096 px = 341 m wide and high (product <= 2^24; a non-integer quotient is >= 2^-12 away from an integer, its rounding error
    <= 2^-13)."""
    limit = 4096
    assert int(np.float32(limit * limit)) == limit * limit and int(np.float32(2 ** 24 + 1)) != 2 ** 24 + 1
    rng = np.random.default_rng(0)
    for den, dx, k in zip(rng.integers(1, limit + 1, 20000), rng.integers(-limit, limit + 1, 20000), rng.random(20000)):
        num = int(k * den) * int(dx)
        q, e = np.float32(num) / np.float32(den), Fraction(num, int(den))
        assert math.floor(q) == math.floor(e) and math.ceil(q) == math.ceil(e)
    v = dlp['set_verts']
    ext = [float((v[..., a].max(1) - v[..., a].min(1)).max()) for a in (0, 1)]
    from hope_amd.scenes import SceneSource
    src = SceneSource(levels=('Normal', 'Complex', 'Extrem'), seed=3)
    for _ in range(300):
        s = src.draw()
        ext += [float((s.verts[..., a].max(1) - s.verts[..., a].min(1)).max()) for a in (0, 1)]
    assert P.K * max(ext) + 2 < limit, max(ext)


def test_car_boxes_are_plain_one_span_per_row_boxes():
    """a thinned repeat of the search the module docstring reports: no car box violates F_SIMPLE, folded corners included"""
    assert P.search_non_simple_car_box(n_head=360, subs=(0.0, 0.5)) == []
    assert not P.car_box_is_simple([(0, 0), (5, 0), (5, 0), (0, 0), (0, 0)])
    assert not P.car_box_is_simple([(0, 0), (10, 10), (10, 0), (0, 10), (0, 0)])         # the bowtie has rows with four


# ---- drives ----------------------------------------------------------------------------------------------------------------
def drive_oracle(drive, max_obst=8):
    """steps the oracle through the drive: [(pose, trajectories, substeps, entries)] at reset and after every step"""
    sc = drive.family.scenes
    n = len(sc)
    orc = O.BatchOracle(n, max_obst)
    start, dest, bbox, verts, nob, nvert = pack_scenes(sc, max_obst)
    orc.set_scenes(np.arange(n), start, dest, bbox, verts, nvert, nob)
    orc.reset_obs(with_rs=False)
    entries = np.ones(n, np.int64)
    hist = [(orc.pose.copy(), [list(t) for t in orc.traj], np.zeros(n, np.int32), entries.copy())]
    for a in drive.actions:
        o = orc.step(a, with_rs=False)
        entries = entries + (o['substeps'] > 0)
        hist.append((orc.pose.copy(), [list(t) for t in orc.traj], o['substeps'].copy(), entries.copy()))
    return orc, hist


def test_trail_drives_reach_their_paths_and_the_oracle_equals_the_literal_renderer():
    d = P.trails()
    orc, hist = drive_oracle(d)
    n = len(d.family)
    assert n <= 256 and len(d.actions) <= 40
    ext_x, ext_y, seam_x, seam_y, stalled = set(), set(), 0, 0, 0
    for it, (pose, traj, sub, entries) in enumerate(hist):
        for k in range(n):
            if len(traj[k]) >= 20:
                b = P.live_box(d.family.scenes[k], traj[k])
                ext_x.add(b[1] - b[0]); ext_y.add(b[3] - b[2])
            c = P.to_pixels(P.car_corners(pose[k]), P.offsets(d.family.scenes[k].bbox))
            seam_x += min(a[0] for a in c) < 256 <= max(a[0] for a in c)
            seam_y += min(a[1] for a in c) < 256 <= max(a[1] for a in c)
            stalled += it > 0 and sub[k] == 0
    # (b) the box around the drawn boxes 255, 256 and 257 px wide and high: x1 - x0 = 256 is the first the torus cannot hold
    assert {254, 255, 256} <= ext_x and {254, 255, 256} <= ext_y, (sorted(ext_x), sorted(ext_y))
    assert seam_x > 50 and seam_y > 50                        # (a) boxes across x = 256 and y = 256
    assert stalled >= 30                                      # (c) steps that keep no sub-step
    for it in (0, 1, 2, 19, 20, 21, 30, 40):
        pose, traj, _, _ = hist[it]
        for k in range(n):
            compare(d.family.scenes[k], pose[k], traj[k], f'trail lot {k} step {it}')


def test_long_drives_pass_the_layer_refresh_on_a_torus_seam():
    d = P.trails(long=True)
    orc, hist = drive_oracle(d)
    n = len(d.family)
    assert n <= 16 and len(d.actions) <= 200
    hit = {e: 0 for e in (96, 97, 192, 193)}
    for pose, traj, sub, entries in hist:
        for k in range(n):
            c = P.to_pixels(P.car_corners(pose[k]), P.offsets(d.family.scenes[k].bbox))
            on_seam = min(a[0] for a in c) < 256 <= max(a[0] for a in c) or min(a[1] for a in c) < 256 <= max(a[1] for a in c)
            e = int(entries[k]) - 1
            if on_seam and e in hit:
                hit[e] += 1
    assert all(v >= 2 for v in hit.values()), hit             # (d)
    for it in (96, 97, 192, 193, 200):
        pose, traj, _, entries = hist[it]
        for k in range(n):
            compare(d.family.scenes[k], pose[k], traj[k], f'long lot {k} step {it}')


def test_shown_vehicle_lies_under_the_newer_trajectory_boxes():
    d = P.shown_vehicle()
    orc, hist = drive_oracle(d)
    n = len(d.family)
    assert n <= 256
    pose, traj, _, entries = hist[-1]
    assert (entries == len(d.actions) + 1).all()
    new = pose + d.replace
    shown, far_end = 0, {0: 0, 1: 0}
    for k in range(n):
        s = d.family.scenes[k]
        lit = compare(s, new[k], traj[k], f'shown lot {k}')
        shown += bool((lit == 4).any() and (lit >= 5).any())
        b = P.live_box(s, traj[k])
        if P.quarter_turns(new[k][2]) is not None:
            m = P.sampled_world_pixels(s.bbox, new[k])
            # the far end of a live set that is one pixel too wide for the torus: column x0 (row y0) of the OLDEST box is observed
            if b[1] - b[0] == 256 and (m[:, b[0]] & (lit[:, b[0]] == 5)).any():
                far_end[0] += 1
            if b[3] - b[2] == 256 and (m[b[2]] & (lit[b[2]] == 5)).any():
                far_end[1] += 1
    assert shown >= 16, shown                                 # the vehicle colour shows next to trajectory colours
    assert far_end[0] >= 1 and far_end[1] >= 1, far_end
