"""Programmed cases for the bird's-eye image (hope_amd/csrc/hope_bev.hip against oracle/hope_oracle_img.c) and a LITERAL reference.

Two halves, CPU only (numpy):

* `literal_world` / `literal_quarter_image` / `sampled_world_pixels`: a plain Python restatement of CarParking._render
  (car_parking_base.py:301-320) on a 500 x 500 id raster and, for headings that are exact multiples of 90 degrees in float32, of
  _get_img_observation + process_img down to the uint8 output.  Written from the rule the oracle's header cites (pygame draw.c:
  integer vertices by C truncation, draw_fillpoly's row loop with floor / ceil on alternate intersections in discovery order, qsort,
  the `y == maxy` rule, the horizontal border pass, clipping, draw_line's Bresenham WALK), with Python ints and numpy.float32 for the
  one float division.  Nothing here is shared with oracle/ or hope_amd/ (only the `Scene` container is imported).  math.cos / math.sin
  stand in for the shared hope_math.h: a corner that differs in its last bit moves a pixel only when 12 x + off lies within an ulp of
  an integer, which the programmed poses avoid (truncation() uses heading 0, where both are exact).

* case families (`polygons`, `truncation`, `outlines`, `headings`, `trails`, `shown_vehicle`): each returns a `Family` -- the lots, the
  pose the image is observed from at reset (the start pose, or a DETACHED observer that the tests upload from outside: a start outline
  is only visible while the car is somewhere else and the trajectory holds one entry), and a dict of facts the builder has checked on
  the CPU, so that a case which stops reaching its path fails instead of passing vacuously.

Only the 2 x 2 centre of every 4 x 4 block of the crop is observed, so a wrong world pixel is invisible at three poses out of four:
`observer_sweep` moves the observer by 0..3 px in x and y and asserts with `sampled_world_pixels` that every pixel of the programmed
shapes' box is sampled by one of the 16 copies.

shown_vehicle(): the library re-renders without moving through reset_obs() (the action-less step), which leaves the trajectory alone,
so the family exists: after the drive the pose is replaced on both sides and the vehicle box lies UNDER the newer trajectory boxes.

Non-simple car boxes.  `car_box_is_simple` restates F_SIMPLE with the literal row rule.  Searched grid (search_non_simple_car_box):
headings k * pi / 1800 for k = 0..3599 x pose pixel offsets {0, 1/4, 1/2, 3/4}^2 px x four placements (inside the surface; straddling
x = 0; straddling y = 0; over the corner (0, 0), where truncation towards zero folds corners in (-1, 0) onto 0): 230 400 boxes, none
violates F_SIMPLE, so there is no such family; tests/test_image_program.py repeats a thinned grid.
"""
import math
from dataclasses import dataclass, field

import numpy as np

from hope_amd.scenes import Scene

WIN, CROP, OUT, K = 500, 256, 64, 12.0          # configs.py:88-93,103
CROP_OFF = (WIN - CROP) // 2
TRAJ_DRAWN = 20                                 # TRAJ_RENDER_LEN configs.py:86
WHEEL_BASE, FRONT_HANG, REAR_HANG, WIDTH = 2.8, 0.96, 0.93, 1.94          # configs.py:13-17
CAR = [(-REAR_HANG, -WIDTH / 2), (FRONT_HANG + WHEEL_BASE, -WIDTH / 2), (FRONT_HANG + WHEEL_BASE, WIDTH / 2), (-REAR_HANG, WIDTH / 2)]
PALETTE = np.array([(0, 0, 0), (150, 150, 150), (100, 149, 237), (69, 139, 0), (30, 144, 255)] +
                   [(10, 10, 10 + 10 * j) for j in range(20)], np.int32)       # id 0: white, black after change_bg_color


# ====================================================================================================================
# the literal renderer
# ====================================================================================================================
def offsets(bbox):
    """coord_transform_matrix (car_parking_base.py:139-147)"""
    return 0.5 * (WIN - K * (bbox[1] + bbox[0])), 0.5 * (WIN - K * (bbox[3] + bbox[2]))


def car_corners(pose):
    """State.create_box (vehicle.py:32-36)"""
    c, s = math.cos(pose[2]), math.sin(pose[2])
    return [(c * x + (-s) * y + pose[0], s * x + c * y + pose[1]) for x, y in CAR]


def to_pixels(ring, off):
    """the closed coordinate list (first point repeated) as pygame's integer points: int() truncates towards zero like C"""
    pts = [(int(K * float(x) + off[0]), int(K * float(y) + off[1])) for x, y in ring]
    return pts + pts[:1]


def scan_rows(px, py):
    """draw_fillpoly's row loop: yields (y, terms) for the rows inside the surface, terms = [(num, den, x1), ...] in discovery order,
    one per edge the row meets: the intersection is x1 + num / den before the floor / ceil"""
    n, miny, maxy = len(px), min(py), max(py)
    for y in range(max(miny, 0), min(maxy, WIN - 1) + 1):
        terms = []
        for i in range(n):
            ip = i - 1 if i else n - 1
            if py[ip] < py[i]:
                x1, y1, x2, y2 = px[ip], py[ip], px[i], py[i]
            elif py[ip] > py[i]:
                x1, y1, x2, y2 = px[i], py[i], px[ip], py[ip]
            else:
                continue
            if (y1 <= y < y2) or (y == maxy and y2 == maxy):
                terms.append(((y - y1) * (x2 - x1), y2 - y1, x1))
        yield y, terms


def crossings(terms):
    """floor on the 1st, 3rd, ... intersection found, ceil on the others (float32 quotient), then qsort"""
    xs = []
    for k, (num, den, x1) in enumerate(terms):
        q = np.float32(num) / np.float32(den)
        xs.append(int(math.floor(q) if k % 2 == 0 else math.ceil(q)) + x1)
    return sorted(xs)


def _hline(surf, ident, xa, y, xb):
    if y < 0 or y >= WIN:
        return
    if xb < xa:
        xa, xb = xb, xa
    xa, xb = max(xa, 0), min(xb, WIN - 1)
    if xb < 0 or xa >= WIN:
        return
    surf[y, xa:xb + 1] = ident


def fill_polygon(surf, pts, ident):
    px, py = [p[0] for p in pts], [p[1] for p in pts]
    miny, maxy = min(py), max(py)
    if miny == maxy:
        _hline(surf, ident, min(px), miny, max(px))
        return
    for y, terms in scan_rows(px, py):
        xs = crossings(terms)
        for i in range(0, len(xs) - 1, 2):
            _hline(surf, ident, xs[i], y, xs[i + 1])
    for i in range(len(px)):
        ip = i - 1 if i else len(px) - 1
        if miny < py[i] < maxy and py[ip] == py[i]:
            _hline(surf, ident, px[i], py[i], px[ip])


def _set_at(surf, x, y, ident):
    if 0 <= x < WIN and 0 <= y < WIN:
        surf[y, x] = ident


def walk_line(surf, x1, y1, x2, y2, ident):
    """draw_line: the Bresenham walk itself"""
    dx, dy = abs(x2 - x1), abs(y2 - y1)
    sx, sy = (1 if x1 < x2 else -1), (1 if y1 < y2 else -1)
    e = dx if dx > dy else -dy
    err = -((-e) // 2) if e < 0 else e // 2                    # C division truncates towards zero
    while (x1, y1) != (x2, y2):
        _set_at(surf, x1, y1, ident)
        e2 = err
        if e2 > -dx:
            err -= dy
            x1 += sx
        if e2 < dy:
            err += dx
            y1 += sy
    _set_at(surf, x2, y2, ident)


def outline_polygon(surf, pts, ident):
    for a, b in zip(pts[:-1], pts[1:]):
        walk_line(surf, a[0], a[1], b[0], b[1], ident)
    walk_line(surf, pts[-1][0], pts[-1][1], pts[0][0], pts[0][1], ident)


def literal_world(scene, pose, traj):
    """_render: obstacles -> start outline -> dest -> vehicle -> the last 20 trajectory boxes (TRAJ_COLORS by recency), ids as in
    the oracle's header.  traj = vehicle.trajectory, oldest first (entries before the last 20 may be missing)."""
    off = offsets(scene.bbox)
    surf = np.zeros((WIN, WIN), np.uint8)
    for v, n in zip(scene.verts, scene.nvert):
        fill_polygon(surf, to_pixels(v[:int(n)], off), 1)
    outline_polygon(surf, to_pixels(car_corners(scene.start), off), 2)
    fill_polygon(surf, to_pixels(car_corners(scene.dest), off), 3)
    fill_polygon(surf, to_pixels(car_corners(pose), off), 4)
    traj = list(traj)
    if len(traj) > 1:
        last = traj[-TRAJ_DRAWN:]
        for i, p in enumerate(last):
            fill_polygon(surf, to_pixels(car_corners(p), off), 5 + TRAJ_DRAWN - len(last) + i)
    return surf


def quarter_turns(heading):
    """None, or rotate90's number of quarter turns when the heading is an exact multiple of 90 degrees as a C float"""
    angle = np.float32(float(heading) * (180.0 / math.pi))
    if math.fmod(float(angle), 90.0) != 0.0:
        return None
    q = int(angle)
    t = int(math.fmod(abs(q) // 90 * (1 if q >= 0 else -1), 4))            # C's / and % truncate towards zero
    return t + 4 if t < 0 else t


def _blit_origin(bbox, pose):
    """crop pixel (x, y) shows pixel (rx0 + x, ry0 + y) of the rotated surface: Rect placement and the two integer blits"""
    off = offsets(bbox)
    box = car_corners(pose)
    ln = sx = sy = 0.0                                                     # LinearRing.centroid: length-weighted segment midpoints
    for i in range(4):
        p, q = box[i], box[(i + 1) % 4]
        seg = math.sqrt((p[0] - q[0]) ** 2 + (p[1] - q[1]) ** 2)
        ln += seg
        sx += seg * ((p[0] + q[0]) / 2)
        sy += seg * ((p[1] + q[1]) / 2)
    vcx, vcy = K * (sx / ln) + off[0], K * (sy / ln) + off[1]
    c, s = math.cos(pose[2]), math.sin(pose[2])
    ddx = (vcx - WIN / 2) * c + (vcy - WIN / 2) * s
    ddy = -(vcx - WIN / 2) * s + (vcy - WIN / 2) * c
    return CROP_OFF - int(-ddx), CROP_OFF - int(-ddy)


def literal_quarter_image(world, bbox, pose):
    """the 64 x 64 x 3 uint8 image for a quarter-turn heading: np.rot90, the blits, the crop, white -> black, (s + 2) >> 2"""
    t = quarter_turns(pose[2])
    assert t is not None
    rot = np.rot90(world, t)
    rx0, ry0 = _blit_origin(bbox, pose)
    ids = np.zeros((CROP, CROP), np.int64)
    ys, xs = np.arange(CROP) + ry0, np.arange(CROP) + rx0
    oky, okx = (ys >= 0) & (ys < WIN), (xs >= 0) & (xs < WIN)
    ids[np.ix_(oky, okx)] = rot[np.ix_(ys[oky], xs[okx])]
    rgb = PALETTE[ids]
    s = rgb[1::4, 1::4] + rgb[1::4, 2::4] + rgb[2::4, 1::4] + rgb[2::4, 2::4]
    return ((s + 2) >> 2).astype(np.uint8)


def sampled_world_pixels(bbox, pose):
    """the set of world pixels the image observes at a quarter-turn heading, as a 500 x 500 bool mask [y, x]"""
    t = quarter_turns(pose[2])
    assert t is not None
    rx0, ry0 = _blit_origin(bbox, pose)
    u = np.arange(OUT)
    c = np.sort(np.r_[4 * u + 1, 4 * u + 2])
    ys, xs = c + ry0, c + rx0
    rot_mask = np.zeros((WIN, WIN), bool)
    rot_mask[np.ix_(ys[(ys >= 0) & (ys < WIN)], xs[(xs >= 0) & (xs < WIN)])] = True
    return np.rot90(rot_mask, -t)


# ====================================================================================================================
# lots
# ====================================================================================================================
BBOX = np.array([-20.0, 21.0, -20.0, 21.0])     # off = 244 on both axes
OFFP = 244.0
FAR_PX = (440, 440, 0.4)


def wq(p):
    """world coordinate a quarter pixel inside pixel p (truncation towards zero gives p back)"""
    return (p + (0.25 if p >= 0 else -0.25) - OFFP) / K


def wr(p):
    """world coordinate of the raw pixel position p"""
    return (p - OFFP) / K


def ring(pts):
    """3 or 4 pixel points -> a 4-vertex slot (triangles repeat their last vertex) and its vertex count"""
    v = np.array([(wq(x), wq(y)) for x, y in pts], float)
    return (v, 4) if len(v) == 4 else (np.vstack([v, v[2:3]]), 3)


def rect(x0, y0, x1, y1):
    return [(x0, y0), (x1, y0), (x1, y1), (x0, y1)]


def make_lot(polys, start_px, dest_px=FAR_PX, bbox=BBOX, raw=()):
    slots = [ring(p) for p in polys] + [(np.asarray(r, float), 4) for r in raw]
    if not slots:
        slots = [ring(rect(-300, -300, -296, -296))]
    off = offsets(bbox)
    pose = lambda p: np.array([(p[0] - off[0]) / K, (p[1] - off[1]) / K, p[2]])
    return Scene(start=pose(start_px), dest=pose(dest_px), bbox=np.array(bbox, float), verts=np.stack([s[0] for s in slots]),
                 nvert=np.array([s[1] for s in slots], np.int32), level='Normal')


def pixel_rings(scene):
    off = offsets(scene.bbox)
    return [to_pixels(v[:int(n)], off)[:-1] for v, n in zip(scene.verts, scene.nvert)]


def shapes_box(scene, which=None):
    """(x0, y0, x1, y1): the box around the obstacles' integer vertices, clipped to the surface; None when nothing is inside"""
    rings = pixel_rings(scene)
    boxes = []
    for k, pts in enumerate(rings):
        x0, y0 = max(min(p[0] for p in pts), 0), max(min(p[1] for p in pts), 0)
        x1, y1 = min(max(p[0] for p in pts), WIN - 1), min(max(p[1] for p in pts), WIN - 1)
        if (which is None or k in which) and x0 <= x1 and y0 <= y1:
            boxes.append((x0, y0, x1, y1))
    if not boxes:
        return None
    return min(b[0] for b in boxes), min(b[1] for b in boxes), max(b[2] for b in boxes), max(b[3] for b in boxes)


def with_start(scene, start):
    return Scene(start=np.array(start, float), dest=scene.dest.copy(), bbox=scene.bbox.copy(), verts=scene.verts.copy(),
                 nvert=scene.nvert.copy(), level=scene.level)


def _sweep(bbox, pose, box):
    poses = [np.array([pose[0] + i / K, pose[1] + j / K, pose[2]]) for j in range(4) for i in range(4)]
    assert quarter_turns(pose[2]) == 0, 'the sweep observes at heading 0'
    if box is not None:
        seen = np.zeros((WIN, WIN), bool)
        for p in poses:
            seen |= sampled_world_pixels(bbox, p)
        assert seen[box[1]:box[3] + 1, box[0]:box[2] + 1].all(), f'the sweep leaves pixels of {box} unobserved'
    return poses


def observer_sweep(scene, box=None):
    """16 copies of the lot whose start poses differ by 0..3 px in x and in y (heading 0); every world pixel of `box` (default: the
    box around the programmed shapes) is sampled by at least one copy -- asserted"""
    box = shapes_box(scene) if box is None else box
    return [with_start(scene, p) for p in _sweep(scene.bbox, scene.start, box)]


def observer_sweep_detached(scene, observer, box):
    """the same sweep for an observer that is not the start pose: 16 observer poses for one lot"""
    return _sweep(scene.bbox, np.asarray(observer, float), box)


@dataclass
class Family:
    scenes: list
    poses: np.ndarray                # [n, 3] the pose each lot is observed from at reset (the start pose unless detached)
    facts: dict = field(default_factory=dict)
    detached: bool = False           # the tests upload `poses` from outside before the first observation

    def __len__(self):
        return len(self.scenes)


def _family(scenes, poses=None, facts=None):
    detached = poses is not None
    poses = np.array([s.start for s in scenes]) if poses is None else np.array(poses, float)
    return Family(list(scenes), poses, facts or {}, detached)


def _clear_of_vehicle(scene, pose, box, margin=2):
    """the observer's own box must not hide the shapes"""
    v = to_pixels(car_corners(pose), offsets(scene.bbox))
    vx0, vx1, vy0, vy1 = min(p[0] for p in v), max(p[0] for p in v), min(p[1] for p in v), max(p[1] for p in v)
    return vx1 + margin < box[0] or vx0 - margin > box[2] or vy1 + margin < box[1] or vy0 - margin > box[3]


def _observer_for(box):
    """pose pixel of an observer 30 px below (or above) the box, centred on it"""
    cx = (box[0] + box[2]) // 2 - 17
    below = box[3] + 30
    if below - 124 <= box[1]:
        return (cx, below, 0.0)
    above = box[1] - 30
    assert above + 124 >= box[3], f'{box} does not fit the crop'
    return (cx, above, 0.0)


# ====================================================================================================================
# polygons()
# ====================================================================================================================
ARROW = [(100, 100), (120, 115), (140, 100), (120, 140)]
BOWTIE = [(150, 100), (190, 140), (190, 100), (150, 140)]
INNER_EDGE = [(200, 100), (230, 120), (260, 120), (220, 150)]


def four_rows(pts):
    return sum(len(t) == 4 for _, t in scan_rows([p[0] for p in pts] + [pts[0][0]], [p[1] for p in pts] + [pts[0][1]]))


def border_pass_rows(pts):
    px, py = [p[0] for p in pts] + [pts[0][0]], [p[1] for p in pts] + [pts[0][1]]
    return [(px[i], py[i], px[i - 1]) for i in range(1, len(px)) if min(py) < py[i] < max(py) and py[i - 1] == py[i] and px[i - 1] != px[i]]


def polygon_lots(pad=0, with_many=True):
    """[(lot without observer, box to observe or None for the shapes' box)]; pad: that many obstacles outside the surface go first"""
    lots = []
    shapes = [ARROW, BOWTIE, INNER_EDGE,
              [(270, 100), (300, 110), (280, 135)], [(305, 140), (330, 104), (318, 101)],          # triangles (nv == 3)
              [(100, 150), (130, 150), (140, 150), (110, 150)],                                      # one row
              [(150, 150), (150, 150), (150, 150), (150, 150)],                                      # one pixel
              [(160, 145), (180, 165), (200, 185), (180, 165)]]                                      # zero area
    lots.append((shapes, None))
    spans = [rect(100 + 37 * (w % 5) + w % 4, 100 + 9 * (w // 5), 100 + 37 * (w % 5) + w % 4 + w - 1, 100 + 9 * (w // 5) + 2 + w % 3)
             for w in range(1, 21)]
    lots.append((spans, None))
    wall = [rect(-20, 200, 520, 203), [(-30, 210), (530, 212), (530, 214), (-30, 215)]]
    for box in ((0, 200, 170, 215), (171, 200, 330, 215), (331, 200, 499, 215)):
        lots.append((wall, box))
    # band seams (16 rows) and block seams (32 columns) of the packed layer: next to the origin and in the middle
    for bx, by in ((0, 0), (96, 96)):
        lots.append(([rect(bx + 28, by + 14, bx + 35, by + 16), rect(bx + 40, by + 16, bx + 44, by + 17), rect(bx + 31, by + 20, bx + 32, by + 24),
                      [(bx + 50, by + 20), (bx + 62, by + 20), (bx + 56, by + 32)], rect(bx + 66, by + 15, bx + 70, by + 15),
                      [(bx + 75, by + 9), (bx + 90, by + 31), (bx + 64, by + 33), (bx + 80, by + 48)]], None))
    # partly outside each of the four surface edges, wholly outside, vertices in (-1, 0) px, surface pixel (0, 0)
    out = [rect(-100, -100, -50, -50), rect(600, 100, 650, 130), rect(100, 600, 130, 640)]
    lots.append(([rect(-30, 100, 20, 120), [(-25, 130), (30, 140), (-5, 160)]] + out, None))
    lots.append(([rect(480, 100, 530, 120), [(470, 130), (540, 150), (490, 165)]] + out, None))
    lots.append(([rect(100, -30, 120, 20), [(130, -25), (160, 5), (140, 30)]] + out, None))
    lots.append(([rect(100, 480, 120, 530), [(130, 470), (150, 540), (165, 490)]] + out, None))
    lots.append(([rect(-5, -5, 6, 6)] + out, None))
    lots = [(make_lot([rect(-300 - 3 * k, -300, -299 - 3 * k, -298) for k in range(pad)] + polys, (0, 0, 0.0)), box) for polys, box in lots]
    # vertices whose pixel coordinate lies in (-1, 0): they fold onto 0
    fold = np.array([[wr(-0.5), wr(60.0)], [wr(9.5), wr(60.5)], [wr(9.5), wr(70.5)], [wr(-0.75), wr(70.5)]])
    fold2 = np.array([[wr(60.5), wr(-0.5)], [wr(70.5), wr(-0.25)], [wr(70.5), wr(9.5)], [wr(60.5), wr(9.5)]])
    lots.append((make_lot([rect(-300 - 3 * k, -300, -299 - 3 * k, -298) for k in range(pad)], (0, 0, 0.0), raw=[fold, fold2]), None))
    if with_many:
        # 70 small obstacles inside one band of 16 rows (two obstacle chunks) + a 71st under the start outline and the dest box
        many = [rect(20 + 6 * (k % 35), 160 + 8 * (k // 35) + k % 3, 23 + 6 * (k % 35) + k % 2, 164 + 8 * (k // 35) + k % 4) for k in range(70)]
        lot = make_lot(many + [rect(90, 150, 170, 190)], (100, 168, 0.0), dest_px=(112, 175, 0.3))
        lots.append((lot, (20, 140, 232, 205)))
    return lots


def polygons(pad=0):
    scenes, poses, facts = [], [], {}
    lots = polygon_lots(pad, with_many=pad == 0)
    for k, (lot, box) in enumerate(lots):
        many = pad == 0 and k == len(lots) - 1
        box = box if box is not None else shapes_box(lot, which=range(pad, len(lot.verts)))
        obs = _observer_for(box)
        off = offsets(lot.bbox)
        obs_pose = np.array([(obs[0] - off[0]) / K, (obs[1] - off[1]) / K, 0.0])
        if many:                                  # the start stays under the 71st obstacle: the observer is detached
            for p in observer_sweep_detached(lot, obs_pose, box):
                scenes.append(lot)
                poses.append(p)
                assert _clear_of_vehicle(lot, p, box)
        else:
            for s in observer_sweep(with_start(lot, obs_pose), box):
                scenes.append(s)
                poses.append(s.start)
                assert _clear_of_vehicle(s, s.start, box)
    facts['four_rows'] = {name: four_rows(p) for name, p in (('arrow', ARROW), ('bowtie', BOWTIE))}
    facts['border_pass'] = border_pass_rows(INNER_EDGE)
    w = literal_world(lots[1][0], np.array([1e4, 1e4, 0.0]), [])
    widths = set()
    for row in (w == 1):
        edges = np.diff(np.r_[0, row.astype(np.int8), 0])
        widths |= set((np.nonzero(edges == -1)[0] - np.nonzero(edges == 1)[0]).tolist())
    facts['span_widths'] = widths
    facts['wall'] = int((literal_world(lots[2][0], np.array([1e4, 1e4, 0.0]), [])[201] == 1).sum())
    # (one lot has a detached observer, so the family has: for the others the uploaded pose is the start pose itself)
    return Family(scenes, np.array(poses), facts, detached=True)


# ====================================================================================================================
# truncation()
# ====================================================================================================================
def boundary_triple(f, x0, p):
    """x_lo, x_eq, x_hi: neighbouring doubles around x0 with f(x_eq) == p exactly, f(x_lo) the first value below p, x_hi = the
    double after x_eq -- or None when no double near x0 hits p exactly"""
    x = x0
    for _ in range(64):
        v = f(x)
        if v == p:
            break
        x = np.nextafter(x, np.inf if v < p else -np.inf)
    else:
        return None
    lo = x
    while f(lo) >= p:
        lo = np.nextafter(lo, -np.inf)
    return float(lo), float(x), float(np.nextafter(x, np.inf))


def truncation():
    scenes, poses, facts = [], [], {'obstacle': [], 'dest': [], 'start': []}
    for bbox in (BBOX, np.array([-20.03, 21.0, -20.0, 21.07])):             # off = 244 / a non-integer off
        off = offsets(bbox)
        tri = None
        for p in range(300, 340):
            tri = boundary_triple(lambda x: K * x + off[0], (p - off[0]) / K, float(p))
            if tri:
                break
        assert tri, 'no exact product for this map box'
        px = [int(K * x + off[0]) for x in tri]
        facts['obstacle'].append((px, p))
        for x in tri:                              # a rectangle whose left edge and (transposed) top edge sit on the boundary
            ya = (100.25 - off[1]) / K
            ob = np.array([[x, ya], [x + 1.0, ya], [x + 1.0, ya + 0.5], [x, ya + 0.5]])
            yt = boundary_triple(lambda y: K * y + off[1], (130 - off[1]) / K, 130.0)
            y = yt[tri.index(x)] if yt else (130.25 - off[1]) / K
            ob2 = np.array([[x - 2.0, y], [x - 1.5, y], [x - 1.5, y + 0.5], [x - 2.0, y + 0.5]])
            lot = make_lot([], (0, 0, 0.0), bbox=bbox, raw=[ob, ob2])
            box = shapes_box(lot)
            o = _observer_for(box)
            for s in observer_sweep(with_start(lot, [(o[0] - off[0]) / K, (o[1] - off[1]) / K, 0.0]), box):
                scenes.append(s)
                poses.append(s.start)
    off = offsets(BBOX)
    for kind in ('dest', 'start'):
        for p in (300, 301, 302, 303) if kind == 'start' else (300,):
            # rear-right corner of a box at heading 0: x = 1 * (-REAR_HANG) + (-0) * (-WIDTH / 2) + px
            f = lambda x: K * (1.0 * CAR[0][0] + (-0.0) * CAR[0][1] + x) + off[0]
            tri = None
            for q in range(p, p + 400, 4):
                tri = boundary_triple(f, (q - off[0]) / K + REAR_HANG, float(q))
                if tri:
                    break
            assert tri
            facts[kind].append(([int(f(x)) for x in tri], q))
            for x in tri:
                y = (150.4 - off[1]) / K
                if kind == 'dest':
                    lot = make_lot([], (0, 0, 0.0))
                    lot.dest = np.array([x, y, 0.0])
                    c = to_pixels(car_corners(lot.dest), off)
                    box = (min(a[0] for a in c), min(a[1] for a in c), max(a[0] for a in c), max(a[1] for a in c))
                    o = _observer_for(box)
                    for s in observer_sweep(with_start(lot, [(o[0] - off[0]) / K, (o[1] - off[1]) / K, 0.0]), box):
                        scenes.append(s)
                        poses.append(s.start)
                else:
                    lot = make_lot([], (0, 0, 0.0))
                    scenes.append(with_start(lot, [x, y, 0.0]))
                    poses.append(scenes[-1].start)
    return _family(scenes, None, facts)


# ====================================================================================================================
# outlines()
# ====================================================================================================================
def edge_features(pts):
    """what the four edges of an integer box realise for draw_line"""
    out = set()
    for (xa, ya), (xb, yb) in zip(pts, pts[1:] + pts[:1]):
        dx, dy = abs(xb - xa), abs(yb - ya)
        if dx == 0:
            out.add('dx0')
        if dy == 0:
            out.add('dy0')
        if dx and dy:
            if dx == dy:
                out.add('diag')
            if dx == dy + 1:
                out.add('diag+1')
            if dx == dy - 1:
                out.add('diag-1')
            major, minor = (dx, dy) if dx > dy else (dy, dx)
            out.add('odd' if major % 2 else 'even')
            if any((k * minor - major // 2) % major == 0 for k in range(1, major)):
                out.add('tie')
    return out


OUTLINE_FEATURES = {'dx0', 'dy0', 'diag', 'diag+1', 'diag-1', 'odd', 'even', 'tie'}


def outlines():
    off = offsets(BBOX)
    want, chosen, feats = set(OUTLINE_FEATURES), [], {}
    cands = [(h, sub) for h in np.r_[0.0, np.linspace(0.0, 2 * np.pi, 1441)[1:-1]] for sub in (0.0, 0.4)]
    for h, sub in cands:
        start = np.array([(250 + sub - off[0]) / K, (150 + sub - off[1]) / K, h])
        f = edge_features(to_pixels(car_corners(start), off)[:-1])
        if f & want:
            want -= f
            chosen.append(start)
            feats[len(chosen) - 1] = f
        if not want:
            break
    scenes, poses = [], []
    for start in chosen:
        lot = with_start(make_lot([], (0, 0, 0.0)), start)
        c = to_pixels(car_corners(start), off)
        box = (min(a[0] for a in c), min(a[1] for a in c), max(a[0] for a in c), max(a[1] for a in c))
        o = _observer_for(box)
        for p in observer_sweep_detached(lot, [(o[0] - off[0]) / K, (o[1] - off[1]) / K, 0.0], box):
            assert _clear_of_vehicle(lot, p, box)
            scenes.append(lot)
            poses.append(p)
    return _family(scenes, poses, {'missing': want, 'features': feats})


# ====================================================================================================================
# headings()
# ====================================================================================================================
QUARTER_DEGREES = (0, 90, -90, 180, -180, 270, -270, 360, -360, 450, -450, 720)


def heading_of_degrees(d32):
    """a heading whose rad2deg, parsed as a C float, is d32"""
    h = float(np.float64(d32) * math.pi / 180.0)
    for _ in range(8):
        a = np.float32(h * (180.0 / math.pi))
        if a == d32:
            return h
        h = float(np.nextafter(h, np.inf if a < d32 else -np.inf))
    raise AssertionError(f'{d32!r} degrees is not reachable')


def headings():
    polys = [rect(270, 260, 320, 285), rect(180, 190, 200, 290), [(250, 320), (290, 327), (262, 345)], [(215, 215), (245, 205), (260, 222), (225, 240)]]
    scenes, poses, facts = [], {}, {'quarter': [], 'general': [], 'corner': []}
    for d in QUARTER_DEGREES:
        for side in (-1, 0, 1):
            d32 = np.float32(d) if side == 0 else np.nextafter(np.float32(d), np.float32(side * np.inf))
            h = heading_of_degrees(d32)
            lot = make_lot(polys, (252, 250, h), dest_px=(300, 200, 0.4))
            facts['quarter' if quarter_turns(h) is not None else 'general'].append(len(scenes))
            assert (quarter_turns(h) is not None) == (side == 0), (d, side)
            scenes.append(lot)
    for h in (7.0, -7.0, 20.0, -20.0):
        facts['general'].append(len(scenes))
        scenes.append(make_lot(polys, (252, 250, h), dest_px=(300, 200, 0.4)))
    # the vehicle near each surface corner and edge: the crop leaves the rotated surface and the source.  Surface pixel (0, 0) is
    # in turn empty, under an obstacle, under the dest box, under the start outline and under the vehicle
    q = [heading_of_degrees(np.float32(d)) for d in (0, 90, 180, -90)]
    for what in ('empty', 'obstacle', 'dest', 'start', 'vehicle'):
        corner_polys = polys + ([rect(-4, -4, 5, 3)] if what == 'obstacle' else [])
        dest = (-20, -6, 0.0) if what == 'dest' else (300, 200, 0.4)
        for px_, py_ in ((40, 45), (470, 35), (30, 465), (465, 470), (250, 20), (20, 250), (480, 250), (250, 480)):
            for h in (0.7, -2.3, q[len(scenes) % 4]):
                observer = None
                if what == 'vehicle':                        # the box's middle (17 px ahead of the pose) on pixel (0, 0)
                    if (px_, py_) != (40, 45):
                        continue
                    start = (-17.0 * math.cos(h), -17.0 * math.sin(h), h)
                elif what == 'start':                        # heading 0: the rear right corner (-11.16, -11.64 px) lands on (0, 0)
                    if (px_, py_) != (40, 45):
                        continue
                    start, observer = (11.5, 12.0, 0.0), (px_ + 30, py_ + 25, h)
                else:
                    start = (px_, py_, h)
                if quarter_turns(h) is None:
                    facts['corner'].append((len(scenes), what))
                else:
                    facts['quarter'].append(len(scenes))
                scenes.append(make_lot(corner_polys, start, dest_px=dest))
                off = offsets(BBOX)
                poses[len(scenes) - 1] = np.array([(observer[0] - off[0]) / K, (observer[1] - off[1]) / K, observer[2]]) if observer else None
    allp = [scenes[k].start if poses.get(k) is None else poses[k] for k in range(len(scenes))]
    return _family(scenes, allp, facts)


# ====================================================================================================================
# trails() and shown_vehicle()
# ====================================================================================================================
TRAIL_BBOX = np.array([-30.0, 31.0, -30.0, 31.0])     # off = 244; the map is larger than the surface


@dataclass
class Drive:
    family: Family
    actions: np.ndarray              # [steps, n, 2]
    replace: np.ndarray = None       # shown_vehicle: [n, 3] added to the pose after the drive


def _empty_lot(start_px, wall=None):
    polys = [rect(590, 590, 600, 600)] + ([wall] if wall else [])              # (off the surface, inside the map)
    return make_lot(polys, start_px, dest_px=(600, 20, 0.0), bbox=TRAIL_BBOX)


TRAIL_SPEEDS = np.round(np.linspace(0.66, 0.74, 33), 4)


def trails(long=False):
    """long=False: 40 steps -- straight and diagonal drives at the speeds that make the box around the 20 drawn boxes 255, 256 and
    257 px wide / high (x1 - x0 = 254, 255, 256: the last is the first that cannot live on the torus), drives against a wall (steps
    that keep no sub-step), all across the torus seams x, y = 256.  long=True: 16 slow drives of 200 steps that pass entries 96, 97,
    192 and 193 on a seam."""
    scenes, acts = [], []
    if long:
        steps = 200
        for axis in (0, 1):
            for speed, p0 in ((0.1, 100), (0.1, 110), (0.052, 95), (0.052, 160), (0.12, 60), (0.08, 40), (0.1, 250), (0.06, 200)):
                h = 0.0 if axis == 0 else heading_of_degrees(np.float32(90))
                scenes.append(_empty_lot((p0, 240 + len(scenes), h) if axis == 0 else (240 + len(scenes), p0, h)))
                acts.append(np.tile([0.0, speed], (steps, 1)))
    else:
        steps = 40
        q1 = heading_of_degrees(np.float32(90))
        for sp in TRAIL_SPEEDS:
            scenes.append(_empty_lot((40, 230, 0.0)))
            acts.append(np.tile([0.0, sp], (steps, 1)))
            scenes.append(_empty_lot((250, 40, q1)))
            acts.append(np.tile([0.0, sp], (steps, 1)))
        for h, p in ((math.pi / 4, (60, 60)), (-3 * math.pi / 4, (420, 430)), (math.pi, (460, 250)), (0.3, (40, 150)), (-1.2, (200, 470))):
            for sp in (1.0, 0.7, 0.4):
                scenes.append(_empty_lot((p[0], p[1], h)))
                acts.append(np.tile([0.0, sp], (steps, 1)))
        # out of the map within a dozen steps (episodes that end: the torus is cleared at the turnover), over each low surface edge too
        for p in ((440, 250, 0.0), (250, 440, q1), (60, 250, math.pi), (250, 60, -q1)):
            scenes.append(_empty_lot(p))
            acts.append(np.tile([0.0, 1.0], (steps, 1)))
        # a wall ahead: the car stops in front of it and every later step keeps no sub-step; then it backs off across the seam
        for gap in (300, 301, 303, 306, 310, 317):
            scenes.append(_empty_lot((150, 250, 0.0), wall=rect(gap, 200, gap + 6, 300)))
            a = np.tile([0.0, 1.0], (steps, 1))
            a[25:, 1] = -0.5
            a[:, 0] = 0.0
            acts.append(a)
    return Drive(_family(scenes), np.stack(acts, 1))


def shown_vehicle():
    """24 steps straight at the trail speeds, then the pose is replaced from outside: 1..3 px off the newest entry (the vehicle box
    shows as a rim under the newest trajectory boxes) or back at the OLDEST drawn box, so that the far end of a live set as wide as the
    torus is observed (moved by 0..3 px: the sweep)."""
    scenes, acts, rep = [], [], []
    q1 = heading_of_degrees(np.float32(90))
    for k, sp in enumerate(TRAIL_SPEEDS[::2]):
        for axis in (0, 1):
            for sweep in range(4):
                scenes.append(_empty_lot((40, 230, 0.0) if axis == 0 else (250, 40, q1)))
                acts.append(np.tile([0.0, sp], (24, 1)))
                back = -(19 * 15 * sp + sweep) / K             # 15 px per step at full speed: 19 steps back to the oldest drawn box
                side = ((k + sweep) % 4) / K
                rep.append([back, side, 0.0] if axis == 0 else [side, back, 0.0])
    for k in range(8):                                         # a rim of 1..3 px of the vehicle box under the newest boxes
        scenes.append(_empty_lot((40, 230, 0.0) if k % 2 == 0 else (250, 40, q1)))
        acts.append(np.tile([0.0, 0.7], (24, 1)))
        rep.append([(1 + k % 3) / K * (-1) ** (k // 2), (k % 4 - 1) / K, 0.0])
    for h in (0.5, -2.0):
        for d in ((0.3, 0.2, 0.0), (-0.5, 0.1, 0.05), (0.1, -0.6, -0.1), (2.0, 1.0, 0.4)):
            scenes.append(_empty_lot((250, 250, h)))
            acts.append(np.tile([0.3, 0.5], (24, 1)))
            rep.append(d)
    return Drive(_family(scenes), np.stack(acts, 1), np.array(rep))


def live_box(scene, traj):
    """box around the integer corners of the (at most 20) drawn trajectory boxes: x0, x1, y0, y1"""
    off = offsets(scene.bbox)
    pts = [p for e in list(traj)[-TRAJ_DRAWN:] for p in to_pixels(car_corners(e), off)]
    return min(p[0] for p in pts), max(p[0] for p in pts), min(p[1] for p in pts), max(p[1] for p in pts)


# ====================================================================================================================
# F_SIMPLE for car boxes
# ====================================================================================================================
def car_box_is_simple(pts):
    """pts: closed integer box.  More than one row, every row exactly two intersections, the border pass inside the row's span"""
    px, py = [p[0] for p in pts], [p[1] for p in pts]
    n, miny, maxy = len(px), min(py), max(py)
    if miny == maxy:
        return False
    spans = {}
    for y in range(miny, maxy + 1):
        terms = []
        for i in range(n):
            ip = i - 1 if i else n - 1
            if py[ip] == py[i]:
                continue
            (x1, y1), (x2, y2) = sorted(((px[ip], py[ip]), (px[i], py[i])), key=lambda a: a[1])
            if (y1 <= y < y2) or (y == maxy and y2 == maxy):
                terms.append(((y - y1) * (x2 - x1), y2 - y1, x1))
        if len(terms) != 2:
            return False
        spans[y] = crossings(terms)
    for i in range(n):
        ip = i - 1 if i else n - 1
        if miny < py[i] < maxy and py[ip] == py[i]:
            a, b = spans[py[i]]
            if not (a <= min(px[i], px[ip]) and max(px[i], px[ip]) <= b):
                return False
    return True


def search_non_simple_car_box(n_head=3600, subs=(0.0, 0.25, 0.5, 0.75)):
    off = offsets(BBOX)
    bad = []
    for k in range(n_head):
        h = k * 2 * math.pi / n_head
        for base in ((250, 250), (-10, 250), (250, -10), (-10, -10)):
            for sx in subs:
                for sy in subs:
                    pose = ((base[0] + sx - off[0]) / K, (base[1] + sy - off[1]) / K, h)
                    if not car_box_is_simple(to_pixels(car_corners(pose), off)):
                        bad.append(pose)
    return bad
