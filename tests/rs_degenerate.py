"""Deterministic lattice of exactly aligned and degenerate poses for the Reeds-Shepp search (no RNG).

The same cases serve the fixture generator (tests/golden/make_golden_r2.py `rsdegen`), the CPU test
(tests/test_rs_degenerate.py) and the GPU test (tests/test_gpu_rs_degenerate.py); tests/golden/rs_degenerate.npz holds
only the reference's results, the poses and obstacles are rebuilt from here.

Lattice: 3 goal headings x 8 offset directions (goal frame) x 9 distances x 10 relative headings = 2 160 poses, each
with up to three obstacle variants; plus a small gate group at planar distance 10.0 and its two float64 neighbours.
"""
import math

import numpy as np

from hope_amd import tables as T

MAXC = 0.3327130214085973                       # math.tan(VALID_STEER[-1]) / WHEEL_BASE (car_parking_base.py:422)
GOAL_XY = (40.0, 25.0)                          # non-origin, so that world coordinates are not trivially exact
GOAL_YAWS = (0.0, math.pi / 2, 0.3)
DISTANCES = (0.5, 1.0, 2.0, 3.0, 1 / MAXC, 2 / MAXC, 4 / MAXC, 6.0, 9.5)
_D = math.sqrt(0.5)
DIRECTIONS = ((1.0, 0.0), (-1.0, 0.0), (0.0, 1.0), (0.0, -1.0), (_D, _D), (_D, -_D), (-_D, _D), (-_D, -_D))
REL_HEADINGS = (0.0, math.pi / 2, -math.pi / 2, math.pi, -math.pi, math.pi / 4, 3 * math.pi / 4, 1e-9, -1e-9,
                0.99 * math.pi)
SQUARE = 0.6                                    # obstacle side (m)
SIDE = 1.5                                      # variant (c): distance of the second square from the first
MAP_HALF = 30.0
VARIANT_NONE, VARIANT_SQUARE, VARIANT_ROTATED_PAIR = 0, 1, 2


def rotate(yaw, x, y):
    """goal frame -> world offset; the quarter turn is exact (cos(pi/2) is 6e-17 in floating point, not 0)"""
    if yaw == 0.0:
        return x, y
    if yaw == math.pi / 2:
        return -y, x
    c, s = math.cos(yaw), math.sin(yaw)
    return c * x - s * y, s * x + c * y


def square(cx, cy, yaw=0.0, side=SQUARE):
    h = side / 2
    return np.array([(cx + dx, cy + dy) for dx, dy in (rotate(yaw, a, b) for a, b in ((-h, -h), (h, -h), (h, h), (-h, h)))])


def car_box(pose):
    c, s = math.cos(pose[2]), math.sin(pose[2])
    return np.array([(c * x - s * y + pose[0], s * x + c * y + pose[1]) for x, y in T.VEHICLE_BOX])


def convex_overlap(a, b):
    """separating-axis test of two convex polygons (touching counts as overlap)"""
    for poly in (a, b):
        for k in range(len(poly)):
            e = poly[(k + 1) % len(poly)] - poly[k]
            ax = np.array([-e[1], e[0]])
            pa, pb = a @ ax, b @ ax
            if pa.max() < pb.min() or pb.max() < pa.min():
                return False
    return True


def map_box(goal):
    """ParkingMapDLP.reset's floor / ceil (parking_map_dlp.py:64-67) around goal +/- MAP_HALF"""
    return np.array([math.floor(goal[0] - MAP_HALF), math.ceil(goal[0] + MAP_HALF),
                     math.floor(goal[1] - MAP_HALF), math.ceil(goal[1] + MAP_HALF)])


def gate_distance(pose, goal):
    """|pos - dest| as the gate evaluates it (car_parking_base.py:293-294; k_rs_compact; orc_env_step_physical)"""
    dx, dy = pose[0] - goal[0], pose[1] - goal[1]
    return math.sqrt(dx * dx + dy * dy)


def _variants(pose, goal):
    """obstacle rings of the variants that keep the car box clear at the start and at the goal"""
    out = [(VARIANT_NONE, [])]
    mx, my = 0.5 * (pose[0] + goal[0]), 0.5 * (pose[1] + goal[1])
    ux, uy = goal[0] - pose[0], goal[1] - pose[1]
    n = math.hypot(ux, uy)
    sx, sy = -uy / n * SIDE, ux / n * SIDE                     # to the left of the chord
    cand = [(VARIANT_SQUARE, [square(mx, my)]),
            (VARIANT_ROTATED_PAIR, [square(mx, my, goal[2]), square(mx + sx, my + sy, goal[2])])]
    boxes = (car_box(pose), car_box(goal))
    for v, rings in cand:
        if not any(convex_overlap(r, b) for r in rings for b in boxes):
            out.append((v, rings))
    return out


def cases():
    """list of dicts: pose, goal, bbox, rings, variant, lattice (index of the pose or -1), gate, t (value AFTER the step's
    increment: the gate needs t > 1)"""
    out = []
    k = 0
    for gyaw in GOAL_YAWS:
        goal = np.array([GOAL_XY[0], GOAL_XY[1], gyaw])
        for dx, dy in DIRECTIONS:
            for dist in DISTANCES:
                ox, oy = rotate(gyaw, dx * dist, dy * dist)
                for rel in REL_HEADINGS:
                    pose = np.array([goal[0] + ox, goal[1] + oy, gyaw + rel])
                    for v, rings in _variants(pose, goal):
                        out.append(dict(pose=pose, goal=goal, bbox=map_box(goal), rings=rings, variant=v, lattice=k,
                                        gate=False, t=2))
                    k += 1
    # gate group: the offset lies on the y axis below the goal, where pos, pos - dest and sqrt(d * d) are all exact
    goal = np.array([GOAL_XY[0], GOAL_XY[1], 0.0])
    for d in (np.nextafter(10.0, 0.0), 10.0, np.nextafter(10.0, 20.0)):
        for heading in (0.0, math.pi / 2):
            for t in (1, 2):
                pose = np.array([goal[0], goal[1] - d, heading])
                assert gate_distance(pose, goal) == d
                out.append(dict(pose=pose, goal=goal, bbox=map_box(goal), rings=[], variant=VARIANT_NONE, lattice=-1,
                                gate=True, t=t))
    return out


def build(max_obst=32):
    """packed arrays in pack_scenes' layout (start = the pose) plus the per-case labels"""
    cs = cases()
    n = len(cs)
    start, dest, bbox = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((n, 4))
    verts = np.zeros((n, max_obst, 4, 2))
    n_obst = np.zeros(n, np.int32)
    nvert = np.full((n, max_obst), 4, np.int32)
    for i, c in enumerate(cs):
        start[i], dest[i], bbox[i] = c['pose'], c['goal'], c['bbox']
        n_obst[i] = len(c['rings'])
        for j, r in enumerate(c['rings']):
            verts[i, j] = r
    return dict(n=n, start=start, dest=dest, bbox=bbox, verts=verts, n_obst=n_obst, nvert=nvert,
                variant=np.array([c['variant'] for c in cs], np.int8), lattice=np.array([c['lattice'] for c in cs], np.int32),
                gate=np.array([c['gate'] for c in cs]), t=np.array([c['t'] for c in cs], np.int32),
                gate_d=np.array([gate_distance(c['pose'], c['goal']) for c in cs]))
