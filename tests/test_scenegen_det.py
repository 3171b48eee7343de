"""The deterministic lot generator's host twin (hope_scenegen_generate_det, hope_amd/csrc/hope_scenegen_core.h): the recipe of
hope_scenegen_generate written with exact operations only, so that the HIP kernel k_scenegen reproduces it bit for bit
(tests/test_gpu_scenegen.py).  No GPU needed here.

Distribution criteria: those of tests/test_scenes_distribution.py::test_native_generator_matches_reference_distribution (same
fixture tests/golden/scene_stats.npz, same features, two-sample KS D < 0.065, obstacle-count shares within 0.04)."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from oracle import oracle as O

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'scene_stats.npz')
NAMES = ['n_obst', 'start_x', 'start_y', 'cos_start_yaw', 'sin_start_yaw', 'dest_x', 'dest_y', 'dest_yaw', 'dist_start_dest',
         'gap_nearest', 'gap_second', 'obstacle_area']
CASES = [('Normal', True), ('Complex', True), ('Normal', False), ('Complex', False), ('Extrem', False)]

# sg_log against the platform's log over (0, 1], in units of the last place of the result.  Measured on the sweep of
# test_log_stays_within_the_measured_distance_of_the_platform_log (4.3 M arguments: uniform, log-uniform down to 1e-300, the
# neighbourhoods of 1, 1/2 and sqrt(1/2), the smallest uniforms): worst 2.0 ulp, at x = 0.6936... where e * ln 2 and log(m) cancel
# to a third of their size.  The sweep is a sample, so the bound is twice the measured worst case.
LOG_WORST_ULP_MEASURED = 2.0
LOG_BOUND_ULP = 2.0 * LOG_WORST_ULP_MEASURED


def features(start, dest, rings):
    dbox = O.create_box(dest)
    gaps = []
    for r in rings:
        d = min(O.pt_seg_dist(p, r[j], r[(j + 1) % len(r)]) for p in dbox for j in range(len(r)))
        d = min(d, min(O.pt_seg_dist(p, dbox[j], dbox[(j + 1) % 4]) for p in r for j in range(4)))
        gaps.append(d)
    gaps = sorted(gaps) + [99.0, 99.0]
    area = sum(O.quad_area(np.asarray(r, float)) for r in rings if len(r) == 4)
    return [len(rings), start[0], start[1], math.cos(start[2]), math.sin(start[2]), dest[0], dest[1], dest[2],
            math.hypot(start[0] - dest[0], start[1] - dest[1]), gaps[0], gaps[1], area]


def ks(a, b):
    a, b = np.sort(a), np.sort(b)
    allv = np.concatenate([a, b])
    return float(np.abs(np.searchsorted(a, allv, side='right') / len(a) - np.searchsorted(b, allv, side='right') / len(b)).max())


def feature_table(arrays):
    start, dest, bbox, verts, nob = arrays[:5]
    return np.array([features(start[i], dest[i], [verts[i, o] for o in range(nob[i])]) for i in range(len(nob))])


def assert_same_distribution(ref, mine, what):
    worst = {}
    for j, name in enumerate(NAMES):
        if np.ptp(ref[:, j]) == 0 and np.ptp(mine[:, j]) == 0:
            assert ref[0, j] == mine[0, j], name
            continue
        worst[name] = ks(ref[:, j], mine[:, j])
    print(what, {k: round(v, 3) for k, v in worst.items()})
    bad = {k: v for k, v in worst.items() if v >= 0.065}
    assert not bad, (what, bad)
    for c in range(0, 14):
        assert abs((ref[:, 0] == c).mean() - (mine[:, 0] == c).mean()) < 0.04, (what, c)


@pytest.mark.parametrize('level,bay', CASES)
def test_twin_matches_reference_distribution_and_the_glibc_generator(level, bay):
    from hope_amd.scene_gen import generate_arrays, generate_arrays_det
    ref = np.load(GOLD)[f'{level}_{"bay" if bay else "par"}']
    n = len(ref)
    out = generate_arrays_det(level, n, seed=1234, max_obst=32, bay_mode=1 if bay else 0, threads=3)
    start, dest, bbox, verts, nob, nvert, cid = out
    assert (cid == (0 if bay else 1)).all()
    assert nob.min() >= 3 and nob.max() <= 17
    mine = feature_table(out)
    assert_same_distribution(ref, mine, f'twin vs reference {level} {"bay" if bay else "parallel"}')
    # the map box rule of ParkingMapNormal.reset (:486-489)
    assert np.array_equal(bbox[:, 0], np.floor(np.minimum(start[:, 0], dest[:, 0]) - 10)) and np.array_equal(bbox[:, 1], np.ceil(np.maximum(start[:, 0], dest[:, 0]) + 10))
    assert np.array_equal(bbox[:, 2], np.floor(np.minimum(start[:, 1], dest[:, 1]) - 10)) and np.array_equal(bbox[:, 3], np.ceil(np.maximum(start[:, 1], dest[:, 1]) + 10))
    # ... and against the glibc generator (other lots: another seed), same criteria
    glibc = generate_arrays(level, n, seed=99, max_obst=32, bay_mode=1 if bay else 0, threads=1)
    assert_same_distribution(feature_table(glibc), mine, f'twin vs glibc generator {level} {"bay" if bay else "parallel"}')


@pytest.mark.parametrize('level', ['Normal', 'Complex', 'Extrem'])
def test_twin_does_not_depend_on_threads_or_on_how_a_range_is_split(level):
    from hope_amd.scene_gen import generate_arrays_det
    n, first = 3000, 2 ** 32 + 77
    one = generate_arrays_det(level, n, seed=7, max_obst=20, first_index=first, threads=1)
    for threads in (2, 5):
        again = generate_arrays_det(level, n, seed=7, max_obst=20, first_index=first, threads=threads)
        assert all(np.array_equal(a, b) for a, b in zip(one, again)), threads
    k = 1234
    a = generate_arrays_det(level, k, seed=7, max_obst=20, first_index=first, threads=2)
    b = generate_arrays_det(level, n - k, seed=7, max_obst=20, first_index=first + k, threads=1)
    for x, y, w in zip(a, b, one):
        assert np.array_equal(np.concatenate([x, y]), w)
    other = generate_arrays_det(level, n, seed=8, max_obst=20, first_index=first)
    assert not np.array_equal(other[0], one[0])
    if level != 'Extrem':
        assert abs((one[6] == 0).mean() - 0.5) < 0.05                    # bay / parallel 50 : 50 at bay_mode -1
    else:
        assert (one[6] == 1).all()


def test_twin_refuses_small_tiles_and_leaves_rows_beyond_n_obst_alone():
    from hope_amd import _lib as L
    lib = L.load_library()
    n, mo, sent = 500, 18, -4321.5
    start, dest, bbox = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((n, 4))
    verts = np.full((n, mo, 4, 2), sent)
    nob = np.zeros(n, np.int32)

    def call(max_obst, nn=n):
        return lib.hope_scenegen_generate_det(2, -1, nn, 5, 0, max_obst, start.ctypes.data, dest.ctypes.data, bbox.ctypes.data,
                                              verts.ctypes.data, nob.ctypes.data, None, 1)
    for bad in (17, 1, 0, -1):
        assert call(bad) == -1                                            # HOPE_EINVAL
    assert (verts == sent).all() and (nob == 0).all()                     # nothing written by a refused call
    assert call(mo, -1) == -1
    assert lib.hope_scenegen_generate_det(3, -1, n, 5, 0, mo, start.ctypes.data, dest.ctypes.data, bbox.ctypes.data,
                                          verts.ctypes.data, nob.ctypes.data, None, 1) == -1
    assert call(mo) == 0                                                  # case_id may be null
    beyond = np.arange(mo)[None, :] >= nob[:, None]
    assert (verts[beyond] == sent).all() and (verts[~beyond] != sent).all()
    assert nob.min() >= 3 and nob.max() <= 17


def log_sweep():
    rng = np.random.default_rng(2024)
    parts = [rng.random(2_000_000),                                        # what Box-Muller feeds it
             np.exp(-rng.random(1_000_000) * 690.0),                       # log-uniform down to ~1e-300
             1.0 - rng.random(500_000) * 2.0 ** -rng.integers(1, 53, 500_000),       # just below 1
             0.5 + (rng.random(300_000) - 0.5) * 2.0 ** -rng.integers(1, 50, 300_000),
             math.sqrt(0.5) + (rng.random(300_000) - 0.5) * 2.0 ** -rng.integers(1, 50, 300_000),
             np.arange(1, 200_001) * 2.0 ** -53,                           # the smallest uniforms
             np.array([1.0, 0.5, 0.25, 1e-300, 2.0 ** -53, 1.0 - 2.0 ** -53, math.sqrt(0.5), np.nextafter(math.sqrt(0.5), 1)])]
    x = np.concatenate(parts)
    return np.ascontiguousarray(x[(x > 0) & (x <= 1.0)])


def test_log_stays_within_the_measured_distance_of_the_platform_log():
    from hope_amd import _lib as L
    lib = L.load_library()
    x = log_sweep()
    y = np.zeros_like(x)
    assert lib.hope_scenegen_log_det(len(x), x.ctypes.data, y.ctypes.data) == 0
    ref = np.log(x)
    ulp = np.abs(y - ref) / np.spacing(np.abs(ref))
    ulp[ref == 0] = np.abs(y[ref == 0]) / np.spacing(0.0)                  # log(1) = 0 exactly
    worst = float(ulp.max())
    print(f'sg_log vs platform log: worst {worst} ulp at x = {x[int(ulp.argmax())]!r} over {len(x)} arguments')
    assert y[x == 1.0].tolist() == [0.0] * int((x == 1.0).sum())
    assert worst <= LOG_BOUND_ULP, worst
    assert lib.hope_scenegen_log_det(-1, None, None) == -1


def test_new_entry_points_are_additive_to_abi_8():
    from hope_amd import _lib as L
    lib = L.load_library()
    assert lib.hope_abi_version() == 8
    for name in ('hope_scenegen_generate_det', 'hope_scenegen_generate_device', 'hope_env_generate_pool', 'hope_scenegen_log_det'):
        assert hasattr(lib, name) and name in L.EXPORTS
    assert lib.hope_env_generate_pool(None, 10, (C.c_int32 * 3)(10, 0, 0), 0, 0, 0) == -1     # null handle: HOPE_EINVAL, no device touched
