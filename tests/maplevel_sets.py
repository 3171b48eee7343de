"""Scene sets of the map-level tests (tests/test_map_level_native.py, tests/test_gpu_map_level.py): the golden set of
tests/test_map_level.py and a fresh set, both as (start, dest, rings) triples for the Python classifier and packed for the native
entries; and the +-1 ulp perturbation run that shows a set holds no knife-edge case."""
import contextlib
import math

import numpy as np

from hope_amd import map_level as M

# the fresh set: FRESH_PER_LEVEL lots of every level from the deterministic generator, and every Dragon-Lake case FRESH_DLP_DRAWS times
FRESH_GEN_SEED, FRESH_PER_LEVEL, FRESH_DLP_SEED, FRESH_DLP_DRAWS = 20261, 700, 4711, 4
LEVELS = ('Normal', 'Complex', 'Extrem')


def _triple(sc):
    return sc.start, sc.dest, [v[:int(n)] for v, n in zip(sc.verts, sc.nvert)]


def golden_scenes():
    """the 496 Dragon-Lake draws and 450 generated scenes of tests/test_map_level.py, in the order of map_level.npz's labels"""
    from hope_amd.scenes import DlpScenePool, SceneSource
    pool = DlpScenePool()
    rng = np.random.default_rng(17)
    out = [_triple(pool.sample(case=case, rng=rng)) for case in range(len(pool)) for _ in range(2)]
    src = SceneSource(levels=LEVELS, seed=123)
    return out + [_triple(src.draw()) for _ in range(450)]


def fresh_scenes(per_level=FRESH_PER_LEVEL, dlp_draws=FRESH_DLP_DRAWS):
    from hope_amd.scene_gen import generate_arrays_det
    from hope_amd.scenes import DlpScenePool
    out = []
    for lv in LEVELS:
        start, dest, _, verts, nob, _, _ = generate_arrays_det(lv, per_level, seed=FRESH_GEN_SEED, max_obst=18)
        out += [(start[k].copy(), dest[k].copy(), [verts[k, o].copy() for o in range(int(nob[k]))]) for k in range(per_level)]
    pool = DlpScenePool()
    rng = np.random.default_rng(FRESH_DLP_SEED)
    out += [_triple(pool.sample(case=case, rng=rng)) for case in range(len(pool)) for _ in range(dlp_draws)]
    return out


class _UlpMath:
    """`math` with every cos / sin / hypot / sqrt result moved by -1, 0 or +1 ulp at random"""
    pi, inf = math.pi, math.inf

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)

    def _p(self, v):
        k = int(self.rng.integers(-1, 2))
        return v if k == 0 else math.nextafter(v, math.inf if k > 0 else -math.inf)

    def cos(self, x): return self._p(math.cos(x))
    def sin(self, x): return self._p(math.sin(x))
    def hypot(self, x, y): return self._p(math.hypot(x, y))
    def sqrt(self, x): return self._p(math.sqrt(x))


@contextlib.contextmanager
def perturbed_math(seed):
    saved = M.math
    M.math = _UlpMath(seed)
    try:
        yield
    finally:
        M.math = saved


def perturbation_flips(scenes, trials=3):
    """indices of `scenes` whose Python label changes in any of `trials` +-1 ulp perturbation runs (the knife-edge cases)"""
    base = [M.get_map_level(*sc) for sc in scenes]
    flips = set()
    for t in range(trials):
        with perturbed_math(1000 + t):
            flips |= {k for k, sc in enumerate(scenes) if M.get_map_level(*sc) != base[k]}
    return sorted(flips)
