"""Shared by tests/test_obsnorm_core.py (CPU, host twin) and tests/test_gpu_obsnorm.py (kernels): the host twin's wrapper over
numpy arrays, a numpy restatement of the rule of hope_amd/csrc/hope_obsnorm_core.h, exact statistics in rational arithmetic and the
test observations."""
import math
from fractions import Fraction

import numpy as np

from hope_amd import _lib as L

NL, NT, NC, CHUNK = L.OBSNORM_LIDAR, L.OBSNORM_TARGET, L.OBSNORM_COLS, 64
ROW_COUNTS = (1, 2, 63, 64, 65, 193, 321)            # one lane; the chunk boundary and one row past it; three chunks with a short
#                                                      last one; six chunks: the tree passes a node through at two levels


class HostNorm:
    """hope_obsnorm_host with a state of its own"""

    def __init__(self):
        self.lib = L.load_library()
        self.state = L.ObsNormState()

    def raw(self, lidar, target, rows, in_f64, flags, out_lidar, out_target):
        P = lambda a: None if a is None else a.ctypes.data  # noqa: E731
        return self.lib.hope_obsnorm_host(self.state, P(lidar), P(target), rows, in_f64, flags, P(out_lidar), P(out_target))

    def __call__(self, lidar, target, update=True, normalize=True):
        """lidar [rows, 120], target [rows, 5]: float32 or float64 (the same) -> (out_lidar f32, out_target f32) or (None, None)"""
        lidar, target = np.ascontiguousarray(lidar), np.ascontiguousarray(target)
        rows = lidar.shape[0]
        assert lidar.dtype in (np.float32, np.float64) and target.dtype == lidar.dtype
        assert lidar.shape == (rows, NL) and target.shape == (rows, NT)
        ol = np.full((rows, NL), 7.0, np.float32) if normalize else None
        ot = np.full((rows, NT), 7.0, np.float32) if normalize else None
        flags = (L.OBSNORM_UPDATE if update else 0) | (L.OBSNORM_NORMALIZE if normalize else 0)
        L.check(self.raw(lidar, target, rows, int(lidar.dtype == np.float64), flags, ol, ot), 'hope_obsnorm_host')
        return ol, ot

    @property
    def n_state(self):
        return int(self.state.n_state)

    def stats(self):
        """-> (mean, S, std): float64 [125] each"""
        return tuple(np.array(a, dtype=np.float64) for a in (self.state.mean, self.state.S, self.state.std))

    def load(self, n_state, mean, S, std):
        self.state.n_state = int(n_state)
        for name, v in (('mean', mean), ('S', S), ('std', std)):
            getattr(self.state, name)[:] = np.asarray(v, dtype=np.float64).tolist()


# ---- the rule in numpy (float64; np.cumsum adds in row order) ------------------------------------------------------------------
def _merge(a, b):
    n = a[0] + b[0]
    d = b[1] - a[1]
    return n, a[1] + d * (b[0] / n), a[2] + b[2] + d * d * (a[0] * b[0] / n)


class NumpyNorm:
    def __init__(self):
        self.n_state, self.mean, self.S, self.std = 0, np.zeros(NC), np.zeros(NC), np.zeros(NC)

    def update(self, lidar, target):
        x = np.concatenate([lidar, target], axis=1).astype(np.float64)
        if self.n_state == 0:
            self.mean, self.std, self.S, self.n_state = x[0].copy(), x[0].copy(), np.zeros(NC), 1
            x = x[1:]
        m = x.shape[0]
        if m == 0:
            return
        parts = []
        for r0 in range(0, m, CHUNK):
            c = x[r0:r0 + CHUNK]
            cnt = float(c.shape[0])
            mean_c = np.cumsum(c, axis=0)[-1] / cnt
            e = c - mean_c
            parts.append((cnt, mean_c, np.cumsum(e * e, axis=0)[-1]))
        h = 1
        while h < len(parts):
            for i in range(0, len(parts) - h, 2 * h):
                parts[i] = _merge(parts[i], parts[i + h])
            h *= 2
        n, self.mean, self.S = _merge((float(self.n_state), self.mean, self.S), parts[0])
        self.std = np.sqrt(self.S / n)
        self.n_state += m

    def normalize(self, lidar, target):
        x = np.concatenate([lidar, target], axis=1).astype(np.float64)
        y = ((x - self.mean) / (self.std + 1e-8)).astype(np.float32)
        return y[:, :NL], y[:, NL:]


# ---- exact statistics of everything folded so far ------------------------------------------------------------------------------
class ExactStats:
    """sum x and sum x^2 per column as integers over a common power-of-two denominator (every float is m / 2^k), so that mean and
    S = sum (x - mean)^2 are exact Fractions"""
    K = 160                                            # 2^-160 divides every float32 (asserted per value)

    def __init__(self):
        self.n, self.sx, self.sxx, self.amax = 0, [0] * NC, [0] * NC, np.zeros(NC)

    def add(self, lidar, target):
        x = np.concatenate([lidar, target], axis=1).astype(np.float64)
        self.n += x.shape[0]
        self.amax = np.maximum(self.amax, np.abs(x).max(axis=0))
        for c in range(NC):
            ints = []
            for v in x[:, c].tolist():
                num, den = v.as_integer_ratio()
                assert den <= 1 << self.K
                ints.append(num * ((1 << self.K) // den))
            self.sx[c] += sum(ints)
            self.sxx[c] += sum(i * i for i in ints)

    def mean(self, c):
        return Fraction(self.sx[c], self.n << self.K)

    def var(self, c):
        """S / n = (n sum x^2 - (sum x)^2) / n^2"""
        return Fraction(self.n * self.sxx[c] - self.sx[c] ** 2, (self.n * self.n) << (2 * self.K))

    def errors(self, mean, std):
        """-> (worst |mean - exact| / scale, worst |std - exact| / scale), scale = max(1, max|x|) of the column"""
        wm = ws = 0.0
        for c in range(NC):
            scale = max(1.0, float(self.amax[c]))
            wm = max(wm, abs(float(Fraction(float(mean[c])) - self.mean(c))) / scale)
            ws = max(ws, abs(float(std[c]) - math.sqrt(self.var(c))) / scale)      # (float(Fraction) rounds once, sqrt once more)
        return wm, ws


# ---- observations --------------------------------------------------------------------------------------------------------------
def observations(rows, seed, dtype=np.float32):
    """lidar-like columns: float32 values in [0, 10] m, column 7 constant, column 11 = 10.0 except for 2 % of the rows; target-like
    columns of scales 30 / 3 / 3 / 1 / 1"""
    rng = np.random.default_rng(seed)
    lidar = rng.uniform(0.0, 10.0, (rows, NL)).astype(np.float32)
    lidar[:, 7] = np.float32(3.7)
    lidar[:, 11] = np.where(rng.random(rows) < 0.02, lidar[:, 11], np.float32(10.0))
    target = (rng.normal(0.0, 1.0, (rows, NT)) * np.array([30.0, 3.0, 3.0, 1.0, 1.0])).astype(np.float32)
    return lidar.astype(dtype), target.astype(dtype)


def words(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


# ---- the loop of tests/test_gpu_obsnorm.py -------------------------------------------------------------------------------------
LOOP_LOTS, LOOP_STEPS, LOOP_LOT_SEED = 512, 24, 7


def loop_arrays():
    from hope_amd.scene_gen import mixed_arrays
    return mixed_arrays(LOOP_LOTS, levels=('Normal', 'Complex', 'Extrem'), seed=LOOP_LOT_SEED, max_obst=32)
