"""Shared by tests/test_gae_core.py (CPU, host twins) and tests/test_gpu_gae.py (kernels): the host twins' wrappers over numpy arrays,
a numpy restatement of the sums' order (hope_amd/csrc/hope_gae_core.h), and the test inputs."""
import ctypes as C

import numpy as np

from hope_amd import _lib as L

CHUNK = 64
PATTERNS = ('none', 'all', 'newest', 'oldest', 'random')            # which transitions are episode ends
GAMMA, LAM = 0.98, 0.95


def words(a):
    """the raw words of a float32 / float64 array"""
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def inputs(rows, t, pattern='random', seed=0):
    """-> reward, done, value, v_last, value_target: float32, standard-normal draws (so |mean adv| <= std adv), done as 0 / 1"""
    rng = np.random.default_rng(1000003 * rows + 101 * t + seed)
    reward, value, value_target = (rng.standard_normal((rows, t)).astype(np.float32) for _ in range(3))
    v_last = rng.standard_normal(rows).astype(np.float32)
    done = np.zeros((rows, t), np.float32)
    if pattern == 'all':
        done[:] = 1
    elif pattern == 'newest':
        done[:, t - 1] = 1
    elif pattern == 'oldest':
        done[:, 0] = 1
    elif pattern == 'random':
        done[rng.random((rows, t)) < 0.2] = 1
    else:
        assert pattern == 'none'
    return reward, done, value, v_last, value_target


def host_gae(reward, done, value, v_last, value_target, gamma=GAMMA, lam=LAM, flags=L.GAE_SUMS, delta=True):
    """hope_gae_host over numpy arrays -> adv, v_target, sums (float64 [3]; untouched -1 without a flag), delta (or None)"""
    lib = L.load_library()
    x = [np.ascontiguousarray(a, dtype=np.float32) for a in (reward, done, value, v_last, value_target)]
    rows, t = x[0].shape
    adv, v_target = np.full((rows, t), 7.0, np.float32), np.full((rows, t), 7.0, np.float32)
    dl = np.full((rows, t), 7.0, np.float32) if delta else None
    sums = np.full(3, -1.0)
    L.check(lib.hope_gae_host(*(a.ctypes.data for a in x), rows, t, gamma, lam, flags, adv.ctypes.data, v_target.ctypes.data, sums.ctypes.data,
                              dl.ctypes.data if delta else None), 'hope_gae_host')
    return adv, v_target, sums, dl


def host_mean_std(sums):
    """the float32 (m, s) the normalisation takes from sums, as numpy float32 scalars"""
    ms = (C.c_float * 2)()
    s = np.ascontiguousarray(sums, dtype=np.float64)
    L.check(L.load_library().hope_adv_normalize_host(None, 0, s.ctypes.data, None, ms), 'hope_adv_normalize_host')
    return np.float32(ms[0]), np.float32(ms[1])


def host_normalize(adv, sums):
    """hope_adv_normalize_host -> out (a new array)"""
    adv = np.ascontiguousarray(adv, dtype=np.float32)
    s = np.ascontiguousarray(sums, dtype=np.float64)
    out = np.full(adv.shape, 7.0, np.float32)
    L.check(L.load_library().hope_adv_normalize_host(adv.ctypes.data, adv.size, s.ctypes.data, out.ctypes.data, None), 'hope_adv_normalize_host')
    return out


def numpy_sums(adv):
    """the rule's sums restated in numpy: per row in scan order (t descending) from +0.0, 64-row chunks padded with +0.0 and
    combined by the aligned tree, the chunk partials by the aligned tree with pass-through"""
    a = np.ascontiguousarray(adv, dtype=np.float32).astype(np.float64)
    rows, t = a.shape
    nk = (rows + CHUNK - 1) // CHUNK
    out = []
    for term in (a, a * a):
        row = np.zeros(nk * CHUNK)
        for j in range(t - 1, -1, -1):
            row[:rows] = row[:rows] + term[:, j]
        c = row.reshape(nk, CHUNK).copy()
        h = 1
        while h < CHUNK:
            c[:, 0::2 * h] = c[:, 0::2 * h] + c[:, h::2 * h]
            h *= 2
        p = c[:, 0].copy()
        h = 1
        while h < nk:
            for i in range(0, nk - h, 2 * h):
                p[i] = p[i] + p[i + h]
            h *= 2
        out.append(p[0])
    return np.array([out[0], out[1], float(rows * t)])
