"""Shared by tests/test_ring_core.py (CPU, host twins) and tests/test_gpu_ring.py (kernels): the host twins' wrappers over numpy arrays,
a numpy restatement of the tally's order (hope_amd/csrc/hope_ring_core.h), the test inputs and the sample cases."""
import ctypes as C
import math

import numpy as np
import torch

from hope_amd import _lib as L
from hope_amd.rollout import TransitionRing

CHUNK = 64
WIDTH = {'lidar': 120, 'target': 5, 'action_mask': 42, 'action': 2, 'log_prob': 2}
KEYS = ('lidar', 'target', 'action_mask')
NS = (1, 63, 64, 65, 193)
TS = (1, 2, 5, 16)
BATCHES = (1, 32, 65, 257)
U = 2.0 ** -53


def words(a):
    """the raw words of a float32 / float64 / int64 array"""
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.ascontiguousarray(a)
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


def step_inputs(n, step, f64=False, seed=0):
    """one step's push: the before half (float32), reward (float32, or float64 values that float32 cannot hold), done u8, status i32"""
    rng = np.random.default_rng(7919 * n + 31 * step + seed)
    x = {k: rng.standard_normal((n, w)).astype(np.float32) for k, w in WIDTH.items()}
    r = rng.standard_normal(n) * 3.0
    x['reward'] = r if f64 else r.astype(np.float32)
    assert not f64 or n < 4 or (r != r.astype(np.float32)).any()
    x['done'] = (rng.random(n) < 0.3).astype(np.uint8)
    x['status'] = rng.integers(0, 6, n).astype(np.int32)
    return x


def last_obs(n, seed=0):
    rng = np.random.default_rng(104729 * n + seed)
    return {k: rng.standard_normal((n, WIDTH[k])).astype(np.float32) for k in KEYS}


def np_ring(n, t, fill=0.0):
    a = {k: np.full((n, t, w), fill, np.float32) for k, w in WIDTH.items()}
    a['reward'], a['done'] = np.full((n, t), fill, np.float32), np.full((n, t), fill, np.float32)
    return a


def desc(a):
    """hope_ring_t over numpy arrays (np_ring's layout) or torch tensors"""
    n, t = a['reward'].shape
    P = lambda v: v.data_ptr() if isinstance(v, torch.Tensor) else v.ctypes.data  # noqa: E731
    return L.Ring(*(P(a[k]) for k in ('lidar', 'target', 'action_mask', 'action', 'log_prob', 'reward', 'done')), n, t)


def _p(a):
    return None if a is None else a.ctypes.data


def host_before(ring, t, x):
    L.check(L.load_library().hope_ring_before_host(desc(ring), t, *(_p(x[k]) for k in ('lidar', 'target', 'action_mask', 'action', 'log_prob'))),
            'hope_ring_before_host')


def host_after(ring, t, x, counts=None, reward_sum=None):
    """counts int64 [2] and reward_sum float64 [1] (numpy, updated in place), or neither: no tally"""
    L.check(L.load_library().hope_ring_after_host(desc(ring), t, _p(x['reward']), int(x['reward'].dtype == np.float64), _p(x['done']),
                                                  _p(x['status']) if counts is not None else None, _p(counts), _p(reward_sum)), 'hope_ring_after_host')


def batch_arrays(batch, fill=7.0):
    o = {'obs_' + k.replace('action_', ''): np.full((batch, WIDTH[k]), fill, np.float32) for k in KEYS}
    o.update({'next_' + k.replace('action_', ''): np.full((batch, WIDTH[k]), fill, np.float32) for k in KEYS})
    o.update(action=np.full((batch, 2), fill, np.float32), reward=np.full(batch, fill, np.float32), done=np.full(batch, fill, np.float32),
             idx=np.full((batch, 3), 7, np.int32))
    return o


BATCH_FIELDS = [f[0] for f in L.RingBatch._fields_]


def batch_desc(o):
    P = lambda v: v.data_ptr() if isinstance(v, torch.Tensor) else v.ctypes.data  # noqa: E731
    return L.RingBatch(*(P(o[k]) for k in BATCH_FIELDS))


def host_sample(ring, head, size, batch, last, s=None, j=None, seed=0, counter=0):
    """hope_ring_sample_host over numpy arrays -> the batch as a dict of numpy arrays (batch_arrays' names)"""
    o = batch_arrays(batch)
    s, j = (None if v is None else np.ascontiguousarray(v, dtype=np.int32) for v in (s, j))
    L.check(L.load_library().hope_ring_sample_host(desc(ring), head, size, batch, _p(s), _p(j), C.c_uint64(seed), C.c_uint64(counter),
                                                   *(_p(last[k]) for k in KEYS), batch_desc(o)), 'hope_ring_sample_host')
    return o


def torch_ring(ring, head, size):
    """a TransitionRing over the very arrays of `ring` (numpy, np_ring's layout)"""
    n, t = ring['reward'].shape
    r = TransitionRing(n, t, KEYS, 'cpu')
    r.obs = {k: torch.from_numpy(ring[k]) for k in KEYS}
    r.action, r.log_prob, r.reward, r.done = (torch.from_numpy(ring[k]) for k in ('action', 'log_prob', 'reward', 'done'))
    r.head, r.size = head, size
    return r


def torch_sample(ring, head, size, last, s, j):
    """TransitionRing.sample with the supplied choices -> batch_arrays' names (without idx)"""
    b = torch_ring(ring, head, size).sample(len(s), {k: torch.from_numpy(v) for k, v in last.items()}, index=(torch.from_numpy(s), torch.from_numpy(j)))
    o = {'obs_' + k.replace('action_', ''): b['obs'][k].numpy() for k in KEYS}
    o.update({'next_' + k.replace('action_', ''): b['next_obs'][k].numpy() for k in KEYS})
    o.update(action=b['action'].numpy(), reward=b['reward'].numpy(), done=b['done'].numpy())
    return o


def expected_idx(head, size, t, s, j):
    col = lambda a: (head - size + a) % t  # noqa: E731
    return np.stack([s, col(j), np.where(j == size - 1, -1, col(np.minimum(j + 1, size - 1)))], axis=1).astype(np.int32)


def filled_ring(n, t, pushes, f64=False):
    """`pushes` steps through the host twins from an empty ring -> (ring arrays, head, size)"""
    ring = np_ring(n, t)
    for step in range(pushes):
        x = step_inputs(n, step, f64)
        host_before(ring, step % t, x)
        host_after(ring, step % t, x)
    return ring, pushes % t, min(pushes, t)


# (T, pushes): size < T; size == T with head 0; size == T with the head in the middle; T = 1
SAMPLE_STATES = ((5, 3), (5, 5), (5, 8), (16, 23), (1, 1), (2, 3))


def case_index(n, size, batch, seed=0):
    """the supplied choices of a sample case: random pairs, then at fixed places the newest column (j = size - 1: the last_obs
    substitution), the one before it (j = size - 2: its next column may lie across the ring's physical end), the oldest, and a
    repeated pair"""
    rng = np.random.default_rng(batch * 1009 + size * 17 + n + seed)
    s, j = rng.integers(0, n, batch).astype(np.int32), rng.integers(0, size, batch).astype(np.int32)
    j[0] = size - 1
    if batch > 3:
        j[1], j[2] = max(size - 2, 0), 0
        s[3], j[3] = s[1], j[1]
    return s, j


def numpy_step_sum(reward):
    """the tally's step_sum restated in numpy: (double)reward in 64-row chunks padded with +0.0 and combined by the aligned tree, the
    chunk partials by the aligned tree with pass-through"""
    r = np.ascontiguousarray(reward).astype(np.float64)
    nk = (len(r) + CHUNK - 1) // CHUNK
    c = np.zeros(nk * CHUNK)
    c[:len(r)] = r
    c = c.reshape(nk, CHUNK)
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
    return p[0]


def sum_bound(n, steps, scale):
    """DESIGN 5i's bound for that tree without the row term: a reward goes through at most 6 additions in the wave and `levels` in the
    chunk tree, then one per step into the running total, each rounding to 2^-53 of a partial sum that is at most sum |term|; one more
    for the exact value's own rounding"""
    nk = (n + CHUNK - 1) // CHUNK
    levels = math.ceil(math.log2(nk)) if nk > 1 else 0
    return (6 + levels + steps + 1) * U * scale
