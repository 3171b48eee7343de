"""Scripted episodes for the evaluation tracker (hope_amd/csrc/hope_evaltrack_core.h): what an env would hand the tracker over 12
steps, with the rows a lane can get wrong, a scalar restatement of the reference's loop (src/evaluation/eval_utils.py:35-53) and a
driver of the host twins that records everything after every call.  Shared by tests/test_evaltrack_core.py (twin against the
restatement) and tests/test_gpu_evaltrack.py (kernels against the twin)."""
import ctypes as C

import numpy as np

STEPS = 12
SIZES = (1, 63, 64, 65, 130)
QNAN = np.uint64(0x7FF8000000000000)
KINDS = 8


def box():
    from hope_amd import tables as T
    return np.array([T.VALID_STEER[0], T.VALID_STEER[1], T.VALID_SPEED[0], T.VALID_SPEED[1]], dtype=np.float64)


def f32_nan(payload, negative=False):
    return np.array([0x7FC00000 | payload | (0x80000000 if negative else 0)], dtype=np.uint32).view(np.float32)[0]


def make_script(n, seed=0, obs_dtype=np.float32):
    """-> dict: 'first' (target, pose) and 'steps': STEPS dicts of target [n, 5], pose [n, 3], reward [n], status [n], done [n],
    rs_word [n, 8], action [n, 2] (the policy's, float64 values exactly representable in float32), u [n, 2].  Scene i is of kind
    i % 8:
      0  finishes at step 5; afterwards `done` is raised again, the reward is huge and the pose jumps (all ignored)
      1  a NaN target component (odd payload) at steps 3, 4 and 5: never stuck there, stored as the one quiet NaN
      2  target[0] alternates +0.0 / -0.0 with the rest constant: stuck at every step
      3  a NaN reward (negative, with a payload) at step 2: the sum is the canonical NaN from then on
      4  finishes at its first step
      5  never finishes; its target repeats now and then (stuck after the first step)
      6  a NaN pose at step 6: the path is the canonical NaN from then on; finishes at step 9
      7  finishes at a random step"""
    rng = np.random.default_rng(1000 * n + seed)
    kind = np.arange(n) % KINDS
    fin_at = np.where(kind == 0, 5, np.where(kind == 4, 0, np.where(kind == 6, 9, np.where(kind == 7, rng.integers(1, STEPS, n), STEPS + 5))))
    target = rng.normal(0, 3, (n, 5)).astype(np.float32)
    target[kind == 2, 0] = 0.0
    pose = rng.normal(0, 10, (n, 3))
    script = {'n': n, 'kind': kind, 'first': (target.astype(obs_dtype), pose.copy()), 'steps': []}
    for t in range(STEPS):
        repeat = rng.random(n) < 0.4                              # the target did not move: stuck
        new = rng.normal(0, 3, (n, 5)).astype(np.float32)
        target = np.where(repeat[:, None] | (kind == 2)[:, None], target, new)
        k1 = (kind == 1) & (t >= 3) & (t <= 5)
        target[k1, 2] = f32_nan(0x1234 + t, negative=bool(t & 1))
        if t == 6:
            target[kind == 1, 2] = 0.5
        k2 = kind == 2
        target[k2, 0] = np.float32(-0.0) if t % 2 == 0 else np.float32(0.0)
        pose = pose + rng.normal(0, 0.4, (n, 3))
        reward = rng.normal(0, 1, n).astype(np.float32)
        if t == 2:
            reward[kind == 3] = f32_nan(0x777, negative=True)
        p = pose.copy()
        if t == 6:
            p[kind == 6, 0] = np.array([0xFFF8000000000ABC], dtype=np.uint64).view(np.float64)[0]
        frozen0 = (kind == 0) & (t > 5)
        reward[frozen0] = 1e30
        p[frozen0, :2] += 1e6 * (t + 1)
        done = (fin_at == t).astype(np.uint8)
        done[frozen0 & (t % 2 == 0)] = 1
        status = np.where(done != 0, rng.integers(2, 6, n), 1).astype(np.int32)
        word = rng.integers(-1, 3, (n, 8)).astype(np.int8)
        word[:, 5] = rng.integers(1, 6, n)
        word[:, 6] = rng.integers(0, 2, n)
        word[:, 7] = rng.integers(-128, 128, n)                   # (a byte the rule must hand on as it is)
        action = rng.uniform(-1, 1, (n, 2)).astype(np.float32).astype(np.float64)
        u = rng.random((n, 2))
        u[rng.random(n) < 0.1] = [0.0, 1.0 - 2.0 ** -53]          # the ends of the draw's range: both clip
        script['steps'].append({'target': target.astype(obs_dtype), 'pose': p, 'reward': reward.astype(obs_dtype), 'status': status, 'done': done,
                                'rs_word': word, 'action': action, 'u': u})
    return script


def scalar_replay(script):
    """the reference's loop, one scene after the other in plain Python / numpy scalars -> per step, before the env step: alive,
    stuck; after it: steps, status, total, path (np.sqrt(dx * dx + dy * dy) summed), path_norm (np.linalg.norm summed), alive, stuck,
    word, done -- lists over steps of arrays over scenes"""
    n = script['n']
    keys = ('alive0', 'stuck0', 'steps', 'status', 'total', 'path', 'path_norm', 'alive', 'stuck', 'word', 'done')
    out = {k: [np.zeros((n, 8), np.int8) if k == 'word' else np.zeros(n, np.float64 if k in ('total', 'path', 'path_norm') else np.int64)
               for _ in range(STEPS)] for k in keys}
    t0, p0 = script['first']
    for i in range(n):
        last_obs = t0[i].astype(np.float64)                       # last_obs = obs['target'] (:39)
        last_xy = p0[i, :2].copy()
        step_num, total, path, path_norm, status = 0, np.float64(0.0), np.float64(0.0), np.float64(0.0), 1
        alive, stuck = True, True                                 # the first comparison is obs['target'] with itself (:46)
        for t, s in enumerate(script['steps']):
            out['alive0'][t][i], out['stuck0'][t][i] = alive, stuck
            if alive:                                             # env.step (:48) ... (:50-53)
                step_num += 1
                with np.errstate(invalid='ignore', over='ignore'):
                    total = total + np.float64(s['reward'][i])
                    d = s['pose'][i, :2] - last_xy
                    path = path + np.sqrt(d[0] * d[0] + d[1] * d[1])
                    path_norm = path_norm + np.linalg.norm(d)
            last_xy = s['pose'][i, :2].copy()
            fin = alive and bool(s['done'][i])
            if fin:
                status = int(s['status'][i])
            obs = s['target'][i].astype(np.float64)
            stuck = bool((obs == last_obs).all())                 # (:46)
            last_obs = obs
            keep = alive and not fin
            w = s['rs_word'][i].copy()
            if not keep:
                w[6] = 0
            alive = keep
            for k, v in (('steps', step_num), ('status', status), ('total', total), ('path', path), ('path_norm', path_norm), ('alive', alive),
                         ('stuck', stuck), ('done', fin)):
                out[k][t][i] = v
            out['word'][t][i] = w
    return out


def expected_action(action, stuck, u, dtype):
    """the action buffer after the override: (lo + span * u).clip(-1, 1) cast once, in the stuck rows"""
    b = box()
    lo, span = np.array([b[0], b[2]]), np.array([b[1] - b[0], b[3] - b[2]])
    rnd = (lo + span * u).clip(-1, 1).astype(dtype)
    return np.where(np.asarray(stuck, bool)[:, None], rnd, action.astype(dtype))


def decode(state):
    """the packed plane -> steps, status, alive, stuck"""
    w = state[9]
    return ((w & np.uint64(0xFFFFFFFF)).astype(np.int64), ((w >> np.uint64(32)) & np.uint64(0xFF)).astype(np.int64),
            ((w >> np.uint64(40)) & np.uint64(1)).astype(np.int64), ((w >> np.uint64(41)) & np.uint64(1)).astype(np.int64))


class Twin:
    """the host twins over a state block of its own"""

    def __init__(self, n, obs_dtype=np.float32):
        from hope_amd import _lib as L
        self.L, self.lib, self.n = L, L.load_library(), n
        self.f64 = int(np.dtype(obs_dtype) == np.float64)
        self.state = np.zeros((L.EVAL_STATE_WORDS, n), np.uint64)
        self.box = box()

    def begin(self, target, pose):
        target, pose = np.ascontiguousarray(target), np.ascontiguousarray(pose, dtype=np.float64)
        self.L.check(self.lib.hope_eval_begin_host(self.n, self.n, self.state.ctypes.data, target.ctypes.data, self.f64, pose.ctypes.data), 'begin')

    def override(self, action, u=None, seed=0, counter=0):
        """action: numpy [n, 2] float32 / float64, changed in place -> active"""
        assert action.flags.c_contiguous and action.dtype in (np.float32, np.float64)
        active = np.zeros(self.n, np.uint8)
        up = None if u is None else np.ascontiguousarray(u, dtype=np.float64)
        self.L.check(self.lib.hope_eval_override_host(self.n, self.n, self.state.ctypes.data, self.box.ctypes.data, action.ctypes.data,
                                                      int(action.dtype == np.float64), None if up is None else up.ctypes.data, seed, counter, 0,
                                                      active.ctypes.data), 'override')
        return active

    def track(self, s):
        word, done = np.zeros((self.n, 8), np.int8), np.zeros(self.n, np.uint8)
        a = [np.ascontiguousarray(s[k]) for k in ('target', 'pose', 'reward', 'status', 'done', 'rs_word')]
        self.L.check(self.lib.hope_eval_track_host(self.n, self.n, self.state.ctypes.data, a[0].ctypes.data, self.f64, a[1].ctypes.data, a[2].ctypes.data,
                                                   a[3].ctypes.data, a[4].ctypes.data, a[5].ctypes.data, word.ctypes.data, done.ctypes.data), 'track')
        return word, done

    def records(self):
        st = self.state
        steps, status, _, _ = decode(st)
        with np.errstate(invalid='ignore', over='ignore'):
            return np.stack([status.astype(np.float32), steps.astype(np.float32), st[7].view(np.float64).astype(np.float32),
                             st[8].view(np.float64).astype(np.float32)], axis=1)


def uses_u(supplied_u, t):
    return t % 2 == 0 if supplied_u == 'alt' else bool(supplied_u)


def run_twin(script, act_dtype=np.float32, supplied_u=True, seed=0):
    """the whole script through the twins -> list of snapshots, one after every call: ('begin' | 'override' | 'track', state copy,
    action buffer, active, word, done).  supplied_u='alt': the script's u at even steps, the counter-based draw at odd ones."""
    obs_dtype = script['first'][0].dtype
    tw = Twin(script['n'], obs_dtype)
    snaps = []
    tw.begin(*script['first'])
    snaps.append(('begin', tw.state.copy(), None, None, None, None))
    for t, s in enumerate(script['steps']):
        a = np.ascontiguousarray(s['action'].astype(act_dtype))
        active = tw.override(a, s['u'] if uses_u(supplied_u, t) else None, seed, t)
        snaps.append(('override', tw.state.copy(), a, active, None, None))
        word, done = tw.track(s)
        snaps.append(('track', tw.state.copy(), None, None, word, done))
    return tw, snaps


def ptr(a):
    return C.c_void_p(a.ctypes.data)
