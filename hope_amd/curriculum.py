"""The map curriculum's rule in numpy (a twin of hope_amd/csrc/hope_curriculum_core.h for users and tests) and the ctypes wrapper
of its pure-host C twin.

The reference picks every new episode's scene with SceneChoose / DlpCaseChoose (src/train/train_HOPE_sac.py:23-97).  The batched
restatement the device runs (include/hope_env.h, DESIGN.md "Curriculum"):

  window   (n, s) += (dn, ds); if n > W: s *= W / n, n = W              (W = 250 for the four types, 10 for a case)
  types    fail = clip(target - s / n, 0.01, 1); pw = fail / sum(fail)   (_choose_case_worst_perform)
           q = max(0.5 * pw, h) with sum(q) = 1                          (long-run frequencies of choose_case); uniform before 200
  cases    rate = 0 if n <= 1 else s / n; fail = clip(1 - rate, 0.005, 1)
           p = 0.2 / n_cases + 0.8 * fail / sum(fail)                     (DlpCaseChoose.choose_case); uniform before 500
"""
import ctypes as C
from functools import partial

import numpy as np

from . import _lib as L

DEFAULTS = dict(target=(0.95, 0.95, 0.9, 0.99), type_window=250.0, case_window=10.0, type_fail_min=0.01, case_fail_min=0.005,
                worst_share=0.5, case_uniform=0.2, type_horizon=200, case_horizon=500)
TYPE_NAMES = ('Normal', 'Complex', 'Extrem', 'dlp')


def fold_window(n, s, dn, ds, window):
    """one update of a bucket's running window -> (n, s)"""
    n, s = n + dn, s + ds
    if n > window:
        s, n = s * (window / n), window
    return n, s


def type_worst_p(win_n, win_s, **params):
    """the p vector _choose_case_worst_perform hands to np.random.choice, from the four type windows"""
    P = dict(DEFAULTS, **params)
    n, s = np.asarray(win_n, float)[:4], np.asarray(win_s, float)[:4]
    rate = np.where(n > 0, s / np.where(n > 0, n, 1.0), 0.0)
    fail = np.clip(np.asarray(P['target']) - rate, P['type_fail_min'], 1.0)
    return fail / fail.sum()


def water_fill(a):
    """q = max(a, h) with h such that sum(q) = 1 (sum(a) <= 1), closed form over the sorted values"""
    a = np.asarray(a, float)
    srt = np.sort(a)
    top, h = 0.0, 1.0 / len(a)
    for k in range(len(a), 0, -1):
        h = (1.0 - top) / k
        if h >= srt[k - 1]:
            break
        top += srt[k - 1]
    return np.maximum(a, h)


def type_q(win_n, win_s, type_episodes=None, **params):
    """long-run scene-type frequencies of SceneChoose.choose_case; uniform before type_horizon episodes"""
    P = dict(DEFAULTS, **params)
    if type_episodes is not None and type_episodes < P['type_horizon']:
        return np.full(4, 0.25)
    return water_fill(P['worst_share'] * type_worst_p(win_n, win_s, **params))


def case_p(win_n, win_s, dlp_episodes=None, **params):
    """the probabilities of DlpCaseChoose.choose_case over the cases (windows of the cases only)"""
    P = dict(DEFAULTS, **params)
    n, s = np.asarray(win_n, float), np.asarray(win_s, float)
    nc = len(n)
    if dlp_episodes is not None and dlp_episodes < P['case_horizon']:
        return np.full(nc, 1.0 / nc)
    rate = np.where(n <= 1.0, 0.0, s / np.where(n > 0, n, 1.0))
    fail = np.clip(1.0 - rate, P['case_fail_min'], 1.0)
    return P['case_uniform'] / nc + (1.0 - P['case_uniform']) * fail / fail.sum()


def fold_host(n, s, dn, ds, window):
    """the C twin of fold_window (hope_curriculum_fold_host)"""
    lib = L.load_library()
    cn, cs = C.c_double(n), C.c_double(s)
    L.check(lib.hope_curriculum_fold_host(C.byref(cn), C.byref(cs), dn, ds, window), 'hope_curriculum_fold_host')
    return cn.value, cs.value


def lists_host(n_obst, buckets, n_cases, max_obstacles, episodes, win_n, win_s, want_lists=True, **params):
    """hope_curriculum_lists_host: the weighted draw lists the device builds from these windows, computed on the host (no GPU).
    -> dict(list0, list1 [2^20] int32 (None without want_lists), prob [4 + n_cases], pw [4], positions [2, 4 + n_cases])"""
    lib = L.load_library()
    arg = partial(L.array_arg, 'hope_curriculum_lists_host')
    nob = arg('n_obst', n_obst, np.int32, (None,))
    bk = arg('buckets', buckets, np.uint8, nob.shape, optional=True)
    nb = 4 + int(n_cases)
    e = arg('episodes', episodes, np.uint64, (nb,))
    wn, ws = arg('win_n', win_n, np.float64, (nb,)), arg('win_s', win_s, np.float64, (nb,))
    l0 = np.full(L.CURRICULUM_LIST_LEN, -1, np.int32) if want_lists else None
    l1 = np.full(L.CURRICULUM_LIST_LEN, -1, np.int32) if want_lists else None
    prob, pw, pos = np.zeros(nb), np.zeros(4), np.zeros((2, nb), np.int32)
    p = L.CurriculumParams(**dict(DEFAULTS, **params))
    L.check(lib.hope_curriculum_lists_host(C.byref(p), len(nob), nob.ctypes, None if bk is None else bk.ctypes, int(n_cases), int(max_obstacles),
                                           e.ctypes, wn.ctypes, ws.ctypes, None if l0 is None else l0.ctypes, None if l1 is None else l1.ctypes,
                                           prob.ctypes, pw.ctypes, pos.ctypes), 'hope_curriculum_lists_host')
    return {'list0': l0, 'list1': l1, 'prob': prob, 'pw': pw, 'positions': pos}


def mix64(z):
    """splitmix64 finaliser on uint64 arrays: the hash of the draws (hope_amd/csrc/hope_dev.h)"""
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over='ignore'):
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def draw_key(seed, scene, episode):
    """key of the draw of `scene` whose episode counter is `episode`: a scene takes list[key % len(list)] of its class"""
    seed = np.uint64(int(seed) & (2 ** 64 - 1))
    return mix64(seed ^ mix64((np.asarray(scene, dtype=np.uint64) << np.uint64(32)) | np.asarray(episode, dtype=np.uint64)))


class CurriculumDriver:
    """what the rollout loops do with `curriculum=dict(update_every=K, **params)`: tally after every step, update every K steps
    (or when the trainer says so).  `env` needs enable_curriculum / curriculum_tally / curriculum_update / curriculum_state."""

    def __init__(self, env, update_every=16, **params):
        self.env, self.update_every = env, int(update_every)
        self.steps = 0
        env.enable_curriculum(**params)

    def after_step(self, update_now=None):
        self.env.curriculum_tally()
        self.steps += 1
        if update_now if update_now is not None else (self.update_every > 0 and self.steps % self.update_every == 0):
            self.env.curriculum_update()

    def stats(self):
        st = self.env.curriculum_state()
        wn, ws = np.asarray(st['win_n'])[:4], np.asarray(st['win_s'])[:4]
        out = {'success_rate_%s' % nm: (float(ws[t] / wn[t]) if wn[t] > 0 else float('nan')) for t, nm in enumerate(TYPE_NAMES)}
        out['curriculum_updates'] = int(st['updates'])
        return out
