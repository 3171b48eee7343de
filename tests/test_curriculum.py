"""The map curriculum's rule without a GPU: the numpy twin (hope_amd/curriculum.py) and the pure-host C twin
(hope_curriculum_lists_host, hope_amd/csrc/hope_curriculum_core.h -- the source the kernels compile) against vectors recorded from
the reference's SceneChoose / DlpCaseChoose (tests/golden/curriculum.npz, written by tests/golden/make_golden_curriculum.py), the
properties of the weighted draw lists, the window rule, and the calls the rollout loops make.

Tolerances: pw / p_c within 1e-12 of the recorded vectors (numpy sums pairwise, the twins sequentially: last bits only).  q against
the recorded long-run frequencies: the generator wrote the largest deviation it saw into the fixture (freq_margin); the test allows
twice that -- the reference's balancing branch works on a 200-choice window, so the frequencies jitter by that order."""
import numpy as np
import pytest
import torch

from hope_amd import _lib as L
from hope_amd import curriculum as cu

LL = L.CURRICULUM_LIST_LEN
BIG = 10 ** 6                                   # cumulative episode counts beyond both horizons


def _windows(type_n, type_s, case_n=None, case_s=None):
    case_n = np.zeros(0) if case_n is None else case_n
    case_s = np.zeros(0) if case_s is None else case_s
    return np.r_[type_n, case_n].astype(np.float64), np.r_[type_s, case_s].astype(np.float64)


# ---- 1. pinned to the reference -------------------------------------------------------------------------------------------
def test_type_probabilities_match_reference_worst_perform(gold):
    g = gold('curriculum.npz')
    assert len(g['type_p']) >= 5
    for n, s, p in zip(g['type_hist_n'], g['type_hist_s'], g['type_p']):
        assert np.abs(cu.type_worst_p(n, s) - p).max() < 1e-12
        wn, ws = _windows(n, s, np.zeros(2), np.zeros(2))
        r = cu.lists_host([5, 5, 5], [0, 1, 2], 2, 128, np.full(6, BIG), wn, ws, want_lists=False)
        assert np.abs(r['pw'] - p).max() < 1e-12
    rates = g['type_hist_s'] / g['type_hist_n']
    assert (rates > np.array([0.95, 0.95, 0.9, 0.99])).all(1).any()          # a history above every target is among them


def test_case_probabilities_match_reference_choose_case(gold):
    g = gold('curriculum.npz')
    assert len(g['case_p']) >= 5 and (g['case_hist_n'] <= 1).any()
    for n, s, p in zip(g['case_hist_n'], g['case_hist_s'], g['case_p']):
        nc = len(n)
        # choose_case reaches its weighted branch with probability 0.8 and is uniform otherwise
        expect = 0.2 / nc + 0.8 * p
        assert np.abs(cu.case_p(n, s) - expect).max() < 1e-12
        wn, ws = _windows(np.full(4, 250.0), np.full(4, 100.0), n, s)
        r = cu.lists_host([], None, nc, 128, np.full(4 + nc, BIG), wn, ws, want_lists=False)
        assert np.abs(r['prob'][4:] - expect).max() < 1e-12
        assert abs(r['prob'][4:].sum() - 1.0) < 1e-12


def test_type_frequencies_follow_water_filling(gold):
    g = gold('curriculum.npz')
    assert len(g['freq']) >= 3 and int(g['freq_choices']) >= 40000
    # the margin in the fixture was measured against the rule under test: a regenerated fixture must not widen it silently.  0.01:
    # twice the 0.005 that one standard deviation of a 0.25 share over 40 000 choices (0.0022) plus the 200-choice balance window's
    # granularity (1 / 200) explain
    assert float(g['freq_margin']) < 0.01
    bound = 2.0 * float(g['freq_margin'])
    for n, s, f in zip(g['freq_hist_n'], g['freq_hist_s'], g['freq']):
        q = cu.type_q(n, s)
        assert abs(q.sum() - 1.0) < 1e-12
        assert np.abs(q - f).max() < bound, (q, f, bound)
        wn, ws = _windows(n, s)
        r = cu.lists_host([5, 5, 5], [0, 1, 2], 0, 128, np.full(4, BIG), wn, ws, want_lists=False)
        assert np.abs(r['prob'][:4] - q).max() < 1e-12


def test_uniform_before_the_horizons():
    wn, ws = _windows(np.full(4, 40.0), [40, 0, 0, 40], np.full(5, 10.0), [10, 0, 0, 10, 10])
    e = np.array([50, 50, 50, 49, 0, 0, 0, 0, 0], np.uint64)             # 199 type episodes, 49 Dragon-Lake episodes
    r = cu.lists_host([5, 5, 5], [0, 1, 2], 5, 128, e, wn, ws, want_lists=False)
    assert np.array_equal(r['prob'][:4], np.full(4, 0.25)) and np.array_equal(r['prob'][4:], np.full(5, 0.2))
    e[0] += 1; e[3] = 500
    r = cu.lists_host([5, 5, 5], [0, 1, 2], 5, 128, e, wn, ws, want_lists=False)
    assert r['prob'][1] > r['prob'][0] and r['prob'][5] > r['prob'][4]
    assert np.abs(r['prob'][:4] - cu.type_q(wn[:4], ws[:4])).max() < 1e-15


# ---- 2. lists -------------------------------------------------------------------------------------------------------------
def _random_case(rng, n_cases):
    n_pool = int(rng.integers(20, 400))
    n_obst = rng.integers(3, 18, n_pool)
    big = rng.random(n_pool) < 0.1
    n_obst[big] = rng.integers(33, 100, big.sum())
    buckets = rng.choice([0, 1, 2, 255], n_pool, p=[0.3, 0.3, 0.3, 0.1]).astype(np.uint8)
    nb = 4 + n_cases
    wn = np.r_[rng.uniform(1, 250, 4), rng.integers(0, 11, n_cases)]
    ws = wn * rng.uniform(0, 1, nb)
    return n_obst, buckets, wn, ws, np.full(nb, BIG, np.uint64)


def test_weighted_lists_properties():
    rng = np.random.default_rng(5)
    for trial, n_cases in enumerate((0, 7, 248)):
        n_obst, buckets, wn, ws, e = _random_case(rng, n_cases)
        r = cu.lists_host(n_obst, buckets, n_cases, 128, e, wn, ws)
        r2 = cu.lists_host(n_obst, buckets, n_cases, 128, e, wn, ws)
        for k in ('list0', 'list1', 'positions'):
            assert r[k].tobytes() == r2[k].tobytes()                  # same input -> same bytes
        pos, prob = r['positions'], r['prob']
        small = n_obst <= 32
        grp = np.where(buckets < 3, buckets, 3)
        for c, lst in enumerate((r['list0'], r['list1'])):
            in_cls = small if c == 0 else ~small
            cnt = np.array([np.sum(in_cls & (grp == g)) for g in range(4)])
            ncs = n_cases if c == 1 else 0
            n_base = cnt.sum() + ncs
            if n_base == 0:
                assert pos[c].sum() == 0
                continue
            assert pos[c].sum() == LL
            # expected probability of every group: each kind keeps its share of the base list
            p = np.zeros(4 + n_cases)
            present = cnt[:3] > 0
            p[:3] = np.where(present, prob[:3], 0) / max(prob[:3][present].sum(), 1e-300) * cnt[:3].sum() / n_base
            p[3] = cnt[3] / n_base
            p[4:] = prob[4:] * ncs / n_base
            has = np.r_[cnt > 0, np.full(n_cases, ncs > 0)]
            assert (np.abs(pos[c] - p * LL) < 1).all()
            assert (pos[c][has] >= 1).all() and (pos[c][~has] == 0).all()
            # entries: pool entries of this class only, in blocks by group, each entry of a group repeated equally (+- 1)
            pool = lst[lst >= 0]
            assert in_cls[pool].all()
            assert set((-2 - lst[lst < 0]).tolist()) == (set(range(n_cases)) if ncs else set())
            off = 0
            for g in range(4):
                seg = lst[off:off + pos[c][g]]
                off += pos[c][g]
                if cnt[g] == 0:
                    continue
                assert (grp[seg] == g).all()
                rep = np.bincount(seg, minlength=len(n_obst))[in_cls & (grp == g)]
                assert rep.max() - rep.min() <= 1
            for k in range(n_cases if ncs else 0):
                seg = lst[off:off + pos[c][4 + k]]
                off += pos[c][4 + k]
                assert (seg == -2 - k).all()


def test_single_class_handle_keeps_cases_in_the_small_list():
    rng = np.random.default_rng(6)
    wn, ws = _windows(np.full(4, 250.0), [200, 100, 50, 240], np.full(3, 10.0), [10, 0, 5])
    r = cu.lists_host(rng.integers(3, 18, 30), np.repeat([0, 1, 2], 10), 3, 32, np.full(7, BIG), wn, ws)
    assert r['positions'][1].sum() == 0 and r['positions'][0].sum() == LL and (r['list1'] == -1).all()
    assert r['positions'][0][5] > r['positions'][0][6] > r['positions'][0][4]      # the failing case is drawn most


def test_lists_host_rejects_misuse():
    lib = L.load_library()
    e, w = np.zeros(4, np.uint64), np.zeros(4)
    nob, bad = np.array([5, 5], np.int32), np.array([0, 3], np.uint8)
    rc = lib.hope_curriculum_lists_host(None, 2, nob.ctypes.data, bad.ctypes.data, 0, 128, e.ctypes.data, w.ctypes.data, w.ctypes.data,
                                        None, None, None, None, None)
    assert rc == -1 and b'out of range' in lib.hope_last_error()
    rc = lib.hope_curriculum_lists_host(None, 0, None, None, 0, 128, e.ctypes.data, w.ctypes.data, w.ctypes.data, None, None, None, None, None)
    assert rc == -1
    rc = lib.hope_curriculum_lists_host(None, 0, None, None, 251, 128, e.ctypes.data, w.ctypes.data, w.ctypes.data, None, None, None, None, None)
    assert rc == -1 and b'250' in lib.hope_last_error()


# ---- 3. the window rule ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('fold', [cu.fold_window, cu.fold_host], ids=['numpy', 'host'])
def test_window_rule_known_answers(fold):
    assert fold(0.0, 0.0, 0.0, 0.0, 250.0) == (0.0, 0.0)                  # a bucket that never finished an episode
    assert fold(0.0, 0.0, 100.0, 40.0, 250.0) == (100.0, 40.0)            # below the window: plain sums
    assert fold(100.0, 40.0, 150.0, 60.0, 250.0) == (250.0, 100.0)        # exactly full: untouched
    assert fold(0.0, 0.0, 1000.0, 500.0, 250.0) == (250.0, 125.0)         # dn > W in one update: the rate of the batch
    n, s = fold(200.0, 200.0, 100.0, 0.0, 250.0)                          # 300 records scaled back to 250
    assert n == 250.0 and s == 200.0 * (250.0 / 300.0)
    assert fold(10.0, 10.0, 10.0, 0.0, 10.0) == (10.0, 5.0)               # the case window


def test_window_rule_twins_agree_bitwise():
    rng = np.random.default_rng(9)
    n = s = hn = hs = 0.0
    for _ in range(200):
        dn = float(rng.integers(0, 400))
        ds = float(rng.integers(0, dn + 1))
        n, s = cu.fold_window(n, s, dn, ds, 250.0)
        hn, hs = cu.fold_host(hn, hs, dn, ds, 250.0)
        assert (n, s) == (hn, hs) and 0.0 <= s <= n <= 250.0
    # a never-finished type counts as failing everything (the reference divides 0 by 0 there)
    assert np.abs(cu.type_worst_p([0, 250, 250, 250], [0, 250, 250, 250]) - np.array([0.95, 0.01, 0.01, 0.01]) / 0.98).max() < 1e-15


# ---- 4. the loops ---------------------------------------------------------------------------------------------------------
def _spy_env(n=8):
    from fake_env import OracleEnv
    from hope_amd.scenes import SceneSource
    src = SceneSource(levels=('Normal', 'Complex', 'Extrem'), seed=3)

    class SpyEnv(OracleEnv):
        def __init__(self, scenes):
            super().__init__(scenes)
            self.calls = []

        def step(self, actions, auto_reset=False, active=None, fresh=False):
            self.calls.append('step')
            return super().step(actions, auto_reset=auto_reset, active=active)

        def enable_curriculum(self, **params):
            self.calls.append(('enable', params))

        def curriculum_tally(self):
            self.calls.append('tally')

        def curriculum_update(self):
            self.calls.append('update')

        def curriculum_state(self):
            return {'win_n': np.array([10.0, 0.0, 4.0, 0.0]), 'win_s': np.array([5.0, 0.0, 4.0, 0.0]), 'updates': self.calls.count('update')}

    return SpyEnv([src.draw() for _ in range(n)])


def test_loops_make_no_curriculum_call_by_default():
    from hope_amd import agents as A
    from hope_amd.rollout import PPOTrainer, SACTrainer
    torch.manual_seed(0)
    for make in (lambda e: PPOTrainer(e, A.BatchedPPO(device='cpu', use_img=False, lr=1e-4, mini_batch=16, mini_epoch=1), horizon=2, seed=1),
                 lambda e: SACTrainer(e, A.BatchedSAC(device='cpu', use_img=False, lr=1e-4, batch_size=8), horizon=2, update_every=2, seed=1)):
        env = _spy_env()
        tr = make(env)
        for _ in range(4):
            tr.step()
        assert env.calls == ['step'] * 4
        assert not any(k.startswith('success_rate_') for k in tr.stats())


def test_loops_tally_every_step_and_update_on_the_kth():
    from hope_amd import agents as A
    from hope_amd.rollout import PPOTrainer, SACTrainer
    torch.manual_seed(0)
    env = _spy_env()
    tr = SACTrainer(env, A.BatchedSAC(device='cpu', use_img=False, lr=1e-4, batch_size=8), horizon=2, update_every=2, seed=1,
                    fresh_scenes=True, curriculum=dict(update_every=3, type_window=100.0))
    for _ in range(7):
        tr.step()
    assert env.calls == [('enable', {'type_window': 100.0})] + ['step', 'tally'] * 2 + ['step', 'tally', 'update'] + \
        ['step', 'tally'] * 2 + ['step', 'tally', 'update'] + ['step', 'tally']
    st = tr.stats()
    assert st['success_rate_Normal'] == 0.5 and st['success_rate_Extrem'] == 1.0 and np.isnan(st['success_rate_dlp'])
    assert st['curriculum_updates'] == 2
    # PPO without an update_every of its own: the weights follow the PPO updates
    env = _spy_env()
    tr = PPOTrainer(env, A.BatchedPPO(device='cpu', use_img=False, lr=1e-4, mini_batch=16, mini_epoch=1), horizon=2, seed=1, fresh_scenes=True,
                    curriculum={})
    for _ in range(4):
        tr.step()
    assert env.calls == [('enable', {})] + ['step', 'tally', 'step', 'tally', 'update'] * 2


def test_curriculum_without_fresh_scenes_is_refused():
    from hope_amd import agents as A
    from hope_amd.rollout import PPOTrainer
    env = _spy_env()
    with pytest.raises(ValueError, match='fresh_scenes'):
        PPOTrainer(env, A.BatchedPPO(device='cpu', use_img=False, lr=1e-4, mini_batch=16, mini_epoch=1), horizon=2, seed=1, curriculum={})
    assert env.calls == []
