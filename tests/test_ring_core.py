"""The transition ring's rule (hope_amd/csrc/hope_ring_core.h) through its host twins hope_ring_before_host / _after_host /
_sample_host, on the CPU: the push and the batch against rollout.TransitionRing word for word, the tally against exact arithmetic and
a numpy restatement of its order, the counter-based draws, DeviceTransitionRing inside PPOTrainer and SACTrainer on the stand-in env,
and the sanitizer driver of the twins."""
import math
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ring_script as RS  # noqa: E402
from hope_amd import _lib as L  # noqa: E402
from hope_amd import agents as A  # noqa: E402
from hope_amd import rollout as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_structures_mirror_the_header():
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'hope_env.h')).read(), flags=re.S)
    for cls, struct in ((L.Ring, 'hope_ring_t'), (L.RingBatch, 'hope_ring_batch_t')):
        body = re.search(r'typedef\s+struct\s+%s\s*\{(.*?)\}\s*%s\s*;' % (struct, struct), hdr, flags=re.S).group(1)
        fields = [re.search(r'(\w+)\s*$', d.strip()).group(1) for d in re.split(r'[;,]', body) if d.strip()]
        assert fields == [f[0] for f in cls._fields_], (struct, fields)


@pytest.mark.parametrize('f64', [False, True])
def test_push_equals_transition_ring_word_for_word(f64):
    """T + 3 pushes (the head wraps, ordered() gathers) into TransitionRing and through the twins: every tensor, as stored and as
    ordered() returns it, as uint32 words; the tally does not change what is stored"""
    for n in RS.NS:
        for t in RS.TS:
            ref = R.TransitionRing(n, t, RS.KEYS, 'cpu')
            ring, tallied = RS.np_ring(n, t, fill=7.0), RS.np_ring(n, t, fill=7.0)
            counts, rsum = np.zeros(2, np.int64), np.zeros(1)
            for step in range(t + 3):
                x = RS.step_inputs(n, step, f64)
                tx = {k: torch.from_numpy(v) for k, v in x.items()}
                ref.write_before(tx, tx['action'], tx['log_prob'])
                ref.write_after(tx['reward'], tx['done'])
                for r in (ring, tallied):
                    RS.host_before(r, step % t, x)
                RS.host_after(ring, step % t, x)
                RS.host_after(tallied, step % t, x, counts, rsum)
                if step + 1 < t:                                   # columns not yet written keep what they held
                    assert (ring['reward'][:, step + 1:] == 7.0).all() and (ring['lidar'][:, step + 1:] == 7.0).all()
            assert (ref.head, ref.size) == ((t + 3) % t, t)
            mine = RS.torch_ring(ring, ref.head, ref.size)
            for got, want in zip(_flat(mine.ordered()), _flat(ref.ordered())):
                assert got.dtype == torch.float32 and np.array_equal(RS.words(got), RS.words(want)), (n, t)
            for k in ring:
                assert np.array_equal(RS.words(ring[k]), RS.words(tallied[k])), (n, t, k)
            assert np.array_equal(RS.words(ring['reward']), RS.words(ref.reward)) and np.array_equal(RS.words(ring['done']), RS.words(ref.done))


def _flat(o):
    obs, action, reward, done, log_prob = o
    return [obs[k] for k in RS.KEYS] + [action, reward, done, log_prob]


@pytest.mark.parametrize('n', [1, 64, 65, 129, 4097])
def test_tally_is_exact_in_the_counts_and_ordered_in_the_sum(n):
    """counts are the integer sums; reward_sum is, word for word, the running total of the numpy restatement's step sums, and within
    the order's bound of math.fsum over every (double)reward_in -- the float64 inputs, not their float32 roundings"""
    ring = RS.np_ring(n, 2)
    worst = 0.0
    for f64 in (False, True):
        counts, rsum = np.array([5, 3], np.int64), np.array([0.25])
        want_counts, want_sum, terms = counts.copy(), rsum.copy(), [0.25]
        for step in range(5):
            x = RS.step_inputs(n, step, f64, seed=11)
            RS.host_after(ring, step % 2, x, counts, rsum)
            want_counts += [int((x['done'] != 0).sum()), int((x['status'] == 2).sum())]
            want_sum = want_sum + RS.numpy_step_sum(x['reward'])
            terms += x['reward'].astype(np.float64).tolist()
            assert np.array_equal(counts, want_counts) and np.array_equal(RS.words(rsum), RS.words(want_sum)), (n, f64, step)
            bound = RS.sum_bound(n, step + 1, math.fsum(abs(v) for v in terms))
            err = abs(float(rsum[0]) - math.fsum(terms))
            assert err <= bound, (n, f64, step, err, bound)
            worst = max(worst, err / bound)
    print('worst error / bound:', worst)


def test_sample_equals_transition_ring_word_for_word():
    """the twin and TransitionRing.sample with the same supplied (s, j): size < T, size == T with the head at 0 and in the middle,
    j = size - 1 (last_obs), j = size - 2 across the physical end, T = 1, a repeated pair, batches of 1, 32, 65 and 257"""
    for n in RS.NS:
        last = RS.last_obs(n)
        for t, pushes in RS.SAMPLE_STATES:
            ring, head, size = RS.filled_ring(n, t, pushes, f64=bool(pushes % 2))
            for batch in RS.BATCHES:
                s, j = RS.case_index(n, size, batch)
                got = RS.host_sample(ring, head, size, batch, last, s, j)
                want = RS.torch_sample(ring, head, size, last, s, j)
                for k, v in want.items():
                    assert got[k].shape == v.shape and np.array_equal(RS.words(got[k]), RS.words(v)), (n, t, pushes, batch, k)
                assert np.array_equal(got['idx'], RS.expected_idx(head, size, t, s, j)), (n, t, pushes, batch)
                assert got['idx'][0, 2] == -1 and np.array_equal(RS.words(got['next_lidar'][0]), RS.words(last['lidar'][s[0]]))
    # the j = size - 2 case did cross the physical end somewhere: column T - 1 followed by column 0
    ring, head, size = RS.filled_ring(65, 5, 8)
    s, j = RS.case_index(65, size, 32)
    idx = RS.host_sample(ring, head, size, 32, RS.last_obs(65), s, j)['idx']
    assert head == 3 and ((idx[:, 1] == 4) & (idx[:, 2] == 0)).any()


def test_rows_out_of_range_are_flagged_not_clamped():
    """a supplied s or j outside its range: zeros and idx = -1 in that row, the neighbouring rows as without it"""
    n, t = 65, 5
    ring, head, size = RS.filled_ring(n, t, 3)
    last = RS.last_obs(n)
    s, j = RS.case_index(n, size, 32)
    good = RS.host_sample(ring, head, size, 32, last, s, j)
    bad_rows = {2: ('s', -1), 9: ('s', n), 10: ('j', size), 17: ('j', -1), 31: ('s', 2 ** 31 - 1), 0: ('j', t)}
    s2, j2 = s.copy(), j.copy()
    for row, (which, v) in bad_rows.items():
        (s2 if which == 's' else j2)[row] = v
    got = RS.host_sample(ring, head, size, 32, last, s2, j2)
    keep = np.array([b not in bad_rows for b in range(32)])
    for k in got:
        assert np.array_equal(RS.words(got[k][keep]), RS.words(good[k][keep])), k
        if k != 'idx':
            assert (RS.words(got[k][~keep]) == 0).all(), k
    assert (got['idx'][~keep] == -1).all()


def test_draws():
    """the twin's draw mode is ring_draws; the draws are in range up to n = 2^31 - 1; another counter, another list; and over a fixed
    seed, n = 7, size = 5 and 70 000 items every one of the 35 cells lies within 6 standard deviations of 2 000"""
    n, t = 65, 5
    ring, head, size = RS.filled_ring(n, t, 8)
    last = RS.last_obs(n)
    lists = []
    for seed, counter in ((0, 0), (0, 1), (12345, 0), (2 ** 64 - 1, 2 ** 40 + 3)):
        s, j = R.ring_draws(seed, counter, 257, n, size)
        assert s.dtype == np.int32 and 0 <= s.min() and s.max() < n and 0 <= j.min() and j.max() < size
        got = RS.host_sample(ring, head, size, 257, last, seed=seed, counter=counter)
        want = RS.host_sample(ring, head, size, 257, last, s, j)
        for k in got:
            assert np.array_equal(RS.words(got[k]), RS.words(want[k])), (seed, counter, k)
        assert np.array_equal(got['idx'], RS.expected_idx(head, size, t, s, j))
        lists.append((tuple(s), tuple(j)))
    assert len(set(lists)) == len(lists)
    for rng in (1, 2, 3, 2 ** 20 + 1, 2 ** 31 - 1):
        s, j = R.ring_draws(9, 4, 4096, rng, min(rng, 4096))
        assert 0 <= s.min() and s.max() < rng and 0 <= j.min() and j.max() < min(rng, 4096)
        assert rng < 4 or len(set(s.tolist())) > 1
    s, j = R.ring_draws(2024, 0, 70000, 7, 5)
    cells = np.bincount(s.astype(np.int64) * 5 + j, minlength=35)
    sd = math.sqrt(70000 * (1 / 35) * (34 / 35))
    print('cells: min %d max %d, 6 sd = %.1f' % (cells.min(), cells.max(), 6 * sd))
    assert cells.sum() == 70000 and (np.abs(cells - 2000) <= 6 * sd).all()


def test_host_twins_refuse_bad_arguments():
    lib = L.load_library()
    n, t = 3, 4
    ring, last, x = RS.np_ring(n, t), RS.last_obs(n), RS.step_inputs(n, 0)
    out = RS.batch_arrays(2)                                       # (held: the descriptors carry addresses only)
    d, o = RS.desc(ring), RS.batch_desc(out)
    P = lambda a: a.ctypes.data  # noqa: E731
    bx = [P(x[k]) for k in ('lidar', 'target', 'action_mask', 'action', 'log_prob')]
    counts, rsum = np.zeros(2, np.int64), np.zeros(1)
    lp = [P(last[k]) for k in RS.KEYS]
    assert lib.hope_ring_before_host(d, 0, *bx) == 0
    assert lib.hope_ring_after_host(d, 3, P(x['reward']), 0, P(x['done']), None, None, None) == 0
    assert lib.hope_ring_sample_host(d, 1, 1, 2, None, None, 0, 0, *lp, o) == 0
    no_T, no_ptr = RS.desc(ring), RS.desc(ring)
    no_T.T, no_ptr.reward = 0, None
    for rc in (lib.hope_ring_before_host(None, 0, *bx), lib.hope_ring_before_host(d, t, *bx), lib.hope_ring_before_host(d, -1, *bx),
               lib.hope_ring_before_host(no_T, 0, *bx), lib.hope_ring_before_host(no_ptr, 0, *bx), lib.hope_ring_before_host(d, 0, None, *bx[1:])):
        assert rc == -1 and b'hope_ring_before_host' in lib.hope_last_error()
    for rc in (lib.hope_ring_after_host(d, t, P(x['reward']), 0, P(x['done']), None, None, None),
               lib.hope_ring_after_host(d, 0, None, 0, P(x['done']), None, None, None),
               lib.hope_ring_after_host(d, 0, P(x['reward']), 0, P(x['done']), P(x['status']), None, P(rsum)),
               lib.hope_ring_after_host(d, 0, P(x['reward']), 0, P(x['done']), None, P(counts), None)):
        assert rc == -1 and b'hope_ring_after_host' in lib.hope_last_error()
    s = np.zeros(2, np.int32)
    for rc in (lib.hope_ring_sample_host(d, t, 1, 2, None, None, 0, 0, *lp, o), lib.hope_ring_sample_host(d, 0, 0, 2, None, None, 0, 0, *lp, o),
               lib.hope_ring_sample_host(d, 0, t + 1, 2, None, None, 0, 0, *lp, o), lib.hope_ring_sample_host(d, 0, 1, 0, None, None, 0, 0, *lp, o),
               lib.hope_ring_sample_host(d, 0, 1, 2, P(s), None, 0, 0, *lp, o), lib.hope_ring_sample_host(d, 0, 1, 2, None, None, 0, 0, *lp, None),
               lib.hope_ring_sample_host(d, 0, 1, 2, None, None, 0, 0, None, *lp[1:], o)):
        assert rc == -1 and b'hope_ring_sample_host' in lib.hope_last_error()
    assert (counts == 0).all() and rsum[0] == 0.0


# ---- DeviceTransitionRing on the CPU stand-in env ------------------------------------------------------------------------------
def _small_scenes(n, seed=3):
    from hope_amd.scenes import SceneSource
    src = SceneSource(levels=('Normal', 'Complex', 'Extrem'), seed=seed)
    return [src.draw() for _ in range(n)]


def _recording(env, log):
    """the env, with every step's reward appended to `log`"""
    inner = env.step

    def step(*a, **kw):
        out = inner(*a, **kw)
        log.append(env.reward.detach().to(torch.float64).cpu().numpy().copy())
        return out
    env.step = step
    return env


def test_ppo_trainer_with_the_device_ring():
    """PPOTrainer(ring='device') against ring=None, same seed: the ring tensors and the losses of two updates bit for bit, stats()
    equal in episodes and success_rate, mean_reward of either within its order's bound of the exact mean"""
    from fake_env import OracleEnv
    scenes = _small_scenes(12)
    runs = []
    for ring in (None, 'device'):
        torch.manual_seed(0)
        ag = A.BatchedPPO(device='cpu', use_img=False, lr=1e-4, mini_batch=24, mini_epoch=2)
        log = []
        tr = R.PPOTrainer(_recording(OracleEnv(scenes), log), ag, horizon=4, seed=1, ring=ring)
        assert isinstance(tr.ring, R.DeviceTransitionRing if ring else R.TransitionRing)
        losses = [o for o in (tr.step() for _ in range(8)) if o is not None]
        assert tr.updates == 2 and len(losses) == 2
        runs.append((tr, losses, log))
    (t0, l0, log0), (t1, l1, log1) = runs
    assert not t1.ring.on_device and np.array_equal(np.array(log0), np.array(log1))
    assert np.array_equal(np.array(l0, np.float64).view(np.uint64), np.array(l1, np.float64).view(np.uint64))
    for got, want in zip(_flat((t1.ring.obs, t1.ring.action, t1.ring.reward, t1.ring.done, t1.ring.log_prob)),
                         _flat((t0.ring.obs, t0.ring.action, t0.ring.reward, t0.ring.done, t0.ring.log_prob))):
        assert np.array_equal(RS.words(got), RS.words(want))
    s0, s1 = t0.stats(), t1.stats()
    assert s0['steps'] == s1['steps'] == 8 and s0['episodes'] == s1['episodes'] and s0['success_rate'] == s1['success_rate']
    assert int(t1.ring.counts[0]) == s1['episodes'] and float(t0.episodes) == s0['episodes'] and float(t0.reward_sum) != 0.0
    terms = np.concatenate(log1).tolist()
    exact, scale = math.fsum(terms), math.fsum(abs(v) for v in terms)
    assert abs(s1['mean_reward'] * 96 - exact) <= RS.sum_bound(12, 8, scale) + abs(exact) * RS.U        # (the division rounds once more)
    assert abs(s0['mean_reward'] * 96 - exact) <= (12 + 8 + 1) * RS.U * scale + abs(exact) * RS.U       # torch: at most n additions per step
    with pytest.raises(ValueError):
        R.PPOTrainer(OracleEnv(scenes[:2]), A.BatchedPPO(device='cpu', use_img=False), ring='gpu')
    with pytest.raises(ValueError):
        R.SACTrainer(OracleEnv(scenes[:2]), A.BatchedSAC(device='cpu', use_img=False), ring=True)


def test_sac_trainer_with_the_device_ring():
    """SACTrainer(ring='device'): every update's batch is the torch gather from the ring's own tensors at ring_draws of its seed and
    counter; and with both rings fed the same choices the two trainers' losses are equal"""
    from fake_env import OracleEnv
    scenes = _small_scenes(8)
    n, horizon, batch = 8, 3, 16
    torch.manual_seed(0)
    ag = A.BatchedSAC(device='cpu', use_img=False, lr=1e-4, batch_size=batch)
    tr = R.SACTrainer(OracleEnv(scenes), ag, horizon=horizon, update_every=2, seed=1, ring='device')
    ring, inner, seen = tr.ring, ag.update, []

    def update(b):
        s, j = R.ring_draws(ring.seed, ring.counter - 1, batch, n, ring.size)
        ref = R.TransitionRing(n, horizon, ag.keys, 'cpu')
        ref.obs, ref.action, ref.log_prob, ref.reward, ref.done, ref.head, ref.size = ring.obs, ring.action, ring.log_prob, ring.reward, ring.done, ring.head, ring.size
        want = ref.sample(batch, tr.last_obs(), index=(s, j))
        for k in ag.keys:
            assert np.array_equal(RS.words(b['obs'][k]), RS.words(want['obs'][k])) and np.array_equal(RS.words(b['next_obs'][k]), RS.words(want['next_obs'][k]))
        for k in ('action', 'reward', 'done'):
            assert np.array_equal(RS.words(b[k]), RS.words(want[k])), k
        assert np.array_equal(b['idx'].numpy(), RS.expected_idx(ring.head, ring.size, horizon, s, j))
        seen.append(ring.counter)
        return inner(b)
    ag.update = update
    out = [tr.step() for _ in range(horizon + 2 * 2 + 1)]
    assert seen == [1, 2, 3] and tr.updates == 3 and all(np.isfinite(o).all() for o in out if o is not None)
    assert tr.stats()['episodes'] == int(ring.counts[0])
    runs = []
    for kind in (None, 'device'):
        torch.manual_seed(0)
        ag = A.BatchedSAC(device='cpu', use_img=False, lr=1e-4, batch_size=batch)
        tr = R.SACTrainer(OracleEnv(scenes), ag, horizon=horizon, update_every=2, seed=1, ring=kind)
        calls, sample = [0], tr.ring.sample

        def spy(batch_size, last, generator=None, index=None, calls=calls, sample=sample, tr=tr):
            s, j = R.ring_draws(77, calls[0], batch_size, n, tr.ring.size)
            calls[0] += 1
            return sample(batch_size, last, generator, index=(s, j))
        tr.ring.sample = spy
        runs.append([o for o in (tr.step() for _ in range(horizon + 2 * 2 + 1)) if o is not None])
    assert len(runs[0]) == 3 and np.array_equal(np.array(runs[0], np.float64).view(np.uint64), np.array(runs[1], np.float64).view(np.uint64))


# ---- the sanitizer driver of the twins -----------------------------------------------------------------------------------------
def test_sanitizer_driver_of_the_twins_runs_clean(tmp_path):
    """tests/ring_host_sanitize.cpp, a stand-alone program, compiled by the host compiler with -fsanitize=address,undefined"""
    cxx = os.environ.get('CXX') or shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    assert cxx, 'no host C++ compiler'
    exe = str(tmp_path / 'ring_host_sanitize')
    cmd = [cxx, '-std=c++17', '-O1', '-g', '-ffp-contract=off', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
           '-I' + os.path.join(ROOT, 'include'), '-I' + os.path.join(ROOT, 'hope_amd', 'csrc'), os.path.join(ROOT, 'tests', 'ring_host_sanitize.cpp'),
           '-o', exe]
    # the runtime linked into the program where the compiler can (gcc's switch; clang does so by default and may not know it)
    if subprocess.run(cmd + ['-static-libasan'], capture_output=True).returncode != 0:
        subprocess.check_call(cmd)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and 'clean' in r.stdout, (r.returncode, r.stdout, r.stderr)
