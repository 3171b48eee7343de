"""The observation normalisation's rule (hope_amd/csrc/hope_obsnorm_core.h) through its host twin hope_obsnorm_host: against exact
rational statistics, against the reference's own recurrence (tests/golden/agent_glue.npz), its bit-level properties, and
agent_glue.DeviceStateNorm on the CPU stand-in env."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import obsnorm_script as OS  # noqa: E402
from hope_amd import _lib as L  # noqa: E402
from hope_amd import agent_glue as G  # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'agent_glue.npz')


def _batched(stats_of):
    """a BatchedStateNorm holding (n_state, mean, S, std) given as numpy [125] arrays"""
    n, mean, S, std = stats_of
    sn = G.BatchedStateNorm()
    for name, a in (('mean', mean), ('S', S), ('std', std)):
        t = torch.from_numpy(np.asarray(a, dtype=np.float64).copy())
        setattr(sn, name, {'lidar': t[:OS.NL].clone(), 'target': t[OS.NL:].clone()})
    sn.n_state = int(n)
    return sn


# ---- against exact statistics --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('rows,calls', [(1, 3), (2, 3), (63, 3), (64, 3), (65, 3), (193, 2), (321, 2), (2049, 1)])
def test_twin_against_exact_rational_statistics(rows, calls):
    """|mean - exact| <= 1e-13 max(1, max|x|), |std - exact| <= 1e-12 max(1, max|x|) per column after every call: a 64-term
    sequential sum plus at most 12 tree levels is below 80 * 2^-53 ~ 9e-15 relative to max|x| for the mean, the two-pass M2 adds
    second-order terms only -- a tenfold margin.  The numpy restatement of the rule gives the twin's very bits.
    Worst values seen: mean 1.0e-16, std 1.4e-16 of the scale."""
    twin, model, exact = OS.HostNorm(), OS.NumpyNorm(), OS.ExactStats()
    worst = [0.0, 0.0]
    for k in range(calls):
        lidar, target = OS.observations(rows, seed=1000 * rows + k, dtype=(np.float32, np.float64)[k & 1])
        twin(lidar, target, update=True, normalize=False)
        model.update(lidar, target)
        exact.add(lidar, target)
        mean, S, std = twin.stats()
        assert twin.n_state == exact.n == model.n_state
        for got, want, what in ((mean, model.mean, 'mean'), (S, model.S, 'S'), (std, model.std, 'std')):
            assert np.array_equal(OS.words(got), OS.words(want)), (what, rows, k)
        if exact.n == 1:                                           # the first-sample quirk: std is the observation, not sqrt(0)
            continue
        wm, ws = exact.errors(mean, std)
        print(f'rows {rows} call {k}: mean {wm:.3g} std {ws:.3g} of the scale')
        worst = [max(worst[0], wm), max(worst[1], ws)]
        assert wm <= 1e-13 and ws <= 1e-12, (rows, k, wm, ws)
        assert S[7] == 0.0 and std[7] == 0.0                       # the constant column: nothing but exact steps
    print('worst', worst)


# ---- against the reference's recurrence ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('split', [1, 37, 300])
def test_twin_against_the_reference_fixture(split):
    """300 samples of the reference's StateNorm, folded one row at a time, in batches of 37 and in one call; the tolerances
    tests/test_agent_glue.py holds BatchedStateNorm to.  The twin's output is float32, the fixture's normalised target float64: the
    1e-8 is asked of the float64 quotient formed from the twin's statistics after each row, and the twin's float32 output has to
    be exactly that quotient rounded once."""
    g = np.load(GOLD)
    lid, tgt = g['sn_lidar'], g['sn_target']
    assert len(lid) == 300
    twin = OS.HostNorm()
    outs = []
    for a in range(0, len(lid), split):
        _, nt = twin(lid[a:a + split], tgt[a:a + split], update=True, normalize=True)
        mean, _, std = twin.stats()
        q = (tgt[a:a + split].astype(np.float64) - mean[OS.NL:]) / (std[OS.NL:] + 1e-8)
        assert np.array_equal(OS.words(nt), OS.words(q.astype(np.float32)))
        outs.append(q)
    mean, _, std = twin.stats()
    assert twin.n_state == int(g['sn_n'])
    assert np.abs(mean[:OS.NL] - g['sn_mean_lidar']).max() < 1e-10 and np.abs(mean[OS.NL:] - g['sn_mean_target']).max() < 1e-10
    assert np.abs(std[OS.NL:] - g['sn_std_target']).max() < 1e-10
    assert np.abs(std[:OS.NL] - g['sn_std_lidar']).max() < 1e-9
    if split == 1:                                                 # the reference normalises each sample right after folding it in
        assert np.abs(np.concatenate(outs) - g['sn_norm_target']).max() < 1e-8


# ---- bit-level properties ------------------------------------------------------------------------------------------------------
def test_first_sample_quirk():
    for dt in (np.float32, np.float64):
        lidar, target = OS.observations(1, seed=5, dtype=dt)
        twin = OS.HostNorm()
        twin(lidar, target, normalize=False)
        mean, S, std = twin.stats()
        row = np.concatenate([lidar[0], target[0]]).astype(np.float64)
        assert twin.n_state == 1 and np.array_equal(OS.words(mean), OS.words(row)) and np.array_equal(OS.words(std), OS.words(row))
        assert not S.any()
    # a longer first call: row 0 is the first sample, the rest is folded onto it
    lidar, target = OS.observations(70, seed=6)
    a, b = OS.HostNorm(), OS.HostNorm()
    a(lidar, target, normalize=False)
    b(lidar[:1], target[:1], normalize=False)
    b(lidar[1:], target[1:], normalize=False)
    assert a.n_state == b.n_state == 70
    for x, y in zip(a.stats(), b.stats()):
        assert np.array_equal(OS.words(x), OS.words(y))


def test_one_row_call_is_the_welford_step_as_raw_words():
    """mean + d * (1 / n), S + 0 + d * d * (n_state * 1 / n), sqrt(S / n) in numpy's float64 give the same words.  So does
    BatchedStateNorm's CPU update of one row for mean and S; its std is within two ulps only, because torch divides a tensor by a
    Python number through the reciprocal and the rule divides."""
    lidar, target = OS.observations(40, seed=9)
    twin = OS.HostNorm()
    twin(lidar[:20], target[:20], normalize=False)
    for i in range(20, 40):
        n0 = twin.n_state
        mean0, S0, _ = twin.stats()
        sn = _batched((n0, *twin.stats()))
        twin(lidar[i:i + 1], target[i:i + 1], normalize=False)
        x = np.concatenate([lidar[i], target[i]]).astype(np.float64)
        n = float(n0) + 1.0
        d = x - mean0
        want = (mean0 + d * (1.0 / n), S0 + 0.0 + d * d * (float(n0) * 1.0 / n))
        want += (np.sqrt(want[1] / n),)
        sn.update({'lidar': torch.from_numpy(lidar[i:i + 1]), 'target': torch.from_numpy(target[i:i + 1])})
        torch_stats = [np.concatenate([d_['lidar'].numpy(), d_['target'].numpy()]) for d_ in (sn.mean, sn.S, sn.std)]
        for got, w, t, what in zip(twin.stats(), want, torch_stats, ('mean', 'S', 'std')):
            assert np.array_equal(OS.words(got), OS.words(w)), (what, i)
            if what != 'std':
                assert np.array_equal(OS.words(got), OS.words(t)), (what, i, 'BatchedStateNorm')
            else:
                assert (np.abs(got - t) <= 2 * np.spacing(np.abs(got))).all(), (what, i, 'BatchedStateNorm')
        assert twin.n_state == n0 + 1 == sn.n_state


@pytest.mark.parametrize('dt', [np.float32, np.float64])
def test_normalize_equals_batched_state_norm_bit_for_bit(dt):
    """the same statistics in both: out == BatchedStateNorm.normalize(...).float() as raw words"""
    lidar, target = OS.observations(300, seed=12)
    twin = OS.HostNorm()
    twin(lidar[:200], target[:200], normalize=False)
    sn = _batched((twin.n_state, *twin.stats()))
    lq, tq = OS.observations(131, seed=13, dtype=dt)
    if dt == np.float64:                                           # values that are no float32
        lq, tq = lq * (1.0 + 2.0 ** -40), tq / 3.0
    before = [a.copy() for a in twin.stats()]
    nl, nt = twin(lq, tq, update=False, normalize=True)
    want = sn.normalize({'lidar': torch.from_numpy(lq), 'target': torch.from_numpy(tq)})
    assert np.array_equal(OS.words(nl), OS.words(want['lidar'].float().numpy()))
    assert np.array_equal(OS.words(nt), OS.words(want['target'].float().numpy()))
    assert twin.n_state == 200 and all(np.array_equal(OS.words(a), OS.words(b)) for a, b in zip(before, twin.stats()))
    # with both flags the call folds first and normalises with the new statistics
    both, split = OS.HostNorm(), OS.HostNorm()
    for t in (both, split):
        t.load(twin.n_state, *twin.stats())
    o1 = both(lq, tq, update=True, normalize=True)
    split(lq, tq, update=True, normalize=False)
    o2 = split(lq, tq, update=False, normalize=True)
    assert all(np.array_equal(OS.words(a), OS.words(b)) for a, b in zip(o1, o2))
    assert all(np.array_equal(OS.words(a), OS.words(b)) for a, b in zip(both.stats(), split.stats()))


def test_misuse_of_the_host_twin():
    twin = OS.HostNorm()
    lidar, target = OS.observations(3, seed=1)
    ol, ot = np.zeros((3, OS.NL), np.float32), np.zeros((3, OS.NT), np.float32)
    U, N = L.OBSNORM_UPDATE, L.OBSNORM_NORMALIZE
    assert twin.raw(lidar, target, 3, 0, U | N, ol, ot) == 0
    for args in ((None, target, 3, 0, U, None, None), (lidar, None, 3, 0, U, None, None), (lidar, target, 0, 0, U, None, None),
                 (lidar, target, -1, 0, U, None, None), (lidar, target, 3, 0, 0, ol, ot), (lidar, target, 3, 0, 4, ol, ot),
                 (lidar, target, 3, 0, N, None, ot), (lidar, target, 3, 0, N, ol, None), (lidar, target, 3, 0, U | N, None, None)):
        assert twin.raw(*args) == -1, args                         # HOPE_EINVAL
        assert b'hope_obsnorm_host' in twin.lib.hope_last_error()
    assert twin.lib.hope_obsnorm_host(None, lidar.ctypes.data, target.ctypes.data, 3, 0, U, None, None) == -1
    assert twin.n_state == 3                                       # the refused calls folded nothing
    twin.state.n_state = -1
    assert twin.raw(lidar, target, 3, 0, U, None, None) == -1
    with pytest.raises(L.HopeError):
        L.check(twin.raw(lidar, target, 3, 0, U, None, None), 'hope_obsnorm_host')


# ---- DeviceStateNorm on the CPU stand-in env -----------------------------------------------------------------------------------
def _small_scenes(n, seed=3):
    from hope_amd.scenes import SceneSource
    src = SceneSource(levels=('Normal', 'Complex', 'Extrem'), seed=seed)
    return [src.draw() for _ in range(n)]


def test_device_state_norm_surface_and_round_trip():
    from fake_env import OracleEnv
    env = OracleEnv(_small_scenes(6))
    lidar, target = (torch.from_numpy(a) for a in OS.observations(6, seed=21))
    sb = G.BatchedStateNorm()
    for k in range(3):
        sb.update({'lidar': lidar + k, 'target': target * (k + 1)})
    dn = G.DeviceStateNorm(env, from_norm=sb)
    assert not dn.on_device and dn.n_state == sb.n_state == 18 and dn.modal == sb.modal and dn.fixed is False
    for name in ('mean', 'S', 'std'):                              # dicts of float64 tensors, equal to the source bit for bit
        got, want = getattr(dn, name), getattr(sb, name)
        assert set(got) == {'lidar', 'target'}
        for k in got:
            assert got[k].dtype == torch.float64 and got[k].shape == want[k].shape and torch.equal(got[k], want[k])
    back = dn.to_batched()
    assert isinstance(back, G.BatchedStateNorm) and back.n_state == 18 and back.fixed is False
    assert all(torch.equal(getattr(back, nm)[k], getattr(sb, nm)[k]) for nm in ('mean', 'S', 'std') for k in sb.modal)
    # normalize: float32, the bits of the torch class; other keys pass through; one observation as a vector
    obs = {'lidar': lidar, 'target': target, 'action_mask': torch.ones(6, 42)}
    out = dn.normalize(obs)
    want = sb.normalize(obs)
    assert out['action_mask'] is obs['action_mask'] and out['lidar'].dtype == torch.float32
    assert torch.equal(out['lidar'], want['lidar'].float()) and torch.equal(out['target'], want['target'].float())
    one = dn.normalize({'lidar': lidar[2], 'target': target[2]})
    assert one['target'].shape == (5,) and torch.equal(one['target'], want['target'][2].float())
    with pytest.raises(ValueError):
        dn.normalize({'target': target})
    # update_and_normalize == update, then normalize; the statistics follow the torch class within the last bits
    twin = G.DeviceStateNorm(env, from_norm=dn)
    fused = {k: v.clone() for k, v in dn.update_and_normalize(obs).items()}
    twin.update(obs)
    split = twin.normalize(obs)
    assert dn.n_state == twin.n_state == 24
    assert all(torch.equal(fused[k], split[k]) for k in ('lidar', 'target'))
    sb.update(obs)
    assert all((dn.mean[k] - sb.mean[k]).abs().max() < 1e-12 and (dn.std[k] - sb.std[k]).abs().max() < 1e-12 for k in sb.modal)
    # fixed changes nothing
    dn.fix_parameters()
    before = [np.concatenate([d['lidar'].numpy(), d['target'].numpy()]) for d in (dn.mean, dn.S, dn.std)]
    dn.update({'lidar': lidar * 3, 'target': target})
    out = dn.update_and_normalize({'lidar': lidar * 3, 'target': target})
    after = [np.concatenate([d['lidar'].numpy(), d['target'].numpy()]) for d in (dn.mean, dn.S, dn.std)]
    assert dn.n_state == 24 and all(np.array_equal(OS.words(a), OS.words(b)) for a, b in zip(before, after))
    assert torch.isfinite(out['lidar']).all()
    assert dn.to_batched().fixed is True and G.DeviceStateNorm(env, from_norm=dn).fixed is True


def test_loops_take_the_device_norm_on_the_cpu():
    """PPOTrainer(obs_norm='device') on the oracle env: the agent's state_norm is swapped, the count is the host's, the losses are
    finite, the stored observations are what the torch class gives for the device's statistics; obs_norm=None is untouched"""
    from fake_env import OracleEnv
    from hope_amd import agents as A
    from hope_amd import evaluate as E
    from hope_amd.rollout import PPOTrainer
    scenes = _small_scenes(8)

    def run(obs_norm, steps=6):
        torch.manual_seed(0)
        env = OracleEnv(scenes)
        ag = A.BatchedPPO(device='cpu', use_img=False, lr=1e-4, mini_batch=24, mini_epoch=2)
        tr = PPOTrainer(env, ag, horizon=3, seed=1, use_planner='device', obs_norm=obs_norm)
        losses = [tr.step() for _ in range(steps)]
        return tr, ag, [x for x in losses if x is not None]

    tr, ag, losses = run('device')
    assert isinstance(ag.state_norm, G.DeviceStateNorm) and tr.obs_norm is ag.state_norm and not ag.state_norm.on_device
    assert ag.state_norm.n_state == 8 * (6 + 1)                    # the first observation and one per step, 8 scenes each
    assert len(losses) == 2 and all(math.isfinite(float(v)) for l_ in losses for v in l_), losses
    last = tr.last_obs()
    want = ag.state_norm.to_batched().normalize({'lidar': tr.env.lidar, 'target': tr.env.target})
    assert torch.equal(last['lidar'], want['lidar'].float()) and torch.equal(last['target'], want['target'].float())
    assert last['action_mask'].dtype == torch.float32 and torch.equal(last['action_mask'], tr.env.action_mask.float())
    base, ag0, _ = run(None)
    again, _, _ = run(None)
    assert isinstance(ag0.state_norm, G.BatchedStateNorm) and base.obs_norm is None
    assert torch.equal(base.ring.action, again.ring.action) and base.stats() == again.stats()
    ev = E.BatchedEvaluator(OracleEnv(scenes), A.BatchedPPO(device='cpu', use_img=False), seed=5, use_planner='device', obs_norm='device')
    assert isinstance(ev.agent.state_norm, G.DeviceStateNorm) and torch.isfinite(ev.run(max_steps=6, gather=False)).all()
    with pytest.raises(ValueError):
        PPOTrainer(OracleEnv(scenes[:2]), A.BatchedPPO(device='cpu', use_img=False), obs_norm='gpu')
    with pytest.raises(ValueError):
        PPOTrainer(OracleEnv(scenes[:2]), A.BatchedPPO(device='cpu', use_img=False, state_norm=False), obs_norm='device')
