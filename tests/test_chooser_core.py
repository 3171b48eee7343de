"""The masked action choice of hope_amd/csrc/hope_chooser_core.h through its host twin hope_chooser_host: against the reference's
own probability vectors (tests/golden/agent_glue.npz), against a float64 numpy restatement of ActionMask.choose_action on random
rows, against hand-computed expectations on the edges of the rule, the counter-based draws, the log-probability, and inside the
rollout / evaluation loops on the CPU stand-in env."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import chooser_script as CS  # noqa: E402

N_RANDOM = 200_000


def test_host_twin_reproduces_the_reference_probability_vectors(gold):
    """the fixture's pa_probs (ActionMask.choose_action's own vector) to 1e-12 absolute: the torch twin is held to 1e-13, the
    log / exp round trip of std adds up to z^2 2^-52 per entry"""
    g = gold('agent_glue.npz')
    out = CS.host_choose(g['pa_mean'], np.log(g['pa_std']), g['pa_mask'], u=np.full(200, 0.5))
    assert np.abs(out['probs'] - g['pa_probs']).max() < 1e-12
    assert (out['idx'] < 64).all() and (g['pa_mask'][np.arange(200), out['idx']] > 0).all()


@pytest.fixture(scope='module')
def random_run():
    mean, log_std, mask, u = CS.random_rows(N_RANDOM)
    out = CS.host_choose(mean.astype(np.float64), log_std, mask, u=u)
    stats = {}
    p = CS.numpy_probs(mean, np.exp(log_std), mask, stats)
    return mean, log_std, mask, u, out, p, stats


def test_random_rows_probabilities_equal_the_numpy_restatement(random_run):
    """200 000 rows: every non-zero probability within 1e-12 relative of action_mask.py:212-224 in float64 numpy"""
    mean, log_std, mask, u, out, p, stats = random_run
    assert stats['clipped'] > 0.2                                 # (the clip is exercised: ~31 % of the per-dimension terms)
    nz = p > 0
    assert np.array_equal(nz, out['probs'] > 0)
    rel = np.abs(out['probs'][nz] - p[nz]) / p[nz]
    print('max relative difference of probs:', rel.max())
    assert rel.max() <= 1e-12
    assert (out['idx'] < 64).all()                                # no row of this generator is degenerate


def test_random_rows_indices_equal_the_cdf_searchsorted_pick(random_run):
    """the same u through np.random.choice's rule (cdf, searchsorted right); rows with u within 1e-9 of a cdf value may be skipped,
    at most 0.1 % of them"""
    mean, log_std, mask, u, out, p, _ = random_run
    want, near = CS.numpy_pick(p, u)
    print('rows skipped:', int(near.sum()), 'index differences outside the band:', int((want != out['idx'])[~near].sum()))
    assert near.mean() <= 1e-3
    assert np.array_equal(want[~near], out['idx'][~near])
    a = CS.ACTS[out['idx']].astype(np.float32).clip(-1, 1)
    assert np.array_equal(out['action'], a) and np.array_equal(out['action_f32'], a)


def test_log_probability_within_one_float32_ulp_of_gaussian_log_prob(random_run):
    from hope_amd.policy import gaussian_log_prob
    mean, log_std, mask, u, out, p, _ = random_run
    want = gaussian_log_prob(torch.from_numpy(mean).double(), torch.from_numpy(log_std).double(), torch.from_numpy(out['action_f32']).double())
    d = CS.ulp_distance_f32(out['log_prob'], want.float().numpy())
    print('max ulp distance of log_prob:', d.max())
    assert d.max() <= 1


def test_input_and_output_types_agree():
    """float32 inputs and masks are the float64 call on the same numbers; a float64 action buffer is (double) action_f32; a
    broadcast log_std row is the repeated row"""
    mean, log_std, mask, u = CS.random_rows(500, seed=3)
    ls32 = log_std.astype(np.float32)
    m32 = mask.astype(np.float32)
    a = CS.host_choose(mean, ls32, m32, u=u)
    b = CS.host_choose(mean.astype(np.float64), ls32.astype(np.float64), m32.astype(np.float64), u=u, action_f64=True)
    for k in ('idx', 'log_prob', 'probs', 'action_f32'):
        assert np.array_equal(a[k], b[k]), k
    assert b['action'].dtype == np.float64 and np.array_equal(b['action'], a['action_f32'].astype(np.float64))
    one = CS.host_choose(mean, ls32[:1], m32, u=u)
    rep = CS.host_choose(mean, np.repeat(ls32[:1], 500, axis=0), m32, u=u)
    for k in one:
        assert np.array_equal(one[k], rep[k]), k


@pytest.mark.parametrize('f64', [True, False])
def test_edge_rows_against_hand_computed_expectations(f64):
    """single-entry masks at k = 0 / 20 / 41, u = 0 and u = 1 - 2^-53, u one ulp either side of every cum_k / S of a row whose sums
    are exact, log_std = -5 (uniform over the masked set) and +2, mean = +-1, an all-zero mask, NaN / infinite means, executing rows,
    the float64 action buffer; nothing raises"""
    rows, want = CS.edge_rows()
    dt = np.float64 if f64 else np.float32
    out = CS.host_choose(rows['mean'].astype(dt), rows['log_std'].astype(dt), rows['mask'].astype(dt), rows['planned'], rows['executing'],
                         rows['u'], action_f64=f64)
    CS.check_edge_rows(rows, want, out)


def test_u_outside_the_unit_interval_and_extreme_log_std_stay_legal():
    mean, log_std, mask, u = CS.random_rows(64, seed=9)
    u[:8] = [1.0, 2.0, -1.0, np.nan, np.inf, -np.inf, 1e300, -0.0]
    log_std[8:14] = [[-800, 0], [800, 0], [0, 1e30], [-1e30, -1e30], [710, 710], [-745, 3]]
    out = CS.host_choose(mean.astype(np.float64), log_std, mask, u=u)
    k = out['idx'] & 63
    assert (k < 42).all() and np.isfinite(out['action']).all()
    ok = out['idx'] < 64
    assert (mask[np.arange(64), k][ok] > 0).all()                 # an unflagged row never takes a masked-out action
    assert ok[:8].all() and ok[14:].all()


def test_bad_arguments():
    lib = CS.L.load_library()
    mean, log_std, mask, u = CS.random_rows(4, seed=1)
    mean = mean.astype(np.float64)
    act = np.zeros((4, 2), np.float32)
    ex = np.zeros(4, np.uint8)
    pl = np.zeros((4, 2))
    bad_steer = CS.ACTS.copy()
    bad_steer[30, 0] += 0.01                                      # a backward steer that is not its forward twin
    P = lambda a: None if a is None else a.ctypes.data  # noqa: E731

    def call(n=4, acts=CS.ACTS, mean=mean, ls=log_std, stride=2, mask=mask, planned=None, executing=None, action=act):
        return lib.hope_chooser_host(n, P(acts), P(mean), P(ls), stride, 1, P(mask), 1, P(planned), P(executing), P(u), 0, 0, 0, P(action), 0, None, None,
                                     None, None)
    assert call() == 0
    assert call(planned=pl, executing=ex) == 0
    for kw in ({'n': 0}, {'acts': None}, {'mean': None}, {'ls': None}, {'mask': None}, {'action': None}, {'stride': 1}, {'planned': pl}, {'executing': ex},
               {'acts': bad_steer}, {'acts': np.zeros((42, 2)) + np.arange(42)[:, None]}):
        assert call(**kw) == -1, kw


# ---- counter-based draws ---------------------------------------------------------------------------------------------------------
def test_counter_based_draws_are_a_function_of_seed_counter_and_scene():
    mean, log_std, mask, _ = CS.random_rows(1001, seed=4)
    a = CS.host_choose(mean, log_std, mask, seed=11, counter=5)
    b = CS.host_choose(mean, log_std, mask, seed=11, counter=5)
    assert all(np.array_equal(a[k], b[k]) for k in a)
    lo = CS.host_choose(mean[:400], log_std[:400], mask[:400], seed=11, counter=5)
    hi = CS.host_choose(mean[400:], log_std[400:], mask[400:], seed=11, counter=5, scene0=400)
    for k in a:
        assert np.array_equal(a[k], np.concatenate([lo[k], hi[k]])), k
    c = CS.host_choose(mean, log_std, mask, seed=11, counter=6)
    d = CS.host_choose(mean, log_std, mask, seed=12, counter=5)
    assert (a['idx'] != c['idx']).mean() > 0.5 and (a['idx'] != d['idx']).mean() > 0.5


def test_scenes_of_one_counter_follow_the_distribution():
    """one fixed row in 2 x 100 000 scenes: every |frequency_k - p_k| <= 5 sqrt(p_k (1 - p_k) / n).  Deterministic: a failure is a bug"""
    n = 200_000
    mean = np.array([[0.2, 0.4]], np.float32)
    log_std = np.array([[-0.4, -0.1]], np.float32)
    mask = np.zeros((1, 42), np.float32)
    mask[0, ::3] = 1.0
    mask[0, 1::5] = 0.4
    p = CS.host_choose(mean, log_std, mask, u=np.zeros(1))['probs'][0]
    # along the scene axis: the same row in 100 000 scenes under two counters (the counter axis is the next test)
    rep = lambda a: np.repeat(a, n // 2, axis=0)  # noqa: E731
    idx = np.concatenate([CS.host_choose(rep(mean), rep(log_std), rep(mask), seed=3, counter=c, probs=False)['idx'] for c in (0, 1)])
    freq = np.bincount(idx, minlength=42) / n
    bound = 5 * np.sqrt(p * (1 - p) / n)
    print('worst |freq - p| / bound:', (np.abs(freq - p) / np.maximum(bound, 1e-300))[p > 0].max())
    assert (np.abs(freq - p) <= bound).all()
    assert (freq[p == 0] == 0).all()


def test_counters_of_one_scene_follow_the_distribution():
    """one fixed row, scene 0, 200 000 consecutive counters: every |frequency_k - p_k| <= 5 sqrt(p_k (1 - p_k) / n).  The draws are
    deterministic: a failure here is a bug, not bad luck with a seed"""
    lib = CS.L.load_library()
    n = 200_000
    mean = np.array([[0.2, 0.4]], np.float64)
    log_std = np.array([[-0.4, -0.1]], np.float64)
    mask = np.zeros((1, 42), np.float64)
    mask[0, ::3] = 1.0
    mask[0, 1::5] = 0.4
    p = CS.host_choose(mean, log_std, mask, u=np.zeros(1))['probs'][0]
    act = np.zeros((1, 2), np.float32)
    idx = np.zeros(1, np.int32)
    args = (1, CS.ACTS.ctypes.data, mean.ctypes.data, log_std.ctypes.data, 0, 1, mask.ctypes.data, 1, None, None, None, 3)
    tail = (0, act.ctypes.data, 0, None, idx.ctypes.data, None, None)
    count = np.zeros(256, np.int64)
    for c in range(n):
        lib.hope_chooser_host(*args, c, *tail)
        count[idx[0]] += 1
    assert count[42:].sum() == 0
    freq = count[:42] / n
    assert (np.abs(freq - p) <= 5 * np.sqrt(p * (1 - p) / n)).all()


# ---- in the loops, on the CPU stand-in env ---------------------------------------------------------------------------------------
def _small_scenes(n, seed=3):
    from hope_amd.scenes import SceneSource
    src = SceneSource(levels=('Normal', 'Complex', 'Extrem'), seed=seed)
    return [src.draw() for _ in range(n)]


def _rollout(scenes, chooser, steps=12):
    from fake_env import OracleEnv
    from hope_amd import agents as A
    from hope_amd.rollout import HopeRollout
    torch.manual_seed(0)
    env = OracleEnv(scenes)
    ro = HopeRollout(env, A.BatchedPPO(device='cpu', use_img=False, lr=1e-4, mini_batch=24, mini_epoch=2), horizon=steps, seed=1,
                     use_planner='device', chooser=chooser)
    for _ in range(steps):
        ro.collect_step()
    return ro


def test_rollout_and_evaluator_take_the_device_chooser_on_the_cpu():
    """HopeRollout and BatchedEvaluator with chooser='device' (the host twin) run and give finite statistics; with chooser=None
    every action and log-probability equals today's path -- a run recorded at the start of this test"""
    from fake_env import OracleEnv
    from hope_amd import agents as A
    from hope_amd import agent_glue as G
    from hope_amd import evaluate as E
    scenes = _small_scenes(10)
    before = _rollout(scenes, None)
    assert before.chooser is None
    ro = _rollout(scenes, 'device')
    assert isinstance(ro.chooser, G.DeviceActionChooser) and not ro.chooser.on_device and ro.chooser.counter == 12
    st = ro.stats()
    assert all(math.isfinite(v) for v in st.values()), st
    a, lp = ro.ring.action, ro.ring.log_prob
    assert torch.isfinite(a).all() and torch.isfinite(lp).all() and a.abs().max() <= 1
    assert ((ro.chooser.idx & 63) < 42).all()
    # the masked choice never takes a masked-out action: the last step's indices against the mask they were drawn under is not
    # kept, so look at the actions -- rows that are not a planner override are rows of the action table
    tab = torch.from_numpy(CS.ACTS.astype(np.float32)).clamp(-1, 1)
    is_row = (a.reshape(-1, 1, 2) == tab.unsqueeze(0)).all(2).any(1)
    assert is_row.float().mean() > 0.5
    again = _rollout(scenes, None)                                # today's path, untouched by the chooser's existence
    assert torch.equal(before.ring.action, again.ring.action) and torch.equal(before.ring.log_prob, again.ring.log_prob)
    assert torch.equal(before.ring.reward, again.ring.reward) and before.stats() == again.stats()
    same = _rollout(scenes, 'device')                             # and the chooser's run is reproduced by its seed
    assert torch.equal(ro.ring.action, same.ring.action) and torch.equal(ro.ring.log_prob, same.ring.log_prob)
    recs = []
    for ch in (None, 'device', None):
        torch.manual_seed(0)
        ev = E.BatchedEvaluator(OracleEnv(scenes), A.BatchedPPO(device='cpu', use_img=False), seed=5, use_planner='device', chooser=ch)
        recs.append(ev.run(max_steps=12, gather=False))
    assert torch.equal(recs[0], recs[2]) and torch.isfinite(recs[1]).all()
    with pytest.raises(ValueError):
        E.BatchedEvaluator(OracleEnv(scenes[:2]), A.BatchedPPO(device='cpu', use_img=False), chooser='gpu')


def test_act_with_a_chooser_keeps_its_signature_and_the_order_of_the_override():
    """_AgentCommon.act(..., chooser=...): plan_fn runs before the choice, executing rows carry (float32) planned, the log-probability
    is gaussian_log_prob of the action returned; use_mask=False ignores the chooser"""
    from fake_env import OracleEnv
    from hope_amd import agents as A
    from hope_amd import agent_glue as G
    from hope_amd.policy import gaussian_log_prob
    scenes = _small_scenes(6)
    env = OracleEnv(scenes)
    env.reset_obs()
    torch.manual_seed(0)
    ag = A.BatchedPPO(device='cpu', use_img=False)
    ch = G.DeviceActionChooser(env, seed=4)
    obs = {'lidar': env.lidar, 'target': env.target, 'action_mask': env.action_mask}
    planned = torch.tensor([[1.0, 0.3], [0.0, 0.0], [-1.0, -1.0], [0.0, 0.0], [0.0, 0.7], [0.0, 0.0]], dtype=torch.float64)
    ex = torch.tensor([1, 0, 1, 0, 1, 0], dtype=torch.bool)
    calls = []

    def plan_fn():
        calls.append(ch.counter)
        return planned, ex
    a, lp, nobs = ag.act(obs, True, None, plan_fn=plan_fn, chooser=ch)
    assert calls == [0] and ch.counter == 1
    assert a.dtype == torch.float32 and a.shape == (6, 2) and lp.shape == (6, 2) and set(nobs) == set(ag.keys)
    assert torch.equal(a[ex], planned[ex].float())
    k = (ch.idx & 63).long()
    assert (env.action_mask[torch.arange(6), k][~ex] > 0).all()
    mean = ag.policy_mean(nobs)
    want = gaussian_log_prob(mean.double(), ag.log_std.detach().double().expand_as(mean), a.double()).float()
    assert CS.ulp_distance_f32(lp.numpy(), want.numpy()).max() <= 1
    assert ch.action_env.dtype == env.action_dtype and torch.equal(ch.action_env.float(), a)
    gen = torch.Generator().manual_seed(3)
    b, _, _ = ag.act(obs, False, gen, planned, ex, chooser=ch)
    gen = torch.Generator().manual_seed(3)
    c, _, _ = ag.act(obs, False, gen, planned, ex)
    assert torch.equal(b, c) and ch.counter == 1
