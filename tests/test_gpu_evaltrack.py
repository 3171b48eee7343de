"""k_eval_begin / k_eval_override / k_eval_track / k_eval_records (hope_amd/csrc/hope_evaltrack_kernel.h) on the device: bit-equal to
their host twins over the scripted episodes, inside the evaluator's real loop next to the torch bookkeeping, and misused."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import evaltrack_script as S  # noqa: E402

pytestmark = pytest.mark.gpu

TORCH = {np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64}


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _words(t):
    a = t.cpu().numpy()
    return a.view({4: np.uint32, 8: np.uint64, 1: np.uint8}[a.dtype.itemsize])


def _script_on_device(env, script, act_dtype, seed):
    """the script through the explicit-pointer form, compared with the twin's snapshot after every call"""
    dev = env.device
    tw, snaps = S.run_twin(script, act_dtype, supplied_u='alt', seed=seed)
    env.eval_begin(_dev(script['first'][0], dev), _dev(script['first'][1], dev))
    assert np.array_equal(env.eval_state(), snaps[0][1]), 'begin'
    for t, s in enumerate(script['steps']):
        _, st, act, active, _, _ = snaps[1 + 2 * t]
        a = _dev(s['action'].astype(act_dtype), dev)
        u = _dev(s['u'], dev) if S.uses_u('alt', t) else None
        alive = env.eval_override(a, u, seed, t)
        assert alive is env.eval_alive
        assert np.array_equal(env.eval_state(), st), (t, 'override: state')
        assert np.array_equal(_words(a), act.view(_words(a).dtype)), (t, 'override: actions')
        assert np.array_equal(alive.cpu().numpy(), active), (t, 'override: active')
        _, st, _, _, word, done = snaps[2 + 2 * t]
        w, d = env.eval_track(*(_dev(s[k], dev) for k in ('target', 'pose', 'reward', 'status', 'done', 'rs_word')))
        assert w is env.eval_word and d is env.eval_done
        assert np.array_equal(env.eval_state(), st), (t, 'track: state')
        assert np.array_equal(w.cpu().numpy(), word) and np.array_equal(d.cpu().numpy(), done), (t, 'track: word / done')
    rec = env.eval_records()
    assert rec.dtype == torch.float32 and rec.shape == (env.n, 4)
    assert np.array_equal(_words(rec), tw.records().view(np.uint32)), 'records'
    return tw


@pytest.mark.parametrize('n', S.SIZES)
@pytest.mark.parametrize('obs_dtype', [np.float32, np.float64])
def test_kernels_equal_the_host_twins_bit_for_bit(n, obs_dtype):
    """a lone lane, a full wave, a wave plus one lane, a partial third wave; float32 and float64 observations, each with float32 and
    float64 action buffers; supplied and counter-based draws alternate"""
    from hope_amd import ParkingBatch
    env = ParkingBatch(n, 32, obs_dtype=TORCH[np.dtype(obs_dtype)])
    env.enable_eval_tracker()
    script = S.make_script(n, obs_dtype=obs_dtype)
    for act_dtype, seed in ((np.float32, 3), (np.float64, 2 ** 63 + 11)):
        _script_on_device(env, script, act_dtype, seed)
    env.close()


# ---- the evaluator's real loop ---------------------------------------------------------------------------------------------------
N_EVAL, MAX_STEPS, EVAL_SEED = 130, 40, 5


def _run(scenes, agent, tracker):
    from hope_amd import ParkingBatch
    from hope_amd import evaluate as E
    env = ParkingBatch(N_EVAL, 32)
    env.set_scenes(np.arange(N_EVAL), scenes)
    ev = E.BatchedEvaluator(env, agent, post_proc_action=True, use_planner='device', chooser='device', seed=EVAL_SEED, tracker=tracker)
    overrides = [0]
    if tracker is None:
        ev._stuck_uniform = lambda step: torch.from_numpy(E.stuck_uniforms(EVAL_SEED, step, env.n)).to(env.device)
    else:
        tr = ev.tracker
        assert tr.on_device and tr.alive is env.eval_alive
        orig = tr.override

        def count(action, u=None):
            if tr.counter > 0:
                _, _, alive, stuck = S.decode(env.eval_state())
                overrides[0] += int((alive & stuck).sum())
            return orig(action, u)
        tr.override = count
    rec = ev.run(max_steps=MAX_STEPS, gather=False, levels=True).cpu().numpy().copy()
    alive = S.decode(env.eval_state())[2] if tracker is not None else None
    env.close()
    return rec, overrides[0], alive


@pytest.fixture(scope='module')
def loop_runs():
    from hope_amd import agents as A
    from test_evaluate import _scenes
    torch.manual_seed(0)
    scenes = _scenes(N_EVAL)
    agent = A.BatchedPPO(device='cuda:0', use_img=False)
    return _run(scenes, agent, None), _run(scenes, agent, 'device')


def test_evaluator_loop_with_the_tracker_matches_the_torch_bookkeeping(loop_runs):
    (ref, _, _), (got, overrides, alive) = loop_runs
    print('stuck overrides after step 1:', overrides, ' finished:', int((got[:, 0] != 1).sum()), ' alive at the end:', int((got[:, 0] == 1).sum()))
    assert got.shape == ref.shape == (N_EVAL, 5) and got.dtype == ref.dtype == np.float32
    assert np.array_equal(got[:, :3].view(np.uint32), ref[:, :3].view(np.uint32))            # status, steps, reward: raw words
    # torch's norm and hm_hypot differ by a few float64 ulp per step over <= 40 steps, far below a float32 ulp: the rounding to
    # float32 can differ by one ulp = 2^-23; the bound allows a factor of two over that
    assert (np.abs(got[:, 3] - ref[:, 3]) <= 2.0 ** -22 * np.abs(ref[:, 3])).all()
    # the premise (the policy's bits differ from the CPU's: asserted, not assumed)
    assert overrides >= 1
    assert ((got[:, 0] != 1) & (got[:, 1] < MAX_STEPS)).any()
    assert (got[:, 0] == 1).any() and (got[got[:, 0] == 1, 1] == MAX_STEPS).all()
    assert np.array_equal(alive == 1, got[:, 0] == 1)


def test_map_levels_ride_along_as_before(loop_runs):
    (ref, _, _), (got, _, _) = loop_runs
    assert np.array_equal(got[:, 4], ref[:, 4]) and set(np.unique(got[:, 4])) <= {0.0, 1.0, 2.0} and len(np.unique(got[:, 4])) > 1


# ---- misuse ------------------------------------------------------------------------------------------------------------------------
def test_misuse_fails_loudly_and_the_handle_stays_usable():
    """HOPE_ESTATE before enable; HOPE_EINVAL for a NULL required pointer or a misaligned buffer, refused before anything is
    launched; after every error a correct call succeeds and matches the twin; disable then enable starts a usable tracker"""
    from hope_amd import ParkingBatch
    from hope_amd import _lib as L
    n = 70
    env = ParkingBatch(n, 32)
    dev, lib = env.device, env.lib
    script = S.make_script(n, seed=9)
    P = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
    a = torch.zeros((n, 2), device=dev)
    for call in (env.eval_begin, lambda: env.eval_override(a), env.eval_track, env.eval_records, env.eval_state):
        with pytest.raises(L.HopeError, match='code -5'):                                  # HOPE_ESTATE
            call()
    assert b'tracker is off' in lib.hope_last_error()
    assert lib.hope_env_eval_disable(env.h) == 0                                           # (idempotent, like the planner's)
    box = S.box()
    bad = box.copy()
    bad[2] = np.nan
    assert lib.hope_env_eval_enable(env.h, None) == -1 and lib.hope_env_eval_enable(env.h, bad.ctypes.data) == -1
    with pytest.raises(L.HopeError, match='code -5'):
        env.eval_begin()
    env.enable_eval_tracker()
    first = [_dev(x, dev) for x in script['first']]
    s0 = script['steps'][0]
    obs = [_dev(s0[k], dev) for k in ('target', 'pose', 'reward', 'status', 'done', 'rs_word')]
    stream = env._stream()
    tw = S.Twin(n)
    tw.begin(*script['first'])

    def good_begin():
        env.eval_begin(*first)
        assert np.array_equal(env.eval_state(), tw.state)
    good_begin()
    for args in ((None, P(first[1])), (P(first[0]), None), (C.c_void_p(first[0].data_ptr() + 2), P(first[1]))):
        assert lib.hope_env_eval_begin(env.h, *args, stream) == -1, args                   # HOPE_EINVAL
        good_begin()
    act = _dev(s0['action'].astype(np.float32), dev)
    keep = act.clone()
    alive = env.eval_alive
    for args in ((None, 0, None, 0, 0, P(alive)), (P(act), 0, None, 0, 0, None), (C.c_void_p(act.data_ptr() + 4), 0, None, 0, 0, P(alive)),
                 (P(act), 0, C.c_void_p(first[1].data_ptr() + 4), 0, 0, P(alive))):         # null, null, misaligned rows, misaligned u
        assert lib.hope_env_eval_override(env.h, *args, stream) == -1, args
        assert torch.equal(act, keep)
    want = np.ascontiguousarray(s0['action'].astype(np.float32))
    active = tw.override(want, s0['u'], 1, 0)
    env.eval_override(act, _dev(s0['u'], dev), 1, 0)
    assert np.array_equal(_words(act), want.view(np.uint32)) and np.array_equal(alive.cpu().numpy(), active)
    wo, do = env.eval_word, env.eval_done
    for k in range(8):
        args = [P(t) for t in obs] + [P(wo), P(do)]
        args[k] = None
        assert lib.hope_env_eval_track(env.h, *args, stream) == -1, k
        assert np.array_equal(env.eval_state(), tw.state), k                               # nothing was launched
    args = [P(t) for t in obs] + [P(wo), P(do)]
    args[5] = C.c_void_p(obs[5].data_ptr() + 4)
    assert lib.hope_env_eval_track(env.h, *args, stream) == -1
    assert lib.hope_env_eval_records(env.h, None, stream) == -1 and lib.hope_env_eval_download_state(env.h, None) == -1
    word, done = tw.track(s0)
    w, d = env.eval_track(*obs)
    assert np.array_equal(env.eval_state(), tw.state) and np.array_equal(w.cpu().numpy(), word) and np.array_equal(d.cpu().numpy(), done)
    assert np.array_equal(_words(env.eval_records()), tw.records().view(np.uint32))
    for kw in (dict(target=obs[0].double()), dict(pose=obs[1][:, :2]), dict(reward=obs[2].cpu()), dict(status=obs[3].long()), dict(rs_word=obs[5][:n - 1])):
        with pytest.raises(L.HopeError):
            env.eval_track(**kw)
    with pytest.raises(L.HopeError):
        env.eval_override(act[:n - 1])
    # enabling again keeps the state; disable and enable start from a zeroed block that begin fills
    env.enable_eval_tracker()
    assert np.array_equal(env.eval_state(), tw.state)
    env.disable_eval_tracker()
    with pytest.raises(L.HopeError, match='code -5'):
        env.eval_track(*obs)
    env.enable_eval_tracker()
    assert not env.eval_state().any()
    _script_on_device(env, script, np.float32, 4)
    env.disable_eval_tracker()
    env.disable_eval_tracker()
    env.close()
