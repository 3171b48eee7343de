"""The evaluation tracker's rule (hope_amd/csrc/hope_evaltrack_core.h) through its host twins, without a device: the twins against
a scalar restatement of the reference's loop (src/evaluation/eval_utils.py:35-53) over scripted episodes, the counter-based draw
against its numpy restatement, and the evaluator with tracker='device' against the torch bookkeeping on the CPU stand-in env."""
import math

import numpy as np
import pytest
import torch

import evaltrack_script as S
from hope_amd import agents as A
from hope_amd import evaluate as E


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _canon(a):
    """float64 values as the state stores them: every NaN is the one quiet NaN"""
    b = _bits(a).copy()
    b[np.isnan(a)] = S.QNAN
    return b


@pytest.mark.parametrize('n', S.SIZES)
@pytest.mark.parametrize('obs_dtype', [np.float32, np.float64])
def test_twin_matches_a_scalar_restatement_of_eval(n, obs_dtype):
    script = S.make_script(n, obs_dtype=obs_dtype)
    want = S.scalar_replay(script)
    tw, snaps = S.run_twin(script, np.float32)
    assert snaps[0][0] == 'begin'
    steps, status, alive, stuck = S.decode(snaps[0][1])
    assert (steps == 0).all() and (status == 1).all() and (alive == 1).all() and (stuck == 1).all()
    assert np.array_equal(snaps[0][1][:5], _canon(script['first'][0].astype(np.float64).T))
    assert np.array_equal(snaps[0][1][5:7], _canon(script['first'][1][:, :2].T)) and not snaps[0][1][7:9].any()
    for t, s in enumerate(script['steps']):
        _, st_o, act, active, _, _ = snaps[1 + 2 * t]
        _, st, _, _, word, done = snaps[2 + 2 * t]
        assert np.array_equal(st_o, snaps[2 * t][1]), t                          # the override reads the state only
        assert np.array_equal(active, want['alive0'][t]), t
        assert np.array_equal(act.view(np.uint32), S.expected_action(s['action'], want['stuck0'][t], s['u'], np.float32).view(np.uint32)), t
        steps, status, alive, stuck = S.decode(st)
        assert np.array_equal(steps, want['steps'][t]) and np.array_equal(status, want['status'][t]), t
        assert np.array_equal(alive, want['alive'][t]) and np.array_equal(stuck, want['stuck'][t]), t
        assert np.array_equal(st[7], _canon(want['total'][t])), t               # the same float64 additions in the same order
        assert np.array_equal(st[8], _canon(want['path'][t])), t                # == np.sqrt(dx * dx + dy * dy) accumulated
        assert np.array_equal(st[:5], _canon(s['target'].astype(np.float64).T)) and np.array_equal(st[5:7], _canon(s['pose'][:, :2].T)), t
        assert np.array_equal(word, want['word'][t]) and np.array_equal(done, want['done'][t]), t
        # against np.linalg.norm: every displacement is within 2 ulp of it -> steps * 2 * 2^-53 relative
        path, ref = st[8].view(np.float64), want['path_norm'][t]
        ok = np.isfinite(ref)
        assert np.array_equal(np.isnan(path), np.isnan(ref))
        assert (np.abs(path[ok] - ref[ok]) <= want['steps'][t][ok] * 2 * 2.0 ** -53 * np.abs(ref[ok])).all(), t
    assert (tw.state[:9][np.isnan(tw.state[:9].view(np.float64))] == S.QNAN).all()
    rec = tw.records()
    assert np.array_equal(rec[:, 0], want['status'][-1]) and np.array_equal(rec[:, 1], want['steps'][-1])
    with np.errstate(invalid='ignore', over='ignore'):
        sums = np.stack([_canon(want['total'][-1]), _canon(want['path'][-1])], 1).view(np.float64)      # (a NaN sum: the one quiet NaN)
        assert np.array_equal(rec[:, 2:].view(np.uint32), sums.astype(np.float32).view(np.uint32))


def test_the_script_holds_the_rows_a_lane_can_get_wrong():
    """the premise of the test above, and what the rule does on those rows"""
    script = S.make_script(130)
    tw, snaps = S.run_twin(script)
    kind = script['kind']
    track = [snaps[2 + 2 * t] for t in range(S.STEPS)]
    dec = [S.decode(s[1]) for s in track]
    # kind 1: a NaN target component -- never stuck, stored canonical although the input carries a payload and a sign
    k = np.nonzero(kind == 1)[0]
    for t in (3, 4, 5):
        raw = script['steps'][t]['target'][k, 2]
        assert np.isnan(raw).all() and (raw.view(np.uint32) != 0x7FC00000).all()
        assert (dec[t][3][k] == 0).all() and (track[t][1][2, k] == S.QNAN).all()
    # kind 2: -0.0 against +0.0 with the rest constant -- stuck at every step
    k = np.nonzero(kind == 2)[0]
    z = np.stack([script['steps'][t]['target'][k, 0] for t in range(S.STEPS)])
    assert (z == 0).all() and (np.signbit(z[0::2])).all() and not np.signbit(z[1::2]).any()
    assert all((dec[t][3][k] == 1).all() for t in range(S.STEPS))
    # kind 0: frozen after step 5; `done`, a huge reward and a pose jump afterwards change nothing but last_xy / last_target
    k = np.nonzero(kind == 0)[0]
    assert any(script['steps'][t]['done'][k].all() for t in range(6, S.STEPS))
    for t in range(6, S.STEPS):
        assert (dec[t][0][k] == 6).all() and (dec[t][2][k] == 0).all() and np.array_equal(dec[t][1][k], dec[5][1][k])
        assert np.array_equal(track[t][1][7:9, k], track[5][1][7:9, k]) and not track[t][5][k].any() and not track[t][4][k, 6].any()
    # kind 3: a NaN reward -- the sum is the canonical NaN, the path is not touched by it
    k = np.nonzero(kind == 3)[0]
    assert (script['steps'][2]['reward'][k].view(np.uint32) == 0xFFC00777).all()
    assert (tw.state[7, k] == S.QNAN).all() and np.isfinite(tw.state[8, k].view(np.float64)).all()
    # kind 4 finishes on its first step, kind 5 never, kind 6 has the canonical NaN as its path
    assert (dec[-1][0][kind == 4] == 1).all() and (dec[-1][2][kind == 4] == 0).all() and (dec[-1][1][kind == 4] != 1).all()
    assert (dec[-1][0][kind == 5] == S.STEPS).all() and (dec[-1][2][kind == 5] == 1).all() and (dec[-1][1][kind == 5] == 1).all()
    assert (tw.state[8, kind == 6] == S.QNAN).all()
    # stuck and not-stuck rows both occur after the first step, among live and among frozen scenes
    live_stuck = sum(int((dec[t][2] & dec[t][3]).sum()) for t in range(S.STEPS))
    frozen_stuck = sum(int(((1 - dec[t][2]) & dec[t][3]).sum()) for t in range(S.STEPS))
    assert live_stuck > 20 and frozen_stuck > 20 and sum(int((1 - dec[t][3]).sum()) for t in range(S.STEPS)) > 200


def _draws(n, seed, counter, scene0=0, state=None, stride=None, f64=True):
    """the twin's own uniforms: with the box [0, 1] x [0, 1] the float64 action written IS u"""
    from hope_amd import _lib as L
    lib = L.load_library()
    if state is None:
        state = np.zeros((L.EVAL_STATE_WORDS, n), np.uint64)
        state[9] = np.uint64(1 << 41)                                          # every scene stuck
        stride = n
    a = np.full((n, 2), -7.0, np.float64)
    active = np.zeros(n, np.uint8)
    unit = np.array([0.0, 1.0, 0.0, 1.0])
    L.check(lib.hope_eval_override_host(n, stride, state.ctypes.data if isinstance(state, np.ndarray) else state, unit.ctypes.data, a.ctypes.data, 1, None,
                                        seed, counter, scene0, active.ctypes.data), 'override')
    return a


@pytest.mark.parametrize('seed, counter', [(0, 0), (5, 0), (5, 1), (5, 39), (2 ** 64 - 1, 2 ** 40 + 3)])
def test_stuck_uniforms_are_the_twins_draws(seed, counter):
    n = 130
    u = _draws(n, seed, counter)
    assert np.array_equal(u.view(np.uint64), E.stuck_uniforms(seed, counter, n).view(np.uint64))
    assert (u >= 0).all() and (u < 1).all() and len(np.unique(u)) == 2 * n
    # a batch split at an arbitrary row: the same draws
    from hope_amd import _lib as L
    state = np.zeros((L.EVAL_STATE_WORDS, n), np.uint64)
    state[9] = np.uint64(1 << 41)
    for r in (1, 37, 64, 129):
        lo = _draws(r, seed, counter, 0, state, n)
        hi = _draws(n - r, seed, counter, r, state.ctypes.data + 8 * r, n)
        assert np.array_equal(np.concatenate([lo, hi]).view(np.uint64), u.view(np.uint64)), r
    assert np.array_equal(E.stuck_uniforms(seed, counter, 7, scene0=40).view(np.uint64), u[40:47].view(np.uint64))


def test_draw_streams_differ_by_seed_step_and_from_the_choosers():
    a, b, c = E.stuck_uniforms(5, 0, 64), E.stuck_uniforms(5, 1, 64), E.stuck_uniforms(6, 0, 64)
    assert not (a == b).any() and not (a == c).any()
    u = np.concatenate([E.stuck_uniforms(3, t, 4096).ravel() for t in range(8)])
    assert abs(u.mean() - 0.5) < 4 / math.sqrt(12 * u.size) and abs((u < 0.25).mean() - 0.25) < 4 * math.sqrt(0.1875 / u.size)


@pytest.mark.parametrize('act_dtype', [np.float32, np.float64])
@pytest.mark.parametrize('supplied', [True, False])
def test_override_writes_the_clipped_draw_once_cast_and_nothing_else(act_dtype, supplied):
    n, seed, counter = 130, 11, 4
    rng = np.random.default_rng(8)
    tw = S.Twin(n)
    tw.state[9] = (rng.integers(0, 4, n).astype(np.uint64) << np.uint64(40)) | np.uint64(3 << 32) | np.uint64(17)
    keep = tw.state.copy()
    alive, stuck = (keep[9] >> np.uint64(40)) & np.uint64(1), ((keep[9] >> np.uint64(41)) & np.uint64(1)).astype(bool)
    raw = rng.integers(0, 256, (n, 2 * np.dtype(act_dtype).itemsize), dtype=np.uint8)       # any bytes: NaNs with payloads included
    a = raw.copy().view(act_dtype).reshape(n, 2)
    u = rng.random((n, 2))
    u[:5] = [[0.0, 0.0], [1 - 2.0 ** -53, 1 - 2.0 ** -53], [0.5, 0.5], [0.3, 0.7], [0.8, 0.1]]
    active = tw.override(a, u if supplied else None, seed, counter)
    uu = u if supplied else E.stuck_uniforms(seed, counter, n)
    b = S.box()
    want = (np.array([b[0], b[2]]) + np.array([b[1] - b[0], b[3] - b[2]]) * uu).clip(-1, 1).astype(act_dtype)
    assert np.array_equal(active, alive.astype(np.uint8)) and np.array_equal(tw.state, keep)
    assert stuck.any() and not stuck.all()
    assert np.array_equal(a[stuck].view(np.uint8), want[stuck].view(np.uint8))
    assert np.array_equal(a.view(np.uint8).reshape(n, -1)[~stuck], raw[~stuck])              # byte for byte
    assert (np.abs(want[:, 1]) == 1).mean() > 0.4                                           # U(-2.5, 2.5) clips 60 % of the speeds


def test_twins_reject_bad_arguments_and_touch_nothing():
    from hope_amd import _lib as L
    lib = L.load_library()
    n = 4
    st = np.zeros((L.EVAL_STATE_WORDS, n), np.uint64)
    t, p, r = np.zeros((n, 5), np.float32), np.zeros((n, 3)), np.zeros(n, np.float32)
    s, d, w, wo, do = np.zeros(n, np.int32), np.zeros(n, np.uint8), np.zeros((n, 8), np.int8), np.zeros((n, 8), np.int8), np.zeros(n, np.uint8)
    a, act = np.zeros((n, 2), np.float32), np.zeros(n, np.uint8)
    b = S.box()
    P = S.ptr
    assert lib.hope_eval_begin_host(0, n, P(st), P(t), 0, P(p)) == -1 and lib.hope_eval_begin_host(n, n - 1, P(st), P(t), 0, P(p)) == -1
    assert lib.hope_eval_begin_host(n, n, None, P(t), 0, P(p)) == -1 and lib.hope_eval_begin_host(n, n, P(st), None, 0, P(p)) == -1
    assert lib.hope_eval_begin_host(n, n, P(st), P(t), 0, None) == -1
    assert lib.hope_eval_override_host(n, n, P(st), None, P(a), 0, None, 0, 0, 0, P(act)) == -1
    bad = b.copy()
    bad[1] = np.inf
    assert lib.hope_eval_override_host(n, n, P(st), P(bad), P(a), 0, None, 0, 0, 0, P(act)) == -1
    assert lib.hope_eval_override_host(n, n, P(st), P(b), None, 0, None, 0, 0, 0, P(act)) == -1
    assert lib.hope_eval_override_host(n, n, P(st), P(b), P(a), 0, None, 0, 0, 0, None) == -1
    args = [P(t), 0, P(p), P(r), P(s), P(d), P(w), P(wo), P(do)]
    for k in (0, 2, 3, 4, 5, 6, 7, 8):
        bad_args = list(args)
        bad_args[k] = None
        assert lib.hope_eval_track_host(n, n, P(st), *bad_args) == -1, k
    assert b'hope_eval_track_host' in lib.hope_last_error()
    assert not st.any() and not a.any()
    assert lib.hope_eval_begin_host(n, n, P(st), P(t), 0, P(p)) == 0 and lib.hope_eval_track_host(n, n, P(st), *args) == 0


# ---- the evaluator on the CPU stand-in env ----------------------------------------------------------------------------------------
N_EVAL, MAX_STEPS, EVAL_SEED = 130, 40, 5


def _run(scenes, agent, tracker, poll_every=8):
    """-> (records, env.step calls, stuck overrides of live scenes after the first step, the evaluator)"""
    from fake_env import OracleEnv
    env = OracleEnv(scenes)
    ev = E.BatchedEvaluator(env, agent, post_proc_action=True, seed=EVAL_SEED, tracker=tracker, poll_every=poll_every)
    calls, overrides = [0], [0]
    orig = env.step

    def spy(actions, **kw):
        calls[0] += 1
        return orig(actions, **kw)
    env.step = spy
    if tracker is None:
        ev._stuck_uniform = lambda step: torch.from_numpy(E.stuck_uniforms(EVAL_SEED, step, env.n))
    else:
        tr = ev.tracker
        orig_override = tr.override

        def count(action, u=None):
            if tr.counter > 0:
                _, _, alive, stuck = S.decode(tr.state())
                overrides[0] += int((alive & stuck).sum())
            return orig_override(action, u)
        tr.override = count
    rec = ev.run(max_steps=MAX_STEPS, gather=False).numpy().copy()
    return rec, calls[0], overrides[0], ev


@pytest.fixture(scope='module')
def oracle_runs():
    from test_evaluate import _scenes
    torch.manual_seed(0)
    scenes = _scenes(N_EVAL)
    agent = A.BatchedPPO(device='cpu', use_img=False)
    ref = _run(scenes, agent, None)
    got = _run(scenes, agent, 'device', 8)
    return scenes, agent, ref, got


def _same_records(got, ref):
    assert got.shape == ref.shape == (len(ref), 4) and got.dtype == ref.dtype == np.float32
    assert np.array_equal(got[:, :3].view(np.uint32), ref[:, :3].view(np.uint32))            # status, steps, reward: raw words
    # torch's norm and hm_hypot differ by a few float64 ulp per step over <= 40 steps, far below a float32 ulp: the rounding to
    # float32 can differ by one ulp = 2^-23; the bound allows a factor of two over that
    assert (np.abs(got[:, 3] - ref[:, 3]) <= 2.0 ** -22 * np.abs(ref[:, 3])).all()


def test_evaluator_with_the_tracker_matches_the_torch_bookkeeping(oracle_runs):
    _, _, (ref, ref_calls, _, _), (got, calls, overrides, ev) = oracle_runs
    print('stuck overrides after step 1:', overrides, ' finished:', int((got[:, 0] != 1).sum()), ' alive at the end:', int((got[:, 0] == 1).sum()),
          ' env.step calls:', calls, 'against', ref_calls)
    _same_records(got, ref)
    # the premise: the inputs reach the stuck override after an episode's first step, frozen slots and slots that never finish
    assert overrides >= 1
    assert ((got[:, 0] != 1) & (got[:, 1] < MAX_STEPS)).any()
    assert (got[:, 0] == 1).any() and (got[got[:, 0] == 1, 1] == MAX_STEPS).all()
    _, _, alive, _ = S.decode(ev.tracker.state())
    assert np.array_equal(alive == 1, got[:, 0] == 1)
    s = E.summarize(got)
    assert s['all']['episodes'] == N_EVAL and s == E.summarize(ref)


def _step_bound(rec, poll_every):
    frozen_at = int(rec[:, 1].max()) if (rec[:, 0] != 1).all() else MAX_STEPS               # the first step with every slot frozen
    return min(-(-frozen_at // poll_every) * poll_every, MAX_STEPS)


@pytest.mark.parametrize('subset', [False, True])
def test_poll_every_changes_the_step_calls_only(oracle_runs, subset):
    scenes, agent, _, (got8, calls8, _, _) = oracle_runs
    if subset:                                            # scenes that park early: the loop can end before max_steps
        order = np.argsort(np.where(got8[:, 0] != 1, got8[:, 1], np.inf))[:6]
        scenes = [scenes[i] for i in order]
        got8, calls8, _, _ = _run(scenes, agent, 'device', 8)
    assert calls8 <= _step_bound(got8, 8)
    for k in (1, 1000):
        rec, calls, _, _ = _run(scenes, agent, 'device', k)
        assert np.array_equal(rec.view(np.uint32), got8.view(np.uint32)), k
        print('poll_every', k, ': env.step calls', calls, 'bound', _step_bound(rec, k), 'all frozen:', bool((rec[:, 0] != 1).all()))
        assert calls <= _step_bound(rec, k), k
