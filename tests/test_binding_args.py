"""The binding's two argument checkers (hope_amd/_lib.py tensor_arg / array_arg): the library sees addresses only, so what they let
through is all that stands between a caller's tensor and a loop that runs over N elements of it.  CPU only: the checkers directly,
`python -O`, and every host-twin path of hope_amd/agent_glue.py on the stand-in env -- a refused call must have touched nothing."""
import ctypes
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
from hope_amd import _lib as L
from hope_amd import agent_glue as G

CPU = torch.device('cpu')


def _refused(match, fn, *args, **kw):
    with pytest.raises(L.HopeError, match=match) as e:
        fn(*args, **kw)
    return str(e.value)


def test_tensor_checker():
    arg = lambda x, dtype=torch.uint8, shape=(64,), **kw: L.tensor_arg('hope_env_step', 'active', x, dtype, shape, CPU, **kw)  # noqa: E731
    good = torch.zeros(64, dtype=torch.uint8)
    p = arg(good)
    assert isinstance(p, ctypes.c_void_p) and p.value == good.data_ptr()
    assert arg(good.bool(), (torch.uint8, torch.bool)).value is not None
    msg = _refused('active', arg, torch.zeros(64), (torch.uint8, torch.bool))                          # wrong dtype
    assert msg == 'hope_env_step: active must be uint8 or bool [64] contiguous on cpu, got float32 [64] on cpu'
    _refused(r'active must be uint8 \[64\].*got uint8 \[64, 1\]', arg, good.view(64, 1))                # wrong rank
    _refused(r'got uint8 \[\] on cpu', arg, torch.zeros((), dtype=torch.uint8))
    _refused(r'got uint8 \[63\]', arg, good[:63])                                                       # one element short
    _refused(r'got uint8 \[65\]', arg, torch.zeros(65, dtype=torch.uint8))                              # one element long
    _refused(r'got uint8 \[64\] strided', arg, torch.zeros(128, dtype=torch.uint8)[::2])                # a strided view
    _refused(r'\[4, 2\].*got float32 \[4, 2\] strided', arg, torch.zeros((2, 4)).t(), torch.float32, (4, 2))    # a transpose
    _refused(r'contiguous on cpu, got uint8 \[64\] on meta', arg, torch.zeros(64, dtype=torch.uint8, device='meta'))  # wrong device
    _refused('got None$', arg, None)                                                                    # None where it is not allowed
    assert arg(None, optional=True) is None                                                             # ... and where it is
    _refused('got ndarray', arg, np.zeros(64, np.uint8))                                                # no tensor at all
    _refused('got list', arg, [0] * 64)
    # a free extent (None) takes any size in that place only
    rows = lambda x: L.tensor_arg('hope_env_obsnorm', 'lidar', x, (torch.float32, torch.float64), (None, 120), CPU)  # noqa: E731
    assert rows(torch.zeros((3, 120))).value and rows(torch.zeros((7, 120), dtype=torch.float64)).value
    _refused(r'lidar must be float32 or float64 \[\?, 120\].*got float32 \[3, 119\]', rows, torch.zeros((3, 119)))
    _refused(r'got float32 \[360\]', rows, torch.zeros(360))


def test_array_checker():
    arg = lambda x, dtype=np.float64, shape=(8, 3), **kw: L.array_arg('hope_env_set_pool', 'start', x, dtype, shape, **kw)  # noqa: E731
    good = np.arange(24.0).reshape(8, 3)
    assert arg(good) is good                                                                            # nothing to convert: the array itself
    for x in (good.astype(np.float32), good.tolist(), np.asfortranarray(good), np.arange(48.0).reshape(8, 6)[:, ::2] / 2):
        a = arg(x)                                                                                      # converted as np.ascontiguousarray does
        assert a.dtype == np.float64 and a.flags.c_contiguous and a.shape == (8, 3) and np.array_equal(a, good)
    msg = _refused('start', arg, good[:7])                                                              # one row short
    assert msg == 'hope_env_set_pool: start must be float64 [8, 3], got float64 [7, 3]'
    _refused(r'got float64 \[9, 3\]', arg, np.zeros((9, 3)))                                            # one row long
    _refused(r'got float64 \[24\]', arg, good.reshape(-1))                                              # wrong rank
    _refused(r'got float64 \[8, 3, 1\]', arg, good[:, :, None])
    _refused('got str', arg, 'eight by three')                                                          # a dtype that does not convert
    _refused('got None$', arg, None)
    assert arg(None, optional=True) is None
    free = arg(np.zeros((5, 16, 4, 2)), shape=(5, None, 4, 2))
    assert free.shape == (5, 16, 4, 2)
    _refused(r'\[5, \?, 4, 2\], got float64 \[5, 16, 4, 3\]', arg, np.zeros((5, 16, 4, 3)), shape=(5, None, 4, 2))
    # what a call takes is the array's ctypes view: it carries the address and keeps the array alive
    f = L.load_library().hope_scenegen_log_det
    x, y = arg([1.0, 2.0, 4.0], shape=(3,)), np.zeros(3)
    assert f(3, x.ctypes, y.ctypes) == 0 and np.allclose(y, np.log([1.0, 2.0, 4.0]), rtol=1e-15)


def test_seed_helper():
    assert L.seed64(-1).value == 2 ** 64 - 1 and L.seed64(2 ** 64 + 5).value == 5 and isinstance(L.seed64(np.int64(7)), ctypes.c_uint64)


def test_checks_survive_python_O():
    """the checks are raise statements: an optimised interpreter still refuses a short tensor"""
    code = ("import torch\nfrom hope_amd import _lib as L\nassert False, 'asserts are off'\n"
            "try:\n    L.tensor_arg('hope_env_step', 'active', torch.zeros(63, dtype=torch.uint8), torch.uint8, (64,), torch.device('cpu'))\n"
            "except L.HopeError as e:\n    print('refused:', e)\n")
    r = subprocess.run([sys.executable, '-O', '-c', code], capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith('refused: hope_env_step: active must be uint8 [64]') and 'got uint8 [63]' in r.stdout, (r.stdout, r.stderr)


# ---- the host twins of agent_glue.py on the stand-in env ---------------------------------------------------------------------------
N = 4


@pytest.fixture(scope='module')
def env():
    from fake_env import OracleEnv
    from hope_amd.scenes import SceneSource
    src = SceneSource(levels=('Normal', 'Complex', 'Extrem'), seed=3)
    e = OracleEnv([src.draw() for _ in range(N)]).reset_obs()
    e.step(torch.zeros((N, 2)))
    return e


def test_planner_host_twin_refuses_before_the_call(env):
    p = G.DeviceRsPlanner(env)
    word = torch.tensor([[1, 0, 2, -1, -1, 3, 1, 0]] * N, dtype=torch.int8)
    lens = torch.tensor([[2.0, 3.0, -1.5, 0.0, 0.0]] * N)
    planned, executing = p.step(done=torch.zeros(N, dtype=torch.uint8), rs_word=word, rs_lengths=lens)
    assert bool(executing.all()) and p._state.any()
    before = (p._state.copy(), planned.clone(), executing.clone())
    zero = torch.zeros(N, dtype=torch.uint8)
    _refused('hope_planner_step_host: rs_word must be int8', p.step, done=zero, rs_word=word[:N - 1], rs_lengths=lens)
    _refused('rs_word must be int8', p.step, done=zero, rs_word=word.to(torch.int32), rs_lengths=lens)
    _refused('rs_lengths must be float32 or float64', p.step, done=zero, rs_word=word, rs_lengths=lens.to(torch.float16))
    _refused('rs_lengths must be', p.set_paths, word, lens[:, :4])
    _refused(r'done must be uint8 \[4\]', p.step, done=zero[:N - 1], rs_word=word, rs_lengths=lens)
    assert np.array_equal(p._state, before[0]) and torch.equal(p._planned, before[1]) and torch.equal(p._exec.bool(), before[2])


def test_chooser_host_twin_refuses_before_the_call(env):
    c = G.DeviceActionChooser(env, seed=1)
    mean, log_std, mask = torch.zeros((N, 2)), torch.full((1, 2), -1.0), torch.ones((N, 42))
    c.choose(mean, log_std, mask)
    before = [t.clone() for t in (c._a, c._a32, c._idx, c._lp)] + [c.counter]
    planned, executing, u = torch.zeros((N, 2), dtype=torch.float64), torch.zeros(N, dtype=torch.uint8), torch.full((N,), 0.5, dtype=torch.float64)
    _refused('hope_chooser_host: mean must be float32 or float64', c.choose, mean[:N - 1], log_std, mask)
    _refused('mean must be', c.choose, mean.to(torch.float16), log_std, mask)
    _refused('log_std must be float32', c.choose, mean, torch.zeros((2, 2)), mask)
    _refused(r'mask must be float32 or float64 \[4, 42\]', c.choose, mean, log_std, mask[:, :41])
    _refused('planned must be float64', c.choose, mean, log_std, mask, planned[:N - 1], executing)
    _refused('executing must be uint8', c.choose, mean, log_std, mask, planned, executing[:N - 1])
    _refused('planned and executing go together', c.choose, mean, log_std, mask, planned, None)
    _refused(r'u must be float64 \[4\]', c.choose, mean, log_std, mask, u=u[:N - 1])
    assert all(torch.equal(a, b) for a, b in zip((c._a, c._a32, c._idx, c._lp), before)) and c.counter == before[4]
    c.choose(mean, log_std, mask, planned, executing, u)                                                # the full-size arguments pass


def test_obsnorm_host_twin_refuses_before_the_call(env):
    dn = G.DeviceStateNorm(env)
    obs = {'lidar': env.lidar, 'target': env.target}
    out = dn.update_and_normalize(obs)
    before = (bytes(dn._state), out['lidar'].clone(), out['target'].clone())
    _refused(r'hope_obsnorm_host: target must be float32 \[4, 5\]', dn.update_and_normalize, {'lidar': env.lidar, 'target': env.target[:N - 1]})
    _refused(r'lidar must be float32 or float64 \[\?, 120\]', dn.update, {'lidar': env.lidar[:, :119], 'target': env.target})
    _refused('target must be', dn.normalize, {'lidar': env.lidar, 'target': env.target[:, :4]})
    bad = G.BatchedStateNorm(shapes={'lidar': 119, 'target': 5})
    _refused(r'mean must be float64 \[125\]', dn.load, bad)
    assert bytes(dn._state) == before[0] and torch.equal(dn._out[0][:N], before[1]) and torch.equal(dn._out[1][:N], before[2])


def test_gae_host_twin_refuses_before_the_call(env):
    g = G.DeviceGae(env)
    t = 5
    gen = torch.Generator().manual_seed(2)
    reward, value, value_target = (torch.randn((N, t), generator=gen) for _ in range(3))
    done, v_last = torch.zeros((N, t)), torch.randn(N, generator=gen)
    adv, v_target = g(reward, done, value, v_last, value_target, 0.98, 0.95)
    sums, before = g.sums, (adv.clone(), v_target.clone(), g.sums.clone())
    _refused(r'hope_gae_host: v_last must be float32 \[4\]', g, reward, done, value, v_last[:N - 1], value_target, 0.98, 0.95)
    _refused(r'done must be float32 \[4, 5\]', g, reward, done[:, :t - 1], value, v_last, value_target, 0.98, 0.95)
    _refused('value must be', g, reward, done, value[:N - 1], v_last, value_target, 0.98, 0.95)
    _refused('value_target must be', g, reward, done, value, v_last, value_target.reshape(-1), 0.98, 0.95)
    _refused(r'reward must be float32 \[\?, \?\]', g, reward.reshape(-1), done, value, v_last, value_target, 0.98, 0.95)
    _refused(r'sums must be float64 \[3\]', g.mean_std, torch.zeros(2, dtype=torch.float64))
    assert g.sums is sums and torch.equal(g.sums, before[2]) and torch.equal(adv, before[0]) and torch.equal(v_target, before[1])


def test_eval_tracker_host_twin_refuses_before_the_call(env, monkeypatch):
    tr = G.DeviceEvalTracker(env, seed=2)
    tr.begin()
    act = torch.zeros((N, 2))
    tr.override(act)
    tr.track()
    tr.override(act)
    before = (tr._state.copy(), tr.alive.clone(), tr.word.clone(), tr.done.clone(), tr.counter, act.clone())
    assert before[0].any() and before[4] == 2
    _refused(r'hope_eval_override_host: action must be float32 or float64 \[4, 2\]', tr.override, act[:N - 1])
    _refused('action must be', tr.override, act.to(torch.float16))
    _refused(r'u must be float64 \[4, 2\]', tr.override, act, torch.full((N - 1, 2), 0.5))
    for name, bad in (('rs_word', env.rs_word.to(torch.int16)), ('rs_word', env.rs_word[:N - 1]), ('pose', env.pose[:N - 1]),
                      ('target', env.target[:, :4]), ('reward', env.reward[:N - 1]), ('status', env.status[:N - 1]), ('done', env.done[:N - 1])):
        with monkeypatch.context() as m:
            m.setattr(env, name, bad)
            _refused(f'hope_eval_track_host: {name} must be', tr.track)
    for name, bad in (('pose', env.pose[:N - 1]), ('target', env.target[:N - 1])):
        with monkeypatch.context() as m:
            m.setattr(env, name, bad)
            _refused(f'hope_eval_begin_host: {name} must be', tr.begin)
    after = (tr._state, tr.alive, tr.word, tr.done, tr.counter, act)
    assert np.array_equal(after[0], before[0]) and all(torch.equal(a, b) for a, b in zip(after[1:4], before[1:4]))
    assert after[4] == before[4] and torch.equal(act, before[5])


def test_host_twins_want_cpu_tensors(env):
    class Elsewhere:
        n, device = N, 'meta'
    for cls in (G.DeviceRsPlanner, G.DeviceActionChooser, G.DeviceStateNorm, G.DeviceGae, G.DeviceEvalTracker):
        _refused('must hold CPU tensors', cls, Elsewhere())
