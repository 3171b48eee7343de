"""The rule of SAC's update (hope_amd/csrc/hope_sac_core.h) through its host twins hope_sac_*_host, on the CPU: the twins against torch's
float64 autograd of BatchedSAC.update's own expressions, the branches and programmed cases, the sums' order against a restatement,
BatchedSAC.update with a DeviceSacUpdate over CPU tensors (the reference's recorded update, the parameter gradients, the trainer loop),
the torch path unchanged, and misuse."""
import copy
import ctypes as C
import os
import shutil
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sac_update_script as S  # noqa: E402

CPU_ENV = types.SimpleNamespace(n=1, device=torch.device('cpu'))


@pytest.fixture(scope='module')
def case():
    """per size: the inputs, the twins' outputs and the float64 reference, computed once"""
    out = {}
    for b in S.SIZES:
        x = S.inputs(b)
        out[b] = (x, S.host_all(x), S.torch_reference(x))
    return out


@pytest.mark.parametrize('b', S.SIZES)
def test_twins_against_float64_autograd(case, b):
    """action, lp, q_target, g_q1, g_q2, s1, s2 and g_raw per item within one float32 ulp of the float64 reference; the four losses and
    g_log_std within one ulp plus 2^-40 sum |terms| (float64 arithmetic rounded once: the reference's own sums run in another order),
    g_log_alpha (a float64 word) within one float64 ulp plus that slack.  From 63 items on the inputs hold every branch of the rule,
    which is asserted."""
    x, h, ref = case[b]
    if b >= 63:
        cs = S.census(x)
        assert min(cs.values()) > 0, cs
    per = {'action': h['sample'][0], 'lp': h['sample'][1], 'q_target': h['critic'][0], 'g_q1': h['critic'][1], 'g_q2': h['critic'][2], 's1': h['seed'][0],
           's2': h['seed'][1], 'g_raw': h['policy'][0]}
    for what, got in per.items():
        want = ref[what]
        err = np.abs(got.astype(np.float64) - want)
        print(b, what, 'largest error in ulp:', float((err / S.ulp32(want)).max()))
        assert got.shape == want.shape and (err <= S.ulp32(want)).all(), (what, float((err / S.ulp32(want)).max()))
    for got, what in ((h['critic'][3], 'critic_losses'), (h['policy'][3], 'policy_losses'), (h['policy'][1], 'g_log_std')):
        want = ref[what]
        err, bound = np.abs(got.astype(np.float64) - want), S.ulp32(want) + 2.0 ** -40 * ref['abs_sums'][what]
        print(b, what, 'error / bound:', (err / np.maximum(bound, 1e-300)).tolist())
        assert (err <= bound).all(), (what, err, bound)
    got, want = float(h['policy'][2]), ref['g_log_alpha']
    err, bound = abs(got - want), float(np.spacing(abs(want))) + 2.0 ** -40 * ref['abs_sums']['g_log_alpha']
    print(b, 'g_log_alpha error / bound:', err / bound)
    assert err <= bound, (got, want)
    assert h['policy'][3][1] == np.float32(got)                                 # the temperature loss: its gradient's value, rounded


def test_programmed_cases():
    """exact ties give 1/2 and 1/2 of the seed; a raw beyond the clamp gives a zero g_raw word and one on the bound does not; a z exactly
    on the bound passes the gradient g_action through, one beyond it does not"""
    b = 8
    x = S.inputs(b)
    x['p1'][:] = [0.5, 0.5, -1.0, 2.0, 0.0, -0.0, 3.0, 3.0]
    x['p2'][:] = [0.5, 0.7, -1.0, 1.0, -0.0, 0.0, 3.0, 2.5]
    s1, s2 = S.host_seed(x)
    w1 = np.array([0.5, 1.0, 0.5, 0.0, 0.5, 0.5, 0.5, 0.0])
    assert np.array_equal(s1, (-w1 / b).astype(np.float32)) and np.array_equal(s2, (-(1 - w1) / b).astype(np.float32))
    #            raw_0: beyond  bound  bound  inside  beyond   inside inside inside
    x['raw'][:, 0] = [1.5, 1.0, -1.0, 0.25, -1.25, 0.0, 0.5, -0.5]
    x['raw'][:, 1] = 0.0
    x['eps'][:] = 0.0                                                           # z = mean: on the bound for items 0 .. 2 and 4
    x['eps'][5, 0], x['eps'][6, 0] = 4.0, -4.0                                  # z beyond +1 / -1 from a mean inside
    x['g_action'][:] = 0.125
    g_raw = S.host_policy(x)[0]
    without = S.host_policy(dict(x, g_action=np.zeros((b, 2), np.float32)))[0]
    # with eps = 0 the sample is the mean: e = 0 and t = 0, so g_raw is g_action where both clamps pass and 0 where the mean's does not
    assert g_raw[[0, 1, 2, 3, 4, 7], 0].tolist() == [0.0, 0.125, 0.125, 0.125, 0.0, 0.125]
    assert g_raw[:, 1].tolist() == [0.125] * 8 and not without[[0, 1, 2, 3, 4, 7]].any()
    # a z beyond the bound stops g_action; what is left is the log-probability's own dependence on the mean
    assert np.array_equal(S.words(g_raw[5:7, 0]), S.words(without[5:7, 0])) and g_raw[5, 0] > 0 > g_raw[6, 0]
    a, _ = S.host_sample(x)
    assert a[:, 0].tolist() == [1.0, 1.0, -1.0, 0.25, -1.0, 1.0, -1.0, -0.5]
    ref = S.torch_reference(x)
    assert np.array_equal(ref['g_raw'][:, 0] != 0, g_raw[:, 0] != 0) and np.abs(g_raw - ref['g_raw']).max() <= 2.0 ** -24


def test_the_sums_have_the_rules_order(case):
    """4097 items (65 chunk partials, an odd one among them) against the script's own restatement: the per-item terms in Python
    floats, the chunk tree, the merge tree -- equal word for word, g_log_alpha as a float64 word"""
    x, h, _ = case[4097]
    critic_losses, policy_losses, g_log_std, g_log_alpha = S.restated_sums(x)
    for got, want, what in ((h['critic'][3], critic_losses, 'critic losses'), (h['policy'][3], policy_losses, 'policy losses'),
                            (h['policy'][1], g_log_std, 'g_log_std'), (h['policy'][2], g_log_alpha, 'g_log_alpha')):
        assert got.dtype == want.dtype and np.array_equal(S.words(got), S.words(want)), (what, got, want)


# ---- BatchedSAC.update with the block ----------------------------------------------------------------------------------------------
def _block():
    from hope_amd import agent_glue as G
    blk = G.make_sac_update('device', CPU_ENV)
    assert isinstance(blk, G.DeviceSacUpdate) and not blk.on_device
    return blk


def test_update_with_the_block_matches_the_reference_recording():
    """test_agents.check_sac_update's scenario -- the reference's SACAgent.update, its recorded noise, losses and post-update probes in
    tests/golden/sac_update.npz -- with update_block=DeviceSacUpdate on CPU tensors, at that test's own tolerances"""
    import test_agents as TA
    from hope_amd import agents as A
    from hope_amd import agent_glue as G
    tol = 5e-4
    g = TA._load('sac_update.npz')
    ag = A.BatchedSAC(device='cpu', use_img=True, lr=2e-4, batch_size=16, state_norm=False, update_block=_block())
    TA.det_fill(ag.actor, 0.1)
    TA.det_fill(ag.critic1, 0.3)
    TA.det_fill(ag.critic2, 0.4)
    ag.critic_target1.load_state_dict(ag.critic1.state_dict())
    ag.critic_target2.load_state_dict(ag.critic2.state_dict())
    with torch.no_grad():
        ag.log_std.copy_(torch.tensor([[-0.5, -0.1]]))
    f = lambda k: torch.from_numpy(g[k])  # noqa: E731
    batch = {'obs': TA._obs(g, 'x_', 'cpu'), 'next_obs': TA._obs(g, 'nx_', 'cpu'), 'action': f('action'), 'reward': f('reward'), 'done': f('done')}
    eps = f('eps')
    for u in range(3):
        a, b = ag.update(batch, noise=(eps[2 * u], eps[2 * u + 1]))
        assert abs(a - g['losses'][u, 0]) < tol * max(1, abs(g['losses'][u, 0])), (u, a, g['losses'][u])
        assert abs(b - g['losses'][u, 1]) < tol * max(1, abs(g['losses'][u, 1])), (u, b, g['losses'][u])
    for name, net in (('probe_actor', ag.actor), ('probe_q1', ag.critic1), ('probe_q2', ag.critic2), ('probe_t1', ag.critic_target1),
                      ('probe_t2', ag.critic_target2)):
        got, exp = TA.probe(net.cpu()).numpy(), g[name]
        assert (np.abs(got - exp) / np.maximum(np.abs(exp[:, 1:2]), 1.0)).max() < tol, name
    assert abs(float(ag.log_alpha.detach()) - float(g['log_alpha'])) < 1e-5
    assert np.allclose(ag.log_std.detach().cpu().numpy(), g['log_std'], atol=tol)
    with pytest.raises(ValueError):
        G.make_sac_update('gpu', CPU_ENV)
    assert G.make_sac_update(None, CPU_ENV) is None


def _ring_batch(n=6, t=4, batch=10, seed=0):
    """a full CPU TransitionRing of n scenes x t columns with drawn contents and a batch drawn from it"""
    from hope_amd.rollout import TransitionRing
    torch.manual_seed(seed)
    ring = TransitionRing(n, t, ('lidar', 'target', 'action_mask'), 'cpu')
    for v in ring.obs.values():
        v.copy_(torch.randn(v.shape))
    ring.obs['action_mask'].copy_((torch.rand(n, t, 42) > 0.3).float())
    ring.action.copy_(torch.randn(n, t, 2).clamp(-1, 1))
    ring.reward.copy_(torch.randn(n, t))
    ring.done.copy_((torch.rand(n, t) < 0.25).to(ring.done.dtype))
    ring.head, ring.size = 0, t
    last = {k: torch.randn(v[:, 0].shape) for k, v in ring.obs.items()}
    return ring.sample(batch, last, torch.Generator().manual_seed(seed + 1))


def _agent(lr, batch_size=10, seed=0):
    from hope_amd import agents as A
    torch.manual_seed(seed)
    ag = A.BatchedSAC(device='cpu', use_img=False, lr=lr, batch_size=batch_size, state_norm=False)
    with torch.no_grad():
        ag.log_std.copy_(torch.tensor([[-0.2, 0.1]]))
    return ag


def _double(ag):
    for net in (ag.actor, ag.critic1, ag.critic2, ag.critic_target1, ag.critic_target2):
        net.double()
    ag.log_std.data = ag.log_std.data.double()
    return ag


def _named(ag):
    return [('actor.' + k, p) for k, p in ag.actor.named_parameters()] + [('log_std', ag.log_std)] + \
        [('critic1.' + k, p) for k, p in ag.critic1.named_parameters()] + [('critic2.' + k, p) for k, p in ag.critic2.named_parameters()] + \
        [('log_alpha', ag.log_alpha)]


def test_parameter_gradients_through_a_whole_update():
    """6 scenes x 4 columns, a batch of 10, learning rate 0: after one update the gradients of the actor, log_std, critic 1, critic 2
    and log_alpha with the block are at most 2 x as far from the float64 torch path as the float32 torch path is (both push float32
    seeds through the same float32 backward and differ in the seeds' last bits only).  The noise is given, so all three paths see the
    same.  The distance of a group is the largest absolute difference over all its elements: the five groups are the ones the bar
    names, and a group must hold enough elements for the ratio to mean anything -- a critic's output bias is ONE float32 number, the
    sum of ten seeds, and the ratio of two single rounding errors has no bound (measured per tensor over four seeds: median 1.0,
    largest 5.4 at such a bias where the float32 path happened to land 0.3 ulp from the float64 value and the block 1.7 ulp).  The
    per-tensor figures are printed."""
    batch = _ring_batch()
    noise = tuple(torch.randn(10, 2, generator=torch.Generator().manual_seed(s)) for s in (5, 6))
    ag = _agent(0.0)
    ag32, ag64 = copy.deepcopy(ag), _double(copy.deepcopy(ag))
    ag.update_block = _block()
    got = ag.update(batch, noise=noise)
    l32 = ag32.update(batch, noise=noise)
    b64 = {'obs': {k: v.double() for k, v in batch['obs'].items()}, 'next_obs': {k: v.double() for k, v in batch['next_obs'].items()},
           'action': batch['action'].double(), 'reward': batch['reward'].double(), 'done': batch['done'].double()}
    l64 = ag64.update(b64, noise=tuple(e.double() for e in noise))
    assert max(abs(a - b) for a, b in zip(got, l64)) <= 1e-5 * max(1.0, *map(abs, l64)) and max(abs(a - b) for a, b in zip(l32, l64)) <= 1e-5 * max(1.0, *map(abs, l64))
    groups, per_tensor, compared = {}, [], 0
    for (name, p), (_, p32), (_, p64) in zip(_named(ag), _named(ag32), _named(ag64)):
        if p64.grad is None:                                                    # a parameter the forward without the image does not use
            assert p.grad is None and p32.grad is None, name
            continue
        assert p.grad is not None and p.grad.shape == p64.grad.shape and p.grad.dtype == p32.grad.dtype, name
        compared += 1
        yard = float((p32.grad.double() - p64.grad).abs().max())
        dist = float((p.grad.double() - p64.grad).abs().max())
        per_tensor.append((dist / yard if yard > 0 else (0.0 if dist == 0 else float('inf')), name, p.numel()))
        g = groups.setdefault(name.split('.')[0], [0.0, 0.0])
        g[0], g[1] = max(g[0], dist), max(g[1], yard)
    assert compared > 40 and float(ag64.log_alpha.grad.abs()) > 0 and set(groups) == {'actor', 'log_std', 'critic1', 'critic2', 'log_alpha'}
    print('distance / yardstick per group:', {k: (d / y if y > 0 else 0.0) for k, (d, y) in groups.items()})
    print('per tensor: median', float(np.median([r[0] for r in per_tensor])), 'largest (ratio, tensor, elements)', sorted(per_tensor, reverse=True)[:3])
    for name, (dist, yard) in groups.items():
        assert dist <= 2.0 * yard, (name, dist, yard)
    for p in list(ag.critic1.parameters()) + list(ag.critic2.parameters()):     # nothing was switched off on the way
        assert p.requires_grad


def test_update_without_a_block_is_todays_path():
    """update_block=None: the losses and every parameter after two updates with a real learning rate equal, bit for bit, those of the
    update as it was before the switch (restated in the script), from the same seed -- drawn noise and given noise"""
    batch = _ring_batch(seed=2)
    ag = _agent(1e-3, seed=3)
    assert ag.update_block is None
    twin = copy.deepcopy(ag)
    nets = lambda a: (a.actor, a.critic1, a.critic2, a.critic_target1, a.critic_target2)  # noqa: E731
    noise = tuple(torch.randn(10, 2, generator=torch.Generator().manual_seed(s)) for s in (7, 8))
    torch.manual_seed(11)
    got = [ag.update(batch), ag.update(batch, noise=noise)]
    torch.manual_seed(11)
    want = [S.parent_update(twin, batch), S.parent_update(twin, batch, noise=noise)]
    assert got == want
    for a, b in zip(nets(ag), nets(twin)):
        for p, q in zip(a.parameters(), b.parameters()):
            assert torch.equal(p, q) and p.requires_grad == q.requires_grad
    assert torch.equal(ag.log_std, twin.log_std) and torch.equal(ag.log_alpha, twin.log_alpha)


def _small_scenes(n, seed=3):
    from hope_amd.scenes import SceneSource
    src = SceneSource(levels=('Normal', 'Complex', 'Extrem'), seed=seed)
    return [src.draw() for _ in range(n)]


def test_trainer_loop_with_the_block():
    """SACTrainer(sac_update='device') on the CPU stand-in env for horizon + 2 update_every steps under the same torch.manual_seed as a
    sac_update=None trainer: the same forwards in the same order and the same draws, so both see the same noise and the same batches.
    The losses of every update agree within 5e-4 max(1, |loss|), the tolerance the recorded reference update is held to above.
    The rings' contents are identical at learning rate 0.  What the ring holds depends on the update through the weights alone, and the
    block's gradients differ from the torch path's in their last bits (float64 against float32 arithmetic), which an optimiser step
    carries into the weights, the next actions and the cars' poses: with a real learning rate the later columns agree to about 1e-4
    and no further, so identity is asserted where the weights stand still -- there it shows that the block consumes the generator
    exactly as the torch path does and touches nothing else of the rollout -- and the run at 1e-4 checks the losses."""
    from fake_env import OracleEnv
    from hope_amd import agent_glue as G
    from hope_amd import agents as A
    from hope_amd.rollout import SACTrainer
    horizon, every = 4, 2
    scenes = _small_scenes(8)
    for lr in (0.0, 1e-4):
        runs = []
        for kind in (None, 'device'):
            torch.manual_seed(0)
            ag = A.BatchedSAC(device='cpu', use_img=False, lr=lr, batch_size=16)
            tr = SACTrainer(OracleEnv(scenes), ag, horizon=horizon, update_every=every, seed=1, sac_update=kind)
            assert (ag.update_block is None) == (kind is None) and (kind is None or isinstance(tr.sac_update, G.DeviceSacUpdate))
            out = [tr.step() for _ in range(horizon + 2 * every)]
            assert tr.updates == 3 and [o is not None for o in out] == [False, False, False, True, False, True, False, True]
            runs.append(([o for o in out if o is not None], tr.ring))
        (l0, r0), (l1, r1) = runs
        for u, (a, b) in enumerate(zip(l0, l1)):
            print('lr', lr, 'update', u, 'losses', a, b)
            for v, w in zip(a, b):
                assert np.isfinite(w) and abs(v - w) <= 5e-4 * max(1.0, abs(v)), (lr, u, a, b)
        assert r0.head == r1.head and r0.size == r1.size == horizon
        if lr == 0.0:
            for k in r0.obs:
                assert torch.equal(r0.obs[k], r1.obs[k]), k
            for a, b, what in ((r0.action, r1.action, 'action'), (r0.reward, r1.reward, 'reward'), (r0.done, r1.done, 'done'),
                               (r0.log_prob, r1.log_prob, 'log_prob')):
                assert torch.equal(a, b), what
            assert float(r0.action.abs().max()) > 0
    with pytest.raises(ValueError):
        SACTrainer(OracleEnv(scenes[:2]), A.BatchedSAC(device='cpu', use_img=False, batch_size=4), horizon=2, sac_update='gpu')
    with pytest.raises(ValueError, match='update block'):
        SACTrainer(OracleEnv(scenes[:2]), A.BatchedPPO(device='cpu', use_img=False), horizon=2, sac_update='device')


def test_misuse_of_the_host_twins():
    """HOPE_EINVAL with the call's name for a NULL pointer, batch < 1 and a gamma or target_entropy that is NaN or infinite; the
    binding's checker refuses a wrong tensor before the call"""
    from hope_amd import _lib as L
    lib = L.load_library()
    x = S.inputs(5)
    P = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    calls = {
        'sample': (('raw', 'log_std', 'eps'), (), [np.zeros((5, 2), np.float32), np.zeros(5, np.float32)]),
        'critic': (('q1', 'q2', 'qt1', 'qt2', 'next_lp', 'reward', 'done', 'log_alpha'), (S.GAMMA,), [np.zeros(5, np.float32) for _ in range(3)] + [np.zeros(2, np.float32)]),
        'seed': (('p1', 'p2'), (), [np.zeros(5, np.float32), np.zeros(5, np.float32)]),
        'policy': (('raw', 'log_std', 'eps', 'p1', 'p2', 'g_action', 'log_alpha'), (S.TARGET_ENTROPY,),
                   [np.zeros((5, 2), np.float32), np.zeros(2, np.float32), np.zeros((), np.float64), np.zeros(2, np.float32)]),
    }
    for call, (ins, scalars, outs) in calls.items():
        name = f'hope_sac_{call}_host'
        fn = getattr(lib, name)

        def run(batch=5, scalar=scalars, null=None):
            ptrs = [P(x[k]) for k in ins] + [P(o) for o in outs]
            if null is not None:
                ptrs[null] = None
            return fn(*ptrs[:len(ins)], *scalar, batch, *ptrs[len(ins):])
        assert run() == 0, name
        bad = [{'batch': 0}, {'batch': -3}] + [{'null': i} for i in range(len(ins) + len(outs))]
        if scalars:
            bad += [{'scalar': (float('nan'),)}, {'scalar': (float('inf'),)}, {'scalar': (-float('inf'),)}]
        for kw in bad:
            assert run(**kw) == -1 and name.encode() in lib.hope_last_error(), (name, kw)
    blk = _block()
    q = torch.zeros(4, 1)
    with pytest.raises(L.HopeError, match=r'hope_sac_critic_host: log_alpha must be float64 \[\]'):
        blk.critic(q, q, q, q, q, q, q, torch.tensor(0.0), 0.99)
    with pytest.raises(L.HopeError, match=r'hope_sac_policy_host: log_alpha must be float64 \[\]'):
        blk.policy(torch.zeros(4, 2), torch.zeros(1, 2), torch.zeros(4, 2), q, q, torch.zeros(4, 2), torch.zeros(1, dtype=torch.float64), -2.0)
    with pytest.raises(RuntimeError):
        blk.seed(q, torch.zeros(3, 1))                                          # another extent than q1's


# ---- the sanitizer driver of the twins -----------------------------------------------------------------------------------------
def test_sanitizer_driver_of_the_twins_runs_clean(tmp_path):
    """tests/sac_update_host_sanitize.cpp, a stand-alone program, compiled by the host compiler with -fsanitize=address,undefined"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cxx = os.environ.get('CXX') or shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    assert cxx, 'no host C++ compiler'
    exe = str(tmp_path / 'sac_update_host_sanitize')
    cmd = [cxx, '-std=c++17', '-O1', '-g', '-ffp-contract=off', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
           '-I' + os.path.join(root, 'include'), '-I' + os.path.join(root, 'hope_amd', 'csrc'), os.path.join(root, 'tests', 'sac_update_host_sanitize.cpp'),
           '-o', exe]
    # the runtime linked into the program where the compiler can (gcc's switch; clang does so by default and may not know it)
    if subprocess.run(cmd + ['-static-libasan'], capture_output=True).returncode != 0:
        subprocess.check_call(cmd)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and 'clean' in r.stdout, (r.returncode, r.stdout, r.stderr)
