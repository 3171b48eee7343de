"""The optimiser block's rule on the host (hope_amd/csrc/hope_optim_core.h through hope_optim_adam_host / hope_optim_polyak_host): word
for word against the numpy restatement of tests/optim_cases.py, the refusals of the ABI, and the measured distance to torch's own Adam
and to agents._soft_update.  No device."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from hope_amd import _lib as L
from hope_amd import agents as A

import optim_cases as OC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = torch.device('cpu')


def twin_adam(params, grads, ms, vs, hypers, group_of=None):
    table, n, _keep = L.optim_entries(params, grads, ms, vs, group_of, 'hope_optim_adam_host')
    groups = (L.OptimGroup * len(hypers))(*(L.OptimGroup(*h) for h in hypers))
    L.check(L.load_library().hope_optim_adam_host(table, n, groups, len(hypers)), 'hope_optim_adam_host')


def twin_polyak(targets, currents, tau):
    table, n, _keep = L.optim_entries(targets, currents, call='hope_optim_polyak_host')
    L.check(L.load_library().hope_optim_polyak_host(table, n, float(tau)), 'hope_optim_polyak_host')


def _check_case(case, hp, offset=0):
    v, bufs = OC.torch_case(case, CPU, offset)
    twin_adam([v['p']], [v['g']], [v['m']], [v['v']], [hp])
    for k, w in zip('pmv', OC.adam_reference(case['p'], case['g'], case['m'], case['v'], hp)):
        assert np.array_equal(OC.words(v[k]), OC.words(w)), (k, int((OC.words(v[k]) != OC.words(w)).sum()))
    assert np.array_equal(OC.words(v['g']), OC.words(case['g']))
    assert all(OC.guards_intact(b, x) for b, x in bufs)
    return v


def test_binding_mirrors_the_header():
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'hope_env.h')).read(), flags=re.S)
    for cls, struct in ((L.OptimEntry, 'hope_optim_entry'), (L.OptimGroup, 'hope_optim_group')):
        body = re.search(r'typedef\s+struct\s+%s\s*\{(.*?)\}\s*%s_t\s*;' % (struct, struct), hdr, flags=re.S).group(1)
        fields = [re.search(r'(\w+)\s*$', d.strip()).group(1) for d in body.split(';') if d.strip()]
        assert fields == [f[0] for f in cls._fields_], (struct, fields)
    assert C.sizeof(L.OptimEntry) == 48 and C.sizeof(L.OptimGroup) == 48
    core = open(os.path.join(ROOT, 'hope_amd', 'csrc', 'hope_optim_kernel.h')).read()
    assert 'sizeof(OkTable) <= 3584' in core                        # the argument block: room under HIP's 4 KiB
    assert 216 + 48 * L.OPTIM_CAP <= 3584 and L.OPTIM_CAP >= 48       # one SacCritic with image (48 tensors) in one launch


@pytest.mark.parametrize('numel', OC.NUMELS)
def test_twin_equals_numpy_for_every_numel(numel):
    for seed, first in ((1, False), (2, True)):
        _check_case(OC.random_case(numel, 1000 * numel + seed, first_step=first), OC.hyper(t=1 if first else 7))
    _check_case(OC.special_case(numel, numel), OC.hyper(lr=1e-3, t=2))
    _check_case(OC.random_case(numel, numel, np.float64), OC.hyper(lr=2.5e-5, t=4))


@pytest.mark.parametrize('t', OC.STEPS)
def test_twin_equals_numpy_at_every_step_count(t):
    hp = OC.hyper(lr=2.5e-5, t=t)
    if t == 10 ** 6:
        assert hp[3] == 2.5e-5 and hp[4] == 1.0                      # both bias corrections are 1 to double precision
    _check_case(OC.random_case(1025, t), hp)


def test_twin_equals_numpy_on_zero_tiny_and_huge_gradients():
    for dtype in (np.float32, np.float64):
        c = OC.special_case(4 * len(OC.SPECIAL_GRADS), 5, dtype)
        v = _check_case(c, OC.hyper(t=3))
        assert np.isfinite(v['m'].numpy()).all()
    g = np.float32(1e-20)
    assert 0 < np.float32(np.float64(0.001) * g * g) < np.finfo(np.float32).tiny      # the subnormal case is one


@pytest.mark.parametrize('value', OC.NONFINITE)
@pytest.mark.parametrize('where', ['g', 'p', 'm', 'v'])
def test_one_nonfinite_element_leaves_its_neighbours_alone(value, where):
    hp = OC.hyper(t=3)
    for n in (5, 257, 1025):
        at = n // 2
        clean = _check_case(OC.random_case(n, 400 + n), hp)
        dirty = _check_case(OC.nonfinite_case(n, 400 + n, value, at, where), hp)
        keep = np.arange(n) != at
        for k in 'pmv':
            assert np.array_equal(OC.words(dirty[k])[keep], OC.words(clean[k])[keep]), (n, k)
        touched = {'g': 'pmv', 'p': 'p', 'm': 'pm', 'v': 'pv'}[where]
        for k in touched:
            assert not np.isfinite(dirty[k].numpy()[at]) or (k == 'p' and where == 'v' and value == np.inf), (n, k)


def test_the_whole_table_in_a_few_calls_aligned_and_not():
    assert OC.run_table(twin_adam, CPU, offsets=(0,)) <= 2
    OC.run_table(twin_adam, CPU, offsets=(1, 0, 3, 2))                # 4, 0, 12 and 8 bytes past a 16-byte boundary


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_entries_four_bytes_past_a_boundary_keep_their_sentinels(dtype):
    for n in OC.NUMELS:
        _check_case(OC.random_case(n, n, dtype), OC.hyper(t=2), offset=1)


@pytest.mark.parametrize('tau', OC.TAUS)
def test_polyak_twin_equals_numpy(tau):
    views, bufs, want = [], [], []
    for i, n in enumerate(OC.NUMELS + (1, 257)):
        dtype = np.float64 if i >= len(OC.NUMELS) else np.float32
        c = OC.random_case(n, 50 + i, dtype)
        if n == 5:
            c['g'][2], c['p'][3] = np.inf, np.nan
        v, b = OC.torch_case({'p': c['p'], 'g': c['g']}, CPU, offset=i % 2)
        views.append(v)
        bufs += b
        want.append((OC.polyak_reference(c['p'], c['g'], tau), c['g']))
    twin_polyak([v['p'] for v in views], [v['g'] for v in views], tau)
    for v, (t, cur) in zip(views, want):
        assert np.array_equal(OC.words(v['p']), OC.words(t)) and np.array_equal(OC.words(v['g']), OC.words(cur))
        if tau in (0.0, 1.0) and np.isfinite(t).all():                # the ends are exact copies
            assert np.array_equal(OC.words(v['p']), OC.words(t if tau == 0.0 else cur))
    assert all(OC.guards_intact(b, x) for b, x in bufs)


def test_two_groups_with_different_lr_and_eps_in_one_call():
    hs = [OC.hyper(lr=5e-6, eps=1e-8, t=3), OC.hyper(lr=1e-3, eps=1e-5, t=3)]
    cases = [OC.random_case(n, 70 + n) for n in (3, 1025, 257, 4)]
    group_of = [0, 1, 1, 0]
    views = [OC.torch_case(c, CPU)[0] for c in cases]
    twin_adam(*[[v[k] for v in views] for k in 'pgmv'], hs, group_of)
    for c, v, gi in zip(cases, views, group_of):
        for k, w in zip('pmv', OC.adam_reference(c['p'], c['g'], c['m'], c['v'], hs[gi])):
            assert np.array_equal(OC.words(v[k]), OC.words(w))
        other = OC.adam_reference(c['p'], c['g'], c['m'], c['v'], hs[1 - gi])[0]
        assert not np.array_equal(OC.words(v['p']), OC.words(other))  # the group index decided


@pytest.mark.parametrize('n_entries', [L.OPTIM_CAP, L.OPTIM_CAP + 1, 2 * L.OPTIM_CAP + 1])
def test_more_entries_than_one_launch_holds(n_entries):
    hp = OC.hyper(t=2)
    cases = [OC.random_case(1 + i % 7, 900 + i) for i in range(n_entries)]
    packed = [OC.torch_case(c, CPU, offset=i % 4) for i, c in enumerate(cases)]
    views = [p[0] for p in packed]
    twin_adam(*[[v[k] for v in views] for k in 'pgmv'], [hp])
    for c, v in zip(cases, views):
        for k, w in zip('pmv', OC.adam_reference(c['p'], c['g'], c['m'], c['v'], hp)):
            assert np.array_equal(OC.words(v[k]), OC.words(w))
    assert all(OC.guards_intact(b, x) for p in packed for b, x in p[1])


def test_every_refusal_names_its_entry_and_writes_nothing():
    lib = L.load_library()
    f32, b32 = OC.torch_case(OC.random_case(64, 1), CPU)
    f64, b64 = OC.torch_case(OC.random_case(4, 2, np.float64), CPU)
    before = [b.clone() for b, _ in b32 + b64]
    cases = OC.refusals(L, f32, f64)
    assert len(cases) >= 50
    for label, mode, table, n, groups, n_groups, tau, text in cases:
        if mode == 'adam':
            rc, name = lib.hope_optim_adam_host(table, n, groups, n_groups), 'hope_optim_adam_host'
        else:
            rc, name = lib.hope_optim_polyak_host(table, n, tau), 'hope_optim_polyak_host'
        msg = lib.hope_last_error().decode()
        assert rc == -1 and msg.startswith(name + ': ') and text in msg, (label, rc, msg)
        for (b, _), was in zip(b32 + b64, before):
            assert torch.equal(b, was), label


def test_optim_entries_refuses_tensors_that_do_not_go_together():
    p, g, m, v = (torch.zeros(4, 6) for _ in range(4))
    good = dict(params=[p], grads=[g], ms=[m], vs=[v])
    assert L.optim_entries(**good)[1] == 1
    for key, bad, text in (('grads', g.t().contiguous().t(), 'not contiguous'), ('ms', m.double(), 'torch.float64'), ('vs', torch.zeros(6, 4), '[6, 4]'),
                           ('params', p.to(torch.float16), 'float32 or float64'), ('grads', g.to_sparse(), 'dense'), ('grads', None, 'dense'),
                           ('ms', torch.zeros(4, 6, device='meta'), 'meta')):
        args = dict(good, **{key: [bad]})
        with pytest.raises(ValueError, match='entry 0') as e:
            L.optim_entries(**args)
        assert text in str(e.value), (key, str(e.value))
    with pytest.raises(ValueError, match='one length'):
        L.optim_entries([p, p], [g], [m], [v])
    with pytest.raises(ValueError, match='the call on cpu'):
        L.optim_entries([torch.zeros(3, device='meta')], [torch.zeros(3)], device='cpu')


# ---- the distance to torch -----------------------------------------------------------------------------------------------
def _errors_against_float64(lr, n=200_000, steps=20, seed=0):
    """20 steps on n elements, gradients randn * 10^k with k per element from -8 .. 1: the errors of the twin and of torch's float32
    Adam (foreach False / True) against torch.optim.Adam on float64 copies fed the same float32 gradients
    -> {path: (displacement error, exp_avg error, exp_avg_sq error)}"""
    r = np.random.default_rng(seed)
    p0 = torch.from_numpy((r.standard_normal(n) * 0.1).astype(np.float32))
    grads = [torch.from_numpy((r.standard_normal(n) * 10.0 ** r.integers(-8, 2, n)).astype(np.float32)) for _ in range(steps)]

    def run_torch(dtype, foreach):
        p = p0.to(dtype).clone().requires_grad_()
        opt = torch.optim.Adam([p], lr, foreach=foreach)
        for g in grads:
            p.grad = g.to(dtype)
            opt.step()
        st = opt.state[p]
        return p.detach().double() - p0.double(), st['exp_avg'].double(), st['exp_avg_sq'].double()
    ref = run_torch(torch.float64, False)
    out = {'foreach=False': run_torch(torch.float32, False), 'foreach=True': run_torch(torch.float32, True)}
    p, m, v = p0.clone(), torch.zeros(n), torch.zeros(n)
    for t, g in enumerate(grads, 1):
        twin_adam([p], [g], [m], [v], [OC.hyper(lr=lr, t=t)])
    out['twin'] = (p.double() - p0.double(), m.double(), v.double())
    return {k: tuple(float((a - b).abs().max()) for a, b in zip(x, ref)) for k, x in out.items()}


@pytest.mark.parametrize('lr', [5e-6, 2.5e-5, 1e-3])
def test_twin_is_as_close_to_float64_adam_as_torch_float32_is(lr):
    """Both paths round every state word once per step, so neither is systematically closer; the factor 2 covers the luck of
    individual roundings.  Measured on these inputs (twin / torch, the same for foreach False and True and at every lr but for the
    displacement's size): displacement 1.00 (1.27e-7, 1.31e-7, 1.57e-7 for both: the parameter's own rounding dominates), exp_avg 0.81
    (4.87e-7 / 6.04e-7), exp_avg_sq 0.55 (5.19e-7 / 9.41e-7)."""
    e = _errors_against_float64(lr)
    print(f'lr {lr}:', {k: tuple(f'{x:.3e}' for x in v) for k, v in e.items()})
    for path in ('foreach=False', 'foreach=True'):
        for name, mine, theirs in zip(('displacement', 'exp_avg', 'exp_avg_sq'), e['twin'], e[path]):
            assert theirs > 0 and mine <= 2.0 * theirs, (lr, path, name, mine, theirs)


@pytest.mark.parametrize('tau', [0.005, 0.1])
def test_polyak_twin_is_as_close_to_float64_as_soft_update_is(tau):
    """50 applications towards a net that moves every time: the twin, and agents._soft_update in float32, against _soft_update on
    float64 copies.  Measured: 3.2e-8 / 5.2e-8 at tau 0.005, 4.3e-8 / 1.0e-7 at tau 0.1."""
    torch.manual_seed(3)
    cur = torch.nn.Linear(400, 500)                                   # 200 500 elements
    nets = {k: torch.nn.Linear(400, 500) for k in ('twin', 'torch')}
    nets['torch'].load_state_dict(nets['twin'].state_dict())
    ref, cur64 = torch.nn.Linear(400, 500).double(), torch.nn.Linear(400, 500).double()
    ref.load_state_dict(nets['twin'].state_dict())
    for _ in range(50):
        with torch.no_grad():
            for p in cur.parameters():
                p.add_(torch.randn_like(p) * 0.01)
        cur64.load_state_dict(cur.state_dict())
        A._soft_update(ref, cur64, tau)
        A._soft_update(nets['torch'], cur, tau)
        twin_polyak([p.detach() for p in nets['twin'].parameters()], [p.detach() for p in cur.parameters()], tau)
    err = {k: max(float((p.detach().double() - q.detach()).abs().max()) for p, q in zip(n.parameters(), ref.parameters())) for k, n in nets.items()}
    print(f'tau {tau}:', err)
    assert err['torch'] > 0 and err['twin'] <= 2.0 * err['torch'], err


def test_sanitizer_driver_of_the_twins_runs_clean(tmp_path):
    """tests/optim_host_sanitize.cpp, a stand-alone program, compiled by the host compiler with -fsanitize=address,undefined"""
    cxx = os.environ.get('CXX') or shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    assert cxx, 'no host C++ compiler'
    exe = str(tmp_path / 'optim_host_sanitize')
    cmd = [cxx, '-std=c++17', '-O1', '-g', '-ffp-contract=off', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
           '-I' + os.path.join(ROOT, 'include'), '-I' + os.path.join(ROOT, 'hope_amd', 'csrc'),
           os.path.join(ROOT, 'tests', 'optim_host_sanitize.cpp'), '-o', exe]
    # the runtime linked into the program where the compiler can (gcc's switch; clang does so by default and may not know it)
    if subprocess.run(cmd + ['-static-libasan'], capture_output=True).returncode != 0:
        subprocess.check_call(cmd)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and 'clean' in r.stdout, (r.returncode, r.stdout, r.stderr)
