"""The advantage block's rule (hope_amd/csrc/hope_gae_core.h) through its host twins hope_gae_host / hope_adv_normalize_host, on the
CPU: the scan against agent_glue.batched_gae word for word, the sums against exact arithmetic, mean / std / normalisation against
the torch formula, the sums' independence of the geometry, DeviceGae inside BatchedPPO and PPOTrainer on the stand-in env, two
gloo ranks, and the sanitizer driver of the twins."""
import math
import os
import shutil
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gae_script as GS  # noqa: E402
from hope_amd import _lib as L  # noqa: E402
from hope_amd import agent_glue as G  # noqa: E402
from hope_amd import agents as A  # noqa: E402

ROWS = (1, 2, 63, 64, 65, 193)
TS = (1, 2, 5, 16, 17)
ULP32 = lambda x: float(np.spacing(np.float32(abs(float(x)))))  # noqa: E731


def _torch_block(reward, done, value, v_last, value_target, gamma, lam):
    """the parent's torch path: batched_gae on a concatenated next_value, the float32 value target"""
    r, d, v, vl, vt = (torch.from_numpy(a) for a in (reward, done, value, v_last, value_target))
    nv = torch.cat([v[:, 1:], vl.unsqueeze(1)], dim=1)
    adv, delta = G.batched_gae(r, v, nv, d, gamma, lam)
    return adv.numpy(), (adv + vt).numpy(), delta.numpy()


@pytest.mark.parametrize('gamma,lam', [(0.98, 0.95), (0.9, 0.5)])
def test_twin_scan_equals_batched_gae_word_for_word(gamma, lam):
    """rows 1 .. 193 x T 1 .. 17 x the five done patterns: adv, v_target and delta as uint32 words; flags do not change them"""
    for rows in ROWS:
        for t in TS:
            for pat in GS.PATTERNS:
                x = GS.inputs(rows, t, pat)
                adv, v_target, sums, delta = GS.host_gae(*x, gamma, lam, flags=0)
                want = _torch_block(*x, gamma, lam)
                for got, ref, name in zip((adv, v_target, delta), want, ('adv', 'v_target', 'delta')):
                    assert np.array_equal(GS.words(got), GS.words(ref)), (rows, t, pat, name)
                assert np.array_equal(sums, [-1.0, -1.0, -1.0])                  # no flag: no sums
    a2, t2, _, d2 = GS.host_gae(*x, gamma, lam, flags=L.GAE_SUMS)
    assert all(np.array_equal(GS.words(p), GS.words(q)) for p, q in ((a2, adv), (t2, v_target), (d2, delta)))


def _levels(rows):
    nk = (rows + 63) // 64
    return math.ceil(math.log2(nk)) if nk > 1 else 0


def test_sums_against_the_exact_value():
    """s0 and s1 against math.fsum over the same float32 adv (the squares of float32 values are exact in float64).  The order gives
    the bound: a term goes through at most T additions in its row, 6 in the wave and `levels` in the chunk tree, each rounding to
    2^-53 of a partial sum that is at most sum |term|; one more for the exact value's own rounding:
    |error| <= (T + 6 + levels + 1) 2^-53 sum |term|."""
    worst = 0.0
    for rows in ROWS + (4097,):
        for t in TS:
            for pat in GS.PATTERNS:
                adv, _, sums, _ = GS.host_gae(*GS.inputs(rows, t, pat), flags=L.GAE_SUMS, delta=False)
                a = adv.astype(np.float64).ravel().tolist()
                bound = (t + 6 + _levels(rows) + 1) * 2.0 ** -53
                for got, terms in ((sums[0], a), (sums[1], [v * v for v in a])):
                    scale = math.fsum(abs(v) for v in terms)
                    err = abs(got - math.fsum(terms))
                    assert err <= bound * scale, (rows, t, pat, err, bound * scale)
                    worst = max(worst, err / (bound * scale) if scale else 0.0)
                assert sums[2] == rows * t
    print('worst error / bound:', worst)


def _formula(s0, s1, n):
    mean = s0 / n
    var = (s1 - n * mean * mean) / max(n - 1.0, 1.0)
    return np.float32(mean), np.float32(math.sqrt(max(var, 0.0)))


def test_mean_and_std_within_one_ulp_of_the_exact_sums():
    """standard-normal inputs with |mean| <= std: the formula's condition number is then a small constant and the sums' float64
    error can only flip a float32 rounding"""
    for rows in ROWS + (4097,):
        for t in TS:
            for seed in range(8):                                               # the first draw that meets the premise (short single rows
                adv, _, sums, _ = GS.host_gae(*GS.inputs(rows, t, 'random', seed=seed), flags=L.GAE_SUMS, delta=False)   # are correlated)
                a = adv.astype(np.float64).ravel().tolist()
                em, es = _formula(math.fsum(a), math.fsum(v * v for v in a), float(rows * t))
                if rows * t == 1 or abs(float(em)) <= float(es):
                    break
            else:
                raise AssertionError(('no draw with |mean| <= std', rows, t))
            m, s = GS.host_mean_std(sums)
            assert abs(float(m) - float(em)) <= ULP32(em) and abs(float(s) - float(es)) <= ULP32(es), (rows, t, m, em, s, es)
            tm, ts = A._global_mean_std(torch.from_numpy(adv))                  # the torch path's, for the record: the same bound
            assert abs(float(m) - float(tm)) <= ULP32(em) and abs(float(s) - float(ts)) <= ULP32(es), (rows, t)


def test_apply_equals_torch_in_float32():
    """out is bit-equal to torch's (adv - m) / (s + 1e-5) from the twin's own float32 m and s; the fused call is the split call; in
    place is the same; a single element gives 0"""
    for rows, t in ((1, 1), (2, 1), (63, 5), (65, 16), (193, 17)):
        x = GS.inputs(rows, t, 'random')
        adv, _, sums, _ = GS.host_gae(*x, flags=L.GAE_SUMS, delta=False)
        m, s = GS.host_mean_std(sums)
        out = GS.host_normalize(adv, sums)
        ref = (torch.from_numpy(adv) - torch.tensor(m)) / (torch.tensor(s) + 1e-5)
        assert ref.dtype == torch.float32 and np.array_equal(GS.words(out), GS.words(ref.numpy())), (rows, t)
        fused, _, sums2, _ = GS.host_gae(*x, flags=L.GAE_NORMALIZE, delta=False)
        assert np.array_equal(GS.words(fused), GS.words(out)) and np.array_equal(GS.words(sums2), GS.words(sums))
        inplace = adv.copy()
        L.check(L.load_library().hope_adv_normalize_host(inplace.ctypes.data, inplace.size, sums.ctypes.data, inplace.ctypes.data, None))
        assert np.array_equal(GS.words(inplace), GS.words(out))
        if rows * t == 1:
            assert float(s) == 0.0 and GS.words(out)[0, 0] == 0


@pytest.mark.parametrize('rows', [1, 64, 65, 129, 4097])
def test_sums_do_not_depend_on_the_geometry(rows):
    """a numpy restatement of the order (rows, 64-row chunks, the tree with pass-through) gives the twin's very words"""
    for t in (1, 5, 16):
        adv, _, sums, _ = GS.host_gae(*GS.inputs(rows, t, 'random', seed=3), flags=L.GAE_SUMS, delta=False)
        assert np.array_equal(GS.words(sums), GS.words(GS.numpy_sums(adv))), (rows, t)


def test_host_twins_refuse_bad_arguments():
    lib = L.load_library()
    x = [np.zeros((2, 3), np.float32) for _ in range(3)] + [np.zeros(2, np.float32), np.zeros((2, 3), np.float32)]
    out = [np.zeros((2, 3), np.float32) for _ in range(2)]
    P = lambda a: None if a is None else a.ctypes.data  # noqa: E731

    def raw(x=x, rows=2, t=3, gamma=0.98, lam=0.95, flags=0, out=out):
        return lib.hope_gae_host(*(P(a) for a in x), rows, t, gamma, lam, flags, P(out[0]), P(out[1]), None, None)
    assert raw() == 0
    for kw in ({'rows': 0}, {'t': 0}, {'flags': 4}, {'gamma': float('nan')}, {'lam': float('inf')}, {'out': [None, out[1]]},
               {'x': x[:3] + [None, x[4]]}):
        assert raw(**kw) == -1 and b'hope_gae_host' in lib.hope_last_error(), kw
    s = np.array([0.0, 0.0, 1.0])
    assert lib.hope_adv_normalize_host(P(out[0]), 6, None, P(out[0]), None) == -1
    assert lib.hope_adv_normalize_host(None, 6, P(s), P(out[0]), None) == -1
    assert lib.hope_adv_normalize_host(P(out[0]), -1, P(s), P(out[0]), None) == -1


# ---- DeviceGae on the CPU stand-in env -----------------------------------------------------------------------------------------
def _small_scenes(n, seed=3):
    from hope_amd.scenes import SceneSource
    src = SceneSource(levels=('Normal', 'Complex', 'Extrem'), seed=seed)
    return [src.draw() for _ in range(n)]


def _norm_tolerance(adv, m, s):
    """how far (adv - m) / (s + 1e-5) in float32 can move when m and s each move by one float32 ulp: the difference by ulp(m) plus
    its own rounding, the divisor by ulp(s) plus its own rounding (relative to s + 1e-5), the quotient's rounding"""
    diff = np.abs(adv - m)
    div = float(s) + 1e-5
    out = diff / div
    sp = lambda a: np.spacing(np.abs(a).astype(np.float32)).astype(np.float64)  # noqa: E731
    return (ULP32(m) + sp(diff)) / div + out * (2 * ULP32(s) / div) + sp(out)


def test_agent_and_trainer_on_the_stand_in_env():
    """BatchedPPO(gae=DeviceGae(cpu env)).advantages: adv_norm=False equals the torch path exactly; adv_norm=True to within what one
    ulp of m and s allows; PPOTrainer(gae='device') runs two updates with finite losses"""
    from fake_env import OracleEnv
    from hope_amd.rollout import PPOTrainer
    scenes = _small_scenes(12)
    env = OracleEnv(scenes)
    n, t = 12, 5
    g = torch.Generator().manual_seed(5)
    obs = {'lidar': torch.rand((n, t, 120), generator=g) * 10, 'target': torch.randn((n, t, 5), generator=g),
           'action_mask': (torch.rand((n, t, 42), generator=g) < 0.7).float()}
    last = {k: v[:, 0].clone() for k, v in obs.items()}
    reward = torch.randn((n, t), generator=g)
    done = (torch.rand((n, t), generator=g) < 0.2).float()
    for adv_norm in (False, True):
        torch.manual_seed(0)
        base = A.BatchedPPO(device='cpu', use_img=False, adv_norm=adv_norm, state_norm=False)
        torch.manual_seed(0)
        dev = A.BatchedPPO(device='cpu', use_img=False, adv_norm=adv_norm, state_norm=False, gae=G.DeviceGae(env))
        assert base.gae is None and not dev.gae.on_device
        a0, v0 = base.advantages(obs, reward, done, last)
        a1, v1 = dev.advantages(obs, reward, done, last)
        assert a1.dtype == torch.float32 and a1.shape == (n, t) and v1.shape == (n, t)
        assert torch.equal(v0.view(torch.int32), v1.view(torch.int32))
        if not adv_norm:
            assert torch.equal(a0.view(torch.int32), a1.view(torch.int32)) and dev.gae.sums is None
        else:
            plain, _ = A.BatchedPPO.advantages(_with(dev, adv_norm=False, gae=None), obs, reward, done, last)
            tm, ts = A._global_mean_std(plain)
            m, s = dev.gae.mean_std()
            assert abs(m - float(tm)) <= ULP32(tm) and abs(s - float(ts)) <= ULP32(ts)
            tol = _norm_tolerance(plain.numpy().astype(np.float64), m, s)
            err = np.abs(a1.numpy().astype(np.float64) - a0.numpy().astype(np.float64))
            print('worst |device - torch| / tolerance:', float((err / tol).max()))
            assert (err <= tol).all()
            assert float(dev.gae.sums[2]) == n * t
    torch.manual_seed(0)
    ag = A.BatchedPPO(device='cpu', use_img=False, lr=1e-4, mini_batch=24, mini_epoch=2)
    tr = PPOTrainer(OracleEnv(scenes), ag, horizon=4, seed=1, gae='device')
    assert isinstance(ag.gae, G.DeviceGae) and tr.gae is ag.gae
    losses = [o for o in (tr.step() for _ in range(8)) if o is not None]
    assert tr.updates == 2 and len(losses) == 2 and np.isfinite(losses).all()
    assert float(ag.gae.sums[2]) == 12 * 4 and all(math.isfinite(v) for v in ag.gae.mean_std())
    with pytest.raises(ValueError):
        PPOTrainer(OracleEnv(scenes[:2]), A.BatchedPPO(device='cpu', use_img=False), gae='gpu')
    assert PPOTrainer(OracleEnv(scenes[:2]), A.BatchedPPO(device='cpu', use_img=False)).gae is None      # the default: the torch path


def _with(agent, **kw):
    """a shallow copy of the agent with some attributes replaced"""
    import copy
    c = copy.copy(agent)
    for k, v in kw.items():
        setattr(c, k, v)
    return c


# ---- two ranks (gloo) ----------------------------------------------------------------------------------------------------------
W2_ROWS, W2_T, W2_CUT = 193, 7, 70


def _w2_rank(rank, world, port, q):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group('gloo', rank=rank, world_size=world)
    torch.set_num_threads(1)
    x = GS.inputs(W2_ROWS, W2_T, 'random', seed=9)
    sl = slice(0, W2_CUT) if rank == 0 else slice(W2_CUT, W2_ROWS)
    dg = G.DeviceGae(types.SimpleNamespace(device='cpu', n=W2_ROWS))
    adv, v_target = dg(*(torch.from_numpy(a[sl]) for a in x), GS.GAMMA, GS.LAM)
    q.put((rank, dg.mean_std(), dg.sums.numpy().copy(), adv.numpy().copy(), v_target.numpy().copy()))
    dist.destroy_process_group()


def test_two_ranks_normalise_like_one_process():
    """both ranks hold different rows, all-reduce the three sums and end with the same m and s: the single-process values over the
    concatenation, to one float32 ulp (the two rank sums added are another order than the one tree)"""
    import torch.multiprocessing as mp
    x = GS.inputs(W2_ROWS, W2_T, 'random', seed=9)
    plain, vt1, sums1, _ = GS.host_gae(*x, flags=L.GAE_SUMS, delta=False)
    m1, s1 = GS.host_mean_std(sums1)
    one = GS.host_normalize(plain, sums1)
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = 39500 + os.getpid() % 2000
    ps = [ctx.Process(target=_w2_rank, args=(r, 2, port, q)) for r in range(2)]
    [p.start() for p in ps]
    res = sorted([q.get(timeout=300) for _ in range(2)], key=lambda r: r[0])
    [p.join(60) for p in ps]
    assert res[0][1] == res[1][1] and np.array_equal(GS.words(res[0][2]), GS.words(res[1][2]))
    m, s = res[0][1]
    assert abs(m - float(m1)) <= ULP32(m1) and abs(s - float(s1)) <= ULP32(s1)
    assert res[0][2][2] == W2_ROWS * W2_T and abs(res[0][2][0] - sums1[0]) <= 1e-12 * np.abs(plain).sum()
    got = np.concatenate([res[0][3], res[1][3]])
    assert np.array_equal(GS.words(np.concatenate([res[0][4], res[1][4]])), GS.words(vt1))       # rows are independent
    tol = _norm_tolerance(plain.astype(np.float64), float(m1), float(s1))
    assert (np.abs(got.astype(np.float64) - one.astype(np.float64)) <= tol).all()
    for r in res:                                                               # each rank's rows: the rule applied to the shared sums
        sl = slice(0, W2_CUT) if r[0] == 0 else slice(W2_CUT, W2_ROWS)
        assert np.array_equal(GS.words(r[3]), GS.words(GS.host_normalize(plain[sl], r[2])))


# ---- the sanitizer driver of the twins -----------------------------------------------------------------------------------------
def test_sanitizer_driver_of_the_twins_runs_clean(tmp_path):
    """tests/gae_host_sanitize.cpp, a stand-alone program, compiled by the host compiler with -fsanitize=address,undefined"""
    cxx = os.environ.get('CXX') or shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    assert cxx, 'no host C++ compiler'
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / 'gae_host_sanitize')
    cmd = [cxx, '-std=c++17', '-O1', '-g', '-ffp-contract=off', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
           '-I' + os.path.join(root, 'include'), '-I' + os.path.join(root, 'hope_amd', 'csrc'), os.path.join(root, 'tests', 'gae_host_sanitize.cpp'),
           '-o', exe]
    # the runtime linked into the program where the compiler can (gcc's switch; clang does so by default and may not know it)
    if subprocess.run(cmd + ['-static-libasan'], capture_output=True).returncode != 0:
        subprocess.check_call(cmd)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and 'clean' in r.stdout, (r.returncode, r.stdout, r.stderr)
