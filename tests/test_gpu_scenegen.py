"""-m gpu: the HIP lot generator (k_scenegen) and the pool refill that never leaves the device (hope_env_generate_pool).

The kernel and the host twin hope_scenegen_generate_det compile one source (hope_amd/csrc/hope_scenegen_core.h) made of operations
IEEE-754 defines exactly, so every comparison of lots below is bit for bit (np.array_equal on float64), and every comparison of
step outputs between a handle whose pool was generated on the device and one that was given the twin's lots is torch.equal."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

LEVELS = ('Normal', 'Complex', 'Extrem')
SENT = -12345.678
OUT_NAMES = ('lidar', 'action_mask', 'target', 'reward', 'reward_info', 'status', 'done', 'pose', 'rs_word', 'rs_lengths')


def sentinel_out(n, mo, dev='cuda:0'):
    f64 = dict(dtype=torch.float64, device=dev)
    return (torch.full((n, 3), SENT, **f64), torch.full((n, 3), SENT, **f64), torch.full((n, 4), SENT, **f64),
            torch.full((n, mo, 4, 2), SENT, **f64), torch.full((n,), -7, dtype=torch.int32, device=dev),
            torch.full((n,), -7, dtype=torch.int32, device=dev))


def twin_with_sentinel(level, n, seed, mo, first_index, bay_mode):
    """generate_arrays_det into arrays pre-filled with the sentinel (rows beyond n_obst keep it)"""
    from hope_amd import _lib as L
    from hope_amd.scene_gen import LEVEL_ID
    lib = L.load_library()
    start, dest, bbox = np.full((n, 3), SENT), np.full((n, 3), SENT), np.full((n, 4), SENT)
    verts = np.full((n, mo, 4, 2), SENT)
    nob, cid = np.full(n, -7, np.int32), np.full(n, -7, np.int32)
    L.check(lib.hope_scenegen_generate_det(LEVEL_ID[level], bay_mode, n, seed, first_index, mo, start.ctypes.data, dest.ctypes.data,
                                           bbox.ctypes.data, verts.ctypes.data, nob.ctypes.data, cid.ctypes.data, 0), 'det')
    return start, dest, bbox, verts, nob, cid


def twin_pool(n_pool, levels, seed, batch, mo):
    """the lots hope_env_generate_pool must produce, from the host twin -> (start, dest, bbox, verts, n_obst, nvert)"""
    from hope_amd.scene_gen import LEVEL_ID, generate_arrays_det, pool_level_counts
    counts = pool_level_counts(n_pool, levels)
    parts = [generate_arrays_det(lv, counts[LEVEL_ID[lv]], seed=seed * 1000003 + LEVEL_ID[lv], max_obst=mo, first_index=batch * n_pool)
             for lv in levels if counts[LEVEL_ID[lv]] > 0]
    return tuple(np.concatenate([p[j] for p in parts]) for j in range(6))


@pytest.mark.parametrize('level,bay_mode', [('Normal', 1), ('Complex', 1), ('Normal', 0), ('Complex', 0), ('Extrem', 0),
                                            ('Normal', -1), ('Complex', -1), ('Extrem', -1)])
def test_device_lots_equal_the_host_twin_bit_for_bit(level, bay_mode):
    from hope_amd.scene_gen import generate_arrays_device
    n = 20000
    for mo, first in ((32, 0), (128, 2 ** 32 + 12345)):
        seed = 4321 + mo
        out = generate_arrays_device(level, n, seed=seed, max_obst=mo, first_index=first, bay_mode=bay_mode, out=sentinel_out(n, mo))
        torch.cuda.synchronize()
        want = twin_with_sentinel(level, n, seed, mo, first, bay_mode)
        for name, a, b in zip(('start', 'dest', 'bbox', 'verts', 'n_obst', 'case_id'), out, want):
            assert np.array_equal(a.cpu().numpy(), b), (level, bay_mode, mo, name)
        nob = want[4]
        assert nob.min() >= 3 and nob.max() <= 17
        v = out[3].cpu().numpy()
        beyond = np.arange(mo)[None, :] >= nob[:, None]
        assert (v[beyond] == SENT).all() and (v[~beyond] != SENT).all()                  # rows beyond n_obst untouched
        if bay_mode >= 0:
            assert (want[5] == (0 if bay_mode == 1 else 1)).all()
        # one call of n == two calls that split it
        k = 7777
        a = generate_arrays_device(level, k, seed=seed, max_obst=mo, first_index=first, bay_mode=bay_mode)
        b = generate_arrays_device(level, n - k, seed=seed, max_obst=mo, first_index=first + k, bay_mode=bay_mode)
        whole = generate_arrays_device(level, n, seed=seed, max_obst=mo, first_index=first, bay_mode=bay_mode)
        torch.cuda.synchronize()
        for x, y, w in zip(a, b, whole):
            assert torch.equal(torch.cat([x, y]), w)


def test_generate_device_refuses_bad_arguments():
    from hope_amd import _lib as L
    from hope_amd.scene_gen import generate_arrays_device
    with pytest.raises(L.HopeError, match='18'):
        generate_arrays_device('Normal', 64, max_obst=17)
    out = generate_arrays_device('Normal', 0, max_obst=32)                               # n = 0: nothing to do
    assert out[0].shape == (0, 3)


def make_env(n, mo=128, seed=3, unique=256, **kw):
    from hope_amd import ParkingBatch
    from hope_amd.scene_gen import mixed_arrays
    init = mixed_arrays(unique, levels=LEVELS, seed=seed, max_obst=mo)
    env = ParkingBatch(n, mo, obs_dtype=torch.float64, action_dtype=torch.float64, **kw)
    sl = np.arange(n) % unique
    env.set_scene_arrays(np.arange(n), init[0][sl], init[1][sl], init[2][sl], init[3][sl], init[4][sl])
    return env


def test_generated_pool_holds_the_twins_lots_and_steps_like_an_uploaded_pool():
    """generate_pool + redraw of every scene: download_scenes returns the twin's lot named by pool_index(); the oracle agrees on
    the downloaded maps; and a few hundred HOPE_AUTO_REDRAW steps equal, output for output, those of a second handle that was
    given the twin's lots through set_pool (so the constant records k_scenegen writes equal what set_pool computes)."""
    from oracle import oracle as O
    n, mo, P = 2048, 128, 1000
    a, b = make_env(n, mo), make_env(n, mo)
    a.generate_pool(P, LEVELS, seed=11, batch=3)
    pool = twin_pool(P, LEVELS, 11, 3, mo)
    assert (pool[4] <= 17).all()
    b.set_pool(pool)
    ones = torch.ones(n, dtype=torch.uint8, device=a.device)
    for e in (a, b):
        e.redraw(ones, seed=77)
    torch.cuda.synchronize()
    idx = a.pool_index()
    assert np.array_equal(idx, b.pool_index()) and (idx >= 0).all() and len(np.unique(idx)) > P // 2
    got_a, got_b = a.download_scenes(np.arange(n)), b.download_scenes(np.arange(n))
    for j, name in enumerate(('start', 'dest', 'bbox')):
        assert np.array_equal(got_a[j], pool[j][idx]), name
    assert np.array_equal(got_a[4], pool[4][idx])
    used = np.arange(mo)[None, :] < got_a[4][:, None]
    assert np.array_equal(got_a[3][used], pool[3][idx][used])
    for x, y in zip(got_a[:3], got_b[:3]):
        assert np.array_equal(x, y)
    assert a.pool_overflow() == 0
    # the oracle on the downloaded maps, as tests/test_gpu_parity.py does for an uploaded pool
    t = a.tables
    O.set_tables(hull_base=t['hull_base'], beam_a=t['beam_ab'][:, 0], beam_b=t['beam_ab'][:, 1], dist_star=t['dist_star'])
    orc = O.BatchOracle(n, mo, omp=True)
    verts = np.where(used[:, :, None, None], got_a[3], 0.0)
    orc.set_scenes(np.arange(n), got_a[0], got_a[1], got_a[2], verts, np.full((n, mo), 4, np.int32), got_a[4])
    a.reset_obs(); b.reset_obs()
    o = orc.reset_obs(with_rs=True)
    rng = np.random.default_rng(5)
    for it in range(3):
        torch.cuda.synchronize()
        assert np.array_equal(a.status.cpu().numpy(), o['status'])
        assert np.array_equal(a.action_mask.cpu().numpy(), o['mask'])
        for k, ok in (('lidar', 'lidar'), ('target', 'target'), ('reward', 'reward')):
            assert np.array_equal(getattr(a, k).cpu().numpy(), o[ok]), (it, k)
        w = a.rs_word.cpu().numpy()
        assert np.array_equal(w[:, 6], o['rs_found']) and np.array_equal(w[:, :5], o['rs_ctypes'])
        act = rng.uniform(-1, 1, (n, 2))
        for e in (a, b):
            e.step(torch.from_numpy(act).to(e.device))
        o = orc.step(act, with_rs=True)
    # fused turnover on the generated pool == on the uploaded twin pool
    t0 = rng.integers(150, 200, n)
    for e in (a, b):
        e.upload_state(t=t0)
        e.set_redraw_seed(555)
    g = torch.Generator(device='cuda').manual_seed(9)
    turned = 0
    for it in range(300):
        act = torch.rand((n, 2), device='cuda', generator=g, dtype=torch.float64) * 2 - 1
        a.step(act, auto_reset=True, fresh=True)
        b.step(act, auto_reset=True, fresh=True)
        if it % 10 == 9 or it == 299:
            torch.cuda.synchronize()
            turned += int(a.done.sum().item())
            for k in OUT_NAMES:
                assert torch.equal(getattr(a, k), getattr(b, k)), (it, k)
    sa, sb = a.download_state(), b.download_state()
    assert all(np.array_equal(x, y) for x, y in zip(sa, sb))
    assert np.array_equal(a.pool_index(), b.pool_index())
    ga, gb = a.download_scenes(np.arange(n)), b.download_scenes(np.arange(n))
    assert all(np.array_equal(x, y) for x, y in zip(ga[:3], gb[:3])) and np.array_equal(ga[4], gb[4])
    assert turned > 100 and a.pool_overflow() == 0
    a.close(); b.close()


@pytest.mark.parametrize('relaxed', [False, True])
def test_strict_and_relaxed_swap_end_with_the_new_pool(relaxed):
    n, mo, P = 1024, 128, 300
    env = make_env(n, mo)
    env.generate_pool(P, LEVELS, seed=1, batch=0)
    env.reset_obs()
    g0 = env.pool_generation()
    env.generate_pool(P, LEVELS, seed=1, batch=1, relaxed=relaxed)
    assert env.pool_generation() != g0                      # (pool_generation applies a pending relaxed swap)
    env.redraw(torch.ones(n, dtype=torch.uint8, device=env.device), seed=5)
    torch.cuda.synchronize()
    idx = env.pool_index()
    new = twin_pool(P, LEVELS, 1, 1, mo)
    got = env.download_scenes(np.arange(n))
    assert np.array_equal(got[0], new[0][idx]) and np.array_equal(got[1], new[1][idx]) and np.array_equal(got[4], new[4][idx])
    env.close()


def test_generate_pool_between_deferred_steps_equals_commit_pool_of_the_twin_at_the_same_step():
    n, mo, P = 4096, 128, 600
    a, b = make_env(n, mo), make_env(n, mo)
    first = twin_pool(P, LEVELS, 21, 0, mo)
    a.generate_pool(P, LEVELS, seed=21, batch=0)
    b.set_pool(first)
    rng = np.random.default_rng(8)
    t0 = rng.integers(170, 200, n)
    for e in (a, b):
        e.set_redraw_seed(31)
        e.reset_obs()
        e.upload_state(t=t0)
    g = torch.Generator(device='cuda').manual_seed(2)
    for it in range(40):
        act = torch.rand((n, 2), device='cuda', generator=g, dtype=torch.float64) * 2 - 1
        if it in (7, 8, 20):                                 # (two refills on consecutive steps as well)
            batch = {7: 1, 8: 2, 20: 3}[it]
            a.generate_pool(P, LEVELS, seed=21, batch=batch)
            nxt = twin_pool(P, LEVELS, 21, batch, mo)
            st = b.pool_staging(P)
            for dst, src in zip(st, nxt[:5]):
                dst[...] = src
            b.commit_pool(P)
        for e in (a, b):
            e.step(act, auto_reset=True, fresh=True, defer_rs=True)
        for e in (a, b):
            e.wait_rs()
        torch.cuda.synchronize()
        for k in OUT_NAMES:
            assert torch.equal(getattr(a, k), getattr(b, k)), (it, k)
        assert np.array_equal(a.pool_index(), b.pool_index())
    assert all(np.array_equal(x, y) for x, y in zip(a.download_state(), b.download_state()))
    a.close(); b.close()


def test_dlp_cases_stay_drawable_after_generate_pool():
    n, mo, P = 2048, 128, 400
    env = make_env(n, mo)
    env.set_draw_class(np.arange(3, n, 4), 1)                # every fourth slot belongs to the large class
    env.set_dlp_cases()
    env.generate_pool(P, LEVELS, seed=2)
    env.generate_pool(P, LEVELS, seed=2, batch=1, relaxed=True)
    env.redraw(torch.ones(n, dtype=torch.uint8, device=env.device), seed=3)
    torch.cuda.synchronize()
    idx = env.pool_index()
    large = np.arange(n) % 4 == 3
    assert (idx[large] <= -2).all() and len(np.unique(idx[large])) > 20       # Dragon-Lake cases, drawn by large-class slots only
    assert (idx[~large] >= 0).all() and (idx[~large] < P).all()
    nob = env.n_obst_now()
    assert (nob[~large] <= 17).all()
    assert env.pool_overflow() == 0
    env.close()


def test_pool_generation_is_a_function_of_the_arguments_and_guards_restore_maps():
    n, mo, P = 512, 128, 200
    a, b = make_env(n, mo), make_env(n, mo)
    a.generate_pool(P, LEVELS, seed=5, batch=2)
    b.generate_pool(P, LEVELS, seed=5, batch=2)
    ga = a.pool_generation()
    assert ga != 0 and ga == b.pool_generation()
    c = make_env(n, mo)
    c.generate_pool(P, LEVELS, seed=6, batch=2)
    d = make_env(n, mo)
    d.generate_pool(P, LEVELS, seed=5, batch=3)
    e = make_env(n, mo)
    e.generate_pool(P, ('Normal', 'Complex'), seed=5, batch=2)
    assert len({ga, c.pool_generation(), d.pool_generation(), e.pool_generation()}) == 4
    for x in (b, c, d, e):
        x.close()
    # snapshot / restore on a generated pool
    a.set_redraw_seed(9)
    a.redraw(torch.ones(n, dtype=torch.uint8, device=a.device), seed=9)
    torch.cuda.synchronize()
    maps = a.download_scenes(np.arange(n))
    pidx, ep = a.pool_state()
    a.redraw(torch.ones(n, dtype=torch.uint8, device=a.device), seed=9)       # move on: other maps
    torch.cuda.synchronize()
    assert not np.array_equal(a.pool_index(), pidx)
    a.restore_maps(pidx, ep, seed=9, generation=ga)
    torch.cuda.synchronize()
    back = a.download_scenes(np.arange(n))
    assert np.array_equal(a.pool_index(), pidx)
    assert all(np.array_equal(x, y) for x, y in zip(maps[:3], back[:3])) and np.array_equal(maps[4], back[4])
    a.generate_pool(P, LEVELS, seed=5, batch=4)
    from hope_amd import _lib as L
    with pytest.raises(L.HopeError, match='replaced'):
        a.restore_maps(pidx, ep, seed=9, generation=ga)
    a.close()


def test_generate_pool_misuse_returns_the_documented_codes():
    import ctypes as C
    from hope_amd import ParkingBatch, _lib as L
    lib = L.load_library()
    n, mo, P = 256, 128, 90
    env = make_env(n, mo)

    def call(h, n_pool, counts, seed=0, first=0, relaxed=0):
        return lib.hope_env_generate_pool(h, n_pool, (C.c_int32 * 3)(*counts) if counts is not None else None, seed, first, relaxed)
    assert call(env.h, 0, (0, 0, 0)) == L_EINVAL
    assert call(env.h, -3, (0, 0, -3)) == L_EINVAL
    assert call(env.h, P, (30, 30, 31)) == L_EINVAL                          # counts do not sum to n_pool
    assert call(env.h, P, (60, 60, -30)) == L_EINVAL                         # a negative count
    assert call(env.h, P, None) == L_EINVAL
    assert call(None, P, (30, 30, 30)) == L_EINVAL                           # null handle
    st = env.pool_staging(P)                                                 # an uncommitted staging fill
    assert call(env.h, P, (30, 30, 30)) == L_ESTATE
    assert b'staging' in lib.hope_last_error()
    nxt = twin_pool(P, LEVELS, 1, 0, mo)
    for dst, src in zip(st, nxt[:5]):
        dst[...] = src
    env.commit_pool(P)
    assert call(env.h, P, (30, 30, 30)) == 0                                 # the handle is still usable
    assert call(env.h, P, (90, 0, 0), relaxed=1) == 0
    env.redraw(torch.ones(n, dtype=torch.uint8, device=env.device), seed=1)
    env.reset_obs()
    torch.cuda.synchronize()
    assert (env.pool_index() >= 0).all() and bool(torch.isfinite(env.lidar).all())
    env.close()
    small = ParkingBatch(64, 16, obs_dtype=torch.float64, action_dtype=torch.float64)    # a handle that cannot hold a generated lot
    assert call(small.h, 30, (10, 10, 10)) == L_EINVAL
    small.close()
    with pytest.raises(ValueError):
        from hope_amd.scene_gen import pool_level_counts
        pool_level_counts(30, ('Complex', 'Normal'))


L_EINVAL, L_ESTATE = -1, -5


@pytest.mark.parametrize('kind', ['ppo', 'sac'])
def test_device_pool_refresher_keeps_a_rollout_fresh_without_the_host_generator(kind, monkeypatch):
    from hope_amd import agents as A, scene_gen as SG
    from hope_amd.rollout import PPOTrainer, SACTrainer

    def refuse(*a, **k):
        raise AssertionError('the host PoolRefresher must not be constructed')
    monkeypatch.setattr(SG.PoolRefresher, '__init__', refuse)
    host_calls = []
    monkeypatch.setattr(SG, 'generate_arrays', lambda *a, **k: host_calls.append(1))
    torch.manual_seed(0)
    n, P = 2048, 512
    env = make_env_f32(n)
    env.generate_pool(P, LEVELS, seed=4)
    ref = SG.DevicePoolRefresher(env, P, LEVELS, seed=4, relaxed=(kind == 'sac'))
    ref.batch = 1
    g0 = env.pool_generation()
    if kind == 'ppo':
        ag = A.BatchedPPO(device='cuda', use_img=False, mini_batch=n, mini_epoch=1)
        tr = PPOTrainer(env, ag, horizon=4, seed=3, fresh_scenes=True, pool_refresher=ref)
        out = [tr.step() for _ in range(12)]
        assert tr.updates == 3 and ref.commits == 3 and ref.batch == 4
    else:
        ag = A.BatchedSAC(device='cuda', use_img=False, batch_size=1024)
        tr = SACTrainer(env, ag, horizon=4, update_every=1, seed=3, fresh_scenes=True, pool_refresher=ref)
        out = [tr.step() for _ in range(40)]
        assert tr.updates >= 32 and ref.commits == tr.updates // 16
    torch.cuda.synchronize()
    assert all(np.isfinite(np.asarray(o, dtype=np.float64)).all() for o in out if o is not None)
    assert env.pool_generation() != g0 and not host_calls
    s = tr.stats()
    assert np.isfinite(s['mean_reward'])
    idx = env.pool_index()
    assert (idx < P).all() and env.pool_overflow() == 0
    ref.close()
    env.close()


def make_env_f32(n, mo=128, unique=256):
    from hope_amd import ParkingBatch
    from hope_amd.scene_gen import generate_arrays_det
    parts = [generate_arrays_det(lv, unique // 2, seed=70 + j, max_obst=mo) for j, lv in enumerate(('Normal', 'Complex'))]
    init = tuple(np.concatenate([p[j] for p in parts]) for j in range(5))
    env = ParkingBatch(n, mo)
    sl = np.arange(n) % (2 * (unique // 2))
    env.set_scene_arrays(np.arange(n), init[0][sl], init[1][sl], init[2][sl], init[3][sl], init[4][sl])
    return env
