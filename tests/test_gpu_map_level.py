"""k_map_level on the MI355X (include/hope_env.h "map difficulty label"): the kernel equals the host compilation of the same core
on every int, on packed arrays and on a handle's own tiles after device-side draws, joined and pipelined; the evaluator's level
column; the error codes; and the time against the Python classifier."""
import ctypes as C
import time

import numpy as np
import pytest
import torch

import maplevel_sets as S
from hope_amd import map_level as M

pytestmark = pytest.mark.gpu

LEVELS = ('Normal', 'Complex', 'Extrem')
OK, EINVAL, ESTATE = 0, -1, -5


@pytest.fixture(scope='module')
def scene_sets():
    return S.golden_scenes() + S.fresh_scenes()


def make_env(n, mo=128, seed=3, unique=256, dlp_every=0, pool=0, pool_seed=11, **kw):
    from hope_amd import ParkingBatch
    from hope_amd.scene_gen import mixed_arrays
    init = mixed_arrays(unique, levels=LEVELS, seed=seed, max_obst=mo)
    env = ParkingBatch(n, mo, **kw)
    sl = np.arange(n) % unique
    env.set_scene_arrays(np.arange(n), init[0][sl], init[1][sl], init[2][sl], init[3][sl], init[4][sl])
    if dlp_every:
        env.set_draw_class(np.arange(dlp_every - 1, n, dlp_every), 1)
        env.set_dlp_cases()
    if pool:
        env.generate_pool(pool, LEVELS, seed=pool_seed)
    return env


def host_labels_of(env):
    start, dest, _, verts, nob = env.download_scenes(np.arange(env.n))
    return M.get_map_levels_host(start, dest, verts, nob, detail=True), (start, dest, verts, nob)


@pytest.mark.parametrize('mo', [32, 128, 255])
def test_device_equals_host_on_every_int(scene_sets, mo):
    """hope_map_level_device == hope_map_level_host, labels and detail records, on the golden and the fresh set (the scenes that
    fit max_obstacles)"""
    sc = [s for s in scene_sets if len(s[2]) <= mo]
    assert len(sc) >= (2500 if mo == 32 else 4000)
    packed = M.pack_rings(sc, mo)
    lv, det = M.get_map_levels_host(*packed, detail=True)
    dev = [torch.from_numpy(a).cuda() for a in packed]
    lv_d, det_d = M.get_map_levels_device(*dev, detail=True)
    lv_only = M.get_map_levels_device(*dev)
    torch.cuda.synchronize()
    assert np.array_equal(lv_d.cpu().numpy(), lv) and np.array_equal(det_d.cpu().numpy(), det)
    assert np.array_equal(lv_only.cpu().numpy(), lv)                           # the early-out form gives the same label
    assert set(lv.tolist()) == {0, 1, 2}


def test_handle_labels_after_device_side_draws_joined_and_pipelined():
    """Two handles in lockstep -- 4 096 scenes, every 4th a Dragon-Lake slot, a generated pool, 300 steps of fused turnover on NEW
    maps -- one joined, one with deferred Reeds-Shepp (pipelined steps), hope_env_map_level called between the steps: both give
    the same labels and detail records at every checkpoint, and they equal download_scenes -> hope_map_level_host.  An `active`
    mask leaves the other entries' sentinel alone."""
    n = 4096
    envs = [make_env(n, dlp_every=4, pool=900), make_env(n, dlp_every=4, pool=900)]
    for env in envs:
        env.redraw(torch.ones(n, dtype=torch.uint8, device=env.device), seed=5)
        env.set_redraw_seed(99)
        env.reset_obs()
        env.upload_state(t=np.random.default_rng(1).integers(120, 200, n))
    g = torch.Generator(device='cuda').manual_seed(4)
    first = envs[0].map_levels().clone()
    turned = torch.zeros(n, dtype=torch.bool, device='cuda')
    for it in range(300):
        act = torch.rand((n, 2), device='cuda', generator=g) * 2 - 1
        envs[0].step(act, auto_reset=True, fresh=True)
        envs[1].step(act, auto_reset=True, fresh=True, defer_rs=True)
        turned |= envs[0].done.bool()
        if it % 60 == 59:
            a = envs[0].map_levels(detail=True)
            b = envs[1].map_levels(detail=True)                                # between two pipelined steps: joins the search itself
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), it
    envs[1].wait_rs()
    torch.cuda.synchronize()
    assert int(turned.sum()) > n // 2                                          # most scenes hold a map drawn inside a step kernel
    for env in envs:
        lv, det = env.map_levels(detail=True)
        (hl, hd), _ = host_labels_of(env)
        assert np.array_equal(lv.cpu().numpy(), hl) and np.array_equal(det.cpu().numpy(), hd)
        assert env.pool_overflow() == 0
    assert set(hl.tolist()) == {0, 1, 2} and not torch.equal(first, lv)
    env = envs[0]
    mask = (torch.arange(n, device='cuda') % 3 == 0).to(torch.uint8)
    out = torch.full((n,), 77, dtype=torch.uint8, device='cuda')
    det = torch.full((n, 8), -9, dtype=torch.int32, device='cuda')
    env.map_levels(active=mask, out=out, detail=det)
    torch.cuda.synchronize()
    on = mask.bool().cpu().numpy()
    assert (out.cpu().numpy()[~on] == 77).all() and (det.cpu().numpy()[~on] == -9).all()
    assert np.array_equal(out.cpu().numpy()[on], hl[on]) and np.array_equal(det.cpu().numpy()[on], hd[on])
    for e in envs:
        e.close()


def _dlp_eval_env(n):
    env = make_env(n, dlp_every=1)
    env.redraw(torch.ones(n, dtype=torch.uint8, device=env.device), seed=21)    # every slot: a Dragon-Lake lot drawn on the device
    return env


def test_evaluator_levels_on_device_drawn_dlp_lots():
    from hope_amd import agents as A
    from hope_amd import evaluate as E
    n = 512
    recs = []
    for levels in (False, True):
        env = _dlp_eval_env(n)
        (hl, _), (_, _, _, nob) = host_labels_of(env)
        assert (env.pool_index() <= -2).all() and nob.min() > 17                # Dragon-Lake draws, none of the uploaded lots
        torch.manual_seed(0)
        ev = E.BatchedEvaluator(env, A.BatchedPPO(device='cuda', use_img=False), post_proc_action=True, seed=3)
        recs.append(ev.run(max_steps=60, **({'levels': True} if levels else {})).cpu().numpy())
        if levels:
            assert np.array_equal(ev.levels.cpu().numpy(), hl)
        env.close()
    plain, with_lv = recs
    assert plain.shape == (n, 4) and with_lv.shape == (n, 5)
    assert np.array_equal(plain, with_lv[:, :4])
    s = E.summarize(with_lv)
    for k, name in enumerate(M.LEVEL_NAMES):
        assert s.get(name, {'episodes': 0})['episodes'] == int((hl == k).sum())
    assert len([k for k in s if k != 'all']) >= 2
    print('per-level episodes:', {k: v['episodes'] for k, v in s.items()})


def test_misuse_returns_the_documented_codes():
    """through the ABI as a foreign binding would call it; nothing reaches a kernel"""
    from hope_amd import _lib as L
    lib = L.load_library()
    n, mo = 16, 32
    st, de = torch.zeros((n, 3), dtype=torch.float64, device='cuda'), torch.zeros((n, 3), dtype=torch.float64, device='cuda')
    ve, nob = torch.zeros((n, mo, 4, 2), dtype=torch.float64, device='cuda'), torch.zeros(n, dtype=torch.int32, device='cuda')
    lv = torch.zeros(n, dtype=torch.uint8, device='cuda')
    p = lambda t: C.c_void_p(t.data_ptr())

    def dev(n_=n, mo_=mo, level=p(lv), start=p(st)):
        return lib.hope_map_level_device(0, n_, mo_, start, p(de), p(ve), p(nob), level, None, None)
    assert dev() == OK
    for kw in (dict(n_=0), dict(n_=-1), dict(mo_=0), dict(mo_=256), dict(level=None), dict(start=None)):
        assert dev(**kw) == EINVAL and lib.hope_last_error(), kw
    torch.cuda.synchronize()
    assert (lv == 0).all()                                                      # no obstacles: Normal
    h = C.c_void_p()
    assert lib.hope_env_create(C.byref(h), n, mo, 0, 0) == OK
    assert lib.hope_env_map_level(h, None, p(lv), None, None) == ESTATE         # no scenes yet
    assert b'set_scenes' in lib.hope_last_error()
    assert lib.hope_env_map_level(h, None, None, None, None) == EINVAL
    assert lib.hope_env_map_level(None, None, p(lv), None, None) == EINVAL
    assert lib.hope_env_destroy(h) == OK
    assert lib.hope_env_map_level(h, None, p(lv), None, None) == EINVAL         # a destroyed handle
    env = make_env(n, mo=mo, unique=16)
    with pytest.raises(L.HopeError):
        env.map_levels(out=torch.zeros(n, dtype=torch.int32, device='cuda'))
    assert env.map_levels().shape == (n,)
    env.close()


def test_a_thousand_times_the_python_route():
    """hope_env_map_level on 4 096 mixed scenes (every 4th a Dragon-Lake lot), event-timed, against the only route the library had:
    download_scenes + Python get_map_level, timed here on a 64-scene sample of the same scenes.  Required: >= 1 000x per scene.
    Measured on an MI355X box: 0.0117 us per scene against 334 us, 28 498x."""
    n = 4096
    from hope_amd import ParkingBatch
    from hope_amd.scene_gen import mixed_arrays
    arr = mixed_arrays(n, levels=LEVELS + ('dlp',), seed=9, max_obst=128)
    env = ParkingBatch(n, 128)
    env.set_scene_arrays(np.arange(n), *arr[:5])
    out = torch.zeros(n, dtype=torch.uint8, device='cuda')
    for _ in range(3):
        env.map_levels(out=out)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    reps = 20
    a.record()
    for _ in range(reps):
        env.map_levels(out=out)
    b.record()
    torch.cuda.synchronize()
    dev_us = a.elapsed_time(b) * 1e3 / reps / n
    ids = np.arange(0, n, n // 64)[:64]
    t0 = time.perf_counter()
    start, dest, _, verts, nob = env.download_scenes(ids)
    labs = [M.get_map_level(start[k], dest[k], [verts[k, o] if not np.array_equal(verts[k, o, 3], verts[k, o, 2]) else verts[k, o, :3]
                                                  for o in range(int(nob[k]))]) for k in range(len(ids))]
    py_us = (time.perf_counter() - t0) * 1e6 / len(ids)
    assert [M.LEVEL_NAMES.index(v) for v in labs] == out.cpu().numpy()[ids].tolist()
    print(f'k_map_level {dev_us:.4f} us per scene ({dev_us * n / 1e3:.3f} ms for {n}); download + Python {py_us:.0f} us per scene; ratio {py_us / dev_us:.0f}x')
    assert py_us / dev_us >= 1000.0
    env.close()
