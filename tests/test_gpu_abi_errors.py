"""Error paths of the C ABI (include/hope_env.h), driven through ctypes the way a foreign binding would: every documented
misuse returns its code (never a crash, never an exception across the ABI), hope_last_error() says why, and the handle is
still usable afterwards -- the abused handle's next step equals a fresh twin's bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch

from hope_amd import _lib as L

pytestmark = pytest.mark.gpu

OK, EINVAL, ENODEV, ENOMEM, EHIP, ESTATE = 0, -1, -2, -3, -4, -5
N, MO = 256, 64


def _lib():
    return L.load_library()


def _err():
    return _lib().hope_last_error().decode(errors='replace')


def _create(flags=L.F_OVERLAP, n=N, mo=MO):
    h = C.c_void_p()
    rc = _lib().hope_env_create(C.byref(h), n, mo, 0, flags)
    assert rc == OK, _err()
    return h


def _tables(h):
    from hope_amd import tables as T
    t = T.all_tables()
    ds = np.ascontiguousarray(t['dist_star'], np.float64)
    hb = np.ascontiguousarray(t['hull_base'], np.float64)
    ab = np.ascontiguousarray(t['beam_ab'], np.float64)
    return _lib().hope_env_upload_tables(h, ds.ctypes.data, hb.ctypes.data, ab.ctypes.data)


def _scene_arrays(n=N, mo=MO, seed=3):
    from hope_amd.scene_gen import mixed_arrays
    start, dest, bbox, verts, nob, nvert = mixed_arrays(n, seed=seed, max_obst=mo, levels=('Normal', 'Complex', 'Extrem'))
    return [np.ascontiguousarray(a) for a in (start, dest, bbox, verts, nob.astype(np.int32))]


def _set_scenes(h, arrays, ids=None, nob=None, n=None):
    start, dest, bbox, verts, nob0 = arrays
    ids = np.arange(len(nob0), dtype=np.int32) if ids is None else np.asarray(ids, np.int32)
    nob = nob0 if nob is None else np.asarray(nob, np.int32)
    return _lib().hope_env_set_scenes(h, ids.ctypes.data, len(ids) if n is None else n, start.ctypes.data, dest.ctypes.data, bbox.ctypes.data,
                                      verts.ctypes.data, nob.ctypes.data)


class Outs:
    def __init__(self, n=N, image=False):
        dev = 'cuda:0'
        self.t = dict(lidar=torch.zeros((n, 120), device=dev), action_mask=torch.zeros((n, 42), device=dev), target=torch.zeros((n, 5), device=dev),
                      reward=torch.zeros(n, device=dev), reward_info=torch.zeros((n, 5), device=dev), status=torch.zeros(n, dtype=torch.int32, device=dev),
                      done=torch.zeros(n, dtype=torch.uint8, device=dev), pose=torch.zeros((n, 3), dtype=torch.float64, device=dev),
                      rs_word=torch.zeros((n, 8), dtype=torch.int8, device=dev), rs_lengths=torch.zeros((n, 5), device=dev),
                      img=torch.zeros((n, 3, 64, 64), dtype=torch.uint8, device=dev) if image else None)
        self.s = L.StepOut(*[C.c_void_p(self.t[k].data_ptr()) if self.t[k] is not None else None
                             for k in ('lidar', 'action_mask', 'target', 'reward', 'reward_info', 'status', 'done', 'pose', 'rs_word', 'rs_lengths', 'img')])


def _step(h, outs, actions, stages=L.STAGE_ALL, active=None):
    return _lib().hope_env_step(h, C.c_void_p(actions.data_ptr()) if actions is not None else None, active, stages,
                                C.byref(outs.s) if outs is not None else None, None)


def test_create_rejects_bad_arguments_and_removed_flags():
    lib = _lib()
    h = C.c_void_p()
    assert lib.hope_env_create(None, 16, 16, 0, 0) == EINVAL
    assert lib.hope_env_create(C.byref(h), 0, 16, 0, 0) == EINVAL
    assert lib.hope_env_create(C.byref(h), 16, 0, 0, 0) == EINVAL
    assert lib.hope_env_create(C.byref(h), 16, 16, 99, 0) == EINVAL and 'device_id' in _err()
    assert lib.hope_env_create(C.byref(h), 16, 16, 0, 0x20) == EINVAL and 'ABI 7' in _err()          # hipGraph replay: removed
    # each limit is named on its own: the 8-bit obstacle count of the Reeds-Shepp queue entry, not the LDS tile,
    # is what bounds max_obstacles
    assert lib.hope_env_create(C.byref(h), 16, 100000, 0, 0) == EINVAL and 'HOPE_MAX_OBSTACLES (255)' in _err()
    assert lib.hope_env_create(C.byref(h), 16, 300, 0, 0) == EINVAL and 'HOPE_MAX_OBSTACLES' in _err() and 'LDS' not in _err()
    assert lib.hope_env_create(C.byref(h), 1 << 24, 16, 0, 0) == EINVAL and '2^24' in _err()
    assert not h.value


@pytest.mark.parametrize('case', ['step_before_tables', 'step_before_scenes', 'n_obst_too_large', 'scene_id_out_of_range', 'null_arrays',
                                  'img_without_flag', 'redraw_without_reset', 'redraw_without_pool', 'pool_without_class', 'null_out',
                                  'null_actions', 'profile_without_flag', 'stale_wait_rs_step', 'null_masks', 'commit_beyond_staging',
                                  'bad_draw_class', 'restore_without_pool', 'debug_geom_bad_arguments', 'step_plan_bad_arguments'])
def test_misuse_returns_its_code_and_leaves_the_handle_usable(case):
    lib = _lib()
    arrays = _scene_arrays()
    g = torch.Generator(device='cuda:0').manual_seed(5)
    acts = [torch.rand((N, 2), device='cuda:0', generator=g) * 2 - 1 for _ in range(3)]
    h = _create()
    outs = Outs()
    ready = case not in ('step_before_tables', 'step_before_scenes')
    if ready:
        assert _tables(h) == OK and _set_scenes(h, arrays) == OK

    if case == 'step_before_tables':
        assert _step(h, outs, acts[0]) == ESTATE and 'upload_tables' in _err()
        assert lib.hope_env_reset_obs(h, None, L.STAGE_ALL, C.byref(outs.s), None) == ESTATE
        assert _tables(h) == OK
        assert _step(h, outs, acts[0]) == ESTATE and 'set_scenes' in _err()
        assert _set_scenes(h, arrays) == OK
    elif case == 'step_before_scenes':
        assert _tables(h) == OK
        assert _step(h, outs, acts[0]) == ESTATE and 'set_scenes' in _err()
        mask = torch.ones(N, dtype=torch.uint8, device='cuda:0')
        assert lib.hope_env_restart(h, C.c_void_p(mask.data_ptr()), None) == ESTATE
        assert _set_scenes(h, arrays) == OK
    elif case == 'n_obst_too_large':
        nob = arrays[4].copy()
        nob[7] = MO + 1
        assert _set_scenes(h, arrays, nob=nob) == EINVAL and 'max_obstacles' in _err()
        nob[7] = -1
        assert _set_scenes(h, arrays, nob=nob) == EINVAL
    elif case == 'scene_id_out_of_range':
        ids = np.arange(N, dtype=np.int32)
        ids[3] = N
        assert _set_scenes(h, arrays, ids=ids) == EINVAL and 'out of range' in _err()
        ids[3] = -1
        assert _set_scenes(h, arrays, ids=ids) == EINVAL
        buf = np.zeros(3)
        assert lib.hope_env_download_scenes(h, np.array([N], np.int32).ctypes.data, 1, buf.ctypes.data, None, None, None, None) == EINVAL
    elif case == 'null_arrays':
        ids = np.arange(N, dtype=np.int32)
        start, dest, bbox, verts, nob = arrays
        assert lib.hope_env_set_scenes(h, ids.ctypes.data, N, None, dest.ctypes.data, bbox.ctypes.data, verts.ctypes.data, nob.ctypes.data) == EINVAL
        assert lib.hope_env_set_scenes(h, ids.ctypes.data, N, start.ctypes.data, dest.ctypes.data, bbox.ctypes.data, None, nob.ctypes.data) == EINVAL
        assert lib.hope_env_set_scenes(h, ids.ctypes.data, -1, start.ctypes.data, dest.ctypes.data, bbox.ctypes.data, verts.ctypes.data, nob.ctypes.data) == EINVAL
        assert lib.hope_env_upload_tables(h, None, None, None) == EINVAL
        assert lib.hope_env_download_n_obst(h, None) == EINVAL
        assert lib.hope_env_last_step(h, None) == EINVAL
    elif case == 'img_without_flag':
        oi = Outs(image=True)
        assert _step(h, oi, acts[0], stages=L.STAGE_ALL | L.STAGE_IMG) == ESTATE and 'HOPE_F_IMAGE' in _err()
        h2 = _create(flags=L.F_OVERLAP | L.F_IMAGE)
        assert _tables(h2) == OK and _set_scenes(h2, arrays) == OK
        assert _step(h2, outs, acts[0], stages=L.STAGE_ALL | L.STAGE_IMG) == EINVAL and 'img' in _err()      # out->img is NULL
        assert _step(h2, oi, acts[0], stages=L.STAGE_ALL | L.STAGE_IMG) == OK
        assert lib.hope_env_destroy(h2) == OK
    elif case == 'redraw_without_reset':
        assert _step(h, outs, acts[0], stages=L.STAGE_ALL | L.AUTO_REDRAW) == EINVAL and 'HOPE_AUTO_RESET' in _err()
    elif case == 'redraw_without_pool':
        assert _step(h, outs, acts[0], stages=L.STAGE_ALL | L.AUTO_RESET | L.AUTO_REDRAW) == ESTATE and 'pool' in _err()
        mask = torch.ones(N, dtype=torch.uint8, device='cuda:0')
        assert lib.hope_env_redraw(h, C.c_void_p(mask.data_ptr()), 1, None) == ESTATE
    elif case == 'pool_without_class':
        # every resident slot is of the small class; a pool of large lots only cannot serve them
        big = _scene_arrays(n=8, seed=9)
        start, dest, bbox, verts, nob = big
        nob = np.full(8, 40, np.int32)                         # (> 32 obstacles: the large class; the vertex data is irrelevant here)
        assert lib.hope_env_set_pool(h, 8, start.ctypes.data, dest.ctypes.data, bbox.ctypes.data, verts.ctypes.data, nob.ctypes.data) == OK
        assert _step(h, outs, acts[0], stages=L.STAGE_ALL | L.AUTO_RESET | L.AUTO_REDRAW) == ESTATE and 'size class' in _err()
        nob[:] = MO + 5
        assert lib.hope_env_set_pool(h, 8, start.ctypes.data, dest.ctypes.data, bbox.ctypes.data, verts.ctypes.data, nob.ctypes.data) == EINVAL
        assert lib.hope_env_set_pool(h, 0, start.ctypes.data, dest.ctypes.data, bbox.ctypes.data, verts.ctypes.data, nob.ctypes.data) == EINVAL
    elif case == 'null_out':
        assert _step(h, None, acts[0]) == EINVAL
        assert lib.hope_env_reset_obs(h, None, L.STAGE_ALL, None, None) == EINVAL
        assert lib.hope_env_step(None, C.c_void_p(acts[0].data_ptr()), None, L.STAGE_ALL, C.byref(outs.s), None) == EINVAL
    elif case == 'null_actions':
        assert _step(h, outs, None) == EINVAL and 'actions' in _err()
    elif case == 'profile_without_flag':
        ms = np.zeros(len(L.KERNELS))
        cnt = np.zeros(len(L.KERNELS), np.int64)
        assert lib.hope_env_kernel_ms(h, ms.ctypes.data, cnt.ctypes.data, 1) == ESTATE and 'HOPE_F_PROFILE' in _err()
        assert lib.hope_env_kernel_union_ms(h, ms.ctypes.data, cnt.ctypes.data, 1) == ESTATE
        assert lib.hope_env_profile_kernels(h, 1) == ESTATE
    elif case == 'stale_wait_rs_step':
        seq = C.c_uint64(0)
        assert _step(h, outs, acts[0], stages=L.STAGE_ALL | L.DEFER_RS) == OK
        assert lib.hope_env_last_step(h, C.byref(seq)) == OK and seq.value >= 1
        first = seq.value
        assert _step(h, outs, acts[1], stages=L.STAGE_ALL | L.DEFER_RS) == OK
        assert lib.hope_env_wait_rs_step(h, first, None) == ESTATE and 'replaced' in _err()       # step k's words are gone
        assert lib.hope_env_wait_rs_step(h, first + 5, None) == EINVAL
        assert lib.hope_env_wait_rs_step(h, 0, None) == EINVAL
        assert lib.hope_env_wait_rs_step(h, first + 1, None) == OK
        assert lib.hope_env_wait_rs(h, None) == OK                                               # (nothing outstanding any more: no-op)
    elif case == 'null_masks':
        assert lib.hope_env_restart(h, None, None) == EINVAL
        assert lib.hope_env_redraw(h, None, 0, None) == EINVAL
        assert lib.hope_env_set_draw_class(h, None, 3, None) == EINVAL
        assert lib.hope_env_pool_overflow(h, None) == EINVAL
        assert lib.hope_env_pool_generation(h, None) == EINVAL
    elif case == 'commit_beyond_staging':
        ptrs = [C.c_void_p() for _ in range(5)]
        assert lib.hope_env_pool_staging(h, 4, *[C.byref(p_) for p_ in ptrs]) == OK
        assert lib.hope_env_commit_pool(h, 64, None) == ESTATE and 'staging' in _err()
        assert lib.hope_env_commit_pool(h, 0, None) == EINVAL
        assert lib.hope_env_pool_staging(h, 0, *[C.byref(p_) for p_ in ptrs]) == EINVAL
    elif case == 'bad_draw_class':
        ids = np.array([N + 3], np.int32)
        cls = np.array([1], np.uint8)
        assert lib.hope_env_set_draw_class(h, ids.ctypes.data, 1, cls.ctypes.data) == EINVAL
    elif case == 'restore_without_pool':
        drawn = np.zeros(N, np.uint8)
        ep = np.zeros(N, np.uint32)
        assert lib.hope_env_restore_maps(h, drawn.ctypes.data, ep.ctypes.data, 0, 0) == ESTATE
        assert lib.hope_env_restore_maps(h, None, ep.ctypes.data, 0, 0) == EINVAL
    elif case == 'debug_geom_bad_arguments':
        a = torch.zeros(4 + 8 * 33, dtype=torch.float64, device='cuda:0')
        o = torch.zeros(2, dtype=torch.int32, device='cuda:0')
        pa, po = C.c_void_p(a.data_ptr()), C.c_void_p(o.data_ptr())
        assert lib.hope_debug_geom(0, -1, 0, pa, po, None) == EINVAL
        assert lib.hope_debug_geom(0, 1, 0, None, po, None) == EINVAL
        assert lib.hope_debug_geom(0, 1, 0, pa, None, None) == EINVAL
        assert lib.hope_debug_geom(10, 1, 0, pa, po, None) == EINVAL and 'unknown fn' in _err()
        assert lib.hope_debug_geom(-1, 1, 0, pa, po, None) == EINVAL
        assert lib.hope_debug_geom(5, 1, 33, pa, po, None) == EINVAL and 'n_obst' in _err()
        assert lib.hope_debug_geom(5, 1, -1, pa, po, None) == EINVAL
        assert lib.hope_debug_geom(5, 0, 32, pa, po, None) == OK                                 # (no case: nothing is launched)
    elif case == 'step_plan_bad_arguments':
        full = L.STEPPLAN_HEAD + 2 * L.STEPPLAN_CHAIN_HEAD + N
        plan = np.full(full, -77, np.int32)
        assert lib.hope_env_step_plan(h, L.STAGE_ALL, 1, None, full) == EINVAL
        assert lib.hope_env_step_plan(h, L.STAGE_ALL, 1, plan.ctypes.data, -1) == EINVAL
        assert lib.hope_env_step_plan(h, L.STAGE_ALL, 1, plan.ctypes.data, N) == EINVAL and 'cap is too small' in _err()
        assert (plan == -77).all()                                                               # a refused call writes nothing
        assert lib.hope_env_step_plan(h, L.STAGE_ALL, 1, plan.ctypes.data, full) == OK
        assert L.STEPPLAN_HEAD + L.STEPPLAN_CHAIN_HEAD + N <= plan[0] <= full and (plan[plan[0]:] == -77).all()
        assert lib.hope_env_step_plan(h, L.STAGE_ALL, 1, plan.ctypes.data, int(plan[0]) - 1) == EINVAL
        assert lib.hope_env_step_plan(h, L.STAGE_ALL, 1, plan.ctypes.data, int(plan[0])) == OK   # exactly the words needed
        fresh = _create()
        assert lib.hope_env_step_plan(fresh, L.STAGE_ALL, 1, plan.ctypes.data, full) == ESTATE and 'set_scenes' in _err()
        assert lib.hope_env_destroy(fresh) == OK

    # ---- the handle still works: its next steps equal a fresh twin's -------------------------------------------------------------
    if case == 'pool_without_class':
        pass                                                   # (the pool stays; plain steps do not draw from it)
    twin = _create()
    o2 = Outs()
    assert _tables(twin) == OK and _set_scenes(twin, arrays) == OK
    # bring both to the same episode state: the abused handle may have stepped (stale_wait_rs_step): restart both
    mask = torch.ones(N, dtype=torch.uint8, device='cuda:0')
    for hh, oo in ((h, outs), (twin, o2)):
        assert lib.hope_env_restart(hh, C.c_void_p(mask.data_ptr()), None) == OK
        assert lib.hope_env_reset_obs(hh, None, L.STAGE_ALL, C.byref(oo.s), None) == OK
        for a in acts:
            assert _step(hh, oo, a) == OK
    torch.cuda.synchronize()
    for k, v in outs.t.items():
        if v is not None:
            assert torch.equal(v, o2.t[k]), (case, k)
    assert lib.hope_env_destroy(twin) == OK
    assert lib.hope_env_destroy(h) == OK


def test_tables_the_mask_stage_cannot_index_are_refused_and_the_handle_keeps_its_tables():
    """hope_env_upload_tables validates before its first copy: a dist_star whose maximum at beam 0 lies below the hull range (the mask
    stage's bin scale would be negative), a NaN and an inf are HOPE_EINVAL with the beam named, nothing is launched on them, and the
    handle's next observation and step equal the oracle's on the tables it had"""
    from hope_amd import tables as T
    from hope_amd.scene_gen import mixed_arrays
    from oracle import oracle as O
    lib = _lib()
    t = T.all_tables()
    start, dest, bbox, verts, nob, nvert = mixed_arrays(N, seed=3, max_obst=MO, levels=('Normal', 'Complex', 'Extrem'))
    arrays = [np.ascontiguousarray(a) for a in (start, dest, bbox, verts, nob.astype(np.int32))]
    h = _create()
    outs = Outs()
    assert _tables(h) == OK and _set_scenes(h, arrays) == OK
    hb = np.ascontiguousarray(t['hull_base'], np.float64)
    ab = np.ascontiguousarray(t['beam_ab'], np.float64)

    def upload(ds, hull=hb):
        ds, hull = np.ascontiguousarray(ds, np.float64), np.ascontiguousarray(hull, np.float64)
        return lib.hope_env_upload_tables(h, ds.ctypes.data, hull.ctypes.data, ab.ctypes.data)

    bad = t['dist_star'].copy()
    bad[:10] = 0.0
    bad[-10:] = 0.0                                            # beam 0's table maximum is 0: below its hull range
    assert upload(bad) == EINVAL and 'beam 0' in _err()
    for v, where in ((np.nan, (770, 5, 3)), (np.inf, (1199, 41, 9))):
        bad = t['dist_star'].copy()
        bad[where] = v
        assert upload(bad) == EINVAL and f'beam {where[0] // 10}' in _err()
    hull = hb.copy()
    hull[64] = np.nan
    assert upload(t['dist_star'], hull) == EINVAL and 'beam 64' in _err()

    O.set_tables(hull_base=t['hull_base'], beam_a=t['beam_ab'][:, 0], beam_b=t['beam_ab'][:, 1], dist_star=t['dist_star'], omp=True)
    orc = O.BatchOracle(N, MO, omp=True, track_traj=False)
    orc.set_scenes(np.arange(N), start, dest, bbox, verts, nvert, nob)
    stages = L.STAGE_MOTION | L.STAGE_OBS | L.STAGE_REWARD
    act = np.random.default_rng(12).integers(-8, 9, (N, 2)) / 8.0                # (float32 holds these exactly)
    want = [{k: v.copy() for k, v in orc.reset_obs(with_rs=False).items()}, {k: v.copy() for k, v in orc.step(act, with_rs=False).items()}]
    assert lib.hope_env_reset_obs(h, None, stages, C.byref(outs.s), None) == OK
    for k, w in enumerate(want):
        if k:
            assert _step(h, outs, torch.from_numpy(act.astype(np.float32)).to('cuda:0'), stages=stages) == OK
        torch.cuda.synchronize()
        assert np.array_equal(outs.t['lidar'].cpu().numpy(), w['lidar'].astype(np.float32)), k
        assert np.array_equal(outs.t['action_mask'].cpu().numpy(), w['mask'].astype(np.float32)), k
        assert np.array_equal(outs.t['status'].cpu().numpy(), w['status']), k
    assert np.array_equal(outs.t['pose'].cpu().numpy(), orc.pose)
    assert lib.hope_env_destroy(h) == OK


def test_destroy_is_idempotent_for_null_and_refuses_a_dead_handle():
    lib = _lib()
    assert lib.hope_env_destroy(None) == OK
    h = _create(n=16, mo=16)
    raw = C.c_void_p(h.value)
    assert lib.hope_env_destroy(h) == OK
    assert lib.hope_env_destroy(raw) == EINVAL and 'live handle' in _err()          # double destroy: refused, nothing touched
    outs = Outs(n=16)
    a = torch.zeros((16, 2), device='cuda:0')
    assert _step(raw, outs, a) == EINVAL and 'live handle' in _err()               # use after destroy: refused


def test_n_obst_download_matches_the_per_scene_download():
    lib = _lib()
    arrays = _scene_arrays()
    h = _create()
    assert _tables(h) == OK and _set_scenes(h, arrays) == OK
    out = np.zeros(N, np.int32)
    assert lib.hope_env_download_n_obst(h, out.ctypes.data) == OK
    assert np.array_equal(out, arrays[4])
    assert lib.hope_env_destroy(h) == OK


@pytest.mark.parametrize('feature', ['planner', 'chooser', 'obsnorm', 'eval'])
def test_enable_disable_enable_starts_from_the_initial_state(feature):
    """the four policy-side features share one "allocate if absent, initialise, free on failure" path: enable, disable, enable again
    -- each round starts from the freshly initialised state whatever the last round left in the memory, and between the rounds the
    feature is off (HOPE_ESTATE, its text)"""
    from hope_amd import tables as T
    lib = _lib()
    n, dev = 64, 'cuda:0'
    h = _create(n=n, mo=16)
    P = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    g = torch.Generator(device=dev).manual_seed(11)
    if feature == 'planner':
        state = np.zeros((L.PLAN_STATE_WORDS, n), np.uint64)
        word = torch.tensor([[1, 0, 2, 0, 0, 3, 1, 0]] * n, dtype=torch.int8, device=dev)       # L S R, three segments, found
        lengths = torch.full((n, 5), 10.0, device=dev)
        enable = lambda r: lib.hope_env_planner_enable(h, 0.0)  # noqa: E731
        disable = lambda: lib.hope_env_planner_disable(h)  # noqa: E731
        probe = lambda: lib.hope_env_planner_download_state(h, state.ctypes.data)  # noqa: E731
        off = 'hope_env_planner_download_state: the planner is off (hope_env_planner_enable first)'

        def fresh(r):
            assert probe() == OK and not state.any()

        def dirty():
            assert lib.hope_env_planner_step(h, P(word), P(lengths), None, L.PLAN_NO_POP, 0, None, None, None, 0, None) == OK, _err()
            assert probe() == OK and state[5].all()                  # every scene replays a path
    elif feature == 'chooser':
        tabs = [np.ascontiguousarray(T.discrete_actions() / [T.VALID_STEER[1], 1.0] * [1.0, sc], dtype=np.float64) for sc in (1.0, 0.5)]
        mean, log_std = torch.zeros((n, 2), device=dev), torch.zeros((1, 2), device=dev)
        mask, action, idx = torch.ones((n, 42), device=dev), torch.zeros((n, 2), device=dev), torch.zeros(n, dtype=torch.int32, device=dev)
        enable = lambda r: lib.hope_env_chooser_enable(h, tabs[r % 2].ctypes.data)  # noqa: E731
        disable = lambda: lib.hope_env_chooser_disable(h)  # noqa: E731
        probe = lambda: lib.hope_env_choose(h, P(mean), P(log_std), 0, 0, P(mask), None, None, None, 7, 1, P(action), None, P(idx), None, None, None)  # noqa: E731
        off = 'hope_env_choose: the chooser is off (hope_env_chooser_enable first)'

        def fresh(r):                                                # the table on the device is this round's: the host twin's choice
            z, o = np.zeros((n, 2), np.float32), np.ones((n, 42), np.float32)
            a, i = np.zeros((n, 2), np.float32), np.zeros(n, np.int32)
            assert lib.hope_chooser_host(n, tabs[r % 2].ctypes.data, z.ctypes.data, z.ctypes.data, 0, 0, o.ctypes.data, 0, None, None, None, 7, 1, 0,
                                         a.ctypes.data, 0, None, i.ctypes.data, None, None) == OK, _err()
            assert probe() == OK, _err()
            torch.cuda.synchronize()
            assert np.array_equal(action.cpu().numpy().view(np.uint32), a.view(np.uint32)) and np.array_equal(idx.cpu().numpy(), i)

        def dirty():
            pass                                                     # (the other round's table is what the memory holds)
    elif feature == 'obsnorm':
        nst = C.c_int64(-1)
        got = [np.full(L.OBSNORM_COLS, np.nan) for _ in range(3)]
        enable = lambda r: lib.hope_env_obsnorm_enable(h)  # noqa: E731
        disable = lambda: lib.hope_env_obsnorm_disable(h)  # noqa: E731
        probe = lambda: lib.hope_env_obsnorm_get(h, C.byref(nst), *[a.ctypes.data for a in got])  # noqa: E731
        off = 'hope_env_obsnorm_get: the normalisation is off (hope_env_obsnorm_enable first)'

        def fresh(r):
            assert probe() == OK and nst.value == 0 and not any(a.any() for a in got)

        def dirty():
            v = np.arange(1.0, 1.0 + L.OBSNORM_COLS)
            assert lib.hope_env_obsnorm_set(h, 5, v.ctypes.data, (2 * v).ctypes.data, (3 * v).ctypes.data) == OK, _err()
            assert probe() == OK and nst.value == 5 and np.array_equal(got[2], 3 * v)
    else:
        state = np.zeros((L.EVAL_STATE_WORDS, n), np.uint64)
        box = np.array([T.VALID_STEER[0], T.VALID_STEER[1], T.VALID_SPEED[0], T.VALID_SPEED[1]], dtype=np.float64)
        target = torch.rand((n, 5), device=dev, generator=g) + 1.0
        pose = torch.rand((n, 3), dtype=torch.float64, device=dev, generator=g) + 1.0
        enable = lambda r: lib.hope_env_eval_enable(h, box.ctypes.data)  # noqa: E731
        disable = lambda: lib.hope_env_eval_disable(h)  # noqa: E731
        probe = lambda: lib.hope_env_eval_download_state(h, state.ctypes.data)  # noqa: E731
        off = 'hope_env_eval_download_state: the evaluation tracker is off (hope_env_eval_enable first)'

        def fresh(r):
            assert probe() == OK and not state.any()

        def dirty():
            assert lib.hope_env_eval_begin(h, P(target), P(pose), None) == OK, _err()
            assert probe() == OK and state[:7].all()                 # previous target and position of every scene
    assert probe() == ESTATE and _err() == off                       # off by default
    for r in range(2):
        assert enable(r) == OK, _err()
        fresh(r)
        dirty()
        assert disable() == OK, _err()
        assert probe() == ESTATE and _err() == off
    assert enable(2) == OK, _err()
    fresh(2)
    assert disable() == OK and disable() == OK                       # (idempotent)
    assert lib.hope_env_destroy(h) == OK


def test_binding_refuses_bad_arguments_by_name():
    """ParkingBatch in front of the ABI: a tensor or array of the wrong dtype, shape or layout is refused by _lib.tensor_arg /
    _lib.array_arg with a HopeError that names the call and the argument, before the library is called -- the step counter and the
    output arena are what they were.  Every bad argument here occupies at least as much memory as the right one (a larger element, one
    element more, one dimension more, a strided view over a larger buffer); too short and wrong device: tests/test_binding_args.py."""
    from hope_amd import ParkingBatch
    from hope_amd.scene_gen import mixed_arrays
    n, mo, t, dev = 64, 16, 5, 'cuda:0'
    start, dest, bbox, verts, nob, _ = mixed_arrays(4 * n, levels=('Normal',), seed=5, max_obst=32)
    keep = np.nonzero(nob <= mo)[0][:n]
    assert len(keep) == n
    arrs = [start[keep], dest[keep], bbox[keep], np.ascontiguousarray(verts[keep][:, :mo]), nob[keep]]
    g = torch.Generator(device=dev).manual_seed(7)
    acts = [torch.rand((n, 2), device=dev, generator=g) * 2 - 1 for _ in range(2)]
    envs = []
    for _ in range(2):
        e = ParkingBatch(n, mo)
        e.set_scene_arrays(np.arange(n), *arrs)
        e.set_pool(tuple(arrs) + (None,))
        e.enable_planner().enable_chooser().enable_obsnorm().enable_gae().enable_eval_tracker()
        e.reset_obs().step(acts[0])
        envs.append(e)
    env, twin = envs

    z = lambda *shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device=dev)  # noqa: E731
    u8, i32, i64, f64 = torch.uint8, torch.int32, torch.int64, torch.float64
    mask, strided = z(n, dtype=u8), z(2 * n, dtype=u8)[::2]
    mean, log_std = z(n, 2), z(1, 2)
    rew = dict(reward=z(n, t), done=z(n, t), value=z(n, t), v_last=z(n), value_target=z(n, t), gamma=0.98, lam=0.95)
    wn = np.ones(4)
    cases = [
        ('hope_env_step', 'actions', lambda: env.step(z(n, 2, dtype=f64))),
        ('hope_env_step', 'actions', lambda: env.step(z(n, 3))),
        ('hope_env_step', 'actions', lambda: env.step(z(2, n).t())),
        ('hope_env_step', 'active', lambda: env.step(acts[1], active=z(n, dtype=i32))),
        ('hope_env_step', 'active', lambda: env.step(acts[1], active=z(n + 1, dtype=u8))),
        ('hope_env_step', 'active', lambda: env.step(acts[1], active=strided)),
        ('hope_env_reset_obs', 'active', lambda: env.reset_obs(active=z(n))),
        ('hope_env_reset_obs', 'active', lambda: env.reset_obs(active=z(n, 1, dtype=u8))),
        ('hope_env_redraw', 'mask', lambda: env.redraw(z(n + 1, dtype=u8))),
        ('hope_env_redraw', 'mask', lambda: env.redraw(strided)),
        ('hope_env_restart', 'mask', lambda: env.restart(strided)),
        ('hope_env_restart', 'mask', lambda: env.restart(z(n, dtype=i64))),
        ('hope_env_map_level', 'out', lambda: env.map_levels(out=z(n, dtype=i32))),
        ('hope_env_map_level', 'active', lambda: env.map_levels(active=z(n + 1, dtype=u8))),
        ('hope_env_map_level', 'detail', lambda: env.map_levels(detail=z(n, 9, dtype=i32))),
        ('hope_env_planner_step', 'rs_word', lambda: env.planner_step(rs_word=z(n, 9, dtype=torch.int8))),
        ('hope_env_planner_step', 'rs_lengths', lambda: env.planner_step(rs_lengths=z(n, 5, dtype=f64))),
        ('hope_env_planner_step', 'done', lambda: env.planner_step(done=z(n + 1, dtype=u8))),
        ('hope_env_planner_step', 'actions', lambda: env.planner_step(actions=z(n, 3))),
        ('hope_env_choose', 'mean', lambda: env.choose_actions(z(n + 1, 2), log_std)),
        ('hope_env_choose', 'log_std', lambda: env.choose_actions(mean, z(n, 2, dtype=f64))),
        ('hope_env_choose', 'mask', lambda: env.choose_actions(mean, log_std, mask=z(n, 43))),
        ('hope_env_choose', 'planned', lambda: env.choose_actions(mean, log_std, planned=z(n, 3, dtype=f64), executing=mask)),
        ('hope_env_choose', 'executing', lambda: env.choose_actions(mean, log_std, planned=z(n, 2, dtype=f64), executing=z(n, dtype=i32))),
        ('hope_env_choose', 'u', lambda: env.choose_actions(mean, log_std, u=z(n + 1, dtype=f64))),
        ('hope_env_obsnorm', 'lidar', lambda: env.obsnorm(lidar=z(n, 121))),
        ('hope_env_obsnorm', 'target', lambda: env.obsnorm(target=z(n, 5, dtype=f64))),
        ('hope_env_obsnorm', 'target', lambda: env.obsnorm(target=z(n + 1, 5))),
        ('hope_env_gae', 'done', lambda: env.gae(**dict(rew, done=z(n, t + 1)))),
        ('hope_env_gae', 'value', lambda: env.gae(**dict(rew, value=z(n, t, dtype=f64)))),
        ('hope_env_gae', 'v_last', lambda: env.gae(**dict(rew, v_last=z(n + 1)))),
        ('hope_env_gae', 'sums', lambda: env.gae(**rew, sums=z(4, dtype=f64))),
        ('hope_env_eval_track', 'target', lambda: env.eval_track(target=z(n, 5, dtype=f64))),
        ('hope_env_eval_track', 'status', lambda: env.eval_track(status=z(n, dtype=i64))),
        ('hope_env_eval_track', 'done', lambda: env.eval_track(done=z(n + 1, dtype=u8))),
        ('hope_env_eval_track', 'rs_word', lambda: env.eval_track(rs_word=z(n, 9, dtype=torch.int8))),
        ('hope_env_set_scenes', 'start', lambda: env.set_scene_arrays(np.arange(n), np.zeros((n, 4)), *arrs[1:])),
        ('hope_env_set_scenes', 'bbox', lambda: env.set_scene_arrays(np.arange(n), arrs[0], arrs[1], np.zeros((n, 5)), arrs[3], arrs[4])),
        ('hope_env_set_scenes', 'verts', lambda: env.set_scene_arrays(np.arange(n), *arrs[:3], np.zeros((n, mo + 1, 4, 2)), arrs[4])),
        ('hope_env_set_scenes', 'n_obst', lambda: env.set_scene_arrays(np.arange(n), *arrs[:4], np.zeros(n + 1, np.int32))),
        ('hope_env_set_pool', 'verts', lambda: env.set_pool((*arrs[:3], np.zeros((n, mo + 1, 4, 2)), arrs[4], None))),
        ('hope_env_set_pool', 'start', lambda: env.set_pool((np.zeros((n + 1, 3)), *arrs[1:], None))),
        ('hope_env_upload_state', 'pose', lambda: env.upload_state(pose=np.zeros((n, 4)))),
        ('hope_env_upload_state', 't', lambda: env.upload_state(t=np.zeros(n + 1, np.int32))),
        ('hope_env_upload_state', 'accum', lambda: env.upload_state(accum=np.zeros((n, 2)))),
        ('hope_env_restore_maps', 'pool_index', lambda: env.restore_maps(np.zeros(n + 1, np.int32), np.zeros(n, np.uint32), seed=1)),
        ('hope_env_restore_maps', 'episode', lambda: env.restore_maps(np.zeros(n, np.int32), np.zeros(n + 1, np.uint32), seed=1)),
        ('hope_env_curriculum_set_windows', 'win_s', lambda: env.curriculum_set_windows(wn, np.ones(5), wn, wn)),
        ('hope_env_curriculum_set_windows', 'successes', lambda: env.curriculum_set_windows(wn, wn, wn, np.ones((4, 2)))),
    ]
    for call, arg, bad in cases:
        torch.cuda.synchronize()
        before = (env.last_step(), env._arena.clone())
        with pytest.raises(L.HopeError, match=f'^{call}: {arg} must be '):
            bad()
        torch.cuda.synchronize()
        assert env.last_step() == before[0] and torch.equal(env._arena, before[1]), (call, arg)
    env.step(acts[1])
    twin.step(acts[1])
    torch.cuda.synchronize()
    assert env.last_step() == twin.last_step() and torch.equal(env._arena, twin._arena)
    assert int(env.status.min()) >= 1 and bool(torch.isfinite(env.lidar).all())
    env.close()
    twin.close()
