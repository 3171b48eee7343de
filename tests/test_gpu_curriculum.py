"""The device side of the map curriculum (include/hope_env.h "curriculum for new-map draws") on the MI355X: the tally is exact, the
weighted lists equal the host twin's byte for byte, every kernel that draws a map follows them, off means off, a refill and a
snapshot behave, and the oracle still agrees with a step on curriculum-drawn maps.

Statistical bounds are derived, not tuned: a share over m draws with probability p may deviate by 5 sigma = 5 sqrt(p (1 - p) / m)
plus the list's quantisation 1 / 2^20."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

LEVELS = ('Normal', 'Complex', 'Extrem')
OUT_NAMES = ('lidar', 'action_mask', 'target', 'reward', 'reward_info', 'status', 'done', 'pose', 'rs_word', 'rs_lengths')
BIG = 10 ** 6


def make_env(n, mo=128, seed=3, unique=256, dlp_every=0, pool=0, pool_seed=11, **kw):
    from hope_amd import ParkingBatch
    from hope_amd.scene_gen import mixed_arrays
    init = mixed_arrays(unique, levels=LEVELS, seed=seed, max_obst=mo)
    env = ParkingBatch(n, mo, obs_dtype=torch.float64, action_dtype=torch.float64, **kw)
    sl = np.arange(n) % unique
    env.set_scene_arrays(np.arange(n), init[0][sl], init[1][sl], init[2][sl], init[3][sl], init[4][sl])
    if dlp_every:
        env.set_draw_class(np.arange(dlp_every - 1, n, dlp_every), 1)         # every dlp_every-th slot is a Dragon-Lake slot
        env.set_dlp_cases()
    if pool:
        env.generate_pool(pool, LEVELS, seed=pool_seed)
    return env


LEVELS_B = ('Normal', 'Extrem')                  # a pool split of other labels: entry k of it is another level than entry k of LEVELS


def level_of(idx, pool, levels=LEVELS):
    from hope_amd.scene_gen import pool_level_counts
    edges = np.cumsum(pool_level_counts(pool, levels))
    return np.searchsorted(edges, idx, side='right')


def bucket_of(idx, pool, levels=LEVELS):
    """bucket of a pool_index value on a generated pool: level, 4 + case, or 255 for a map set_scenes uploaded"""
    idx = np.asarray(idx)
    out = np.full(idx.shape, 255, np.int64)
    out[idx >= 0] = level_of(idx[idx >= 0], pool, levels)
    out[idx <= -2] = 4 + (-2 - idx[idx <= -2])
    return out


def hand_windows(nb, type_s=(240, 240, 20, 245), failing_cases=(3, 17, 101, 200)):
    wn = np.r_[np.full(4, 250.0), np.full(nb - 4, 10.0)]
    ws = np.r_[np.array(type_s, float), np.full(nb - 4, 10.0)]
    for c in failing_cases:
        if 4 + c < nb:
            ws[4 + c] = 0.0
    return wn, ws, np.full(nb, BIG, np.uint64), np.full(nb, BIG // 2, np.uint64)


def within_5_sigma(count, m, p):
    return abs(count / m - p) <= 5.0 * np.sqrt(p * (1.0 - p) / m) + 2.0 ** -20


def host_lists(env, pool, st, levels=LEVELS, **kw):
    from hope_amd import curriculum as cu
    from hope_amd.scene_gen import pool_level_counts
    labels = np.repeat(np.arange(3), pool_level_counts(pool, levels)).astype(np.uint8)
    return cu.lists_host(np.full(pool, 7), labels, getattr(env, 'n_dlp_cases', 0), env.max_obst, st['episodes'], st['win_n'], st['win_s'], **kw)


def test_tally_is_exact_and_lists_equal_the_host_twin():
    """4 096 mixed scenes (every 4th a Dragon-Lake slot), generated pool, fused turnover on new maps for 320 steps: the per-bucket
    counters equal a numpy recount from each step's status / done and the bucket of the map every scene held BEFORE the step
    (from the pool_index downloaded then and the labels of the pool it was drawn from).  In the middle a relaxed refill with ANOTHER
    level split (entry k changes its label), and later a strict refill issued BETWEEN a step and its tally: the tally must read the
    labels of the set that step drew from, not of the set resident by then.  One more tally on hand-made status / done buffers
    exercises the success counters.  Then update:
    windows == the window rule on the counters, device lists == hope_curriculum_lists_host byte for byte; again after more steps."""
    from hope_amd import curriculum as cu
    n, P = 4096, 900
    env = make_env(n, dlp_every=4, pool=P)
    lib = env.lib
    keep = (np.arange(n) % 8 != 0)                                      # an eighth of the scenes keeps its uploaded (unlabelled) map
    env.redraw(torch.from_numpy(keep.astype(np.uint8)).to(env.device), seed=5)
    env.set_redraw_seed(99)
    env.reset_obs()
    env.upload_state(t=np.random.default_rng(1).integers(150, 200, n))
    env.enable_curriculum()
    nb = 4 + env.n_dlp_cases
    e_ref, s_ref = np.zeros(nb + 1, np.int64), np.zeros(nb + 1, np.int64)
    torch.cuda.synchronize()
    held = bucket_of(env.pool_index(), P)                              # bucket of the map every scene holds
    layout = [LEVELS]                                                   # level split of the pool set the next step draws from

    def recount(b, status, done):
        b = np.where(b == 255, nb, b)
        fin = done != 0
        ok = fin & (status == 2)
        np.add.at(e_ref, b[fin], 1); np.add.at(s_ref, b[ok], 1)
        np.add.at(e_ref, 3, int((fin & (b >= 4) & (b < nb)).sum())); np.add.at(s_ref, 3, int((ok & (b >= 4) & (b < nb)).sum()))

    g = torch.Generator(device='cuda').manual_seed(4)

    def run(steps, refill_at=-1, strict_at=-1):
        for it in range(steps):
            if it == refill_at:
                env.generate_pool(P, LEVELS_B, seed=12, batch=1, relaxed=True)
                env.pool_generation()                                   # (waits for the generator and applies the swap: from this step on)
                layout[0] = LEVELS_B
            act = torch.rand((n, 2), device='cuda', generator=g, dtype=torch.float64) * 2 - 1
            env.step(act, auto_reset=True, fresh=True)
            drew_from = layout[0]
            if it == strict_at:                                         # a swap between the step and its tally
                env.generate_pool(P, LEVELS, seed=13, batch=2)
                layout[0] = LEVELS
            env.curriculum_tally()
            torch.cuda.synchronize()
            status, done = env.status.cpu().numpy(), env.done.cpu().numpy()
            recount(held, status, done)
            fin = done != 0
            held[fin] = bucket_of(env.pool_index()[fin], P, drew_from)   # the map a finished scene drew in this step

    def check_counters():
        st = env.curriculum_state()
        print('episodes per type', e_ref[:4], 'unlabelled', e_ref[nb], 'successes', s_ref[:4], 'total', e_ref[:3].sum() + e_ref[3] + e_ref[nb])
        assert np.array_equal(st['episodes'].astype(np.int64), e_ref[:nb]) and np.array_equal(st['successes'].astype(np.int64), s_ref[:nb])
        assert st['unlabelled_episodes'] == e_ref[nb] and st['unlabelled_successes'] == s_ref[nb]
        return st

    run(320, refill_at=150, strict_at=230)
    assert e_ref[:3].sum() + e_ref[3] + e_ref[nb] >= 1000 and (e_ref[:4] > 0).all() and e_ref[nb] > 0      # not "nothing counted"
    assert (e_ref[4:nb] > 0).sum() > 50
    check_counters()
    # hand-made outcome buffers: many arrivals, so that the success counters are exercised whatever the random policy achieved
    rng = np.random.default_rng(2)
    status = rng.integers(1, 6, n).astype(np.int32)
    done = ((status != 1) & (rng.random(n) < 0.7)).astype(np.uint8)
    ts, td = torch.from_numpy(status).to(env.device), torch.from_numpy(done).to(env.device)
    rc = lib.hope_env_curriculum_tally(env.h, C.c_void_p(ts.data_ptr()), C.c_void_p(td.data_ptr()), env._stream())
    assert rc == 0
    recount(held, status, done)
    assert s_ref[:4].min() > 0
    st0 = check_counters()
    assert st0['updates'] == 0 and np.all(st0['win_n'] == 0)

    def check_update(st_before, folded_e, folded_s):
        env.curriculum_update()
        st = env.curriculum_state()
        for b in range(nb):                                             # the window rule on what was tallied since the last update
            W = 250.0 if b < 4 else 10.0
            exp = cu.fold_host(st_before['win_n'][b], st_before['win_s'][b], float(st['episodes'][b] - folded_e[b]),
                               float(st['successes'][b] - folded_s[b]), W)
            assert (st['win_n'][b], st['win_s'][b]) == exp, b
        l0, l1, pos = env.curriculum_lists()
        h = host_lists(env, P, st)
        assert np.array_equal(st['prob'], h['prob']) and np.array_equal(st['pw'], h['pw'])
        assert np.array_equal(pos, h['positions'])
        assert l0.tobytes() == h['list0'].tobytes() and l1.tobytes() == h['list1'].tobytes()
        assert st['episodes'][3] >= 500 and st['prob'][4:].std() > 0                    # past the case horizon: a real reweighting
        return st

    st1 = check_update(st0, np.zeros(nb, np.uint64), np.zeros(nb, np.uint64))
    assert st1['updates'] == 1
    run(40)
    st2 = check_counters()
    st3 = check_update(st2, st1['episodes'], st1['successes'])
    assert st3['updates'] == 2 and not np.array_equal(st3['win_s'], st1['win_s'])
    assert env.pool_overflow() == 0
    env.close()


@pytest.mark.parametrize('form', ['one_launch', 'pair', 'redraw'])
def test_every_draw_follows_the_weighted_lists(form):
    """Hand-set windows (Extrem failing, four cases failing); every scene of a 16 384-scene handle takes a new map -- inside the
    one-launch step kernel, inside the two-launch form (pair kernels for the small-tile class; HOPE_SPLIT_MIN as
    tests/test_gpu_parity.py forces it) or through hope_env_redraw: every pool_index equals list[key % 2^20] of the scene's class
    (exact), and the share of every level and case lies within 5 sigma of its probability."""
    from hope_amd import curriculum as cu
    n, P, seed = 16384, 3000, 4242
    if form == 'pair':
        os.environ['HOPE_SPLIT_MIN'] = '1'                   # two-launch form: pair kernels for the small-tile class
    elif form == 'one_launch':
        os.environ['HOPE_SPLIT_MIN'] = '1000000000'
    try:
        env = make_env(n, dlp_every=4, pool=P)
        env.enable_curriculum()
        nb = 4 + env.n_dlp_cases
        wn, ws, e, s = hand_windows(nb)
        env.curriculum_set_windows(wn, ws, e, s)
        st = env.curriculum_state()
        l0, l1, pos = env.curriculum_lists()
        h = host_lists(env, P, st)
        assert l0.tobytes() == h['list0'].tobytes() and l1.tobytes() == h['list1'].tobytes()
        q, pc = st['prob'][:4], st['prob'][4:]
        assert q[2] > 0.4 and np.abs(q - cu.type_q(wn[:4], ws[:4])).max() < 1e-15
        env.reset_obs()
        _, ep = env.pool_state()
        if form == 'redraw':
            env.redraw(torch.ones(n, dtype=torch.uint8, device=env.device), seed=seed)
        else:
            env.set_redraw_seed(seed)
            env.upload_state(t=np.full(n, 1000, np.int32))              # out of time: every scene turns over in this step
            g = torch.Generator(device='cuda').manual_seed(1)
            env.step(torch.rand((n, 2), device='cuda', generator=g, dtype=torch.float64) * 2 - 1, auto_reset=True, fresh=True)
        torch.cuda.synchronize()
        if form != 'redraw':
            assert env.done.cpu().numpy().all()
        idx, ep1 = env.pool_state()
        assert np.array_equal(ep1, ep + 1)
        key = cu.draw_key(seed, np.arange(n), ep)
        large = np.arange(n) % 4 == 3
        pos_in_list = (key % np.uint64(1 << 20)).astype(np.int64)
        expect = np.where(large, l1[pos_in_list], l0[pos_in_list])
        assert np.array_equal(idx, expect)
        lev = level_of(idx[~large], P)
        m0 = int((~large).sum())
        for l in range(3):
            assert within_5_sigma((lev == l).sum(), m0, q[l] / q[:3].sum()), (l, (lev == l).mean(), q)
        assert (lev == 2).mean() > 0.5                                   # Extrem is failing: it gets more than half of the draws
        cases = -2 - idx[large]
        m1 = int(large.sum())
        cnt = np.bincount(cases, minlength=nb - 4)
        for c in range(nb - 4):
            assert within_5_sigma(cnt[c], m1, pc[c]), (c, cnt[c] / m1, pc[c])
        failing = np.array([3, 17, 101, 200])
        assert cnt[failing].sum() / m1 > 5 * len(failing) / (nb - 4)     # p of a failing case is ~100 x that of a solved one
        assert env.pool_overflow() == 0
        env.close()
    finally:
        os.environ.pop('HOPE_SPLIT_MIN', None)


def test_off_means_off():
    """enable -> tally -> update -> disable leaves no trace: 100 steps with turnover on new maps equal those of a handle that
    never heard of the curriculum, output for output and pool_index for pool_index"""
    n, P = 2048, 600
    a, b = make_env(n, dlp_every=4, pool=P), make_env(n, dlp_every=4, pool=P)
    a.enable_curriculum()
    nb = 4 + a.n_dlp_cases
    a.curriculum_set_windows(*hand_windows(nb))
    a.curriculum_update()
    assert a.curriculum_state()['on']
    a.disable_curriculum()
    assert not a.curriculum_state()['on'] and a.pool_generation() == b.pool_generation()
    t0 = np.random.default_rng(3).integers(150, 200, n)
    for e in (a, b):
        e.set_redraw_seed(31)
        e.reset_obs()
        e.upload_state(t=t0)
    g = torch.Generator(device='cuda').manual_seed(2)
    turned = 0
    for it in range(100):
        act = torch.rand((n, 2), device='cuda', generator=g, dtype=torch.float64) * 2 - 1
        a.step(act, auto_reset=True, fresh=True)
        b.step(act, auto_reset=True, fresh=True)
        if it % 10 == 9:
            torch.cuda.synchronize()
            turned += int(a.done.sum().item())
            for k in OUT_NAMES:
                assert torch.equal(getattr(a, k), getattr(b, k)), (it, k)
            assert np.array_equal(a.pool_index(), b.pool_index())
    assert turned > 100
    assert all(np.array_equal(x, y) for x, y in zip(a.download_state(), b.download_state()))
    a.close(); b.close()


@pytest.mark.parametrize('relaxed', [False, True])
def test_refill_keeps_the_weights_and_a_snapshot_knows_them(relaxed):
    """generate_pool under an active curriculum: the next redraw still follows q (no silent fall-back to uniform).  A snapshot
    carries the generation of the weighted lists: restore_maps repeats the draws under the same weights and refuses after an update
    that changed them."""
    from hope_amd import _lib as L
    n, P = 8192, 1200
    env = make_env(n, pool=P)
    env.enable_curriculum()
    wn, ws, e, s = hand_windows(4)
    env.curriculum_set_windows(wn, ws, e, s)
    q = env.curriculum_state()['q']
    env.generate_pool(P, LEVELS, seed=11, batch=1, relaxed=relaxed)
    ones = torch.ones(n, dtype=torch.uint8, device=env.device)
    env.redraw(ones, seed=8)                                             # (relaxed: draws from whichever set is active, weighted either way)
    torch.cuda.synchronize()
    gen = env.pool_generation()                                          # (applies a pending relaxed swap)
    env.redraw(ones, seed=9)
    torch.cuda.synchronize()
    idx, ep = env.pool_state()
    lev = level_of(idx, P)
    for l in range(3):
        assert within_5_sigma((lev == l).sum(), n, q[l] / q[:3].sum()), (l, (lev == l).mean(), q)
    assert (lev == 2).mean() > 0.5
    maps = env.download_scenes(np.arange(256))
    env.redraw(ones, seed=9)
    torch.cuda.synchronize()
    assert not np.array_equal(env.pool_index(), idx)
    env.restore_maps(idx, ep, seed=9, generation=gen)                    # same pool, same weights: the same maps again
    torch.cuda.synchronize()
    back = env.download_scenes(np.arange(256))
    assert np.array_equal(env.pool_index(), idx) and all(np.array_equal(x, y) for x, y in zip(maps[:3], back[:3]))
    # an update that changes the weights: Normal fails now
    status = torch.full((n,), 3, dtype=torch.int32, device=env.device)
    done = torch.from_numpy((level_of(idx, P) == 0).astype(np.uint8)).to(env.device)
    L.check(env.lib.hope_env_curriculum_tally(env.h, C.c_void_p(status.data_ptr()), C.c_void_p(done.data_ptr()), env._stream()), 'tally')
    env.curriculum_update()
    assert env.curriculum_state()['q'][0] > q[0] and env.pool_generation() != gen
    with pytest.raises(L.HopeError, match='replaced'):
        env.restore_maps(idx, ep, seed=9, generation=gen)
    env.close()


def test_host_labelled_pool_equals_the_host_twin():
    """a pool uploaded from the host and labelled with set_pool_buckets (shuffled labels, some unlabelled, a few large lots)"""
    from hope_amd import curriculum as cu
    from hope_amd.scene_gen import mixed_arrays
    n, mo, P = 512, 128, 400
    env = make_env(n, dlp_every=4)
    pool = mixed_arrays(P, levels=('Normal', 'Complex', 'Extrem', 'dlp'), seed=9, max_obst=mo)
    env.set_pool(pool)
    rng = np.random.default_rng(4)
    labels = rng.choice([0, 1, 2, 255], P, p=[0.3, 0.3, 0.3, 0.1]).astype(np.uint8)
    env.enable_curriculum()
    env.set_pool_buckets(labels)
    nb = 4 + env.n_dlp_cases
    env.curriculum_set_windows(*hand_windows(nb))
    st = env.curriculum_state()
    l0, l1, pos = env.curriculum_lists()
    h = cu.lists_host(pool[4], labels, env.n_dlp_cases, mo, st['episodes'], st['win_n'], st['win_s'])
    assert np.array_equal(pos, h['positions']) and l0.tobytes() == h['list0'].tobytes() and l1.tobytes() == h['list1'].tobytes()
    assert (pool[4][l0] <= 32).all() and (pool[4][l1[l1 >= 0]] > 32).all() and (l1 < 0).any() and (l1 >= 0).any()
    # a tally sees the host's labels
    env.redraw(torch.ones(n, dtype=torch.uint8, device=env.device), seed=3)
    status = torch.full((n,), 2, dtype=torch.int32, device=env.device)
    done = torch.ones(n, dtype=torch.uint8, device=env.device)
    idx = env.pool_index()
    from hope_amd import _lib as L
    env.curriculum_tally()                                               # (notes the buckets of the maps just drawn; done is all 0)
    L.check(env.lib.hope_env_curriculum_tally(env.h, C.c_void_p(status.data_ptr()), C.c_void_p(done.data_ptr()), env._stream()), 'tally')
    st1 = env.curriculum_state()
    de, ds = st1['episodes'] - st['episodes'], st1['successes'] - st['successes']          # (set_windows set the counters)
    b = np.where(idx >= 0, labels[np.maximum(idx, 0)], 4 + (-2 - idx))
    for l in range(3):
        assert de[l] == ds[l] == (b == l).sum() and de[l] > 0
    assert st1['unlabelled_episodes'] == (b == 255).sum() > 0 and de[3] == (idx <= -2).sum() > 0
    env.close()


def test_oracle_agrees_on_curriculum_drawn_maps():
    """the step's outputs do not depend on how a map was chosen: 1 024 scenes redraw from weighted lists after an update; the
    oracle, given the downloaded maps, equals the reset observation and one further step exactly (float64, tolerance 0.0)"""
    from oracle import oracle as O
    n, mo, P = 1024, 128, 500
    env = make_env(n, pool=P)
    env.enable_curriculum()
    env.curriculum_set_windows(*hand_windows(4))
    env.curriculum_update()
    env.redraw(torch.ones(n, dtype=torch.uint8, device=env.device), seed=21)
    torch.cuda.synchronize()
    idx = env.pool_index()
    assert (level_of(idx, P) == 2).mean() > 0.5
    got = env.download_scenes(np.arange(n))
    t = env.tables
    O.set_tables(hull_base=t['hull_base'], beam_a=t['beam_ab'][:, 0], beam_b=t['beam_ab'][:, 1], dist_star=t['dist_star'])
    orc = O.BatchOracle(n, mo, omp=True)
    used = np.arange(mo)[None, :] < got[4][:, None]
    verts = np.where(used[:, :, None, None], got[3], 0.0)
    orc.set_scenes(np.arange(n), got[0], got[1], got[2], verts, np.full((n, mo), 4, np.int32), got[4])
    env.reset_obs()
    o = orc.reset_obs(with_rs=True)
    rng = np.random.default_rng(5)
    for it in range(2):
        torch.cuda.synchronize()
        assert np.array_equal(env.status.cpu().numpy(), o['status'])
        assert np.array_equal(env.action_mask.cpu().numpy(), o['mask'])
        for k in ('lidar', 'target', 'reward'):
            assert np.abs(getattr(env, k).cpu().numpy() - o[k]).max() <= 0.0, (it, k)
        w = env.rs_word.cpu().numpy()
        assert np.array_equal(w[:, 6], o['rs_found']) and np.array_equal(w[:, :5], o['rs_ctypes'])
        act = rng.uniform(-1, 1, (n, 2))
        env.step(torch.from_numpy(act).to(env.device))
        o = orc.step(act, with_rs=True)
    env.close()


def test_bucket_follows_the_map_not_the_resident_pool():
    """A finished scene that restarts on the SAME map (no new-map bit) keeps its bucket although the pool has been replaced by one
    with other labels in the meantime; a map uploaded with set_scenes is unlabelled from then on."""
    n, P = 1024, 600
    env = make_env(n, pool=P)
    env.redraw(torch.ones(n, dtype=torch.uint8, device=env.device), seed=2)
    env.enable_curriculum()
    env.reset_obs()
    torch.cuda.synchronize()
    b0 = bucket_of(env.pool_index(), P)
    env.generate_pool(P, LEVELS_B, seed=5, batch=1)                      # entry k is another level now
    assert (bucket_of(env.pool_index(), P, LEVELS_B) != b0).mean() > 0.3
    g = torch.Generator(device='cuda').manual_seed(1)

    def all_finish():
        env.upload_state(t=np.full(n, 1000, np.int32))
        env.step(torch.rand((n, 2), device='cuda', generator=g, dtype=torch.float64) * 2 - 1, auto_reset=True)
        env.curriculum_tally()
        torch.cuda.synchronize()
        assert env.done.cpu().numpy().all()
        return env.curriculum_state()

    for k in (1, 2):
        st = all_finish()
        assert np.array_equal(st['episodes'][:3].astype(np.int64), k * np.bincount(b0, minlength=3)) and st['unlabelled_episodes'] == 0
    from hope_amd.scene_gen import mixed_arrays
    init = mixed_arrays(n // 2, levels=LEVELS, seed=8, max_obst=env.max_obst)
    ids = np.arange(0, n, 2)
    env.set_scene_arrays(ids, *[a for a in init[:5]])
    env.reset_obs()
    st = all_finish()
    kept = np.bincount(b0[1::2], minlength=3)
    assert np.array_equal(st['episodes'][:3].astype(np.int64), 2 * np.bincount(b0, minlength=3) + kept) and st['unlabelled_episodes'] == n // 2
    env.close()


def test_misuse_returns_the_documented_codes():
    from hope_amd import _lib as L
    n, P = 256, 120
    env = make_env(n)
    lib = env.lib
    st, dn = C.c_void_p(env.status.data_ptr()), C.c_void_p(env.done.data_ptr())
    assert lib.hope_env_curriculum_enable(env.h, None) == -5 and b'no scene pool' in lib.hope_last_error()      # HOPE_ESTATE
    env.generate_pool(P, LEVELS, seed=1)
    assert lib.hope_env_curriculum_tally(env.h, st, dn, None) == -5 and b'off' in lib.hope_last_error()
    assert lib.hope_env_curriculum_update(env.h, None) == -5
    lab = np.zeros(P + 1, np.uint8)
    assert lib.hope_env_set_pool_buckets(env.h, P + 1, lab.ctypes.data) == -1 and b'labels for a resident pool' in lib.hope_last_error()
    lab[5] = 3
    assert lib.hope_env_set_pool_buckets(env.h, P, lab.ctypes.data) == -1 and b'out of range' in lib.hope_last_error()
    bad = L.CurriculumParams(type_window=0.0)
    assert lib.hope_env_curriculum_enable(env.h, C.byref(bad)) == -1
    env.enable_curriculum()
    assert lib.hope_env_curriculum_tally(env.h, None, dn, None) == -1
    w = np.zeros(5)
    e = np.zeros(5, np.uint64)
    assert lib.hope_env_curriculum_set_windows(env.h, 5, w.ctypes.data, w.ctypes.data, e.ctypes.data, e.ctypes.data) == -1
    assert lib.hope_env_set_dlp_cases(env.h, 0, None, None, None, None, 0, None, None) == -5
    env.curriculum_tally().curriculum_update()                           # and the handle still works
    assert env.curriculum_state()['updates'] == 1
    env.disable_curriculum()
    env.set_dlp_cases(False)
    env.close()
