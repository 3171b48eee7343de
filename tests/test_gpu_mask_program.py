"""-m gpu: the action-mask stage on the programmed scans of tests/mask_program.py -- table entries and their 1e-9 bands, bin edges of
the count-interval table, 0 .. 120 active beams in every visit order, second-visit truncation, the post_process corners, hull
contacts with the 119 -> 0 wrap -- against the oracle with tolerance 0, in every launch form.

The lots (<= 32 obstacles: two per wave of k_obs_pair, in the wave layout mask_program builds) and their twins with fillers (> 32
obstacles: the one-scene stage of k_env_step) share one handle of max_obstacles 128; HOPE_CLS1_FRAC = 0 while the handle is filled
keeps the tail of the small-tile list out of the large-tile chain.  The premise -- which lot reaches which branch -- is asserted on
the CPU by tests/test_mask_program.py and re-evaluated here on the oracle's lidar of every compared observation.  A mismatch is
reported as (family, tag, scene, action or beam, got, want); the mirror (mask_program.kernel_mask_trace) then names the beam, the
table word and the bound."""
import functools
import os

import numpy as np
import pytest

import lidar_adversarial as A
import mask_program as M

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

MO = 128
CONTINUE = 1
OBS = ('lidar', 'action_mask', 'status')


def _stages():
    from hope_amd import _lib as L
    return L.STAGE_MOTION | L.STAGE_OBS | L.STAGE_REWARD


def _snap(orc, o):
    return dict(lidar=o['lidar'].copy(), action_mask=o['mask'].copy(), status=o['status'].copy(), pose=orc.pose.copy())


def _floors_hold(census):
    cats, pairs, waves = census
    return (all(cats.get(c, 0) >= f for c, f in M.FLOORS.items()) and all(pairs.get(g, 0) >= f for g, f in M.PAIR_FLOORS.items())
            and all(waves.get(k, 0) >= M.WAVE_FLOOR for k in M.PAIR_KINDS))


@functools.lru_cache(maxsize=None)
def reference(name):
    """the lots of one table set, then their twins; the oracle's reset observation, zero-action step and moving step on them, once"""
    from oracle import oracle as O
    P = M.program(name)
    lots = P.lots + P.twins
    n, n_small = len(lots), len(P.lots)
    assert n <= 4096 and n_small % 2 == 1
    sc = A.arrays(lots, MO)
    sc['n_small'] = n_small
    with M.oracle_tables(P.tables):
        orc = O.BatchOracle(n, MO, omp=True, track_traj=False)
        orc.set_scenes(np.arange(n), sc['start'], sc['dest'], sc['bbox'], sc['verts'], sc['nvert'], sc['nob'])
        ref = [_snap(orc, orc.reset_obs(with_rs=False))]
        zero = np.zeros((n, 2))
        free = ref[0]['status'] == CONTINUE
        k = np.arange(n) % n_small                                       # a lot and its twin move alike
        move = np.where(free[:, None], np.stack([((k * 37) % 101 - 50) / 100.0, ((k * 53) % 97 - 48) / 96.0], axis=1), 0.0)
        ref.append(_snap(orc, orc.step(zero, with_rs=False)))
        ref.append(_snap(orc, orc.step(move, with_rs=False)))
    assert np.array_equal(ref[0]['lidar'][:n_small], np.array([f['raw'] for f in P.info]))        # the scans the CPU premises were computed on
    assert np.array_equal(ref[1]['pose'], sc['start']) and np.array_equal(ref[1]['lidar'], ref[0]['lidar'])
    for k, r in enumerate(ref):
        assert np.array_equal(r['lidar'][:n_small], r['lidar'][n_small:]) and np.array_equal(r['action_mask'][:n_small], r['action_mask'][n_small:]), k
    # the premises on the lidar of the compared observations: reset_obs and the zero-action step give, bit for bit (asserted above), the
    # scans the categories were computed from, so the census of those scans is theirs; the moving step programs nothing
    census = M.census(P)
    held = sum(census[0].get(c, 0) >= f for c, f in M.FLOORS.items())
    print(f'{name}, reset_obs and zero-action step: {held} of {len(M.FLOORS)} programmed categories at their floor; ties '
          f'{census[0].get("tie", 0)}, straddle pairs {sum(census[1].values())}, waves {census[2]}')
    assert _floors_hold(census), census
    moved = [M.kernel_mask_trace(P.L, np.clip(row, 0, 10) + P.L['hb']) for row in ref[2]['lidar'][:n_small]]
    print(f'{name}, moving step: {sum(len(t["act"]) > 0 for t in moved)} lots with an active beam, {sum(bool(t["walks"]) for t in moved)} with a '
          f'second visit, {sum(t["tie"] for t in moved)} with a tie')
    assert (np.abs(ref[2]['pose'] - ref[1]['pose']).max(axis=1) > 0).sum() >= 0.3 * n                # the moving step moves
    return P, lots, sc, (zero, move), ref


class _Env:
    """HOPE_SPLIT_MIN for the life of the handle; HOPE_CLS1_FRAC = 0 while it is filled"""

    def __init__(self, split):
        self.split = split

    def __enter__(self):
        self.before = {k: os.environ.get(k) for k in ('HOPE_SPLIT_MIN', 'HOPE_CLS1_FRAC')}
        os.environ['HOPE_SPLIT_MIN'] = self.split
        return self

    def make(self, P, sc, rows=None, dtype=None):
        from hope_amd import ParkingBatch
        rows = np.arange(len(sc['nob'])) if rows is None else rows
        n = len(rows)
        os.environ['HOPE_CLS1_FRAC'] = '0'
        try:
            env = ParkingBatch(n, MO, obs_dtype=dtype or torch.float64, action_dtype=torch.float64, overlap=True, tables=P.tables)
            env.set_scene_arrays(np.arange(n), sc['start'][rows], sc['dest'][rows], sc['bbox'][rows], sc['verts'][rows], sc['nob'][rows])
        finally:
            self._restore('HOPE_CLS1_FRAC')
        return env

    def _restore(self, k):
        if self.before[k] is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = self.before[k]

    def __exit__(self, *exc):
        self._restore('HOPE_SPLIT_MIN')
        self._restore('HOPE_CLS1_FRAC')


def _mismatches(lots, rows, got, want):
    g, w = got.reshape(len(got), -1), want.reshape(len(got), -1)
    bad = np.argwhere(g != w)
    return [(lots[rows[i]].fam, lots[rows[i]].tag, int(i), int(j), g[i, j], w[i, j]) for i, j in bad[:6]]


def _check(env, lots, rows, ref, tag, cast=None):
    torch.cuda.synchronize()
    for k in OBS:
        got = getattr(env, k).cpu().numpy()
        want = ref[k][rows] if cast is None or k == 'status' else ref[k][rows].astype(cast)
        n_bad = int((got != want).sum())
        assert n_bad == 0, (tag, k, n_bad) + tuple(_mismatches(lots, rows, got, want))
    if cast is None:
        assert np.array_equal(env.download_state()[0], ref['pose'][rows]), tag


def _run(env, lots, rows, acts, ref, tag, cast=None, extra=0):
    env.reset_obs(stages=_stages() | extra)
    _check(env, lots, rows, ref[0], (tag, 'reset_obs'), cast)
    for a, r, name in zip(acts, ref[1:], ('zero-action step', 'moving step')):
        env.step(torch.from_numpy(a[rows]).to(env.device), stages=_stages() | extra)
        _check(env, lots, rows, r, (tag, name), cast)


def _padded_rows(n):
    """the handle padded past 4 096 scenes by repeating lots: k_kinematics runs on its own in the one-launch form"""
    return np.concatenate([np.arange(n), np.arange(4200 - n) % n])


FORMS = {'pair_and_split_kernels': ('1', False), 'one_launch_fused_kinematics': ('1000000000', False),
         'one_launch_separate_kinematics': ('1000000000', True)}


@pytest.mark.parametrize('form', list(FORMS))
def test_programmed_scans_equal_the_oracle_in_every_launch_form(form):
    """lidar, action mask, status and pose with tolerance 0 on reset_obs, a zero-action step (the pose stays the start pose: the
    programmed scans are read again by the step's observation launch) and one moving step"""
    P, lots, sc, acts, ref = reference('shipped')
    split, padded = FORMS[form]
    rows = _padded_rows(len(lots)) if padded else np.arange(len(lots))
    assert (len(rows) > 4096) == padded
    with _Env(split) as e:
        env = e.make(P, sc, rows)
        _run(env, lots, rows, acts, ref, form)
        env.close()
    print(f'{form}: {len(rows)} scenes ({sc["n_small"]} lots, as many twins), 0 mismatches on 3 observations')


def test_pair_kernels_equal_the_one_scene_kernels_on_programmed_scans():
    """HOPE_SPLIT_MIN = 1 with and without STAGE_ONE_SCENE: every output and the state bit for bit, and the oracle's observations"""
    from hope_amd import _lib as L
    P, lots, sc, acts, ref = reference('shipped')
    rows = np.arange(len(lots))
    with _Env('1') as e:
        envs = [e.make(P, sc) for _ in range(2)]
        extras = (0, L.STAGE_ONE_SCENE)
        for env, extra in zip(envs, extras):
            env.reset_obs(stages=_stages() | extra)
        for step, a in enumerate((None,) + acts):
            if a is not None:
                for env, extra in zip(envs, extras):
                    env.step(torch.from_numpy(a).to(env.device), stages=_stages() | extra)
            torch.cuda.synchronize()
            for k in ('lidar', 'action_mask', 'status', 'done', 'pose', 'reward', 'reward_info', 'target'):
                u, v = getattr(envs[0], k).cpu().numpy(), getattr(envs[1], k).cpu().numpy()
                assert np.array_equal(u, v), (step, k) + tuple(_mismatches(lots, rows, u, v))
            for u, v in zip(envs[0].download_state(), envs[1].download_state()):
                assert np.array_equal(u, v), step
            _check(envs[1], lots, rows, ref[step], ('one-scene kernels', step))
        for env in envs:
            env.close()


def test_float32_masks_are_the_rounded_float64_ones():
    """float32 observations, pair form: mask == float32(oracle mask) and lidar == float32(oracle lidar)"""
    P, lots, sc, acts, ref = reference('shipped')
    with _Env('1') as e:
        env = e.make(P, sc, dtype=torch.float32)
        _run(env, lots, np.arange(len(lots)), acts, ref, 'float32', cast=np.float32)
        env.close()


@pytest.mark.parametrize('form', ['pair_and_split_kernels', 'one_launch_fused_kinematics'])
def test_another_table_set_through_the_public_upload(form):
    """the coarse rows on a 0.05 m grid (bins of up to ten equal entries), uploaded through ParkingBatch(tables=...) and injected into
    the oracle, the lots programmed anew against this table's entries and bin edges"""
    P, lots, sc, acts, ref = reference('quantised')
    with _Env(FORMS[form][0]) as e:
        env = e.make(P, sc)
        assert env.tables is P.tables
        _run(env, lots, np.arange(len(lots)), acts, ref, ('quantised', form))
        env.close()
