"""Shared inputs of the planner tests (test_planner_core.py, test_gpu_planner.py): a scripted sequence of search results and
episode ends, and helpers that drive hope_planner_step_host.  Test infrastructure only."""
import ctypes as C

import numpy as np

N_SCENES, N_STEPS, SEED = 193, 60, 20240611
STEP_RATIO = 1.25


def make_script(n=N_SCENES, steps=N_STEPS, seed=SEED):
    """-> dict of numpy arrays: word int8 [T,n,8], lengths float64 [T,n,5], done uint8 [T,n], forced bool [T], base float64 [T,n,2].
    Per scene and step a word is offered with probability 0.3 (one, three or five segments of random type; lengths up to 6 m, so at
    most 5 actions per segment and 25 per path -- far below the torch class's 96; one offer in eight is a word of sub-millimetre
    segments that expands to nothing), an episode ends with probability 0.04, every seventh step is forced.  `base` are the
    policy's actions that the planner overrides."""
    rng = np.random.default_rng(seed)
    word = np.full((steps, n, 8), -1, np.int8)
    word[:, :, 7] = 0
    lengths = np.zeros((steps, n, 5))
    nseg = rng.choice([1, 3, 5], size=(steps, n))
    types = rng.integers(0, 3, size=(steps, n, 5)).astype(np.int8)
    mag = rng.uniform(0.05, 6.0, size=(steps, n, 5))
    # some exact multiples of a step and sub-threshold lengths among them
    special = rng.random((steps, n, 5))
    mag = np.where(special < 0.06, 1.25 * rng.integers(1, 5, size=mag.shape), mag)
    mag = np.where((special >= 0.06) & (special < 0.10), 1e-3, mag)
    sign = np.where(rng.random((steps, n, 5)) < 0.5, -1.0, 1.0)
    empty = rng.random((steps, n)) < 0.125
    mag = np.where(empty[:, :, None], 1e-4, mag)
    used = np.arange(5)[None, None, :] < nseg[:, :, None]
    word[:, :, :5] = np.where(used, types, -1)
    word[:, :, 5] = nseg
    word[:, :, 6] = rng.random((steps, n)) < 0.3
    lengths[:] = np.where(used, mag * sign, 0.0)
    done = (rng.random((steps, n)) < 0.04).astype(np.uint8)
    forced = (np.arange(steps) % 7) == 6
    base = rng.uniform(-1, 1, size=(steps, n, 2))
    return {'word': word, 'lengths': lengths, 'done': done, 'forced': forced, 'base': base}


def torch_reference(script, lengths_dtype=np.float64):
    """the script through agent_glue.BatchedRsPlanner in HopeRollout._plan's order -> executing bool [T,n], planned f64 [T,n,2],
    and the counts (adoptions, refusals while busy, resets in mid-replay)"""
    import torch
    from hope_amd.agent_glue import BatchedRsPlanner
    T, n = script['done'].shape
    pl = BatchedRsPlanner(n, step_ratio=STEP_RATIO)
    ex_all, planned_all = np.zeros((T, n), bool), np.zeros((T, n, 2))
    adopted = refused = mid = 0
    for t in range(T):
        done = torch.from_numpy(script['done'][t]).bool()
        word = torch.from_numpy(script['word'][t])
        lens = torch.from_numpy(script['lengths'][t].astype(lengths_dtype))
        mid += int((done & pl.executing).sum())
        pl.reset(done)
        busy = pl.executing.clone()
        forced = bool(script['forced'][t])
        take = pl.set_paths(word, lens, forced=forced)
        adopted += int(take.sum())
        if not forced:
            refused += int(((word[:, 6] > 0) & busy).sum())
        a, ex = pl.get_actions()
        ex_all[t], planned_all[t] = ex.numpy(), a.numpy()
    return ex_all, planned_all, (adopted, refused, mid)


class HostPlanner:
    """hope_planner_step_host with its state block"""

    def __init__(self, n, step_ratio=STEP_RATIO):
        from hope_amd import _lib as L
        self.L, self.lib, self.n, self.step_ratio = L, L.load_library(), n, step_ratio
        self.state = np.zeros((L.PLAN_STATE_WORDS, n), np.uint64)

    def step(self, word, lengths, done=None, flags=0, actions=None):
        """-> (planned f64 [n,2], executing u8 [n]); actions (float32 / float64 [n,2]) are overridden in place"""
        n = self.n
        word = np.ascontiguousarray(word, dtype=np.int8)
        assert lengths.dtype in (np.float32, np.float64) and word.shape == (n, 8) and lengths.shape == (n, 5)
        lengths = np.ascontiguousarray(lengths)
        planned, ex = np.full((n, 2), np.nan), np.full(n, 255, np.uint8)
        dp = None
        if done is not None:
            done = np.ascontiguousarray(done, dtype=np.uint8)
            dp = done.ctypes.data
        ap, af64 = None, 0
        if actions is not None:
            assert actions.flags.c_contiguous and actions.dtype in (np.float32, np.float64)
            ap, af64 = actions.ctypes.data, int(actions.dtype == np.float64)
        self.L.check(self.lib.hope_planner_step_host(n, self.step_ratio, self.state.ctypes.data, word.ctypes.data, lengths.ctypes.data,
                                                     int(lengths.dtype == np.float64), dp, flags, planned.ctypes.data, ex.ctypes.data, ap, af64),
                     'hope_planner_step_host')
        return planned, ex

    @property
    def busy(self):
        return ((self.state[5] >> np.uint64(13)) & np.uint64(1)).astype(bool)


def expand_all(words5, lengths, max_steps=1 << 20):
    """every path of (words int8 [M,5], lengths [M,5]) replayed to its end by the host twin -> list of [k_i, 2] arrays"""
    m = len(words5)
    word = np.full((m, 8), -1, np.int8)
    word[:, :5] = words5
    word[:, 5] = (words5 >= 0).sum(1)
    word[:, 6] = 1
    word[:, 7] = 0
    hp = HostPlanner(m)
    none = np.zeros((m, 8), np.int8)
    out = [[] for _ in range(m)]
    w = word
    for _ in range(max_steps):
        planned, ex = hp.step(w, lengths)
        w = none
        idx = np.nonzero(ex)[0]
        if len(idx) == 0:
            break
        for i in idx:
            out[i].append(planned[i].copy())
        assert (planned[ex == 0] == 0).all()
    assert not hp.busy.any() and not hp.state.any()
    return [np.array(o).reshape(-1, 2) for o in out]


def as_c_void(a):
    return C.c_void_p(a.ctypes.data)
