"""Batched counterparts of the agent-side glue that sits right after the env step.
Plain torch tensor code (any device); no custom kernels -- these are a few elementwise ops per step.

  BatchedRsPlanner     <-> RsPlanner                 src/model/agent/parking_agent.py:2-47
  mask_action_probs /
  choose_action        <-> ActionMask.choose_action  src/model/action_mask.py:199-227
  BatchedStateNorm     <-> StateNorm                 src/model/state_norm.py:7-46
  DeviceStateNorm      <-> the same through the library's kernels (hope_env_obsnorm) or their host twin
  DeviceEvalTracker    <-> eval()'s per-episode tally   src/evaluation/eval_utils.py:35-57 (hope_env_eval_* or their host twins)
  batched_gae          <-> PPO.update's GAE loop    src/model/agent/ppo_agent.py:258-273
  DevicePpoBatch       <-> PPO.update's minibatch loop around the forwards   src/model/agent/ppo_agent.py:278-336 (hope_env_ppo_* or
                                                     their host twins)
  DeviceSacUpdate      <-> SACAgent.update between its forwards   src/model/agent/sac_agent.py:250-337 (hope_env_sac_* or their host twins)
  DeviceActor          <-> the actor's inference forward   src/model/network.py:34-187 (hope_env_policy_forward or its host twin)
  DeviceAdam /
  DevicePolyak         <-> the optimiser steps and AgentBase._soft_update   src/model/agent/sac_agent.py:293-331, ppo_agent.py:337-340,
                                                     agent_base.py:64 (hope_env_optim_adam / _polyak or their host twins)
  RolloutStorage       <-> ReplayMemory              src/model/replay_memory.py:6-49
"""
import ctypes as C
import math
from functools import partial

import numpy as np
import torch

from . import _lib as L
from . import tables as T

STEP_RATIO = 0.05 * 10 * 2.5            # kinetic_model.step_len * n_step * VALID_SPEED[1] (train_HOPE_sac.py:164)


class BatchedRsPlanner:
    """Open-loop replay of a found Reeds-Shepp path as unit actions [steer in {1,0,-1}, signed fraction of a full
    1.25 m step], one queue per scene.  Expansion rule = RsPlanner.set_rs_path (:12-41), including its quirks: a
    segment of exactly +-1 step or of |step| <= 1e-3 is dropped; a longer one becomes ceil(|x|)-1 unit actions plus
    the remainder."""

    def __init__(self, n, device='cpu', step_ratio=STEP_RATIO, max_actions=96):
        self.n, self.step_ratio, self.tmax = n, step_ratio, max_actions
        self.device = torch.device(device)
        self.actions = torch.zeros((n, max_actions, 2), dtype=torch.float64, device=self.device)
        self.length = torch.zeros(n, dtype=torch.int64, device=self.device)
        self.cursor = torch.zeros(n, dtype=torch.int64, device=self.device)

    @property
    def executing(self):
        """bool [N]: scenes currently replaying a path (ParkingAgent.executing_rs)."""
        return self.cursor < self.length

    def reset(self, mask=None):
        if mask is None:
            self.length.zero_(); self.cursor.zero_()
        else:
            self.length[mask] = 0; self.cursor[mask] = 0

    @staticmethod
    def expand(rs_word, rs_lengths, step_ratio=STEP_RATIO, max_actions=96):
        """rs_word int8 [N,8] (types S=0 L=1 R=2, -1 unused; [5]=n_seg), rs_lengths [N,5] metres ->
        (actions [N,max_actions,2] float64, count [N])."""
        n = rs_word.shape[0]
        dev = rs_word.device
        types = rs_word[:, :5].to(torch.int64)
        used = types >= 0
        steer = torch.where(types == 1, 1.0, torch.where(types == 2, -1.0, 0.0)).to(torch.float64)   # L:1 S:0 R:-1
        # a python-float divisor makes the GPU kernel multiply by the reciprocal (not correctly rounded): divide by a
        # device tensor so that x equals the reference's `length / step_ratio` bit for bit on every device
        x = rs_lengths.to(torch.float64) / torch.full((1,), float(step_ratio), dtype=torch.float64, device=dev)
        ax = x.abs()
        k = torch.where(ax > 1, torch.ceil(ax) - 1, torch.zeros_like(ax))             # unit actions
        rem = torch.where(ax > 1, torch.sign(x) * (ax - k), x)
        keep_rem = (ax != 1) & (rem.abs() > 1e-3) & used
        k = torch.where(used, k, torch.zeros_like(k)).to(torch.int64)
        cnt = k + keep_rem.to(torch.int64)                                            # [N,5]
        off = torch.cumsum(cnt, dim=1) - cnt
        total = cnt.sum(dim=1)
        t = torch.arange(max_actions, device=dev).view(1, -1, 1)                      # [1,T,1]
        rel = t - off.unsqueeze(1)                                                    # [N,T,5]
        inseg = (rel >= 0) & (rel < cnt.unsqueeze(1))
        unit = inseg & (rel < k.unsqueeze(1))
        val = torch.where(unit, torch.sign(x).unsqueeze(1).expand(-1, max_actions, -1), rem.unsqueeze(1).expand(-1, max_actions, -1))
        a_step = (val * inseg).sum(dim=2)
        a_steer = (steer.unsqueeze(1) * inseg).sum(dim=2)
        actions = torch.stack([a_steer, a_step], dim=2)
        return actions, torch.clamp(total, max=max_actions)

    def set_paths(self, rs_word, rs_lengths, forced=False):
        """ParkingAgent.set_planner_path (:65-69): adopt a newly found path unless one is being replayed."""
        found = rs_word[:, 6] > 0
        take = found if forced else (found & ~self.executing)
        if bool(take.any()):
            acts, cnt = self.expand(rs_word[take], rs_lengths[take], self.step_ratio, self.tmax)
            self.actions[take] = acts
            self.length[take] = cnt
            self.cursor[take] = 0
        return take

    def get_actions(self):
        """pop the next planned action of every executing scene -> ([N,2] actions, bool [N] which rows are valid)."""
        ex = self.executing
        idx = torch.clamp(self.cursor, max=self.tmax - 1)
        a = self.actions[torch.arange(self.n, device=self.device), idx]
        self.cursor = torch.where(ex, self.cursor + 1, self.cursor)
        done = ex & (self.cursor >= self.length)
        self.length[done] = 0
        self.cursor[done] = 0
        return a, ex


def _host_library(device, method):
    """the library for a host twin: its loops run over CPU tensors only"""
    if device.type != 'cpu':
        raise L.HopeError(f'an env without {method} must hold CPU tensors, not {device}')
    return L.load_library()


class DeviceRsPlanner:
    """BatchedRsPlanner's surface over the library's planner (include/hope_env.h "replay of found Reeds-Shepp paths"): the
    state lives in the env's handle (48 B per scene), one k_plan launch per call, no host synchronisation, no cap on the number
    of actions.  `step(done, rs_word, rs_lengths)` fuses reset(done) + set_paths + get_actions -- what a rollout does between
    two env steps.  Rows of `planned` that are not executing are 0 (the torch class leaves stale values there).
    On an env without the library (CPU tensors; tests/fake_env.OracleEnv) the same step runs on the host through
    hope_planner_step_host: the rule is one source for both."""

    def __init__(self, env, step_ratio=STEP_RATIO):
        self.env, self.n, self.step_ratio = env, env.n, float(step_ratio)
        self.device = torch.device(env.device)
        self.on_device = hasattr(env, 'planner_step')
        if self.on_device:
            env.enable_planner(self.step_ratio)
            self._zero_word = torch.zeros((self.n, 8), dtype=torch.int8, device=self.device)
            self._lens = torch.zeros((self.n, 5), dtype=env.obs_dtype, device=self.device)
        else:
            self._lib = _host_library(self.device, 'planner_step')
            self._state = np.zeros((L.PLAN_STATE_WORDS, self.n), np.uint64)
            self._planned = torch.zeros((self.n, 2), dtype=torch.float64)
            self._exec = torch.zeros(self.n, dtype=torch.uint8)
            self._zero_word = torch.zeros((self.n, 8), dtype=torch.int8)
            self._lens = torch.zeros((self.n, 5), dtype=torch.float32)

    @property
    def executing(self):
        """bool [N]: scenes currently replaying a path.  Downloads the state: host-synchronous (statistics, tests)."""
        st = self.env.planner_state() if self.on_device else self._state
        busy = ((st[5] >> 13) & 1).astype('uint8')
        return torch.from_numpy(busy).to(self.device).bool()

    def _host_step(self, word, lens, done, flags, step=None):
        n, arg = self.n, partial(L.tensor_arg, 'hope_planner_step_host', device=self.device)
        word, lens = word.contiguous(), lens.contiguous()
        done = None if done is None else done.to(torch.uint8).contiguous()
        wp, lp = arg('rs_word', word, torch.int8, (n, 8)), arg('rs_lengths', lens, (torch.float32, torch.float64), (n, 5))
        dp = arg('done', done, torch.uint8, (n,), optional=True)
        pp, ep = arg('planned', self._planned, torch.float64, (n, 2)), arg('executing', self._exec, torch.uint8, (n,))
        L.check(self._lib.hope_planner_step_host(n, self.step_ratio, self._state.ctypes, wp, lp, int(lens.dtype == torch.float64), dp, flags,
                                                 pp, ep, None, 0), 'hope_planner_step_host')
        return self._planned, self._exec.view(torch.bool)

    def reset(self, mask=None):
        if self.on_device:
            self.env.planner_reset(None if mask is None else mask.to(torch.uint8).contiguous())
        elif mask is None:
            self._state[:] = 0
        else:
            self._state[:, mask.bool().numpy()] = 0

    def set_paths(self, rs_word, rs_lengths, forced=False):
        """adopt newly found paths (idle scenes, or all with forced); nothing is popped.  Returns None: which scenes took a path is
        known on the device only."""
        if self.on_device:
            self.env.planner_step(forced=forced, step=0, rs_word=rs_word, rs_lengths=rs_lengths, done=None, pop=False)
        else:
            self._host_step(rs_word, rs_lengths, None, (L.PLAN_FORCED if forced else 0) | L.PLAN_NO_POP)

    def get_actions(self):
        """pop the next planned action of every executing scene -> ([N,2] float64 actions, bool [N] which rows are valid)"""
        if self.on_device:
            return self.env.planner_step(step=0, rs_word=self._zero_word, rs_lengths=self._lens, done=None)
        return self._host_step(self._zero_word, self._lens, None, 0)

    def step(self, done=None, rs_word=None, rs_lengths=None, forced=False, step=None):
        """reset(done) + set_paths(rs_word, rs_lengths, forced) + get_actions() in one call.  On the device the arguments default to
        the env's own outputs of its last step, and step = env.last_step() of that step makes the call wait for its search."""
        if self.on_device:
            return self.env.planner_step(forced=forced, step=step, rs_word=rs_word, rs_lengths=rs_lengths,
                                         done=True if done is None else done.to(torch.uint8))
        env = self.env
        return self._host_step(env.rs_word if rs_word is None else rs_word, env.rs_lengths if rs_lengths is None else rs_lengths,
                               env.done if done is None else done, L.PLAN_FORCED if forced else 0)


class DeviceActionChooser:
    """The block of `_AgentCommon.act` from choose_action to gaussian_log_prob as ONE k_choose launch (include/hope_env.h "masked
    choice of the discrete action"; rule: csrc/hope_chooser_core.h): mask-weighted draw, cast, clamp, the planner's override and the
    log-probability of the action taken.  Draws are counter-based, keyed by (seed, call number, scene): this object keeps the
    counter, so a run is reproduced by its seed and resumed by restoring `counter`.  They are NOT torch.multinomial's stream.
    On an env without the library (CPU tensors; tests/fake_env.OracleEnv) the same choice runs on the host through
    hope_chooser_host: the rule is one source for both."""

    def __init__(self, env, seed=0):
        self.env, self.n, self.seed, self.counter = env, env.n, int(seed) & (2 ** 64 - 1), 0
        self.device = torch.device(env.device)
        self.on_device = hasattr(env, 'choose_actions')
        self.action_env = None                        # the last choice in the env's action dtype: what env.step takes
        if self.on_device:
            env.enable_chooser()
        else:
            self._lib = _host_library(self.device, 'choose_actions')
            self._acts = L.array_arg('hope_chooser_host', 'actions', T.discrete_actions() / [T.VALID_STEER[1], 1.0], np.float64, (L.N_ACTION, 2))
            self._adt = getattr(env, 'action_dtype', torch.float32)
            self._a32 = torch.zeros((self.n, 2), dtype=torch.float32)
            self._a = self._a32 if self._adt == torch.float32 else torch.zeros((self.n, 2), dtype=torch.float64)
            self._idx = torch.zeros(self.n, dtype=torch.int32)
            self._lp = torch.zeros((self.n, 2), dtype=torch.float32)

    def _host(self, mean, log_std, mask, planned, executing, u):
        n, arg = self.n, partial(L.tensor_arg, 'hope_chooser_host', device=self.device)
        mean = mean.contiguous()
        mp = arg('mean', mean, (torch.float32, torch.float64), (n, 2))
        log_std = log_std.to(mean.dtype).contiguous()
        one_row = n > 1 and tuple(log_std.shape) == (1, 2)
        sp = arg('log_std', log_std, mean.dtype, (1, 2) if one_row else (n, 2))
        if mask.dtype not in (torch.float32, torch.float64):
            mask = mask.to(torch.float32)
        mask = mask.contiguous()
        kp = arg('mask', mask, (torch.float32, torch.float64), (n, L.N_ACTION))
        if (planned is None) != (executing is None):
            raise L.HopeError('hope_chooser_host: planned and executing go together')
        planned = None if planned is None else planned.to(torch.float64).contiguous()
        executing = None if executing is None else executing.to(torch.uint8).contiguous()
        u = None if u is None else u.to(torch.float64).contiguous()
        pp, ep = arg('planned', planned, torch.float64, (n, 2), optional=True), arg('executing', executing, torch.uint8, (n,), optional=True)
        up = arg('u', u, torch.float64, (n,), optional=True)
        ap, fp = arg('action', self._a, self._adt, (n, 2)), arg('action_f32', self._a32, torch.float32, (n, 2))
        ip, lp = arg('idx', self._idx, torch.int32, (n,)), arg('log_prob', self._lp, torch.float32, (n, 2))
        L.check(self._lib.hope_chooser_host(n, self._acts.ctypes, mp, sp, 0 if one_row or n == 1 else 2, int(mean.dtype == torch.float64), kp,
                                            int(mask.dtype == torch.float64), pp, ep, up, self.seed, self.counter, 0, ap,
                                            int(self._adt == torch.float64), fp, ip, lp, None), 'hope_chooser_host')
        return self._a, self._a32, self._idx, self._lp

    def choose(self, mean, log_std, mask, planned=None, executing=None, u=None):
        """mean [N, 2]; log_std [N, 2] or the agents' [1, 2] parameter (an expanded view of it is taken back to one row); mask
        [N, 42]; planned / executing: the planner's outputs or None.  -> (action_f32 [N, 2], log_prob f32 [N, 2], action of the env's
        action dtype): persistent tensors, overwritten by the next call.  Advances the counter."""
        if log_std.dim() == 2 and log_std.shape[0] == self.n and self.n > 1 and log_std.stride(0) == 0:
            log_std = log_std[:1]
        if self.on_device:
            env = self.env
            mean = mean.contiguous()
            log_std = log_std.to(mean.dtype).contiguous()
            if mask.dtype != env.obs_dtype:
                mask = mask.to(env.obs_dtype)
            if planned is not None and planned.dtype != torch.float64:
                planned = planned.to(torch.float64)
            a, a32, self.idx, lp = env.choose_actions(mean, log_std, mask.contiguous(), None if planned is None else planned.contiguous(),
                                                      None if executing is None else executing.contiguous(), u, self.seed, self.counter)
        else:
            a, a32, self.idx, lp = self._host(mean, log_std, mask, planned, executing, u)
        self.counter += 1
        self.action_env = a
        return a32, lp, a


def make_chooser(chooser, env, seed=0):
    """the loops' `chooser` argument: None (today's torch path), 'device', or a DeviceActionChooser"""
    if chooser is None or isinstance(chooser, DeviceActionChooser):
        return chooser
    if chooser == 'device':
        return DeviceActionChooser(env, seed)
    raise ValueError(f"chooser must be None, 'device' or a DeviceActionChooser, not {chooser!r}")


class DeviceEvalTracker:
    """The bookkeeping of the reference's eval() (src/evaluation/eval_utils.py:35-57) over the library's tracker (include/hope_env.h
    "bookkeeping of an evaluation run"; rule: csrc/hope_evaltrack_core.h): the stuck detector and its random action, step count,
    summed reward, path length, final status, the alive mask and the hiding of frozen slots' Reeds-Shepp words, as one launch before
    and one after the env step, with no host synchronisation.  The stuck detector's draws are counter-based, keyed by (seed, episode
    step, scene, dimension): this object keeps the step counter; `evaluate.stuck_uniforms` restates them.
    On an env without the library (CPU tensors; tests/fake_env.OracleEnv) the same operations run on the host through
    hope_eval_begin_host / hope_eval_override_host / hope_eval_track_host: the rule is one source for both.

    alive: uint8 [N], the episodes still running as of the last `override` (what env.step takes as `active`); word: int8 [N, 8] and
    done: uint8 [N], the planner's inputs as of the last `track`.  Persistent tensors."""

    def __init__(self, env, seed=0):
        self.env, self.n, self.seed, self.counter = env, env.n, int(seed) & (2 ** 64 - 1), 0
        self.device = torch.device(env.device)
        self.on_device = hasattr(env, 'eval_track')
        if self.on_device:
            env.enable_eval_tracker()
            self.alive, self.word, self.done = env.eval_alive, env.eval_word, env.eval_done
        else:
            self._lib = _host_library(self.device, 'eval_track')
            self._state = np.zeros((L.EVAL_STATE_WORDS, self.n), np.uint64)
            self._box = L.array_arg('hope_eval_override_host', 'box', T.VALID_STEER + T.VALID_SPEED, np.float64, (4,))
            self.alive = torch.zeros(self.n, dtype=torch.uint8)
            self.word = torch.zeros((self.n, 8), dtype=torch.int8)
            self.done = torch.zeros(self.n, dtype=torch.uint8)

    def _obs(self, t):
        """the tensor as contiguous float32 / float64"""
        if t.dtype not in (torch.float32, torch.float64):
            t = t.to(torch.float32)
        return t.contiguous()

    def begin(self):
        """a new episode in every scene, from the env's first observation; the step counter restarts"""
        env, n = self.env, self.n
        if self.on_device:
            env.eval_begin()
        else:
            target, pose = self._obs(env.target), env.pose.to(torch.float64).contiguous()
            tp = L.tensor_arg('hope_eval_begin_host', 'target', target, (torch.float32, torch.float64), (n, 5), self.device)
            pp = L.tensor_arg('hope_eval_begin_host', 'pose', pose, torch.float64, (n, 3), self.device)
            L.check(self._lib.hope_eval_begin_host(n, n, self._state.ctypes, tp, int(target.dtype == torch.float64), pp), 'hope_eval_begin_host')
        self.counter = 0                              # (after the call: a refused begin leaves the object as it was)
        self.alive.fill_(1)
        self.done.zero_()

    def override(self, action, u=None):
        """the stuck detector's random action, in place on `action` ([N, 2] float32 / float64, contiguous); -> `alive`.  Advances the
        step counter."""
        if self.on_device:
            self.env.eval_override(action, u, self.seed, self.counter)
        else:
            n, arg = self.n, partial(L.tensor_arg, 'hope_eval_override_host', device=self.device)
            ap = arg('action', action, (torch.float32, torch.float64), (n, 2))
            u = None if u is None else u.to(torch.float64).contiguous()
            up, lp = arg('u', u, torch.float64, (n, 2), optional=True), arg('alive', self.alive, torch.uint8, (n,))
            L.check(self._lib.hope_eval_override_host(n, n, self._state.ctypes, self._box.ctypes, ap, int(action.dtype == torch.float64), up,
                                                      self.seed, self.counter, 0, lp), 'hope_eval_override_host')
        self.counter += 1
        return self.alive

    def track(self):
        """the tally of the env step just taken; -> (word, done)"""
        if self.on_device:
            self.env.eval_track()
            return self.word, self.done
        env, n, arg = self.env, self.n, partial(L.tensor_arg, 'hope_eval_track_host', device=self.device)
        target, pose = self._obs(env.target), env.pose.to(torch.float64).contiguous()
        reward = env.reward.to(target.dtype).contiguous()
        status, done, word = env.status.to(torch.int32).contiguous(), env.done.to(torch.uint8).contiguous(), env.rs_word.contiguous()
        tp, pp = arg('target', target, (torch.float32, torch.float64), (n, 5)), arg('pose', pose, torch.float64, (n, 3))
        rp, sp = arg('reward', reward, target.dtype, (n,)), arg('status', status, torch.int32, (n,))
        dp, wp = arg('done', done, torch.uint8, (n,)), arg('rs_word', word, torch.int8, (n, 8))
        ow, od = arg('word', self.word, torch.int8, (n, 8)), arg('done_out', self.done, torch.uint8, (n,))
        L.check(self._lib.hope_eval_track_host(n, n, self._state.ctypes, tp, int(target.dtype == torch.float64), pp, rp, sp, dp, wp, ow, od),
                'hope_eval_track_host')
        return self.word, self.done

    def any_alive(self):
        """is an episode still running, as of the last call of any kind?  alive (of the last override) and not done (of the track
        behind it) is alive after that track.  Host-synchronous: the evaluator asks every poll_every steps."""
        return bool((self.alive & (self.done ^ 1)).any())

    def state(self):
        """numpy uint64 [10, N]: the state planes (host-synchronous on the device)"""
        return self.env.eval_state() if self.on_device else self._state

    def records(self):
        """-> float32 [N, 4]: status, steps, summed reward, path length"""
        if self.on_device:
            return self.env.eval_records()
        st = self._state
        w = st[9]
        with np.errstate(invalid='ignore', over='ignore'):
            rec = np.stack([((w >> np.uint64(32)) & np.uint64(0xFF)).astype(np.float32), (w & np.uint64(0xFFFFFFFF)).astype(np.float32),
                            st[7].view(np.float64).astype(np.float32), st[8].view(np.float64).astype(np.float32)], axis=1)
        return torch.from_numpy(rec)


def make_tracker(tracker, env, seed=0):
    """the evaluator's `tracker` argument: None (the torch bookkeeping), 'device', or a DeviceEvalTracker"""
    if tracker is None or isinstance(tracker, DeviceEvalTracker):
        return tracker
    if tracker == 'device':
        return DeviceEvalTracker(env, seed)
    raise ValueError(f"tracker must be None, 'device' or a DeviceEvalTracker, not {tracker!r}")


_ACTIONS = None


def _scaled_actions(device, dtype):
    global _ACTIONS
    if _ACTIONS is None:
        _ACTIONS = torch.from_numpy(T.discrete_actions() / [T.VALID_STEER[1], 1.0])      # action_mask.py:217-221
    return _ACTIONS.to(device=device, dtype=dtype)


def mask_action_probs(action_mean, action_std, action_mask):
    """ActionMask.choose_action (:212-224) for a batch: probability of each of the 42 discrete actions under the
    Gaussian policy head, re-weighted by the action mask.  mean/std [N,2], mask [N,42] -> [N,42]."""
    mean, std = action_mean.to(torch.float64), action_std.to(torch.float64)
    acts = _scaled_actions(mean.device, torch.float64)                                     # [42,2]
    z = (acts.unsqueeze(0) - mean.unsqueeze(1)) / std.unsqueeze(1)
    logp = -0.5 * z ** 2 - torch.log(math.sqrt(2 * math.pi) * std).unsqueeze(1)
    prob = torch.clamp(logp, -10, 10).sum(dim=2)
    e = torch.exp(prob) * action_mask.to(torch.float64)
    return e / e.sum(dim=1, keepdim=True)


def choose_action(action_mean, action_std, action_mask, generator=None):
    """sample one discrete action per scene -> [N,2] in the policy's [-1,1] scaling (action_mask.py:225-227)."""
    p = mask_action_probs(action_mean, action_std, action_mask)
    idx = torch.multinomial(p, 1, generator=generator).squeeze(1)
    return _scaled_actions(p.device, torch.float64)[idx], idx


class BatchedStateNorm:
    """StateNorm (state_norm.py:7-46) for batches: running mean / std of the 'lidar' and 'target' observations
    (DEFAULT_UPDATE_MODAL).  The reference folds observations in one at a time (Welford); `update` folds a whole
    batch with the parallel-merge form of the same recurrence, and keeps the reference's first-sample quirk
    (mean = std = first observation)."""

    def __init__(self, shapes=None, update_modal=('lidar', 'target'), device='cpu'):
        shapes = shapes or {'lidar': 120, 'target': 5, 'action_mask': 42}
        self.modal = tuple(update_modal)
        self.n_state = 0
        self.fixed = False
        dev = torch.device(device)
        self.mean = {k: torch.zeros(shapes[k], dtype=torch.float64, device=dev) for k in self.modal}
        self.S = {k: torch.zeros(shapes[k], dtype=torch.float64, device=dev) for k in self.modal}
        self.std = {k: torch.zeros(shapes[k], dtype=torch.float64, device=dev) for k in self.modal}

    def fix_parameters(self):
        self.fixed = True

    def normalize(self, obs):
        return {k: ((v.to(torch.float64) - self.mean[k]) / (self.std[k] + 1e-8) if k in self.modal else v) for k, v in obs.items()}

    def update(self, obs):
        """fold obs[k] of shape [B, dim] into the running statistics (no-op when fixed)."""
        if self.fixed:
            return
        b = next(iter(obs.values())).shape[0]
        start = 0
        if self.n_state == 0:                                   # first sample: mean = std = observation (:27-31)
            for k in self.modal:
                self.mean[k] = obs[k][0].to(torch.float64).clone()
                self.std[k] = obs[k][0].to(torch.float64).clone()
            self.n_state = 1
            start = 1
        m = b - start
        if m <= 0:
            return
        n0 = self.n_state
        for k in self.modal:
            x = obs[k][start:].to(torch.float64)
            bm = x.mean(dim=0)
            bS = ((x - bm) ** 2).sum(dim=0)
            delta = bm - self.mean[k]
            self.mean[k] = self.mean[k] + delta * (m / (n0 + m))
            self.S[k] = self.S[k] + bS + delta ** 2 * (n0 * m / (n0 + m))
            self.std[k] = torch.sqrt(self.S[k] / (n0 + m))
        self.n_state = n0 + m


class DeviceStateNorm:
    """BatchedStateNorm's surface over the library's observation normalisation (include/hope_env.h "normalisation of the
    observations"; rule: csrc/hope_obsnorm_core.h), so that it can stand in as `agent.state_norm`: the statistics live in the env's
    handle (one set per env), `update` is two launches (k_obsnorm_partial, k_obsnorm_merge), `normalize` one (k_obsnorm_apply), and
    `update_and_normalize(obs)` fuses the two -- what a rollout does with an observation between two env steps.  The arithmetic
    order of the fold is fixed, so the statistics do not depend on the launch geometry; they differ from BatchedStateNorm's in the
    last bits only.  `normalize` returns lidar / target as float32 -- what the agents cast to anyway -- in persistent tensors that
    the next normalising call overwrites; other keys pass through.  Both modalities go together and hold at most env.n rows.
    `mean` / `S` / `std` download the statistics on access (host-synchronous).  `fixed` is host-side: update is then a no-op.
    On an env without the library (CPU tensors; tests/fake_env.OracleEnv) the same runs on the host through hope_obsnorm_host: the
    rule is one source for both.
    from_norm: a BatchedStateNorm (e.g. from checkpoint.load_hope_checkpoint) or DeviceStateNorm whose statistics and `fixed` are
    taken over; to_batched() goes the other way, for saving."""

    modal = ('lidar', 'target')

    def __init__(self, env, from_norm=None):
        self.env, self.n, self.fixed = env, env.n, False
        self.device = torch.device(env.device)
        self.on_device = hasattr(env, 'obsnorm')
        if self.on_device:
            env.enable_obsnorm()
        else:
            self._lib = _host_library(self.device, 'obsnorm')
            self._state = L.ObsNormState()
            self._out = None
        if from_norm is not None:
            self.load(from_norm)
        elif self.on_device:                          # a new object starts from nothing, whatever the handle held
            z = np.zeros(L.OBSNORM_COLS)
            env.obsnorm_load(0, z, z, z)

    # -- statistics ----------------------------------------------------------------------------------------------------
    def _stats(self):
        if self.on_device:
            return self.env.obsnorm_state()
        s = self._state
        return (int(s.n_state),) + tuple(np.array(a, dtype=np.float64) for a in (s.mean, s.S, s.std))

    def _split(self, a):
        t = torch.from_numpy(a).to(self.device)
        nl = L.OBSNORM_LIDAR
        return {'lidar': t[:nl], 'target': t[nl:]}

    @property
    def n_state(self):
        return self.env.obsnorm_count() if self.on_device else int(self._state.n_state)

    @property
    def mean(self):
        return self._split(self._stats()[1])

    @property
    def S(self):
        return self._split(self._stats()[2])

    @property
    def std(self):
        return self._split(self._stats()[3])

    def load(self, norm):
        """take over n_state, mean, S, std and `fixed` of a BatchedStateNorm / DeviceStateNorm"""
        if tuple(norm.modal) != self.modal:
            raise ValueError('the device normalisation covers lidar and target')
        a = {name: L.array_arg('hope_obsnorm_host', name, np.concatenate([d[k].detach().double().cpu().numpy().reshape(-1) for k in self.modal]),
                               np.float64, (L.OBSNORM_COLS,)) for name, d in (('mean', norm.mean), ('S', norm.S), ('std', norm.std))}
        if self.on_device:
            self.env.obsnorm_load(int(norm.n_state), *a.values())
        else:
            self._state.n_state = int(norm.n_state)
            for name, v in a.items():
                getattr(self._state, name)[:] = v.tolist()
        self.fixed = bool(norm.fixed)
        return self

    def to_batched(self, device=None):
        """-> a BatchedStateNorm with these statistics (bit for bit)"""
        n, mean, S, std = self._stats()
        out = BatchedStateNorm(device=self.device if device is None else device)
        nl = L.OBSNORM_LIDAR
        for name, a in (('mean', mean), ('S', S), ('std', std)):
            t = torch.from_numpy(a).to(out.mean['lidar'].device)
            setattr(out, name, {'lidar': t[:nl].clone(), 'target': t[nl:].clone()})
        out.n_state, out.fixed = n, self.fixed
        return out

    def fix_parameters(self):
        self.fixed = True

    # -- the calls -----------------------------------------------------------------------------------------------------
    def _pair(self, obs):
        if 'lidar' not in obs or 'target' not in obs:
            raise ValueError('DeviceStateNorm takes lidar and target together')
        lidar, target = obs['lidar'], obs['target']
        if lidar.dim() == 1 and target.dim() == 1:
            lidar, target = lidar.unsqueeze(0), target.unsqueeze(0)
        if target.dtype != lidar.dtype:
            target = target.to(lidar.dtype)
        if lidar.dtype not in (torch.float32, torch.float64):
            lidar, target = lidar.float(), target.float()
        return lidar.contiguous(), target.contiguous()

    def _run(self, obs, update, normalize):
        lidar, target = self._pair(obs)
        if self.on_device:
            return self.env.obsnorm(lidar, target, update, normalize)
        arg = partial(L.tensor_arg, 'hope_obsnorm_host', device=self.device)
        lp = arg('lidar', lidar, (torch.float32, torch.float64), (None, L.OBSNORM_LIDAR))
        rows = lidar.shape[0]
        tp = arg('target', target, lidar.dtype, (rows, L.OBSNORM_TARGET))
        ol = ot = None
        if normalize:
            if self._out is None or self._out[0].shape[0] < rows:
                self._out = (torch.zeros((max(rows, self.n), L.OBSNORM_LIDAR)), torch.zeros((max(rows, self.n), L.OBSNORM_TARGET)))
            ol = arg('out_lidar', self._out[0], torch.float32, (self._out[0].shape[0], L.OBSNORM_LIDAR))
            ot = arg('out_target', self._out[1], torch.float32, (self._out[0].shape[0], L.OBSNORM_TARGET))
        flags = (L.OBSNORM_UPDATE if update else 0) | (L.OBSNORM_NORMALIZE if normalize else 0)
        L.check(self._lib.hope_obsnorm_host(self._state, lp, tp, rows, int(lidar.dtype == torch.float64), flags, ol, ot), 'hope_obsnorm_host')
        return (self._out[0][:rows], self._out[1][:rows]) if normalize else (None, None)

    def update(self, obs):
        """fold obs['lidar'] [B, 120] / obs['target'] [B, 5] into the running statistics (no-op when fixed)"""
        if not self.fixed:
            self._run(obs, True, False)

    def _dict(self, obs, nl, nt):
        if obs['lidar'].dim() == 1:
            nl, nt = nl[0], nt[0]
        out = dict(obs)
        out['lidar'], out['target'] = nl, nt
        return out

    def normalize(self, obs):
        return self._dict(obs, *self._run(obs, False, True))

    def update_and_normalize(self, obs):
        """update(obs) then normalize(obs) with the new statistics, in one call of the library"""
        return self._dict(obs, *self._run(obs, not self.fixed, True))


def make_obs_norm(obs_norm, env, agent):
    """the loops' `obs_norm` argument: None (today's torch path: the agent's BatchedStateNorm), or 'device' -- the agent's
    `state_norm` is swapped for a DeviceStateNorm over `env` that takes over its statistics.  -> the DeviceStateNorm or None."""
    if obs_norm is None:
        return None
    if obs_norm != 'device':
        raise ValueError(f"obs_norm must be None or 'device', not {obs_norm!r}")
    sn = getattr(agent, 'state_norm', None)
    if sn is None:
        raise ValueError("obs_norm='device' needs an agent with a state_norm (state_norm=True)")
    if not (isinstance(sn, DeviceStateNorm) and sn.env is env):
        agent.state_norm = DeviceStateNorm(env, from_norm=sn)
    return agent.state_norm


# ---- PPO / SAC storage over [N, T] -----------------------------------------------------------
def batched_gae(reward, value, next_value, done, gamma=0.98, lam=0.95, use_gae=True):
    """Advantages of PPO.update (src/model/agent/ppo_agent.py:258-273) for N parallel scenes at once.

    The reference keeps ONE env's transitions in time order and runs
        delta = r + gamma * (1 - done) * V(s') - V(s);  gae = delta + gamma * lambda * gae * (1 - done)   (backwards)
    so with N scenes the recurrence runs along T independently per row.  reward / value / next_value / done: [N, T]
    (done as 0/1).  The accumulation is done in float64 like the reference's Python-float loop and returned in
    value's dtype.  Returns (adv [N, T], delta [N, T])."""
    r, v, nv, d = (x.to(torch.float64) for x in (reward, value, next_value, done))
    delta = (r + gamma * (1 - d) * nv - v).to(value.dtype).to(torch.float64)       # deltas are float32 tensors there
    if not use_gae:
        return delta.to(value.dtype), delta.to(value.dtype)
    adv = torch.zeros_like(delta)
    gae = torch.zeros(delta.shape[0], dtype=torch.float64, device=delta.device)
    for t in range(delta.shape[1] - 1, -1, -1):
        gae = delta[:, t] + gamma * lam * gae * (1.0 - d[:, t])
        adv[:, t] = gae
    return adv.to(value.dtype), delta.to(value.dtype)


class DeviceGae:
    """What BatchedPPO.advantages does after the critic forwards -- batched_gae, the critic's target, agents._global_mean_std and the
    normalisation -- over the library's advantage block (include/hope_env.h "PPO's advantage block"; rule: csrc/hope_gae_core.h), so
    that it can stand in as `agent.gae`: one fused call of three launches (k_gae_scan, k_gae_merge, k_adv_apply) instead of a Python
    loop along T.  With torch.distributed and more than one rank the call is split: scan and sums, an all-reduce of the three
    doubles {sum adv, sum adv^2, count}, then the normalisation -- what _global_mean_std does.  The sums' arithmetic order is fixed,
    so mean and std do not depend on the launch geometry; they differ from the torch path's in the last bits only, adv before the
    normalisation and v_target not at all.  On the device adv and v_target are (views of) persistent tensors of the env that the next
    call overwrites.  On an env without the library (CPU tensors; tests/fake_env.OracleEnv) the same runs on the host through
    hope_gae_host / hope_adv_normalize_host: the rule is one source for both.
    `sums`: the float64 [3] tensor of the last call that reduced them (after the all-reduce, if there was one)."""

    def __init__(self, env):
        self.env = env
        self.device = torch.device(env.device)
        self.on_device = hasattr(env, 'gae')
        self.sums = None
        if self.on_device:
            env.enable_gae()
        else:
            self._lib = _host_library(self.device, 'gae')

    @staticmethod
    def _world():
        import torch.distributed as dist
        return dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1

    def mean_std(self, sums=None):
        """the float32 (mean, std) the normalisation takes from `sums` (default: the last call's), as Python floats; downloads the
        three doubles (host-synchronous)"""
        s = (self.sums if sums is None else sums).detach().to('cpu', torch.float64).contiguous()
        ms = np.zeros(2, np.float32)
        sp = L.tensor_arg('hope_adv_normalize_host', 'sums', s, torch.float64, (3,), s.device)
        L.check(L.load_library().hope_adv_normalize_host(None, 0, sp, None, ms.ctypes), 'hope_adv_normalize_host')
        return float(ms[0]), float(ms[1])

    def _host(self, x, gamma, lam, flags):
        arg = partial(L.tensor_arg, 'hope_gae_host', dtype=torch.float32, device=self.device)
        reward, done, value, v_last, value_target = x
        rp = arg('reward', reward, shape=(None, None))
        rows, t = reward.shape
        adv, v_target = torch.empty((rows, t), dtype=torch.float32), torch.empty((rows, t), dtype=torch.float32)
        sums = torch.zeros(3, dtype=torch.float64)
        ptrs = [rp, arg('done', done, shape=(rows, t)), arg('value', value, shape=(rows, t)), arg('v_last', v_last, shape=(rows,)),
                arg('value_target', value_target, shape=(rows, t))]
        out = [arg('adv', adv, shape=(rows, t)), arg('v_target', v_target, shape=(rows, t)),
               L.tensor_arg('hope_gae_host', 'sums', sums, torch.float64, (3,), self.device)]
        L.check(self._lib.hope_gae_host(*ptrs, rows, t, float(gamma), float(lam), flags, *out, None), 'hope_gae_host')
        return adv, v_target, sums

    def __call__(self, reward, done, value, v_last, value_target, gamma, lam, normalize=True):
        """reward / done / value / value_target [N, T], v_last [N] -> (adv [N, T], v_target [N, T]), float32.  normalize=False
        (adv_norm=False): the scan alone, adv is the plain estimate."""
        import torch.distributed as dist
        x = [a.detach().to(torch.float32).contiguous() for a in (reward, done, value, v_last, value_target)]
        split = normalize and self._world() > 1
        if self.on_device:
            adv, v_target, sums = self.env.gae(*x, gamma, lam, normalize=(None if not normalize else not split))
            if split:
                dist.all_reduce(sums)
                self.env.adv_normalize(adv, sums)
        else:
            adv, v_target, sums = self._host(x, gamma, lam, 0 if not normalize else (L.GAE_SUMS if split else L.GAE_NORMALIZE))
            if split:
                dist.all_reduce(sums)
                ap = L.tensor_arg('hope_adv_normalize_host', 'adv', adv, torch.float32, tuple(adv.shape), self.device)
                sp = L.tensor_arg('hope_adv_normalize_host', 'sums', sums, torch.float64, (3,), self.device)
                L.check(self._lib.hope_adv_normalize_host(ap, adv.numel(), sp, ap, None), 'hope_adv_normalize_host')
        if normalize:
            self.sums = sums
        return adv, v_target


def make_gae(gae, env, agent):
    """the trainers' `gae` argument: None (today's torch path: batched_gae and _global_mean_std), or 'device' -- the agent's `gae` becomes
    a DeviceGae over `env`.  -> the DeviceGae or None."""
    if gae is None:
        return None
    if gae != 'device':
        raise ValueError(f"gae must be None or 'device', not {gae!r}")
    if not hasattr(agent, 'advantages'):
        raise ValueError("gae='device' needs an agent with an advantage block (BatchedPPO)")
    cur = getattr(agent, 'gae', None)
    if not (isinstance(cur, DeviceGae) and cur.env is env):
        agent.gae = DeviceGae(env)
    return agent.gae


class PpoMinibatch:
    """what DevicePpoBatch.gather hands to DevicePpoBatch.backward: the gathered tensors (`t`: lidar, target, mask, action [mb, .],
    old_lp, adv, v_target [mb], idx int32 [mb]), their descriptor and the extent"""

    def __init__(self, t, desc, mb):
        self.t, self.desc, self.mb = t, desc, mb


class DevicePpoBatch:
    """The body of BatchedPPO.update's inner loop around the two network forwards over the library's minibatch calls (include/hope_env.h
    "PPO's minibatch"; rule: csrc/hope_ppo_core.h), so that it can stand in as `agent.minibatch`: `gather` is ONE k_ppo_gather launch
    instead of seven index launches, `backward` two (k_ppo_loss, k_ppo_merge) and one torch.autograd.backward seeded with the loss's
    gradients at the networks' outputs, instead of about twenty elementwise launches and their autograd replay.  The loss is computed
    in float64 from the float32 network outputs, so the seeds differ from the torch path's in the last bits only.
    `ring`: a rollout.TransitionRing or DeviceTransitionRing; the gather reads its tensors as [n T] rows, so it must be full and start
    at column 0 (head == 0, size == T: what PPOTrainer updates from, where `ring.ordered()` returns the ring's own tensors).
    The gathered tensors and the gradients are persistent per minibatch size and overwritten by the next call with that size.  On an
    env without the library (CPU tensors; tests/fake_env.OracleEnv) the same runs on the host through hope_ppo_gather_host /
    hope_ppo_loss_host: the rule is one source for both.  The image key stays a torch gather by the same indices."""

    def __init__(self, env, ring):
        self.env, self.ring = env, ring
        self.device = torch.device(env.device)
        self.on_device = hasattr(env, 'ppo_gather')
        self.n, self.T = ring.n, ring.T
        if not self.on_device:
            self._lib = _host_library(self.device, 'ppo_gather')
        self._max = 0                                 # the handle's max_batch
        self._desc = L.ring_desc('DevicePpoBatch', self.device, self.n, self.T, lidar=ring.obs['lidar'], target=ring.obs['target'],
                                 action_mask=ring.obs['action_mask'], action=ring.action, log_prob=ring.log_prob, reward=ring.reward, done=ring.done)
        self._out = {}                                # mb -> PpoMinibatch
        self._grads = {}                              # mb -> (g_raw, g_log_std, g_value, losses), host path

    def _outputs(self, mb):
        if mb not in self._out:
            dev, f = self.device, torch.float32
            t = {'lidar': torch.zeros((mb, 120), dtype=f, device=dev), 'target': torch.zeros((mb, 5), dtype=f, device=dev),
                 'mask': torch.zeros((mb, 42), dtype=f, device=dev), 'action': torch.zeros((mb, 2), dtype=f, device=dev),
                 'old_lp': torch.zeros(mb, dtype=f, device=dev), 'adv': torch.zeros(mb, dtype=f, device=dev),
                 'v_target': torch.zeros(mb, dtype=f, device=dev), 'idx': torch.zeros(mb, dtype=torch.int32, device=dev)}
            self._out[mb] = PpoMinibatch(t, L.ppo_batch_desc('DevicePpoBatch.gather', dev, mb, **t), mb)
        return self._out[mb]

    def bind(self, obs, action, log_prob):
        """BatchedPPO.update's arguments must be the ring's own tensors (what `ring.ordered()` returns from a full ring that starts at
        column 0): the gather reads the ring, not them.  ValueError otherwise."""
        ring = self.ring
        pairs = [(obs.get(k), v) for k, v in ring.obs.items()] + [(action, ring.action), (log_prob, ring.log_prob)]
        if any(x is None or x.data_ptr() != v.data_ptr() or x.shape != v.shape for x, v in pairs):
            raise ValueError('DevicePpoBatch: update() was given other tensors than its ring holds (a full ring that starts at column 0?)')

    def gather(self, adv, v_target, ri):
        """adv, v_target: float32 with n T elements ([n, T] or flat); ri: int64 [mb] flat transitions (a slice of a permutation).
        -> (st, batch): st = {'lidar', 'target', 'action_mask'(, 'img')} of the minibatch, batch the PpoMinibatch for `backward`."""
        ring = self.ring
        if ring.head != 0 or ring.size != ring.T:
            raise ValueError(f'DevicePpoBatch reads a full ring that starts at column 0 (head 0, size {ring.T}), not head {ring.head}, size {ring.size}')
        m = self.n * self.T
        adv, v_target = (x.detach().to(torch.float32).contiguous().view(-1) for x in (adv, v_target))
        ri = ri.detach().to(torch.int64).contiguous()
        mb = int(ri.shape[0])
        batch = self._outputs(mb)
        if self.on_device:
            if mb > self._max:
                self.env.enable_ppo_batch(mb)
                self._max = mb
            self.env.ppo_gather(self._desc, adv, v_target, ri, batch.desc)
        else:
            arg = partial(L.tensor_arg, 'hope_ppo_gather_host', device=self.device)
            ptrs = [arg('adv', adv, torch.float32, (m,)), arg('v_target', v_target, torch.float32, (m,)), arg('index', ri, torch.int64, (mb,))]
            L.check(self._lib.hope_ppo_gather_host(self._desc, *ptrs, mb, batch.desc), 'hope_ppo_gather_host')
        t = batch.t
        st = {'lidar': t['lidar'], 'target': t['target'], 'action_mask': t['mask']}
        if 'img' in ring.obs:                         # the image key: a torch gather by the same indices
            img = ring.obs['img']
            st['img'] = img.reshape((m,) + img.shape[2:])[ri]
        return {k: st[k] for k in ring.obs}, batch

    def backward(self, raw, value, log_std, batch, clip):
        """raw [mb, 2]: the actor's output for the gathered observation, NOT clamped; value [mb, 1] or [mb]: the critic's; log_std
        [1, 2]: the agent's parameter.  The loss call, then one backward pass through both networks from its gradients.
        -> (actor_loss, critic_loss) as 0-dim tensors (views of a persistent tensor)."""
        mb = batch.mb
        r, v, ls = raw.detach().contiguous(), value.detach().reshape(-1).contiguous(), log_std.detach().reshape(-1).contiguous()
        if self.on_device:
            g_raw, g_log_std, g_value, losses = self.env.ppo_loss(r, ls, v, batch.desc, mb, clip)
        else:
            out = self._grads.get(mb)
            if out is None:
                out = self._grads[mb] = tuple(torch.zeros(s, dtype=torch.float32) for s in ((mb, 2), (2,), (mb,), (2,)))
            g_raw, g_log_std, g_value, losses = out
            arg = partial(L.tensor_arg, 'hope_ppo_loss_host', dtype=torch.float32, device=self.device)
            ptrs = [arg('raw', r, shape=(mb, 2)), arg('log_std', ls, shape=(2,)), arg('value', v, shape=(mb,))]
            gp = [arg(k, x, shape=tuple(x.shape)) for k, x in zip(('g_raw', 'g_log_std', 'g_value', 'losses'), out)]
            L.check(self._lib.hope_ppo_loss_host(*ptrs, batch.desc, mb, float(clip), *gp), 'hope_ppo_loss_host')
        torch.autograd.backward((raw, value, log_std), (g_raw, g_value.view(value.shape), g_log_std.view(log_std.shape)))
        return losses[0], losses[1]


def make_ppo_batch(minibatch, env, ring):
    """the trainers' `minibatch` argument: None (today's torch path: index gathers, the elementwise loss and autograd through it), or
    'device' -- a DevicePpoBatch over `env` and `ring`, for `agent.minibatch`.  -> the DevicePpoBatch or None."""
    if minibatch is None:
        return None
    if minibatch != 'device':
        raise ValueError(f"minibatch must be None or 'device', not {minibatch!r}")
    return DevicePpoBatch(env, ring)


class DeviceSacUpdate:
    """The arithmetic of BatchedSAC.update between its seven network forwards over the library's calls (include/hope_env.h "SAC's
    update"; rule: csrc/hope_sac_core.h), so that it can stand in as `agent.update_block`: the reparameterised sample is ONE launch
    (k_sac_sample), the Q target with the critics' losses and their gradients two (k_sac_critic, k_sac_merge), the actor loss's
    gradient at the critic outputs one (k_sac_seed), and the actor and temperature losses with their gradients at the actor's output,
    log_std and log_alpha two (k_sac_policy, k_sac_merge) -- instead of some eighty elementwise launches and their autograd replay.
    Autograd then runs through the networks only.  All arithmetic is float64 on the float32 network outputs, so the gradients differ
    from the torch path's in the last bits only.  The temperature is read on the device: no host synchronisation.
    The outputs are persistent per batch size and overwritten by the next call with that size.  On an env without the library (CPU
    tensors; tests/fake_env.OracleEnv) the same runs on the host through hope_sac_*_host: the rule is one source for both."""

    def __init__(self, env):
        self.env = env
        self.device = torch.device(env.device)
        self.on_device = hasattr(env, 'sac_sample')
        if not self.on_device:
            self._lib = _host_library(self.device, 'sac_sample')
        self._max = 0                                 # the handle's max_batch
        self._out = {}                                # (call, B) -> outputs, host path

    def _room(self, b):
        if self.on_device and b > self._max:
            self.env.enable_sac_update(b)
            self._max = b

    def _host(self, call, b, ins, scalars, shapes):
        """hope_sac_<call>_host over CPU tensors: ins = [(name, tensor, shape)], scalars = [(position among the arguments, value)],
        shapes = the outputs' (None: the float64 scalar) -> the persistent outputs"""
        name = f'hope_sac_{call}_host'
        out = self._out.get((call, b))
        if out is None:
            out = self._out[(call, b)] = tuple(torch.zeros((), dtype=torch.float64) if s is None else torch.zeros(s, dtype=torch.float32) for s in shapes)
        args = [L.tensor_arg(name, k, x, torch.float64 if s == () else torch.float32, s, self.device) for k, x, s in ins]
        for at, v in scalars:
            args.insert(at, v)
        args += [L.tensor_arg(name, f'output {i}', x, x.dtype, tuple(x.shape), self.device) for i, x in enumerate(out)]
        L.check(getattr(self._lib, name)(*args), name)
        return out

    @staticmethod
    def _f32(x, shape):
        return x.detach().to(torch.float32).reshape(shape).contiguous()

    def sample(self, raw, log_std, eps):
        """raw [B, 2]: the actor's output, NOT clamped; log_std [1, 2]: the agent's parameter; eps [B, 2]: the normal draw
        -> (action [B, 2], lp [B]) without a graph"""
        b = int(raw.shape[0])
        r, ls, e = self._f32(raw, (b, 2)), self._f32(log_std, (2,)), self._f32(eps, (b, 2))
        self._room(b)
        if self.on_device:
            return self.env.sac_sample(r, ls, e)
        return self._host('sample', b, [('raw', r, (b, 2)), ('log_std', ls, (2,)), ('eps', e, (b, 2))], [(3, b)], ((b, 2), (b,)))

    def critic(self, q1, q2, qt1, qt2, next_lp, reward, done, log_alpha, gamma):
        """q1, q2, qt1, qt2, reward, done: [B, 1] or [B]; next_lp [B]; log_alpha: the agent's float64 scalar
        -> (q_target [B], g_q1 [B], g_q2 [B], losses [2])"""
        b = int(q1.shape[0])
        names = ('q1', 'q2', 'qt1', 'qt2', 'next_lp', 'reward', 'done')
        t = [self._f32(x, (b,)) for x in (q1, q2, qt1, qt2, next_lp, reward, done)]
        la = log_alpha.detach()
        self._room(b)
        if self.on_device:
            return self.env.sac_critic(*t, la, gamma)
        return self._host('critic', b, [(k, x, (b,)) for k, x in zip(names, t)] + [('log_alpha', la, ())], [(8, float(gamma)), (9, b)],
                          ((b,), (b,), (b,), (2,)))

    def seed(self, q1, q2):
        """q1, q2 [B, 1] or [B]: the critics at the sampled action -> (s1 [B], s2 [B])"""
        b = int(q1.shape[0])
        t1, t2 = self._f32(q1, (b,)), self._f32(q2, (b,))
        self._room(b)
        if self.on_device:
            return self.env.sac_seed(t1, t2)
        return self._host('seed', b, [('q1', t1, (b,)), ('q2', t2, (b,))], [(2, b)], ((b,), (b,)))

    def policy(self, raw, log_std, eps, q1, q2, g_action, log_alpha, target_entropy):
        """raw, log_std, eps as for `sample`; q1, q2 as for `seed`; g_action [B, 2]: autograd's gradient at the sampled action for the
        seeds -> (g_raw [B, 2], g_log_std [2], g_log_alpha (float64 scalar), losses [2] = actor loss, temperature loss)"""
        b = int(raw.shape[0])
        r, ls, e, g = self._f32(raw, (b, 2)), self._f32(log_std, (2,)), self._f32(eps, (b, 2)), self._f32(g_action, (b, 2))
        t1, t2 = self._f32(q1, (b,)), self._f32(q2, (b,))
        la = log_alpha.detach()
        self._room(b)
        if self.on_device:
            return self.env.sac_policy(r, ls, e, t1, t2, g, la, target_entropy)
        return self._host('policy', b, [('raw', r, (b, 2)), ('log_std', ls, (2,)), ('eps', e, (b, 2)), ('q1', t1, (b,)), ('q2', t2, (b,)),
                                        ('g_action', g, (b, 2)), ('log_alpha', la, ())], [(7, float(target_entropy)), (8, b)],
                          ((b, 2), (2,), None, (2,)))


def make_sac_update(kind, env):
    """the trainers' `sac_update` argument: None (today's torch path: the elementwise lines of BatchedSAC.update and autograd through
    them), or 'device' -- a DeviceSacUpdate over `env`, for `agent.update_block`.  -> the DeviceSacUpdate or None."""
    if kind is None:
        return None
    if kind != 'device':
        raise ValueError(f"sac_update must be None or 'device', not {kind!r}")
    return DeviceSacUpdate(env)


class DeviceImgEncoder:
    """The image token of a HopeNet over the library's image encoder (include/hope_env.h "the image encoder's inference forward";
    rule: csrc/hope_imgenc_core.h): `enc(img)` takes img uint8 [B, 3, 64, 64] and returns what
    `net.re_embed_img(net.embed_img(img.float() * (1 / 255)))` returns, float32 [B, 128], from two launches (k_imgenc_conv,
    k_imgenc_head).  The 14 encoder tensors are re-packed (one more launch, k_imgenc_pack) when they changed: the key is their storage
    and the sum of their version counters, as DeviceActor's, taken over these tensors only; `packs` counts the loads.  A handle holds
    one set of packed encoder tensors: two encoders over one env each re-pack when the other ran in between.  On an env without the
    library (CPU tensors) the same forward runs on the host through hope_imgenc_forward_host.  A float image is not this path's
    input: it goes through torch, as it always did.  ValueError for a net of another configuration."""

    def __init__(self, env, net):
        self.act = L.imgenc_shape(net)                    # before any state changes
        self.env, self.net = env, net
        self.device = torch.device(env.device)
        self.on_device = hasattr(env, 'img_encoder_forward')
        if not self.on_device:
            self._lib = _host_library(self.device, 'img_encoder_forward')
        self.packs = 0
        self._key = self._params = self._held = None
        self._max = 0

    def _net_key(self):
        sd = dict(self.net.named_parameters())
        ps = [sd[key] for _, key, _ in L.IMGENC_FIELDS]     # the 14 encoder tensors only
        return tuple(p.data_ptr() for p in ps), sum(p._version for p in ps)

    def _load(self):
        if self.on_device:
            self.env.img_encoder_load(self.net)
            self.env._imgenc_owner = self
        else:
            self._params, self._held = L.imgenc_params('hope_imgenc_forward_host', self.net, self.device)
        self.packs += 1

    @torch.no_grad()
    def __call__(self, img, features=False):
        if img.dtype != torch.uint8:                      # not the device path's input
            return self.net.re_embed_img(self.net.embed_img(img.to(torch.float32))).to(torch.float32).contiguous()
        img = img.detach().contiguous()
        b = int(img.shape[0])
        mine = True
        if self.on_device:
            if b > self._max or self.env._imgenc_act != self.act:
                self._max = max(self._max, b)
                self.env.enable_img_encoder(self.act, max_batch=self._max)
            mine = self.env._imgenc_owner is self
        key = self._net_key()
        if key != self._key or not mine:
            self._load()
            self._key = key
        if self.on_device:
            return self.env.img_encoder_forward(img, features=features)
        name = 'hope_imgenc_forward_host'
        token = torch.zeros((b, 128), dtype=torch.float32)
        feat = torch.zeros((b, 2048), dtype=torch.float32) if features else None
        L.check(self._lib.hope_imgenc_forward_host(C.byref(self._params), self.act, L.tensor_arg(name, 'img', img, torch.uint8, (b, 3, 64, 64), self.device), b,
                                                   L.tensor_arg(name, 'token', token, torch.float32, (b, 128), self.device),
                                                   L.tensor_arg(name, 'features', feat, torch.float32, (b, 2048), self.device, optional=True)), name)
        return (token, feat) if features else token


class DeviceActor:
    """The actor's inference forward over the library's fused kernel (include/hope_env.h "the policy's inference forward"; rule:
    csrc/hope_policy_core.h), so that it can stand in as `agent.device_actor`: `actor(nobs)` returns what
    `torch.clamp(net(nobs), -1, 1)` returns, from ONE launch (k_policy_forward) instead of the net's hundred.  Every Linear is the
    float32 fmaf chain of the matrix cores, the rest float64 rounded once, so the result differs from torch's float32 forward by
    rounding only.  The parameters are re-packed (one more launch, k_policy_pack) when they changed: the key is the parameters'
    storage and the sum of their version counters, which in-place optimiser steps and load_state_dict both advance; an unchanged
    net costs no launch (`packs` counts the loads).  A handle holds one set of packed parameters: two actors over one env each re-pack
    when the other ran in between (a second net is better served by an env of its own).  With an image the net's encoder (convolutions, re_embed_img) runs in torch by
    default and its token goes in ready-made; img_encoder='device' sends a uint8 image through a DeviceImgEncoder instead (two more
    launches, the 128-float token the only intermediate torch sees; a float image still goes through torch).  On an env without the library (CPU tensors; tests/fake_env.OracleEnv) the same forward runs on the
    host through hope_policy_forward_host: the rule is one source for both.  ValueError for a net of another configuration."""

    def __init__(self, env, net, img_encoder=None):
        self.shape = L.policy_shape(net)                  # before any state changes
        if img_encoder not in (None, 'device'):
            raise ValueError(f"img_encoder must be None or 'device', not {img_encoder!r}")
        if img_encoder == 'device' and self.shape[0] != 4:
            raise ValueError("img_encoder='device' needs a net with an image token (use_img)")
        self.img_encoder = DeviceImgEncoder(env, net) if img_encoder == 'device' else None
        self.env, self.net = env, net
        self.device = torch.device(env.device)
        self.on_device = hasattr(env, 'policy_forward')
        if not self.on_device:
            self._lib = _host_library(self.device, 'policy_forward')
        self.packs = 0
        self._key = self._params = self._held = None
        self._max = 0

    def _net_key(self):
        ps = list(self.net.parameters())
        return tuple(p.data_ptr() for p in ps), sum(p._version for p in ps)

    def _load(self):
        if self.on_device:
            self.env.policy_load(self.net)
            self.env._policy_owner = self
        else:
            self._params, self._held = L.policy_params('hope_policy_forward_host', self.net, self.device)
        self.packs += 1

    @torch.no_grad()
    def __call__(self, nobs):
        f32 = lambda k: nobs[k].detach().to(torch.float32).contiguous()  # noqa: E731
        lidar, target, mask = f32('lidar'), f32('target'), f32('action_mask')
        b = int(lidar.shape[0])
        token = nobs.get('img_token')                     # [B, 128], when the caller already has it
        if token is not None:
            token = token.detach().to(torch.float32).contiguous()
        elif self.shape[0] == 4:
            img = nobs['img']
            if self.img_encoder is not None and img.dtype == torch.uint8:
                token = self.img_encoder(img)
            else:
                if img.dtype == torch.uint8:              # as HopeNet.tokens
                    img = img.to(torch.float32) * (1.0 / 255.0)
                token = self.net.re_embed_img(self.net.embed_img(img)).to(torch.float32).contiguous()
        mine = True
        if self.on_device:                                # a handle holds ONE shape and ONE set of packed parameters: take them back if another actor had them
            if b > self._max or self.env._policy_shape != self.shape:
                self._max = max(self._max, b)
                self.env.enable_policy(*self.shape, max_batch=self._max)
            mine = self.env._policy_owner is self
        key = self._net_key()
        if key != self._key or not mine:
            self._load()
            self._key = key
        if self.on_device:
            out = self.env.policy_forward(lidar, target, mask, token)
        else:
            name = 'hope_policy_forward_host'
            out = torch.zeros((b, self.shape[1]), dtype=torch.float32)
            arg = partial(L.tensor_arg, name, dtype=torch.float32, device=self.device)
            L.check(self._lib.hope_policy_forward_host(C.byref(self._params), *self.shape, arg('lidar', lidar, shape=(b, L.LIDAR_NUM)),
                                                       arg('target', target, shape=(b, L.TARGET_DIM)), arg('action_mask', mask, shape=(b, L.N_ACTION)),
                                                       arg('img_token', token, shape=(b, 128), optional=True), b, arg('out', out, shape=tuple(out.shape))), name)
        return torch.clamp(out, -1, 1)


def make_actor(kind, env, agent, img_encoder=None):
    """the `actor` argument of rollouts, trainers and evaluators: None (today's torch forward, with the fast-policy levers if they
    are on), or 'device' -- a DeviceActor over `env` and the agent's actor, set as `agent.device_actor`.  img_encoder: None (the
    image encoder stays in torch) or 'device' (a DeviceImgEncoder inside the DeviceActor): valid only with actor='device' and an
    agent whose actor takes an image, ValueError otherwise.  -> the DeviceActor or None."""
    if img_encoder not in (None, 'device'):
        raise ValueError(f"img_encoder must be None or 'device', not {img_encoder!r}")
    if kind is None:
        if img_encoder is not None:
            raise ValueError("img_encoder='device' needs actor='device'")
        return None
    if kind != 'device':
        raise ValueError(f"actor must be None or 'device', not {kind!r}")
    if img_encoder is not None and not getattr(agent.actor, 'use_img', False):
        raise ValueError("img_encoder='device' needs an agent with an image token (use_img)")
    agent.device_actor = DeviceActor(env, agent.actor, img_encoder=img_encoder)
    return agent.device_actor


class DeviceCritics:
    """The no-gradient forward of up to four critics of one shape over the library's fused kernel (include/hope_env.h "the critics'
    inference forward"; rule: csrc/hope_critic_core.h), so that it can stand in as `agent.device_critics`: `crit(nobs)` (PPO critics:
    HopeNets with one linear output) or `crit(nobs, action)` (SacCritics) returns a list of [B, 1] float32 tensors holding what
    `net(nobs)` / `net(nobs, action)` returns for each net, from ONE launch (k_critic_forward on a grid of tiles x nets) instead of a
    hundred per net.  which: the indices into `nets` to evaluate, in the order of the result (default: all).  Every Linear is the
    float32 fmaf chain of the matrix cores, the rest float64 rounded once, so the result differs from torch's float32 forward by
    rounding only.  Net i lives in slot i of the handle.  A slot is re-packed (one more launch, k_critic_pack) when its net changed:
    the key, kept per slot, is the parameters' storage and the sum of their version counters, which in-place optimiser steps,
    `_soft_update` and load_state_dict all advance; an unchanged net costs no launch (`packs[i]` counts the loads of net i).  With an
    image each net's own encoder (convolutions, re_embed_img) runs in torch and its token goes in ready-made; `nobs['img_token']`
    [len(which), B, 128], when the caller already has the tokens, is taken instead.  Inputs longer than `chunk` rows (default: the
    library's largest batch) go through in pieces.  On an env without the library (CPU tensors; tests/fake_env.OracleEnv) the same
    forward runs on the host through hope_critic_forward_host, a net at a time: the rule is one source for both.  ValueError for a
    net of another configuration, or nets of different shapes."""

    def __init__(self, env, nets):
        nets = list(nets)
        if not 1 <= len(nets) <= L.CRITIC_SLOTS:
            raise ValueError(f'DeviceCritics takes 1 .. {L.CRITIC_SLOTS} nets, not {len(nets)}')
        shapes = [L.critic_shape(n) for n in nets]        # before any state changes
        if any(s != shapes[0] for s in shapes):
            raise ValueError(f'DeviceCritics: the nets must share one shape (has_img, has_action), got {shapes}')
        self.shape = shapes[0]
        self.env, self.nets = env, nets
        self.device = torch.device(env.device)
        self.on_device = hasattr(env, 'critic_forward')
        if not self.on_device:
            self._lib = _host_library(self.device, 'critic_forward')
        self.packs = [0] * len(nets)
        self._keys, self._params, self._held = [None] * len(nets), [None] * len(nets), [None] * len(nets)
        self._max = 0
        self.chunk = L.POLICY_MAX_BATCH

    def _net_key(self, i):
        ps = list(self.nets[i].parameters())
        return tuple(p.data_ptr() for p in ps), sum(p._version for p in ps)

    def _load(self, i):
        if self.on_device:
            self.env.critic_load(i, self.nets[i])
            self.env._critic_owner[i] = self
        else:
            self._params[i], self._held[i] = L.critic_params('hope_critic_forward_host', self.nets[i], self.device)
        self.packs[i] += 1

    def _token(self, i, img):
        net = L.critic_net(self.nets[i])
        if img.dtype == torch.uint8:                      # as HopeNet.tokens
            img = img.to(torch.float32) * (1.0 / 255.0)
        return net.re_embed_img(net.embed_img(img)).to(torch.float32)

    @torch.no_grad()
    def __call__(self, nobs, action=None, which=None):
        which = list(range(len(self.nets))) if which is None else [int(i) for i in which]
        has_img, has_action = self.shape
        if has_action != int(action is not None):
            raise ValueError('DeviceCritics: SacCritics take an action, critic HopeNets take none')
        f32 = lambda x: x.detach().to(torch.float32).contiguous()  # noqa: E731
        lidar, target, mask = f32(nobs['lidar']), f32(nobs['target']), f32(nobs['action_mask'])
        act = f32(action) if has_action else None
        tokens = nobs.get('img_token') if has_img else None   # [len(which), B, 128], when the caller already has them
        b, n = int(lidar.shape[0]), len(which)
        c = min(b, int(self.chunk))
        if self.on_device:                                # the handle holds ONE shape: take it back if other critics had it
            want = (len(self.nets),) + self.shape
            if c > self._max or self.env._critic_shape != want:
                self._max = max(self._max, c)
                self.env.enable_critics(*want, max_batch=self._max)
        for i in which:
            key = self._net_key(i)
            if key != self._keys[i] or (self.on_device and self.env._critic_owner.get(i) is not self):
                self._load(i)
                self._keys[i] = key
        res = torch.empty((n, b), dtype=torch.float32, device=self.device)
        for at in range(0, b, c):
            m = min(c, b - at)
            rows = slice(at, at + m)
            tok = None
            if has_img:
                tok = f32(tokens[:, rows]) if tokens is not None else torch.stack([self._token(i, nobs['img'][rows]) for i in which]).contiguous()
            a = act[rows] if has_action else None
            if self.on_device:
                r = self.env.critic_forward(which, lidar[rows], target[rows], mask[rows], tok, a, out=res if m == b else None)
                if m != b:
                    res[:, rows] = r
                continue
            name = 'hope_critic_forward_host'
            arg = partial(L.tensor_arg, name, dtype=torch.float32, device=self.device)
            for j, i in enumerate(which):
                out = torch.zeros((m,), dtype=torch.float32)
                L.check(self._lib.hope_critic_forward_host(C.byref(self._params[i]), has_img, has_action, arg('lidar', lidar[rows], shape=(m, L.LIDAR_NUM)),
                                                           arg('target', target[rows], shape=(m, L.TARGET_DIM)), arg('action_mask', mask[rows], shape=(m, L.N_ACTION)),
                                                           arg('img_token', None if tok is None else tok[j], shape=(m, 128), optional=True),
                                                           arg('action', a, shape=(m, 2), optional=True), m, arg('out', out, shape=(m,))), name)
                res[j, rows] = out
        return [res[j].unsqueeze(1) for j in range(n)]


def make_critics(kind, env, agent):
    """the `critics` argument of rollouts, trainers and evaluators: None (today's torch forwards), or 'device' -- a DeviceCritics over
    `env` and the agent's no-gradient critics, set as `agent.device_critics`: a BatchedSAC's (critic_target1, critic_target2), a
    BatchedPPO's (critic, critic_target).  -> the DeviceCritics or None."""
    if kind is None:
        return None
    if kind != 'device':
        raise ValueError(f"critics must be None or 'device', not {kind!r}")
    if hasattr(agent, 'critic_target1'):
        nets = (agent.critic_target1, agent.critic_target2)
    elif hasattr(agent, 'critic_target'):
        nets = (agent.critic, agent.critic_target)
    else:
        raise ValueError(f"critics='device' needs a BatchedSAC or a BatchedPPO, not {type(agent).__name__}")
    agent.device_critics = DeviceCritics(env, nets)
    return agent.device_critics


_ADAM_REFUSED = ('amsgrad', 'maximize', 'capturable', 'differentiable', 'fused')


class DeviceAdam:
    """A `torch.optim.Adam` whose `step()` is the library's optimiser block (include/hope_env.h "the optimiser block"; rule:
    csrc/hope_optim_core.h): ONE launch of k_optim per 64 tensors instead of torch's chain of multi-tensor launches.  The wrapped
    optimiser stays the truth and is kept as `.optimizer`: the step reads lr, betas and eps from its param_groups at every call (a
    scheduler works), creates a parameter's state on first use exactly as torch does (`step` a CPU float32 scalar tensor, `exp_avg`
    and `exp_avg_sq` from zeros_like), advances `step` by one, skips a parameter whose grad is None, and updates the same parameter
    and state tensors in place -- so state_dict / load_state_dict / checkpoints go through `.optimizer` unchanged and a run can switch
    between the two at any step.  After the launch the version counters of the parameters and the state tensors advance by one, so
    that DeviceActor / DeviceCritics / DeviceImgEncoder re-pack as after a torch step.  The arithmetic is the library's one rule, not
    torch's bits: see DESIGN 5p for the measured distance.  ValueError naming the option for amsgrad, weight_decay != 0, maximize,
    capturable, differentiable, fused, a tensor lr, a sparse gradient, or an optimiser that is not Adam.  On an env without the
    library (CPU tensors; tests/fake_env.OracleEnv) the same step runs on the host through hope_optim_adam_host."""

    def __init__(self, env, optimizer):
        if type(optimizer) is not torch.optim.Adam:
            raise ValueError(f'optimizer: DeviceAdam wraps a torch.optim.Adam, not {type(optimizer).__name__}')
        self.env, self.optimizer = env, optimizer
        self.device = torch.device(env.device)
        self.on_device = hasattr(env, 'optim_adam')
        if not self.on_device:
            self._lib = _host_library(self.device, 'optim_adam')
        self.steps = 0                                    # calls that moved at least one tensor
        self._check()

    # the wrapped optimiser's own surface
    param_groups = property(lambda self: self.optimizer.param_groups)
    state = property(lambda self: self.optimizer.state)

    def state_dict(self):
        return self.optimizer.state_dict()

    def load_state_dict(self, state_dict):
        return self.optimizer.load_state_dict(state_dict)

    def zero_grad(self, set_to_none=True):
        return self.optimizer.zero_grad(set_to_none=set_to_none)

    def add_param_group(self, param_group):
        return self.optimizer.add_param_group(param_group)

    def _check(self):
        for gi, group in enumerate(self.optimizer.param_groups):
            for k in _ADAM_REFUSED:
                if group.get(k):
                    raise ValueError(f'{k}: DeviceAdam does not take {k}=True (param group {gi})')
            if group.get('weight_decay', 0) != 0:
                raise ValueError(f"weight_decay: DeviceAdam does not take weight_decay != 0 (param group {gi})")
            if torch.is_tensor(group['lr']):
                raise ValueError(f'lr: DeviceAdam does not take a tensor lr (param group {gi})')
            if any(p.grad is not None and p.grad.is_sparse for p in group['params']):
                raise ValueError(f'sparse gradient: DeviceAdam does not take sparse gradients (param group {gi})')

    def _gather(self):
        """what torch's _init_group does -> [(p, grad, exp_avg, exp_avg_sq, hyper key)] of the parameters that move; their `step`
        has advanced.  `_check` comes first (step_optimizers): nothing here refuses."""
        jobs = []
        for group in self.optimizer.param_groups:
            lr, betas, eps = float(group['lr']), group['betas'], float(group['eps'])
            for p in group['params']:
                if p.grad is None:
                    continue
                st = self.optimizer.state[p]
                if len(st) == 0:
                    st['step'] = torch.tensor(0.0, dtype=torch.float32)
                    st['exp_avg'] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st['exp_avg_sq'] = torch.zeros_like(p, memory_format=torch.preserve_format)
                jobs.append((p, p.grad, st['exp_avg'], st['exp_avg_sq'], (lr, float(betas[0]), float(betas[1]), eps), st['step']))
        if jobs:                                          # only now, with nothing left to refuse, the counters move
            torch._foreach_add_([j[5] for j in jobs], 1)
        return [(p, g, m, v, hp + (int(step.item()),)) for p, g, m, v, hp, step in jobs]

    @staticmethod
    def _run(env, lib, jobs):
        """jobs as ONE call per four distinct groups, in order"""
        at = 0
        while at < len(jobs):
            keys, end = [], at
            while end < len(jobs) and (jobs[end][4] in keys or len(keys) < L.OPTIM_MAX_GROUPS):
                if jobs[end][4] not in keys:
                    keys.append(jobs[end][4])
                end += 1
            part = jobs[at:end]
            groups = [L.optim_group(k[0], (k[1], k[2]), k[3], k[4]) for k in keys]
            cols = [[j[c] for j in part] for c in range(4)]
            cols[1] = [g.contiguous() for g in cols[1]]   # (a gradient that autograd left strided: a copy; the others are updated in place)
            group_of = [keys.index(j[4]) for j in part]
            if lib is None:
                env.optim_adam(*cols, groups, group_of)
            else:
                table, n, _keep = L.optim_entries(*cols, group_of, 'hope_optim_adam_host')
                L.check(lib.hope_optim_adam_host(table, n, (L.OptimGroup * len(groups))(*groups), len(groups)), 'hope_optim_adam_host')
            at = end
        torch.autograd.graph.increment_version([x for j in jobs for x in (j[0], j[2], j[3])])

    @torch.no_grad()
    def step(self, closure=None):
        if closure is not None:
            raise ValueError('closure: DeviceAdam does not take a closure')
        step_optimizers(self)


def step_optimizers(*opts):
    """`.step()` of every optimiser, in order.  DeviceAdams over one env run as ONE call of the library (one group per param group,
    at most four to a call, else several calls); anything else -- torch optimisers, or a mix -- is each `.step()` in turn."""
    if opts and all(isinstance(o, DeviceAdam) for o in opts) and all(o.env is opts[0].env for o in opts):
        with torch.no_grad():
            for o in opts:                                # every refusal before anything moves
                o._check()
            jobs = [o._gather() for o in opts]
            flat = [j for js in jobs for j in js]
            if flat:
                DeviceAdam._run(opts[0].env, None if opts[0].on_device else opts[0]._lib, flat)
            for o, js in zip(opts, jobs):
                o.steps += bool(js)
        return
    for o in opts:
        o.step()


class DevicePolyak:
    """agents._soft_update over the library's optimiser block: `polyak(pairs, tau)` with pairs = [(target_module, current_module), ...]
    is target <- (1 - tau) * target + tau * current for every parameter of every pair, as ONE call (one launch per 64 tensors)
    instead of two multi-tensor launches per pair.  The targets' version counters advance by one, so a DeviceCritics over them
    re-packs as after `_soft_update`.  On an env without the library the same runs on the host through hope_optim_polyak_host."""

    def __init__(self, env):
        self.env = env
        self.device = torch.device(env.device)
        self.on_device = hasattr(env, 'optim_polyak')
        if not self.on_device:
            self._lib = _host_library(self.device, 'optim_polyak')
        self.calls = 0

    @torch.no_grad()
    def polyak(self, pairs, tau):
        targets, currents = [], []
        for t, c in pairs:
            tp, cp = list(t.parameters()), list(c.parameters())
            if len(tp) != len(cp):
                raise ValueError(f'DevicePolyak: a target with {len(tp)} parameters against a net with {len(cp)}')
            targets += tp
            currents += cp
        if self.on_device:
            self.env.optim_polyak(targets, currents, tau)
        else:
            table, n, _keep = L.optim_entries(targets, currents, call='hope_optim_polyak_host')
            L.check(self._lib.hope_optim_polyak_host(table, n, float(tau)), 'hope_optim_polyak_host')
        torch.autograd.graph.increment_version(targets)
        self.calls += 1

    __call__ = polyak


_OPTIMIZER_NAMES = ('actor_opt', 'critic_opt', 'critic_opt1', 'critic_opt2', 'alpha_opt')


def make_optimizers(kind, env, agent):
    """the trainers' `optimizer` argument: None (today's path: torch.optim.Adam.step and agents._soft_update), or 'device' -- every
    optimiser of the agent (actor_opt, critic_opt / critic_opt1, critic_opt2, alpha_opt: its float64 scalar is one entry, one launch)
    becomes a DeviceAdam over `env` around the torch optimiser it was, and `agent.soft_update` a DevicePolyak's `polyak`.
    -> {name: DeviceAdam} or None."""
    if kind is None:
        return None
    if kind != 'device':
        raise ValueError(f"optimizer must be None or 'device', not {kind!r}")
    made = {}
    for name in _OPTIMIZER_NAMES:
        opt = getattr(agent, name, None)
        if opt is None:
            continue
        if not isinstance(opt, DeviceAdam):
            opt = DeviceAdam(env, opt)
            setattr(agent, name, opt)
        made[name] = opt
    if not made:
        raise ValueError(f"optimizer='device' needs an agent with Adam optimisers (BatchedPPO, BatchedSAC), not {type(agent).__name__}")
    agent.soft_update = DevicePolyak(env)
    return made


def torch_optimizers(agent):
    """the agent's optimisers as torch objects, in _OPTIMIZER_NAMES' order: what a checkpoint's 'optimizer' tuple holds, whichever path
    steps them"""
    opts = [getattr(agent, name, None) for name in _OPTIMIZER_NAMES]
    return tuple(getattr(o, 'optimizer', o) for o in opts if o is not None)


class RolloutStorage:
    """Device-resident [N, T] ring of transitions: the batched stand-in for ReplayMemory (src/model/replay_memory.py)
    as both agents use it -- PPO reads everything in time order (get_items(arange), ppo_agent.py:241), SAC samples
    uniformly (sample(batch_size), sac_agent.py) with next_state = None at episode ends / at the newest entry
    (:27-30), which is reported here as `next_valid`."""

    def __init__(self, n, horizon, obs_shapes, device='cpu', action_dim=2, extra=('log_prob',)):
        self.n, self.T, self.device = n, horizon, torch.device(device)
        self.obs = {k: torch.zeros((n, horizon) + tuple(s), dtype=torch.uint8 if k == 'img' else torch.float32, device=self.device)
                    for k, s in obs_shapes.items()}
        self.action = torch.zeros((n, horizon, action_dim), dtype=torch.float32, device=self.device)
        self.reward = torch.zeros((n, horizon), dtype=torch.float32, device=self.device)
        self.done = torch.zeros((n, horizon), dtype=torch.float32, device=self.device)
        self.extra = {k: torch.zeros((n, horizon, action_dim), dtype=torch.float32, device=self.device) for k in extra}
        self.head, self.size = 0, 0

    def push(self, obs, action, reward, done, **extra):
        """one step of all N scenes (ReplayMemory.push :12-15)"""
        t = self.head
        for k in self.obs:
            self.obs[k][:, t] = obs[k].to(self.obs[k].dtype)
        self.action[:, t] = action
        self.reward[:, t] = reward
        self.done[:, t] = done.to(torch.float32)
        for k, v in extra.items():
            self.extra[k][:, t] = v
        self.head = (t + 1) % self.T
        self.size = min(self.size + 1, self.T)

    def _time_index(self):
        """column indices oldest -> newest"""
        return (torch.arange(self.size, device=self.device) + (self.head - self.size)) % self.T

    def ordered(self):
        """everything in time order, [N, size, ...] (PPO); next-observation of column j is column j + 1"""
        idx = self._time_index()
        out = {'obs': {k: v[:, idx] for k, v in self.obs.items()}, 'action': self.action[:, idx],
               'reward': self.reward[:, idx], 'done': self.done[:, idx]}
        out.update({k: v[:, idx] for k, v in self.extra.items()})
        return out

    def sample(self, batch_size, generator=None):
        """uniform transitions over (scene, time) like ReplayMemory.sample (:33-35).  next_valid is False where the
        reference returns next_state None: episode end or newest entry (:27-28)."""
        idx = self._time_index()
        s = torch.randint(self.n, (batch_size,), device=self.device, generator=generator)
        j = torch.randint(self.size, (batch_size,), device=self.device, generator=generator)
        t = idx[j]
        nxt = idx[torch.clamp(j + 1, max=self.size - 1)]
        next_valid = (j < self.size - 1) & (self.done[s, t] == 0)
        return {'obs': {k: v[s, t] for k, v in self.obs.items()}, 'next_obs': {k: v[s, nxt] for k, v in self.obs.items()},
                'next_valid': next_valid, 'action': self.action[s, t], 'reward': self.reward[s, t], 'done': self.done[s, t]}

    def clear(self):
        self.head, self.size = 0, 0
