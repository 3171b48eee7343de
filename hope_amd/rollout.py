"""Batched rollout / training loops over N scenes: the N >> 1 counterparts of the episode loops in
src/train/train_HOPE_ppo.py:177-213, src/train/train_HOPE_sac.py:177-221 and src/evaluation/eval_utils.py:16-84, with
the hybrid controller of src/model/agent/parking_agent.py (replay a found Reeds-Shepp path, otherwise ask the policy).

  HopeRollout.collect_step   one env step of every scene: state-norm -> actor -> mask-weighted / Gaussian action (or the
                             planner's) -> ParkingBatch.step(auto_reset) -> storage -> planner bookkeeping
  PPOTrainer                 BASELINE config 5 (train_HOPE_ppo.py): T steps of all scenes, then BatchedPPO.update
  SACTrainer                 BASELINE config 4 / train_HOPE_sac.py: [N, T] ring replay, one BatchedSAC.update every
                             `update_every` steps once the ring holds `warmup` columns
  BatchedRollout             round-1 loop with a stand-in MLP policy (kept for the examples)

`env` is a `hope_amd.ParkingBatch` (HIP path) or anything with the same attributes (tests use a CPU fake).
ParkingBatch's observation tensors are persistent buffers that the next step overwrites in place, so every loop
copies what it keeps BEFORE stepping.
"""
import numpy as np
import torch

from . import _lib as L
from . import agent_glue as G


class StandInPolicy(torch.nn.Module):
    def __init__(self, hidden=256):
        super().__init__()
        self.net = torch.nn.Sequential(torch.nn.Linear(120 + 5 + 42, hidden), torch.nn.Tanh(),
                                       torch.nn.Linear(hidden, hidden), torch.nn.Tanh(), torch.nn.Linear(hidden, 2), torch.nn.Tanh())
        self.log_std = torch.nn.Parameter(torch.zeros(2))

    def forward(self, lidar, target, mask):
        mean = self.net(torch.cat([lidar, target, mask], dim=1))
        return mean, self.log_std.exp().expand_as(mean)


class BatchedRollout:
    def __init__(self, env, policy=None, seed=0, update_norm=True):
        self.env = env
        dev = env.device
        self.policy = (policy or StandInPolicy()).to(dev)
        self.norm = G.BatchedStateNorm(device=dev)
        self.planner = G.BatchedRsPlanner(env.n, device=dev)
        self.gen = torch.Generator(device=dev)
        self.gen.manual_seed(seed)
        self.update_norm = update_norm
        self.episodes = torch.zeros(env.n, dtype=torch.int64, device=dev)
        self.successes = torch.zeros(env.n, dtype=torch.int64, device=dev)
        self.steps = 0
        env.reset_obs()

    @torch.no_grad()
    def step(self):
        env = self.env
        obs = {'lidar': env.lidar.to(torch.float32), 'target': env.target.to(torch.float32)}
        if self.update_norm:
            self.norm.update(obs)
        nz = self.norm.normalize(obs)
        mean, std = self.policy(nz['lidar'].float(), nz['target'].float(), env.action_mask.float())
        rl_action, _ = G.choose_action(mean, std, env.action_mask, self.gen)          # mask-weighted discrete sampling
        plan_action, executing = self.planner.get_actions()                          # replay of a found RS path
        action = torch.where(executing.unsqueeze(1), plan_action, rl_action).to(env.action_dtype).contiguous()
        env.step(action, auto_reset=True)
        done = env.done.bool()
        self.episodes += done
        self.successes += (env.status == 2)
        self.planner.reset(done)                                                     # ParkingAgent.reset at episode end
        self.planner.set_paths(env.rs_word, env.rs_lengths)                          # info['path_to_dest'] (:212-213)
        self.steps += 1
        return action

    def stats(self):
        ep = int(self.episodes.sum().item())
        return {'steps': self.steps, 'episodes': ep, 'success_rate': float(self.successes.sum().item()) / max(ep, 1),
                'executing_rs': float(self.planner.executing.float().mean().item())}


class TransitionRing:
    """[N, T] device ring of (normalised obs, action, log_prob, reward, done): the batched ReplayMemory
    (src/model/replay_memory.py:6-49).  A column is written in two halves -- what the agent saw and did before the env
    step, what the env answered after it."""

    def __init__(self, n, horizon, keys, device, img_shape=(3, 64, 64)):
        self.n, self.T, self.device = n, horizon, torch.device(device)
        shp = {'lidar': (120,), 'target': (5,), 'action_mask': (42,), 'img': tuple(img_shape)}
        self.obs = {k: torch.zeros((n, horizon) + shp[k], dtype=torch.uint8 if k == 'img' else torch.float32, device=self.device)
                    for k in keys}
        self.action = torch.zeros((n, horizon, 2), dtype=torch.float32, device=self.device)
        self.log_prob = torch.zeros((n, horizon, 2), dtype=torch.float32, device=self.device)
        self.reward = torch.zeros((n, horizon), dtype=torch.float32, device=self.device)
        self.done = torch.zeros((n, horizon), dtype=torch.float32, device=self.device)
        self.head, self.size = 0, 0

    def write_before(self, nobs, action, log_prob):
        t = self.head
        for k, buf in self.obs.items():
            buf[:, t].copy_(nobs[k])
        self.action[:, t].copy_(action)
        self.log_prob[:, t].copy_(log_prob)

    def write_after(self, reward, done):
        t = self.head
        self.reward[:, t].copy_(reward)
        self.done[:, t].copy_(done)
        self.head = (t + 1) % self.T
        self.size = min(self.size + 1, self.T)

    def columns(self):
        """column indices oldest -> newest"""
        return (torch.arange(self.size, device=self.device) + (self.head - self.size)) % self.T

    def ordered(self):
        idx = self.columns()
        if self.size == self.T and self.head == 0:                      # the PPO case: no gather needed
            return self.obs, self.action, self.reward, self.done, self.log_prob
        return ({k: v[:, idx] for k, v in self.obs.items()}, self.action[:, idx], self.reward[:, idx], self.done[:, idx],
                self.log_prob[:, idx])

    def sample(self, batch_size, last_obs, generator=None, index=None):
        """uniform (scene, time) transitions like ReplayMemory.sample (:33-35); the observation after the newest column
        is `last_obs` (the one the agent is about to act on).  index=(s, j): the scene and the age (0: the oldest column) of every
        item instead of the two draws -- tests feed this ring and DeviceTransitionRing the same choices."""
        idx = self.columns()
        if index is None:
            s = torch.randint(self.n, (batch_size,), device=self.device, generator=generator)
            j = torch.randint(self.size, (batch_size,), device=self.device, generator=generator)
        else:
            s, j = (torch.as_tensor(x, device=self.device).long() for x in index)
        t = idx[j]
        newest = j == self.size - 1
        tn = idx[torch.clamp(j + 1, max=self.size - 1)]
        nxt = {}
        for k, v in self.obs.items():
            a = v[s, tn]
            m = newest.view((-1,) + (1,) * (a.dim() - 1))
            nxt[k] = torch.where(m, last_obs[k][s].to(a.dtype), a)
        return {'obs': {k: v[s, t] for k, v in self.obs.items()}, 'next_obs': nxt, 'action': self.action[s, t],
                'reward': self.reward[s, t], 'done': self.done[s, t]}

    def clear(self):
        self.head, self.size = 0, 0


def _mix64(z):
    """splitmix64's finaliser over uint64 arrays (hope_chooser_core.h's ch_mix64)"""
    z = z + np.uint64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def ring_draws(seed, counter, batch, n, size):
    """the counter-based draws of hope_ring_core.h restated in numpy: -> (s, j) int32 [batch], the scene (0 .. n-1) and the age
    (0 .. size-1) of every batch item for (seed, counter)"""
    with np.errstate(over='ignore'):
        key = _mix64(_mix64(np.array([int(seed) & (2 ** 64 - 1)], dtype=np.uint64)) ^ np.uint64(int(counter) & (2 ** 64 - 1)))
        b = np.arange(batch, dtype=np.uint64)
        out = []
        for d, rng in ((0, n), (1, size)):
            x = _mix64(key ^ (np.uint64(2) * b + np.uint64(d)))
            out.append((((x >> np.uint64(32)) * np.uint64(rng)) >> np.uint64(32)).astype(np.int32))
    return out[0], out[1]


class DeviceTransitionRing:
    """TransitionRing's surface over the library's transition ring (include/hope_env.h "the transition ring"; rule:
    csrc/hope_ring_core.h): write_before is ONE k_ring_before launch, write_after one k_ring_after launch -- with `status` two, and
    the step's episodes, successes and reward sum are tallied into `counts` (int64 [2]) and `reward_sum` (float64 [1]) on the
    device -- and sample one k_ring_sample launch.  The tensors are this object's, in TransitionRing's layout, and hold the same
    words.  The image key stays torch code (one large copy_ per push, a gather from `idx` per batch).  On an env without the library
    (CPU tensors; tests/fake_env.OracleEnv) the same runs on the host through hope_ring_*_host: the rule is one source for both.
    sample's draws are counter-based, keyed by `seed` and the number of draws so far (`counter`), not torch.randint's stream; the
    tensors it returns for a batch size are persistent and overwritten by the next call with that size."""
    CORE = ('lidar', 'target', 'action_mask')

    def __init__(self, env, horizon, keys, seed=0, img_shape=(3, 64, 64)):
        self.env, self.n, self.T, self.device = env, env.n, horizon, torch.device(env.device)
        missing = [k for k in self.CORE if k not in keys]
        if missing:
            raise ValueError(f'DeviceTransitionRing needs the observation keys {self.CORE}, missing {missing}')
        n, dev = self.n, self.device
        shp = {'lidar': (120,), 'target': (5,), 'action_mask': (42,), 'img': tuple(img_shape)}
        self.obs = {k: torch.zeros((n, horizon) + shp[k], dtype=torch.uint8 if k == 'img' else torch.float32, device=dev) for k in keys}
        self.action = torch.zeros((n, horizon, 2), dtype=torch.float32, device=dev)
        self.log_prob = torch.zeros((n, horizon, 2), dtype=torch.float32, device=dev)
        self.reward = torch.zeros((n, horizon), dtype=torch.float32, device=dev)
        self.done = torch.zeros((n, horizon), dtype=torch.float32, device=dev)
        self.counts = torch.zeros(2, dtype=torch.int64, device=dev)
        self.reward_sum = torch.zeros(1, dtype=torch.float64, device=dev)
        self.head, self.size = 0, 0
        self.seed, self.counter = seed, 0
        self.on_device = hasattr(env, 'ring_before')
        if self.on_device:
            env.enable_ring()
        else:
            self._lib = G._host_library(dev, 'ring_before')
        self._desc = L.ring_desc('DeviceTransitionRing', dev, n, horizon, lidar=self.obs['lidar'], target=self.obs['target'],
                                 action_mask=self.obs['action_mask'], action=self.action, log_prob=self.log_prob, reward=self.reward, done=self.done)
        self._out = {}                                # batch size -> (tensors, descriptor)

    @staticmethod
    def _f32(x):
        return x.detach().to(torch.float32).contiguous()

    def write_before(self, nobs, action, log_prob):
        t = self.head
        x = [self._f32(nobs[k]) for k in self.CORE] + [self._f32(action), self._f32(log_prob)]
        if self.on_device:
            self.env.ring_before(self._desc, t, *x)
        else:
            arg = partial_arg('hope_ring_before_host', self.device)
            ptrs = [arg(k, v, torch.float32, (self.n, w)) for k, v, w in zip(('lidar', 'target', 'mask', 'action', 'log_prob'), x, (120, 5, 42, 2, 2))]
            L.check(self._lib.hope_ring_before_host(self._desc, t, *ptrs), 'hope_ring_before_host')
        if 'img' in self.obs:
            self.obs['img'][:, t].copy_(nobs['img'])

    def write_after(self, reward, done, status=None):
        """status (int32 [n], the env's): the step is also tallied into `counts` and `reward_sum`"""
        t = self.head
        reward = reward.detach().contiguous()
        if reward.dtype not in (torch.float32, torch.float64):
            reward = reward.to(torch.float32)
        done = done.detach().contiguous()
        if done.dtype not in (torch.uint8, torch.bool):
            done = (done != 0).to(torch.uint8)
        tally = (None, None, None) if status is None else (status.detach().to(torch.int32).contiguous(), self.counts, self.reward_sum)
        if self.on_device:
            self.env.ring_after(self._desc, t, reward, done, *tally)
        else:
            arg = partial_arg('hope_ring_after_host', self.device)
            ptrs = [arg('status', tally[0], torch.int32, (self.n,), optional=True), arg('counts', tally[1], torch.int64, (2,), optional=True),
                    arg('reward_sum', tally[2], torch.float64, (1,), optional=True)]
            L.check(self._lib.hope_ring_after_host(self._desc, t, arg('reward', reward, (torch.float32, torch.float64), (self.n,)),
                                                   int(reward.dtype == torch.float64), arg('done', done, (torch.uint8, torch.bool), (self.n,)), *ptrs),
                    'hope_ring_after_host')
        self.head = (t + 1) % self.T
        self.size = min(self.size + 1, self.T)

    columns = TransitionRing.columns
    ordered = TransitionRing.ordered

    def _outputs(self, batch):
        if batch not in self._out:
            dev, f = self.device, torch.float32
            t = {'obs_lidar': torch.zeros((batch, 120), dtype=f, device=dev), 'obs_target': torch.zeros((batch, 5), dtype=f, device=dev),
                 'obs_mask': torch.zeros((batch, 42), dtype=f, device=dev), 'next_lidar': torch.zeros((batch, 120), dtype=f, device=dev),
                 'next_target': torch.zeros((batch, 5), dtype=f, device=dev), 'next_mask': torch.zeros((batch, 42), dtype=f, device=dev),
                 'action': torch.zeros((batch, 2), dtype=f, device=dev), 'reward': torch.zeros(batch, dtype=f, device=dev),
                 'done': torch.zeros(batch, dtype=f, device=dev), 'idx': torch.zeros((batch, 3), dtype=torch.int32, device=dev)}
            self._out[batch] = (t, L.ring_batch_desc('DeviceTransitionRing.sample', dev, batch, **t))
        return self._out[batch]

    def sample(self, batch_size, last_obs, generator=None, index=None):
        """TransitionRing.sample's dict plus 'idx' (int32 [batch, 3]: scene, column, next column or -1 where next_obs is last_obs).
        index=(s, j): the scene and the age of every item (a pair out of range gives a zero row with idx -1); None: the counter-based
        draws of `ring_draws(seed, counter, ...)`, and the counter moves on.  `generator` is not used."""
        if self.size < 1:
            raise ValueError('sample from an empty ring')
        t, desc = self._outputs(batch_size)
        last = [self._f32(last_obs[k]) for k in self.CORE]
        if index is None:
            s = j = None
            counter = self.counter
            self.counter += 1
        else:
            s, j = (torch.as_tensor(x, device=self.device).to(torch.int32).contiguous() for x in index)
            counter = 0
        if self.on_device:
            self.env.ring_sample(self._desc, self.head, self.size, batch_size, desc, *last, s=s, j=j, seed=self.seed, counter=counter)
        else:
            arg = partial_arg('hope_ring_sample_host', self.device)
            ptrs = [arg(k, v, torch.float32, (self.n, w)) for k, v, w in zip(('last_lidar', 'last_target', 'last_mask'), last, (120, 5, 42))]
            L.check(self._lib.hope_ring_sample_host(self._desc, self.head, self.size, batch_size, arg('s', s, torch.int32, (batch_size,), optional=True),
                                                    arg('j', j, torch.int32, (batch_size,), optional=True), L.seed64(self.seed), L.seed64(counter), *ptrs, desc),
                    'hope_ring_sample_host')
        obs = {'lidar': t['obs_lidar'], 'target': t['obs_target'], 'action_mask': t['obs_mask']}
        nxt = {'lidar': t['next_lidar'], 'target': t['next_target'], 'action_mask': t['next_mask']}
        if 'img' in self.obs:                         # the image key: gathered in torch from the kernel's indices
            ix = t['idx'].long()
            sc, tc, tn = ix[:, 0].clamp(min=0), ix[:, 1].clamp(min=0), ix[:, 2]
            img = self.obs['img']
            obs['img'] = img[sc, tc]
            newest = ((tn < 0) & (ix[:, 0] >= 0)).view(-1, 1, 1, 1)
            nxt['img'] = torch.where(newest, last_obs['img'][sc].to(img.dtype), img[sc, tn.clamp(min=0)])
        return {'obs': {k: obs[k] for k in self.obs}, 'next_obs': {k: nxt[k] for k in self.obs}, 'action': t['action'], 'reward': t['reward'],
                'done': t['done'], 'idx': t['idx']}

    def clear(self):
        self.head, self.size = 0, 0


def partial_arg(call, device):
    """_lib.tensor_arg for one call and device: arg(name, x, dtype, shape, optional=False)"""
    def arg(name, x, dtype, shape, optional=False):
        return L.tensor_arg(call, name, x, dtype, shape, device, optional)
    return arg


def make_ring(ring, env, horizon, keys, seed):
    """the trainers' `ring` argument: None -- today's TransitionRing (torch copies and gathers); 'device' -- a DeviceTransitionRing"""
    if ring is None:
        return TransitionRing(env.n, horizon, keys, env.device)
    if ring != 'device':
        raise ValueError(f"ring must be None or 'device', not {ring!r}")
    return DeviceTransitionRing(env, horizon, keys, seed=seed)


class HopeRollout:
    def __init__(self, env, agent, horizon, use_mask=True, seed=0, use_planner=True, fresh_scenes=False, pool_refresher=None,
                 defer_rs=True, curriculum=None, chooser=None, obs_norm=None, ring=None, actor=None, img_encoder=None):
        """defer_rs: step the env with two completion points (HOPE_DEFER_RS): the next policy forward is enqueued as soon as the
        observation is written, the planner reads rs_word / rs_lengths (after ParkingBatch.wait_rs) just before its override --
        the same actions as with the joined step, the forward overlaps the Reeds-Shepp kernels.
        fresh_scenes: finished episodes continue on a NEW map drawn from the env's device-resident scene pool
        (ParkingBatch.set_pool / set_dlp_cases), as the reference's loop does with `env.reset(...)`; otherwise on the same map.
        pool_refresher: a `scene_gen.PoolRefresher` (host generator + upload) or `scene_gen.DevicePoolRefresher` (lots drawn on the
        device); the trainers poll it after every update, so the pool of generated lots is
        replaced by new ones in the background (asynchronous upload, no synchronisation with the step loop).
        use_planner: True -- the torch planner (agent_glue.BatchedRsPlanner); 'device' -- the library's planner
        (agent_glue.DeviceRsPlanner): its bookkeeping and the pop are ONE k_plan launch per step that waits for the step's search on
        the device (`planner_step(step=...)`), with no wait_rs, no `.any()` and no boolean indexing, so the host never stops on the
        search result; the same actions as True.  False / None: no planner.
        curriculum: None, or dict(update_every=K, **rule parameters) -- the reference's SceneChoose / DlpCaseChoose
        (train_HOPE_sac.py:23-97) on the device: the env tallies every finished episode's outcome per scene type / Dragon-Lake case
        after each step and rebuilds its weighted draw lists every K steps (hope_amd.curriculum.CurriculumDriver); needs
        fresh_scenes (ValueError without).  Measured cost at 65 536 scenes: ~8 % per step.  None: no call at all.
        chooser: None -- the mask-weighted sampling, the planner's override and the log-probability are torch code (agent_glue.
        choose_action, torch.multinomial); 'device' -- one k_choose launch per step (agent_glue.DeviceActionChooser; counter-based
        draws keyed by `seed`, not torch.multinomial's stream), whose env-typed action tensor goes straight into the step.  Used
        where the mask is (use_mask); the plain Gaussian sample and the uniform exploration are not its business.
        obs_norm: None -- the agent's BatchedStateNorm (torch code: `agent.observe` after the step, `_norm_obs` in the next `act`);
        'device' -- the agent's state_norm is swapped for an agent_glue.DeviceStateNorm that takes over its statistics, and the two
        become ONE update_and_normalize call after the step (three launches), whose float32 result is handed to the next `act`.  The
        fold's arithmetic order is fixed there, so the statistics differ from the torch path's in the last bits.
        ring: None -- TransitionRing: the push is seven strided copy_ launches, the tally of episodes, successes and rewards about
        eight more, a SAC batch about thirty; 'device' -- DeviceTransitionRing: one launch for the before half, two for the after half
        with the tally in it (the totals live in the ring: `ring.counts`, `ring.reward_sum`), one for a batch (counter-based draws
        keyed by `seed`, not torch.randint's stream).  The ring's tensors hold the same words either way.
        actor: None -- the actor's inference forward is the torch module (about a hundred launches per step; the agent's fast-policy
        levers apply); 'device' -- `agent.device_actor` becomes an agent_glue.DeviceActor over `env`: one fused launch per step
        (k_policy_forward), the parameters re-packed by one more launch after every update.  The means differ from the torch
        forward's by float32 rounding.  The forwards inside the agent's update stay torch's.
        img_encoder: None -- with an image the actor's image token is computed by the torch encoder (MIOpen convolutions); 'device' --
        the DeviceActor sends the env's uint8 image through an agent_glue.DeviceImgEncoder (two launches: k_imgenc_conv,
        k_imgenc_head).  Only with actor='device' and an agent whose actor takes an image (ValueError otherwise)."""
        self.chooser = G.make_chooser(chooser, env, seed)
        self.device_actor = G.make_actor(actor, env, agent, img_encoder=img_encoder)
        self.obs_norm = G.make_obs_norm(obs_norm, env, agent)
        self._nobs = None                             # device norm: the normalised observation the next act takes
        self.curriculum = None
        if curriculum is not None:
            if not fresh_scenes:
                raise ValueError('curriculum needs fresh_scenes=True: it reweights the draws of new maps, and without them nothing '
                                 'reads its lists')
            from .curriculum import CurriculumDriver
            self.curriculum = CurriculumDriver(env, **dict(curriculum))
        self.env, self.agent, self.use_mask, self.fresh = env, agent, use_mask, fresh_scenes
        self.refresher = pool_refresher
        self.seed = seed
        self.defer_rs = bool(defer_rs) and hasattr(env, 'wait_rs')
        self._plan_pending = False                    # the planner has not yet seen the last step's done / RS outputs
        self._rs_step = None                          # hope_env_last_step() of the deferred step whose search the planner waits for
        dev = env.device
        self.ring = make_ring(ring, env, horizon, agent.keys, seed)
        self._device_ring = isinstance(self.ring, DeviceTransitionRing)
        if use_planner == 'device':
            self.planner = G.DeviceRsPlanner(env)
        elif use_planner is True or use_planner == 1:
            self.planner = G.BatchedRsPlanner(env.n, device=dev)
        elif not use_planner:
            self.planner = None
        else:
            raise ValueError(f"use_planner must be True, False or 'device', not {use_planner!r}")
        self._device_planner = isinstance(self.planner, G.DeviceRsPlanner)
        self.gen = torch.Generator(device=dev)
        self.gen.manual_seed(seed)
        self.episodes = torch.zeros((), dtype=torch.int64, device=dev)
        self.successes = torch.zeros((), dtype=torch.int64, device=dev)
        self.reward_sum = torch.zeros((), dtype=torch.float64, device=dev)
        self.steps = 0
        if fresh_scenes and hasattr(env, 'set_redraw_seed'):
            env.set_redraw_seed(seed * 1000003 + 17)
        env.reset_obs()
        if self.obs_norm is not None:
            self._nobs = self._fold(self._raw_obs())
        else:
            agent.observe(self._raw_obs())

    def _agent_obs(self, raw, nz):
        """what `_norm_obs` returns, with lidar / target from the device norm; mask and image pass through as there"""
        o = {k: raw[k] for k in self.agent.keys}
        o['lidar'], o['target'] = nz['lidar'], nz['target']
        o['action_mask'] = o['action_mask'].float()
        return o

    def _fold(self, raw):
        """device norm: observe + _norm_obs of the same observation.  The result lives in the norm's persistent tensors until its
        next normalising call -- the ring copies it in write_before, and last_obs() rewrites the same values."""
        return self._agent_obs(raw, self.obs_norm.update_and_normalize({'lidar': raw['lidar'], 'target': raw['target']}))

    def _raw_obs(self):
        e = self.env
        o = {'lidar': e.lidar, 'target': e.target, 'action_mask': e.action_mask}
        if 'img' in self.agent.keys:
            o['img'] = e.img
        return o

    def _plan(self):
        """the planner's part of ParkingAgent.choose_action: bookkeeping of the last step (its done flags and RS paths), then
        the actions of the scenes that are replaying a path"""
        if self.planner is None:
            return None, None
        if self._device_planner:
            if not self._plan_pending:                              # before the first step: nothing to adopt, every scene idle
                return self.planner.get_actions()
            self._plan_pending = False
            return self.planner.step(step=self._rs_step)            # one launch; waits for that step's search on the device
        if self._plan_pending:
            env = self.env
            if self.defer_rs:
                # the search of THE step whose words the planner is about to read (a newer step would have replaced them: HOPE_ESTATE)
                env.wait_rs(step=self._rs_step) if self._rs_step is not None and hasattr(env, 'last_step') else env.wait_rs()
            self.planner.reset(env.done.bool())                     # ParkingAgent.reset at episode end
            self.planner.set_paths(env.rs_word, env.rs_lengths)     # info['path_to_dest'] -> set_planner_path
            self._plan_pending = False
        return self.planner.get_actions()

    @torch.no_grad()
    def collect_step(self, random_action=False):
        env, agent = self.env, self.agent
        executing = None
        if random_action:
            planned, executing = self._plan()
            action, log_prob, nobs = agent.act(self._raw_obs(), self.use_mask, self.gen, planned, executing, nobs=self._nobs)
        else:
            action, log_prob, nobs = agent.act(self._raw_obs(), self.use_mask, self.gen, plan_fn=self._plan, chooser=self.chooser,
                                               nobs=self._nobs)
        if random_action:                             # train_HOPE_sac.py:196-198: uniform exploration while the memory fills
            rnd = torch.rand(action.shape, device=action.device, generator=self.gen) * 2 - 1
            action = rnd if executing is None else torch.where(executing.unsqueeze(1), action, rnd)
            mean = agent.policy_mean(nobs)
            from .policy import gaussian_log_prob
            log_prob = gaussian_log_prob(mean, agent.log_std.expand_as(mean), action)
        self.ring.write_before(nobs, action, log_prob)              # copies: env.step overwrites the buffers in place
        kw = {'defer_rs': True} if self.defer_rs else {}
        if self.chooser is not None and self.use_mask and not random_action:
            step_action = self.chooser.action_env     # the chooser's own tensor in the env's action dtype, contiguous
        else:
            step_action = action.to(env.action_dtype).contiguous()
        if self.fresh:                                # new map per episode, drawn inside the step kernel (HOPE_AUTO_REDRAW)
            env.step(step_action, auto_reset=True, fresh=True, **kw)
        else:
            env.step(step_action, auto_reset=True, **kw)
        if self.curriculum is not None:               # update_success_record (:215-225), and every K steps the new draw weights
            self.curriculum.after_step()
        if self._device_ring:                         # the after half and the three tallies: two launches
            self.ring.write_after(env.reward, env.done, env.status)
        else:
            self.ring.write_after(env.reward, env.done)
        if self.obs_norm is not None:
            self._nobs = self._fold(self._raw_obs())
        else:
            agent.observe(self._raw_obs())                          # push_memory: state_norm(next_obs, update=True)
        if not self._device_ring:
            done = env.done.bool()
            self.episodes += done.sum()
            self.successes += (env.status == 2).sum()
            self.reward_sum += env.reward.sum(dtype=torch.float64)
        self._plan_pending = self.planner is not None               # (its bookkeeping runs in _plan, before the next override)
        self._rs_step = env.last_step() if (self.defer_rs and hasattr(env, 'last_step')) else None
        self.steps += 1

    def last_obs(self):
        """normalised observation the agent will act on next (value bootstrap / newest next_obs)"""
        if self.obs_norm is not None:                 # normalise only: the observation was folded in after its step
            raw = self._raw_obs()
            return self._agent_obs(raw, self.obs_norm.normalize({'lidar': raw['lidar'], 'target': raw['target']}))
        return self.agent._norm_obs(self._raw_obs())

    def stats(self):
        if self._device_ring:
            (ep, ok), total = self.ring.counts.tolist(), float(self.ring.reward_sum.item())
        else:
            ep, ok, total = int(self.episodes.item()), self.successes.item(), float(self.reward_sum.item())
        out = {'steps': self.steps, 'episodes': ep, 'success_rate': float(ok) / max(ep, 1),
               'mean_reward': total / max(self.steps * self.env.n, 1)}
        if self.curriculum is not None:               # success_rate_<type>, as the reference logs them (:233-235)
            out.update(self.curriculum.stats())
        return out


class PPOTrainer(HopeRollout):
    """train_HOPE_ppo.py:177-213: act -> step -> push; when the buffer is full (`horizon` steps of all scenes,
    the batched `len(memory) % batch_size == 0`) run PPO.update and clear."""

    def __init__(self, env, agent, horizon=16, seed=0, use_planner=True, fresh_scenes=False, pool_refresher=None, defer_rs=True,
                 curriculum=None, chooser=None, obs_norm=None, gae=None, ring=None, minibatch=None, actor=None, img_encoder=None,
                 critics=None, optimizer=None):
        """ring, actor, img_encoder: as HopeRollout.
        optimizer: None -- every optimiser step is torch.optim.Adam.step and the target's soft update agents._soft_update (a chain of
        multi-tensor launches each); 'device' -- the agent's optimisers become agent_glue.DeviceAdams over `env` around the torch
        optimisers they were and `agent.soft_update` an agent_glue.DevicePolyak: one launch of the library's k_optim per call.
        critics: None -- the three no-gradient critic forwards of the agent's advantage block are torch modules (a hundred launches
        each); 'device' -- `agent.device_critics` becomes an agent_glue.DeviceCritics over `env`, the critic and its target: two launches
        of the library's fused kernel (the critics' image encoders stay in torch).
        minibatch: None -- the inner loop of the agent's update is torch code (seven index launches per minibatch, about twenty for the
        loss, as many again in autograd); 'device' -- the agent's `minibatch` becomes an agent_glue.DevicePpoBatch over `env` and this
        trainer's ring (either class): one launch for the gather, two for the loss and its gradients.
        curriculum: as HopeRollout; without an update_every of its own the draw weights are rebuilt after each PPO update
        gae: None -- the agent's advantage block is torch code (a Python loop along the horizon); 'device' -- the agent's `gae` becomes
        an agent_glue.DeviceGae over `env`: GAE, the critic's target and the advantages' normalisation in three launches."""
        self._curriculum_per_update = curriculum is not None and 'update_every' not in curriculum
        if self._curriculum_per_update:
            curriculum = dict(curriculum, update_every=0)
        super().__init__(env, agent, horizon, use_mask=True, seed=seed, use_planner=use_planner, fresh_scenes=fresh_scenes,
                         pool_refresher=pool_refresher, defer_rs=defer_rs, curriculum=curriculum, chooser=chooser, obs_norm=obs_norm, ring=ring,
                         actor=actor, img_encoder=img_encoder)
        self.gae = G.make_gae(gae, env, agent)
        self.device_critics = G.make_critics(critics, env, agent)
        self.minibatch = G.make_ppo_batch(minibatch, env, self.ring)
        if self.minibatch is not None:
            if not hasattr(agent, 'minibatch'):
                raise ValueError("minibatch='device' needs an agent with a minibatch loop (BatchedPPO)")
            agent.minibatch = self.minibatch
        self.optimizers = G.make_optimizers(optimizer, env, agent)
        self.updates = 0

    def step(self):
        self.collect_step()
        if self.ring.size == self.ring.T:
            obs, action, reward, done, log_prob = self.ring.ordered()
            losses = self.agent.update(obs, action, reward, done, log_prob, self.last_obs(), generator=self.gen)
            self.ring.clear()
            self.updates += 1
            if self._curriculum_per_update:
                self.env.curriculum_update()
            if self.refresher is not None:
                self.refresher.poll()
            return losses
        return None


class SACTrainer(HopeRollout):
    """train_HOPE_sac.py:177-221: uniform random actions until the memory is full, then the policy (plain Gaussian
    sample, no action mask), one SAC update every `update_every` env steps on a uniform batch from the ring."""

    def __init__(self, env, agent, horizon=8, update_every=10, seed=0, use_planner=True, learn=True, fresh_scenes=False,
                 pool_refresher=None, defer_rs=True, curriculum=None, chooser=None, obs_norm=None, ring=None, sac_update=None, actor=None,
                 img_encoder=None, critics=None, optimizer=None):
        """actor, img_encoder: as HopeRollout (the policy's mean once the memory is full)
        optimizer: as PPOTrainer: 'device' wraps critic_opt1, critic_opt2, actor_opt and alpha_opt and sends both soft updates through
        one call.
        critics: None -- the update's two target-critic forwards are torch modules; 'device' -- `agent.device_critics` becomes an
        agent_glue.DeviceCritics over `env` and the two targets: one launch of the library's fused kernel for both (their image encoders
        and `_soft_update` stay in torch; the two critics that autograd runs through do too).
        chooser: accepted for symmetry with PPOTrainer; SAC samples without the mask (use_mask=False), where it is not used
        ring: as HopeRollout; with 'device' the batch is one k_ring_sample launch
        sac_update: None -- the agent's update computes the sample, the Q target and the losses in torch and autograd differentiates
        them; 'device' -- the agent's `update_block` becomes an agent_glue.DeviceSacUpdate over `env`: eight launches between the
        network forwards, autograd through the networks only."""
        super().__init__(env, agent, horizon, use_mask=False, seed=seed, use_planner=use_planner, fresh_scenes=fresh_scenes,
                         pool_refresher=pool_refresher, defer_rs=defer_rs, curriculum=curriculum, chooser=chooser, obs_norm=obs_norm, ring=ring,
                         actor=actor, img_encoder=img_encoder)
        self.sac_update = G.make_sac_update(sac_update, env)
        if self.sac_update is not None:
            if not hasattr(agent, 'update_block'):
                raise ValueError("sac_update='device' needs an agent with an update block (BatchedSAC)")
            agent.update_block = self.sac_update
        self.device_critics = G.make_critics(critics, env, agent)
        self.optimizers = G.make_optimizers(optimizer, env, agent)
        self.update_every, self.learn, self.updates = update_every, learn, 0

    def step(self):
        self.collect_step(random_action=self.learn and self.ring.size < self.ring.T)
        if self.learn and self.ring.size == self.ring.T and self.steps % self.update_every == 0:
            batch = self.ring.sample(self.agent.batch_size, self.last_obs(), self.gen)
            self.updates += 1
            if self.refresher is not None and self.updates % 16 == 0:
                self.refresher.poll()
            return self.agent.update(batch)
        return None
