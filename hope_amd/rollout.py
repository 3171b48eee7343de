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
import torch

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

    def sample(self, batch_size, last_obs, generator=None):
        """uniform (scene, time) transitions like ReplayMemory.sample (:33-35); the observation after the newest column
        is `last_obs` (the one the agent is about to act on)."""
        idx = self.columns()
        s = torch.randint(self.n, (batch_size,), device=self.device, generator=generator)
        j = torch.randint(self.size, (batch_size,), device=self.device, generator=generator)
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


class HopeRollout:
    def __init__(self, env, agent, horizon, use_mask=True, seed=0, use_planner=True, fresh_scenes=False, pool_refresher=None,
                 defer_rs=True, curriculum=None, chooser=None, obs_norm=None):
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
        fold's arithmetic order is fixed there, so the statistics differ from the torch path's in the last bits."""
        self.chooser = G.make_chooser(chooser, env, seed)
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
        self.ring = TransitionRing(env.n, horizon, agent.keys, dev)
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
        self.ring.write_after(env.reward, env.done)
        if self.obs_norm is not None:
            self._nobs = self._fold(self._raw_obs())
        else:
            agent.observe(self._raw_obs())                          # push_memory: state_norm(next_obs, update=True)
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
        ep = int(self.episodes.item())
        out = {'steps': self.steps, 'episodes': ep, 'success_rate': float(self.successes.item()) / max(ep, 1),
               'mean_reward': float(self.reward_sum.item()) / max(self.steps * self.env.n, 1)}
        if self.curriculum is not None:               # success_rate_<type>, as the reference logs them (:233-235)
            out.update(self.curriculum.stats())
        return out


class PPOTrainer(HopeRollout):
    """train_HOPE_ppo.py:177-213: act -> step -> push; when the buffer is full (`horizon` steps of all scenes,
    the batched `len(memory) % batch_size == 0`) run PPO.update and clear."""

    def __init__(self, env, agent, horizon=16, seed=0, use_planner=True, fresh_scenes=False, pool_refresher=None, defer_rs=True,
                 curriculum=None, chooser=None, obs_norm=None, gae=None):
        """curriculum: as HopeRollout; without an update_every of its own the draw weights are rebuilt after each PPO update
        gae: None -- the agent's advantage block is torch code (a Python loop along the horizon); 'device' -- the agent's `gae` becomes
        an agent_glue.DeviceGae over `env`: GAE, the critic's target and the advantages' normalisation in three launches."""
        self._curriculum_per_update = curriculum is not None and 'update_every' not in curriculum
        if self._curriculum_per_update:
            curriculum = dict(curriculum, update_every=0)
        super().__init__(env, agent, horizon, use_mask=True, seed=seed, use_planner=use_planner, fresh_scenes=fresh_scenes,
                         pool_refresher=pool_refresher, defer_rs=defer_rs, curriculum=curriculum, chooser=chooser, obs_norm=obs_norm)
        self.gae = G.make_gae(gae, env, agent)
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
                 pool_refresher=None, defer_rs=True, curriculum=None, chooser=None, obs_norm=None):
        """chooser: accepted for symmetry with PPOTrainer; SAC samples without the mask (use_mask=False), where it is not used"""
        super().__init__(env, agent, horizon, use_mask=False, seed=seed, use_planner=use_planner, fresh_scenes=fresh_scenes,
                         pool_refresher=pool_refresher, defer_rs=defer_rs, curriculum=curriculum, chooser=chooser, obs_norm=obs_norm)
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
