"""Batched evaluator: `eval()` of the reference (src/evaluation/eval_utils.py:16-84, driven by eval_mix_scene.py:86-115) for N
episodes at once -- one evaluation episode per scene slot, all slots stepped together, finished slots frozen.

Per episode, as the reference records them (:28-84): the final status, the step count, the summed wrapper reward and the path
length (sum of the rear-axle displacement per step, :52-53).  The loop keeps the reference's stuck detector (:46-47: when
obs['target'] did not change since the previous step the action is replaced by `env.action_space.sample()`, a uniform draw from
the PHYSICAL action box that the wrapper then clips to [-1, 1]) and hands found Reeds-Shepp paths to the planner (:55-56).
`summarize` produces the numbers result.txt holds (:131-149): success rate, steps of the successful episodes, and per map level
(`env.map.map_level`, :69) success rate, steps and the path length of the episodes shorter than 200 steps; OUTBOUND episodes
count 200 steps in the per-case step record (:73-76).  `BatchedEvaluator.run` returns one record per episode; with
torch.distributed initialised the records of all ranks are gathered (hope_amd.dist.gather_eval_stats: one all-gather).
`run(levels=True)` adds the map level of every episode's lot, labelled on the device (`ParkingBatch.map_levels`, k_map_level), so
that the per-level blocks exist for device-drawn Dragon-Lake lots too.  `BatchedEvaluator(tracker='device')` keeps the per-episode
tally in the library (agent_glue.DeviceEvalTracker: k_eval_override / k_eval_track) instead of the torch one-liners of `run`."""
import numpy as np
import torch

from . import agent_glue as G
from . import dist as D
from . import tables as T

LEVELS = ('Normal', 'Complex', 'Extrem', 'dlp')          # map_level labels; DLP lots get get_map_level's label when asked
TOLERANT_TIME = 200


class BatchedEvaluator:
    def __init__(self, env, agent, post_proc_action=True, use_planner=True, seed=0, chooser=None, obs_norm=None, tracker=None,
                 poll_every=8, actor=None, img_encoder=None):
        """agent: a hope_amd.agents agent (`act(obs, use_mask, generator, planned, executing)`); post_proc_action: PPO's
        mask-weighted choose_action (eval_utils.py:42-43) instead of the plain sample (:44-45).
        chooser: None, or 'device' -- with post_proc_action the choice, the planner's override and the log-probability are one
        k_choose launch per step (agent_glue.DeviceActionChooser; counter-based draws keyed by `seed`).  The stuck detector's
        random action is applied after it, as before.
        obs_norm: None, or 'device' -- the agent's state_norm is swapped for an agent_glue.DeviceStateNorm with the same statistics:
        the normalisation in `act` is then one k_obsnorm_apply launch.  Evaluation folds nothing in, as before.
        tracker: None, or 'device' -- the bookkeeping of the loop (stuck detector and its random action, step count, summed reward,
        path length, final status, alive mask, the hiding of frozen slots' Reeds-Shepp words) is one launch before and one after the
        env step (agent_glue.DeviceEvalTracker: k_eval_override, k_eval_track), and the host asks whether an episode is still running
        only every `poll_every` steps instead of every step; steps taken with every slot frozen change nothing.  The stuck
        detector's draws are then counter-based, keyed by `seed` (`stuck_uniforms`), not the generator's.
        actor: None, or 'device' -- the actor's forward in `act` is one fused launch of the library (agent_glue.DeviceActor, set as
        `agent.device_actor`) instead of the torch module's hundred; the means differ by float32 rounding.
        img_encoder: None, or 'device' -- with actor='device' and an agent whose actor takes an image, the image token comes from the
        library's image encoder (agent_glue.DeviceImgEncoder) instead of the torch convolutions; ValueError otherwise."""
        self.env, self.agent, self.use_mask = env, agent, bool(post_proc_action)
        self.chooser = G.make_chooser(chooser, env, seed)
        self.obs_norm = G.make_obs_norm(obs_norm, env, agent)
        self.device_actor = G.make_actor(actor, env, agent, img_encoder=img_encoder)
        self.tracker = G.make_tracker(tracker, env, seed)
        self.poll_every = max(1, int(poll_every))
        if use_planner == 'device':          # the library's planner: one k_plan launch per step (agent_glue.DeviceRsPlanner)
            self.planner = G.DeviceRsPlanner(env)
        else:
            self.planner = G.BatchedRsPlanner(env.n, device=env.device) if use_planner else None
        self._device_planner = use_planner == 'device'
        self.gen = torch.Generator(device=env.device)
        self.gen.manual_seed(seed)
        lo = torch.tensor([T.VALID_STEER[0], T.VALID_SPEED[0]], dtype=torch.float64, device=env.device)
        hi = torch.tensor([T.VALID_STEER[1], T.VALID_SPEED[1]], dtype=torch.float64, device=env.device)
        self._lo, self._span = lo, hi - lo

    def _obs(self):
        e = self.env
        o = {'lidar': e.lidar, 'target': e.target, 'action_mask': e.action_mask}
        if 'img' in self.agent.keys:
            o['img'] = e.img
        return o

    def _stuck_uniform(self, step):
        """the stuck detector's uniforms of episode step `step`: float64 [n, 2] in [0, 1)"""
        return torch.rand((self.env.n, 2), device=self.env.device, dtype=torch.float64, generator=self.gen)

    def _run_tracked(self, max_steps):
        """the loop of `run` with the bookkeeping on the tracker -> float32 [n, 4]"""
        env, agent, tr = self.env, self.agent, self.tracker
        tr.begin()
        pending = None
        for step in range(max_steps):
            if step % self.poll_every == 0 and not tr.any_alive():       # the loop's only host synchronisation
                break
            if self._device_planner and pending is not None:
                planned, executing = self.planner.step(*pending)
            else:
                planned, executing = self.planner.get_actions() if self.planner is not None else (None, None)
            action, _, _ = agent.act(self._obs(), self.use_mask, self.gen, planned, executing, chooser=self.chooser)
            action = action.contiguous()
            tr.override(action)                                       # stuck detector (:46-47), in place
            env.step(action.to(env.action_dtype).contiguous(), active=tr.alive)
            tr.track()
            if self.planner is not None:
                if self._device_planner:
                    pending = (tr.done, tr.word, env.rs_lengths)
                else:
                    self.planner.reset(tr.done.bool())
                    self.planner.set_paths(tr.word, env.rs_lengths)
        return tr.records()

    @torch.no_grad()
    def run(self, max_steps=TOLERANT_TIME + 2, gather=True, levels=False):
        """one episode per scene slot from the slots' current maps (the caller has uploaded / drawn them and not stepped yet).
        -> float32 [n_total, 4]: status, steps, reward, path length.
        levels=True: the slots' maps are labelled right after the first observation (`env.map_levels()`: get_map_level on the
        device, eval_utils.py:69) -> [n_total, 5] with the level (0 Normal, 1 Complex, 2 Extrem) as the fifth column, gathered
        over the ranks like the rest; `self.levels` keeps this rank's labels (uint8 [n])."""
        env, agent = self.env, self.agent
        n, dev = env.n, env.device
        env.reset_obs()                                               # env.reset(i + 1) -> first observation (:32)
        if levels:
            self.levels = env.map_levels().clone()                    # env.map.map_level (:69), before the first step
        if self.planner is not None:
            self.planner.reset()                                      # agent.reset() (:33)
        if self.tracker is not None:
            rec = self._run_tracked(max_steps)
            if gather:
                rec = D.gather_eval_stats(rec[:, 0], rec[:, 1], rec[:, 2], rec[:, 3])
                return D.gather_eval_levels(rec, self.levels) if levels else rec
            rec = rec.clone()
            return torch.cat([rec, self.levels.to(torch.float32).reshape(-1, 1)], dim=1) if levels else rec
        alive = torch.ones(n, dtype=torch.bool, device=dev)
        steps = torch.zeros(n, dtype=torch.int32, device=dev)
        total = torch.zeros(n, dtype=torch.float64, device=dev)
        path = torch.zeros(n, dtype=torch.float64, device=dev)
        status = torch.ones(n, dtype=torch.int32, device=dev)
        last_xy = env.pose[:, :2].clone()
        last_target = env.target.clone()                              # last_obs = obs['target'] (:39)
        first = True
        pending = None                                                # device planner: (done, word, lengths) of the last step
        for step in range(max_steps):
            if not bool(alive.any()):
                break
            if self._device_planner and pending is not None:       # reset(done) + set_paths + get_actions of the last step, fused
                planned, executing = self.planner.step(*pending)
            else:
                planned, executing = self.planner.get_actions() if self.planner is not None else (None, None)
            action, _, _ = agent.act(self._obs(), self.use_mask, self.gen, planned, executing, chooser=self.chooser)
            # stuck detector (:46-47): the very first comparison is obs['target'] with itself -> always a random first action
            same = torch.ones(n, dtype=torch.bool, device=dev) if first else (env.target == last_target).all(dim=1)
            first = False
            rnd = self._lo + self._span * self._stuck_uniform(step)
            action = torch.where(same.unsqueeze(1), rnd.clamp(-1, 1).to(action.dtype), action)
            last_target = env.target.clone()
            env.step(action.to(env.action_dtype).contiguous(), active=alive.to(torch.uint8))
            steps += alive.to(torch.int32)
            total += torch.where(alive, env.reward.double(), torch.zeros_like(total))
            xy = env.pose[:, :2]
            path += torch.where(alive, (xy - last_xy).norm(dim=1), torch.zeros_like(path))
            last_xy = xy.clone()
            done = alive & env.done.bool()
            status = torch.where(done, env.status, status)
            if self.planner is not None:
                word = env.rs_word.clone()                         # info['path_to_dest'] -> agent.set_planner_path (:55-56)
                word[~(alive & ~done), 6] = 0                      # (frozen slots keep stale outputs)
                if self._device_planner:
                    pending = (done, word, env.rs_lengths)
                else:
                    self.planner.reset(done)
                    self.planner.set_paths(word, env.rs_lengths)
            alive = alive & ~done
        rec = torch.stack([status.float(), steps.float(), total.float(), path.float()], dim=1)
        if gather:
            rec = D.gather_eval_stats(status, steps, total.float(), path.float())
            return D.gather_eval_levels(rec, self.levels) if levels else rec
        return torch.cat([rec, self.levels.to(torch.float32).reshape(-1, 1)], dim=1) if levels else rec


_STUCK_TAG = 0x4556414C54524B31                         # csrc/hope_evaltrack_core.h's ET_TAG


def _mix64(z):
    """the splitmix64 finaliser over numpy uint64 (wrapping arithmetic)"""
    z = z + np.uint64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def stuck_uniforms(seed, step, n, scene0=0):
    """the tracker's counter-based draw (csrc/hope_evaltrack_core.h) restated in numpy: float64 [n, 2] in [0, 1), row i =
    the uniforms of scene scene0 + i at episode step `step` under `seed`"""
    with np.errstate(over='ignore'):
        key = _mix64(_mix64(np.array([(int(seed) ^ _STUCK_TAG) & (2 ** 64 - 1)], dtype=np.uint64)) ^ np.uint64(int(step) & (2 ** 64 - 1)))
        idx = np.uint64(2) * (np.uint64(scene0) + np.arange(n, dtype=np.uint64))[:, None] + np.arange(2, dtype=np.uint64)[None, :]
        x = _mix64(key ^ idx)
    return (x >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def summarize(records, levels=None):
    """records [n, 4] (status, steps, reward, path length) [+ levels: sequence of n map-level labels] -> the numbers of
    result.txt (eval_utils.py:131-149).  Records with a fifth column (`BatchedEvaluator.run(levels=True)`) carry their labels:
    without `levels` the blocks are named after it ('Normal' / 'Complex' / 'Extrem')."""
    r = records.detach().cpu().numpy() if torch.is_tensor(records) else np.asarray(records)
    if levels is None and r.ndim == 2 and r.shape[1] >= 5:
        from .map_level import LEVEL_NAMES
        levels = [LEVEL_NAMES[int(v)] for v in r[:, 4]]
    status, steps, reward, plen = r[:, 0].astype(int), r[:, 1], r[:, 2], r[:, 3]
    succ = status == 2

    def block(sel, per_case):
        # per_case: the per-case / all-episodes `step_record`, in which an OUTBOUND episode counts 200 steps (eval_utils.py:73-76);
        # the per-level "step num" of result.txt comes from step_num_level = the raw step_num (:71, :143)
        s = sel & succ
        step_rec = np.where(status[sel] == 4, float(TOLERANT_TIME), steps[sel]) if per_case else steps[sel]
        short = sel & (steps < TOLERANT_TIME)
        return {'episodes': int(sel.sum()), 'success_rate': float(succ[sel].mean()) if sel.any() else 0.0,
                'step_num_mean': float(step_rec.mean()) if sel.any() else 0.0, 'step_num_std': float(step_rec.std()) if sel.any() else 0.0,
                'success_step_mean': float(steps[s].mean()) if s.any() else 0.0,
                'path_length_mean': float(plen[short].mean()) if short.any() else 0.0,
                'path_length_std': float(plen[short].std()) if short.any() else 0.0,
                'reward_mean': float(reward[sel].mean()) if sel.any() else 0.0}
    out = {'all': block(np.ones(len(r), bool), True)}
    if levels is not None:
        lv = np.asarray(levels)
        for k in sorted(set(lv.tolist())):
            out[str(k)] = block(lv == k, False)
    return out
