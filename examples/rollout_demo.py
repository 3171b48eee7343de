#!/usr/bin/env python3
"""End-to-end batched rollout on one GPU (or one rank per GPU under torch.distributed.run): scenes -> env step
(auto-reset) -> StateNorm -> stand-in policy -> mask-weighted sampling / RS-path replay.
usage: python examples/rollout_demo.py [--scenes 16384] [--steps 200]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from hope_amd import ParkingBatch
from hope_amd import dist as D
from hope_amd.rollout import BatchedRollout
from hope_amd.scenes import SceneSource


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--scenes', type=int, default=16384)
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--unique', type=int, default=1024)
    ap.add_argument('--device-pool', type=int, default=0, metavar='LOTS',
                    help='also run a short PPO loop whose finished episodes draw new maps from a pool of LOTS generated lots that is '
                         'refilled ON THE DEVICE after every update (scene_gen.DevicePoolRefresher: no host generator thread, no upload)')
    ap.add_argument('--curriculum', action='store_true',
                    help='with --device-pool: pick the new maps with the device-side curriculum (SceneChoose / DlpCaseChoose of '
                         'train_HOPE_sac.py: outcomes tallied per scene type, draw weights rebuilt after every PPO update)')
    ap.add_argument('--device-planner', action='store_true',
                    help='also run a short PPO loop and the evaluation with the Reeds-Shepp path replay on the device '
                         "(use_planner='device': one k_plan launch per step instead of the torch planner and its host synchronisations)")
    ap.add_argument('--device-chooser', action='store_true',
                    help='also run a short PPO loop and the evaluation with the masked action choice on the device '
                         "(chooser='device': one k_choose launch per step instead of mask_action_probs, torch.multinomial and gaussian_log_prob)")
    ap.add_argument('--device-norm', action='store_true',
                    help='also run a short PPO loop and the evaluation with the observation normalisation on the device '
                         "(obs_norm='device': k_obsnorm_partial / _merge / _apply per step instead of BatchedStateNorm's torch code)")
    ap.add_argument('--device-gae', action='store_true',
                    help="also run a short PPO loop with the advantage block on the device (gae='device': k_gae_scan / k_gae_merge / "
                         "k_adv_apply per update instead of batched_gae's Python loop along the horizon and _global_mean_std)")
    ap.add_argument('--device-ring', action='store_true',
                    help="also run a short PPO loop with the transition ring on the device (ring='device': k_ring_before / k_ring_after / "
                         'k_ring_tally per step instead of seven strided copy_ launches and the three torch tallies)')
    ap.add_argument('--device-ppo-batch', action='store_true',
                    help="also run a short PPO loop with the minibatch on the device (minibatch='device': k_ppo_gather, then k_ppo_loss / "
                         'k_ppo_merge per minibatch instead of seven index launches, the elementwise loss and autograd through it)')
    ap.add_argument('--device-sac-update', action='store_true',
                    help="also run a short SAC loop with the update's arithmetic on the device (sac_update='device': k_sac_sample, k_sac_critic, "
                         'k_sac_seed, k_sac_policy and k_sac_merge between the network forwards instead of the elementwise lines and autograd '
                         'through them)')
    ap.add_argument('--device-actor', action='store_true',
                    help="also run a short PPO loop with the actor's inference forward on the device (actor='device': one fused "
                         'k_policy_forward launch per step instead of the torch module, k_policy_pack after every update)')
    ap.add_argument('--device-critics', action='store_true',
                    help="also run a short SAC and a short PPO loop with the updates' no-gradient critic forwards on the device "
                         "(critics='device': the two target critics, or the critic and its target, in one k_critic_forward launch instead of "
                         'two torch modules, k_critic_pack of a slot after its net changed)')
    ap.add_argument('--device-optimizer', action='store_true',
                    help="also run a short SAC and a short PPO loop with the optimiser block on the device (optimizer='device': every "
                         'Adam step and every soft update of a target one k_optim launch per 64 tensors instead of torch\'s chain of '
                         'multi-tensor launches; the torch optimisers keep the state)')
    ap.add_argument('--device-img-encoder', action='store_true',
                    help="also run a short PPO loop of an agent WITH the image token on an env that renders the bird's-eye image, the "
                         "actor's forward and its image encoder on the device (actor='device', img_encoder='device': k_imgenc_conv and "
                         'k_imgenc_head on the env\'s uint8 image instead of the MIOpen convolutions, then k_policy_forward)')
    ap.add_argument('--device-eval', action='store_true',
                    help="run the evaluation with its per-episode bookkeeping on the device (tracker='device': k_eval_override and k_eval_track "
                         'per step instead of the torch one-liners, and one host synchronisation every 8 steps instead of every step)')
    ap.add_argument('--eval-levels', action='store_true',
                    help='one more batched evaluation over Dragon-Lake lots DRAWN ON THE DEVICE (jitter, cull, flips per slot), labelled by '
                         'the HIP kernel k_map_level: the per-level block of result.txt for maps that exist on the device only')
    args = ap.parse_args()
    rank, world, local = D.init_from_env()
    dev = f'cuda:{local}'
    src = SceneSource(seed=42 + rank)
    uniq = [src.draw() for _ in range(args.unique)]
    env = ParkingBatch(args.scenes, 128, device=dev)
    env.set_scenes(np.arange(args.scenes), [uniq[i % len(uniq)] for i in range(args.scenes)])
    ro = BatchedRollout(env, seed=rank)
    for _ in range(10):
        ro.step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        ro.step()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    s = ro.stats()
    if rank == 0:
        print(f'{world} rank(s) x {args.scenes} scenes: {args.scenes * world * args.steps / dt / 1e6:.2f} M env+agent steps/s, '
              f'{s["episodes"]} episodes on rank 0, success rate {s["success_rate"]:.3f}, RS replay active {s["executing_rs"]:.3f}')
    if args.device_planner:
        from hope_amd import agents as A
        from hope_amd.rollout import PPOTrainer
        tr = PPOTrainer(env, A.BatchedPPO(device=dev, use_img=False, mini_batch=min(args.scenes, 16384), mini_epoch=1), horizon=4,
                        seed=rank, use_planner='device')
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(16):
            tr.step()
        torch.cuda.synchronize()
        if rank == 0:
            print(f'  device planner: 16 PPO steps ({tr.updates} updates) in {(time.perf_counter() - t0) * 1e3:.1f} ms, '
                  f'RS replay active {float(tr.planner.executing.float().mean()):.3f}')
    if args.device_chooser:
        from hope_amd import agents as A
        from hope_amd.rollout import PPOTrainer
        tr = PPOTrainer(env, A.BatchedPPO(device=dev, use_img=False, mini_batch=min(args.scenes, 16384), mini_epoch=1), horizon=4,
                        seed=rank, use_planner='device' if args.device_planner else True, chooser='device')
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(16):
            tr.step()
        torch.cuda.synchronize()
        if rank == 0:
            flagged = int((tr.chooser.idx >= 64).sum())
            print(f'  device chooser: 16 PPO steps ({tr.updates} updates) in {(time.perf_counter() - t0) * 1e3:.1f} ms, '
                  f'{flagged} degenerate rows in the last step')
    if args.device_norm:
        from hope_amd import agents as A
        from hope_amd.rollout import PPOTrainer
        tr = PPOTrainer(env, A.BatchedPPO(device=dev, use_img=False, mini_batch=min(args.scenes, 16384), mini_epoch=1), horizon=4,
                        seed=rank, use_planner='device' if args.device_planner else True,
                        chooser='device' if args.device_chooser else None, obs_norm='device')
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(16):
            tr.step()
        torch.cuda.synchronize()
        if rank == 0:
            sn = tr.obs_norm
            print(f'  device norm: 16 PPO steps ({tr.updates} updates) in {(time.perf_counter() - t0) * 1e3:.1f} ms, '
                  f"{sn.n_state} observations folded in, mean lidar std {float(sn.std['lidar'].mean()):.3f} m")
    if args.device_gae:
        from hope_amd import agents as A
        from hope_amd.rollout import PPOTrainer
        tr = PPOTrainer(env, A.BatchedPPO(device=dev, use_img=False, mini_batch=min(args.scenes, 16384), mini_epoch=1), horizon=4,
                        seed=rank, use_planner='device' if args.device_planner else True,
                        chooser='device' if args.device_chooser else None, obs_norm='device' if args.device_norm else None, gae='device')
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(16):
            tr.step()
        torch.cuda.synchronize()
        if rank == 0:
            m, s = tr.gae.mean_std()
            print(f'  device gae: 16 PPO steps ({tr.updates} updates) in {(time.perf_counter() - t0) * 1e3:.1f} ms, '
                  f'advantages of the last update: mean {m:.4f}, std {s:.4f} over {int(tr.gae.sums[2])} transitions')
    if args.device_ring:
        from hope_amd import agents as A
        from hope_amd.rollout import PPOTrainer
        tr = PPOTrainer(env, A.BatchedPPO(device=dev, use_img=False, mini_batch=min(args.scenes, 16384), mini_epoch=1), horizon=4,
                        seed=rank, use_planner='device' if args.device_planner else True,
                        chooser='device' if args.device_chooser else None, obs_norm='device' if args.device_norm else None,
                        gae='device' if args.device_gae else None, ring='device')
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(16):
            tr.step()
        torch.cuda.synchronize()
        if rank == 0:
            st = tr.stats()
            print(f'  device ring: 16 PPO steps ({tr.updates} updates) in {(time.perf_counter() - t0) * 1e3:.1f} ms, '
                  f"{st['episodes']} episodes tallied on the device, success rate {st['success_rate']:.3f}, mean reward {st['mean_reward']:.4f}")
    if args.device_ppo_batch:
        from hope_amd import agents as A
        from hope_amd.rollout import PPOTrainer
        tr = PPOTrainer(env, A.BatchedPPO(device=dev, use_img=False, mini_batch=min(args.scenes, 4096), mini_epoch=2), horizon=4,
                        seed=rank, use_planner='device' if args.device_planner else True,
                        chooser='device' if args.device_chooser else None, obs_norm='device' if args.device_norm else None,
                        gae='device' if args.device_gae else None, ring='device' if args.device_ring else None, minibatch='device')
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(16):
            tr.step()
        torch.cuda.synchronize()
        if rank == 0:
            al, cl = tr.agent.last_losses
            print(f'  device ppo batch: 16 PPO steps ({tr.updates} updates) in {(time.perf_counter() - t0) * 1e3:.1f} ms, '
                  f'last minibatch: actor loss {al:.5f}, critic loss {cl:.5f}')
    if args.device_sac_update:
        from hope_amd import agents as A
        from hope_amd.rollout import SACTrainer
        tr = SACTrainer(env, A.BatchedSAC(device=dev, use_img=False, batch_size=min(args.scenes, 4096)), horizon=4, update_every=2, seed=rank,
                        use_planner='device' if args.device_planner else True, obs_norm='device' if args.device_norm else None,
                        ring='device' if args.device_ring else None, sac_update='device')
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        losses = [x for x in (tr.step() for _ in range(16)) if x is not None]
        torch.cuda.synchronize()
        if rank == 0:
            print(f'  device sac update: 16 SAC steps ({tr.updates} updates) in {(time.perf_counter() - t0) * 1e3:.1f} ms, '
                  f'last update: actor loss {losses[-1][0]:.5f}, critic loss {losses[-1][1]:.5f}, temperature {float(tr.agent.alpha):.5f}')
    if args.device_actor:
        from hope_amd import agents as A
        from hope_amd.rollout import PPOTrainer
        tr = PPOTrainer(env, A.BatchedPPO(device=dev, use_img=False, mini_batch=min(args.scenes, 16384), mini_epoch=1), horizon=4,
                        seed=rank, use_planner='device' if args.device_planner else True,
                        chooser='device' if args.device_chooser else None, obs_norm='device' if args.device_norm else None,
                        gae='device' if args.device_gae else None, ring='device' if args.device_ring else None, actor='device')
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(16):
            tr.step()
        torch.cuda.synchronize()
        if rank == 0:
            print(f'  device actor: 16 PPO steps ({tr.updates} updates) in {(time.perf_counter() - t0) * 1e3:.1f} ms, '
                  f'{tr.device_actor.packs} parameter packs')
    if args.device_critics:
        from hope_amd import agents as A
        from hope_amd.rollout import PPOTrainer, SACTrainer
        common = dict(seed=rank, use_planner='device' if args.device_planner else True, obs_norm='device' if args.device_norm else None,
                      ring='device' if args.device_ring else None, critics='device')
        for tr in (SACTrainer(env, A.BatchedSAC(device=dev, use_img=False, batch_size=min(args.scenes, 4096)), horizon=4, update_every=2,
                              sac_update='device' if args.device_sac_update else None, **common),
                   PPOTrainer(env, A.BatchedPPO(device=dev, use_img=False, mini_batch=min(args.scenes, 16384), mini_epoch=1), horizon=4,
                              gae='device' if args.device_gae else None, **common)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(16):
                tr.step()
            torch.cuda.synchronize()
            if rank == 0:
                print(f'  device critics: 16 {type(tr).__name__[:3]} steps ({tr.updates} updates) in {(time.perf_counter() - t0) * 1e3:.1f} ms, '
                      f'{tr.device_critics.packs} parameter packs per slot')
    if args.device_optimizer:
        from hope_amd import agents as A
        from hope_amd.rollout import PPOTrainer, SACTrainer
        common = dict(seed=rank, use_planner='device' if args.device_planner else True, obs_norm='device' if args.device_norm else None,
                      ring='device' if args.device_ring else None, critics='device' if args.device_critics else None, optimizer='device')
        for tr in (SACTrainer(env, A.BatchedSAC(device=dev, use_img=False, batch_size=min(args.scenes, 4096)), horizon=4, update_every=2,
                              sac_update='device' if args.device_sac_update else None, **common),
                   PPOTrainer(env, A.BatchedPPO(device=dev, use_img=False, mini_batch=min(args.scenes, 16384), mini_epoch=1), horizon=4,
                              gae='device' if args.device_gae else None, **common)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(16):
                tr.step()
            torch.cuda.synchronize()
            if rank == 0:
                print(f'  device optimizer: 16 {type(tr).__name__[:3]} steps ({tr.updates} updates) in {(time.perf_counter() - t0) * 1e3:.1f} ms, '
                      f'{ {k: o.steps for k, o in tr.optimizers.items()} } optimiser steps, {tr.agent.soft_update.calls} soft updates')
    if args.device_img_encoder:
        from hope_amd import agents as A
        from hope_amd.rollout import PPOTrainer
        n_img = min(args.scenes, 8192)
        env_img = ParkingBatch(n_img, 128, device=dev, image=True)
        env_img.set_scenes(np.arange(n_img), [uniq[i % len(uniq)] for i in range(n_img)])
        tr = PPOTrainer(env_img, A.BatchedPPO(device=dev, use_img=True, mini_batch=min(n_img, 4096), mini_epoch=1), horizon=4, seed=rank,
                        actor='device', img_encoder='device')
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(8):
            tr.step()
        torch.cuda.synchronize()
        if rank == 0:
            print(f'  device image encoder: 8 PPO steps of {n_img} scenes ({tr.updates} updates) in {(time.perf_counter() - t0) * 1e3:.1f} ms, '
                  f'{tr.device_actor.img_encoder.packs} encoder packs, {tr.device_actor.packs} actor packs')
        env_img.close()
    if args.device_pool > 0:
        from hope_amd import agents as A
        from hope_amd.rollout import PPOTrainer
        from hope_amd.scene_gen import DevicePoolRefresher
        levels = ('Normal', 'Complex', 'Extrem')
        env.generate_pool(args.device_pool, levels, seed=7 + rank)            # the first pool, drawn by the HIP generator as well
        ref = DevicePoolRefresher(env, args.device_pool, levels, seed=7 + rank, relaxed=True)
        ref.batch = 1
        tr = PPOTrainer(env, A.BatchedPPO(device=dev, use_img=False, mini_batch=min(args.scenes, 16384), mini_epoch=1), horizon=4,
                        seed=rank, fresh_scenes=True, pool_refresher=ref, curriculum={} if args.curriculum else None)
        for _ in range(16):
            tr.step()
        torch.cuda.synchronize()
        if rank == 0:
            print(f'  device pool: {tr.updates} PPO updates, {ref.commits} refills of {args.device_pool} lots generated on the device, '
                  f'pool generation {env.pool_generation():#x}')
            if args.curriculum:
                st = tr.stats()
                cs = env.curriculum_state()
                print('  curriculum: ' + ', '.join(f'{k} {v:.3f}' for k, v in st.items() if k.startswith('success_rate_')) +
                      f'; q = {np.round(cs["q"], 3).tolist()} after {cs["updates"]} updates')
        if args.curriculum:
            env.disable_curriculum()
    # evaluation as eval_utils.py does it (one episode per slot, per-level table), records gathered over the ranks
    from hope_amd import agents as A
    from hope_amd import evaluate as E
    ag = A.BatchedPPO(device=dev, use_img=False)
    env.set_scenes(np.arange(args.scenes), [uniq[i % len(uniq)] for i in range(args.scenes)])
    rec = E.BatchedEvaluator(env, ag, seed=rank, use_planner='device' if args.device_planner else True,
                             chooser='device' if args.device_chooser else None,
                             obs_norm='device' if args.device_norm else None, tracker='device' if args.device_eval else None).run()
    if rank == 0:
        levels = [uniq[i % len(uniq)].level for i in range(args.scenes)] * world
        for k, v in E.summarize(rec, levels).items():
            print(f'  eval {k:8s}: {v["episodes"]} episodes, success {v["success_rate"]:.3f}, steps {v["step_num_mean"]:.1f} +- {v["step_num_std"]:.1f}, '
                  f'path {v["path_length_mean"]:.2f} m')
    if args.eval_levels:
        n = min(args.scenes, 4096)
        env.close()
        env = ParkingBatch(n, 128, device=dev)
        env.set_scenes(np.arange(n), [uniq[i % len(uniq)] for i in range(n)])
        env.set_draw_class(np.arange(n), 1)                                   # every slot draws Dragon-Lake lots
        env.set_dlp_cases()
        env.redraw(torch.ones(n, dtype=torch.uint8, device=dev), seed=1 + rank)
        rec = E.BatchedEvaluator(env, ag, seed=rank).run(levels=True)         # [n_total, 5]: the fifth column is the level
        if rank == 0:
            for k, v in E.summarize(rec).items():
                print(f'  eval-levels {k:8s}: {v["episodes"]} episodes, success {v["success_rate"]:.3f}, steps {v["step_num_mean"]:.1f}, '
                      f'path {v["path_length_mean"]:.2f} m')


if __name__ == '__main__':
    main()
