"""ParkingBatch -- N independent parking scenes stepped on one MI355X through libhope_env.so.

Tensor-in / tensor-out counterpart of `CarParkingWrapper.step` (src/env/env_wrapper.py:73-81) for N >> 1.
PyTorch is used for device memory and streams only; all arithmetic is in the HIP kernels.
"""
import ctypes as C
from functools import partial

import numpy as np
import torch

from . import _lib as L
from . import tables as T
from .scenes import pack_scenes


class ParkingBatch:
    def __init__(self, n_scenes, max_obstacles=128, device='cuda:0', obs_dtype=torch.float32,
                 action_dtype=torch.float32, tables=None, profile=False, image=False, overlap=None,
                 rescale_f32=False):
        """overlap: run the launch chains of the two obstacle-tile classes on two streams (default on: +15 % at 65 536
        scenes, +45 % at 4 096-8 192, measured).  rescale_f32: with float32 actions, evaluate action_rescale in float32 as the reference does with gym's float32 Box
        (env_wrapper.py:46-47); default: float64 arithmetic whatever the action dtype."""
        if not torch.cuda.is_available():
            raise L.HopeError('ParkingBatch needs a HIP device (torch.cuda.is_available() is False); no CPU fallback')
        self.lib = L.load_library()
        self.device = torch.device(device)
        if self.device.index is None:              # 'cuda' -> the current device, so that tensor.device == self.device
            self.device = torch.device('cuda', torch.cuda.current_device())
        self.n, self.max_obst = int(n_scenes), int(max_obstacles)
        if obs_dtype not in (torch.float32, torch.float64) or action_dtype not in (torch.float32, torch.float64):
            raise L.HopeError(f'ParkingBatch: obs_dtype and action_dtype must be torch.float32 or torch.float64, got {obs_dtype} and {action_dtype}')
        self.obs_dtype, self.action_dtype = obs_dtype, action_dtype
        if overlap is None:
            overlap = True
        flags = (L.F_OBS_F64 if obs_dtype == torch.float64 else 0) | (L.F_ACTION_F64 if action_dtype == torch.float64 else 0) | (L.F_PROFILE if profile else 0) | (L.F_IMAGE if image else 0) | (L.F_OVERLAP if overlap else 0)
        self.overlap = bool(overlap)
        self.image = bool(image)
        self._action_bits = L.ACTION_RESCALE_F32 if (rescale_f32 and action_dtype == torch.float32) else 0
        h = C.c_void_p()
        L.check(self.lib.hope_env_create(C.byref(h), self.n, self.max_obst, self.device.index or 0, flags),
                'hope_env_create')
        self.h = h
        self.arch = self.lib.hope_env_device_arch(self.h).decode()
        t = T.all_tables() if tables is None else tables
        self.tables = t
        ds, hb, ab = (L.array_arg('hope_env_upload_tables', k, t[k], np.float64, shape)
                      for k, shape in (('dist_star', (1200, 42, 10)), ('hull_base', (120,)), ('beam_ab', (120, 2))))
        L.check(self.lib.hope_env_upload_tables(self.h, ds.ctypes, hb.ctypes, ab.ctypes), 'hope_env_upload_tables')
        n, dev, od = self.n, self.device, obs_dtype
        # every output lives in ONE device arena (typed views at 256-byte aligned offsets): `download_outputs()` brings all of a
        # step's results to the host with a single copy -- what the N = 1 look-alike classes (hope_amd/env.py) need per step
        spec = [('lidar', (n, L.LIDAR_NUM), od), ('action_mask', (n, L.N_ACTION), od), ('target', (n, L.TARGET_DIM), od),
                ('reward', (n,), od), ('reward_info', (n, 5), od), ('status', (n,), torch.int32), ('done', (n,), torch.uint8),
                ('pose', (n, 3), torch.float64), ('rs_word', (n, 8), torch.int8), ('rs_lengths', (n, L.RS_MAX_SEG), od)]
        if image:       # obs['img'] * 255 as uint8, channel-first (env_wrapper.py:53-54); the reference's float image is img / 255
            spec.append(('img', (n, L.IMG_CHANNELS, L.IMG_SIZE, L.IMG_SIZE), torch.uint8))
        off, self._layout = 0, {}
        for name, shape, dt in spec:
            nbytes = int(np.prod(shape)) * torch.empty((), dtype=dt).element_size()
            self._layout[name] = (off, nbytes, shape, dt)
            off = (off + nbytes + 255) & ~255
        self._arena = torch.zeros(off, dtype=torch.uint8, device=dev)
        self._arena_host = None
        for name, (o, nbytes, shape, dt) in self._layout.items():
            setattr(self, name, self._arena[o:o + nbytes].view(dt).view(shape))
        self.rs_word.fill_(-1)
        if not image:
            self.img = None
        self._done_mask = torch.zeros(n, dtype=torch.uint8, device=dev)
        # observation-only view for turnover(): the finished step's reward / status / done / RS outputs are kept
        self._out_obs = L.StepOut(self.lidar.data_ptr(), self.action_mask.data_ptr(), self.target.data_ptr(), None, None, None,
                                  None, self.pose.data_ptr(), None, None, self.img.data_ptr() if image else None)
        self._out = L.StepOut(self.lidar.data_ptr(), self.action_mask.data_ptr(), self.target.data_ptr(),
                              self.reward.data_ptr(), self.reward_info.data_ptr(), self.status.data_ptr(),
                              self.done.data_ptr(), self.pose.data_ptr(), self.rs_word.data_ptr(),
                              self.rs_lengths.data_ptr(), self.img.data_ptr() if image else None)
        # what the enable_* methods allocate on first use (None: that part is off, and its calls say so) and what the pool setters record
        self.planned = self._plan_exec = self.plan_executing = None
        self.chosen_action = self.chosen_action_f32 = self.chosen_idx = self.chosen_log_prob = self.chosen_probs = None
        self.norm_lidar = self.norm_target = self.gae_sums = self._gae_out = None
        self.eval_alive = self.eval_word = self.eval_done = self._eval_rec = None
        self._ppo_out = {}                            # mb -> (g_raw, g_log_std, g_value, losses) of ppo_loss
        self._sac_out = {}                            # (call, B) -> the outputs of sac_sample / sac_critic / sac_seed / sac_policy
        self._policy_shape, self._policy_out, self._policy_held = None, {}, None   # enable_policy's shape, B -> out, the loaded net's tensors
        self._policy_owner = None                     # the agent_glue.DeviceActor whose parameters the handle holds (one set per handle)
        self._critic_shape, self._critic_out = None, {}            # enable_critics' (n_slots, has_img, has_action), (n, B) -> out
        self._critic_held, self._critic_owner = {}, {}             # slot -> the loaded net's tensors / the agent_glue.DeviceCritics that loaded it
        self._imgenc_act, self._imgenc_max, self._imgenc_out, self._imgenc_held = None, 0, {}, None   # enable_img_encoder's act and room, B -> (token, features)
        self._imgenc_owner = None                     # the agent_glue.DeviceImgEncoder whose parameters the handle holds
        self.pool_size = self.n_dlp_cases = None
        self._refresher_filling = False

    # -- scenes ------------------------------------------------------------------------------------
    def set_scenes(self, ids, scenes):
        """map.reset + vehicle.reset for the listed scene slots (host -> device; synchronous)."""
        start, dest, bbox, verts, nob, _nv = pack_scenes(scenes, self.max_obst)
        self.set_scene_arrays(ids, start, dest, bbox, verts, nob)

    def set_draw_class(self, ids, cls):
        """size class of scene slots (0: lots of <= 32 obstacles, 1: larger lots / Dragon-Lake cases): which launch chain steps a
        slot and which pool entries it draws at turnover; set_scenes derives it from the obstacle count of the uploaded map"""
        ids = L.array_arg('hope_env_set_draw_class', 'ids', ids, np.int32, (None,))
        c = L.array_arg('hope_env_set_draw_class', 'cls', np.broadcast_to(np.asarray(cls, dtype=np.uint8), ids.shape), np.uint8, ids.shape)
        torch.cuda.synchronize(self.device)
        L.check(self.lib.hope_env_set_draw_class(self.h, ids.ctypes, len(ids), c.ctypes), 'hope_env_set_draw_class')
        return self

    def set_scene_arrays(self, ids, start, dest, bbox, verts, n_obst):
        ids = L.array_arg('hope_env_set_scenes', 'ids', ids, np.int32, (None,))
        a = self._scene_arrays('hope_env_set_scenes', len(ids), start, dest, bbox, verts, n_obst)
        torch.cuda.synchronize(self.device)
        L.check(self.lib.hope_env_set_scenes(self.h, ids.ctypes, len(ids), *[x.ctypes for x in a]), 'hope_env_set_scenes')

    def _scene_arrays(self, call, n, start, dest, bbox, verts, n_obst):
        """n maps in the library's layout: start [n, 3], dest [n, 3], bbox [n, 4], verts [n, max_obst, 4, 2] float64, n_obst [n] int32"""
        return [L.array_arg(call, 'start', start, np.float64, (n, 3)), L.array_arg(call, 'dest', dest, np.float64, (n, 3)),
                L.array_arg(call, 'bbox', bbox, np.float64, (n, 4)), L.array_arg(call, 'verts', verts, np.float64, (n, self.max_obst, 4, 2)),
                L.array_arg(call, 'n_obst', n_obst, np.int32, (n,))]

    def set_pool(self, scenes):
        """upload a pool of complete scenes (list[Scene] or the tuple pack_scenes returns) that redraw() draws from"""
        start, dest, bbox, verts, nob, _nv = pack_scenes(scenes, self.max_obst) if isinstance(scenes, list) else scenes
        nob = L.array_arg('hope_env_set_pool', 'n_obst', nob, np.int32, (None,))
        a = self._scene_arrays('hope_env_set_pool', len(nob), start, dest, bbox, verts, nob)
        if self._refresher_filling:
            raise L.HopeError('set_pool while a PoolRefresher fill is running: the pinned staging arrays are being written by its '
                              'thread (close() / poll(wait=True) the refresher first)')
        torch.cuda.synchronize(self.device)
        L.check(self.lib.hope_env_set_pool(self.h, len(nob), *[x.ctypes for x in a]), 'hope_env_set_pool')
        self.pool_size = len(nob)

    def pool_staging(self, n_pool):
        """pinned host arrays (start[n,3], dest[n,3], bbox[n,4], verts[n,max_obst,4,2], n_obst[n]) of the handle that the next
        commit_pool(n_pool) uploads; any host thread may fill them (e.g. the native generator, GIL released)"""
        ptr = [C.c_void_p() for _ in range(5)]
        L.check(self.lib.hope_env_pool_staging(self.h, int(n_pool), *[C.byref(q) for q in ptr]), 'hope_env_pool_staging')
        shapes = [(n_pool, 3), (n_pool, 3), (n_pool, 4), (n_pool, self.max_obst, 4, 2), (n_pool,)]
        out = []
        for q, shp, ct in zip(ptr, shapes, (C.c_double,) * 4 + (C.c_int32,)):
            out.append(np.ctypeslib.as_array(C.cast(q, C.POINTER(ct)), shape=(int(np.prod(shp)),)).reshape(shp))
        return tuple(out)

    def pool_staging_ready(self):
        """True when pool_staging() would not wait (the previous commit's copies have left the pinned arrays)"""
        rc = self.lib.hope_env_pool_staging_ready(self.h)
        if rc < 0:
            L.check(rc, 'hope_env_pool_staging_ready')
        return bool(rc)

    def pool_generation(self):
        """changes whenever the set of maps a draw can return changes (set_pool / commit_pool / set_dlp_cases)"""
        g = C.c_uint64(0)
        L.check(self.lib.hope_env_pool_generation(self.h, C.byref(g)), 'hope_env_pool_generation')
        return int(g.value)

    def commit_pool(self, n_pool, relaxed=False):
        """asynchronous upload of the staged pool + swap: steps enqueued afterwards draw from it (no host synchronisation; the next
        step's launch waits on its stream for the upload).  relaxed=True (hope_env_commit_pool_relaxed): the swap happens at the first
        step enqueued after the upload has completed -- no step waits at all"""
        if relaxed:
            L.check(self.lib.hope_env_commit_pool_relaxed(self.h, int(n_pool)), 'hope_env_commit_pool_relaxed')
        else:
            L.check(self.lib.hope_env_commit_pool(self.h, int(n_pool), self._stream()), 'hope_env_commit_pool')
        self.pool_size = int(n_pool)
        return self

    def generate_pool(self, n_pool, levels=('Normal', 'Complex', 'Extrem'), seed=0, batch=0, relaxed=False):
        """refill the pool on the device (hope_env_generate_pool): n_pool lots of the listed levels (split as PoolRefresher splits
        them), drawn by the HIP generator into the pool set the kernels are not reading and swapped in as commit_pool(relaxed=)
        does.  Lot k of a level is lot batch * n_pool + k of scene_gen.generate_arrays_det(level, seed=seed * 1000003 + level id).
        No host thread, staging or upload; asynchronous."""
        from .scene_gen import pool_level_counts
        counts = (C.c_int32 * 3)(*pool_level_counts(n_pool, levels))
        L.check(self.lib.hope_env_generate_pool(self.h, int(n_pool), counts, L.seed64(seed),
                                                C.c_int64(int(batch) * int(n_pool)), 1 if relaxed else 0), 'hope_env_generate_pool')
        self.pool_size = int(n_pool)
        return self

    # -- curriculum for new-map draws (hope_env.h; rule: hope_amd/curriculum.py) --------------------------------------
    def enable_curriculum(self, **params):
        """tally episode outcomes per bucket on the device and draw new maps from weighted lists rebuilt from them (SceneChoose /
        DlpCaseChoose of train_HOPE_sac.py:23-97).  params: fields of _lib.CurriculumParams (default: the reference's constants).
        Needs a pool or Dragon-Lake cases; off by default."""
        p = L.CurriculumParams(**params)
        torch.cuda.synchronize(self.device)
        L.check(self.lib.hope_env_curriculum_enable(self.h, C.byref(p)), 'hope_env_curriculum_enable')
        return self

    def disable_curriculum(self):
        torch.cuda.synchronize(self.device)
        L.check(self.lib.hope_env_curriculum_disable(self.h), 'hope_env_curriculum_disable')
        return self

    def set_pool_buckets(self, buckets):
        """level (0 Normal, 1 Complex, 2 Extrem; 255 unlabelled) of every entry of the resident pool (generate_pool labels its own)"""
        b = L.array_arg('hope_env_set_pool_buckets', 'buckets', buckets, np.uint8, (None,))
        torch.cuda.synchronize(self.device)
        L.check(self.lib.hope_env_set_pool_buckets(self.h, len(b), b.ctypes), 'hope_env_set_pool_buckets')
        return self

    def curriculum_tally(self):
        """count the episodes the last step finished (its own status / done buffers), asynchronously on the current stream"""
        L.check(self.lib.hope_env_curriculum_tally(self.h, self._out.status, self._out.done, self._stream()), 'hope_env_curriculum_tally')
        return self

    def curriculum_update(self):
        """fold the tallies into the windows and rebuild the weighted draw lists (asynchronous; applied at the next step)"""
        L.check(self.lib.hope_env_curriculum_update(self.h, self._stream()), 'hope_env_curriculum_update')
        return self

    def curriculum_state(self):
        """{'episodes', 'successes' (cumulative), 'win_n', 'win_s', 'prob' (q_0..q_3, then p_c): [4 + n_cases]; 'q', 'pw': [4];
        'updates', 'unlabelled_episodes', 'unlabelled_successes', 'on'} -- host-synchronous"""
        nb = C.c_int32(0)
        misc = np.zeros(4, np.uint64)
        L.check(self.lib.hope_env_curriculum_state(self.h, C.byref(nb), None, None, None, None, None, None, misc.ctypes), 'hope_env_curriculum_state')
        out = {'on': bool(misc[3]), 'updates': int(misc[0]), 'n_buckets': int(nb.value)}
        if not out['on']:
            return out
        n = nb.value
        e, s = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
        wn, ws, prob, pw = np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(4)
        L.check(self.lib.hope_env_curriculum_state(self.h, None, e.ctypes, s.ctypes, wn.ctypes, ws.ctypes, prob.ctypes, pw.ctypes, misc.ctypes),
                'hope_env_curriculum_state')
        out.update(episodes=e, successes=s, win_n=wn, win_s=ws, prob=prob, q=prob[:4].copy(), pw=pw, updates=int(misc[0]),
                   unlabelled_episodes=int(misc[1]), unlabelled_successes=int(misc[2]))
        return out

    def curriculum_set_windows(self, win_n, win_s, episodes, successes):
        """set the windows and cumulative counters by hand (checkpoint restore, tests) and rebuild the lists from them"""
        arg = partial(L.array_arg, 'hope_env_curriculum_set_windows')
        wn = arg('win_n', win_n, np.float64, (None,))                   # (the library compares the count with its number of buckets)
        a = [wn, arg('win_s', win_s, np.float64, wn.shape), arg('episodes', episodes, np.uint64, wn.shape), arg('successes', successes, np.uint64, wn.shape)]
        torch.cuda.synchronize(self.device)
        L.check(self.lib.hope_env_curriculum_set_windows(self.h, len(wn), *[x.ctypes for x in a]), 'hope_env_curriculum_set_windows')
        return self

    def curriculum_lists(self):
        """(list of class 0, list of class 1, positions [2, n_buckets]) as the next step reads them; a class without entries: all -1"""
        nb = C.c_int32(0)
        L.check(self.lib.hope_env_curriculum_state(self.h, C.byref(nb), None, None, None, None, None, None, None), 'hope_env_curriculum_state')
        l0, l1 = np.full(L.CURRICULUM_LIST_LEN, -1, np.int32), np.full(L.CURRICULUM_LIST_LEN, -1, np.int32)
        pos = np.zeros((2, nb.value), np.int32)
        L.check(self.lib.hope_env_curriculum_download_lists(self.h, l0.ctypes, l1.ctypes, pos.ctypes), 'hope_env_curriculum_download_lists')
        return l0, l1, pos

    def set_dlp_cases(self, pool=None):
        """make the Dragon-Lake-Parking cases (a `DlpScenePool`, default data/dlp_scenes.npz) drawable on the device: at episode
        turnover a large-tile scene then gets a case with a freshly drawn start candidate, jitter, flips and obstacle cull
        (ParkingMapDLP.reset) instead of a frozen host-side sample.  pool=False removes them."""
        if pool is False:
            L.check(self.lib.hope_env_set_dlp_cases(self.h, 0, None, None, None, None, 0, None, None), 'hope_env_set_dlp_cases')
            return self
        from .scenes import DlpScenePool
        pool = pool or DlpScenePool()
        arg = partial(L.array_arg, 'hope_env_set_dlp_cases')
        dest = arg('dest', pool.dest, np.float64, (None, 3))
        cand_off = arg('start_off', pool.start_off, np.int32, (len(dest) + 1,))
        cand = arg('starts', pool.starts, np.float64, (None, 3))
        case_set = arg('case_set', pool.case_set, np.int32, (len(dest),))
        set_off = arg('set_off', pool.set_off, np.int32, (None,))
        sv = np.array(pool.set_verts, dtype=np.float64)          # [total][4][2]; triangles repeat their last vertex
        tri = np.asarray(pool.set_nvert) == 3
        sv[tri, 3] = sv[tri, 2]
        sv = arg('set_verts', sv, np.float64, (None, 4, 2))
        torch.cuda.synchronize(self.device)
        L.check(self.lib.hope_env_set_dlp_cases(self.h, len(dest), dest.ctypes, cand_off.ctypes, cand.ctypes, case_set.ctypes,
                                                len(set_off) - 1, set_off.ctypes, sv.ctypes), 'hope_env_set_dlp_cases')
        self.n_dlp_cases = len(dest)
        return self

    def pool_overflow(self):
        out = np.zeros(1, np.int32)
        L.check(self.lib.hope_env_pool_overflow(self.h, out.ctypes), 'hope_env_pool_overflow')
        return int(out[0])

    def download_scenes(self, ids):
        """the maps the listed scene slots hold now -> (start, dest, bbox, verts, n_obst) (host arrays)"""
        ids = L.array_arg('hope_env_download_scenes', 'ids', ids, np.int32, (None,))
        n = len(ids)
        start, dest, bbox = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((n, 4))
        verts, nob = np.zeros((n, self.max_obst, 4, 2)), np.zeros(n, np.int32)
        L.check(self.lib.hope_env_download_scenes(self.h, ids.ctypes, n, start.ctypes, dest.ctypes, bbox.ctypes, verts.ctypes, nob.ctypes),
                'hope_env_download_scenes')
        return start, dest, bbox, verts, nob

    def pool_state(self):
        """(pool index, episode counter) of every scene: with download_state() and pool_generation() the whole snapshot of a
        run that draws maps from a pool that is NOT replaced in the meantime (refreshed runs: download_scenes / set_scene_arrays)"""
        idx, ep = np.zeros(self.n, np.int32), np.zeros(self.n, np.uint32)
        L.check(self.lib.hope_env_download_pool_state(self.h, idx.ctypes, ep.ctypes), 'hope_env_download_pool_state')
        return idx, ep

    def restore_maps(self, pool_index, episode, seed, generation=0):
        """repeat the draws of a snapshot (the seed in use then); `generation` = pool_generation() saved with the snapshot: the
        call fails (HOPE_ESTATE) if the pool has been replaced since -- the draws would return other maps; 0 skips the check.
        Follow with upload_state()"""
        drawn = L.array_arg('hope_env_restore_maps', 'pool_index', np.asarray(pool_index) != -1, np.uint8, (self.n,))
        ep = L.array_arg('hope_env_restore_maps', 'episode', episode, np.uint32, (self.n,))
        L.check(self.lib.hope_env_restore_maps(self.h, drawn.ctypes, ep.ctypes, L.seed64(seed), C.c_uint64(int(generation))),
                'hope_env_restore_maps')
        return self

    def redraw(self, mask, seed=0):
        """map.reset for the flagged scenes: each takes a pool scene of its tile class and restarts (asynchronous)"""
        mp = L.tensor_arg('hope_env_redraw', 'mask', mask, torch.uint8, (self.n,), self.device)
        L.check(self.lib.hope_env_redraw(self.h, mp, L.seed64(seed), self._stream()), 'hope_env_redraw')
        return self

    def turnover(self, seed=0):
        """episode turnover with a NEW map, as the reference's training loop does (`env.reset(...)` after `done`):
        finished scenes draw a pool scene and get their first observation; reward / reward_info / status / done / RS
        outputs keep the values of the finished step (like auto_reset)."""
        self._done_mask.copy_(self.done)
        self.redraw(self._done_mask, seed)
        stages = L.STAGE_ALL | (L.STAGE_IMG if self.image else 0)
        mp = L.tensor_arg('hope_env_reset_obs', 'done mask', self._done_mask, torch.uint8, (self.n,), self.device)
        L.check(self.lib.hope_env_reset_obs(self.h, mp, stages, C.byref(self._out_obs), self._stream()), 'hope_env_reset_obs')
        return self

    def pool_index(self):
        out = np.zeros(self.n, np.int32)
        L.check(self.lib.hope_env_download_pool_index(self.h, out.ctypes), 'hope_env_download_pool_index')
        return out

    # -- the hot path ------------------------------------------------------------------------------
    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def reset_obs(self, active=None, stages=L.STAGE_ALL):
        """the action-less step of CarParking.reset (car_parking_base.py:138)."""
        if self.image and (stages & L.STAGE_ALL) == L.STAGE_ALL:
            stages |= L.STAGE_IMG
        ap = L.tensor_arg('hope_env_reset_obs', 'active', active, (torch.uint8, torch.bool), (self.n,), self.device, optional=True)
        L.check(self.lib.hope_env_reset_obs(self.h, ap, stages, C.byref(self._out), self._stream()), 'hope_env_reset_obs')
        return self

    def set_redraw_seed(self, seed):
        """seed of the draws of step(..., auto_reset=True, fresh=True)"""
        L.check(self.lib.hope_env_set_redraw_seed(self.h, L.seed64(seed)), 'hope_env_set_redraw_seed')
        return self

    def step(self, actions, active=None, stages=L.STAGE_ALL, auto_reset=False, fresh=False, defer_rs=False):
        """actions: [N, 2] (steer, speed) in [-1, 1] on this device.  auto_reset=True: finished scenes restart inside
        the step (their lidar / action_mask / target are the new episode's first observation) -- on the same map, or with
        fresh=True on a NEW map drawn from the device-resident scene pool (set_pool), like step() + turnover() in one call.
        defer_rs=True (HOPE_DEFER_RS): the current stream is ordered after the observation / reward / status outputs only;
        call wait_rs() before reading rs_word / rs_lengths (the planner override), the policy forward in between overlaps the
        Reeds-Shepp kernels."""
        if defer_rs:
            stages |= L.DEFER_RS
        if self.image and (stages & L.STAGE_ALL) == L.STAGE_ALL:
            stages |= L.STAGE_IMG                    # USE_IMG (configs.py:100): the image is part of the observation
        if auto_reset:
            stages |= L.AUTO_RESET | (L.AUTO_REDRAW if fresh else 0)
        stages |= self._action_bits
        xp = L.tensor_arg('hope_env_step', 'actions', actions, self.action_dtype, (self.n, 2), self.device)
        ap = L.tensor_arg('hope_env_step', 'active', active, (torch.uint8, torch.bool), (self.n,), self.device, optional=True)
        L.check(self.lib.hope_env_step(self.h, xp, ap, stages, C.byref(self._out), self._stream()), 'hope_env_step')
        return self

    def step_plan(self, stages=L.STAGE_ALL, has_action=True, defer_rs=False):
        """the launch plan of the next step(stages=..., defer_rs=...) (has_action=False: of reset_obs) as the library computes it
        (hope_env_step_plan: a test hook; nothing is launched).  -> dict(split, pipe, fuse_kin, auto_subs: bool, chains: list, in
        launch order, of dict(tile_class, tile_cap, motion, obs: names of _lib.MOTION_KERNELS / OBS_KERNELS, scenes: int32 ids in
        list order -- entries 2b and 2b + 1 share a wave of the pair kernels))"""
        if defer_rs:
            stages |= L.DEFER_RS
        if self.image and (stages & L.STAGE_ALL) == L.STAGE_ALL:
            stages |= L.STAGE_IMG
        stages |= self._action_bits
        out = np.zeros(L.STEPPLAN_HEAD + 2 * L.STEPPLAN_CHAIN_HEAD + self.n, np.int32)
        L.check(self.lib.hope_env_step_plan(self.h, stages, 1 if has_action else 0, out.ctypes, len(out)), 'hope_env_step_plan')
        flags, chains, w = int(out[1]), [], L.STEPPLAN_HEAD
        for _ in range(int(out[2])):
            c, cap, motion, obs, m = (int(v) for v in out[w:w + L.STEPPLAN_CHAIN_HEAD])
            w += L.STEPPLAN_CHAIN_HEAD
            chains.append(dict(tile_class=c, tile_cap=cap, motion=L.MOTION_KERNELS[motion], obs=L.OBS_KERNELS[obs], scenes=out[w:w + m].copy()))
            w += m
        assert w == out[0]
        return dict(split=bool(flags & L.STEPPLAN_SPLIT), pipe=bool(flags & L.STEPPLAN_PIPE), fuse_kin=bool(flags & L.STEPPLAN_FUSE_KIN),
                    auto_subs=bool(flags & L.STEPPLAN_AUTO_SUBS), chains=chains)

    def last_step(self):
        """sequence number of the most recent step() / reset_obs() of this handle (hope_env_last_step)"""
        g = C.c_uint64(0)
        L.check(self.lib.hope_env_last_step(self.h, C.byref(g)), 'hope_env_last_step')
        return int(g.value)

    def wait_rs(self, step=None):
        """orders the current stream after the Reeds-Shepp outputs of the last step(defer_rs=True); no-op otherwise.
        step = a value of last_step(): the wait is for THAT step's search and raises (HOPE_ESTATE) when a newer step has been
        enqueued since -- consecutive deferred steps pipeline and the newer one replaces rs_word / rs_lengths."""
        if step is None:
            L.check(self.lib.hope_env_wait_rs(self.h, self._stream()), 'hope_env_wait_rs')
        else:
            L.check(self.lib.hope_env_wait_rs_step(self.h, C.c_uint64(int(step)), self._stream()), 'hope_env_wait_rs_step')
        return self

    # -- replay of found Reeds-Shepp paths on the device (hope_env.h; rule: csrc/hope_planner_core.h) -----------------
    def enable_planner(self, step_ratio=L.PLAN_STEP_RATIO):
        """RsPlanner / ParkingAgent's path replay as device state of the handle (48 B per scene, every scene idle).  Off by default."""
        torch.cuda.synchronize(self.device)
        L.check(self.lib.hope_env_planner_enable(self.h, float(step_ratio)), 'hope_env_planner_enable')
        if self.planned is None:
            self.planned = torch.zeros((self.n, 2), dtype=torch.float64, device=self.device)
            self._plan_exec = torch.zeros(self.n, dtype=torch.uint8, device=self.device)
            self.plan_executing = self._plan_exec.view(torch.bool)
        return self

    def disable_planner(self):
        torch.cuda.synchronize(self.device)
        L.check(self.lib.hope_env_planner_disable(self.h), 'hope_env_planner_disable')
        return self

    def planner_reset(self, mask=None):
        """clear the path of the scenes flagged in mask (u8 [N]), or of all (asynchronous on the current stream)"""
        mp = L.tensor_arg('hope_env_planner_reset', 'mask', mask, torch.uint8, (self.n,), self.device, optional=True)
        L.check(self.lib.hope_env_planner_reset(self.h, mp, self._stream()), 'hope_env_planner_reset')
        return self

    def planner_step(self, forced=False, step=None, actions=None, rs_word=None, rs_lengths=None, done=True, pop=True):
        """one k_plan launch on the current stream, no host synchronisation: the scenes the last step finished drop their path,
        found words are adopted (by idle scenes, or by all with forced), busy scenes pop their next action.
        -> (planned f64 [N, 2], executing bool [N]): persistent tensors of this object, overwritten by the next call.
        step = a value of last_step(): the call waits for THAT step's search (as wait_rs(step)) and raises when a newer step has
        replaced its words; None: a plain wait_rs() first.  actions: [N, 2] of the env's action dtype, the executing rows are
        overwritten in place.  rs_word / rs_lengths / done default to the env's own outputs (done=None: no scene is cleared);
        pop=False: bookkeeping only."""
        if step is None:
            L.check(self.lib.hope_env_wait_rs(self.h, self._stream()), 'hope_env_wait_rs')
        n, arg = self.n, partial(L.tensor_arg, 'hope_env_planner_step', device=self.device)
        wp = arg('rs_word', self.rs_word if rs_word is None else rs_word, torch.int8, (n, 8))
        lp = arg('rs_lengths', self.rs_lengths if rs_lengths is None else rs_lengths, self.obs_dtype, (n, 5))
        dp = arg('done', self.done if done is True else done, torch.uint8, (n,), optional=True)
        ap = arg('actions', actions, (torch.float32, torch.float64), (n, 2), optional=True)
        af64 = int(actions is not None and actions.dtype == torch.float64)
        flags = (L.PLAN_FORCED if forced else 0) | (0 if pop else L.PLAN_NO_POP)
        pp = arg('planned', self.planned, torch.float64, (n, 2), optional=True)    # (None: the library reports that the planner is off)
        ep = arg('executing', self._plan_exec, torch.uint8, (n,), optional=True)
        L.check(self.lib.hope_env_planner_step(self.h, wp, lp, dp, flags, C.c_uint64(int(step or 0)), pp, ep, ap, af64, self._stream()),
                'hope_env_planner_step')
        return self.planned, self.plan_executing

    def planner_state(self):
        """the planner's state block (numpy uint64 [6, N]: the five segment lengths in steps as float64 bits, the packed cursor
        word) -- host-synchronous; tests"""
        out = np.zeros((L.PLAN_STATE_WORDS, self.n), np.uint64)
        L.check(self.lib.hope_env_planner_download_state(self.h, out.ctypes), 'hope_env_planner_download_state')
        return out

    # -- masked choice of the discrete action on the device (hope_env.h; rule: csrc/hope_chooser_core.h) -----------------
    def enable_chooser(self):
        """ActionMask.choose_action + the agent's cast / clamp / planner override / log-probability as one kernel (k_choose).
        Uploads the 42 x 2 action table in the policy's scaling (numpy's own bits).  Off by default."""
        torch.cuda.synchronize(self.device)
        acts = L.array_arg('hope_env_chooser_enable', 'actions', T.discrete_actions() / [T.VALID_STEER[1], 1.0], np.float64, (L.N_ACTION, 2))
        L.check(self.lib.hope_env_chooser_enable(self.h, acts.ctypes), 'hope_env_chooser_enable')
        if self.chosen_action is None:
            dev = self.device
            self.chosen_action_f32 = torch.zeros((self.n, 2), dtype=torch.float32, device=dev)
            # a float32 env steps with the very tensor the transition ring stores
            self.chosen_action = self.chosen_action_f32 if self.action_dtype == torch.float32 else torch.zeros((self.n, 2), dtype=torch.float64, device=dev)
            self.chosen_idx = torch.zeros(self.n, dtype=torch.int32, device=dev)
            self.chosen_log_prob = torch.zeros((self.n, 2), dtype=torch.float32, device=dev)
            # (chosen_probs, [N, 42] float64, is allocated by the first call that asks for it)
        return self

    def disable_chooser(self):
        torch.cuda.synchronize(self.device)
        L.check(self.lib.hope_env_chooser_disable(self.h), 'hope_env_chooser_disable')
        return self

    def choose_actions(self, mean, log_std, mask=None, planned=None, executing=None, u=None, seed=0, counter=0, probs=False):
        """one k_choose launch on the current stream, no host synchronisation, no wait for a deferred search (planner_step does that).
        mean [N, 2] and log_std [N, 2] or [1, 2] (broadcast): both float32 or both float64; mask [N, 42] of the env's observation
        dtype (None: the env's own action_mask); planned f64 [N, 2] + executing bool / u8 [N] (planner_step's outputs): those rows
        take the planned action; u f64 [N] in [0, 1) or None: counter-based draws keyed by (seed, counter, scene).
        -> (action [N, 2] of the env's action dtype, contiguous: goes straight into step(); action_f32 [N, 2]; idx int32 [N], index |
        CHOOSE_NOMASK / CHOOSE_FIXED on a degenerate row; log_prob f32 [N, 2][; probs f64 [N, 42]]): persistent tensors of this
        object, overwritten by the next call."""
        n, dev = self.n, self.device
        arg = partial(L.tensor_arg, 'hope_env_choose', device=dev)
        mp = arg('mean', mean, (torch.float32, torch.float64), (n, 2))
        one_row = n > 1 and tuple(getattr(log_std, 'shape', ())) == (1, 2)
        sp = arg('log_std', log_std, mean.dtype, (1, 2) if one_row else (n, 2))
        kp = arg('mask', self.action_mask if mask is None else mask, self.obs_dtype, (n, L.N_ACTION))
        if (planned is None) != (executing is None):
            raise L.HopeError('hope_env_choose: planned and executing go together')
        pp = arg('planned', planned, torch.float64, (n, 2), optional=True)
        ep = arg('executing', executing, (torch.bool, torch.uint8), (n,), optional=True)
        up = arg('u', u, torch.float64, (n,), optional=True)
        if probs and self.chosen_probs is None and self.chosen_action is not None:
            self.chosen_probs = torch.zeros((n, L.N_ACTION), dtype=torch.float64, device=dev)
        ap = arg('chosen_action', self.chosen_action, self.action_dtype, (n, 2), optional=True)    # (None: the library reports that the chooser is off)
        fp = arg('chosen_action_f32', self.chosen_action_f32, torch.float32, (n, 2), optional=True)
        ip = arg('chosen_idx', self.chosen_idx, torch.int32, (n,), optional=True)
        lp = arg('chosen_log_prob', self.chosen_log_prob, torch.float32, (n, 2), optional=True)
        qp = arg('chosen_probs', self.chosen_probs, torch.float64, (n, L.N_ACTION), optional=True) if probs else None
        L.check(self.lib.hope_env_choose(self.h, mp, sp, 0 if one_row or n == 1 else 2, int(mean.dtype == torch.float64), kp, pp, ep, up,
                                         L.seed64(seed), L.seed64(counter), ap, fp, ip, lp, qp, self._stream()), 'hope_env_choose')
        out = (self.chosen_action, self.chosen_action_f32, self.chosen_idx, self.chosen_log_prob)
        return out + (self.chosen_probs,) if probs else out

    # -- normalisation of the observations on the device (hope_env.h; rule: csrc/hope_obsnorm_core.h) -------------------
    def enable_obsnorm(self):
        """StateNorm's running mean / std of lidar and target and the normalised float32 observation as three kernels
        (k_obsnorm_partial, k_obsnorm_merge, k_obsnorm_apply).  The statistics start at zero (n_state = 0); enabling again keeps
        them.  Off by default."""
        torch.cuda.synchronize(self.device)
        L.check(self.lib.hope_env_obsnorm_enable(self.h), 'hope_env_obsnorm_enable')
        if self.norm_lidar is None:
            self.norm_lidar = torch.zeros((self.n, L.OBSNORM_LIDAR), dtype=torch.float32, device=self.device)
            self.norm_target = torch.zeros((self.n, L.OBSNORM_TARGET), dtype=torch.float32, device=self.device)
        return self

    def disable_obsnorm(self):
        torch.cuda.synchronize(self.device)
        L.check(self.lib.hope_env_obsnorm_disable(self.h), 'hope_env_obsnorm_disable')
        return self

    def obsnorm(self, lidar=None, target=None, update=True, normalize=True):
        """fold `lidar` [rows, 120] / `target` [rows, 5] (both float32 or both float64, contiguous, 1 <= rows <= N; None: the env's
        own observation tensors) into the running statistics and / or normalise them with the statistics as they then are: at most
        three launches on the current stream, no host synchronisation, no wait for a deferred search.
        -> (lidar f32 [rows, 120], target f32 [rows, 5]): (views of) persistent tensors of this object, overwritten by the next
        normalising call; (None, None) without normalize."""
        arg = partial(L.tensor_arg, 'hope_env_obsnorm', device=self.device)
        lidar = self.lidar if lidar is None else lidar
        lp = arg('lidar', lidar, (torch.float32, torch.float64), (None, L.OBSNORM_LIDAR))
        rows = lidar.shape[0]                                                   # (the library checks 1 <= rows <= N)
        tp = arg('target', self.target if target is None else target, lidar.dtype, (rows, L.OBSNORM_TARGET))
        flags = (L.OBSNORM_UPDATE if update else 0) | (L.OBSNORM_NORMALIZE if normalize else 0)
        ol = ot = None
        if normalize:                                                           # (None: the library reports that it is off)
            ol = arg('norm_lidar', self.norm_lidar, torch.float32, (self.n, L.OBSNORM_LIDAR), optional=True)
            ot = arg('norm_target', self.norm_target, torch.float32, (self.n, L.OBSNORM_TARGET), optional=True)
        L.check(self.lib.hope_env_obsnorm(self.h, lp, tp, rows, int(lidar.dtype == torch.float64), flags, ol, ot, self._stream()), 'hope_env_obsnorm')
        if not normalize:
            return None, None
        return (self.norm_lidar, self.norm_target) if rows == self.n else (self.norm_lidar[:rows], self.norm_target[:rows])

    def obsnorm_count(self):
        """n_state: the handle keeps it on the host, so this does not wait for the device"""
        n = C.c_int64(0)
        L.check(self.lib.hope_env_obsnorm_get(self.h, C.byref(n), None, None, None), 'hope_env_obsnorm_get')
        return int(n.value)

    def obsnorm_state(self):
        """-> (n_state, mean, S, std): numpy float64 [125] each (columns 0..119 lidar, 120..124 target); host-synchronous"""
        n = C.c_int64(0)
        mean, S, std = (np.zeros(L.OBSNORM_COLS, np.float64) for _ in range(3))
        L.check(self.lib.hope_env_obsnorm_get(self.h, C.byref(n), mean.ctypes, S.ctypes, std.ctypes), 'hope_env_obsnorm_get')
        return int(n.value), mean, S, std

    def obsnorm_load(self, n_state, mean, S, std):
        """replace the statistics (e.g. a checkpoint's); host-synchronous"""
        a = [L.array_arg('hope_env_obsnorm_set', k, x, np.float64, (L.OBSNORM_COLS,)) for k, x in (('mean', mean), ('S', S), ('std', std))]
        L.check(self.lib.hope_env_obsnorm_set(self.h, int(n_state), *[x.ctypes for x in a]), 'hope_env_obsnorm_set')
        return self

    # -- PPO's advantage block on the device (hope_env.h; rule: csrc/hope_gae_core.h) -----------------------------------
    def enable_gae(self):
        """GAE along T, the critic's target and the advantages' normalisation as three kernels (k_gae_scan, k_gae_merge,
        k_adv_apply) over [rows, T] float32 tensors.  Off by default."""
        torch.cuda.synchronize(self.device)
        L.check(self.lib.hope_env_gae_enable(self.h), 'hope_env_gae_enable')
        if self.gae_sums is None:                                  # (_gae_out, (adv, v_target) [N, T], is allocated at the first call for its T)
            self.gae_sums = torch.zeros(3, dtype=torch.float64, device=self.device)
        return self

    def disable_gae(self):
        torch.cuda.synchronize(self.device)
        L.check(self.lib.hope_env_gae_disable(self.h), 'hope_env_gae_disable')
        return self

    def gae(self, reward, done, value, v_last, value_target, gamma, lam, normalize=True, sums=None):
        """reward / done / value / value_target [rows, T], v_last [rows]: float32, contiguous, on the env's device; 1 <= rows <= N,
        1 <= T <= 4096.  At most three launches on the current stream, no host synchronisation.
        normalize: True -- scan, sums and the normalisation of adv; False -- scan and sums only (the split call: all-reduce `sums`,
        then adv_normalize); None -- the scan alone (adv_norm=False).
        sums: a float64 [3] device tensor that takes {sum adv, sum adv^2, rows T}; None: this object's `gae_sums`.
        -> (adv [rows, T], v_target [rows, T], sums): (views of) persistent tensors of this object, overwritten by the next call."""
        dev = self.device
        arg = partial(L.tensor_arg, 'hope_env_gae', device=dev)
        rp = arg('reward', reward, torch.float32, (None, None))    # (the library checks 1 <= rows <= N and 1 <= T <= 4096)
        rows, t = reward.shape
        dp, vp = arg('done', done, torch.float32, (rows, t)), arg('value', value, torch.float32, (rows, t))
        lp, tp = arg('v_last', v_last, torch.float32, (rows,)), arg('value_target', value_target, torch.float32, (rows, t))
        sums = self.gae_sums if sums is None else sums
        sp = arg('sums', sums, torch.float64, (3,), optional=True)
        out = self._gae_out
        if out is None or out[0].shape[1] != t:                    # (before enable_gae the library reports that it is off)
            out = self._gae_out = tuple(torch.zeros((max(self.n, rows), t), dtype=torch.float32, device=dev) for _ in range(2))
        ap, op = (arg(k, x, torch.float32, (out[0].shape[0], t)) for k, x in zip(('adv', 'v_target'), out))
        flags = 0 if normalize is None else (L.GAE_SUMS | (L.GAE_NORMALIZE if normalize else 0))
        L.check(self.lib.hope_env_gae(self.h, rp, dp, vp, lp, tp, rows, t, float(gamma), float(lam), flags, ap, op, sp, self._stream()), 'hope_env_gae')
        return out[0][:rows], out[1][:rows], sums

    def adv_normalize(self, adv, sums, out=None):
        """out = (adv - mean) / (std + 1e-5) from sums = {sum, sum of squares, count} (float64 [3] on the device, e.g. all-reduced);
        out=None: in place.  One launch on the current stream."""
        out = adv if out is None else out
        arg = partial(L.tensor_arg, 'hope_env_adv_normalize', device=self.device)
        ap = arg('adv', adv, torch.float32, (None,) * getattr(adv, 'ndim', 1))
        op, sp = arg('out', out, torch.float32, tuple(adv.shape)), arg('sums', sums, torch.float64, (3,))
        L.check(self.lib.hope_env_adv_normalize(self.h, ap, adv.numel(), sp, op, self._stream()), 'hope_env_adv_normalize')
        return out

    # -- the transition ring on the device (hope_env.h; rule: csrc/hope_ring_core.h) ------------------------------------
    def enable_ring(self):
        """TransitionRing's push, the episode / success / reward tally of the step and the SAC batch as four kernels (k_ring_before,
        k_ring_after, k_ring_tally, k_ring_sample) over the caller's ring tensors (rollout.DeviceTransitionRing owns a set).  Off by
        default."""
        torch.cuda.synchronize(self.device)
        L.check(self.lib.hope_env_ring_enable(self.h), 'hope_env_ring_enable')
        return self

    def disable_ring(self):
        torch.cuda.synchronize(self.device)
        L.check(self.lib.hope_env_ring_disable(self.h), 'hope_env_ring_disable')
        return self

    @staticmethod
    def _ring_arg(call, ring):
        if not isinstance(ring, L.Ring):
            raise L.HopeError(f'{call}: ring must be a hope_amd._lib.Ring (ring_desc), got {type(ring).__name__}')
        return ring

    def ring_before(self, ring, t, lidar, target, mask, action, log_prob):
        """the before half of column t: lidar [n, 120], target [n, 5], mask [n, 42], action [n, 2], log_prob [n, 2], float32, contiguous,
        n = the ring's; `ring` is a `_lib.Ring` (ring_desc).  One launch on the current stream, no host synchronisation."""
        r, n = self._ring_arg('hope_env_ring_before', ring), ring.n
        arg = partial(L.tensor_arg, 'hope_env_ring_before', dtype=torch.float32, device=self.device)
        L.check(self.lib.hope_env_ring_before(self.h, r, int(t), arg('lidar', lidar, shape=(n, L.LIDAR_NUM)), arg('target', target, shape=(n, L.TARGET_DIM)),
                                              arg('mask', mask, shape=(n, L.N_ACTION)), arg('action', action, shape=(n, 2)),
                                              arg('log_prob', log_prob, shape=(n, 2)), self._stream()), 'hope_env_ring_before')

    def ring_after(self, ring, t, reward, done, status=None, counts=None, reward_sum=None):
        """the after half of column t: reward [n] float32 / float64, done [n] uint8 / bool.  status int32 [n], counts int64 [2] and
        reward_sum float64 [1] go together: then the step is tallied into them (two launches), otherwise one launch."""
        r, n = self._ring_arg('hope_env_ring_after', ring), ring.n
        arg = partial(L.tensor_arg, 'hope_env_ring_after', device=self.device)
        rp = arg('reward', reward, (torch.float32, torch.float64), (n,))
        dp = arg('done', done, (torch.uint8, torch.bool), (n,))
        sp, cp = arg('status', status, torch.int32, (n,), optional=True), arg('counts', counts, torch.int64, (2,), optional=True)
        tp = arg('reward_sum', reward_sum, torch.float64, (1,), optional=True)
        L.check(self.lib.hope_env_ring_after(self.h, r, int(t), rp, int(reward.dtype == torch.float64), dp, sp, cp, tp, self._stream()), 'hope_env_ring_after')

    def ring_sample(self, ring, head, size, batch, out, last_lidar, last_target, last_mask, s=None, j=None, seed=0, counter=0):
        """`batch` transitions into `out` (a `_lib.RingBatch`, ring_batch_desc) from the ring's `size` newest columns; s, j int32
        [batch] (scene, age; 0 = the oldest column), or both None: counter-based draws keyed by (seed, counter, item).  last_*: the
        float32 observation after the newest column.  One launch on the current stream, no host synchronisation."""
        r, n = self._ring_arg('hope_env_ring_sample', ring), ring.n
        if not isinstance(out, L.RingBatch):
            raise L.HopeError(f'hope_env_ring_sample: out must be a hope_amd._lib.RingBatch (ring_batch_desc), got {type(out).__name__}')
        arg = partial(L.tensor_arg, 'hope_env_ring_sample', device=self.device)
        sp, jp = arg('s', s, torch.int32, (batch,), optional=True), arg('j', j, torch.int32, (batch,), optional=True)
        lp, tp = arg('last_lidar', last_lidar, torch.float32, (n, L.LIDAR_NUM)), arg('last_target', last_target, torch.float32, (n, L.TARGET_DIM))
        mp = arg('last_mask', last_mask, torch.float32, (n, L.N_ACTION))
        L.check(self.lib.hope_env_ring_sample(self.h, r, int(head), int(size), int(batch), sp, jp, L.seed64(seed), L.seed64(counter), lp, tp, mp, out,
                                              self._stream()), 'hope_env_ring_sample')

    # -- PPO's minibatch on the device (hope_env.h; rule: csrc/hope_ppo_core.h) ----------------------------------------
    def enable_ppo_batch(self, max_batch):
        """the gather of a PPO minibatch by a permutation's indices and the clipped loss with its gradients as three kernels
        (k_ppo_gather, k_ppo_loss, k_ppo_merge).  max_batch: the largest minibatch; a larger one later reallocates, an equal or
        smaller one changes nothing.  Off by default."""
        torch.cuda.synchronize(self.device)
        L.check(self.lib.hope_env_ppo_enable(self.h, int(max_batch)), 'hope_env_ppo_enable')
        return self

    def disable_ppo_batch(self):
        torch.cuda.synchronize(self.device)
        L.check(self.lib.hope_env_ppo_disable(self.h), 'hope_env_ppo_disable')
        return self

    @staticmethod
    def _ppo_batch_arg(call, name, desc):
        if not isinstance(desc, L.PpoBatch) or not hasattr(desc, 'batch'):
            raise L.HopeError(f'{call}: {name} must be a hope_amd._lib.PpoBatch (ppo_batch_desc), got {type(desc).__name__}')
        return desc

    def ppo_gather(self, ring_desc, adv, v_target, index, out_desc):
        """out_desc (a `_lib.PpoBatch`, ppo_batch_desc) takes the transitions index (int64 [batch], flat: scene * T + column) of the ring
        `ring_desc` (a `_lib.Ring`): observation, action, summed log-probability, and adv / v_target (float32 [n * T]) at the same
        places; an index out of range gives a zero row with idx -1.  One launch on the current stream, no host synchronisation."""
        r = self._ring_arg('hope_env_ppo_gather', ring_desc)
        o = self._ppo_batch_arg('hope_env_ppo_gather', 'out_desc', out_desc)
        arg = partial(L.tensor_arg, 'hope_env_ppo_gather', device=self.device)
        m = r.n * r.T
        ap, vp = arg('adv', adv, torch.float32, (m,)), arg('v_target', v_target, torch.float32, (m,))
        ip = arg('index', index, torch.int64, (o.batch,))
        L.check(self.lib.hope_env_ppo_gather(self.h, r, ap, vp, ip, o.batch, o, self._stream()), 'hope_env_ppo_gather')

    def ppo_loss(self, raw, log_std, value, batch_desc, mb, clip):
        """the clipped surrogate and the critic's squared error of the minibatch `batch_desc` (its action, old_lp, adv, v_target) and
        their gradients: raw [mb, 2] the actor's output before its clamp, log_std [2], value [mb], float32 contiguous.
        -> (g_raw [mb, 2], g_log_std [2], g_value [mb], losses [2] = actor, critic): persistent tensors per mb, overwritten by the next
        call with that mb.  Two launches on the current stream, no host synchronisation."""
        b = self._ppo_batch_arg('hope_env_ppo_loss', 'batch_desc', batch_desc)
        mb = int(mb)
        if mb != b.batch:
            raise L.HopeError(f'hope_env_ppo_loss: mb must be the extent of batch_desc ({b.batch}), got {mb}')
        arg = partial(L.tensor_arg, 'hope_env_ppo_loss', dtype=torch.float32, device=self.device)
        rp, lp, vp = arg('raw', raw, shape=(mb, 2)), arg('log_std', log_std, shape=(2,)), arg('value', value, shape=(mb,))
        out = self._ppo_out.get(mb)
        if out is None:
            out = self._ppo_out[mb] = tuple(torch.zeros(s, dtype=torch.float32, device=self.device) for s in ((mb, 2), (2,), (mb,), (2,)))
        gp = [arg(k, x, shape=tuple(x.shape)) for k, x in zip(('g_raw', 'g_log_std', 'g_value', 'losses'), out)]
        L.check(self.lib.hope_env_ppo_loss(self.h, rp, lp, vp, b, mb, float(clip), *gp, self._stream()), 'hope_env_ppo_loss')
        return out

    # -- SAC's update on the device (hope_env.h; rule: csrc/hope_sac_core.h) -------------------------------------------
    def enable_sac_update(self, max_batch):
        """the arithmetic of BatchedSAC.update between its network forwards as kernels (k_sac_sample, k_sac_critic, k_sac_seed,
        k_sac_policy, k_sac_merge).  max_batch: the largest batch; a larger one later reallocates, an equal or smaller one changes
        nothing.  Off by default."""
        torch.cuda.synchronize(self.device)
        L.check(self.lib.hope_env_sac_enable(self.h, int(max_batch)), 'hope_env_sac_enable')
        return self

    def disable_sac_update(self):
        torch.cuda.synchronize(self.device)
        L.check(self.lib.hope_env_sac_disable(self.h), 'hope_env_sac_disable')
        return self

    def _sac_outputs(self, call, batch, shapes):
        """the persistent outputs of `call` for this batch size: float32 tensors of `shapes` (a shape of None: a float64 scalar)"""
        out = self._sac_out.get((call, batch))
        if out is None:
            out = self._sac_out[(call, batch)] = tuple(
                torch.zeros((), dtype=torch.float64, device=self.device) if s is None else torch.zeros(s, dtype=torch.float32, device=self.device)
                for s in shapes)
        return out

    def sac_sample(self, raw, log_std, eps):
        """raw [B, 2] the actor's output before its clamp, log_std [2], eps [B, 2] the normal draw, float32 contiguous
        -> (action [B, 2], lp [B]): persistent tensors per B, overwritten by the next call with that B.  One launch on the current
        stream, no host synchronisation."""
        arg = partial(L.tensor_arg, 'hope_env_sac_sample', dtype=torch.float32, device=self.device)
        b = int(raw.shape[0]) if hasattr(raw, 'shape') and len(raw.shape) == 2 else None
        ins = [arg('raw', raw, shape=(b, 2)), arg('log_std', log_std, shape=(2,)), arg('eps', eps, shape=(b, 2))]
        out = self._sac_outputs('sample', b, ((b, 2), (b,)))
        L.check(self.lib.hope_env_sac_sample(self.h, *ins, b, *(arg(k, x, shape=tuple(x.shape)) for k, x in zip(('action', 'lp'), out)), self._stream()),
                'hope_env_sac_sample')
        return out

    def sac_critic(self, q1, q2, qt1, qt2, next_lp, reward, done, log_alpha, gamma):
        """q1, q2 (the critics at the stored action), qt1, qt2 (the target critics at the sampled next action), next_lp, reward, done:
        float32 [B] contiguous; log_alpha: a float64 scalar tensor on the device (read there)
        -> (q_target [B], g_q1 [B], g_q2 [B], losses [2]): persistent per B.  Two launches, no host synchronisation."""
        arg = partial(L.tensor_arg, 'hope_env_sac_critic', dtype=torch.float32, device=self.device)
        b = int(q1.shape[0]) if hasattr(q1, 'shape') and len(q1.shape) == 1 else None
        ins = [arg(k, x, shape=(b,)) for k, x in zip(('q1', 'q2', 'qt1', 'qt2', 'next_lp', 'reward', 'done'), (q1, q2, qt1, qt2, next_lp, reward, done))]
        la = L.tensor_arg('hope_env_sac_critic', 'log_alpha', log_alpha, torch.float64, (), self.device)
        out = self._sac_outputs('critic', b, ((b,), (b,), (b,), (2,)))
        outs = [arg(k, x, shape=tuple(x.shape)) for k, x in zip(('q_target', 'g_q1', 'g_q2', 'losses'), out)]
        L.check(self.lib.hope_env_sac_critic(self.h, *ins, la, float(gamma), b, *outs, self._stream()), 'hope_env_sac_critic')
        return out

    def sac_seed(self, q1, q2):
        """q1, q2: the critics at the sampled action, float32 [B] -> (s1 [B], s2 [B]), the gradient of -mean(min(q1, q2)) at them:
        persistent per B.  One launch, no host synchronisation."""
        arg = partial(L.tensor_arg, 'hope_env_sac_seed', dtype=torch.float32, device=self.device)
        b = int(q1.shape[0]) if hasattr(q1, 'shape') and len(q1.shape) == 1 else None
        ins = [arg('q1', q1, shape=(b,)), arg('q2', q2, shape=(b,))]
        out = self._sac_outputs('seed', b, ((b,), (b,)))
        L.check(self.lib.hope_env_sac_seed(self.h, *ins, b, *(arg(k, x, shape=(b,)) for k, x in zip(('s1', 's2'), out)), self._stream()), 'hope_env_sac_seed')
        return out

    def sac_policy(self, raw, log_std, eps, q1, q2, g_action, log_alpha, target_entropy):
        """raw, log_std, eps as for sac_sample; q1, q2 [B] the critics at the sampled action; g_action [B, 2] the gradient the seeds give
        there; log_alpha: a float64 scalar tensor on the device
        -> (g_raw [B, 2], g_log_std [2], g_log_alpha (a float64 scalar tensor), losses [2] = actor, temperature): persistent per B.
        Two launches, no host synchronisation."""
        arg = partial(L.tensor_arg, 'hope_env_sac_policy', dtype=torch.float32, device=self.device)
        b = int(raw.shape[0]) if hasattr(raw, 'shape') and len(raw.shape) == 2 else None
        ins = [arg('raw', raw, shape=(b, 2)), arg('log_std', log_std, shape=(2,)), arg('eps', eps, shape=(b, 2)), arg('q1', q1, shape=(b,)),
               arg('q2', q2, shape=(b,)), arg('g_action', g_action, shape=(b, 2))]
        la = L.tensor_arg('hope_env_sac_policy', 'log_alpha', log_alpha, torch.float64, (), self.device)
        out = self._sac_outputs('policy', b, ((b, 2), (2,), None, (2,)))
        outs = [arg('g_raw', out[0], shape=(b, 2)), arg('g_log_std', out[1], shape=(2,)),
                L.tensor_arg('hope_env_sac_policy', 'g_log_alpha', out[2], torch.float64, (), self.device), arg('losses', out[3], shape=(2,))]
        L.check(self.lib.hope_env_sac_policy(self.h, *ins, la, float(target_entropy), b, *outs, self._stream()), 'hope_env_sac_policy')
        return out

    # -- the policy's inference forward on the device (hope_env.h; rule: csrc/hope_policy_core.h) ----------------------
    def enable_policy(self, n_tokens=3, out_dim=2, tanh_out=True, max_batch=None):
        """HopeNet's inference forward for the reference configuration as one fused kernel (k_policy_forward) over parameters that
        k_policy_pack lays out in the handle.  n_tokens 3, or 4 with a ready-made image token; out_dim 2 with tanh_out for an actor,
        1 without for a PPO critic; max_batch: the largest batch (default: the env's scenes).  Another shape drops the loaded
        parameters.  ValueError for a shape that is not compiled in.  Off by default."""
        shape = (int(n_tokens), int(out_dim), int(bool(tanh_out)))
        if shape[0] not in (3, 4) or shape[1] not in (1, 2):
            raise ValueError(f'enable_policy: n_tokens must be 3 or 4 and out_dim 1 or 2, not {n_tokens} and {out_dim}')
        torch.cuda.synchronize(self.device)
        L.check(self.lib.hope_env_policy_enable(self.h, *shape, int(self.n if max_batch is None else max_batch)), 'hope_env_policy_enable')
        if shape != self._policy_shape:
            self._policy_shape, self._policy_out, self._policy_held, self._policy_owner = shape, {}, None, None
        return self

    def disable_policy(self):
        torch.cuda.synchronize(self.device)
        L.check(self.lib.hope_env_policy_disable(self.h), 'hope_env_policy_disable')
        self._policy_shape, self._policy_out, self._policy_held, self._policy_owner = None, {}, None, None
        return self

    def policy_load(self, module):
        """pack the parameters of `module` (a policy.HopeNet of the enabled shape, float32 on this device) into the handle: one
        launch on the current stream, no host synchronisation; the module's tensors are held until the next load.  ValueError for a
        net of another configuration (nothing changes)."""
        shape = L.policy_shape(module)
        if self._policy_shape is None:
            raise L.HopeError('hope_env_policy_load: the policy forward is off (enable_policy first)')
        if shape != self._policy_shape:
            raise ValueError(f'policy_load: the net is (n_tokens, out_dim, tanh_out) = {shape}, the handle was enabled for {self._policy_shape}')
        p, keep = L.policy_params('hope_env_policy_load', module, self.device)
        L.check(self.lib.hope_env_policy_load(self.h, C.byref(p), self._stream()), 'hope_env_policy_load')
        self._policy_held, self._policy_owner = keep, None
        return self

    def policy_forward(self, lidar, target, mask, img_token=None, out=None):
        """lidar [B, 120], target [B, 5], mask [B, 42], img_token [B, 128] (n_tokens 4) or None: float32 contiguous
        -> out [B, out_dim], a persistent tensor per B (overwritten by the next call with that B) unless `out` is given.  One launch
        on the current stream, no host synchronisation."""
        arg = partial(L.tensor_arg, 'hope_env_policy_forward', dtype=torch.float32, device=self.device)
        b = int(lidar.shape[0]) if hasattr(lidar, 'shape') and len(lidar.shape) == 2 else None
        ins = [arg('lidar', lidar, shape=(b, L.LIDAR_NUM)), arg('target', target, shape=(b, L.TARGET_DIM)), arg('mask', mask, shape=(b, L.N_ACTION)),
               arg('img_token', img_token, shape=(b, 128), optional=True)]
        od = self._policy_shape[1] if self._policy_shape is not None else 2
        if out is None:
            out = self._policy_out.get(b)
            if out is None:
                out = self._policy_out[b] = torch.zeros((b, od), dtype=torch.float32, device=self.device)
        L.check(self.lib.hope_env_policy_forward(self.h, *ins, b, arg('out', out, shape=(b, od)), self._stream()), 'hope_env_policy_forward')
        return out

    # -- the critics' inference forward on the device (hope_env.h; rule: csrc/hope_critic_core.h) ----------------------
    def enable_critics(self, n_slots=2, has_img=False, has_action=False, max_batch=None):
        """the no-gradient forward of up to `n_slots` (1 .. 4) critic nets of one shape over one set of inputs as one fused kernel
        (k_critic_forward) over parameter slots that k_critic_pack fills.  has_img: the nets take a ready-made image token; has_action:
        they are SacCritics (a 2-wide action token); max_batch: the largest batch (default: the env's scenes).  The same n_slots and
        shape again keeps the loaded slots; anything else drops them.  Independent of enable_policy.  Off by default."""
        shape = (int(n_slots), int(bool(has_img)), int(bool(has_action)))
        if not 1 <= shape[0] <= L.CRITIC_SLOTS:
            raise ValueError(f'enable_critics: n_slots must be 1 .. {L.CRITIC_SLOTS}, not {n_slots}')
        torch.cuda.synchronize(self.device)
        L.check(self.lib.hope_env_critic_enable(self.h, *shape, int(self.n if max_batch is None else max_batch)), 'hope_env_critic_enable')
        if shape != self._critic_shape:
            self._critic_shape, self._critic_out, self._critic_held, self._critic_owner = shape, {}, {}, {}
        return self

    def disable_critics(self):
        torch.cuda.synchronize(self.device)
        L.check(self.lib.hope_env_critic_disable(self.h), 'hope_env_critic_disable')
        self._critic_shape, self._critic_out, self._critic_held, self._critic_owner = None, {}, {}, {}
        return self

    def critic_load(self, slot, net):
        """pack the parameters of `net` (a critic policy.HopeNet or a policy.SacCritic of the enabled shape, float32 on this device)
        into slot `slot`: one launch on the current stream, no host synchronisation; the net's tensors are held until the slot's next
        load.  ValueError for a net of another configuration (nothing changes)."""
        shape = L.critic_shape(net)
        if self._critic_shape is None:
            raise L.HopeError("hope_env_critic_load: the critics' forward is off (enable_critics first)")
        if shape != self._critic_shape[1:]:
            raise ValueError(f'critic_load: the net is (has_img, has_action) = {shape}, the handle was enabled for {self._critic_shape[1:]}')
        p, keep = L.critic_params('hope_env_critic_load', net, self.device)
        L.check(self.lib.hope_env_critic_load(self.h, int(slot), C.byref(p), self._stream()), 'hope_env_critic_load')
        self._critic_held[int(slot)] = keep
        self._critic_owner.pop(int(slot), None)
        return self

    def critic_forward(self, slots, lidar, target, mask, img_token=None, action=None, out=None):
        """slots: the n slots to evaluate, in the order of the result's rows; lidar [B, 120], target [B, 5], mask [B, 42], img_token
        [n, B, 128] (has_img; token i for slots[i]) or None, action [B, 2] (has_action) or None: float32 contiguous -> out [n, B], a
        persistent tensor per (n, B) (overwritten by the next call with that n and B) unless `out` is given.  One launch on the current
        stream, no host synchronisation."""
        arg = partial(L.tensor_arg, 'hope_env_critic_forward', dtype=torch.float32, device=self.device)
        sl = [int(s) for s in slots]
        n = len(sl)
        b = int(lidar.shape[0]) if hasattr(lidar, 'shape') and len(lidar.shape) == 2 else None
        ins = [arg('lidar', lidar, shape=(b, L.LIDAR_NUM)), arg('target', target, shape=(b, L.TARGET_DIM)), arg('mask', mask, shape=(b, L.N_ACTION)),
               arg('img_token', img_token, shape=(n, b, 128), optional=True), arg('action', action, shape=(b, 2), optional=True)]
        if out is None:
            out = self._critic_out.get((n, b))
            if out is None:
                out = self._critic_out[(n, b)] = torch.zeros((n, b), dtype=torch.float32, device=self.device)
        L.check(self.lib.hope_env_critic_forward(self.h, (C.c_int * max(n, 1))(*sl), n, *ins, b, arg('out', out, shape=(n, b)), self._stream()),
                'hope_env_critic_forward')
        return out

    # -- the optimiser block on the device (hope_env.h; rule: csrc/hope_optim_core.h) ---------------------------------
    def optim_adam(self, params, grads, exp_avgs, exp_avg_sqs, groups, group_of=None):
        """one Adam step over the tensors params[i] with gradients grads[i] and state exp_avgs[i], exp_avg_sqs[i] (float32 or float64,
        contiguous, on this device), updated in place.  groups: 1 .. 4 `_lib.OptimGroup`s (`_lib.optim_group`); group_of[i]: the
        group of entry i (default 0).  ceil(len / 64) launches of k_optim on the current stream, no host synchronisation; nothing
        is kept.  ValueError for tensors that do not go together (`_lib.optim_entries`)."""
        table, n, _keep = L.optim_entries(params, grads, exp_avgs, exp_avg_sqs, group_of, 'hope_env_optim_adam', self.device)
        garr = (L.OptimGroup * max(len(groups), 1))(*groups)
        L.check(self.lib.hope_env_optim_adam(self.h, table, n, garr, len(groups), self._stream()), 'hope_env_optim_adam')
        return self

    def optim_polyak(self, targets, currents, tau):
        """targets[i] <- (1 - tau) * targets[i] + tau * currents[i], in place: the same launches, the same rules."""
        table, n, _keep = L.optim_entries(targets, currents, call='hope_env_optim_polyak', device=self.device)
        L.check(self.lib.hope_env_optim_polyak(self.h, table, n, float(tau), self._stream()), 'hope_env_optim_polyak')
        return self

    # -- the image encoder's inference forward on the device (hope_env.h; rule: csrc/hope_imgenc_core.h) ----------------
    def enable_img_encoder(self, act='tanh', max_batch=None):
        """HopeNet's image token (the two convolution blocks, fc1, output_mean, re_embed_img) for the reference configuration as two
        kernels (k_imgenc_conv, k_imgenc_head) over parameters that k_imgenc_pack lays out in the handle.  act: 'tanh' or 'leaky';
        max_batch: the largest batch (default: the env's scenes); the handle keeps a feature buffer of 8 KiB per image of it.  Independent
        of enable_policy.  Off by default."""
        if act not in ('tanh', 'leaky', 0, 1):
            raise ValueError(f"enable_img_encoder: act must be 'tanh' or 'leaky', not {act!r}")
        a = {'tanh': 0, 'leaky': 1}.get(act, act)
        mb = int(self.n if max_batch is None else max_batch)
        torch.cuda.synchronize(self.device)
        L.check(self.lib.hope_env_imgenc_enable(self.h, a, mb), 'hope_env_imgenc_enable')
        self._imgenc_act, self._imgenc_max = a, max(self._imgenc_max, mb)
        return self

    def disable_img_encoder(self):
        torch.cuda.synchronize(self.device)
        L.check(self.lib.hope_env_imgenc_disable(self.h), 'hope_env_imgenc_disable')
        self._imgenc_act, self._imgenc_max, self._imgenc_out, self._imgenc_held, self._imgenc_owner = None, 0, {}, None, None
        return self

    def img_encoder_load(self, module):
        """pack the 14 encoder tensors of `module` (a policy.HopeNet with an image token, float32 on this device) into the handle: one
        launch on the current stream, no host synchronisation; the tensors are held until the next load.  ValueError for a net of
        another configuration or activation (nothing changes)."""
        act = L.imgenc_shape(module)
        if self._imgenc_act is None:
            raise L.HopeError('hope_env_imgenc_load: the image encoder is off (enable_img_encoder first)')
        if act != self._imgenc_act:
            raise ValueError(f"img_encoder_load: the net's encoder activation is {('tanh', 'leaky')[act]}, the handle was enabled for "
                             f"{('tanh', 'leaky')[self._imgenc_act]}")
        p, keep = L.imgenc_params('hope_env_imgenc_load', module, self.device)
        L.check(self.lib.hope_env_imgenc_load(self.h, C.byref(p), self._stream()), 'hope_env_imgenc_load')
        self._imgenc_held, self._imgenc_owner = keep, None
        return self

    def img_encoder_forward(self, img, out=None, features=False):
        """img uint8 [B, 3, 64, 64] contiguous (the env's own `img` goes in without a copy) -> token float32 [B, 128], a persistent
        tensor per B (overwritten by the next call with that B) unless `out` is given.  features: True -> (token, features [B, 2048],
        persistent per B), or a float32 [B, 2048] tensor to receive them.  Two launches on the current stream, no host synchronisation."""
        name = 'hope_env_imgenc_forward'
        b = int(img.shape[0]) if hasattr(img, 'shape') and len(img.shape) == 4 else None
        im = L.tensor_arg(name, 'img', img, torch.uint8, (b, 3, 64, 64), self.device)
        keep = self._imgenc_out.setdefault(b, [None, None])
        if out is None:
            if keep[0] is None:
                keep[0] = torch.zeros((b, 128), dtype=torch.float32, device=self.device)
            out = keep[0]
        feat = None
        if features is True:
            if keep[1] is None:
                keep[1] = torch.zeros((b, 2048), dtype=torch.float32, device=self.device)
            feat = keep[1]
        elif features is not False and features is not None:
            feat = features
        L.check(self.lib.hope_env_imgenc_forward(self.h, im, b, L.tensor_arg(name, 'out', out, torch.float32, (b, 128), self.device),
                                                 L.tensor_arg(name, 'features', feat, torch.float32, (b, 2048), self.device, optional=True), self._stream()), name)
        return out if feat is None else (out, feat)

    # -- bookkeeping of an evaluation run on the device (hope_env.h; rule: csrc/hope_evaltrack_core.h) ------------------
    def enable_eval_tracker(self):
        """eval()'s per-episode tally (eval_utils.py:35-57) as device state of the handle (80 B per scene) and three kernels:
        k_eval_begin, k_eval_override, k_eval_track.  The stuck detector draws from the physical action box (tables.VALID_STEER /
        VALID_SPEED).  Enabling again keeps the state.  Off by default."""
        torch.cuda.synchronize(self.device)
        box = L.array_arg('hope_env_eval_enable', 'box', T.VALID_STEER + T.VALID_SPEED, np.float64, (4,))
        L.check(self.lib.hope_env_eval_enable(self.h, box.ctypes), 'hope_env_eval_enable')
        if self.eval_alive is None:
            dev = self.device
            self.eval_alive = torch.zeros(self.n, dtype=torch.uint8, device=dev)
            self.eval_word = torch.zeros((self.n, 8), dtype=torch.int8, device=dev)
            self.eval_done = torch.zeros(self.n, dtype=torch.uint8, device=dev)
            self._eval_rec = torch.zeros((self.n, 4), dtype=torch.float32, device=dev)
        return self

    def disable_eval_tracker(self):
        torch.cuda.synchronize(self.device)
        L.check(self.lib.hope_env_eval_disable(self.h), 'hope_env_eval_disable')
        return self

    def eval_begin(self, target=None, pose=None):
        """a new episode in every scene, from the first observation (None: the env's own target / pose); one k_eval_begin launch on
        the current stream, no host synchronisation"""
        tp = L.tensor_arg('hope_env_eval_begin', 'target', self.target if target is None else target, self.obs_dtype, (self.n, 5), self.device)
        pp = L.tensor_arg('hope_env_eval_begin', 'pose', self.pose if pose is None else pose, torch.float64, (self.n, 3), self.device)
        L.check(self.lib.hope_env_eval_begin(self.h, tp, pp, self._stream()), 'hope_env_eval_begin')
        return self

    def eval_override(self, actions, u=None, seed=0, counter=0):
        """the stuck detector's random action, in place: the rows of `actions` ([N, 2] float32 or float64, contiguous) of the scenes
        whose target did not change in the last step are replaced by the clipped draw from the physical action box.  u f64 [N, 2] in
        [0, 1) or None: counter-based draws keyed by (seed, counter, scene, dimension).  One k_eval_override launch, no host
        synchronisation.  -> eval_alive (uint8 [N], persistent): the scenes whose episode is still running -- step()'s `active`."""
        n, arg = self.n, partial(L.tensor_arg, 'hope_env_eval_override', device=self.device)
        ap = arg('actions', actions, (torch.float32, torch.float64), (n, 2))
        up = arg('u', u, torch.float64, (n, 2), optional=True)
        lp = arg('eval_alive', self.eval_alive, torch.uint8, (n,), optional=True)    # (None: the library reports that the tracker is off)
        L.check(self.lib.hope_env_eval_override(self.h, ap, int(actions.dtype == torch.float64), up, L.seed64(seed), L.seed64(counter), lp,
                                                self._stream()), 'hope_env_eval_override')
        return self.eval_alive

    def eval_track(self, target=None, pose=None, reward=None, status=None, done=None, rs_word=None):
        """the tally of the step just taken (None: the env's own outputs); one k_eval_track launch on the current stream, no host
        synchronisation, no wait for a deferred search.  -> (eval_word int8 [N, 8]: rs_word with the found flag cleared for frozen
        scenes, eval_done uint8 [N]: episodes that ended in this step): persistent tensors, overwritten by the next call."""
        n, arg = self.n, partial(L.tensor_arg, 'hope_env_eval_track', device=self.device)
        ptrs = [arg('target', self.target if target is None else target, self.obs_dtype, (n, 5)),
                arg('pose', self.pose if pose is None else pose, torch.float64, (n, 3)),
                arg('reward', self.reward if reward is None else reward, self.obs_dtype, (n,)),
                arg('status', self.status if status is None else status, torch.int32, (n,)),
                arg('done', self.done if done is None else done, torch.uint8, (n,)),
                arg('rs_word', self.rs_word if rs_word is None else rs_word, torch.int8, (n, 8)),
                arg('eval_word', self.eval_word, torch.int8, (n, 8), optional=True),    # (None: the library reports that the tracker is off)
                arg('eval_done', self.eval_done, torch.uint8, (n,), optional=True)]
        L.check(self.lib.hope_env_eval_track(self.h, *ptrs, self._stream()), 'hope_env_eval_track')
        return self.eval_word, self.eval_done

    def eval_records(self):
        """-> float32 [N, 4]: status, steps, summed reward, path length of every scene's episode so far (a persistent tensor,
        overwritten by the next call); one launch, no host synchronisation"""
        rp = L.tensor_arg('hope_env_eval_records', 'records', self._eval_rec, torch.float32, (self.n, 4), self.device, optional=True)
        L.check(self.lib.hope_env_eval_records(self.h, rp, self._stream()), 'hope_env_eval_records')
        return self._eval_rec

    def eval_state(self):
        """the tracker's state block (numpy uint64 [10, N]: previous target, previous position, summed reward, path length as
        float64 bits, the packed steps / status / alive / stuck word) -- host-synchronous; tests"""
        out = np.zeros((L.EVAL_STATE_WORDS, self.n), np.uint64)
        L.check(self.lib.hope_env_eval_download_state(self.h, out.ctypes), 'hope_env_eval_download_state')
        return out

    def queue_check(self):
        """hope_env_create's measurement of which library streams share a hardware queue (hope_env_queue_check):
        {'queue_of_role': [8 ints, [0] = the NULL stream], 'distinct_queues': n, 'roles_shared': pairs of roles busy in the same step
        form that sit on one queue, 'ms': cost of the measurement}"""
        q = (C.c_int32 * 8)()
        n, ms = C.c_int32(0), C.c_double(0)
        L.check(self.lib.hope_env_queue_check(self.h, q, C.byref(n), C.byref(ms)), 'hope_env_queue_check')
        q = [int(v) for v in q]
        shared = []
        for group in ((0, 5, 1, 3), (0, 1, 3, 4), (5, 1, 3, 7)):
            for i, a in enumerate(group):
                for b in group[i + 1:]:
                    if q[a] >= 0 and q[a] == q[b] and [a, b] not in shared:
                        shared.append([a, b])
        return {'queue_of_role': q, 'distinct_queues': int(n.value), 'roles_shared': shared, 'ms': float(ms.value)}

    def n_obst_now(self):
        """obstacle count of every scene as it is on the device now (device-side draws change it): numpy int32 [N]"""
        out = np.zeros(self.n, np.int32)
        L.check(self.lib.hope_env_download_n_obst(self.h, out.ctypes), 'hope_env_download_n_obst')
        return out

    def map_levels(self, active=None, out=None, detail=False):
        """`map.map_level` of the maps the scenes hold NOW (pool draws, Dragon-Lake draws and uploads alike), labelled on the device
        by k_map_level (asynchronous on the current stream) -> torch.uint8 [N], 0 Normal / 1 Complex / 2 Extrem
        (hope_amd.map_level.LEVEL_NAMES) [, int32 [N, 8] detail].  active: u8 [N]; scenes with active[i] == 0 keep out[i] (pass the
        last step's `done` and the previous labels as `out` to relabel only the scenes that drew a new map)."""
        if out is None:
            out = torch.zeros(self.n, dtype=torch.uint8, device=self.device)
        arg = partial(L.tensor_arg, 'hope_env_map_level', device=self.device)
        det = None
        if detail is not False and detail is not None:
            det = detail if torch.is_tensor(detail) else torch.zeros((self.n, 8), dtype=torch.int32, device=self.device)
        ap, op = arg('active', active, torch.uint8, (self.n,), optional=True), arg('out', out, torch.uint8, (self.n,))
        dp = arg('detail', det, torch.int32, (self.n, 8), optional=True)
        L.check(self.lib.hope_env_map_level(self.h, ap, op, dp, self._stream()), 'hope_env_map_level')
        return (out, det) if det is not None else out

    def restart(self, mask):
        """episodes flagged in mask (u8 [N]) go back to their start pose, t = 0 (same map)."""
        mp = L.tensor_arg('hope_env_restart', 'mask', mask, torch.uint8, (self.n,), self.device)
        L.check(self.lib.hope_env_restart(self.h, mp, self._stream()), 'hope_env_restart')
        return self

    def kernel_ms(self, reset=True):
        """{kernel name: (accumulated ms, launches)} from the library's per-launch HIP events (profile=True)."""
        ms = np.zeros(len(L.KERNELS))
        cnt = np.zeros(len(L.KERNELS), np.int64)
        L.check(self.lib.hope_env_kernel_ms(self.h, ms.ctypes, cnt.ctypes, int(reset)), 'hope_env_kernel_ms')
        return {k: (float(ms[i]), int(cnt[i])) for i, k in enumerate(L.KERNELS)}

    def kernel_union_ms(self, reset=True):
        """{kernel name: (accumulated ms during which >= 1 launch of the kernel ran, calls)}: per step call the UNION of the
        kernel's launch intervals (the two tile classes overlap on two streams).  Read it before kernel_ms(reset=True)."""
        ms = np.zeros(len(L.KERNELS))
        cnt = np.zeros(len(L.KERNELS), np.int64)
        L.check(self.lib.hope_env_kernel_union_ms(self.h, ms.ctypes, cnt.ctypes, int(reset)), 'hope_env_kernel_union_ms')
        return {k: (float(ms[i]), int(cnt[i])) for i, k in enumerate(L.KERNELS)}

    def profile_kernels(self, names=None):
        """time only the listed kernels (names from _lib.KERNELS; None = all) -- every event pair costs launch latency"""
        mask = 0xffffffff if names is None else sum(1 << L.KERNELS.index(k) for k in names)
        L.check(self.lib.hope_env_profile_kernels(self.h, mask), 'hope_env_profile_kernels')

    def obs(self, clone=False):
        """the observation dict in the reference's key order (car_parking_base.py:399-407).  The tensors are this
        object's persistent output buffers: the next step()/reset_obs() overwrites them IN PLACE (asynchronously), so
        `obs = env.obs(); env.step(a); next_obs = env.obs()` aliases obs and next_obs -- pass clone=True (or copy what
        you keep before stepping, as hope_amd.rollout does) when both are needed."""
        o = {'img': self.img, 'lidar': self.lidar, 'target': self.target, 'action_mask': self.action_mask}
        return {k: (v.clone() if (clone and v is not None) else v) for k, v in o.items()}

    def download_outputs(self):
        """every output of the last step on the host, through ONE device-to-host copy of the output arena into pinned memory (and one
        stream synchronisation): {name: numpy view}.  The views alias the pinned buffer: valid until the next call."""
        if self._arena_host is None:
            self._arena_host = torch.empty(self._arena.shape, dtype=torch.uint8, pin_memory=True)
        self._arena_host.copy_(self._arena, non_blocking=True)
        torch.cuda.current_stream(self.device).synchronize()
        hb = self._arena_host.numpy()
        np_dt = {torch.float32: np.float32, torch.float64: np.float64, torch.int32: np.int32, torch.uint8: np.uint8, torch.int8: np.int8}
        return {name: hb[o:o + nbytes].view(np_dt[dt]).reshape(shape) for name, (o, nbytes, shape, dt) in self._layout.items()}

    # -- state -------------------------------------------------------------------------------------
    def download_state(self):
        pose, t, acc = np.zeros((self.n, 3)), np.zeros(self.n, np.int32), np.zeros(self.n)
        L.check(self.lib.hope_env_download_state(self.h, pose.ctypes, t.ctypes, acc.ctypes), 'hope_env_download_state')
        return pose, t, acc

    def upload_state(self, pose=None, t=None, accum=None):
        a = [L.array_arg('hope_env_upload_state', 'pose', pose, np.float64, (self.n, 3), optional=True),
             L.array_arg('hope_env_upload_state', 't', t, np.int32, (self.n,), optional=True),
             L.array_arg('hope_env_upload_state', 'accum', accum, np.float64, (self.n,), optional=True)]
        L.check(self.lib.hope_env_upload_state(self.h, *[None if x is None else x.ctypes for x in a]), 'hope_env_upload_state')

    def close(self):
        if getattr(self, 'h', None):
            self.lib.hope_env_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
