"""ParkingBatch -- N independent parking scenes stepped on one MI355X through libhope_env.so.

Tensor-in / tensor-out counterpart of `CarParkingWrapper.step` (src/env/env_wrapper.py:73-81) for N >> 1.
PyTorch is used for device memory and streams only; all arithmetic is in the HIP kernels.
"""
import ctypes as C

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
        assert obs_dtype in (torch.float32, torch.float64) and action_dtype in (torch.float32, torch.float64)
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
        ds, hb, ab = (np.ascontiguousarray(t[k], dtype=np.float64) for k in ('dist_star', 'hull_base', 'beam_ab'))
        assert ds.shape == (1200, 42, 10) and hb.shape == (120,) and ab.shape == (120, 2)
        L.check(self.lib.hope_env_upload_tables(self.h, ds.ctypes.data, hb.ctypes.data, ab.ctypes.data),
                'hope_env_upload_tables')
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

    # -- scenes ------------------------------------------------------------------------------------
    def set_scenes(self, ids, scenes):
        """map.reset + vehicle.reset for the listed scene slots (host -> device; synchronous)."""
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        start, dest, bbox, verts, nob, _nv = pack_scenes(scenes, self.max_obst)
        self.set_scene_arrays(ids, start, dest, bbox, verts, nob)

    def set_draw_class(self, ids, cls):
        """size class of scene slots (0: lots of <= 32 obstacles, 1: larger lots / Dragon-Lake cases): which launch chain steps a
        slot and which pool entries it draws at turnover; set_scenes derives it from the obstacle count of the uploaded map"""
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        c = np.ascontiguousarray(np.broadcast_to(np.asarray(cls, dtype=np.uint8), ids.shape))
        torch.cuda.synchronize(self.device)
        L.check(self.lib.hope_env_set_draw_class(self.h, ids.ctypes.data, len(ids), c.ctypes.data), 'hope_env_set_draw_class')
        return self

    def set_scene_arrays(self, ids, start, dest, bbox, verts, n_obst):
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        a = [np.ascontiguousarray(x, dtype=np.float64) for x in (start, dest, bbox, verts)]
        nob = np.ascontiguousarray(n_obst, dtype=np.int32)
        assert a[3].shape == (len(ids), self.max_obst, 4, 2)
        torch.cuda.synchronize(self.device)
        L.check(self.lib.hope_env_set_scenes(self.h, ids.ctypes.data, len(ids), a[0].ctypes.data, a[1].ctypes.data,
                                             a[2].ctypes.data, a[3].ctypes.data, nob.ctypes.data),
                'hope_env_set_scenes')

    def set_pool(self, scenes):
        """upload a pool of complete scenes (list[Scene] or the tuple pack_scenes returns) that redraw() draws from"""
        start, dest, bbox, verts, nob, _nv = pack_scenes(scenes, self.max_obst) if isinstance(scenes, list) else scenes
        a = [np.ascontiguousarray(x, dtype=np.float64) for x in (start, dest, bbox, verts)]
        nob = np.ascontiguousarray(nob, dtype=np.int32)
        if getattr(self, '_refresher_filling', False):
            raise L.HopeError('set_pool while a PoolRefresher fill is running: the pinned staging arrays are being written by its '
                              'thread (close() / poll(wait=True) the refresher first)')
        torch.cuda.synchronize(self.device)
        L.check(self.lib.hope_env_set_pool(self.h, len(nob), a[0].ctypes.data, a[1].ctypes.data, a[2].ctypes.data,
                                           a[3].ctypes.data, nob.ctypes.data), 'hope_env_set_pool')
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
        L.check(self.lib.hope_env_generate_pool(self.h, int(n_pool), counts, C.c_uint64(int(seed) & (2 ** 64 - 1)),
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
        b = np.ascontiguousarray(buckets, dtype=np.uint8)
        torch.cuda.synchronize(self.device)
        L.check(self.lib.hope_env_set_pool_buckets(self.h, len(b), b.ctypes.data), 'hope_env_set_pool_buckets')
        return self

    def curriculum_tally(self):
        """count the episodes the last step finished (its own status / done buffers), asynchronously on the current stream"""
        L.check(self.lib.hope_env_curriculum_tally(self.h, C.c_void_p(self.status.data_ptr()), C.c_void_p(self.done.data_ptr()),
                                                   self._stream()), 'hope_env_curriculum_tally')
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
        L.check(self.lib.hope_env_curriculum_state(self.h, C.byref(nb), None, None, None, None, None, None, misc.ctypes.data), 'hope_env_curriculum_state')
        out = {'on': bool(misc[3]), 'updates': int(misc[0]), 'n_buckets': int(nb.value)}
        if not out['on']:
            return out
        n = nb.value
        e, s = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
        wn, ws, prob, pw = np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(4)
        L.check(self.lib.hope_env_curriculum_state(self.h, None, e.ctypes.data, s.ctypes.data, wn.ctypes.data, ws.ctypes.data, prob.ctypes.data,
                                                   pw.ctypes.data, misc.ctypes.data), 'hope_env_curriculum_state')
        out.update(episodes=e, successes=s, win_n=wn, win_s=ws, prob=prob, q=prob[:4].copy(), pw=pw, updates=int(misc[0]),
                   unlabelled_episodes=int(misc[1]), unlabelled_successes=int(misc[2]))
        return out

    def curriculum_set_windows(self, win_n, win_s, episodes, successes):
        """set the windows and cumulative counters by hand (checkpoint restore, tests) and rebuild the lists from them"""
        a = [np.ascontiguousarray(win_n, dtype=np.float64), np.ascontiguousarray(win_s, dtype=np.float64),
             np.ascontiguousarray(episodes, dtype=np.uint64), np.ascontiguousarray(successes, dtype=np.uint64)]
        torch.cuda.synchronize(self.device)
        L.check(self.lib.hope_env_curriculum_set_windows(self.h, len(a[0]), *[x.ctypes.data for x in a]), 'hope_env_curriculum_set_windows')
        return self

    def curriculum_lists(self):
        """(list of class 0, list of class 1, positions [2, n_buckets]) as the next step reads them; a class without entries: all -1"""
        nb = C.c_int32(0)
        L.check(self.lib.hope_env_curriculum_state(self.h, C.byref(nb), None, None, None, None, None, None, None), 'hope_env_curriculum_state')
        l0, l1 = np.full(L.CURRICULUM_LIST_LEN, -1, np.int32), np.full(L.CURRICULUM_LIST_LEN, -1, np.int32)
        pos = np.zeros((2, nb.value), np.int32)
        L.check(self.lib.hope_env_curriculum_download_lists(self.h, l0.ctypes.data, l1.ctypes.data, pos.ctypes.data), 'hope_env_curriculum_download_lists')
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
        dest = np.ascontiguousarray(pool.dest, dtype=np.float64)
        cand_off = np.ascontiguousarray(pool.start_off, dtype=np.int32)
        cand = np.ascontiguousarray(pool.starts, dtype=np.float64)
        case_set = np.ascontiguousarray(pool.case_set, dtype=np.int32)
        set_off = np.ascontiguousarray(pool.set_off, dtype=np.int32)
        sv = np.array(pool.set_verts, dtype=np.float64)          # [total][4][2]; triangles repeat their last vertex
        tri = np.asarray(pool.set_nvert) == 3
        sv[tri, 3] = sv[tri, 2]
        sv = np.ascontiguousarray(sv)
        torch.cuda.synchronize(self.device)
        L.check(self.lib.hope_env_set_dlp_cases(self.h, len(dest), dest.ctypes.data, cand_off.ctypes.data, cand.ctypes.data,
                                                case_set.ctypes.data, len(set_off) - 1, set_off.ctypes.data, sv.ctypes.data),
                'hope_env_set_dlp_cases')
        self.n_dlp_cases = len(dest)
        return self

    def pool_overflow(self):
        out = np.zeros(1, np.int32)
        L.check(self.lib.hope_env_pool_overflow(self.h, out.ctypes.data), 'hope_env_pool_overflow')
        return int(out[0])

    def download_scenes(self, ids):
        """the maps the listed scene slots hold now -> (start, dest, bbox, verts, n_obst) (host arrays)"""
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        n = len(ids)
        start, dest, bbox = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((n, 4))
        verts, nob = np.zeros((n, self.max_obst, 4, 2)), np.zeros(n, np.int32)
        L.check(self.lib.hope_env_download_scenes(self.h, ids.ctypes.data, n, start.ctypes.data, dest.ctypes.data, bbox.ctypes.data,
                                                  verts.ctypes.data, nob.ctypes.data), 'hope_env_download_scenes')
        return start, dest, bbox, verts, nob

    def pool_state(self):
        """(pool index, episode counter) of every scene: with download_state() and pool_generation() the whole snapshot of a
        run that draws maps from a pool that is NOT replaced in the meantime (refreshed runs: download_scenes / set_scene_arrays)"""
        idx, ep = np.zeros(self.n, np.int32), np.zeros(self.n, np.uint32)
        L.check(self.lib.hope_env_download_pool_state(self.h, idx.ctypes.data, ep.ctypes.data), 'hope_env_download_pool_state')
        return idx, ep

    def restore_maps(self, pool_index, episode, seed, generation=0):
        """repeat the draws of a snapshot (the seed in use then); `generation` = pool_generation() saved with the snapshot: the
        call fails (HOPE_ESTATE) if the pool has been replaced since -- the draws would return other maps; 0 skips the check.
        Follow with upload_state()"""
        drawn = np.ascontiguousarray(np.asarray(pool_index) != -1, dtype=np.uint8)
        ep = np.ascontiguousarray(episode, dtype=np.uint32)
        L.check(self.lib.hope_env_restore_maps(self.h, drawn.ctypes.data, ep.ctypes.data, C.c_uint64(int(seed) & (2 ** 64 - 1)),
                                               C.c_uint64(int(generation))), 'hope_env_restore_maps')
        return self

    def redraw(self, mask, seed=0):
        """map.reset for the flagged scenes: each takes a pool scene of its tile class and restarts (asynchronous)"""
        assert mask.dtype == torch.uint8 and mask.shape == (self.n,) and mask.device == self.device
        L.check(self.lib.hope_env_redraw(self.h, C.c_void_p(mask.data_ptr()), C.c_uint64(int(seed) & (2 ** 64 - 1)), self._stream()),
                'hope_env_redraw')
        return self

    def turnover(self, seed=0):
        """episode turnover with a NEW map, as the reference's training loop does (`env.reset(...)` after `done`):
        finished scenes draw a pool scene and get their first observation; reward / reward_info / status / done / RS
        outputs keep the values of the finished step (like auto_reset)."""
        self._done_mask.copy_(self.done)
        self.redraw(self._done_mask, seed)
        stages = L.STAGE_ALL | (L.STAGE_IMG if self.image else 0)
        L.check(self.lib.hope_env_reset_obs(self.h, C.c_void_p(self._done_mask.data_ptr()), stages, C.byref(self._out_obs),
                                            self._stream()), 'hope_env_reset_obs')
        return self

    def pool_index(self):
        out = np.zeros(self.n, np.int32)
        L.check(self.lib.hope_env_download_pool_index(self.h, out.ctypes.data), 'hope_env_download_pool_index')
        return out

    # -- the hot path ------------------------------------------------------------------------------
    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def reset_obs(self, active=None, stages=L.STAGE_ALL):
        """the action-less step of CarParking.reset (car_parking_base.py:138)."""
        if self.image and (stages & L.STAGE_ALL) == L.STAGE_ALL:
            stages |= L.STAGE_IMG
        ap = C.c_void_p(active.data_ptr()) if active is not None else None
        L.check(self.lib.hope_env_reset_obs(self.h, ap, stages, C.byref(self._out), self._stream()),
                'hope_env_reset_obs')
        return self

    def set_redraw_seed(self, seed):
        """seed of the draws of step(..., auto_reset=True, fresh=True)"""
        L.check(self.lib.hope_env_set_redraw_seed(self.h, C.c_uint64(int(seed) & (2 ** 64 - 1))), 'hope_env_set_redraw_seed')
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
        assert actions.shape == (self.n, 2) and actions.dtype == self.action_dtype and actions.is_contiguous()
        assert actions.device == self.device
        ap = C.c_void_p(active.data_ptr()) if active is not None else None
        L.check(self.lib.hope_env_step(self.h, C.c_void_p(actions.data_ptr()), ap, stages, C.byref(self._out),
                                       self._stream()), 'hope_env_step')
        return self

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
        if getattr(self, 'planned', None) is None:
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
        if mask is not None:
            assert mask.dtype == torch.uint8 and mask.shape == (self.n,) and mask.device == self.device and mask.is_contiguous()
        L.check(self.lib.hope_env_planner_reset(self.h, C.c_void_p(mask.data_ptr()) if mask is not None else None, self._stream()),
                'hope_env_planner_reset')
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
        word = self.rs_word if rs_word is None else rs_word
        lens = self.rs_lengths if rs_lengths is None else rs_lengths
        dn = self.done if done is True else done
        assert word.dtype == torch.int8 and word.shape == (self.n, 8) and word.device == self.device and word.is_contiguous()
        assert lens.dtype == self.obs_dtype and lens.shape == (self.n, 5) and lens.device == self.device and lens.is_contiguous()
        if dn is not None:
            assert dn.dtype == torch.uint8 and dn.shape == (self.n,) and dn.device == self.device and dn.is_contiguous()
        af64 = 0
        if actions is not None:
            assert actions.shape == (self.n, 2) and actions.dtype in (torch.float32, torch.float64) and actions.is_contiguous()
            assert actions.device == self.device
            af64 = int(actions.dtype == torch.float64)
        flags = (L.PLAN_FORCED if forced else 0) | (0 if pop else L.PLAN_NO_POP)
        if getattr(self, 'planned', None) is None:       # (the library then reports that the planner is off)
            pp = ep = None
        else:
            pp, ep = C.c_void_p(self.planned.data_ptr()), C.c_void_p(self._plan_exec.data_ptr())
        L.check(self.lib.hope_env_planner_step(self.h, C.c_void_p(word.data_ptr()), C.c_void_p(lens.data_ptr()),
                                               C.c_void_p(dn.data_ptr()) if dn is not None else None, flags, C.c_uint64(int(step or 0)),
                                               pp, ep, C.c_void_p(actions.data_ptr()) if actions is not None else None, af64,
                                               self._stream()), 'hope_env_planner_step')
        return self.planned, self.plan_executing

    def planner_state(self):
        """the planner's state block (numpy uint64 [6, N]: the five segment lengths in steps as float64 bits, the packed cursor
        word) -- host-synchronous; tests"""
        out = np.zeros((L.PLAN_STATE_WORDS, self.n), np.uint64)
        L.check(self.lib.hope_env_planner_download_state(self.h, out.ctypes.data), 'hope_env_planner_download_state')
        return out

    # -- masked choice of the discrete action on the device (hope_env.h; rule: csrc/hope_chooser_core.h) -----------------
    def enable_chooser(self):
        """ActionMask.choose_action + the agent's cast / clamp / planner override / log-probability as one kernel (k_choose).
        Uploads the 42 x 2 action table in the policy's scaling (numpy's own bits).  Off by default."""
        torch.cuda.synchronize(self.device)
        acts = np.ascontiguousarray(T.discrete_actions() / [T.VALID_STEER[1], 1.0], dtype=np.float64)
        L.check(self.lib.hope_env_chooser_enable(self.h, acts.ctypes.data), 'hope_env_chooser_enable')
        if getattr(self, 'chosen_action', None) is None:
            dev = self.device
            self.chosen_action_f32 = torch.zeros((self.n, 2), dtype=torch.float32, device=dev)
            # a float32 env steps with the very tensor the transition ring stores
            self.chosen_action = self.chosen_action_f32 if self.action_dtype == torch.float32 else torch.zeros((self.n, 2), dtype=torch.float64, device=dev)
            self.chosen_idx = torch.zeros(self.n, dtype=torch.int32, device=dev)
            self.chosen_log_prob = torch.zeros((self.n, 2), dtype=torch.float32, device=dev)
            self.chosen_probs = None                      # [N, 42] float64, allocated by the first call that asks for it
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
        mask = self.action_mask if mask is None else mask
        assert mean.dtype in (torch.float32, torch.float64) and log_std.dtype == mean.dtype
        assert mean.shape == (n, 2) and mean.device == dev and mean.is_contiguous()
        assert log_std.shape in ((n, 2), (1, 2)) and log_std.device == dev and log_std.is_contiguous()
        assert mask.dtype == self.obs_dtype and mask.shape == (n, 42) and mask.device == dev and mask.is_contiguous()
        assert (planned is None) == (executing is None), 'planned and executing go together'
        pp = ep = up = None
        if planned is not None:
            assert planned.dtype == torch.float64 and planned.shape == (n, 2) and planned.device == dev and planned.is_contiguous()
            assert executing.dtype in (torch.bool, torch.uint8) and executing.shape == (n,) and executing.device == dev and executing.is_contiguous()
            pp, ep = C.c_void_p(planned.data_ptr()), C.c_void_p(executing.data_ptr())
        if u is not None:
            assert u.dtype == torch.float64 and u.shape == (n,) and u.device == dev and u.is_contiguous()
            up = C.c_void_p(u.data_ptr())
        if getattr(self, 'chosen_action', None) is None:  # (the library then reports that the chooser is off)
            ap = fp = ip = lp = qp = None
        else:
            if probs and self.chosen_probs is None:
                self.chosen_probs = torch.zeros((n, 42), dtype=torch.float64, device=dev)
            ap, fp = C.c_void_p(self.chosen_action.data_ptr()), C.c_void_p(self.chosen_action_f32.data_ptr())
            ip, lp = C.c_void_p(self.chosen_idx.data_ptr()), C.c_void_p(self.chosen_log_prob.data_ptr())
            qp = C.c_void_p(self.chosen_probs.data_ptr()) if probs else None
        L.check(self.lib.hope_env_choose(self.h, C.c_void_p(mean.data_ptr()), C.c_void_p(log_std.data_ptr()), 2 if log_std.shape[0] == n and n > 1 else 0,
                                         int(mean.dtype == torch.float64), C.c_void_p(mask.data_ptr()), pp, ep, up,
                                         C.c_uint64(int(seed) & (2 ** 64 - 1)), C.c_uint64(int(counter) & (2 ** 64 - 1)), ap, fp, ip, lp, qp,
                                         self._stream()), 'hope_env_choose')
        out = (self.chosen_action, self.chosen_action_f32, self.chosen_idx, self.chosen_log_prob)
        return out + (self.chosen_probs,) if probs else out

    # -- normalisation of the observations on the device (hope_env.h; rule: csrc/hope_obsnorm_core.h) -------------------
    def enable_obsnorm(self):
        """StateNorm's running mean / std of lidar and target and the normalised float32 observation as three kernels
        (k_obsnorm_partial, k_obsnorm_merge, k_obsnorm_apply).  The statistics start at zero (n_state = 0); enabling again keeps
        them.  Off by default."""
        torch.cuda.synchronize(self.device)
        L.check(self.lib.hope_env_obsnorm_enable(self.h), 'hope_env_obsnorm_enable')
        if getattr(self, 'norm_lidar', None) is None:
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
        dev = self.device
        lidar = self.lidar if lidar is None else lidar
        target = self.target if target is None else target
        assert lidar.dtype in (torch.float32, torch.float64) and target.dtype == lidar.dtype
        assert lidar.dim() == 2 and target.dim() == 2 and lidar.shape[1] == L.OBSNORM_LIDAR and target.shape[1] == L.OBSNORM_TARGET
        assert lidar.shape[0] == target.shape[0]
        assert lidar.device == dev and target.device == dev and lidar.is_contiguous() and target.is_contiguous()
        rows = lidar.shape[0]
        flags = (L.OBSNORM_UPDATE if update else 0) | (L.OBSNORM_NORMALIZE if normalize else 0)
        ol = ot = None
        if normalize and getattr(self, 'norm_lidar', None) is not None:         # (without them the library reports that it is off)
            ol, ot = C.c_void_p(self.norm_lidar.data_ptr()), C.c_void_p(self.norm_target.data_ptr())
        L.check(self.lib.hope_env_obsnorm(self.h, C.c_void_p(lidar.data_ptr()), C.c_void_p(target.data_ptr()), rows,
                                          int(lidar.dtype == torch.float64), flags, ol, ot, self._stream()), 'hope_env_obsnorm')
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
        L.check(self.lib.hope_env_obsnorm_get(self.h, C.byref(n), mean.ctypes.data, S.ctypes.data, std.ctypes.data), 'hope_env_obsnorm_get')
        return int(n.value), mean, S, std

    def obsnorm_load(self, n_state, mean, S, std):
        """replace the statistics (e.g. a checkpoint's); host-synchronous"""
        a = [np.ascontiguousarray(x, dtype=np.float64) for x in (mean, S, std)]
        assert all(x.shape == (L.OBSNORM_COLS,) for x in a)
        L.check(self.lib.hope_env_obsnorm_set(self.h, int(n_state), a[0].ctypes.data, a[1].ctypes.data, a[2].ctypes.data), 'hope_env_obsnorm_set')
        return self

    # -- PPO's advantage block on the device (hope_env.h; rule: csrc/hope_gae_core.h) -----------------------------------
    def enable_gae(self):
        """GAE along T, the critic's target and the advantages' normalisation as three kernels (k_gae_scan, k_gae_merge,
        k_adv_apply) over [rows, T] float32 tensors.  Off by default."""
        torch.cuda.synchronize(self.device)
        L.check(self.lib.hope_env_gae_enable(self.h), 'hope_env_gae_enable')
        if getattr(self, 'gae_sums', None) is None:
            self.gae_sums = torch.zeros(3, dtype=torch.float64, device=self.device)
            self._gae_out = None                                   # (adv, v_target): [N, T], allocated at the first call for its T
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
        assert reward.dim() == 2 and v_last.dim() == 1
        rows, t = reward.shape
        for x in (reward, done, value, value_target):
            assert x.shape == (rows, t)
        assert v_last.shape == (rows,)
        for x in (reward, done, value, v_last, value_target):
            assert x.dtype == torch.float32 and x.device == dev and x.is_contiguous()
        sums = getattr(self, 'gae_sums', None) if sums is None else sums
        if sums is not None:
            assert sums.dtype == torch.float64 and sums.shape == (3,) and sums.device == dev and sums.is_contiguous()
        out = getattr(self, '_gae_out', None)
        if out is None or out[0].shape[1] != t:                    # (before enable_gae the library reports that it is off)
            out = self._gae_out = tuple(torch.zeros((max(self.n, rows), t), dtype=torch.float32, device=dev) for _ in range(2))
        P = lambda x: None if x is None else C.c_void_p(x.data_ptr())  # noqa: E731
        flags = 0 if normalize is None else (L.GAE_SUMS | (L.GAE_NORMALIZE if normalize else 0))
        L.check(self.lib.hope_env_gae(self.h, P(reward), P(done), P(value), P(v_last), P(value_target), rows, t, float(gamma), float(lam), flags,
                                      P(out[0]), P(out[1]), P(sums), self._stream()), 'hope_env_gae')
        return out[0][:rows], out[1][:rows], sums

    def adv_normalize(self, adv, sums, out=None):
        """out = (adv - mean) / (std + 1e-5) from sums = {sum, sum of squares, count} (float64 [3] on the device, e.g. all-reduced);
        out=None: in place.  One launch on the current stream."""
        out = adv if out is None else out
        assert adv.dtype == torch.float32 and adv.is_contiguous() and adv.device == self.device
        assert out.dtype == torch.float32 and out.is_contiguous() and out.device == self.device and out.shape == adv.shape
        assert sums.dtype == torch.float64 and sums.shape == (3,) and sums.device == self.device and sums.is_contiguous()
        L.check(self.lib.hope_env_adv_normalize(self.h, C.c_void_p(adv.data_ptr()), adv.numel(), C.c_void_p(sums.data_ptr()),
                                                C.c_void_p(out.data_ptr()), self._stream()), 'hope_env_adv_normalize')
        return out

    # -- bookkeeping of an evaluation run on the device (hope_env.h; rule: csrc/hope_evaltrack_core.h) ------------------
    def enable_eval_tracker(self):
        """eval()'s per-episode tally (eval_utils.py:35-57) as device state of the handle (80 B per scene) and three kernels:
        k_eval_begin, k_eval_override, k_eval_track.  The stuck detector draws from the physical action box (tables.VALID_STEER /
        VALID_SPEED).  Enabling again keeps the state.  Off by default."""
        torch.cuda.synchronize(self.device)
        box = np.array([T.VALID_STEER[0], T.VALID_STEER[1], T.VALID_SPEED[0], T.VALID_SPEED[1]], dtype=np.float64)
        L.check(self.lib.hope_env_eval_enable(self.h, box.ctypes.data), 'hope_env_eval_enable')
        if getattr(self, 'eval_alive', None) is None:
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

    def _eval_obs(self, t, shape, dtype):
        assert t.dtype == dtype and tuple(t.shape) == shape and t.device == self.device and t.is_contiguous()
        return C.c_void_p(t.data_ptr())

    def eval_begin(self, target=None, pose=None):
        """a new episode in every scene, from the first observation (None: the env's own target / pose); one k_eval_begin launch on
        the current stream, no host synchronisation"""
        n = self.n
        tp = self._eval_obs(self.target if target is None else target, (n, 5), self.obs_dtype)
        pp = self._eval_obs(self.pose if pose is None else pose, (n, 3), torch.float64)
        L.check(self.lib.hope_env_eval_begin(self.h, tp, pp, self._stream()), 'hope_env_eval_begin')
        return self

    def eval_override(self, actions, u=None, seed=0, counter=0):
        """the stuck detector's random action, in place: the rows of `actions` ([N, 2] float32 or float64, contiguous) of the scenes
        whose target did not change in the last step are replaced by the clipped draw from the physical action box.  u f64 [N, 2] in
        [0, 1) or None: counter-based draws keyed by (seed, counter, scene, dimension).  One k_eval_override launch, no host
        synchronisation.  -> eval_alive (uint8 [N], persistent): the scenes whose episode is still running -- step()'s `active`."""
        n, dev = self.n, self.device
        assert actions.shape == (n, 2) and actions.dtype in (torch.float32, torch.float64) and actions.is_contiguous() and actions.device == dev
        up = None
        if u is not None:
            assert u.dtype == torch.float64 and u.shape == (n, 2) and u.device == dev and u.is_contiguous()
            up = C.c_void_p(u.data_ptr())
        al = getattr(self, 'eval_alive', None)               # (without it the library reports that the tracker is off)
        L.check(self.lib.hope_env_eval_override(self.h, C.c_void_p(actions.data_ptr()), int(actions.dtype == torch.float64), up,
                                                C.c_uint64(int(seed) & (2 ** 64 - 1)), C.c_uint64(int(counter) & (2 ** 64 - 1)),
                                                C.c_void_p(al.data_ptr()) if al is not None else None, self._stream()), 'hope_env_eval_override')
        return al

    def eval_track(self, target=None, pose=None, reward=None, status=None, done=None, rs_word=None):
        """the tally of the step just taken (None: the env's own outputs); one k_eval_track launch on the current stream, no host
        synchronisation, no wait for a deferred search.  -> (eval_word int8 [N, 8]: rs_word with the found flag cleared for frozen
        scenes, eval_done uint8 [N]: episodes that ended in this step): persistent tensors, overwritten by the next call."""
        n = self.n
        ptrs = [self._eval_obs(self.target if target is None else target, (n, 5), self.obs_dtype),
                self._eval_obs(self.pose if pose is None else pose, (n, 3), torch.float64),
                self._eval_obs(self.reward if reward is None else reward, (n,), self.obs_dtype),
                self._eval_obs(self.status if status is None else status, (n,), torch.int32),
                self._eval_obs(self.done if done is None else done, (n,), torch.uint8),
                self._eval_obs(self.rs_word if rs_word is None else rs_word, (n, 8), torch.int8)]
        if getattr(self, 'eval_word', None) is None:         # (the library then reports that the tracker is off)
            wp = dp = None
        else:
            wp, dp = C.c_void_p(self.eval_word.data_ptr()), C.c_void_p(self.eval_done.data_ptr())
        L.check(self.lib.hope_env_eval_track(self.h, *ptrs, wp, dp, self._stream()), 'hope_env_eval_track')
        return getattr(self, 'eval_word', None), getattr(self, 'eval_done', None)

    def eval_records(self):
        """-> float32 [N, 4]: status, steps, summed reward, path length of every scene's episode so far (a persistent tensor,
        overwritten by the next call); one launch, no host synchronisation"""
        rec = getattr(self, '_eval_rec', None)
        L.check(self.lib.hope_env_eval_records(self.h, C.c_void_p(rec.data_ptr()) if rec is not None else None, self._stream()),
                'hope_env_eval_records')
        return rec

    def eval_state(self):
        """the tracker's state block (numpy uint64 [10, N]: previous target, previous position, summed reward, path length as
        float64 bits, the packed steps / status / alive / stuck word) -- host-synchronous; tests"""
        out = np.zeros((L.EVAL_STATE_WORDS, self.n), np.uint64)
        L.check(self.lib.hope_env_eval_download_state(self.h, out.ctypes.data), 'hope_env_eval_download_state')
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
        L.check(self.lib.hope_env_download_n_obst(self.h, out.ctypes.data), 'hope_env_download_n_obst')
        return out

    def map_levels(self, active=None, out=None, detail=False):
        """`map.map_level` of the maps the scenes hold NOW (pool draws, Dragon-Lake draws and uploads alike), labelled on the device
        by k_map_level (asynchronous on the current stream) -> torch.uint8 [N], 0 Normal / 1 Complex / 2 Extrem
        (hope_amd.map_level.LEVEL_NAMES) [, int32 [N, 8] detail].  active: u8 [N]; scenes with active[i] == 0 keep out[i] (pass the
        last step's `done` and the previous labels as `out` to relabel only the scenes that drew a new map)."""
        if out is None:
            out = torch.zeros(self.n, dtype=torch.uint8, device=self.device)
        assert out.dtype == torch.uint8 and out.shape == (self.n,) and out.device == self.device and out.is_contiguous()
        ap = None
        if active is not None:
            assert active.dtype == torch.uint8 and active.shape == (self.n,) and active.device == self.device and active.is_contiguous()
            ap = C.c_void_p(active.data_ptr())
        det = None
        if detail is not False and detail is not None:
            det = detail if torch.is_tensor(detail) else torch.zeros((self.n, 8), dtype=torch.int32, device=self.device)
            assert det.dtype == torch.int32 and det.shape == (self.n, 8) and det.device == self.device and det.is_contiguous()
        L.check(self.lib.hope_env_map_level(self.h, ap, C.c_void_p(out.data_ptr()), C.c_void_p(det.data_ptr()) if det is not None else None,
                                            self._stream()), 'hope_env_map_level')
        return (out, det) if det is not None else out

    def restart(self, mask):
        """episodes flagged in mask (u8 [N]) go back to their start pose, t = 0 (same map)."""
        assert mask.dtype == torch.uint8 and mask.shape == (self.n,) and mask.device == self.device
        L.check(self.lib.hope_env_restart(self.h, C.c_void_p(mask.data_ptr()), self._stream()), 'hope_env_restart')
        return self

    def kernel_ms(self, reset=True):
        """{kernel name: (accumulated ms, launches)} from the library's per-launch HIP events (profile=True)."""
        ms = np.zeros(len(L.KERNELS))
        cnt = np.zeros(len(L.KERNELS), np.int64)
        L.check(self.lib.hope_env_kernel_ms(self.h, ms.ctypes.data, cnt.ctypes.data, int(reset)), 'hope_env_kernel_ms')
        return {k: (float(ms[i]), int(cnt[i])) for i, k in enumerate(L.KERNELS)}

    def kernel_union_ms(self, reset=True):
        """{kernel name: (accumulated ms during which >= 1 launch of the kernel ran, calls)}: per step call the UNION of the
        kernel's launch intervals (the two tile classes overlap on two streams).  Read it before kernel_ms(reset=True)."""
        ms = np.zeros(len(L.KERNELS))
        cnt = np.zeros(len(L.KERNELS), np.int64)
        L.check(self.lib.hope_env_kernel_union_ms(self.h, ms.ctypes.data, cnt.ctypes.data, int(reset)), 'hope_env_kernel_union_ms')
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
        L.check(self.lib.hope_env_download_state(self.h, pose.ctypes.data, t.ctypes.data, acc.ctypes.data),
                'hope_env_download_state')
        return pose, t, acc

    def upload_state(self, pose=None, t=None, accum=None):
        p = np.ascontiguousarray(pose, dtype=np.float64) if pose is not None else None
        tt = np.ascontiguousarray(t, dtype=np.int32) if t is not None else None
        a = np.ascontiguousarray(accum, dtype=np.float64) if accum is not None else None
        L.check(self.lib.hope_env_upload_state(self.h, p.ctypes.data if p is not None else None,
                                               tt.ctypes.data if tt is not None else None,
                                               a.ctypes.data if a is not None else None), 'hope_env_upload_state')

    def close(self):
        if getattr(self, 'h', None):
            self.lib.hope_env_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
