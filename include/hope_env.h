/*
 * hope_env.h -- C ABI of libhope_env.so, the MI355X-native batched parking simulator for HOPE.
 *
 * The reference (jiamiya/HOPE) has NO FFI / plugin layer: its boundary is the Python class surface
 * `CarParking` (src/env/car_parking_base.py:39) wrapped by `CarParkingWrapper`
 * (src/env/env_wrapper.py:58).  This header is therefore the interface a maintainer would bind
 * with ctypes from a `CarParking` look-alike (INTEGRATION.md shows the stub); each entry point
 * names the reference method(s) whose work it replaces.
 *
 * Conventions
 *   - plain C, no HIP/torch types: device buffers are `void*` device addresses (e.g.
 *     tensor.data_ptr()), streams are the raw hipStream_t passed as `void*` (NULL = default stream);
 *   - every call returns 0 on success or a negative HOPE_E* code; hope_last_error() gives the text.
 *     Nothing throws across the ABI;
 *   - one handle per GPU process; a handle is not thread-safe, distinct handles are independent;
 *   - the library owns the tables, the per-scene obstacle tiles and the per-scene episode state
 *     (pose, t, accum_arrive_reward); the caller owns every observation/reward buffer;
 *   - all launches are asynchronous on the caller's stream; no hidden synchronisation except in
 *     functions documented as host-synchronous (create/destroy/upload/set_scenes/download).
 *   - the library fails loudly when no HIP device is usable: there is NO CPU fallback.
 *
 * Obstacle tile: every obstacle is a ring of 3 or 4 vertices stored in a fixed 4-vertex slot
 * (64 B, float64 x,y pairs); a triangle repeats its last vertex in slot 3.  The reference's scenes
 * (data/dlp.data, parking_map_normal.py) contain only 3- and 4-vertex rings.
 */
#ifndef HOPE_ENV_H
#define HOPE_ENV_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HOPE_ABI_VERSION 8

#define HOPE_LIDAR_NUM 120   /* configs.py:96  */
#define HOPE_N_ACTION 42     /* configs.py:108-115 */
#define HOPE_N_ITER 10       /* action_mask.py:9 n_iter */
#define HOPE_UPSAMPLE 10     /* action_mask.py:18 */
#define HOPE_TARGET_DIM 5    /* car_parking_base.py:72 */
#define HOPE_RS_MAX_SEG 5    /* longest Reeds-Shepp word (CCSCC) */
#define HOPE_IMG_SIZE 64      /* OBS_W // downsample_rate (configs.py:88, observation_processor.py:8) */
#define HOPE_IMG_CHANNELS 3
#define HOPE_TRAJ_RENDER_LEN 20 /* configs.py:86 */

/* error codes */
#define HOPE_OK 0
#define HOPE_EINVAL (-1)     /* bad argument                       */
#define HOPE_ENODEV (-2)     /* no usable HIP device               */
#define HOPE_ENOMEM (-3)     /* device/host allocation failed      */
#define HOPE_EHIP (-4)       /* a HIP runtime call failed          */
#define HOPE_ESTATE (-5)     /* call order violated (e.g. step before tables/scenes) */

/* vehicle.py:13-18 Status */
#define HOPE_STATUS_CONTINUE 1
#define HOPE_STATUS_ARRIVED 2
#define HOPE_STATUS_COLLIDED 3
#define HOPE_STATUS_OUTBOUND 4
#define HOPE_STATUS_OUTTIME 5

/* Reeds-Shepp segment types in rs_word[] */
#define HOPE_RS_NONE (-1)
#define HOPE_RS_S 0
#define HOPE_RS_L 1
#define HOPE_RS_R 2

/* hope_env_create flags */
#define HOPE_F_OBS_F64 0x1      /* observation/reward buffers are float64 (parity mode); default float32 */
#define HOPE_F_ACTION_F64 0x2   /* action buffer is float64; default float32 */
#define HOPE_F_PROFILE 0x4      /* record HIP events around every kernel launch (hope_env_kernel_ms) */
#define HOPE_F_IMAGE 0x8        /* keep vehicle.trajectory (last 20 poses/scene) so that HOPE_STAGE_IMG can be used */
#define HOPE_F_OVERLAP 0x10     /* launch the two obstacle-tile classes of a step on two streams (fork / join with events),
                                   and from 16 k scenes on the observation half of the step kernel on further streams
                                   next to the Reeds-Shepp kernels: one chain alone leaves issue slots idle */
/* 0x20 was HOPE_F_GRAPH (hipGraph replay of a step's launches, ABI <= 6).  Removed in ABI 7: measured slower than plain asynchronous
 * launches at every batch size (4 096 scenes 0.269 vs 0.237 ms, 8 192 0.293 vs 0.263, 16 384 0.511 vs 0.352; profiles/r04_bench_modes.txt
 * of the commit before the removal) -- the launches are not host-bound, and the runtime runs a captured multi-stream graph on fewer
 * queues than the streams it was captured from.  hope_env_create rejects the bit. */

/* Environment variables read by the library (tuning / diagnostics only; results never depend on them):
 *   HOPE_SPLIT_MIN   scenes per handle from which HOPE_F_OVERLAP launches k_env_step as a motion and an observation launch
 *   HOPE_AUTO_CHAINS lo0:hi0:lo1:hi1 -- scene-count ranges in which a one-class batch is stepped as two sub-chains of that class
 *   HOPE_RS_EXACT    validate Reeds-Shepp words with the all-float64 kernel (the reference of the default kernel's float32 filter)
 *   HOPE_RS_SPLIT    1: the two-kernel Reeds-Shepp validation (k_rs_screen, then the walk; measured and not adopted)
 *   HOPE_RS_DEBUG    Reeds-Shepp profiling and self-check switches (hope_rs.hip)
 *   HOPE_STEP_TIMING cycle-accounting build of the step kernel (tools/step_timing.py)
 *   HOPE_RS_TIMING   cycle-accounting build of the validation kernel (tools/rs_timing.py)
 *   HOPE_BEV_LEGACY  image: the per-tile raster of the moving boxes instead of the trajectory layer
 *   HOPE_BEV_DEBUG   image: profiling switches of the image kernels (hope_bev.hip)
 *   HOPE_CLS1_FRAC   share of the scenes the large-tile launch chain holds after the small-tile class hands scenes over
 *   HOPE_HOST_THREADS  CPU threads of the scene generator (hope_scenegen_generate)
 * Defaults and the measurements behind them: hope_amd/csrc/hope_env.hip (plan_step). */

/* hope_env_step stage mask */
#define HOPE_STAGE_MOTION 0x1   /* kinematics + arrival + collision sub-step loop (CarParking.step :255-277) */
#define HOPE_STAGE_OBS 0x2      /* lidar + action mask + target (CarParking.render :399-407)               */
#define HOPE_STAGE_REWARD 0x4   /* status + reward (:279-289) + wrapper reward_shaping                     */
#define HOPE_STAGE_RS 0x8       /* Reeds-Shepp feasibility search (:293-297, find_rs_path :413)           */
#define HOPE_STAGE_ALL 0xF
/* Bits 0x1000, 0x2000, 0x4000 and 0x8000 are reserved for the library's internal test and profiling switches. */
/* bird's-eye image observation obs['img'] (_render :301-320, _get_img_observation :322-350, Obs_Processor
 * observation_processor.py:11-23, transpose env_wrapper.py:53-54).  Not part of HOPE_STAGE_ALL (the reference's
 * USE_IMG switch, configs.py:100); needs a handle created with HOPE_F_IMAGE and out->img. */
#define HOPE_STAGE_IMG 0x40
/* modifier bit: actions are already physical (steer [rad], speed [m/s]) as CarParking.step receives them
 * (car_parking_base.py:235); without it they are the wrapper's [-1,1] actions and action_rescale
 * (env_wrapper.py:37-50) is applied first.  KSModel's own clip (vehicle.py:85-86) always applies. */
#define HOPE_ACTION_PHYSICAL 0x10
/* modifier bit: with a float32 action buffer, action_rescale is evaluated in float32 -- what the reference's
 * action_rescale (env_wrapper.py:37-50) does when the agent hands it a float32 array: gym's Box bounds are float32, so
 * clip, scale and shift all round to float32 before CarParking.step sees the action.  Everything after the rescale
 * (KSModel.step) is float64 as without the bit.  No effect with a float64 buffer or with HOPE_ACTION_PHYSICAL. */
#define HOPE_ACTION_RESCALE_F32 0x80
/* modifier bit: fused episode turnover (gym VectorEnv "autoreset").  A scene whose step ends with status !=
 * CONTINUE is reset in the same kernel exactly as CarParking.reset (:127-138) does on the same map: pose = start,
 * accum_arrive_reward = 0, t = 0 and the action-less step (t = 1, incl. its _get_reward bookkeeping).  reward /
 * reward_info / status / done / RS outputs are those of the FINISHED step; lidar / action_mask / target / pose are
 * the new episode's first observation.  Equivalent to hope_env_step + hope_env_restart(done) +
 * hope_env_reset_obs(active = done) without the extra launches. */
#define HOPE_AUTO_RESET 0x20
/* modifier bit, with HOPE_AUTO_RESET: the finished scene continues on a NEW map, as CarParking.reset does
 * (map.reset, car_parking_base.py:134): a pool entry of its obstacle-tile class (hope_env_set_pool), chosen exactly as
 * hope_env_redraw chooses it -- by a counter-based hash of (the seed of hope_env_set_redraw_seed, scene, episodes drawn
 * so far) -- is copied into the scene inside the step kernel.  Equivalent to hope_env_step + hope_env_redraw(done, seed) +
 * hope_env_reset_obs(active = done) without the extra launches.  HOPE_ESTATE without a pool. */
#define HOPE_AUTO_REDRAW 0x100
/* modifier bit: TWO completion points per step.  Without it `stream` is ordered after every output of the step when
 * hope_env_step returns.  With it `stream` is ordered after the observation half only -- lidar / action_mask / target / img,
 * reward / reward_info / status / done / pose -- so that the caller's policy forward (which reads the observation,
 * parking_agent.py:78-99) runs while the Reeds-Shepp kernels of the step finish on the library's own streams; rs_word /
 * rs_lengths are ordered by hope_env_wait_rs(h, stream) (the planner override just before the next step).  A caller that does
 * not read them enqueues the next hope_env_step without waiting: the search of step k then runs on the library's search streams
 * NEXT TO the kinematics / motion / observation launches of step k + 1 (consecutive steps pipeline; ABI 7), and its rs_word /
 * rs_lengths are replaced by step k + 1's -- they can only be read after a hope_env_wait_rs issued BEFORE the next step.  The outputs are the same bits either way.  The bit takes effect on handles with HOPE_F_OVERLAP whose scenes
 * span both obstacle-tile classes, at every batch size (the one-launch form of the step kernel below 32 768 scenes, the two-launch
 * form from there on); elsewhere the step is joined as without it and hope_env_wait_rs is a no-op.  Every other entry point that reads or writes the handle's state joins first by itself.
 * Lifetime of the inputs: `actions` and `active` are only read by launches `stream` is ordered after when hope_env_step returns
 * (the Reeds-Shepp chain reads a snapshot of `active` that the motion launch takes into a buffer of the handle), so the caller
 * may free or overwrite both right after the call, in stream order, as without the bit. */
#define HOPE_DEFER_RS 0x200

typedef struct hope_env hope_env_t;

/* Caller-owned DEVICE buffers filled by hope_env_step / hope_env_reset_obs.  Any pointer may be NULL
 * (that output is skipped).  "real" = float32, or float64 when the handle has HOPE_F_OBS_F64. */
typedef struct hope_step_out {
    void *lidar;        /* real [N][120]  obs['lidar']  (range minus hull range; may be slightly < 0) */
    void *action_mask;  /* real [N][42]   obs['action_mask'] in {0,.1,..,1} or all .01               */
    void *target;       /* real [N][5]    obs['target']                                               */
    void *reward;       /* real [N]       wrapper reward (env_wrapper.py:10-35)                       */
    void *reward_info;  /* real [N][5]    time_cost, rs_dist, dist, angle, box_union                  */
    int32_t *status;    /* i32  [N]       HOPE_STATUS_*                                               */
    uint8_t *done;      /* u8   [N]       status != CONTINUE                                          */
    double *pose;       /* f64  [N][3]    x, y, heading after the step (always float64)               */
    int8_t *rs_word;    /* i8   [N][8]    [0..4] segment types (HOPE_RS_*), [5] n_seg, [6] found, [7] 0 */
    void *rs_lengths;   /* real [N][5]    signed segment lengths in metres (PATH.lengths)             */
    uint8_t *img;       /* u8   [N][3][64][64]  obs['img'] * 255 (channel-first as the wrapper returns it); the
                           reference's float image is this / 255.0                                    */
} hope_step_out;

/* ---- lifetime ------------------------------------------------------------------------------ */
/* Replaces CarParking.__init__ (car_parking_base.py:48-115) for n_scenes parallel environments.
 * max_obstacles bounds the obstacle count of any scene (LDS tile = 64 B x max_obstacles per wave).  It is limited to
 * HOPE_MAX_OBSTACLES: the Reeds-Shepp queue entry carries a scene's obstacle count in 8 bits (the LDS formulas alone would admit
 * over a thousand; the reference's largest map, a Dragon-Lake case after its +-20 m cull, holds 125).  A larger value -- or one
 * whose tile does not fit the 160 KiB LDS of a CU, or n_scenes >= 2^24 -- fails with HOPE_EINVAL and a message naming the limit. */
#define HOPE_MAX_OBSTACLES 255
int hope_env_create(hope_env_t **out, int n_scenes, int max_obstacles, int device_id, uint32_t flags);
int hope_env_destroy(hope_env_t *h);                       /* CarParking.close (:536) */
/* Every entry point that takes a handle fails with HOPE_EINVAL and "<name>: not a live handle (destroyed?)" when given a pointer
 * that hope_env_create did not return or that hope_env_destroy has released, before it reads anything through the pointer. */
const char *hope_last_error(void);
int hope_abi_version(void);

/* ---- tables: ActionMask.__init__ / LidarSimlator.__init__ products (host pointers, host-sync) -- */
/* dist_star  [1200][42][10] float64, reference order (action_mask.py:114-143 `precompute`);
 * hull_base  [120]  range from the rear axle to the hull per beam (lidar_simulator.py:48-53);
 * beam_ab    [120][2]  (sin theta_i, -cos theta_i) of lidar_simulator.py:86-88.
 * The library derives its device tables from them on the host: dist_star prefix-maxed over k and transposed, its per-beam maximum,
 * and (round 6) the count-interval table of the mask stage -- per coarse beam 128 scan-value bins, per bin and action the interval that
 * brackets ActionMask.get_steps' first-exceed count (action_mask.py:166-177) for every scan value of the bin (hope_debug_mask_lut).
 * The mask stage finds a beam's bin as (int)((scan - (hull_base - 1e-6)) * 128 / (max of dist_star at the beam + 4e-9 - (hull_base - 1e-6))),
 * so tables it could not index are refused: HOPE_EINVAL if a dist_star or hull_base value is not finite, or if at one of the 120 coarse
 * beams (rows 0, 10, 20, ...) the maximum of dist_star over actions and increments does not lie above hull_base - 1e-6;
 * hope_last_error() names the beam.  The tables are validated before the first copy: a refused call leaves the handle's tables, and
 * whether it has any, as they were. */
int hope_env_upload_tables(hope_env_t *h, const double *dist_star, const double *hull_base,
                           const double *beam_ab);

/* ---- scenes: map.reset + vehicle.reset (car_parking_base.py:127-137), host pointers, host-sync -- */
/* For k in [0,n): scene scene_ids[k] gets start[k][3], dest[k][3] (x,y,heading), bbox[k][4]
 * (xmin,xmax,ymin,ymax; parking_map_dlp.py:70-73 / parking_map_normal.py:486-489), n_obst[k]
 * obstacles whose vertices are verts[k][max_obstacles][4][2].  Episode state is reset: pose=start,
 * t=0, accum_arrive_reward=0.  The caller then runs hope_env_reset_obs (reset's `self.step()`). */
int hope_env_set_scenes(hope_env_t *h, const int32_t *scene_ids, int n, const double *start,
                        const double *dest, const double *bbox, const double *verts,
                        const int32_t *n_obst);

/* ---- the hot path (asynchronous on `stream`) ------------------------------------------------- */
/* CarParkingWrapper.step(action) (env_wrapper.py:73-81) for all scenes:
 * actions = DEVICE [N][2] (steer, speed) in [-1,1] (float32, or float64 with HOPE_F_ACTION_F64).
 * active  = optional DEVICE u8 [N]; scenes with active[i]==0 are left untouched (outputs too). */
int hope_env_step(hope_env_t *h, const void *actions, const uint8_t *active, uint32_t stages,
                  const hope_step_out *out, void *stream);

/* Orders `stream` after the Reeds-Shepp outputs of the LAST hope_env_step that carried HOPE_DEFER_RS (no-op if none is
 * outstanding).  "Last" is literal: since ABI 7 consecutive deferred steps pipeline, and step k + 1 REPLACES step k's rs_word /
 * rs_lengths instead of ordering them -- a hope_env_wait_rs issued after step k + 1 was enqueued joins step k + 1's search. */
int hope_env_wait_rs(hope_env_t *h, void *stream);
/* (ABI 8) The same wait with the caller saying WHICH step's search it means: hope_env_last_step returns the sequence number of
 * the most recent hope_env_step / hope_env_reset_obs call of the handle (1, 2, ...); hope_env_wait_rs_step(h, step, stream)
 * orders `stream` after that step's Reeds-Shepp outputs and fails with HOPE_ESTATE -- touching nothing -- when a newer step has
 * been enqueued since (its outputs have been, or are being, replaced).  What a planner-in-the-loop caller should use: an
 * accidental "step, step, wait" then fails loudly instead of handing it the other step's (or a mix of both steps') words. */
int hope_env_last_step(hope_env_t *h, uint64_t *step);
int hope_env_wait_rs_step(hope_env_t *h, uint64_t step, void *stream);

/* The action-less step of CarParking.reset (:138) / CarParkingWrapper.step(None) (:74-75):
 * t += 1, observation, status, reward; no motion. */
int hope_env_reset_obs(hope_env_t *h, const uint8_t *active, uint32_t stages, const hope_step_out *out,
                       void *stream);

/* vehicle.reset(initial_state) + accumulator reset of CarParking.reset (:128-136) WITHOUT a new map:
 * scenes with mask[i] != 0 go back to pose = start, t = 0, accum_arrive_reward = 0 (asynchronous).
 * Follow with hope_env_reset_obs(active = mask) to obtain the first observation. */
int hope_env_restart(hope_env_t *h, const uint8_t *mask, void *stream);

/* ---- scene pool: a new map at episode turnover without the host in the loop -------------------------------------- */
/* The reference draws a new case for EVERY episode (ParkingMapNormal.reset parking_map_normal.py:474-494, ParkingMapDLP.reset
 * parking_map_dlp.py:38-86, called from CarParking.reset car_parking_base.py:134).  hope_env_set_pool uploads n_pool complete
 * scenes (host pointers, layout as hope_env_set_scenes, host-synchronous) into device memory owned by the handle;
 * hope_env_redraw (asynchronous on `stream`) gives every scene with mask[i] != 0 a pool entry of ITS obstacle-tile class
 * (n_obst <= 32 or larger: the dense per-class launch lists stay valid), chosen by a counter-based hash of
 * (seed, scene, episodes drawn so far), and restarts it (pose = start, t = 0, accum_arrive_reward = 0).  Follow with
 * hope_env_reset_obs(active = mask) for the first observation.  The host refills / replaces the pool whenever it likes.
 * The size-class mix of the resident scenes therefore stays what hope_env_set_scenes made it (a slot that holds a <= 32-obstacle
 * lot keeps drawing such lots); a resident class without pool entries is an error (HOPE_ESTATE), not a silent restart. */
int hope_env_set_pool(hope_env_t *h, int n_pool, const double *start, const double *dest, const double *bbox,
                      const double *verts, const int32_t *n_obst);
/* The same without blocking the step loop: hope_env_pool_staging hands out PINNED host arrays of the handle (layout as above, for
 * n_pool entries; valid until the next hope_env_pool_staging call) that any host thread may fill -- e.g. hope_scenegen_generate
 * writing into them directly -- and hope_env_commit_pool uploads them asynchronously into the pool set the kernels are not reading
 * and swaps the sets: launches enqueued afterwards wait (on the device, in stream order) for the upload and draw from the new pool;
 * launches already enqueued keep the old one.  Neither call synchronises with the step kernels (hope_env_pool_staging waits at most
 * for the previous upload's copy to leave the staging).  Both must be called from the thread that owns the handle. */
int hope_env_pool_staging(hope_env_t *h, int n_pool, double **start, double **dest, double **bbox, double **verts, int32_t **n_obst);
int hope_env_commit_pool(hope_env_t *h, int n_pool, void *stream);
/* (ABI 8) The same upload, with the swap RELAXED: the new pool takes over at the first step (or hope_env_redraw) enqueued after the
 * upload has COMPLETED -- no step ever waits for an upload.  (hope_env_commit_pool swaps at once, so the next step's launch waits on
 * its stream for the 67 MB of an 8 192-lot pool: 2-3 ms, five 65 536-scene steps.)  Which step that is depends on timing, like the
 * moment a background refresher's fill finishes; a later commit of either kind, hope_env_set_pool and hope_env_pool_generation first
 * wait for and apply a swap still pending.  What a rollout's background refresher should use (hope_amd.scene_gen.PoolRefresher).
 * With the curriculum on (below) the step that applies the swap is not wait-free: it enqueues the incoming set's labels and weighted
 * lists on the pool stream and waits for them in stream order (~0.15 ms for 252 buckets), so that no draw falls back to uniform. */
int hope_env_commit_pool_relaxed(hope_env_t *h, int n_pool);
/* 1 when hope_env_pool_staging would return without waiting (the previous commit's copies have left the pinned arrays), 0 when not
 * yet, < 0 on error: a background refresher polls this instead of blocking the thread that drives the step loop */
int hope_env_pool_staging_ready(hope_env_t *h);
/* An identity of the set of maps a draw can return: changes whenever that set changes (hope_env_set_pool / hope_env_commit_pool /
 * hope_env_set_dlp_cases).  Part of a snapshot of drawn maps: hope_env_restore_maps refuses a snapshot of another generation.
 * ABI 8: the value is a HASH CHAIN over the contents of every upload since hope_env_create (pool entries' start / dest / box /
 * obstacle counts and a strided sample of their vertices; the Dragon-Lake case table), not a per-handle counter -- a snapshot taken
 * in one process is refused by another process whose pool holds other maps even if both uploaded "one pool".  0 is never
 * returned for a handle with a pool (0 = "no pool yet" / "skip the check" in hope_env_restore_maps).
 * With the curriculum on the value also folds in what the applied weighted lists are made of (groups and positions): the call then
 * synchronises with the handle's pool stream and downloads ~2 KB. */
int hope_env_pool_generation(hope_env_t *h, uint64_t *generation);
/* seed of HOPE_AUTO_REDRAW's draws (default 0) */
int hope_env_set_redraw_seed(hope_env_t *h, uint64_t seed);
int hope_env_redraw(hope_env_t *h, const uint8_t *mask, uint64_t seed, void *stream);
/* pool entry each scene currently holds: >= 0 a complete pool scene, -1 the map hope_env_set_scenes uploaded;
 * values <= -2 name Dragon-Lake-Parking case c = -2 - value drawn on the device (hope_env_set_dlp_cases); host-synchronous */
int hope_env_download_pool_index(hope_env_t *h, int32_t *out /*[N]*/);

/* Dragon-Lake-Parking cases drawn ON THE DEVICE at episode turnover (ParkingMapDLP.reset, src/env/parking_map_dlp.py:38-86): per
 * episode a start candidate of the case chosen uniformly (:58-59) with N(0, 0.05^2) m / N(0, 0.02^2) rad jitter (:60-65), the map
 * box floor / ceil(min / max(start, dest) -/+ 20 m) (:70-73), the case's obstacles culled by that box (:88-101), independent 50 %
 * flips of dest and start about their box centres (:80-83).  The data of data/dlp.data (host pointers, host-synchronous):
 * dest [n_cases][3]; cand_off [n_cases + 1] + cand [][3]: the start candidates of each case; case_set [n_cases]: the obstacle set
 * a case uses; set_off [n_sets + 1] + set_verts [][4][2]: the rings of each set (a triangle repeats its last vertex).  The cases
 * join the draw list of the large-tile class (every culled lot has 37 .. 125 obstacles): hope_env_redraw / HOPE_AUTO_REDRAW pick
 * uniformly among that class's complete pool scenes and the cases.  n_cases = 0 removes them. */
int hope_env_set_dlp_cases(hope_env_t *h, int n_cases, const double *dest, const int32_t *cand_off, const double *cand,
                           const int32_t *case_set, int n_sets, const int32_t *set_off, const double *set_verts);
/* The size class of scene slots: 0 = lots of at most 32 obstacles (small LDS tile, draws from the pool's small maps), 1 = larger
 * lots (draws from the large maps and the Dragon-Lake cases).  hope_env_set_scenes sets it from the uploaded map's obstacle count;
 * this call overrides it, e.g. to keep a slot among the Dragon-Lake lots although its first map kept only 30 obstacles (class 1 is
 * always allowed, class 0 only for maps of <= 32 obstacles).  cls: host u8 [n].  Host-synchronous. */
int hope_env_set_draw_class(hope_env_t *h, const int32_t *scene_ids, int n, const uint8_t *cls);
/* draws whose culled obstacle set did not fit max_obstacles and was truncated (must stay 0); host-synchronous */
int hope_env_pool_overflow(hope_env_t *h, int32_t *count);
/* the maps the listed scenes hold NOW (after device-side draws they exist on the device only); any output may be NULL; layout as
 * hope_env_set_scenes; host-synchronous */
int hope_env_download_scenes(hope_env_t *h, const int32_t *scene_ids, int n, double *start, double *dest, double *bbox, double *verts,
                             int32_t *n_obst);
/* (ABI 8) the obstacle count of EVERY scene as it is now (device-side draws change it behind the host): one copy; host-synchronous */
int hope_env_download_n_obst(hope_env_t *h, int32_t *n_obst /*[N]*/);
/* Snapshot / restore of drawn maps.  A draw is a pure function of (seed, scene, episode counter) and of the pool / case lists:
 * hope_env_download_pool_state returns the pool index and the episode counter of every scene; hope_env_restore_maps (host arrays:
 * drawn[i] != 0 where the scene held a drawn map, the saved counters, the seed in use when the maps were drawn) repeats those draws
 * with the SAME pool / cases resident: pass the hope_env_pool_generation value saved with the snapshot and the call fails with
 * HOPE_ESTATE when the pool has been replaced since (a background refresher, hope_env_commit_pool) instead of silently restoring
 * other maps; 0 skips the check.  Runs whose pool is refreshed snapshot the maps themselves (hope_env_download_scenes ->
 * hope_env_set_scenes).  Restore pose / t / accumulator afterwards with hope_env_upload_state.  Host-synchronous. */
int hope_env_download_pool_state(hope_env_t *h, int32_t *pool_index /*[N]*/, uint32_t *episode /*[N]*/);
int hope_env_restore_maps(hope_env_t *h, const uint8_t *drawn /*[N]*/, const uint32_t *episode /*[N]*/, uint64_t seed, uint64_t pool_generation);

/* (ABI 8) Which of the library's streams share a HARDWARE queue.  The runtime spreads HIP streams over a few hardware queues (4 by
 * default) in creation order, and launches of streams that share one serialise: which library stream plays which role of the step's
 * launch structure decides 0.52 vs 0.6+ ms per 65 536-scene step.  Up to round 4 the assignment was a table found by search on one
 * box; since round 5 hope_env_create MEASURES it (pairs of ~100 us spin kernels: two streams on one queue take twice as long; < 5 ms
 * once) and assigns the roles so that the streams a deferred / joined / sub-chain step keeps busy at the same time sit on different
 * queues, whatever other streams the process created first.  queue_of_role[r]: hardware-queue class (0, 1, ...) of role r's stream,
 * -1 = not measured.  Roles (enum Role in hope_amd/csrc/hope_env.hip):
 *   0 caller      the caller's stream (the NULL stream for the usual caller)
 *   1 chain       the second chain (small-tile class): all of it, or its search launches in a pipelined (deferred) step
 *   2 image       the image beside the chains (joined steps) / the static-layer rebuild beside it (pipelined steps)
 *   3 obs large   observation half of the first chain (large-tile class)
 *   4 obs small   observation half of the second chain (small-tile class)
 *   5 search 0    search launches of the first chain in a pipelined step
 *   6 spare       created, not used
 *   7 obs sub     observation half of the second sub-chain of a one-class batch
 * *n_queues = distinct classes seen; *ms = what the measurement took.  Any pointer may be NULL. */
int hope_env_queue_check(hope_env_t *h, int32_t *queue_of_role /*[8]*/, int32_t *n_queues, double *ms);

/* With HOPE_F_PROFILE every kernel launch is bracketed by its own HIP event pair on the launch stream.
 * Returns the accumulated time (ms) and launch count per kernel since the last call with reset != 0:
 * arrays of HOPE_N_KERNELS entries indexed by HOPE_K_*.  Host-synchronous. */
#define HOPE_K_KINEMATICS 0    /* k_kinematics   (four lanes per scene)                      */
#define HOPE_K_STEP 1          /* k_env_step     (wave per scene; one launch per tile class) */
#define HOPE_K_RS_WORDS 2      /* k_rs_words     (wave per queued scene)                     */
#define HOPE_K_RS_VALIDATE 3   /* k_rs_validate  (wave per queued scene; per tile class)     */
#define HOPE_K_IMAGE 4         /* k_bev_image    (wave per scene tile: 16 per scene)         */
#define HOPE_K_IMAGE_PREP 5    /* k_bev_prep     (wave per scene: map + new boxes' spans)    */
#define HOPE_K_RS_COMPACT 6    /* k_rs_compact   (Reeds-Shepp work queues from per-scene flags) */
#define HOPE_K_POST 7           /* k_post         (reward + target arithmetic, one lane per scene; per tile class) */
#define HOPE_K_RS_SEGS 8       /* k_rs_segs      (segment origins of the words to test, one lane per word; per tile class) */
#define HOPE_K_RS_SCREEN 9     /* k_rs_screen    (ABI 8: coarse look at up to four words per pass, wave per queued scene; per tile class) */
#define HOPE_N_KERNELS 10
int hope_env_kernel_ms(hope_env_t *h, double *ms /*[HOPE_N_KERNELS]*/, int64_t *launches /*[HOPE_N_KERNELS]*/,
                       int reset);
/* Same bookkeeping, per CALL instead of per launch: for every hope_env_step / hope_env_reset_obs call and kernel, the time
 * during which at least one launch of that kernel was running (with HOPE_F_OVERLAP the launches of the two tile classes run
 * concurrently on two streams, so this union is shorter than the sum of the per-launch durations).  ms / calls: arrays of
 * HOPE_N_KERNELS entries.  Host-synchronous; call it BEFORE hope_env_kernel_ms with reset (both drain the same events). */
int hope_env_kernel_union_ms(hope_env_t *h, double *ms /*[HOPE_N_KERNELS]*/, int64_t *calls /*[HOPE_N_KERNELS]*/, int reset);
/* Restricts the event bracketing to the kernels whose bit (1 << HOPE_K_*) is set; default all.  An event pair costs
 * a few microseconds of launch latency, so a throughput measurement times only the kernel it reports on. */
int hope_env_profile_kernels(hope_env_t *h, uint32_t kernel_mask);

/* ---- state access (host-sync; tests, checkpointing) ------------------------------------------ */
int hope_env_download_state(hope_env_t *h, double *pose /*[N][3]*/, int32_t *t /*[N]*/,
                            double *accum /*[N]*/);
int hope_env_upload_state(hope_env_t *h, const double *pose, const int32_t *t, const double *accum);

/* ---- test hook ------------------------------------------------------------------------------------------ */
/* Evaluates one elementary function of hope_amd/csrc/hope_math.h (plus sqrt and division) on the DEVICE for n
 * float64 inputs: fn 0 sin, 1 cos, 2 tan, 3 atan2(a,b), 4 asin, 5 acos, 6 hypot(a,b), 7 fmod(a,b), 8 tanh, 9 exp,
 * 10 sqrt, 11 a/b, 12 the kinematics kernel's three-instruction a/20.  a, b, out are DEVICE pointers (b may be NULL for unary functions).  The functions are built
 * from IEEE-exact operations only, so the results must equal the host evaluation bit for bit. */
int hope_debug_math(int fn, int n, const double *a, const double *b, double *out, void *stream);

/* Test hook for the geometry primitives behind the collision, arrival and ring-cull decisions (hope_amd/csrc/hope_dev.h,
 * hope_step_kernel.h): runs the shipped inline function itself on n packed cases on the DEVICE, one 64-lane wave per block, in the
 * calling pattern of the step kernels.  `in`: DEVICE pointer, the cases' float64 records back to back; `out`: DEVICE pointer, int32
 * (fn 0-5, 9) or float64 (fn 6-8), one value per case (fn 5: two).
 *   fn 0 orient_filter             a b c (6)                        -> -1 / 0 / 1, 2 = undecided
 *   fn 1 orient_exact_lds          a b c (6), the expansion on EVERY case -> sign
 *   fn 2 orient_robust_lds         a b c (6)                        -> sign
 *   fn 3 segments_intersect_fast   p1 p2 q1 q2 (8)                  -> 0 / 1, 2 = undecided
 *   fn 4 hull_edge_intersect_robust  pose x, y, cos, sin, edge x1 y1 x2 y2 (8) -> 0 / 1
 *   fn 5 detect_collision          pose x, y, cos, sin, n_obst quads (4 + 8 n_obst); the whole wave, one block per case, quads staged
 *                                  to an LDS tile with the identity list -> hit, number of lanes the filter left undecided
 *   fn 6 quad_intersection_area_lane0    quad A, quad B (16)        -> area
 *   fn 7 quad_intersection_area_private  quad A, quad B (16), 16 lanes clipping 16 cases at a time in k_post's column layout -> area
 *   fn 8 origin_seg_dist           a b (4)                          -> distance
 *   fn 9 arrival_possible          x, y, cos, sin, dest centre x, y, cos, sin of the dest heading (8) -> 0 / 1
 * fn 1, 2 and 4 give the single LDS work area to the 64 cases of a block one lane after the other, as the step kernels do.
 * n_obst is read by fn 5 only (0..32).  HOPE_EINVAL for n < 0, a null pointer, an unknown fn, n_obst out of range.  Additive to ABI 8. */
int hope_debug_geom(int fn, int n, int n_obst, const double *in, void *out, void *stream);

/* Test hook: the launch plan of the NEXT hope_env_step (has_action != 0) or hope_env_reset_obs (has_action == 0) with these `stages`,
 * computed by the function the step itself calls, from the same handle state and the same HOPE_SPLIT_MIN / HOPE_AUTO_CHAINS reads, for a
 * step whose out->rs_word is given.  No HIP call, no change of state.  out: HOST array of `cap` int32 words --
 *   [0] words written  [1] HOPE_STEPPLAN_* flag bits  [2] number of chains, then per chain, in launch order:
 *   tile class (0: <= 32 obstacles), LDS tile capacity, motion kernel (HOPE_STEPPLAN_MOTION_*), observation kernel (HOPE_STEPPLAN_OBS_*),
 *   number of scenes m, and the m scene ids in the order of the chain's launch list (block b of a one-scene kernel steps entry b; a
 *   wave of the pair kernels steps entries 2b and 2b + 1).
 * 3 + 2 * 5 + N words always suffice.  HOPE_EINVAL for a null `out` or a `cap` below the words needed (the message gives the number; nothing
 * is written), HOPE_ESTATE before hope_env_set_scenes.  Additive to ABI 8. */
#define HOPE_STEPPLAN_HEAD 3
#define HOPE_STEPPLAN_CHAIN_HEAD 5
#define HOPE_STEPPLAN_SPLIT 0x1               /* two-launch step kernel: motion launch, then the observation launch */
#define HOPE_STEPPLAN_PIPE 0x2                /* pipelined (HOPE_DEFER_RS): the search streams stay unjoined */
#define HOPE_STEPPLAN_FUSE_KIN 0x4            /* one-launch step kernel that computes its sub-step poses itself: no k_kinematics launch */
#define HOPE_STEPPLAN_AUTO_SUBS 0x8           /* two sub-chains of one tile class */
#define HOPE_STEPPLAN_MOTION_ONE_LAUNCH 0     /* k_env_step, all parts, behind k_kinematics (or action-less) */
#define HOPE_STEPPLAN_MOTION_FUSED_KIN 1      /* k_env_step, all parts, kinematics fused in */
#define HOPE_STEPPLAN_MOTION_TIMING 2         /* the cycle-accounting build of k_env_step (HOPE_STEP_TIMING) */
#define HOPE_STEPPLAN_MOTION_SPLIT 3          /* k_env_step, motion part only, one scene per wave */
#define HOPE_STEPPLAN_MOTION_PAIR 4           /* k_motion_pair, two scenes per wave */
#define HOPE_STEPPLAN_OBS_IN_STEP 0           /* the one-launch step kernel computes the observation */
#define HOPE_STEPPLAN_OBS_SPLIT 1             /* k_env_step, observation part only */
#define HOPE_STEPPLAN_OBS_PAIR 2              /* k_obs_pair */
int hope_env_step_plan(hope_env_t *h, uint32_t stages, int has_action, int32_t *out, int cap);

/* Test hook (pure host code, no device needed): the count-interval table hope_env_upload_tables derives from dist_star / hull_base for
 * the action-mask stage (hope_amd/csrc/hope_step_kernel.h MASK_LUT_*): lut_out [(120 * 128 + 1)][32] uint16, scale_out [120] bins per
 * metre.  tests/test_mask_lut.py checks its bracketing property against the float64 table (action_mask.py:166-177).  HOPE_EINVAL, with
 * the beam named, on the tables hope_env_upload_tables refuses; the outputs are then left untouched. */
int hope_debug_mask_lut(const double *dist_star, const double *hull_base, uint16_t *lut_out, double *scale_out);

/* Profiling hook: one sweep over `bytes` of the DEVICE buffer `buf` with a known byte count in one of the library's access widths --
 * mode 0 / 1 / 2: reads of 16 / 8 / 4 bytes per lane, 3: one 8-byte word per 64-byte line; 4 / 5 / 6 / 7: the same as writes.  Run
 * under `rocprofv3 --pmc FETCH_SIZE` / `WRITE_SIZE` it calibrates those counters (tools/pmc_calib.py; the MI355X guide calibrates the
 * 16-byte read only).  `bytes` should exceed the 256 MiB Infinity Cache several times. */
int hope_debug_traffic(int mode, size_t bytes, void *buf, void *stream);

/* Cycle accounting of the Reeds-Shepp validation kernel: 16 counters accumulated by the instrumented build that the library
 * launches when the environment variable HOPE_RS_TIMING is set (hope_amd/csrc/hope_rs.hip lists the sections); zeros
 * otherwise.  Host-synchronous.  tools/rs_timing.py prints the breakdown. */
int hope_debug_rs_prof(uint64_t *out /*[16]*/, int reset);
/* Statistics of k_rs_validate's float32 filter, accumulated while the environment variable HOPE_RS_DEBUG has bit 0x4000 set:
 * [0] passes [1] passes decided by a certain float32 hit [2] passes that re-evaluated undecided samples in float64 [3] those
 * samples; with bit 0x2000 (self-check: float64 for EVERY sample) also [4] float32 "hit" verdicts float64 contradicts, [5] float32
 * "clear" verdicts float64 contradicts (both must stay 0), [6] samples checked; [8..12] passes left undecided because of: no certain crossing / an
 * axis-parallel obstacle edge / an axis-parallel hull / a hull corner near the edge line / a shallow crossing angle.  Host-synchronous. */
int hope_debug_rs_filter_stats(uint64_t *out /*[16]*/, int reset);
/* details of the first 64 contradicted verdicts of the self-check (16 doubles each; tools/rs_filter_stats.py --check) */
int hope_debug_rs_filter_dump(double *out /*[64][16]*/);
/* Per-search log of the same instrumented build: up to cap records of 4 int32 {wave cycles, words tested | words allowed << 8 |
 * large-tile class << 16, passes, found}; *n = records logged since the last reset.  Host-synchronous.  tools/rs_tail.py. */
int hope_debug_rs_log(int32_t *out /*[cap][4]*/, int cap, int32_t *n, int reset);
/* the same for k_env_step (environment variable HOPE_STEP_TIMING; float32 observation / action handles); tools/step_timing.py */
int hope_debug_step_prof(uint64_t *out /*[16]*/, int reset);
/* Tie census of the same instrumented build (HOPE_STEP_TIMING): how close the workload comes to the decisions whose arithmetic the
 * reference delegates to GEOS (rows a-3, a-4, the ring cull of a-8) and to the mask compares.  out: [0] arrival-ratio evaluations,
 * [1] min |overlap / dest area - 0.95| (bit pattern of a double), [2] lidar ring-keep evaluations, [3] min |ring distance - 10 m|
 * (double), [4] (hull edge, obstacle edge) pairs the orientation filter left undecided (decided by the exact expansion), [6] mask table
 * compares, [7] min non-zero |table entry - scan value| (double), [8] scene-steps whose mask took the exact 1200-beam evaluation,
 * [9] scene-steps, [10] compares whose entry equals the scan value bit for bit.
 * Call once with reset != 0 before counting (the minima start at +inf then).  tools/tie_census.py. */
int hope_debug_census(uint64_t *out /*[16]*/, int reset);

/* ---- host-side scene generator (no device involved; any thread) ------------------------------------------------------ */
/* n scenes of `level` (0 Normal, 1 Complex, 2 Extrem) drawn as ParkingMapNormal.reset does (src/env/parking_map_normal.py:474-494
 * over generate_bay_parking_case :40-246 / generate_parallel_parking_case :248-457): bay lot with probability 1/2 for Normal /
 * Complex, parallel otherwise; map box = floor / ceil of min / max(start, dest) -/+ 10 m.  bay_mode: -1 as the reference, 0
 * parallel only, 1 bay only.  Outputs are HOST arrays in the layout of hope_env_set_scenes / hope_env_set_pool: start [n][3],
 * dest [n][3], bbox [n][4], verts [n][max_obstacles][4][2] (slots beyond n_obst[i] untouched), n_obst [n], case_id [n] (0 bay,
 * 1 parallel; may be NULL).  Scene i depends only on (seed, first_index + i), not on n_threads (<= 0: the environment variable
 * HOPE_HOST_THREADS, else the CPUs in the calling process's affinity mask -- one rank's share of the node once it has pinned
 * itself, hope_amd.dist.pin_rank_to_cores -- never more).
 * Returns 0, HOPE_EINVAL, or -100 - i when scene i has more than max_obstacles obstacles (impossible for max_obstacles >= 18). */
int hope_scenegen_generate(int level, int bay_mode, int n, uint64_t seed, int64_t first_index, int max_obstacles, double *start,
                           double *dest, double *bbox, double *verts, int32_t *n_obst, int32_t *case_id, int n_threads);
/* the fan-out hope_scenegen_generate uses for n_threads <= 0 in this process, now */
int hope_scenegen_default_threads(void);

/* ---- the deterministic generator: one recipe for host and device (hope_amd/csrc/hope_scenegen_core.h) ----------------------------
 * hope_scenegen_generate calls the platform's sin / cos / log, which no device kernel can reproduce bit for bit.  The entry points
 * below draw the SAME recipe (same draws in the same order from the same (seed, index) stream, same rejection rules) with
 * operations IEEE-754 defines exactly, so host and device agree on every bit.  Their lots are distributed as those of
 * hope_scenegen_generate, but are not the same lots.  A lot holds up to 17 obstacles: max_obstacles < 18 is HOPE_EINVAL.
 * (Additive to ABI 8.) */
/* the host twin: signature and semantics of hope_scenegen_generate (the result does not depend on n_threads) */
int hope_scenegen_generate_det(int level, int bay_mode, int n, uint64_t seed, int64_t first_index, int max_obstacles, double *start,
                               double *dest, double *bbox, double *verts, int32_t *n_obst, int32_t *case_id, int n_threads);
/* the same lots drawn by the kernel k_scenegen on device `device_id`, asynchronously on `stream`, into caller-owned DEVICE buffers
 * of the same layout (case_id may be NULL); no handle involved.  Bit-equal to hope_scenegen_generate_det. */
int hope_scenegen_generate_device(int device_id, int level, int bay_mode, int n, uint64_t seed, int64_t first_index, int max_obstacles,
                                  double *start, double *dest, double *bbox, double *verts, int32_t *n_obst, int32_t *case_id, void *stream);
/* y[i] = the generator's own log of x[i] > 0 (exact operations only; what the tests measure against the platform's log) */
int hope_scenegen_log_det(int n, const double *x, double *y);
/* A pool refill that never leaves the device: fills the pool set the kernels are NOT reading with n_per_level[0] Normal, then
 * n_per_level[1] Complex, then n_per_level[2] Extrem lots (sum = n_pool; lot k of level l is lot first_index + k of
 * hope_scenegen_generate_det for seed * 1000003 + l, bay_mode -1) and swaps it in exactly as hope_env_commit_pool (relaxed == 0:
 * launches enqueued afterwards wait in stream order for the generator and draw from the new pool) or hope_env_commit_pool_relaxed
 * (relaxed != 0: the new pool takes over at the first step enqueued after the generator has finished) does.  The kernel writes the
 * pool's own formats (obstacle tiles, counts, constant records) on the handle's pool stream; no host thread, pinned staging or
 * upload is involved, and the call never synchronises with the step kernels.  Dragon-Lake cases stay drawable.
 * hope_env_pool_generation folds in a hash of (n_pool, n_per_level, seed, first_index).  HOPE_EINVAL: n_pool <= 0, a negative
 * count, counts that do not sum to n_pool, a handle with max_obstacles < 18; HOPE_ESTATE: a hope_env_pool_staging fill that has
 * not been committed. */
int hope_env_generate_pool(hope_env_t *h, int n_pool, const int32_t *n_per_level /*[3]*/, uint64_t seed, int64_t first_index, int relaxed);

/* ---- curriculum for new-map draws (additive to ABI 8) -----------------------------------------------------------------
 * The reference's training loops never draw a uniform scene mix: SceneChoose sends half of the choices to the scene type whose
 * recent success rate is furthest below its target and balances the counts with the other half, DlpCaseChoose prefers the
 * Dragon-Lake cases that failed recently, and every finished episode is fed back (src/train/train_HOPE_sac.py:23-97, :215-225).
 * Here the outcome of an episode and the map it ran on exist on the device only, so the curriculum lives there too: a tally of
 * episode outcomes per BUCKET and weighted draw lists rebuilt from it.  Off by default; with it off nothing differs.
 *
 * Buckets: 0 / 1 / 2 generated lots of level Normal / Complex / Extrem (hope_env_generate_pool labels its lots itself; a
 * host-filled pool is labelled with hope_env_set_pool_buckets), 3 "dlp" as a scene type (every Dragon-Lake episode), 4 + c
 * Dragon-Lake case c.  n_buckets = 4 + n_cases <= 254.  Unlabelled pool entries and maps uploaded with hope_env_set_scenes are
 * counted in one extra counter and keep the share of the draws they have without a curriculum.
 *
 * The draw stays `list[key % n]` inside the step kernels; the list becomes a WEIGHTED list of HOPE_CURRICULUM_LIST_LEN positions
 * in which a bucket owns p_b * HOPE_CURRICULUM_LIST_LEN positions (largest remainder, at least one per bucket with entries), so a
 * draw follows p_b to within 1 / HOPE_CURRICULUM_LIST_LEN.  The rule (hope_amd/csrc/hope_curriculum_core.h):
 *   window     per bucket (n, s): an update with (dn, ds) new episodes / successes does n += dn, s += ds and, if n > W,
 *              s *= W / n, n = W (W = type_window for buckets 0 - 3, case_window for the cases);
 *   types      fail_t = clip(target_t - s_t / n_t, type_fail_min, 1), pw = fail / sum(fail) (_choose_case_worst_perform);
 *              q_t = max(worst_share * pw_t, h), h such that sum(q) = 1: the long-run type frequencies of SceneChoose.choose_case;
 *              uniform before type_horizon episodes.  The small-tile class draws level l with q_l / (q_0 + q_1 + q_2) over the
 *              levels its pool holds.  LIMIT: which scene slots are Dragon-Lake slots is fixed (tile class 1), so q_3 cannot move
 *              scenes between the classes: it is reported and otherwise unused;
 *   cases      rate_c = 0 if n_c <= 1 else s_c / n_c, fail_c = clip(1 - rate_c, case_fail_min, 1),
 *              p_c = case_uniform / n_cases + (1 - case_uniform) * fail_c / sum(fail); uniform before case_horizon Dragon-Lake
 *              episodes.  Unlabelled lots in the same list keep their share n_lots / (n_lots + n_cases).
 * Misuse returns HOPE_EINVAL / HOPE_ESTATE with a message: tally before enable, labels of the wrong length, a bucket id out of
 * range, hope_env_set_dlp_cases while the curriculum is on. */
#define HOPE_CURRICULUM_LIST_LEN (1 << 20)
typedef struct hope_curriculum_params {
    double target[4];        /* target success rate of Normal / Complex / Extrem / dlp: 0.95 0.95 0.9 0.99 */
    double type_window;      /* 250 */
    double case_window;      /* 10 */
    double type_fail_min;    /* 0.01 */
    double case_fail_min;    /* 0.005 */
    double worst_share;      /* 0.5: share of the choices that go to the worst-performing type */
    double case_uniform;     /* 0.2: share of the case choices that stay uniform */
    int64_t type_horizon;    /* 200 */
    int64_t case_horizon;    /* 500 */
} hope_curriculum_params;
/* Switches the curriculum on (params NULL: the reference's constants above) with empty counters and windows, builds the weighted
 * lists of the resident pool (uniform within each kind at this point) and notes the bucket of the map every scene holds now.
 * HOPE_ESTATE without a pool or Dragon-Lake cases; HOPE_EINVAL for more than 250 cases or non-positive windows.  Host-synchronous. */
int hope_env_curriculum_enable(hope_env_t *h, const hope_curriculum_params *params);
/* back to the uniform base lists; counters and windows are dropped.  Host-synchronous. */
int hope_env_curriculum_disable(hope_env_t *h);
/* labels the RESIDENT pool set: bucket[k] in {0, 1, 2} = level of pool entry k, 255 = unlabelled; n_pool must be the resident
 * pool's size.  Host array, host-synchronous; the labels last until that set is replaced. */
int hope_env_set_pool_buckets(hope_env_t *h, int n_pool, const uint8_t *bucket);
/* k_curriculum_tally, asynchronous on `stream` (the stream of the steps), right after a step: for every scene with done[i] != 0 the
 * bucket of the map the FINISHED episode ran on gets one episode and, if status[i] == HOPE_STATUS_ARRIVED, one success (a
 * Dragon-Lake episode counts in bucket 3 and in 4 + c); then the bucket of the map the scene holds now (after the fused redraw) is
 * noted for the next time, if the scene drew a new map (a scene that restarts on the same map keeps its bucket; hope_env_redraw notes
 * the buckets of the maps it draws; a map uploaded with hope_env_set_scenes is unlabelled).  status / done: the DEVICE buffers of that
 * step's hope_step_out.  Every scene with done[i] != 0 is counted: call it once per step. */
int hope_env_curriculum_tally(hope_env_t *h, const int32_t *status, const uint8_t *done, void *stream);
/* k_curriculum_weights + k_curriculum_fill: folds the counters since the last update into the windows, recomputes the
 * probabilities and fills the weighted lists the kernels are NOT reading, on the handle's pool stream, ordered after everything
 * enqueued on `stream` so far; the swap is applied at the next step enqueued, which waits in stream order (as hope_env_commit_pool).
 * No host synchronisation.  A pool swap of any kind while the curriculum is on rebuilds the lists for the incoming set with the
 * current windows before that set is drawn from.  Counters that a tally enqueued behind the update adds while the fold reads them
 * are folded by the next update (never more successes than episodes in one fold). */
int hope_env_curriculum_update(hope_env_t *h, void *stream);
/* Download (host-synchronous; any pointer may be NULL): *n_buckets = 4 + n_cases; episodes / successes [n_buckets] cumulative since
 * enable; win_n / win_s [n_buckets] the windows; prob [n_buckets]: q_0 .. q_3, then p_c per case; pw [4]; misc [4]: updates
 * applied, episodes and successes on unlabelled maps, 1 when the curriculum is on. */
int hope_env_curriculum_state(hope_env_t *h, int32_t *n_buckets, uint64_t *episodes, uint64_t *successes, double *win_n, double *win_s,
                              double *prob, double *pw, uint64_t *misc);
/* Test hook: sets the windows (and the cumulative episode counters the two horizons look at) by hand and rebuilds the lists from them,
 * as an update without counters would.  It carries the curriculum's own state over to another handle, NOT the per-scene part: the
 * bucket noted for the map each scene holds is whatever the handle has (hope_env_curriculum_enable notes it from the scenes' current
 * pool indices).  Host arrays [n_buckets]; host-synchronous. */
int hope_env_curriculum_set_windows(hope_env_t *h, int n_buckets, const double *win_n, const double *win_s, const uint64_t *episodes,
                                    const uint64_t *successes);
/* the two weighted lists as the next step will read them (host arrays [HOPE_CURRICULUM_LIST_LEN] int32 each, either may be NULL; a
 * class without entries is left untouched) and the positions every group owns in them (positions [2][n_buckets], may be NULL: per
 * class, groups 0 - 2 the levels, 3 the unlabelled lots, 4 + c case c).  Host-synchronous. */
int hope_env_curriculum_download_lists(hope_env_t *h, int32_t *list0, int32_t *list1, int32_t *positions);
/* Test hooks, pure host code, no device needed.  hope_curriculum_lists_host: the lists hope_env_curriculum_update builds for a pool
 * of n_pool entries with obstacle counts n_obst and labels bucket (NULL: all unlabelled), n_cases Dragon-Lake cases and a handle
 * with max_obstacles, from the windows win_n / win_s and the cumulative episode counters episodes (all [4 + n_cases]) -- the same
 * source compiled for the host (hope_amd/csrc/hope_curriculum_core.h), bit-equal to the device's.  Outputs (any may be NULL):
 * list0 / list1 [HOPE_CURRICULUM_LIST_LEN], prob [4 + n_cases], pw [4], positions [2][4 + n_cases].
 * hope_curriculum_fold_host: the window rule for one bucket. */
int hope_curriculum_lists_host(const hope_curriculum_params *params, int n_pool, const int32_t *n_obst, const uint8_t *bucket, int n_cases,
                               int max_obstacles, const uint64_t *episodes, const double *win_n, const double *win_s, int32_t *list0,
                               int32_t *list1, double *prob, double *pw, int32_t *positions);
int hope_curriculum_fold_host(double *n, double *s, double dn, double ds, double window);

/* ---- map difficulty label (additive to ABI 8) ----------------------------------------------------------------------------------
 * `get_map_level` of the reference (src/env/map_level.py:27-112), which ParkingMapDLP.reset stores as map.map_level on every reset
 * (src/env/parking_map_dlp.py:84) and the evaluation buckets its statistics by (src/evaluation/eval_utils.py:69-72, :99), for
 * whole batches: one source (hope_amd/csrc/hope_maplevel_core.h, a restatement of hope_amd/map_level.py in exact operations) compiled
 * for the host and as the kernel k_map_level (one wavefront per scene), bit-equal to each other.  Scene layout as
 * hope_env_set_scenes: start [n][3], dest [n][3], verts [n][max_obstacles][4][2], n_obst [n] (clamped to 0 .. max_obstacles; <= 1
 * gives Normal).  A triangle's slot (last vertex repeated) is read as a ring of three vertices.
 * level [n] uint8: 0 Normal, 1 Complex, 2 Extrem.  detail [n][8] int32, may be NULL: [0..3] index of the left / right / front /
 * back obstacle of the dest box (-1 none; each obstacle used once, the lower index wins equal distances), [4] which return fired
 * (ML_B_* in hope_maplevel_core.h: 1 few obstacles, 2 - 4 the Extrem tests, 5 - 7 bay, 8 - 10 parallel, 11 - 12 the fall-through
 * rules), [5] start further than 15 m from dest, [6] obstacles that meet the free rectangle (counted only with a detail buffer; the
 * label needs the first), [7] 0.
 * Misuse: HOPE_EINVAL (NULL level or input, n <= 0, max_obstacles outside 1 .. HOPE_MAX_OBSTACLES), HOPE_ESTATE (handle without
 * scenes). */
/* pure host code, no device; the result does not depend on n_threads (<= 0: as hope_scenegen_generate) */
int hope_map_level_host(int n, int max_obstacles, const double *start, const double *dest, const double *verts, const int32_t *n_obst,
                        uint8_t *level, int32_t *detail, int n_threads);
/* the same from DEVICE buffers on device `device_id`, asynchronously on `stream`; no handle involved */
int hope_map_level_device(int device_id, int n, int max_obstacles, const double *start, const double *dest, const double *verts,
                          const int32_t *n_obst, uint8_t *level, int32_t *detail, void *stream);
/* labels the maps the handle's scenes hold NOW (pool draws, Dragon-Lake draws and hope_env_set_scenes uploads alike), reading the
 * handle's own tiles, start and dest: asynchronous on `stream`, ordered like every other entry that reads the handle's state (it
 * joins a pipelined step first).  active: DEVICE u8 [N] or NULL; scenes with active[i] == 0 keep level[i] / detail[i] -- after a step
 * with HOPE_AUTO_REDRAW pass that step's `done` to relabel only the scenes that drew a new map.  level: DEVICE u8 [N]; detail:
 * DEVICE i32 [N][8] or NULL. */
int hope_env_map_level(hope_env_t *h, const uint8_t *active, uint8_t *level, int32_t *detail, void *stream);

/* ---- replay of found Reeds-Shepp paths (additive to ABI 8) --------------------------------------------------------------------
 * The reference's hybrid controller: RsPlanner (src/model/agent/parking_agent.py:2-47) turns a found path into unit actions
 * [steer in {1, 0, -1}, signed fraction of a full step] and ParkingAgent.choose_action (:78-95) replays them instead of asking the
 * policy; a new path is adopted only while none is being replayed (set_planner_path :65-69) and the path is dropped at episode end
 * (reset :61-63).  Here the planner is device-resident state of the handle: 48 bytes per scene (the five segment lengths in steps
 * and a packed cursor word; nothing is expanded into a queue, so there is no cap on the number of actions) and one kernel, k_plan,
 * per step.  Off until enabled; with it off no launch, pointer or output of any other entry point differs.  The rule, the state
 * layout and the bit-equal host twin: hope_amd/csrc/hope_planner_core.h, DESIGN.md 5e.
 *
 * One planner step does, per scene and in this order: done[s] != 0 clears the path; a found word (rs_word[s][6] > 0) is adopted
 * if the scene is idle, or always with HOPE_PLAN_FORCED (a word that expands to no action leaves the scene idle); a busy scene
 * pops its next action and is idle again after its last one. */
#define HOPE_PLAN_STATE_WORDS 6     /* 8-byte words of state per scene, stored as planes: [6][N] */
#define HOPE_PLAN_STEP_RATIO 1.25   /* kinetic_model.step_len * n_step * VALID_SPEED[1] = 0.05 * 10 * 2.5 (train_HOPE_sac.py:164) */
/* bits of the `forced` argument */
#define HOPE_PLAN_FORCED 0x1        /* set_planner_path(forced=True): a found word replaces a path that is being replayed */
#define HOPE_PLAN_NO_POP 0x2        /* sub-steps 1 and 2 only: nothing is popped, no output is written */
/* allocate and zero the state (every scene idle).  step_ratio: metres per full action; <= 0 takes HOPE_PLAN_STEP_RATIO.  Enabling an
 * enabled planner clears it.  Host-synchronous. */
int hope_env_planner_enable(hope_env_t *h, double step_ratio);
/* free the state.  Host-synchronous (planner steps in flight read it). */
int hope_env_planner_disable(hope_env_t *h);
/* clears the path of the scenes with mask[s] != 0 (DEVICE u8 [N]), or of every scene when mask is NULL; asynchronous on `stream` */
int hope_env_planner_reset(hope_env_t *h, const uint8_t *mask, void *stream);
/* k_plan, asynchronous on `stream`; never synchronises the host.  DEVICE buffers: rs_word i8 [N][8] (8-byte aligned) and rs_lengths
 * real [N][5] as hope_step_out has them (float64 iff the handle has HOPE_F_OBS_F64); done u8 [N] or NULL; planned_out f64 [N][2]
 * (16-byte aligned; rows of scenes that pop nothing are written as 0) or NULL; executing_out u8 [N] (1 where planned_out holds an
 * action) or NULL; actions_inout [N][2] float32 or float64 (action_is_f64; 8- / 16-byte aligned) or NULL: the rows of executing
 * scenes are overwritten with the planned action rounded to that type, the others are left as they are.  forced: HOPE_PLAN_* bits.
 * step != 0: the call first does exactly what hope_env_wait_rs_step(h, step, stream) does -- the words it reads are those of THAT
 * step's search, and HOPE_ESTATE (nothing touched) when a newer step has been enqueued since.  step == 0: no wait; the caller has
 * ordered `stream` after whatever wrote the buffers.  HOPE_ESTATE before hope_env_planner_enable, HOPE_EINVAL for a NULL or
 * misaligned rs_word / rs_lengths / output. */
int hope_env_planner_step(hope_env_t *h, const int8_t *rs_word, const void *rs_lengths, const uint8_t *done, int forced, uint64_t step,
                          double *planned_out, uint8_t *executing_out, void *actions_inout, int action_is_f64, void *stream);
/* The same step over HOST arrays with a caller-owned state block (HOPE_PLAN_STATE_WORDS * n 8-byte words, zeroed = every scene
 * idle; zeroing a scene's six words clears its path): pure host code from the same source, no handle, no device.  Bit-equal to k_plan. */
int hope_planner_step_host(int n, double step_ratio, void *state, const int8_t *rs_word, const void *rs_lengths, int lengths_f64,
                           const uint8_t *done, int forced, double *planned_out, uint8_t *executing_out, void *actions_inout,
                           int action_is_f64);
/* the state block as the next planner step will read it (host array of HOPE_PLAN_STATE_WORDS * N 8-byte words); host-synchronous */
int hope_env_planner_download_state(hope_env_t *h, void *state_out);

/* ---- masked choice of the discrete action (additive to ABI 8) -------------------------------------------------------------------
 * The reference's ActionMask.choose_action (src/model/action_mask.py:199-227) as one kernel, k_choose, behind the policy forward:
 * the Gaussian head's density at the 42 discrete actions, weighed with the action mask, one draw per scene, the cast / clamp / path
 * replay override of the agent (parking_agent.py:80-99) and the log-probability of the action taken -- two numbers per scene out of
 * one launch.  Off until enabled; with it off no launch, pointer or output of any other entry point differs.  The rule, the
 * treatment of degenerate rows and the bit-equal host twin: hope_amd/csrc/hope_chooser_core.h, DESIGN.md 5f. */
/* flag bits of the index output; idx & 63 is always a legal action index */
#define HOPE_CHOOSE_NOMASK 64       /* the row's mask was unusable (sum of weights not positive / not finite): drawn with every mask = 1 */
#define HOPE_CHOOSE_FIXED 128       /* still unusable, or a non-finite mean / log_std: index 10 (straight ahead) was taken */
/* upload the action table: HOST float64 [42][2] in the policy's [-1, 1] scaling, rows 0 .. 20 the 21 steers at one speed, rows
 * 21 .. 41 the same steers at the other (HOPE_EINVAL otherwise).  Enabling again replaces the table.  Host-synchronous. */
int hope_env_chooser_enable(hope_env_t *h, const double *actions);
/* free the table.  Host-synchronous (choices in flight read it). */
int hope_env_chooser_disable(hope_env_t *h);
/* k_choose, asynchronous on `stream`; waits for nothing and never synchronises the host -- it does not join a deferred search
 * (hope_env_planner_step / hope_env_wait_rs do; call them first when planned / executing come from that step).  DEVICE buffers, N =
 * the handle's scenes:
 *   mean [N][2], log_std     float32, or float64 with in_f64 != 0; mean aligned to a row (8 / 16 bytes).  log_std_row_stride: 2 for
 *                            [N][2], 0 to broadcast one row
 *   mask [N][42]             the handle's observation type (hope_step_out.action_mask); required
 *   planned f64 [N][2] (16-byte aligned), executing u8 [N]: both or neither (hope_env_planner_step's outputs); rows with
 *                            executing != 0 take (float)planned
 *   u f64 [N] in [0, 1)      or NULL: the draw of scene s is then the counter-based uniform of (seed, counter, s)
 *   action [N][2]            the handle's action type (float64 iff HOPE_F_ACTION_F64: (double) of the float32 value); required;
 *                            8- / 16-byte aligned
 *   action_f32 f32 [N][2], idx i32 [N] (index | HOPE_CHOOSE_* bits), log_prob f32 [N][2], probs f64 [N][42] (= e_k / S): each may
 *                            be NULL; action_f32 may be `action` itself on a float32 handle
 * HOPE_ESTATE before hope_env_chooser_enable; HOPE_EINVAL for a NULL mean / log_std / mask / action, planned without executing or
 * the reverse, a stride other than 0 / 2, a misaligned buffer. */
int hope_env_choose(hope_env_t *h, const void *mean, const void *log_std, int log_std_row_stride, int in_f64, const void *mask,
                    const double *planned, const uint8_t *executing, const double *u, uint64_t seed, uint64_t counter, void *action,
                    float *action_f32, int32_t *idx, float *log_prob, double *probs, void *stream);
/* The same choice over HOST arrays of n scenes: pure host code from the same source, no handle, no device.  Bit-equal to k_choose.
 * mask_f64 / action_f64: the types the handle's flags give on the device.  scene0: the index of row 0 in the counter-based draw, so
 * that a batch may be split.  No alignment requirements. */
int hope_chooser_host(int n, const double *actions, const void *mean, const void *log_std, int log_std_row_stride, int in_f64,
                      const void *mask, int mask_f64, const double *planned, const uint8_t *executing, const double *u, uint64_t seed,
                      uint64_t counter, uint64_t scene0, void *action, int action_f64, float *action_f32, int32_t *idx, float *log_prob,
                      double *probs);

/* ---- normalisation of the observations (additive to ABI 8) ----------------------------------------------------------------------
 * The reference's StateNorm (src/model/state_norm.py:25-47) for every scene at once: running mean / S / std of the 120 lidar and 5
 * target columns in float64, folded in with a parallel merge whose arithmetic order is fixed (64-row chunks, an aligned binary tree),
 * and out = (float)((x - mean) / (std + 1e-8)).  Three kernels: k_obsnorm_partial, k_obsnorm_merge (update), k_obsnorm_apply
 * (normalize).  Off until enabled; with it off no launch, pointer or output of any other entry point differs.  The rule and the
 * bit-equal host twin: hope_amd/csrc/hope_obsnorm_core.h, DESIGN.md 5g. */
#define HOPE_OBSNORM_LIDAR 120
#define HOPE_OBSNORM_TARGET 5
#define HOPE_OBSNORM_COLS 125       /* columns 0 .. 119 lidar, 120 .. 124 target */
#define HOPE_OBSNORM_UPDATE 0x1u    /* fold the rows into the running statistics */
#define HOPE_OBSNORM_NORMALIZE 0x2u /* write the normalised rows (after the fold when both are set) */
/* the statistics as the host twin holds them */
typedef struct hope_obsnorm_state {
    int64_t n_state;                /* observations folded in so far */
    double mean[HOPE_OBSNORM_COLS], S[HOPE_OBSNORM_COLS], std[HOPE_OBSNORM_COLS];
} hope_obsnorm_state;
/* allocate the statistics (zero, n_state = 0) and the chunk partials (3 x 125 x ceil(N / 64) doubles).  Enabling an enabled handle
 * keeps its statistics.  Host-synchronous. */
int hope_env_obsnorm_enable(hope_env_t *h);
/* free both.  Host-synchronous (calls in flight use them). */
int hope_env_obsnorm_disable(hope_env_t *h);
/* replace / read the statistics: HOST arrays of 125 doubles each.  Both wait for the device (calls in flight read and write the
 * statistics).  `set` is how statistics from a checkpoint reach the device; n_state >= 0.  `get` with mean, S and std all NULL
 * returns n_state alone, which the handle keeps on the host, without waiting. */
int hope_env_obsnorm_set(hope_env_t *h, int64_t n_state, const double *mean, const double *S, const double *std);
int hope_env_obsnorm_get(hope_env_t *h, int64_t *n_state, double *mean, double *S, double *std);
/* asynchronous on `stream`; waits for nothing, never synchronises the host and does not join a deferred search (the observation
 * buffers are complete at the step's first completion point).  DEVICE buffers:
 *   lidar [rows][120], target [rows][5]    float32, or float64 with in_f64 != 0; aligned to their element; 1 <= rows <= N
 *   out_lidar [rows][120], out_target [rows][5]   float32; required with HOPE_OBSNORM_NORMALIZE, ignored without
 * flags: HOPE_OBSNORM_UPDATE | HOPE_OBSNORM_NORMALIZE, at least one.  With both the call folds first and normalises with the new
 * statistics.  The handle counts n_state at the call, so calls belong on one stream (or are ordered by the caller).
 * HOPE_ESTATE before hope_env_obsnorm_enable; HOPE_EINVAL for a NULL or misaligned pointer, rows out of range, no or an unknown
 * flag, NORMALIZE without both outputs. */
int hope_env_obsnorm(hope_env_t *h, const void *lidar, const void *target, int rows, int in_f64, uint32_t flags, float *out_lidar,
                     float *out_target, void *stream);
/* The same over HOST arrays: pure host code from the same source, no handle, no device; bit-equal to the kernels.  The caller owns
 * `state` (zero it to start).  No alignment requirements, no upper bound on rows.  HOPE_EINVAL for a NULL state / lidar / target,
 * rows < 1, a negative n_state, no or an unknown flag, NORMALIZE without both outputs. */
int hope_obsnorm_host(hope_obsnorm_state *state, const void *lidar, const void *target, int64_t rows, int in_f64, uint32_t flags,
                      float *out_lidar, float *out_target);

/* ---- bookkeeping of an evaluation run (additive to ABI 8) -----------------------------------------------------------------------
 * What the reference's eval() keeps per episode (src/evaluation/eval_utils.py:35-57) for every scene at once: the stuck detector
 * and its random physical action (:46-47), the step count, the summed reward, the path length (:52-53), the final status, the mask of
 * the episodes still running, and the hiding of a frozen slot's stale Reeds-Shepp word from the planner.  Three kernels, one lane per
 * scene: k_eval_begin (after the first observation), k_eval_override (between the policy and the env step), k_eval_track (after the
 * env step).  Off until enabled; with it off no launch, pointer or output of any other entry point differs.  The rule, the state
 * layout, the counter-based draw and the bit-equal host twins: hope_amd/csrc/hope_evaltrack_core.h, DESIGN.md 5h.
 *
 * State: 80 bytes per scene, stored as planes [10][N] of 8-byte words -- planes 0-4 the previous target (float64), 5-6 the previous
 * rear-axle position, 7 the summed reward, 8 the path length, 9 packed: bits 0-31 steps, 32-39 status, bit 40 alive, bit 41 stuck.
 * A stored NaN is always 0x7FF8000000000000.  `target` and `reward` below have the handle's observation type (float64 iff
 * HOPE_F_OBS_F64), `pose` is f64 [N][3], `status` i32 [N], `done` u8 [N], `rs_word` i8 [N][8] (8-byte aligned), as hope_step_out has
 * them; every pointer is explicit and a DEVICE pointer.  All calls but enable / disable / download_state are asynchronous on
 * `stream`, wait for nothing (they do not join a deferred search) and never synchronise the host.  HOPE_ESTATE before
 * hope_env_eval_enable; HOPE_EINVAL for a NULL required pointer or a misaligned buffer; the handle stays usable after an error. */
#define HOPE_EVAL_STATE_WORDS 10    /* 8-byte words of state per scene, stored as planes: [10][N] */
/* allocate and zero the state.  box: HOST float64 [4] = steer lo, steer hi, speed lo, speed hi of the physical action box the stuck
 * detector draws from (finite, HOPE_EINVAL otherwise).  Enabling an enabled handle replaces the box and keeps the state.
 * Host-synchronous. */
int hope_env_eval_enable(hope_env_t *h, const double *box);
/* free the state.  Host-synchronous (calls in flight use it). */
int hope_env_eval_disable(hope_env_t *h);
/* k_eval_begin: a new episode in every scene -- the previous target and position are (target, pose), sums and steps 0, status 1,
 * alive, stuck (the reference's first comparison is obs['target'] with itself: the first action of every episode is the random one) */
int hope_env_eval_begin(hope_env_t *h, const void *target, const double *pose, void *stream);
/* k_eval_override: active_out u8 [N] = alive; the action row of every scene whose `stuck` bit is set (alive or not) is replaced by
 * clamp(lo_d + (hi_d - lo_d) * u_d, -1, 1) rounded once to the action type; other rows are not touched.  actions_inout [N][2]
 * float32 or float64 (action_is_f64; 8- / 16-byte aligned).  u f64 [N][2] in [0, 1) or NULL: the draw of scene s, dimension d is then
 * the counter-based uniform of (seed, counter, s, d); counter = the index of the episode step. */
int hope_env_eval_override(hope_env_t *h, void *actions_inout, int action_is_f64, const double *u, uint64_t seed, uint64_t counter,
                           uint8_t *active_out, void *stream);
/* k_eval_track, after the env step: a live scene counts the step, adds reward and displacement; `done` on a live scene freezes it
 * with the env's status; every scene compares target with the previous one (stuck) and takes over target and position.  word_out i8
 * [N][8] (8-byte aligned; may be rs_word itself) = rs_word with byte 6 (found) zeroed unless the scene is still alive after this
 * step; done_out u8 [N] = the scene's episode ended in this step. */
int hope_env_eval_track(hope_env_t *h, const void *target, const double *pose, const void *reward, const int32_t *status,
                        const uint8_t *done, const int8_t *rs_word, int8_t *word_out, uint8_t *done_out, void *stream);
/* rec_out f32 [N][4] (16-byte aligned) = status, steps, (float)summed reward, (float)path length */
int hope_env_eval_records(hope_env_t *h, float *rec_out, void *stream);
/* the state block as the next call will read it (host array of HOPE_EVAL_STATE_WORDS * N 8-byte words); host-synchronous */
int hope_env_eval_download_state(hope_env_t *h, void *state_out);
/* The same three operations over HOST arrays with a caller-owned state block: pure host code from the same source, no handle, no
 * device; bit-equal to the kernels.  state: HOPE_EVAL_STATE_WORDS planes, `state_stride` words apart, whose words 0 .. n-1 are this
 * call's scenes (state_stride >= n; a part of a larger block passes the block's stride and the address of its first scene's word in
 * plane 0).  obs_f64: the type of target and reward.  scene0: the index of row 0 in the counter-based draw, so that a batch may be
 * split.  No alignment requirements.  HOPE_EINVAL for n <= 0, state_stride < n, a NULL required pointer or a box that is not finite. */
int hope_eval_begin_host(int64_t n, int64_t state_stride, void *state, const void *target, int obs_f64, const double *pose);
int hope_eval_override_host(int64_t n, int64_t state_stride, const void *state, const double *box, void *actions_inout,
                            int action_is_f64, const double *u, uint64_t seed, uint64_t counter, uint64_t scene0, uint8_t *active_out);
int hope_eval_track_host(int64_t n, int64_t state_stride, void *state, const void *target, int obs_f64, const double *pose,
                         const void *reward, const int32_t *status, const uint8_t *done, const int8_t *rs_word, int8_t *word_out,
                         uint8_t *done_out);

/* ---- PPO's advantage block (additive to ABI 8) ----------------------------------------------------------------------------------
 * What BatchedPPO.advantages does after the critic forwards (the reference's PPO.update, src/model/agent/ppo_agent.py:255-273), for
 * every scene at once: the generalised advantage estimate along T, the critic's target adv + V_target(s), and the advantages'
 * normalisation by their global mean and unbiased standard deviation.  Three kernels: k_gae_scan (one lane per row: the backward
 * scan and the row's share of the two sums), k_gae_merge (the chunk partials' tree), k_adv_apply.  The sums have one arithmetic
 * order, independent of the launch geometry, and are plain sums {sum adv, sum adv^2, count}: ranks add theirs between
 * hope_env_gae(HOPE_GAE_SUMS) and hope_env_adv_normalize.  Off until enabled; with it off no launch, pointer or output of any other
 * entry point differs.  The rule and the bit-equal host twins: hope_amd/csrc/hope_gae_core.h, DESIGN.md 5i. */
#define HOPE_GAE_SUMS 0x1u          /* also reduce {sum adv, sum adv^2, rows * T} into `sums` */
#define HOPE_GAE_NORMALIZE 0x2u     /* implies HOPE_GAE_SUMS; then adv = (adv - mean) / (std + 1e-5f) in place */
#define HOPE_GAE_MAX_T 4096
/* allocate the chunk partials (2 x ceil(N / 64) doubles) and the handle's own sums[3].  Enabling an enabled handle changes nothing.
 * Host-synchronous. */
int hope_env_gae_enable(hope_env_t *h);
/* free both.  Host-synchronous (calls in flight use them). */
int hope_env_gae_disable(hope_env_t *h);
/* asynchronous on `stream`; waits for nothing, never synchronises the host and does not join a deferred search.  DEVICE buffers,
 * float32, contiguous, 4-byte aligned (with T % 4 == 0 and every [rows][T] base 16-byte aligned the scan moves four time steps per
 * load and store; the results do not depend on that):
 *   reward, done, value, value_target [rows][T]   done holds 0 / 1; value_target is the target critic's output
 *   v_last [rows]                                 the critic's value of the observation after the newest column
 *   adv, v_target [rows][T]                       outputs
 *   sums double[3] (8-byte aligned) or NULL       NULL: the handle's own block (what a later hope_env_adv_normalize with NULL reads)
 * 1 <= rows <= N, 1 <= T <= HOPE_GAE_MAX_T; gamma and lam finite.  flags: 0 (scan only), HOPE_GAE_SUMS, HOPE_GAE_NORMALIZE or
 * both.  The chunk partials belong to the handle, so calls belong on one stream (or are ordered by the caller).
 * HOPE_ESTATE before hope_env_gae_enable; HOPE_EINVAL for a NULL required pointer, a misaligned pointer, rows or T out of range, an
 * unknown flag, a gamma or lam that is not finite.  The handle stays usable after an error. */
int hope_env_gae(hope_env_t *h, const float *reward, const float *done, const float *value, const float *v_last,
                 const float *value_target, int rows, int T, double gamma, double lam, uint32_t flags, float *adv, float *v_target,
                 double *sums, void *stream);
/* step 3 alone: out[e] = (adv[e] - mean) / (std + 1e-5f) for e < count, mean and std from `sums` (DEVICE double[3], e.g. all-reduced
 * by the caller; NULL: the handle's own).  out may be adv.  count >= 1.  Asynchronous on `stream`. */
int hope_env_adv_normalize(hope_env_t *h, const float *adv, int64_t count, const double *sums, float *out, void *stream);
/* The same over HOST arrays: pure host code from the same source, no handle, no device; bit-equal to the kernels.  No alignment
 * requirements, no upper bound on rows or T.  hope_gae_host: sums and delta may be NULL; delta [rows][T] takes the float32
 * one-step residuals (agent_glue.batched_gae's second result).  hope_adv_normalize_host: mean_std (may be NULL) takes the float32
 * mean and std that the normalisation uses; count == 0 computes those alone (adv and out are then not read).  HOPE_EINVAL for a
 * NULL required pointer, rows or T < 1, an unknown flag, a gamma or lam that is not finite, a negative count. */
int hope_gae_host(const float *reward, const float *done, const float *value, const float *v_last, const float *value_target,
                  int64_t rows, int64_t T, double gamma, double lam, uint32_t flags, float *adv, float *v_target, double *sums,
                  float *delta);
int hope_adv_normalize_host(const float *adv, int64_t count, const double *sums, float *out, float *mean_std);

/* ---- the transition ring (additive to ABI 8) ------------------------------------------------------------------------------------
 * What rollout.TransitionRing and the three running statistics behind it do between the env step and the policy (the batched
 * ReplayMemory of the reference, src/model/replay_memory.py:6-49): the push of a column in two halves, the tally of episodes,
 * successes and rewards of the same step, and the uniform draw of a SAC batch with its next observations.  Four kernels:
 * k_ring_before (a wave per scene row), k_ring_after (a lane per scene: the two column stores and the chunk's share of the tally),
 * k_ring_tally (one wave: the partials into the running totals), k_ring_sample (a wave per batch item).  The ring's tensors and the
 * totals are the caller's; the handle holds the chunk partials only.  Off until enabled; with it off no launch, pointer or output of
 * any other entry point differs.  The rule and the bit-equal host twins: hope_amd/csrc/hope_ring_core.h, DESIGN.md 5j. */
#define HOPE_RING_MAX_T 4096
#define HOPE_RING_MAX_BATCH 1048576
/* the ring: float32, contiguous; n scenes x T columns */
typedef struct hope_ring_t {
    float *lidar;          /* [n][T][120] */
    float *target;         /* [n][T][5] */
    float *action_mask;    /* [n][T][42] */
    float *action;         /* [n][T][2] */
    float *log_prob;       /* [n][T][2] */
    float *reward;         /* [n][T] */
    float *done;           /* [n][T]: 0 / 1 */
    int32_t n, T;
} hope_ring_t;
/* a batch drawn from it: float32, contiguous */
typedef struct hope_ring_batch_t {
    float *obs_lidar;      /* [batch][120] */
    float *obs_target;     /* [batch][5] */
    float *obs_mask;       /* [batch][42] */
    float *next_lidar;     /* [batch][120] */
    float *next_target;    /* [batch][5] */
    float *next_mask;      /* [batch][42] */
    float *action;         /* [batch][2] */
    float *reward;         /* [batch] */
    float *done;           /* [batch] */
    int32_t *idx;          /* [batch][3]: scene, column, next column (-1: the newest column, next_* is last_*); all -1: a refused row */
} hope_ring_batch_t;
/* allocate the chunk partials of the tally (ceil(N / 64) doubles and 2 x ceil(N / 64) int32).  Enabling an enabled handle changes
 * nothing.  Host-synchronous. */
int hope_env_ring_enable(hope_env_t *h);
/* free them.  Host-synchronous (calls in flight use them). */
int hope_env_ring_disable(hope_env_t *h);
/* The three calls below are asynchronous on `stream`; they wait for nothing, never synchronise the host and do not join a deferred
 * search.  The structs are HOST memory, read during the call; everything they and the other arguments point to is DEVICE memory,
 * aligned to its element (float32 4, int64 / float64 8 bytes).  1 <= ring->n <= N, 1 <= ring->T <= HOPE_RING_MAX_T.
 * HOPE_ESTATE before hope_env_ring_enable; HOPE_EINVAL for a NULL or misaligned pointer or a number out of range; on any error
 * nothing is launched and the handle stays usable.
 *
 * before half of column t (0 <= t < T): lidar [n][120], target [n][5], mask [n][42], action [n][2], log_prob [n][2], float32, go
 * into [i][t] word for word.  One launch; with the lidar bases (input and ring) 16-byte and the mask / action / log_prob bases
 * 8-byte aligned a lane moves 16 / 8 bytes, otherwise 4; the results do not depend on that. */
int hope_env_ring_before(hope_env_t *h, const hope_ring_t *ring, int t, const float *lidar, const float *target, const float *mask,
                         const float *action, const float *log_prob, void *stream);
/* after half of column t: reward [n] (float32, or float64 with reward_f64 != 0: rounded to nearest), done u8 [n] -> 0 / 1.
 * status i32 [n], counts int64[2] and reward_sum double[1] go together: all three, and the step is tallied (counts[0] += the
 * scenes with done != 0, counts[1] += those with status == 2, reward_sum += the sum of (double)reward in the one order of
 * hope_ring_core.h; two launches, the partials are the handle's, so calls belong on one stream), or all NULL: one launch. */
int hope_env_ring_after(hope_env_t *h, const hope_ring_t *ring, int t, const void *reward, int reward_f64, const uint8_t *done,
                        const int32_t *status, int64_t *counts, double *reward_sum, void *stream);
/* a batch of 1 <= batch <= HOPE_RING_MAX_BATCH transitions from the ring's `size` newest columns (1 <= size <= T), the next write
 * going to column `head` (0 <= head < T).  s, j i32 [batch]: the scene and the age (0: the oldest column) of every item -- an item
 * whose s or j is out of range gets zeros and idx = {-1, -1, -1}; both NULL: counter-based draws keyed by (seed, counter, item).
 * last_lidar [n][120], last_target [n][5], last_mask [n][42] float32: the observation after the newest column.  One launch. */
int hope_env_ring_sample(hope_env_t *h, const hope_ring_t *ring, int head, int size, int batch, const int32_t *s, const int32_t *j,
                         uint64_t seed, uint64_t counter, const float *last_lidar, const float *last_target, const float *last_mask,
                         const hope_ring_batch_t *out, void *stream);
/* The same over HOST arrays: pure host code from the same source, no handle, no device; bit-equal to the kernels.  No alignment
 * requirements, no upper bound on n, T or batch.  HOPE_EINVAL for a NULL required pointer, n or T < 1, t / head / size out of
 * range, batch < 1, or a status / counts / reward_sum (s / j) given without the others. */
int hope_ring_before_host(const hope_ring_t *ring, int t, const float *lidar, const float *target, const float *mask,
                          const float *action, const float *log_prob);
int hope_ring_after_host(const hope_ring_t *ring, int t, const void *reward, int reward_f64, const uint8_t *done,
                         const int32_t *status, int64_t *counts, double *reward_sum);
int hope_ring_sample_host(const hope_ring_t *ring, int head, int size, int64_t batch, const int32_t *s, const int32_t *j,
                          uint64_t seed, uint64_t counter, const float *last_lidar, const float *last_target, const float *last_mask,
                          const hope_ring_batch_t *out);

/* ---- PPO's minibatch (additive to ABI 8) ----------------------------------------------------------------------------------------
 * What the inner loop of BatchedPPO.update does around the two network forwards (the reference's PPO.update,
 * src/model/agent/ppo_agent.py:278-336): the gather of a minibatch from the ring by a permutation's indices, and the clipped
 * surrogate, the critic's squared error and their gradients with respect to the networks' outputs and log_std.  Three kernels:
 * k_ppo_gather (a wave per item), k_ppo_loss (a lane per item: its gradients and the chunk's share of the four sums), k_ppo_merge
 * (one wave: the chunk partials' trees).  The sums have one arithmetic order, independent of the launch geometry.  The handle holds
 * the chunk partials only.  Off until enabled; with it off no launch, pointer or output of any other entry point differs.  The rule
 * and the bit-equal host twins: hope_amd/csrc/hope_ppo_core.h, DESIGN.md 5k. */
#define HOPE_PPO_MAX_BATCH 1048576
/* a gathered minibatch: float32, contiguous */
typedef struct hope_ppo_batch_t {
    float *lidar;          /* [mb][120] */
    float *target;         /* [mb][5] */
    float *mask;           /* [mb][42] */
    float *action;         /* [mb][2] */
    float *old_lp;         /* [mb]: the pair of log-probabilities summed */
    float *adv;            /* [mb] */
    float *v_target;       /* [mb] */
    int32_t *idx;          /* [mb]: the flat transition scene * T + column; -1: a refused row */
} hope_ppo_batch_t;
/* allocate the chunk partials (4 x ceil(max_batch / 64) doubles), 1 <= max_batch <= HOPE_PPO_MAX_BATCH.  On an enabled handle a
 * larger max_batch reallocates, an equal or smaller one changes nothing.  Host-synchronous. */
int hope_env_ppo_enable(hope_env_t *h, int max_batch);
/* free them.  Host-synchronous (calls in flight use them). */
int hope_env_ppo_disable(hope_env_t *h);
/* The two calls below are asynchronous on `stream`; they wait for nothing, never synchronise the host and do not join a deferred
 * search.  The structs are HOST memory, read during the call; everything they and the other arguments point to is DEVICE memory,
 * aligned to its element (float32 and int32 4, int64 8 bytes).  HOPE_ESTATE before hope_env_ppo_enable; HOPE_EINVAL for a NULL or
 * misaligned pointer, a number out of range or a clip that is not finite; on any error nothing is launched and the handle stays
 * usable.
 *
 * item b of 1 <= batch <= max_batch takes the ring's flat transition index[b] = scene * T + column (int64 [batch]; the ring as
 * hope_env_ring_*: 1 <= ring->n <= N, 1 <= ring->T <= HOPE_RING_MAX_T): lidar, target, action_mask and action word for word, the two
 * log-probabilities summed, adv and v_target (float32 [n * T], e.g. hope_env_gae's outputs) and the index itself.  An index outside
 * 0 .. n * T - 1 gives a zero row and idx -1.  One launch; with the lidar bases (ring and out) 16-byte and the mask / action bases
 * and the ring's log_prob 8-byte aligned a lane moves 16 / 8 bytes, otherwise 4; the results do not depend on that. */
int hope_env_ppo_gather(hope_env_t *h, const hope_ring_t *ring, const float *adv, const float *v_target, const int64_t *index,
                        int batch, const hope_ppo_batch_t *out, void *stream);
/* the loss of 1 <= mb <= max_batch items and its gradients: raw [mb][2] is the actor's output BEFORE its clamp to [-1, 1],
 * log_std [2], value [mb] the critic's output; action, old_lp, adv and v_target are read from `batch` (its other fields are not
 * used).  clip is finite and >= 0.  Outputs: g_raw [mb][2], g_log_std [2], g_value [mb] -- the gradients of actor loss + critic
 * loss, the seeds of one backward pass through both networks -- and losses [2] = {actor loss, critic loss}.  Two launches, the
 * partials are the handle's, so calls belong on one stream; with raw, action and g_raw 8-byte aligned a lane moves a pair at once;
 * the results do not depend on that. */
int hope_env_ppo_loss(hope_env_t *h, const float *raw, const float *log_std, const float *value, const hope_ppo_batch_t *batch,
                      int mb, double clip, float *g_raw, float *g_log_std, float *g_value, float *losses, void *stream);
/* The same over HOST arrays: pure host code from the same source, no handle, no device; bit-equal to the kernels.  No alignment
 * requirements, no upper bound on n, T, batch or mb.  HOPE_EINVAL for a NULL required pointer, n or T < 1, batch or mb < 1, or a
 * clip that is negative or not finite. */
int hope_ppo_gather_host(const hope_ring_t *ring, const float *adv, const float *v_target, const int64_t *index, int64_t batch,
                         const hope_ppo_batch_t *out);
int hope_ppo_loss_host(const float *raw, const float *log_std, const float *value, const hope_ppo_batch_t *batch, int64_t mb,
                       double clip, float *g_raw, float *g_log_std, float *g_value, float *losses);

/* ---- SAC's update (additive to ABI 8) --------------------------------------------------------------------------------------------
 * What BatchedSAC.update does between its seven network forwards (the reference's SACAgent.update,
 * src/model/agent/sac_agent.py:250-337): the reparameterised sample with its log-probability, the Q target with the two critics'
 * squared errors and their gradients, the gradient of the actor loss at the two critic outputs, and -- from what autograd returns
 * for it at the sampled action -- the gradients of the actor loss at the actor's output and log_std and of the temperature loss at
 * log_alpha.  Kernels: k_sac_sample, k_sac_critic, k_sac_seed, k_sac_policy (a lane per item) and k_sac_merge (one wave: the chunk
 * partials' trees).  The sums have one arithmetic order, independent of the launch geometry.  The handle holds the chunk partials
 * only.  Off until enabled; with it off no launch, pointer or output of any other entry point differs.  The rule and the bit-equal
 * host twins: hope_amd/csrc/hope_sac_core.h, DESIGN.md 5l. */
#define HOPE_SAC_MAX_BATCH 1048576
/* allocate the chunk partials (4 x ceil(max_batch / 64) doubles), 1 <= max_batch <= HOPE_SAC_MAX_BATCH.  On an enabled handle a
 * larger max_batch reallocates, an equal or smaller one changes nothing.  Host-synchronous. */
int hope_env_sac_enable(hope_env_t *h, int max_batch);
/* free them.  Host-synchronous (calls in flight use them). */
int hope_env_sac_disable(hope_env_t *h);
/* The four calls below are asynchronous on `stream`; they wait for nothing, never synchronise the host and do not join a deferred
 * search.  Every pointer is DEVICE memory, float32 and contiguous, aligned to 4 bytes; log_alpha and g_log_alpha are float64 scalars
 * aligned to 8 bytes (the temperature is read on the device).  1 <= batch <= max_batch.  HOPE_ESTATE before hope_env_sac_enable;
 * HOPE_EINVAL for a NULL or misaligned pointer, a batch out of range or a gamma / target_entropy that is not finite; on any error
 * nothing is launched and the handle stays usable.  With the [batch][2] arrays of a call 8-byte aligned a lane moves a pair at
 * once; the results do not depend on that.  The critic and policy calls use the handle's partials, so calls belong on one stream.
 *
 * raw [batch][2] is the actor's output BEFORE its clamp to [-1, 1], log_std [2], eps [batch][2] the standard normal draw:
 * action [batch][2] = clamp(clamp(raw) + exp(log_std) eps), lp [batch] its log-probability summed over the pair.  One launch. */
int hope_env_sac_sample(hope_env_t *h, const float *raw, const float *log_std, const float *eps, int batch, float *action, float *lp,
                        void *stream);
/* q1, q2 [batch]: the critics at the stored action; qt1, qt2 [batch]: the target critics at the sampled next action, next_lp
 * [batch] its log-probability; reward, done [batch].  Outputs: q_target [batch] = reward + (1 - done) gamma (min(qt1, qt2) -
 * alpha next_lp), g_q1, g_q2 [batch] the gradients of the two mean squared errors at q1 and q2, losses [2] the two errors.  Two
 * launches. */
int hope_env_sac_critic(hope_env_t *h, const float *q1, const float *q2, const float *qt1, const float *qt2, const float *next_lp,
                        const float *reward, const float *done, const double *log_alpha, double gamma, int batch, float *q_target,
                        float *g_q1, float *g_q2, float *losses, void *stream);
/* q1, q2 [batch]: the critics at the sampled action.  s1, s2 [batch]: the gradient of -mean(min(q1, q2)) at q1 and q2 (a tie gives
 * half to each).  One launch. */
int hope_env_sac_seed(hope_env_t *h, const float *q1, const float *q2, int batch, float *s1, float *s2, void *stream);
/* raw, log_std, eps as for the sample; q1, q2 as for the seed; g_action [batch][2]: the gradient that the seeds give at the sampled
 * action.  Outputs: g_raw [batch][2] and g_log_std [2], the gradients of the actor loss mean(alpha lp - min(q1, q2)) at raw and
 * log_std; g_log_alpha, the gradient of the temperature loss at log_alpha (float64); losses [2] = {actor loss, temperature loss}.
 * Two launches. */
int hope_env_sac_policy(hope_env_t *h, const float *raw, const float *log_std, const float *eps, const float *q1, const float *q2,
                        const float *g_action, const double *log_alpha, double target_entropy, int batch, float *g_raw,
                        float *g_log_std, double *g_log_alpha, float *losses, void *stream);
/* The same over HOST arrays: pure host code from the same source, no handle, no device; bit-equal to the kernels.  No alignment
 * requirements, no upper bound on batch.  HOPE_EINVAL for a NULL pointer, batch < 1, or a gamma / target_entropy that is not
 * finite. */
int hope_sac_sample_host(const float *raw, const float *log_std, const float *eps, int64_t batch, float *action, float *lp);
int hope_sac_critic_host(const float *q1, const float *q2, const float *qt1, const float *qt2, const float *next_lp,
                         const float *reward, const float *done, const double *log_alpha, double gamma, int64_t batch,
                         float *q_target, float *g_q1, float *g_q2, float *losses);
int hope_sac_seed_host(const float *q1, const float *q2, int64_t batch, float *s1, float *s2);
int hope_sac_policy_host(const float *raw, const float *log_std, const float *eps, const float *q1, const float *q2,
                         const float *g_action, const double *log_alpha, double target_entropy, int64_t batch, float *g_raw,
                         float *g_log_std, double *g_log_alpha, float *losses);

/* ---- the policy's inference forward (additive to ABI 8) ----------------------------------------------------------------------------
 * HopeNet's forward (hope_amd/policy.py; the reference's MultiObsEmbedding with the attention trunk, src/model/network.py:34-187)
 * for the reference's configuration as ONE kernel, k_policy_forward: embed 128, two-layer embedding MLPs with tanh, one pre-norm
 * encoder layer (8 heads x 32, bias-free qkv, a 128-wide token MLP), a (n_tokens x 128) -> 128 -> out_dim head.  n_tokens = 3
 * (lidar 120, target 5, action mask 42) or 4: the fourth token is handed in ready-made as [batch][128] (the image encoder's
 * convolutions and re_embed_img stay with the caller).  out_dim 1 or 2, the output tanh on or off, so a PPO critic runs through
 * the same code.  Every Linear is a k-ascending float32 fmaf chain from its bias (the f32-input matrix instruction), everything
 * else float64 rounded once; the order is fixed in hope_amd/csrc/hope_policy_core.h, so the host twin below gives the same bits.
 * A row's result depends on that row only.  Off until enabled; with it off no launch, pointer or output of any other entry point
 * differs.  DESIGN.md 5m. */
#define HOPE_POLICY_MAX_BATCH 1048576
/* the float32 parameter tensors as torch holds them, [out][in] row-major and contiguous */
typedef struct hope_policy_params {
    const float *lidar_w1, *lidar_b1, *lidar_w2, *lidar_b2;      /* embed_lidar.0 [128][120], [128]; embed_lidar.2 [128][128], [128] */
    const float *target_w1, *target_b1, *target_w2, *target_b2;  /* embed_tgt.0 [128][5], .2 */
    const float *mask_w1, *mask_b1, *mask_w2, *mask_b2;          /* embed_am.0 [128][42], .2 */
    const float *ln1_g, *ln1_b;                                  /* net.encoder.layers.0.0.norm [128] */
    const float *qkv_w;                                          /* ...layers.0.0.fn.to_qkv [768][128], no bias */
    const float *out_w, *out_b;                                  /* ...layers.0.0.fn.to_out.0 [128][256], [128] */
    const float *ln2_g, *ln2_b;                                  /* ...layers.0.1.norm [128] */
    const float *ff1_w, *ff1_b, *ff2_w, *ff2_b;                  /* ...layers.0.1.fn.net.0 and .3 [128][128], [128] */
    const float *head1_w, *head1_b;                              /* net.output.0 [128][n_tokens * 128], [128] */
    const float *head2_w, *head2_b;                              /* net.output.2 [out_dim][128], [out_dim] */
} hope_policy_params_t;
/* allocate the packed parameter buffer for this shape.  n_tokens 3 or 4, out_dim 1 or 2, tanh_out 0 or 1, 1 <= max_batch <=
 * HOPE_POLICY_MAX_BATCH, anything else HOPE_EINVAL.  Enabling again with the same shape keeps the loaded parameters and takes the
 * larger max_batch; another shape drops them (a load must follow).  Host-synchronous. */
int hope_env_policy_enable(hope_env_t *h, int n_tokens, int out_dim, int tanh_out, int max_batch);
/* free it.  Host-synchronous (calls in flight use it). */
int hope_env_policy_disable(hope_env_t *h);
/* p: a HOST struct of DEVICE pointers, each aligned to 4 bytes.  k_policy_pack copies the tensors into the handle's buffer, in the
 * layout that the forward loads coalesced: one launch on `stream`, no host synchronisation; the tensors must stay unchanged until
 * it has run.  HOPE_ESTATE before the enable; HOPE_EINVAL for a NULL struct or a NULL or misaligned tensor (nothing is launched, the
 * buffer keeps what it had). */
int hope_env_policy_load(hope_env_t *h, const hope_policy_params_t *p, void *stream);
/* lidar [batch][120], target [batch][5], mask [batch][42], img_token [batch][128] (n_tokens 4) or NULL (n_tokens 3), out
 * [batch][out_dim]: DEVICE memory, float32, contiguous, aligned to 4 bytes.  One launch on `stream` (ceil(batch / 32) workgroups),
 * no host synchronisation.  HOPE_ESTATE before the enable or before the first load; HOPE_EINVAL for a NULL or misaligned pointer,
 * a batch outside 1 .. max_batch, or an image token that does not go with n_tokens; on any error nothing is launched. */
int hope_env_policy_forward(hope_env_t *h, const float *lidar, const float *target, const float *mask, const float *img_token,
                            int batch, float *out, void *stream);
/* The same over HOST arrays and a struct of HOST pointers: pure host code from the same source, no handle, no device; bit-equal
 * to the kernel.  No alignment requirements, no upper bound on batch.  HOPE_EINVAL for a NULL pointer, a shape as above, batch < 1. */
int hope_policy_forward_host(const hope_policy_params_t *host_params, int n_tokens, int out_dim, int tanh_out, const float *lidar,
                             const float *target, const float *mask, const float *img_token, int64_t batch, float *out);

/* ---- the image encoder's inference forward (additive to ABI 8) ------------------------------------------------------------------
 * HopeNet's image token (hope_amd/policy.py _ImgEncoder and re_embed_img; the reference's ImgEncoder / ConvBlock,
 * src/model/network.py:198-299) for img_shape (3, 64, 64), img_conv_layers [4, 8], k_img_conv 3, img_linear_layers [256], embed
 * 128, as two kernels: k_imgenc_conv (uint8 images -> the 2 048 features behind the two convolution blocks, a workgroup per image,
 * VALU) and k_imgenc_head (fc1 -> act -> output_mean -> tanh -> re_embed_img.1 on the f32-input matrix instruction, 32 images per
 * workgroup).  act: 0 tanh, 1 LeakyReLU(0.01).  Every convolution and Linear output is one float32 fmaf chain from its bias in a
 * fixed order, everything else float64 rounded once; the order is fixed in hope_amd/csrc/hope_imgenc_core.h, so the host twin below
 * gives the same bits.  An image's result depends on that image only.  Independent of the policy forward above: enabling one leaves
 * the other as it was.  Off until enabled; with it off no launch, pointer or output of any other entry point differs.  DESIGN.md 5n. */
#define HOPE_IMGENC_MAX_BATCH 262144
/* the float32 parameter tensors as torch holds them, row-major and contiguous */
typedef struct hope_imgenc_params {
    const float *conv1_w, *conv1_b;      /* embed_img.net.0.layer.0 [4][3][3][3], [4] */
    const float *short1_w, *short1_b;    /* embed_img.net.0.shortcut.0 [4][3][1][1], [4] */
    const float *conv2_w, *conv2_b;      /* embed_img.net.1.layer.0 [8][4][3][3], [8] */
    const float *short2_w, *short2_b;    /* embed_img.net.1.shortcut.0 [8][4][1][1], [8] */
    const float *fc1_w, *fc1_b;          /* embed_img.net.3 [256][2048], [256] */
    const float *mean_w, *mean_b;        /* embed_img.output_mean [128][256], [128] */
    const float *re_w, *re_b;            /* re_embed_img.1 [128][128], [128] */
} hope_imgenc_params_t;
/* allocate the packed parameter buffer and the feature buffer [max_batch][2048] float32 (8 KiB per image).  act 0 or 1, 1 <=
 * max_batch <= HOPE_IMGENC_MAX_BATCH, anything else HOPE_EINVAL.  Enabling again keeps the loaded parameters (the packed
 * words do not depend on act) and takes the new act; a larger max_batch reallocates the feature buffer (host-synchronous). */
int hope_env_imgenc_enable(hope_env_t *h, int act, int max_batch);
/* free both.  Host-synchronous (calls in flight use them). */
int hope_env_imgenc_disable(hope_env_t *h);
/* p: a HOST struct of DEVICE pointers, each aligned to 4 bytes.  k_imgenc_pack copies the tensors into the handle's buffer (the
 * convolutions as they are, the three Linear weights [k][out]): one launch on `stream`, no host synchronisation; the tensors must
 * stay unchanged until it has run.  HOPE_ESTATE before the enable; HOPE_EINVAL for a NULL struct or a NULL or misaligned tensor
 * (nothing is launched, the buffer keeps what it had). */
int hope_env_imgenc_load(hope_env_t *h, const hope_imgenc_params_t *p, void *stream);
/* img [batch][3][64][64] uint8, token [batch][128] float32, feat NULL or [batch][2048] float32 (the features, for tests that
 * localise a difference; NULL: they stay in the handle's buffer): DEVICE memory, contiguous, aligned to 4 bytes.  Two launches on
 * `stream`, no host synchronisation; calls share the handle's feature buffer, so they belong on one stream.  HOPE_ESTATE before the
 * enable or before the first load; HOPE_EINVAL for a NULL or misaligned pointer or a batch outside 1 .. max_batch; on any error
 * nothing is launched and nothing written. */
int hope_env_imgenc_forward(hope_env_t *h, const uint8_t *img, int64_t batch, float *token, float *feat_or_null, void *stream);
/* one of the two kernels alone, for timing (tools/img_encoder_bench.py): stage 0 k_imgenc_conv (img -> feat; token unused), stage 1
 * k_imgenc_head (feat -> token; img unused).  feat is required.  Checks and errors as hope_env_imgenc_forward. */
int hope_debug_imgenc_stage(hope_env_t *h, int stage, const uint8_t *img, int64_t batch, float *token, float *feat, void *stream);
/* The same over HOST arrays and a struct of HOST pointers: pure host code from the same source, no handle, no device; bit-equal
 * to the kernels.  No upper bound on batch.  HOPE_EINVAL for a NULL pointer (feat_or_null may be NULL), an act that is not 0 or 1,
 * batch < 1, or img / token / feat not aligned to 4 bytes. */
int hope_imgenc_forward_host(const hope_imgenc_params_t *host_params, int act, const uint8_t *img, int64_t batch, float *token,
                             float *feat_or_null);

/* ---- the critics' inference forward (additive to ABI 8) -------------------------------------------------------------------------
 * The no-gradient forward of up to HOPE_CRITIC_SLOTS critic HopeNets (hope_amd/policy.py: a HopeNet with one linear output, or a
 * SacCritic; the reference's SACCriticAdapter, src/model/agent/sac_agent.py:15-30) over ONE set of inputs as ONE kernel,
 * k_critic_forward: the policy forward's network with T = 3 + has_img + has_action tokens in HopeNet.tokens' order -- lidar, target,
 * mask, [the image token, ready-made, one per net: each critic has its own encoder, which stays with the caller], [action [batch][2]
 * through embed_action] -- a (T x 128) -> 128 -> 1 head and no output tanh.  The handle keeps n_slots packed parameter sets of one
 * shape, so that SAC's two target critics, or PPO's critic and its target, are evaluated by one launch without re-packing in turn.
 * The arithmetic is the policy forward's rule extended to the action token (hope_amd/csrc/hope_critic_core.h), so the host twin below
 * gives the same bits, and without an action token the bits of hope_policy_forward_host(..., out_dim 1, tanh_out 0).  A row's result
 * depends on that row and that net only.  Independent of the policy forward and the image encoder above: enabling one leaves the
 * others as they were.  Off until enabled; with it off no launch, pointer or output of any other entry point differs.  DESIGN.md 5o. */
#define HOPE_CRITIC_SLOTS 4
/* the float32 parameter tensors as torch holds them, [out][in] row-major and contiguous: hope_policy_params_t's fields (head2 is
 * [1][128], [1]), then the action embedding, all four NULL exactly when has_action is 0 */
typedef struct hope_critic_params {
    const float *lidar_w1, *lidar_b1, *lidar_w2, *lidar_b2;
    const float *target_w1, *target_b1, *target_w2, *target_b2;
    const float *mask_w1, *mask_b1, *mask_w2, *mask_b2;
    const float *ln1_g, *ln1_b;
    const float *qkv_w;
    const float *out_w, *out_b;
    const float *ln2_g, *ln2_b;
    const float *ff1_w, *ff1_b, *ff2_w, *ff2_b;
    const float *head1_w, *head1_b;                              /* net.output.0 [128][T * 128], [128] */
    const float *head2_w, *head2_b;                              /* net.output.2 [1][128], [1] */
    const float *action_w1, *action_b1, *action_w2, *action_b2;  /* embed_action.0 [128][2], [128]; embed_action.2 [128][128], [128] */
} hope_critic_params_t;
/* allocate n_slots packed parameter sets of this shape.  1 <= n_slots <= HOPE_CRITIC_SLOTS, has_img and has_action 0 or 1, 1 <=
 * max_batch <= HOPE_POLICY_MAX_BATCH, anything else HOPE_EINVAL.  Enabling again with the same n_slots and shape keeps the loaded
 * slots and takes the larger max_batch; anything else drops them (loads must follow).  Host-synchronous. */
int hope_env_critic_enable(hope_env_t *h, int n_slots, int has_img, int has_action, int max_batch);
/* free them.  Host-synchronous (calls in flight use them). */
int hope_env_critic_disable(hope_env_t *h);
/* p: a HOST struct of DEVICE pointers, each aligned to 4 bytes.  k_critic_pack copies the tensors into slot `slot`, in the layout that
 * the forward loads coalesced: one launch on `stream`, no host synchronisation; the tensors must stay unchanged until it has run.
 * HOPE_ESTATE before the enable; HOPE_EINVAL for a slot outside 0 .. n_slots - 1, a NULL struct, a NULL or misaligned tensor, or
 * action tensors that do not go with has_action (nothing is launched, the slot keeps what it had). */
int hope_env_critic_load(hope_env_t *h, int slot, const hope_critic_params_t *p, void *stream);
/* slots: HOST const int[n], 1 <= n <= n_slots, each loaded, no slot twice.  lidar [batch][120], target [batch][5], mask [batch][42],
 * img_token [n][batch][128] (has_img; token i for net slots[i]) or NULL, action [batch][2] (has_action) or NULL, out [n][batch]:
 * DEVICE memory, float32, contiguous, aligned to 4 bytes.  One launch on `stream` (a grid of ceil(batch / 32) x n workgroups), no
 * host synchronisation.  HOPE_ESTATE before the enable or before the load of a slot that is used; HOPE_EINVAL for a NULL `slots`, an
 * n, a slot or a batch out of range, a slot named twice, a NULL or misaligned pointer, or an image token or action that does not
 * go with the shape; on any error nothing is launched. */
int hope_env_critic_forward(hope_env_t *h, const int *slots, int n, const float *lidar, const float *target, const float *mask,
                            const float *img_token, const float *action, int batch, float *out, void *stream);
/* One net over HOST arrays and a struct of HOST pointers: pure host code from the same source, no handle, no device; bit-equal to
 * the kernel.  img_token [batch][128] or NULL, action [batch][2] or NULL, out [batch].  No alignment requirements, no upper bound
 * on batch.  HOPE_EINVAL for a NULL pointer, has_img / has_action not 0 or 1, an image token, action or action tensors that do not
 * go with them, batch < 1. */
int hope_critic_forward_host(const hope_critic_params_t *host_params, int has_img, int has_action, const float *lidar,
                             const float *target, const float *mask, const float *img_token, const float *action, int64_t batch,
                             float *out);

/* ---- the optimiser block (additive to ABI 8) ----------------------------------------------------------------------------------
 * What an update does after backward, for many tensors at once: Adam's step (torch.optim.Adam without amsgrad, weight decay or
 * maximize) and the Polyak average of a target network (agents._soft_update; the reference's AgentBase._soft_update,
 * src/model/agent/agent_base.py:64).  One kernel, k_optim, in two modes; a launch covers up to HOPE_OPTIM_CAP tensors, a workgroup
 * HOPE_OPTIM_CHUNK elements of one of them, and the entry table travels as the kernel's argument.  The arithmetic is ONE rule
 * (hope_amd/csrc/hope_optim_core.h: every operation a double operation, no fused multiply-add, each stored word rounded once), so
 * the host twins below give the same bits; against torch's own Adam the difference is rounding, measured in DESIGN.md 5p.  The calls
 * keep no state in the handle: there is nothing to enable, and with them unused no launch, pointer or output of any other entry
 * point differs. */
#define HOPE_OPTIM_F32 0
#define HOPE_OPTIM_F64 1
#define HOPE_OPTIM_MAX_GROUPS 4
#define HOPE_OPTIM_CAP 64         /* entries per launch; a call with more becomes several launches, back to back on the stream */
#define HOPE_OPTIM_CHUNK 1024
/* one tensor of a call: contiguous, `numel` elements of float32 (HOPE_OPTIM_F32) or float64 (HOPE_OPTIM_F64), every pointer aligned
 * to its element (16-byte alignment of all of an entry's pointers buys 16-byte accesses, nothing else).  Adam: p the parameter, g its
 * gradient, m exp_avg, v exp_avg_sq, group the index into the call's groups; p, m and v are updated in place.  Polyak: p the TARGET
 * tensor, updated in place, g the current net's tensor; m, v and group are not looked at.  No two entries of a call may overlap. */
typedef struct hope_optim_entry {
    void *p;
    const void *g;
    void *m;
    void *v;
    int64_t numel;
    int32_t group;
    int32_t dtype;
} hope_optim_entry_t;
/* a parameter group's step, from its lr, (beta1, beta2), eps and the step count t >= 1 this call is:
 * c1 = 1 - beta1, b2 = beta2, c2 = 1 - beta2, step_size = lr / (1 - beta1^t), bc2s = sqrt(1 - beta2^t), eps */
typedef struct hope_optim_group {
    double c1;
    double b2;
    double c2;
    double step_size;
    double bc2s;
    double eps;
} hope_optim_group_t;
/* entries: a HOST table of DEVICE pointers, n_entries >= 1; groups: a HOST table, 1 <= n_groups <= HOPE_OPTIM_MAX_GROUPS.  Both are
 * read before the call returns (nothing is staged: gradients may live elsewhere at the next call).  ceil(n_entries / HOPE_OPTIM_CAP)
 * launches on `stream`, no host synchronisation.  HOPE_EINVAL, with a text that names the entry or group, nothing launched and
 * nothing written, for: a NULL table or a NULL pointer in an entry; n_entries < 1, a numel < 1 or more than 2^31 elements in all; a
 * pointer not aligned to its element; a group index out of range or n_groups outside 1 .. 4; a dtype that is neither value; a
 * hyper-parameter that is not finite, eps < 0 or bc2s <= 0. */
int hope_env_optim_adam(hope_env_t *h, const hope_optim_entry_t *entries, int n_entries, const hope_optim_group_t *groups, int n_groups,
                        void *stream);
/* target <- (1 - tau) * target + tau * current for every entry.  As above; HOPE_EINVAL also for a tau outside [0, 1]. */
int hope_env_optim_polyak(hope_env_t *h, const hope_optim_entry_t *entries, int n_entries, double tau, void *stream);
/* The same over HOST pointers: pure host code from the same source, no handle, no device; bit-equal to the kernel.  The same
 * refusals. */
int hope_optim_adam_host(const hope_optim_entry_t *entries, int n_entries, const hope_optim_group_t *groups, int n_groups);
int hope_optim_polyak_host(const hope_optim_entry_t *entries, int n_entries, double tau);

/* ---- introspection ---------------------------------------------------------------------------- */
int hope_env_num_scenes(const hope_env_t *h);
int hope_env_max_obstacles(const hope_env_t *h);
/* name of the device the handle runs on (e.g. "gfx950"), static storage */
const char *hope_env_device_arch(const hope_env_t *h);

#ifdef __cplusplus
}
#endif
#endif /* HOPE_ENV_H */
