// hope_handle.h -- the handle behind hope_env_t and the opening every hope_env_* entry point shares.  Private to the library's own
// .hip files (hope_env.hip: create / destroy, step, pool, curriculum, debug; hope_agent.hip: planner, chooser, normalisation, evaluation, advantages, transition ring, PPO's minibatch, SAC's update, the optimiser block; hope_policy.hip: the fused policy forward, the image encoder, the critics' forward).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "hope_env.h"
#include "hope_internal.h"
#include "hope_curriculum_core.h"
#include "hope_evaltrack_core.h"

namespace hope {

// hope_last_error's text (thread-local, hope_env.hip); returns `code`
int fail(int code, const std::string& msg);
// Live handles (the registry is hope_env.hip's): a pointer that is not, or no longer, a handle fails with HOPE_EINVAL instead of
// touching freed memory (a ~50 ns set lookup per call next to ~15 launches).
bool is_live(const void* h);

// every entry point runs on the handle's device and puts the caller's current device back (a process that drives
// several GPUs keeps PyTorch's notion of the current device)
struct DeviceGuard {
    int prev = -1;
    bool ok = true;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) ok = hipSetDevice(dev) == hipSuccess; else prev = -1;
    }
    ~DeviceGuard() { if (prev >= 0) hipSetDevice(prev); }
};

}  // namespace hope

#define HIPCHK(expr)                                                                              \
    do {                                                                                          \
        hipError_t e_ = (expr);                                                                   \
        if (e_ != hipSuccess)                                                                     \
            return hope::fail(HOPE_EHIP, std::string(#expr) + ": " + hipGetErrorString(e_));      \
    } while (0)

// ---- the opening of an entry point `name` (a string literal) ----
// HOPE_ENTER: the null and liveness checks, before anything else reads the handle.  (_AS: entries whose null-handle text is another.)
#define HOPE_NOT_LIVE(name, hint) name ": not a live handle (" hint ")"
#define HOPE_ENTER_AS(h, name, null_text)                                                                        \
    do {                                                                                                         \
        if (!(h)) return hope::fail(HOPE_EINVAL, name ": " null_text);                                           \
        if (!hope::is_live(h)) return hope::fail(HOPE_EINVAL, HOPE_NOT_LIVE(name, "destroyed?"));                \
    } while (0)
#define HOPE_ENTER(h, name) HOPE_ENTER_AS(h, name, "null handle")
// HOPE_NEED: a feature that must be on / a call that must have come first
#define HOPE_NEED(cond, name, text) do { if (!(cond)) return hope::fail(HOPE_ESTATE, name ": " text); } while (0)
// HOPE_ON_DEVICE: the rest of the function runs on the handle's device (`guard`).  (_AS: the calls that take a device id.)
#define HOPE_ON_DEVICE_AS(dev, code, prefix) hope::DeviceGuard guard(dev); if (!guard.ok) return hope::fail(code, prefix "hipSetDevice failed")
#define HOPE_ON_DEVICE(h) HOPE_ON_DEVICE_AS((h)->device, HOPE_EHIP, "")

using hope::CwDev; using hope::DlpCases; using hope::StepCold;   // (hope_internal.h)

// Stream roles of a step's launch structure.  The numbers are those hope_env_queue_check reports (include/hope_env.h).
enum Role {
    ROLE_CALLER = 0,      // the caller's stream
    ROLE_CHAIN = 1,       // the second chain (small-tile class): all of it, or its search launches in a pipelined step
    ROLE_IMAGE = 2,       // the image (joined steps) / the static-layer rebuild next to it (pipelined steps)
    ROLE_OBS_LARGE = 3,   // observation half of the first chain (large-tile class)
    ROLE_OBS_SMALL = 4,   // observation half of the second chain (small-tile class)
    ROLE_SEARCH0 = 5,     // search launches of the first chain in a pipelined step
    ROLE_SPARE = 6,       // created, never used: the runtime spreads streams over hardware queues in creation order
    ROLE_OBS_SUB = 7,     // observation half of the second sub-chain of a single-class batch
    N_ROLES = 8
};

struct hope_env {
    int n = 0, max_obst = 0, device = 0;
    uint32_t flags = 0;
    uint32_t profile_mask = ~0u;   // HOPE_F_PROFILE: kernels (bit = HOPE_K_*) whose launches are bracketed by events
    bool have_tables = false, have_scenes = false;
    char arch[64] = {0};
    // device memory
    double* verts = nullptr;
    int32_t* n_obst = nullptr;
    double* scene_c = nullptr;
    double* state = nullptr;
    double* cs = nullptr;         // [n][2] cos / sin of state's heading (motion launch -> observation launch)
    int32_t* tstep = nullptr;
    double* tab = nullptr;
    double* pmax = nullptr;
    uint16_t* mask_lut = nullptr;   // count-interval table of the action mask's coarse beams (MASK_LUT_*, hope_step_kernel.h)
    double* mask_bsc = nullptr;     // [NBEAM] bins per metre of every coarse beam's table
    double* hull_base = nullptr;
    double* beam_ab = nullptr;
    int32_t* rs_count = nullptr;
    int32_t* rs_list = nullptr;
    double* rs_in = nullptr;      // [2 n][RS_IN_WORDS] search inputs by queue position (k_rs_compact -> k_rs_words / k_rs_segs)
    uint8_t* rs_flag = nullptr;
    double* kin = nullptr;
    double* post = nullptr;        // [n][POST_WORDS] k_env_step -> k_post hand-over
    double* traj = nullptr;        // HOPE_F_IMAGE: [n][20][3] ring of vehicle.trajectory
    int32_t* traj_len = nullptr;   // HOPE_F_IMAGE: [n] len(vehicle.trajectory)
    int32_t* traj_valid = nullptr; // HOPE_F_IMAGE: [n] entries below this index have span tables in bev_scratch
    int32_t* layer_valid = nullptr; // HOPE_F_IMAGE: [n] the static image layer (obstacles, start outline, dest) matches the scene's map
    uint8_t* bev_layer = nullptr;   // HOPE_F_IMAGE: [n][64 KiB] the static layer, 2 bits per pixel, tiled
    uint8_t* bev_dyn = nullptr;     // HOPE_F_IMAGE: [n][256 KiB] the trajectory layer, one byte per pixel, tiled
    int32_t* bev_list = nullptr;    // HOPE_F_IMAGE: [1 + n] count + scenes whose layer must be rebuilt this step
    int32_t* bev_legacy = nullptr;  // HOPE_F_IMAGE: [1 + n] count + scenes for the per-tile raster launch of k_bev_image
    int* bev_scratch = nullptr;    // HOPE_F_IMAGE: [n][BEV_SCENE_INTS]
    // per tile class (0: n_obst <= SMALL_TILE, 1: larger) dense scene lists; classes are static between set_scenes calls
    int32_t* cls_list[2] = {nullptr, nullptr};
    int cls_count[2] = {0, 0};
    std::vector<int32_t> cls_list_host[2];       // the same lists on the host (hope_env_step_plan)
    std::vector<int32_t> n_obst_host;
    std::vector<uint8_t> slot_cls_host;          // draw / launch class of every scene slot (0: <= 32 obstacles, 1: larger lots)
    uint8_t* slot_cls = nullptr;                 // the same on the device
    double* rs_rec = nullptr;
    int32_t* rs_surv_count = nullptr;            // [MAX_CHAIN] two-kernel validation: searches k_rs_screen left a word of, per chain
    int2* rs_surv = nullptr;                     // [2 n] (queue index, queue entry), laid out like rs_list
    uint8_t* active_snap = nullptr; // [n] the caller's `active` mask as the motion launch saw it (read by k_rs_compact, HOPE_DEFER_RS)
    // StepCold (rarely used kernel parameters) in device memory: a ring of immutable versions, uploaded stream-ordered on change
    static constexpr int COLD_RING = 8;
    StepCold* cold_dev = nullptr;   // [COLD_RING]
    StepCold* cold_host = nullptr;  // [COLD_RING] pinned
    hipEvent_t cold_ev[COLD_RING] = {};
    int cold_idx = -1;
    StepCold cold_last;
    uint64_t pool_generation = 0;   // bumped by every change of what a draw can return (pool commit / upload, Dragon-Lake cases)
    uint64_t redraw_seed = 0;       // HOPE_AUTO_REDRAW
    float4* obb = nullptr;          // [n][max_obst] obstacle boxes (xmin, xmax, ymin, ymax), float32 rounded outwards
    float4* fverts = nullptr;       // [n][max_obst][2] float32 view of the obstacles relative to (map box xmin, ymin): obstacle_f32
    float4* fbox = nullptr;         // [n][max_obst]
    uint8_t* eflag = nullptr;       // [n][eflag_stride(max_obst)]
    // staging for set_scenes
    void* stage = nullptr;
    size_t stage_bytes = 0;
    // HOPE_F_PROFILE: event pairs recorded on the launch stream, drained by hope_env_kernel_ms
    struct EvPair { hipEvent_t a, b; int kind; uint64_t seq; };   // seq: the hope_env_step / reset_obs call the launch belongs to
    uint64_t step_seq = 0;
    double union_ms[HOPE_N_KERNELS] = {};       // per kernel: time during which >= 1 launch of a call was running
    int64_t union_calls[HOPE_N_KERNELS] = {};
    std::vector<EvPair> pending;
    std::vector<hipEvent_t> free_events;
    double ms[HOPE_N_KERNELS] = {};
    int64_t launches[HOPE_N_KERNELS] = {};
    // scene pool (hope_env_set_pool): complete scenes resident in HBM; hope_env_redraw copies one into a finished slot
    int pool_n = 0;
    double* pool_verts = nullptr;   // [pool_n][max_obst][8]
    double* pool_c = nullptr;       // [pool_n][SC_WORDS]
    int32_t* pool_nobst = nullptr;  // [pool_n]
    // double-buffered storage behind the pointers above: a new pool is uploaded (asynchronously, from pinned staging) into the
    // set the step kernels are NOT reading and swapped in by stream order (hope_env_pool_staging / hope_env_commit_pool)
    struct PoolSet { double* verts = nullptr; double* c = nullptr; int32_t* nobst = nullptr; int32_t* list[2] = {nullptr, nullptr}; int cap = 0, list_cap = 0;
                     // curriculum labels of the set's entries (device table: written while the curriculum is on)
                     uint8_t* label = nullptr;
                     int n_pool = 0, npool_cls[2] = {0, 0};    // entries, and the pool entries (without the cases) at the head of list[c]
                     int lab_kind = 0;                         // 0: all unlabelled, 1: generated (gen_counts lots per level, in order), 2: lab_host
                     int gen_counts[3] = {0, 0, 0};
                     std::vector<uint8_t> lab_host;            // hope_env_set_pool_buckets
                     int32_t* sorted_own[2] = {nullptr, nullptr}; int sorted_own_cap = 0; };   // lab_kind 2: list[c]'s pool entries ordered by label
    PoolSet pset[2];
    int pactive = -1;
    struct PoolStage { double* start = nullptr; double* dest = nullptr; double* bbox = nullptr; double* verts = nullptr; int32_t* nobst = nullptr;
                       int32_t* list = nullptr; int cap = 0; bool busy = false;
                       bool staged = false; };   // staged: handed out by hope_env_pool_staging, not committed yet
    PoolStage pstage;                            // pinned host memory
    double* pstage_dev = nullptr;                // device staging of start | dest | bbox
    // hope_env_generate_pool: n_obst of a generated set travels back through the set's own pinned array, asynchronously on pool_stream;
    // pool_nobst_host takes it over lazily, when somebody needs it (settle_gen_nobst: refresh_pool_lists_sync), so that no call
    // waits for the generator.  gen_host_set: the ACTIVE set if its host copy is still outstanding, else -1.
    int32_t* gen_nobst[2] = {nullptr, nullptr};
    int gen_nobst_cap[2] = {0, 0}, gen_nobst_n[2] = {0, 0};
    hipEvent_t ev_gen_copied[2] = {nullptr, nullptr};
    int gen_host_set = -1;
    int pstage_dev_cap = 0;
    hipStream_t pool_stream = nullptr;
    hipEvent_t ev_pool_ready = nullptr, ev_pool_copied = nullptr, ev_last_step = nullptr;
    bool pool_wait_pending = false;
    // hope_env_commit_pool_relaxed: the uploaded set takes over once ev_pool_ready has passed (apply_pending_pool)
    struct PendingPool { bool on = false, generated = false; int set = 0, n_pool = 0, cls_n[2] = {0, 0}; uint64_t content = 0; std::vector<int32_t> nobst_host; } pend;
    int32_t* pool_cls[2] = {nullptr, nullptr};   // pool entries of each tile class
    int pool_cls_n[2] = {0, 0};
    std::vector<int32_t> pool_nobst_host;        // n_obst of the pool's complete scenes (class lists are rebuilt from it)
    // Dragon-Lake-Parking cases drawn on the device (hope_env_set_dlp_cases)
    DlpCases dlp = {};
    void* dlp_mem[6] = {};
    int32_t* pool_overflow = nullptr;            // [1] device counter: draws truncated to max_obst obstacles
    int32_t* cur_pool = nullptr;    // [n] pool entry a scene currently holds (-1: uploaded by set_scenes; -1 - c... see hope_env.h)
    uint32_t* episode = nullptr;    // [n] redraw counter (part of the draw's hash)
    // HOPE_F_OVERLAP: the two tile classes' launches go to library streams, one per role (fork / join with events)
    static constexpr int MAX_CHAIN = 2;                     // launch chains of a step: one per tile class, or two sub-chains of one class
    hipStream_t side[N_ROLES] = {};                         // stream of each role ([ROLE_CALLER] unused: the caller's stream)
    hipEvent_t ev_fork = nullptr, ev_step[MAX_CHAIN] = {}, ev_segs[MAX_CHAIN] = {}, ev_post[MAX_CHAIN] = {};
    hipEvent_t ev_chain1_done = nullptr, ev_image_done = nullptr, ev_obs_done[MAX_CHAIN] = {}, ev_search0_done = nullptr;
    hipEvent_t ev_collect = nullptr;                        // round 6: ONE join point for the caller's stream (the library stream of the other chain's observation collects the rest)
    bool last_via_steps = false;                            // the last step recorded ev_step[0 / 1] behind both motion launches (the pool's only readers)
    hipEvent_t ev_bev[2] = {};                              // image: fork / join of the static-layer rebuild next to k_bev_prep
    int rs_parity = 0;                                      // which of the two queue counters of a chain this step uses (pipelined steps)
    int queue_of_role[N_ROLES] = {-1, -1, -1, -1, -1, -1, -1, -1};   // measured hardware-queue class of role r's stream ([0]: the NULL stream)
    int n_queues = 0;
    double queue_check_ms = 0.0;
    // curriculum for new-map draws (hope_curriculum_kernel.h): device tally + weighted draw lists, double-buffered like the pool sets
    struct Curriculum {
        bool on = false;
        hope_curriculum_params P = {};
        int n_cases = 0, nb = 0;
        void* mem = nullptr;                                // the arrays of `dev`
        CwDev dev = {};
        uint8_t* scene_bucket = nullptr;                    // [n] bucket of the map a scene holds
        uint32_t* noted_ep = nullptr;                       // [n] the scene's redraw counter when that bucket was noted
        int32_t* wl[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}};   // [buffer][class][CW_LIST_LEN]
        int32_t* prefix[2] = {nullptr, nullptr};            // [buffer][2][CW_MAX_GROUPS + 1]
        int wactive = -1;                                   // buffer the next step reads
        CwClass cls[2] = {};                                // what the active buffer's lists are made of
        uint64_t updates = 0;
        hipEvent_t ev_order = nullptr;
    } cur;
    int draw_set = -1;                                      // pool set the last step / hope_env_redraw drew from
    // replay of found Reeds-Shepp paths (hope_planner_kernel.h): [PL_WORDS][n] state words, nullptr while the planner is off
    struct Planner { bool on = false; double step_ratio = HOPE_PLAN_STEP_RATIO; uint64_t* state = nullptr; } plan;
    // masked choice of the discrete action (hope_chooser_kernel.h): the [42][2] action table, nullptr while the chooser is off
    struct Chooser { bool on = false; double* actions = nullptr; } choose;
    // normalisation of the observations (hope_obsnorm_kernel.h): state = mean | S | std ([3][125] doubles), part = the chunk partials
    // ([125][3][stride]); n_state lives here, on the host, and reaches the kernels as an argument
    struct ObsNorm { bool on = false; int64_t n_state = 0; long long stride = 0; double* state = nullptr; double* part = nullptr; } onorm;
    // bookkeeping of an evaluation run (hope_evaltrack_kernel.h): [ET_WORDS][n] state words, nullptr while it is off; the action box
    // of the stuck detector's draw reaches k_eval_override as an argument
    struct EvalTrack { bool on = false; EtBox box = {}; uint64_t* state = nullptr; } evalt;
    // PPO's advantage block (hope_gae_kernel.h): part = the chunk partials of the two sums ([2][chunks of the call], room for
    // ceil(n / 64) chunks), sums = the handle's own {sum adv, sum adv^2, count}
    struct Gae { bool on = false; double* part = nullptr; double* sums = nullptr; } gae;
    // the transition ring (hope_ring_kernel.h): the chunk partials of a step's tally, part = the reward sums ([chunks]) and cnt = the
    // done / success counts ([chunks][2]), room for ceil(n / 64) chunks; the ring's tensors and the totals are the caller's
    struct Ring { bool on = false; double* part = nullptr; int32_t* cnt = nullptr; } ring;
    // PPO's minibatch (hope_ppo_kernel.h): part = the chunk partials of the loss call's four sums ([4][chunks of the call], room for
    // ceil(max_batch / 64) chunks)
    struct Ppo { bool on = false; double* part = nullptr; int max_batch = 0; } ppo;
    // SAC's update (hope_sac_kernel.h): part = the chunk partials of the critic call's two sums and the policy call's four ([4][chunks
    // of the call], room for ceil(max_batch / 64) chunks)
    struct Sac { bool on = false; double* part = nullptr; int max_batch = 0; } sac;
    // the fused policy forward (hope_policy_kernel.h): packed = the parameters in the forward's layout (hope_policy_core.h pc_layout),
    // written by k_policy_pack on the caller's stream; loaded: a hope_env_policy_load has been enqueued since the enable
    struct Policy { bool on = false, loaded = false; int n_tokens = 0, out_dim = 0, tanh_out = 0, max_batch = 0; float* packed = nullptr; } policy;
    // the image encoder (hope_imgenc_kernel.h): packed = the 14 tensors in the kernels' layout (hope_imgenc_core.h IE_OFF_*), written by
    // k_imgenc_pack on the caller's stream; feat = the features between the two kernels, [max_batch][2048]; loaded: as for the policy
    struct ImgEnc { bool on = false, loaded = false; int act = 0, max_batch = 0; float* packed = nullptr; float* feat = nullptr; } imgenc;
    // the critics' fused forward (hope_critic_kernel.h): packed = n_slots parameter sets, each in the forward's layout (hope_critic_core.h
    // cc_layout), slot s written by k_critic_pack on the caller's stream; loaded[s]: a hope_env_critic_load of slot s has been enqueued
    // since the enable
    struct Critics { bool on = false, loaded[HOPE_CRITIC_SLOTS] = {}; int n_slots = 0, has_img = 0, has_action = 0, max_batch = 0; float* packed = nullptr; } critics;
    // HOPE_DEFER_RS: the search streams of the last step have not been joined into the caller's stream (ev_chain1_done, ev_search0_done)
    bool rs_pending = false;
};

namespace hope {
// HOPE_DEFER_RS bookkeeping (hope_env.hip): `s` waits for the search chains the last step left unjoined / the host does
int join_rs(hope_env_t* h, hipStream_t s);
int settle_rs(hope_env_t* h);
// hope_agent.hip: release a feature's device memory and put its struct back to the default (hope_env_*_disable, hope_env_destroy)
void plan_free(hope_env_t* h);
void choose_free(hope_env_t* h);
void onorm_free(hope_env_t* h);
void evalt_free(hope_env_t* h);
void gae_free(hope_env_t* h);
void ring_free(hope_env_t* h);
void ppo_free(hope_env_t* h);
void sac_free(hope_env_t* h);
// hope_policy.hip
void policy_free(hope_env_t* h);
void imgenc_free(hope_env_t* h);
void critics_free(hope_env_t* h);
}  // namespace hope
