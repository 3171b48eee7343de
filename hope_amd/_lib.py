"""ctypes binding of include/hope_env.h.  Fails loudly: there is no CPU fallback."""
import ctypes as C
import math
import os

import numpy as np

from .build import lib_path

# mirror of include/hope_env.h
LIDAR_NUM, N_ACTION, N_ITER, UPSAMPLE, TARGET_DIM, RS_MAX_SEG = 120, 42, 10, 10, 5, 5
F_OBS_F64, F_ACTION_F64, F_PROFILE, F_IMAGE, F_OVERLAP = 0x1, 0x2, 0x4, 0x8, 0x10
STAGE_MOTION, STAGE_OBS, STAGE_REWARD, STAGE_RS, STAGE_ALL = 0x1, 0x2, 0x4, 0x8, 0xF
ACTION_PHYSICAL = 0x10
ACTION_RESCALE_F32 = 0x80
AUTO_REDRAW = 0x100
DEFER_RS = 0x200
STAGE_IMG = 0x40
STAGE_NO_CULL, STAGE_ONE_SCENE = 0x4000, 0x8000   # reserved internal A/B switches (hope_amd/csrc/hope_internal.h): tests only
IMG_SIZE, IMG_CHANNELS, TRAJ_RENDER_LEN = 64, 3, 20
AUTO_RESET = 0x20
KERNELS = ('k_kinematics', 'k_env_step', 'k_rs_words', 'k_rs_validate', 'k_bev_image', 'k_bev_prep', 'k_rs_compact', 'k_post', 'k_rs_segs', 'k_rs_screen')
ABI_VERSION = 8

CURRICULUM_LIST_LEN = 1 << 20
PLAN_STATE_WORDS, PLAN_STEP_RATIO, PLAN_FORCED, PLAN_NO_POP = 6, 1.25, 0x1, 0x2
CHOOSE_NOMASK, CHOOSE_FIXED, CHOOSE_FALLBACK = 64, 128, 10     # flag bits of the chooser's index output; the fixed index
OBSNORM_LIDAR, OBSNORM_TARGET, OBSNORM_COLS, OBSNORM_UPDATE, OBSNORM_NORMALIZE = 120, 5, 125, 0x1, 0x2
GAE_SUMS, GAE_NORMALIZE, GAE_MAX_T = 0x1, 0x2, 4096
RING_MAX_T, RING_MAX_BATCH = 4096, 1 << 20
PPO_MAX_BATCH = 1 << 20
SAC_MAX_BATCH = 1 << 20
POLICY_MAX_BATCH = 1 << 20
IMGENC_MAX_BATCH = 1 << 18
CRITIC_SLOTS = 4
OPTIM_F32, OPTIM_F64, OPTIM_MAX_GROUPS, OPTIM_CAP, OPTIM_CHUNK = 0, 1, 4, 64, 1024
EVAL_STATE_WORDS = 10                                          # planes of the evaluation tracker's state block
BUCKET_UNLABELLED = 255
# hope_env_step_plan: words ahead of the chains / of a chain's scene ids, flag bits, kernel numbers
STEPPLAN_HEAD, STEPPLAN_CHAIN_HEAD = 3, 5
STEPPLAN_SPLIT, STEPPLAN_PIPE, STEPPLAN_FUSE_KIN, STEPPLAN_AUTO_SUBS = 0x1, 0x2, 0x4, 0x8
STEPPLAN_MOTION_ONE_LAUNCH, STEPPLAN_MOTION_FUSED_KIN, STEPPLAN_MOTION_TIMING, STEPPLAN_MOTION_SPLIT, STEPPLAN_MOTION_PAIR = 0, 1, 2, 3, 4
STEPPLAN_OBS_IN_STEP, STEPPLAN_OBS_SPLIT, STEPPLAN_OBS_PAIR = 0, 1, 2
MOTION_KERNELS = ('one_launch', 'one_launch_fused_kin', 'timing', 'split_one_scene', 'pair')
OBS_KERNELS = ('in_step', 'split_one_scene', 'pair')


class HopeError(RuntimeError):
    pass


class StepOut(C.Structure):
    _fields_ = [('lidar', C.c_void_p), ('action_mask', C.c_void_p), ('target', C.c_void_p), ('reward', C.c_void_p),
                ('reward_info', C.c_void_p), ('status', C.c_void_p), ('done', C.c_void_p), ('pose', C.c_void_p),
                ('rs_word', C.c_void_p), ('rs_lengths', C.c_void_p), ('img', C.c_void_p)]


class CurriculumParams(C.Structure):
    """hope_curriculum_params; the defaults are the reference's constants (train_HOPE_sac.py:30, :35, :63, :66, :77, :80, :88, :91)"""
    _fields_ = [('target', C.c_double * 4), ('type_window', C.c_double), ('case_window', C.c_double), ('type_fail_min', C.c_double),
                ('case_fail_min', C.c_double), ('worst_share', C.c_double), ('case_uniform', C.c_double), ('type_horizon', C.c_int64),
                ('case_horizon', C.c_int64)]

    def __init__(self, target=(0.95, 0.95, 0.9, 0.99), type_window=250.0, case_window=10.0, type_fail_min=0.01, case_fail_min=0.005,
                 worst_share=0.5, case_uniform=0.2, type_horizon=200, case_horizon=500):
        super().__init__((C.c_double * 4)(*target), type_window, case_window, type_fail_min, case_fail_min, worst_share, case_uniform,
                         type_horizon, case_horizon)


class ObsNormState(C.Structure):
    """hope_obsnorm_state: the statistics as the host twin hope_obsnorm_host holds them (zero to start)"""
    _fields_ = [('n_state', C.c_int64), ('mean', C.c_double * OBSNORM_COLS), ('S', C.c_double * OBSNORM_COLS), ('std', C.c_double * OBSNORM_COLS)]


class Ring(C.Structure):
    """hope_ring_t: the transition ring's tensors (float32, contiguous) and extents; `ring_desc` builds one from torch tensors"""
    _fields_ = [('lidar', C.c_void_p), ('target', C.c_void_p), ('action_mask', C.c_void_p), ('action', C.c_void_p), ('log_prob', C.c_void_p),
                ('reward', C.c_void_p), ('done', C.c_void_p), ('n', C.c_int32), ('T', C.c_int32)]


class RingBatch(C.Structure):
    """hope_ring_batch_t: the tensors a sampled batch goes to; `ring_batch_desc` builds one"""
    _fields_ = [('obs_lidar', C.c_void_p), ('obs_target', C.c_void_p), ('obs_mask', C.c_void_p), ('next_lidar', C.c_void_p),
                ('next_target', C.c_void_p), ('next_mask', C.c_void_p), ('action', C.c_void_p), ('reward', C.c_void_p), ('done', C.c_void_p),
                ('idx', C.c_void_p)]


class PpoBatch(C.Structure):
    """hope_ppo_batch_t: the tensors a gathered PPO minibatch goes to; `ppo_batch_desc` builds one (and notes its `batch`)"""
    _fields_ = [('lidar', C.c_void_p), ('target', C.c_void_p), ('mask', C.c_void_p), ('action', C.c_void_p), ('old_lp', C.c_void_p),
                ('adv', C.c_void_p), ('v_target', C.c_void_p), ('idx', C.c_void_p)]


# hope_policy_params_t's fields, in order, and the HopeNet state_dict entry behind each
POLICY_FIELDS = (('lidar_w1', 'embed_lidar.0.weight'), ('lidar_b1', 'embed_lidar.0.bias'), ('lidar_w2', 'embed_lidar.2.weight'),
                 ('lidar_b2', 'embed_lidar.2.bias'), ('target_w1', 'embed_tgt.0.weight'), ('target_b1', 'embed_tgt.0.bias'),
                 ('target_w2', 'embed_tgt.2.weight'), ('target_b2', 'embed_tgt.2.bias'), ('mask_w1', 'embed_am.0.weight'),
                 ('mask_b1', 'embed_am.0.bias'), ('mask_w2', 'embed_am.2.weight'), ('mask_b2', 'embed_am.2.bias'),
                 ('ln1_g', 'net.encoder.layers.0.0.norm.weight'), ('ln1_b', 'net.encoder.layers.0.0.norm.bias'),
                 ('qkv_w', 'net.encoder.layers.0.0.fn.to_qkv.weight'), ('out_w', 'net.encoder.layers.0.0.fn.to_out.0.weight'),
                 ('out_b', 'net.encoder.layers.0.0.fn.to_out.0.bias'), ('ln2_g', 'net.encoder.layers.0.1.norm.weight'),
                 ('ln2_b', 'net.encoder.layers.0.1.norm.bias'), ('ff1_w', 'net.encoder.layers.0.1.fn.net.0.weight'),
                 ('ff1_b', 'net.encoder.layers.0.1.fn.net.0.bias'), ('ff2_w', 'net.encoder.layers.0.1.fn.net.3.weight'),
                 ('ff2_b', 'net.encoder.layers.0.1.fn.net.3.bias'), ('head1_w', 'net.output.0.weight'), ('head1_b', 'net.output.0.bias'),
                 ('head2_w', 'net.output.2.weight'), ('head2_b', 'net.output.2.bias'))


class PolicyParams(C.Structure):
    """hope_policy_params_t: the addresses of a HopeNet's float32 parameter tensors; `policy_params` builds one"""
    _fields_ = [(k, C.c_void_p) for k, _ in POLICY_FIELDS]


# hope_critic_params_t's fields, in order, and the HopeNet state_dict entry behind each: the policy's, then the action embedding
CRITIC_FIELDS = POLICY_FIELDS + (('action_w1', 'embed_action.0.weight'), ('action_b1', 'embed_action.0.bias'),
                                 ('action_w2', 'embed_action.2.weight'), ('action_b2', 'embed_action.2.bias'))


class CriticParams(C.Structure):
    """hope_critic_params_t: the addresses of a critic HopeNet's float32 parameter tensors (the four action tensors None without an
    action token); `critic_params` builds one"""
    _fields_ = [(k, C.c_void_p) for k, _ in CRITIC_FIELDS]


# hope_imgenc_params_t's fields, in order, the HopeNet state_dict entry behind each and its shape
IMGENC_FIELDS = (('conv1_w', 'embed_img.net.0.layer.0.weight', (4, 3, 3, 3)), ('conv1_b', 'embed_img.net.0.layer.0.bias', (4,)),
                 ('short1_w', 'embed_img.net.0.shortcut.0.weight', (4, 3, 1, 1)), ('short1_b', 'embed_img.net.0.shortcut.0.bias', (4,)),
                 ('conv2_w', 'embed_img.net.1.layer.0.weight', (8, 4, 3, 3)), ('conv2_b', 'embed_img.net.1.layer.0.bias', (8,)),
                 ('short2_w', 'embed_img.net.1.shortcut.0.weight', (8, 4, 1, 1)), ('short2_b', 'embed_img.net.1.shortcut.0.bias', (8,)),
                 ('fc1_w', 'embed_img.net.3.weight', (256, 2048)), ('fc1_b', 'embed_img.net.3.bias', (256,)),
                 ('mean_w', 'embed_img.output_mean.weight', (128, 256)), ('mean_b', 'embed_img.output_mean.bias', (128,)),
                 ('re_w', 're_embed_img.1.weight', (128, 128)), ('re_b', 're_embed_img.1.bias', (128,)))


class ImgEncParams(C.Structure):
    """hope_imgenc_params_t: the addresses of the 14 float32 tensors of a HopeNet's image encoder; `imgenc_params` builds one"""
    _fields_ = [(k, C.c_void_p) for k, _, _ in IMGENC_FIELDS]


class OptimEntry(C.Structure):
    """hope_optim_entry_t: one tensor of an optimiser call; `optim_entries` builds a table of them"""
    _fields_ = [('p', C.c_void_p), ('g', C.c_void_p), ('m', C.c_void_p), ('v', C.c_void_p), ('numel', C.c_int64), ('group', C.c_int32),
                ('dtype', C.c_int32)]


class OptimGroup(C.Structure):
    """hope_optim_group_t: a parameter group's step; `optim_group` computes one from lr, betas, eps and the step count"""
    _fields_ = [('c1', C.c_double), ('b2', C.c_double), ('c2', C.c_double), ('step_size', C.c_double), ('bc2s', C.c_double), ('eps', C.c_double)]


# the prototypes of include/hope_env.h, one entry per exported call: name -> (return type, parameter types).  The parameter kinds:
# pointer, int / int32_t, uint32_t, int64_t, uint64_t, double, size_t; S is the `const char *` of the two calls that return text.
# tests/test_host.py compares this table, the constants above and the three structures with the header.
P, I, U32, I64, U64, D, SZ, S = C.c_void_p, C.c_int, C.c_uint32, C.c_int64, C.c_uint64, C.c_double, C.c_size_t, C.c_char_p
PP = C.POINTER(C.c_void_p)
PROTOTYPES = {
    'hope_env_create': (I, [PP, I, I, I, U32]),
    'hope_env_destroy': (I, [P]),
    'hope_last_error': (S, []),
    'hope_abi_version': (I, []),
    'hope_env_upload_tables': (I, [P] * 4),
    'hope_env_set_scenes': (I, [P, P, I] + [P] * 5),
    'hope_env_step': (I, [P, P, P, U32, C.POINTER(StepOut), P]),
    'hope_env_step_plan': (I, [P, U32, I, P, I]),
    'hope_env_wait_rs': (I, [P, P]),
    'hope_env_last_step': (I, [P, P]),
    'hope_env_wait_rs_step': (I, [P, U64, P]),
    'hope_env_reset_obs': (I, [P, P, U32, C.POINTER(StepOut), P]),
    'hope_env_restart': (I, [P, P, P]),
    'hope_env_set_pool': (I, [P, I] + [P] * 5),
    'hope_env_pool_staging': (I, [P, I] + [PP] * 5),
    'hope_env_commit_pool': (I, [P, I, P]),
    'hope_env_commit_pool_relaxed': (I, [P, I]),
    'hope_env_pool_staging_ready': (I, [P]),
    'hope_env_pool_generation': (I, [P, P]),
    'hope_env_set_redraw_seed': (I, [P, U64]),
    'hope_env_redraw': (I, [P, P, U64, P]),
    'hope_env_download_pool_index': (I, [P, P]),
    'hope_env_set_dlp_cases': (I, [P, I] + [P] * 4 + [I, P, P]),
    'hope_env_set_draw_class': (I, [P, P, I, P]),
    'hope_env_pool_overflow': (I, [P, P]),
    'hope_env_download_scenes': (I, [P, P, I] + [P] * 5),
    'hope_env_download_n_obst': (I, [P, P]),
    'hope_env_download_pool_state': (I, [P, P, P]),
    'hope_env_restore_maps': (I, [P, P, P, U64, U64]),
    'hope_env_queue_check': (I, [P] * 4),
    'hope_env_kernel_ms': (I, [P, P, P, I]),
    'hope_env_kernel_union_ms': (I, [P, P, P, I]),
    'hope_env_profile_kernels': (I, [P, U32]),
    'hope_env_download_state': (I, [P] * 4),
    'hope_env_upload_state': (I, [P] * 4),
    'hope_debug_math': (I, [I, I] + [P] * 4),
    'hope_debug_geom': (I, [I, I, I, P, P, P]),
    'hope_debug_mask_lut': (I, [P] * 4),
    'hope_debug_traffic': (I, [I, SZ, P, P]),
    'hope_debug_rs_prof': (I, [P, I]),
    'hope_debug_rs_filter_stats': (I, [P, I]),
    'hope_debug_rs_filter_dump': (I, [P]),
    'hope_debug_rs_log': (I, [P, I, P, I]),
    'hope_debug_step_prof': (I, [P, I]),
    'hope_debug_census': (I, [P, I]),
    'hope_scenegen_generate': (I, [I, I, I, U64, I64, I] + [P] * 6 + [I]),
    'hope_scenegen_default_threads': (I, []),
    'hope_scenegen_generate_det': (I, [I, I, I, U64, I64, I] + [P] * 6 + [I]),
    'hope_scenegen_generate_device': (I, [I] * 4 + [U64, I64, I] + [P] * 7),
    'hope_scenegen_log_det': (I, [I, P, P]),
    'hope_env_generate_pool': (I, [P, I, P, U64, I64, I]),
    'hope_env_curriculum_enable': (I, [P, P]),
    'hope_env_curriculum_disable': (I, [P]),
    'hope_env_set_pool_buckets': (I, [P, I, P]),
    'hope_env_curriculum_tally': (I, [P] * 4),
    'hope_env_curriculum_update': (I, [P, P]),
    'hope_env_curriculum_state': (I, [P] * 9),
    'hope_env_curriculum_set_windows': (I, [P, I] + [P] * 4),
    'hope_env_curriculum_download_lists': (I, [P] * 4),
    'hope_curriculum_lists_host': (I, [P, I, P, P, I, I] + [P] * 8),
    'hope_curriculum_fold_host': (I, [P, P, D, D, D]),
    'hope_map_level_host': (I, [I, I] + [P] * 6 + [I]),
    'hope_map_level_device': (I, [I, I, I] + [P] * 7),
    'hope_env_map_level': (I, [P] * 5),
    'hope_env_planner_enable': (I, [P, D]),
    'hope_env_planner_disable': (I, [P]),
    'hope_env_planner_reset': (I, [P, P, P]),
    'hope_env_planner_step': (I, [P] * 4 + [I, U64, P, P, P, I, P]),
    'hope_planner_step_host': (I, [I, D, P, P, P, I, P, I, P, P, P, I]),
    'hope_env_planner_download_state': (I, [P, P]),
    'hope_env_chooser_enable': (I, [P, P]),
    'hope_env_chooser_disable': (I, [P]),
    'hope_env_choose': (I, [P, P, P, I, I] + [P] * 4 + [U64, U64] + [P] * 6),
    'hope_chooser_host': (I, [I, P, P, P, I, I, P, I, P, P, P, U64, U64, U64, P, I] + [P] * 4),
    'hope_env_obsnorm_enable': (I, [P]),
    'hope_env_obsnorm_disable': (I, [P]),
    'hope_env_obsnorm_set': (I, [P, I64, P, P, P]),
    'hope_env_obsnorm_get': (I, [P, C.POINTER(I64), P, P, P]),
    'hope_env_obsnorm': (I, [P, P, P, I, I, U32, P, P, P]),
    'hope_obsnorm_host': (I, [C.POINTER(ObsNormState), P, P, I64, I, U32, P, P]),
    'hope_env_eval_enable': (I, [P, P]),
    'hope_env_eval_disable': (I, [P]),
    'hope_env_eval_begin': (I, [P] * 4),
    'hope_env_eval_override': (I, [P, P, I, P, U64, U64, P, P]),
    'hope_env_eval_track': (I, [P] * 10),
    'hope_env_eval_records': (I, [P, P, P]),
    'hope_env_eval_download_state': (I, [P, P]),
    'hope_eval_begin_host': (I, [I64, I64, P, P, I, P]),
    'hope_eval_override_host': (I, [I64, I64, P, P, P, I, P, U64, U64, U64, P]),
    'hope_eval_track_host': (I, [I64, I64, P, P, I] + [P] * 7),
    'hope_env_gae_enable': (I, [P]),
    'hope_env_gae_disable': (I, [P]),
    'hope_env_gae': (I, [P] * 6 + [I, I, D, D, U32] + [P] * 4),
    'hope_env_adv_normalize': (I, [P, P, I64, P, P, P]),
    'hope_gae_host': (I, [P] * 5 + [I64, I64, D, D, U32] + [P] * 4),
    'hope_adv_normalize_host': (I, [P, I64, P, P, P]),
    'hope_env_ring_enable': (I, [P]),
    'hope_env_ring_disable': (I, [P]),
    'hope_env_ring_before': (I, [P, C.POINTER(Ring), I] + [P] * 6),
    'hope_env_ring_after': (I, [P, C.POINTER(Ring), I, P, I] + [P] * 5),
    'hope_env_ring_sample': (I, [P, C.POINTER(Ring), I, I, I, P, P, U64, U64, P, P, P, C.POINTER(RingBatch), P]),
    'hope_ring_before_host': (I, [C.POINTER(Ring), I] + [P] * 5),
    'hope_ring_after_host': (I, [C.POINTER(Ring), I, P, I] + [P] * 4),
    'hope_ring_sample_host': (I, [C.POINTER(Ring), I, I, I64, P, P, U64, U64, P, P, P, C.POINTER(RingBatch)]),
    'hope_env_ppo_enable': (I, [P, I]),
    'hope_env_ppo_disable': (I, [P]),
    'hope_env_ppo_gather': (I, [P, C.POINTER(Ring), P, P, P, I, C.POINTER(PpoBatch), P]),
    'hope_env_ppo_loss': (I, [P, P, P, P, C.POINTER(PpoBatch), I, D] + [P] * 5),
    'hope_ppo_gather_host': (I, [C.POINTER(Ring), P, P, P, I64, C.POINTER(PpoBatch)]),
    'hope_ppo_loss_host': (I, [P, P, P, C.POINTER(PpoBatch), I64, D] + [P] * 4),
    'hope_env_sac_enable': (I, [P, I]),
    'hope_env_sac_disable': (I, [P]),
    'hope_env_sac_sample': (I, [P, P, P, P, I, P, P, P]),
    'hope_env_sac_critic': (I, [P] * 9 + [D, I] + [P] * 5),
    'hope_env_sac_seed': (I, [P, P, P, I, P, P, P]),
    'hope_env_sac_policy': (I, [P] * 8 + [D, I] + [P] * 5),
    'hope_sac_sample_host': (I, [P, P, P, I64, P, P]),
    'hope_sac_critic_host': (I, [P] * 8 + [D, I64] + [P] * 4),
    'hope_sac_seed_host': (I, [P, P, I64, P, P]),
    'hope_sac_policy_host': (I, [P] * 7 + [D, I64] + [P] * 4),
    'hope_env_policy_enable': (I, [P, I, I, I, I]),
    'hope_env_policy_disable': (I, [P]),
    'hope_env_policy_load': (I, [P, C.POINTER(PolicyParams), P]),
    'hope_env_policy_forward': (I, [P, P, P, P, P, I, P, P]),
    'hope_policy_forward_host': (I, [C.POINTER(PolicyParams), I, I, I, P, P, P, P, I64, P]),
    'hope_env_critic_enable': (I, [P, I, I, I, I]),
    'hope_env_critic_disable': (I, [P]),
    'hope_env_critic_load': (I, [P, I, C.POINTER(CriticParams), P]),
    'hope_env_critic_forward': (I, [P, C.POINTER(C.c_int), I, P, P, P, P, P, I, P, P]),
    'hope_critic_forward_host': (I, [C.POINTER(CriticParams), I, I, P, P, P, P, P, I64, P]),
    'hope_env_imgenc_enable': (I, [P, I, I]),
    'hope_env_imgenc_disable': (I, [P]),
    'hope_env_imgenc_load': (I, [P, C.POINTER(ImgEncParams), P]),
    'hope_env_imgenc_forward': (I, [P, P, I64, P, P, P]),
    'hope_debug_imgenc_stage': (I, [P, I, P, I64, P, P, P]),
    'hope_imgenc_forward_host': (I, [C.POINTER(ImgEncParams), I, P, I64, P, P]),
    'hope_env_optim_adam': (I, [P, C.POINTER(OptimEntry), I, C.POINTER(OptimGroup), I, P]),
    'hope_env_optim_polyak': (I, [P, C.POINTER(OptimEntry), I, D, P]),
    'hope_optim_adam_host': (I, [C.POINTER(OptimEntry), I, C.POINTER(OptimGroup), I]),
    'hope_optim_polyak_host': (I, [C.POINTER(OptimEntry), I, D]),
    'hope_env_num_scenes': (I, [P]),
    'hope_env_max_obstacles': (I, [P]),
    'hope_env_device_arch': (S, [P]),
}
EXPORTS = list(PROTOTYPES)


_lib = None


def load_library():
    """dlopen hope_amd/libhope_env.so (built by hope_amd.build.build_extension / __graft_entry__.build)."""
    global _lib
    if _lib is not None:
        return _lib
    # PyTorch-ROCm bundles its own libamdhip64/libhsa-runtime64.  Import it FIRST so that this library
    # binds to the HIP runtime torch already initialised (one runtime per process); loading in the other
    # order leaves the process with two runtimes and "no ROCm-capable device" from the second one.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    path = lib_path()
    if not os.path.exists(path):
        raise HopeError(f'{path} is missing: run `python -c "import __graft_entry__ as g; g.build()"` '
                        '(hipcc --offload-arch=gfx950). There is no CPU fallback.')
    L = C.CDLL(path)
    for name, (restype, argtypes) in PROTOTYPES.items():
        if not hasattr(L, name):
            raise HopeError(f'{path} does not export {name}')
        f = getattr(L, name)
        f.restype, f.argtypes = restype, argtypes
    if L.hope_abi_version() != ABI_VERSION:
        raise HopeError(f'ABI mismatch: library {L.hope_abi_version()} vs binding {ABI_VERSION}')
    _lib = L
    return L


def check(rc, what=''):
    if rc != 0:
        msg = load_library().hope_last_error().decode(errors='replace')
        raise HopeError(f'{what} failed (code {rc}): {msg}')


def seed64(seed):
    """a Python int of any size or sign as the uint64_t seed / counter of the draws"""
    return C.c_uint64(int(seed) & (2 ** 64 - 1))


# The library sees addresses only: the two functions below are the one size check between a caller's memory and a kernel or a host
# loop that runs over it.  Every tensor or array handed to a call goes through one of them, with the call's and the argument's name.
def tensor_arg(call, name, x, dtype, shape, device, optional=False):
    """the torch tensor x as a call's pointer argument (c_void_p): x has `dtype` (one torch dtype or a tuple of them) and exactly
    `shape` (None in it: any extent), lives on `device` and is contiguous -- or HopeError.  optional: None passes as None (NULL)."""
    if x is None and optional:
        return None
    dtypes = dtype if type(dtype) is tuple else (dtype,)
    try:
        got = x.shape                                # (the passing case is the hot path: step() comes through here twice)
        if x.dtype in dtypes and x.device == device and x.is_contiguous() \
                and (got == shape or (len(got) == len(shape) and all(w is None or w == s for s, w in zip(got, shape)))):
            return C.c_void_p(x.data_ptr())
        got = f"{str(x.dtype).replace('torch.', '')} {list(got)}{'' if x.is_contiguous() else ' strided'} on {x.device}"
    except AttributeError:                           # None, a numpy array, a list: no tensor
        got = 'None' if x is None else type(x).__name__
    want = ' or '.join(str(d).replace('torch.', '') for d in dtypes)
    raise HopeError(f"{call}: {name} must be {want} {str(list(shape)).replace('None', '?')} contiguous on {device}, got {got}")


def array_arg(call, name, x, dtype, shape, optional=False):
    """x as the C-contiguous numpy array of `dtype` (np.ascontiguousarray: lists and other dtypes convert, as they always did) and
    exactly `shape` (None in it: any extent) that a call reads or writes -- or HopeError.  Returns the array: pass its `.ctypes`, and
    hold the array until the call has returned.  optional: None passes as None."""
    if x is None and optional:
        return None
    try:
        a = None if x is None else np.ascontiguousarray(x, dtype=dtype)
    except (TypeError, ValueError):                  # not convertible to dtype
        a = None
    if a is not None and a.ndim == len(shape) and all(w is None or w == s for s, w in zip(a.shape, shape)):
        return a
    got = f'{a.dtype.name} {list(a.shape)}' if a is not None else 'None' if x is None else type(x).__name__
    raise HopeError(f"{call}: {name} must be {np.dtype(dtype).name} {str(list(shape)).replace('None', '?')}, got {got}")


_RING_FIELDS = (('lidar', LIDAR_NUM), ('target', TARGET_DIM), ('action_mask', N_ACTION), ('action', 2), ('log_prob', 2), ('reward', None), ('done', None))
_BATCH_FIELDS = (('obs_lidar', LIDAR_NUM), ('obs_target', TARGET_DIM), ('obs_mask', N_ACTION), ('next_lidar', LIDAR_NUM), ('next_target', TARGET_DIM),
                 ('next_mask', N_ACTION), ('action', 2), ('reward', None), ('done', None))
_PPO_FIELDS = (('lidar', LIDAR_NUM), ('target', TARGET_DIM), ('mask', N_ACTION), ('action', 2), ('old_lp', None), ('adv', None), ('v_target', None))


def ring_desc(call, device, n, horizon, **tensors):
    """the hope_ring_t over the float32 tensors lidar, target, action_mask, action, log_prob [n, T, width], reward, done [n, T], each
    checked by tensor_arg.  The struct holds addresses only: keep the tensors alive as long as it is used."""
    import torch
    r = Ring(n=n, T=horizon)
    for name, width in _RING_FIELDS:
        shape = (n, horizon) if width is None else (n, horizon, width)
        setattr(r, name, tensor_arg(call, name, tensors.get(name), torch.float32, shape, device).value)
    return r


def ring_batch_desc(call, device, batch, **tensors):
    """the hope_ring_batch_t over float32 tensors [batch, width] / [batch] and idx int32 [batch, 3], each checked by tensor_arg"""
    import torch
    o = RingBatch()
    for name, width in _BATCH_FIELDS:
        setattr(o, name, tensor_arg(call, name, tensors.get(name), torch.float32, (batch,) if width is None else (batch, width), device).value)
    o.idx = tensor_arg(call, 'idx', tensors.get('idx'), torch.int32, (batch, 3), device).value
    return o


def ppo_batch_desc(call, device, batch, **tensors):
    """the hope_ppo_batch_t over float32 tensors lidar, target, mask, action [batch, width], old_lp, adv, v_target [batch] and idx int32
    [batch], each checked by tensor_arg; `.batch` of the result is the extent they were checked for"""
    import torch
    o = PpoBatch()
    for name, width in _PPO_FIELDS:
        setattr(o, name, tensor_arg(call, name, tensors.get(name), torch.float32, (batch,) if width is None else (batch, width), device).value)
    o.idx = tensor_arg(call, 'idx', tensors.get('idx'), torch.int32, (batch,), device).value
    o.batch = batch
    return o


def policy_shape(module):
    """(n_tokens, out_dim, tanh_out) of a `policy.HopeNet` whose configuration is the one the fused forward is compiled for (the
    reference's: embed 128, two tanh embedding layers, one encoder layer of 8 heads x 32 with a 128-wide token MLP, hidden_dim 128,
    lidar 120 / target 5 / action mask 42, with or without the image token, no action token) -- or ValueError naming what differs."""
    cfg = getattr(module, 'cfg', None)
    if cfg is None or not hasattr(module, 'embed_lidar'):
        raise ValueError(f'the fused policy forward takes a hope_amd.policy.HopeNet, not {type(module).__name__}')
    att = cfg.get('attention_configs')
    if att is None:
        raise ValueError('the fused policy forward needs the attention trunk (use_attention=False is not compiled in)')
    want = {'depth': 1, 'heads': 8, 'dim_head': 32, 'mlp_dim': 128, 'hidden_dim': 128}
    bad = [f'attention {k} = {att.get(k)} (compiled for {v})' for k, v in want.items() if att.get(k) != v]
    n_tokens = 3 + int(cfg.get('img_shape') is not None)
    want = {'embed_size': 128, 'n_embed_layers': 2, 'lidar_shape': 120, 'target_shape': 5, 'action_mask_shape': 42, 'n_modal': n_tokens,
            'use_tanh_activate': True}
    bad += [f'{k} = {cfg.get(k)} (compiled for {v})' for k, v in want.items() if cfg.get(k) != v]
    if cfg.get('input_action_dim', 0) > 0:
        bad.append('an action token (SAC critics are out of scope)')
    if cfg.get('output_size') not in (1, 2):
        bad.append(f"output_size = {cfg.get('output_size')} (compiled for 1 or 2)")
    if bad:
        raise ValueError('the fused policy forward is compiled for the reference configuration only: ' + '; '.join(bad))
    return n_tokens, int(cfg['output_size']), int(bool(cfg['use_tanh_output']))


def policy_params(call, module, device):
    """the hope_policy_params_t over the float32 parameters of a HopeNet on `device`, each checked by tensor_arg -> (struct, tensors).
    The struct holds addresses only: keep the tensors (the module) alive and unchanged until the call that takes it has run."""
    import torch
    n_tokens, out_dim, _ = policy_shape(module)
    sd = dict(module.named_parameters())
    shapes = {'lidar_w1': (128, LIDAR_NUM), 'target_w1': (128, TARGET_DIM), 'mask_w1': (128, N_ACTION), 'qkv_w': (768, 128), 'out_w': (128, 256),
              'head1_w': (128, n_tokens * 128), 'head2_w': (out_dim, 128), 'head2_b': (out_dim,)}
    p, keep = PolicyParams(), []
    for field, key in POLICY_FIELDS:
        t = sd[key].detach()
        shape = shapes.get(field, (128, 128) if field.endswith(('_w1', '_w2', '_w')) else (128,))
        setattr(p, field, tensor_arg(call, key, t, torch.float32, shape, device).value)
        keep.append(t)
    return p, keep


def critic_net(module):
    """the HopeNet behind a critic: a `policy.SacCritic`'s `.net`, or the HopeNet itself"""
    inner = getattr(module, 'net', None)
    return inner if not hasattr(module, 'embed_lidar') and hasattr(inner, 'embed_lidar') else module


def critic_shape(module):
    """(has_img, has_action) of a critic -- a `policy.HopeNet` with one linear output, or a `policy.SacCritic` -- whose configuration
    is the one the critics' fused forward is compiled for (the reference's: embed 128, two tanh embedding layers, one encoder layer of
    8 heads x 32 with a 128-wide token MLP, hidden_dim 128, lidar 120 / target 5 / action mask 42, with or without the image token,
    with or without a 2-wide action token) -- or ValueError naming what differs."""
    net = critic_net(module)
    cfg = getattr(net, 'cfg', None)
    if cfg is None or not hasattr(net, 'embed_lidar'):
        raise ValueError(f"the critics' fused forward takes a hope_amd.policy.HopeNet or SacCritic, not {type(module).__name__}")
    att = cfg.get('attention_configs')
    if att is None:
        raise ValueError("the critics' fused forward needs the attention trunk (use_attention=False is not compiled in)")
    want = {'depth': 1, 'heads': 8, 'dim_head': 32, 'mlp_dim': 128, 'hidden_dim': 128}
    bad = [f'attention {k} = {att.get(k)} (compiled for {v})' for k, v in want.items() if att.get(k) != v]
    has_img, act_dim = int(cfg.get('img_shape') is not None), cfg.get('input_action_dim', 0)
    if act_dim not in (0, 2):
        bad.append(f'input_action_dim = {act_dim} (compiled for 0 or 2)')
    has_action = int(act_dim > 0)
    want = {'embed_size': 128, 'n_embed_layers': 2, 'lidar_shape': 120, 'target_shape': 5, 'action_mask_shape': 42,
            'n_modal': 3 + has_img + has_action, 'use_tanh_activate': True, 'output_size': 1, 'use_tanh_output': False}
    bad += [f'{k} = {cfg.get(k)} (compiled for {v})' for k, v in want.items() if cfg.get(k) != v]
    if bad:
        raise ValueError("the critics' fused forward is compiled for the reference's critic configuration only: " + '; '.join(bad))
    return has_img, has_action


def critic_params(call, module, device):
    """the hope_critic_params_t over the float32 parameters of a critic (HopeNet or SacCritic) on `device`, each checked by tensor_arg
    -> (struct, tensors).  The struct holds addresses only: keep the tensors (the module) alive and unchanged until the call that
    takes it has run."""
    import torch
    has_img, has_action = critic_shape(module)
    sd = dict(critic_net(module).named_parameters())
    shapes = {'lidar_w1': (128, LIDAR_NUM), 'target_w1': (128, TARGET_DIM), 'mask_w1': (128, N_ACTION), 'qkv_w': (768, 128), 'out_w': (128, 256),
              'head1_w': (128, (3 + has_img + has_action) * 128), 'head2_w': (1, 128), 'head2_b': (1,), 'action_w1': (128, 2)}
    p, keep = CriticParams(), []
    for field, key in CRITIC_FIELDS[:len(CRITIC_FIELDS) if has_action else len(POLICY_FIELDS)]:
        t = sd[key].detach()
        shape = shapes.get(field, (128, 128) if field.endswith(('_w1', '_w2', '_w')) else (128,))
        setattr(p, field, tensor_arg(call, key, t, torch.float32, shape, device).value)
        keep.append(t)
    return p, keep


def imgenc_shape(module):
    """act (0 tanh, 1 LeakyReLU) of the image encoder of a `policy.HopeNet` whose configuration is the one the fused image encoder
    is compiled for (the reference's: img_shape (3, 64, 64), img_conv_layers [4, 8], k_img_conv 3, img_linear_layers [256], embed
    128, tanh between the token's layers, float32) -- or ValueError naming what differs."""
    cfg = getattr(module, 'cfg', None)
    if cfg is None or not hasattr(module, 'embed_lidar'):
        raise ValueError(f'the fused image encoder takes a hope_amd.policy.HopeNet, not {type(module).__name__}')
    if cfg.get('img_shape') is None or not hasattr(module, 'embed_img'):
        raise ValueError('the fused image encoder needs a net with an image token (use_img=False has none)')
    want = {'img_shape': (3, 64, 64), 'img_conv_layers': [4, 8], 'k_img_conv': 3, 'img_linear_layers': [256], 'embed_size': 128,
            'use_tanh_activate': True}
    norm = lambda v: list(v) if isinstance(v, (tuple, list)) else v  # noqa: E731
    bad = [f'{k} = {cfg.get(k)} (compiled for {v})' for k, v in want.items() if norm(cfg.get(k)) != norm(v)]
    if getattr(module.embed_img, 'amp', False):
        bad.append('amp = True (bf16 autocast is out of scope: set_img_amp(net, False))')
    if bad:
        raise ValueError('the fused image encoder is compiled for the reference configuration only: ' + '; '.join(bad))
    import torch
    return 0 if isinstance(module.embed_img.net[0].layer[1], torch.nn.Tanh) else 1


def imgenc_params(call, module, device):
    """the hope_imgenc_params_t over the 14 float32 encoder tensors of a HopeNet on `device`, each checked by tensor_arg
    -> (struct, tensors).  The struct holds addresses only: keep the tensors alive and unchanged until the call that takes it has run."""
    import torch
    imgenc_shape(module)
    sd = dict(module.named_parameters())
    p, keep = ImgEncParams(), []
    for field, key, shape in IMGENC_FIELDS:
        t = sd[key].detach()
        setattr(p, field, tensor_arg(call, key, t, torch.float32, shape, device).value)
        keep.append(t)
    return p, keep


def optim_group(lr, betas, eps, t):
    """the hope_optim_group_t of a parameter group at its step t >= 1: the bias corrections folded into the step, as doubles"""
    b1, b2 = float(betas[0]), float(betas[1])
    return OptimGroup(1.0 - b1, b2, 1.0 - b2, float(lr) / (1.0 - b1 ** t), math.sqrt(1.0 - b2 ** t), float(eps))


def optim_entries(params, grads, ms=None, vs=None, groups=None, call='hope_env_optim_adam', device=None):
    """the table of hope_optim_entry_t over the tensors params[i], grads[i], ms[i], vs[i] (Adam), or over targets and current tensors
    (Polyak: optim_entries(targets, currents)) -> (pointer to the table, n, what must stay alive: the table's memory and the tensors).
    groups[i]: the group index of entry i (default 0).  ValueError, naming the entry, for a tensor that is not contiguous, not float32
    / float64, on another device than `device` (default: that of params[0]), or whose partners differ in shape or dtype -- tensor_arg's
    conditions, asked here in one pass because a call has a hundred entries.  The table holds addresses only: keep the tensors alive
    and in place until the call that takes it has been enqueued."""
    import torch
    cols = [list(params), list(grads)] + ([list(ms), list(vs)] if ms is not None else [])
    names = ('p', 'g', 'm', 'v') if ms is not None else ('target', 'current')
    n = len(cols[0])
    if n < 1 or any(len(c) != n for c in cols):
        raise ValueError(f'{call}: the lists must have one length >= 1, got {[len(c) for c in cols]}')
    first = cols[0][0]
    device = torch.device(device) if device is not None else first.device if torch.is_tensor(first) else None
    f32, f64, strided, is_tensor = torch.float32, torch.float64, torch.strided, torch.is_tensor
    table = np.zeros(n, dtype=_OPTIM_ENTRY)
    try:
        for k, col in zip('pgmv', cols):
            table[k] = [x.data_ptr() for x in col]
        heads = [(p.dtype, p.shape) for p in cols[0]]
        ok = all(dt is f32 or dt is f64 for dt, _ in heads) and \
            all(x.dtype is h[0] and x.shape == h[1] and x.device == device and x.layout is strided and x.is_contiguous() for col in cols for x, h in zip(col, heads))
    except (AttributeError, RuntimeError):           # no tensor, or one without storage (sparse)
        ok = False
    if not ok:
        _optim_entries_refuse(call, names, cols, device)
    table['numel'] = [p.numel() for p in cols[0]]
    table['dtype'] = [OPTIM_F64 if dt is f64 else OPTIM_F32 for dt, _ in heads]
    if groups is not None:
        table['group'] = groups
    return table.ctypes.data_as(C.POINTER(OptimEntry)), n, (table, cols)


_OPTIM_ENTRY = np.dtype([('p', np.uint64), ('g', np.uint64), ('m', np.uint64), ('v', np.uint64), ('numel', np.int64), ('group', np.int32),
                         ('dtype', np.int32)])
assert _OPTIM_ENTRY.itemsize == C.sizeof(OptimEntry)


def _optim_entries_refuse(call, names, cols, device):
    """the ValueError of optim_entries: the first entry that does not pass, and why"""
    import torch
    for i, p in enumerate(cols[0]):
        if not torch.is_tensor(p) or p.dtype not in (torch.float32, torch.float64):
            raise ValueError(f'{call}: entry {i}: {names[0]} must be a float32 or float64 tensor, got {getattr(p, "dtype", type(p).__name__)}')
        for name, col in zip(names, cols):
            x = col[i]
            if not torch.is_tensor(x) or x.layout != torch.strided:
                raise ValueError(f'{call}: entry {i}: {name} must be a dense tensor, got {type(x).__name__ if not torch.is_tensor(x) else x.layout}')
            if x.dtype != p.dtype or x.shape != p.shape:
                raise ValueError(f'{call}: entry {i}: {name} is {x.dtype} {list(x.shape)}, {names[0]} is {p.dtype} {list(p.shape)}')
            if x.device != device:
                raise ValueError(f'{call}: entry {i}: {name} is on {x.device}, the call on {device}')
            if not x.is_contiguous():
                raise ValueError(f'{call}: entry {i}: {name} is not contiguous')
    raise ValueError(f'{call}: the tensors do not go together')
