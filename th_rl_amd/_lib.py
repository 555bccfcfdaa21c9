"""ctypes binding of libthrl_hip.so (include/thrl.h).  No CPU fallback: every
compute entry point raises if the library or a GPU is missing."""
import ctypes
import os

HERE = os.path.dirname(os.path.abspath(__file__))
# THRL_LIB: an alternative build of the SAME ABI (the timing-only ablation variants of profiles/ablate.py)
LIB_PATH = os.environ.get("THRL_LIB") or os.path.join(HERE, "libthrl_hip.so")
MAXA = 8

KERNEL_AUTO, KERNEL_GENERIC, KERNEL_WAVE, KERNEL_WAVE_PLAIN, KERNEL_WAVE_GREEDY, KERNEL_TUPLE = 0, 1, 2, 3, 4, 5
KERNEL_NAMES = {0: "auto", 1: "generic", 2: "wave", 5: "tuple"}
ABI_VERSION = 4


class ThrlError(RuntimeError):
    code = None             # the negative thrl_err when the error came from the library

ERR_BAD_CONFIG = -1
ERR_UNSUPPORTED = -3


class Cfg(ctypes.Structure):
    """thrl_cfg"""
    _fields_ = [
        ("n_games", ctypes.c_int32), ("n_agents", ctypes.c_int32),
        ("max_steps", ctypes.c_int32), ("q_dtype", ctypes.c_int32),
        ("env_a", ctypes.c_double), ("env_b", ctypes.c_double),
        ("noise_prob", ctypes.c_double),
        ("n_states", ctypes.c_int32 * MAXA), ("n_actions", ctypes.c_int32 * MAXA),
        ("min_memory", ctypes.c_int32 * MAXA), ("capacity", ctypes.c_int32 * MAXA),
        ("max_state", ctypes.c_double * MAXA), ("gamma", ctypes.c_double * MAXA),
        ("alpha", ctypes.c_double * MAXA), ("eps_end", ctypes.c_double * MAXA),
        ("eps_step", ctypes.c_double * MAXA), ("act_lo", ctypes.c_double * MAXA),
        ("act_hi", ctypes.c_double * MAXA),
    ]


class Buffers(ctypes.Structure):
    """thrl_buffers"""
    _fields_ = [
        ("q", ctypes.c_void_p), ("counter", ctypes.c_void_p), ("state", ctypes.c_void_p),
        ("replay_mem", ctypes.c_void_p), ("replay_mem_bytes", ctypes.c_size_t),
        ("reward_log", ctypes.c_void_p), ("action_log", ctypes.c_void_p),
        ("game_reward_log", ctypes.c_void_p), ("game_action_log", ctypes.c_void_p),
        ("inj_u", ctypes.c_void_p), ("inj_choice", ctypes.c_void_p),
        ("inj_noise_u", ctypes.c_void_p), ("inj_noise_a", ctypes.c_void_p),
        ("workspace", ctypes.c_void_p), ("workspace_bytes", ctypes.c_size_t),
        ("sweep_gamma", ctypes.c_void_p), ("sweep_alpha", ctypes.c_void_p),
        ("sweep_eps_end", ctypes.c_void_p), ("sweep_eps_step", ctypes.c_void_p),
        ("sweep_eps", ctypes.c_void_p), ("sweep_noise_prob", ctypes.c_void_p),
    ]


class Run(ctypes.Structure):
    """thrl_run"""
    _fields_ = [
        ("seed", ctypes.c_uint64), ("game_offset", ctypes.c_uint64),
        ("first_episode", ctypes.c_uint64), ("n_episodes", ctypes.c_int32),
        ("kernel", ctypes.c_int32), ("eps", ctypes.c_double * MAXA),
        ("mem_count", ctypes.c_int32 * MAXA), ("kernel_used", ctypes.c_int32),
    ]


class Mixed(ctypes.Structure):
    """thrl_mixed"""
    _fields_ = [
        ("kind", ctypes.c_int32 * MAXA), ("nn_params", ctypes.c_void_p * MAXA),
        ("buf_price", ctypes.c_void_p * MAXA), ("buf_action", ctypes.c_void_p * MAXA),
        ("buf_reward", ctypes.c_void_p * MAXA), ("buf_nprice", ctypes.c_void_p * MAXA),
        ("buf_scratch", ctypes.c_void_p * MAXA), ("buf_len", ctypes.c_int32 * MAXA),
        ("min_memory", ctypes.c_int32 * MAXA), ("count", ctypes.c_int32 * MAXA),
        ("sweep_gamma", ctypes.c_void_p), ("sweep_alpha", ctypes.c_void_p),
        ("sweep_eps_end", ctypes.c_void_p), ("sweep_eps_step", ctypes.c_void_p),
        ("sweep_eps", ctypes.c_void_p), ("sweep_noise_prob", ctypes.c_void_p),
        ("policy_tab", ctypes.c_void_p), ("policy_tab_bytes", ctypes.c_size_t), ("flags", ctypes.c_int32),
        # parity mode: recorded draws and sampled actions (device pointers, all None = Philox)
        ("inj_u", ctypes.c_void_p), ("inj_choice", ctypes.c_void_p), ("inj_noise_u", ctypes.c_void_p),
        ("inj_noise_a", ctypes.c_void_p), ("inj_action", ctypes.c_void_p),
    ]


STATS_MAX_BINS = 1024
STATS_MAXQ = 2 * MAXA + 1


class GroupStatsArgs(ctypes.Structure):
    """thrl_group_stats_args"""
    _fields_ = [
        ("n_games", ctypes.c_int32), ("n_agents", ctypes.c_int32), ("n_episodes", ctypes.c_int32),
        ("n_groups", ctypes.c_int32), ("n_bins", ctypes.c_int32), ("reserved", ctypes.c_int32),
        ("game_reward_log", ctypes.c_void_p), ("game_action_log", ctypes.c_void_p),
        ("group_of", ctypes.c_void_p), ("perm", ctypes.c_void_p), ("seg_off", ctypes.c_void_p),
        ("lo", ctypes.c_double * STATS_MAXQ), ("hi", ctypes.c_double * STATS_MAXQ),
        ("inv_w", ctypes.c_double * STATS_MAXQ), ("scale", (ctypes.c_double * 2) * STATS_MAXQ),
        ("hist", ctypes.c_void_p), ("sums", ctypes.c_void_p), ("minmax", ctypes.c_void_p),
    ]


class EwmRowsArgs(ctypes.Structure):
    """thrl_ewm_rows_args"""
    _fields_ = [
        ("n_games", ctypes.c_int32), ("n_agents", ctypes.c_int32), ("n_episodes", ctypes.c_int32),
        ("reserved", ctypes.c_int32), ("decay", ctypes.c_double), ("den", ctypes.c_double),
        ("reward_rows", ctypes.c_void_p), ("action_rows", ctypes.c_void_p),
        ("reward_out", ctypes.c_void_p), ("action_out", ctypes.c_void_p),
        ("state_in", ctypes.c_void_p), ("state_out", ctypes.c_void_p), ("den_out", ctypes.POINTER(ctypes.c_double)),
    ]


DEV_MAX_STEPS = 1 << 20
DEV_MAX_HORIZON = 1 << 24


class DeviationArgs(ctypes.Structure):
    """thrl_deviation_args"""
    _fields_ = [
        ("n_games", ctypes.c_int32), ("deviator", ctypes.c_int32), ("dev_len", ctypes.c_int32),
        ("n_steps", ctypes.c_int32), ("horizon", ctypes.c_int32), ("dev_action", ctypes.c_int32),
        ("row_begin", ctypes.c_int32), ("row_count", ctypes.c_int32),
        ("state0", ctypes.c_void_p), ("sweep_gamma", ctypes.c_void_p),
        ("mu", ctypes.c_void_p), ("lam", ctypes.c_void_p), ("mu_post", ctypes.c_void_p), ("lam_post", ctypes.c_void_p),
        ("ret_step", ctypes.c_void_p), ("act_dev", ctypes.c_void_p),
        ("cycle_reward", ctypes.c_void_p), ("cycle_action", ctypes.c_void_p), ("gain", ctypes.c_void_p),
        ("reward_rows", ctypes.c_void_p), ("action_rows", ctypes.c_void_p),
    ]


TRACK_BASELINE = 1


class PolicyTrackArgs(ctypes.Structure):
    """thrl_policy_track_args"""
    _fields_ = [
        ("n_games", ctypes.c_int32), ("flags", ctypes.c_int32), ("episode", ctypes.c_int64), ("window", ctypes.c_int64),
        ("policy", ctypes.c_void_p), ("stable_since", ctypes.c_void_p), ("converged_at", ctypes.c_void_p),
        ("conv_since", ctypes.c_void_p), ("changes", ctypes.c_void_p), ("n_converged", ctypes.c_void_p),
        ("state", ctypes.c_void_p), ("q_conv", ctypes.c_void_p), ("state_conv", ctypes.c_void_p),
    ]


EQ_MAX_ITERS = 64
EQ_MAX_TUPLES = 4096
EQ_MAX_STATES = 1024


class EquilibriumArgs(ctypes.Structure):
    """thrl_equilibrium_args"""
    _fields_ = [
        ("n_games", ctypes.c_int32), ("agents", ctypes.c_int32),
        ("state0", ctypes.c_void_p), ("sweep_gamma", ctypes.c_void_p), ("n_states", ctypes.POINTER(ctypes.c_int32)),
        ("mu", ctypes.c_void_p), ("lam", ctypes.c_void_p), ("iters", ctypes.c_void_p),
        ("n_diff_all", ctypes.c_void_p), ("n_diff_on", ctypes.c_void_p),
        ("loss_all", ctypes.c_void_p), ("loss_on", ctypes.c_void_p), ("loss_all_mean", ctypes.c_void_p),
        ("loss_on_mean", ctypes.c_void_p), ("v_on", ctypes.c_void_p),
        ("br_policy", ctypes.c_void_p), ("v_opt", ctypes.c_void_p), ("v_pi", ctypes.c_void_p),
    ]


XPLAY_POLICY_GIVEN = 1


class CrossplayArgs(ctypes.Structure):
    """thrl_crossplay_args"""
    _fields_ = [
        ("n_games", ctypes.c_int32), ("n_matches", ctypes.c_int32), ("n_steps", ctypes.c_int32),
        ("horizon", ctypes.c_int32), ("row_begin", ctypes.c_int32), ("row_count", ctypes.c_int32),
        ("flags", ctypes.c_int32), ("reserved", ctypes.c_int32),
        ("seat", ctypes.c_void_p), ("state0", ctypes.c_void_p), ("policy", ctypes.c_void_p),
        ("mu", ctypes.c_void_p), ("lam", ctypes.c_void_p),
        ("cycle_reward", ctypes.c_void_p), ("cycle_action", ctypes.c_void_p),
        ("reward_rows", ctypes.c_void_p), ("action_rows", ctypes.c_void_p),
    ]


ATTR_KEEP = 8
ATTR_POLICY_GIVEN = 1
ATTR_MAX_STARTS = 1 << 20


class AttractorsArgs(ctypes.Structure):
    """thrl_attractors_args"""
    _fields_ = [
        ("n_games", ctypes.c_int32), ("flags", ctypes.c_int32), ("n_starts", ctypes.c_int32), ("reserved", ctypes.c_int32),
        ("state0", ctypes.c_void_p), ("policy", ctypes.c_void_p), ("start_rows", ctypes.c_void_p),
        ("start_w", ctypes.c_void_p), ("n_states", ctypes.POINTER(ctypes.c_int32)),
        ("n_attr", ctypes.c_void_p), ("mu_max", ctypes.c_void_p), ("n_cycle_states", ctypes.c_void_p),
        ("rep", ctypes.c_void_p), ("lam", ctypes.c_void_p), ("basin", ctypes.c_void_p),
        ("cycle_reward", ctypes.c_void_p), ("cycle_action", ctypes.c_void_p),
        ("rep_x0", ctypes.c_void_p), ("mu_x0", ctypes.c_void_p), ("slot_x0", ctypes.c_void_p),
        ("reset_mass", ctypes.c_void_p), ("reset_mass_other", ctypes.c_void_p), ("reset_reward", ctypes.c_void_p),
        ("state_rep", ctypes.c_void_p), ("state_mu", ctypes.c_void_p),
    ]


STAT_POLICY_GIVEN = 1
STAT_START_STATE = 2
STAT_MAX_CELLS = 4096
STAT_MAX_ITERS = 65536


class StationaryArgs(ctypes.Structure):
    """thrl_stationary_args"""
    _fields_ = [
        ("n_games", ctypes.c_int32), ("flags", ctypes.c_int32), ("n_cells", ctypes.c_int32), ("band_w", ctypes.c_int32),
        ("max_iters", ctypes.c_int32), ("reserved", ctypes.c_int32),
        ("noise_prob", ctypes.c_double), ("tol", ctypes.c_double),
        ("noise_prob_g", ctypes.c_void_p), ("state0", ctypes.c_void_p), ("policy", ctypes.c_void_p),
        ("cell_rows", ctypes.c_void_p), ("cell_w", ctypes.c_void_p), ("det_cell", ctypes.c_void_p),
        ("band_lo", ctypes.c_void_p), ("band", ctypes.c_void_p), ("noise_reward", ctypes.c_void_p),
        ("noise_price", ctypes.c_void_p), ("n_tuples", ctypes.POINTER(ctypes.c_int32)),
        ("iters", ctypes.c_void_p), ("change", ctypes.c_void_p), ("mass", ctypes.c_void_p),
        ("stat_reward", ctypes.c_void_p), ("stat_action", ctypes.c_void_p), ("stat_price", ctypes.c_void_p),
        ("pi", ctypes.c_void_p),
    ]


EQN_POLICY_GIVEN = 1


class EquilibriumNoiseArgs(ctypes.Structure):
    """thrl_equilibrium_noise_args"""
    _fields_ = [
        ("n_games", ctypes.c_int32), ("agents", ctypes.c_int32), ("flags", ctypes.c_int32), ("n_cells", ctypes.c_int32),
        ("band_w", ctypes.c_int32), ("max_sweeps", ctypes.c_int32),
        ("noise_prob", ctypes.c_double), ("eval_tol", ctypes.c_double),
        ("noise_prob_g", ctypes.c_void_p), ("sweep_gamma", ctypes.c_void_p), ("policy", ctypes.c_void_p),
        ("cell_rows", ctypes.c_void_p), ("det_cell", ctypes.c_void_p), ("band_lo", ctypes.c_void_p),
        ("band", ctypes.c_void_p), ("noise_reward", ctypes.c_void_p), ("weights", ctypes.c_void_p),
        ("n_tuples", ctypes.POINTER(ctypes.c_int32)),
        ("iters", ctypes.c_void_p), ("sweeps", ctypes.c_void_p), ("n_diff_all", ctypes.c_void_p),
        ("loss_all", ctypes.c_void_p), ("loss_all_mean", ctypes.c_void_p), ("loss_w", ctypes.c_void_p),
        ("diff_w", ctypes.c_void_p), ("v_w", ctypes.c_void_p),
        ("br_policy", ctypes.c_void_p), ("v_opt", ctypes.c_void_p), ("v_pi", ctypes.c_void_p),
    ]


class DeviationNoiseArgs(ctypes.Structure):
    """thrl_deviation_noise_args"""
    _fields_ = [
        ("n_games", ctypes.c_int32), ("flags", ctypes.c_int32), ("n_cells", ctypes.c_int32), ("band_w", ctypes.c_int32),
        ("deviator", ctypes.c_int32), ("dev_len", ctypes.c_int32), ("n_steps", ctypes.c_int32),
        ("dev_action", ctypes.c_int32), ("row_begin", ctypes.c_int32), ("row_count", ctypes.c_int32),
        ("noise_prob", ctypes.c_double), ("ret_tol", ctypes.c_double),
        ("noise_prob_g", ctypes.c_void_p), ("sweep_gamma", ctypes.c_void_p), ("policy", ctypes.c_void_p),
        ("cell_rows", ctypes.c_void_p), ("det_cell", ctypes.c_void_p), ("band_lo", ctypes.c_void_p),
        ("band", ctypes.c_void_p), ("noise_reward", ctypes.c_void_p), ("weights", ctypes.c_void_p),
        ("n_tuples", ctypes.POINTER(ctypes.c_int32)),
        ("base_reward", ctypes.c_void_p), ("base_action", ctypes.c_void_p), ("dev_share", ctypes.c_void_p),
        ("gain", ctypes.c_void_p), ("gain_dev", ctypes.c_void_p), ("low", ctypes.c_void_p),
        ("low_step", ctypes.c_void_p), ("ret_step", ctypes.c_void_p), ("dist", ctypes.c_void_p), ("mass", ctypes.c_void_p),
        ("reward_rows", ctypes.c_void_p), ("action_rows", ctypes.c_void_p), ("dist_rows", ctypes.c_void_p),
    ]


TP_MAX_TUPLES = 4096


class TuplePolicyArgs(ctypes.Structure):
    """thrl_tuple_policy_args"""
    _fields_ = [
        ("n_games", ctypes.c_int32), ("n_tuples", ctypes.c_int32),
        ("kind", ctypes.c_int32 * MAXA), ("nn_params", ctypes.c_void_p * MAXA),
        ("price", ctypes.c_void_p), ("tuple_policy", ctypes.c_void_p),
    ]


class TupleWalkArgs(ctypes.Structure):
    """thrl_tuple_walk_args"""
    _fields_ = [
        ("n_games", ctypes.c_int32), ("n_matches", ctypes.c_int32), ("n_tuples", ctypes.c_int32),
        ("n_steps", ctypes.c_int32), ("horizon", ctypes.c_int32), ("row_begin", ctypes.c_int32),
        ("row_count", ctypes.c_int32), ("reserved", ctypes.c_int32),
        ("seat", ctypes.c_void_p), ("start", ctypes.c_void_p), ("tuple_policy", ctypes.c_void_p),
        ("reward", ctypes.c_void_p), ("scaled", ctypes.c_void_p),
        ("mu", ctypes.c_void_p), ("lam", ctypes.c_void_p), ("cycle_start", ctypes.c_void_p),
        ("cycle_reward", ctypes.c_void_p), ("cycle_action", ctypes.c_void_p),
        ("reward_rows", ctypes.c_void_p), ("action_rows", ctypes.c_void_p),
    ]


class TupleDeviationArgs(ctypes.Structure):
    """thrl_tuple_deviation_args"""
    _fields_ = [
        ("n_games", ctypes.c_int32), ("n_tuples", ctypes.c_int32), ("deviator", ctypes.c_int32),
        ("dev_len", ctypes.c_int32), ("n_steps", ctypes.c_int32), ("horizon", ctypes.c_int32),
        ("dev_action", ctypes.c_int32), ("row_begin", ctypes.c_int32), ("row_count", ctypes.c_int32),
        ("reserved", ctypes.c_int32),
        ("start", ctypes.c_void_p), ("tuple_policy", ctypes.c_void_p), ("reward", ctypes.c_void_p),
        ("scaled", ctypes.c_void_p), ("sweep_gamma", ctypes.c_void_p),
        ("mu", ctypes.c_void_p), ("lam", ctypes.c_void_p), ("mu_post", ctypes.c_void_p), ("lam_post", ctypes.c_void_p),
        ("ret_step", ctypes.c_void_p), ("act_dev", ctypes.c_void_p),
        ("cycle_reward", ctypes.c_void_p), ("cycle_action", ctypes.c_void_p), ("gain", ctypes.c_void_p),
        ("reward_rows", ctypes.c_void_p), ("action_rows", ctypes.c_void_p),
    ]


class TupleEquilibriumArgs(ctypes.Structure):
    """thrl_tuple_equilibrium_args"""
    _fields_ = [
        ("n_games", ctypes.c_int32), ("n_tuples", ctypes.c_int32), ("agents", ctypes.c_int32),
        ("reserved", ctypes.c_int32),
        ("start", ctypes.c_void_p), ("tuple_policy", ctypes.c_void_p), ("reward", ctypes.c_void_p),
        ("sweep_gamma", ctypes.c_void_p),
        ("mu", ctypes.c_void_p), ("lam", ctypes.c_void_p), ("iters", ctypes.c_void_p),
        ("n_diff_all", ctypes.c_void_p), ("n_diff_on", ctypes.c_void_p),
        ("loss_all", ctypes.c_void_p), ("loss_on", ctypes.c_void_p), ("loss_all_mean", ctypes.c_void_p),
        ("loss_on_mean", ctypes.c_void_p), ("v_on", ctypes.c_void_p),
        ("br_policy", ctypes.c_void_p), ("v_opt", ctypes.c_void_p), ("v_pi", ctypes.c_void_p),
    ]


class TupleAttractorsArgs(ctypes.Structure):
    """thrl_tuple_attractors_args"""
    _fields_ = [
        ("n_games", ctypes.c_int32), ("n_tuples", ctypes.c_int32), ("reserved", ctypes.c_int32),
        ("reserved2", ctypes.c_int32),
        ("start", ctypes.c_void_p), ("tuple_policy", ctypes.c_void_p), ("reward", ctypes.c_void_p),
        ("scaled", ctypes.c_void_p), ("start_w", ctypes.c_void_p),
        ("n_attr", ctypes.c_void_p), ("mu_max", ctypes.c_void_p), ("n_cycle_states", ctypes.c_void_p),
        ("rep", ctypes.c_void_p), ("lam", ctypes.c_void_p), ("basin", ctypes.c_void_p),
        ("cycle_reward", ctypes.c_void_p), ("cycle_action", ctypes.c_void_p),
        ("rep_x0", ctypes.c_void_p), ("mu_x0", ctypes.c_void_p), ("slot_x0", ctypes.c_void_p),
        ("start_mass", ctypes.c_void_p), ("start_mass_other", ctypes.c_void_p), ("start_reward", ctypes.c_void_p),
        ("tuple_rep", ctypes.c_void_p), ("tuple_mu", ctypes.c_void_p),
    ]


PP_PER_GAME = 1
TS_START_TUPLE = 1


class PricePolicyArgs(ctypes.Structure):
    """thrl_price_policy_args"""
    _fields_ = [
        ("n_games", ctypes.c_int32), ("n_prices", ctypes.c_int32), ("flags", ctypes.c_int32), ("reserved", ctypes.c_int32),
        ("kind", ctypes.c_int32 * MAXA), ("nn_params", ctypes.c_void_p * MAXA),
        ("price", ctypes.c_void_p), ("price_policy", ctypes.c_void_p),
    ]


class TupleStationaryArgs(ctypes.Structure):
    """thrl_tuple_stationary_args"""
    _fields_ = [
        ("n_games", ctypes.c_int32), ("n_tuples", ctypes.c_int32), ("n_cells", ctypes.c_int32), ("band_w", ctypes.c_int32),
        ("max_iters", ctypes.c_int32), ("flags", ctypes.c_int32), ("kind", ctypes.c_int32 * MAXA),
        ("noise_prob", ctypes.c_double), ("tol", ctypes.c_double),
        ("noise_prob_g", ctypes.c_void_p), ("start", ctypes.c_void_p), ("tuple_policy", ctypes.c_void_p),
        ("cell_policy", ctypes.c_void_p), ("cell_w", ctypes.c_void_p), ("reward", ctypes.c_void_p),
        ("scaled", ctypes.c_void_p), ("price", ctypes.c_void_p), ("band_lo", ctypes.c_void_p), ("band", ctypes.c_void_p),
        ("noise_reward", ctypes.c_void_p), ("noise_price", ctypes.c_void_p),
        ("iters", ctypes.c_void_p), ("change", ctypes.c_void_p), ("mass", ctypes.c_void_p),
        ("stat_reward", ctypes.c_void_p), ("stat_action", ctypes.c_void_p), ("stat_price", ctypes.c_void_p),
        ("pi", ctypes.c_void_p), ("n_switch", ctypes.c_void_p), ("unresolved", ctypes.c_void_p),
    ]


TEN_MAX_LDS = 160 * 1024


class TupleEquilibriumNoiseArgs(ctypes.Structure):
    """thrl_tuple_equilibrium_noise_args"""
    _fields_ = [
        ("n_games", ctypes.c_int32), ("n_tuples", ctypes.c_int32), ("n_cells", ctypes.c_int32), ("band_w", ctypes.c_int32),
        ("max_sweeps", ctypes.c_int32), ("agents", ctypes.c_int32), ("flags", ctypes.c_int32), ("reserved", ctypes.c_int32),
        ("kind", ctypes.c_int32 * MAXA), ("gamma", ctypes.c_double * MAXA),
        ("noise_prob", ctypes.c_double), ("eval_tol", ctypes.c_double),
        ("noise_prob_g", ctypes.c_void_p), ("sweep_gamma", ctypes.c_void_p), ("tuple_policy", ctypes.c_void_p),
        ("cell_policy", ctypes.c_void_p), ("reward", ctypes.c_void_p), ("band_lo", ctypes.c_void_p),
        ("band", ctypes.c_void_p), ("noise_reward", ctypes.c_void_p), ("pi", ctypes.c_void_p),
        ("iters", ctypes.c_void_p), ("sweeps", ctypes.c_void_p), ("n_diff_tuples", ctypes.c_void_p),
        ("n_diff_cells", ctypes.c_void_p),
        ("loss_all", ctypes.c_void_p), ("loss_tuples_mean", ctypes.c_void_p), ("loss_cells_mean", ctypes.c_void_p),
        ("loss_w", ctypes.c_void_p), ("diff_w", ctypes.c_void_p), ("v_w", ctypes.c_void_p),
        ("br_policy", ctypes.c_void_p), ("v_opt", ctypes.c_void_p), ("v_pi", ctypes.c_void_p),
    ]


TDN_MAX_LDS = 160 * 1024


class TupleDeviationNoiseArgs(ctypes.Structure):
    """thrl_tuple_deviation_noise_args"""
    _fields_ = [
        ("n_games", ctypes.c_int32), ("n_tuples", ctypes.c_int32), ("n_cells", ctypes.c_int32), ("band_w", ctypes.c_int32),
        ("deviator", ctypes.c_int32), ("dev_len", ctypes.c_int32), ("n_steps", ctypes.c_int32),
        ("dev_action", ctypes.c_int32), ("row_begin", ctypes.c_int32), ("row_count", ctypes.c_int32),
        ("flags", ctypes.c_int32), ("reserved", ctypes.c_int32), ("kind", ctypes.c_int32 * MAXA),
        ("noise_prob", ctypes.c_double), ("ret_tol", ctypes.c_double),
        ("noise_prob_g", ctypes.c_void_p), ("sweep_gamma", ctypes.c_void_p), ("tuple_policy", ctypes.c_void_p),
        ("cell_policy", ctypes.c_void_p), ("reward", ctypes.c_void_p), ("scaled", ctypes.c_void_p),
        ("band_lo", ctypes.c_void_p), ("band", ctypes.c_void_p), ("noise_reward", ctypes.c_void_p),
        ("weights", ctypes.c_void_p),
        ("base_reward", ctypes.c_void_p), ("base_action", ctypes.c_void_p), ("dev_share", ctypes.c_void_p),
        ("gain", ctypes.c_void_p), ("gain_dev", ctypes.c_void_p), ("low", ctypes.c_void_p),
        ("low_step", ctypes.c_void_p), ("ret_step", ctypes.c_void_p), ("dist", ctypes.c_void_p), ("mass", ctypes.c_void_p),
        ("reward_rows", ctypes.c_void_p), ("action_rows", ctypes.c_void_p), ("dist_rows", ctypes.c_void_p),
    ]


SP_START_TUPLE = 1
SP_MAX_LDS = 160 * 1024


class PriceProbsArgs(ctypes.Structure):
    """thrl_price_probs_args"""
    _fields_ = [
        ("n_games", ctypes.c_int32), ("n_prices", ctypes.c_int32), ("flags", ctypes.c_int32), ("reserved", ctypes.c_int32),
        ("kind", ctypes.c_int32 * MAXA), ("nn_params", ctypes.c_void_p * MAXA),
        ("price", ctypes.c_void_p), ("prob", ctypes.c_void_p * MAXA),
    ]


class SampledChainArgs(ctypes.Structure):
    """thrl_sampled_chain_args"""
    _fields_ = [
        ("n_games", ctypes.c_int32), ("n_tuples", ctypes.c_int32), ("n_prices", ctypes.c_int32),
        ("max_iters", ctypes.c_int32), ("flags", ctypes.c_int32), ("reserved", ctypes.c_int32),
        ("kind", ctypes.c_int32 * MAXA), ("eps", ctypes.c_double * MAXA), ("tol", ctypes.c_double),
        ("eps_g", ctypes.c_void_p), ("start", ctypes.c_void_p), ("prob", ctypes.c_void_p * MAXA),
        ("dpolicy", ctypes.c_void_p), ("grp_first", ctypes.c_void_p), ("grp_perm", ctypes.c_void_p),
        ("reward", ctypes.c_void_p), ("scaled", ctypes.c_void_p), ("price", ctypes.c_void_p),
        ("iters", ctypes.c_void_p), ("change", ctypes.c_void_p), ("mass", ctypes.c_void_p),
        ("samp_reward", ctypes.c_void_p), ("samp_action", ctypes.c_void_p), ("samp_price", ctypes.c_void_p),
        ("agree", ctypes.c_void_p), ("pi", ctypes.c_void_p),
    ]


SPN_START_TUPLE = 1
SPN_START_RESET = 2
SPN_TILE = 64


class SampledNoiseChainArgs(ctypes.Structure):
    """thrl_sampled_noise_chain_args"""
    _fields_ = [
        ("n_games", ctypes.c_int32), ("n_tuples", ctypes.c_int32), ("n_prices", ctypes.c_int32), ("n_nodes", ctypes.c_int32),
        ("band_w", ctypes.c_int32), ("max_iters", ctypes.c_int32), ("flags", ctypes.c_int32), ("reserved", ctypes.c_int32),
        ("kind", ctypes.c_int32 * MAXA), ("eps", ctypes.c_double * MAXA), ("tol", ctypes.c_double),
        ("noise_prob", ctypes.c_double),
        ("eps_g", ctypes.c_void_p), ("noise_prob_g", ctypes.c_void_p), ("start", ctypes.c_void_p),
        ("prob", ctypes.c_void_p * MAXA), ("nprob", ctypes.c_void_p * MAXA),
        ("dpolicy", ctypes.c_void_p), ("npolicy", ctypes.c_void_p), ("grp_first", ctypes.c_void_p), ("grp_perm", ctypes.c_void_p),
        ("reward", ctypes.c_void_p), ("scaled", ctypes.c_void_p), ("price", ctypes.c_void_p),
        ("band_lo", ctypes.c_void_p), ("band", ctypes.c_void_p), ("noise_price", ctypes.c_void_p),
        ("noise_reward", ctypes.c_void_p), ("node_w", ctypes.c_void_p),
        ("iters", ctypes.c_void_p), ("change", ctypes.c_void_p), ("mass", ctypes.c_void_p),
        ("samp_reward", ctypes.c_void_p), ("samp_action", ctypes.c_void_p), ("samp_price", ctypes.c_void_p),
        ("agree", ctypes.c_void_p), ("pi", ctypes.c_void_p), ("max_jump", ctypes.c_void_p),
    ]


SR_MAX_LDS = 160 * 1024


class SampledResponseArgs(ctypes.Structure):
    """thrl_sampled_response_args (include/thrl_response.h)"""
    _fields_ = [
        ("n_games", ctypes.c_int32), ("n_tuples", ctypes.c_int32), ("n_prices", ctypes.c_int32), ("agents", ctypes.c_int32),
        ("max_sweeps", ctypes.c_int32), ("flags", ctypes.c_int32), ("reserved", ctypes.c_int32 * 2),
        ("kind", ctypes.c_int32 * MAXA), ("eps", ctypes.c_double * MAXA), ("gamma", ctypes.c_double * MAXA),
        ("eval_tol", ctypes.c_double),
        ("eps_g", ctypes.c_void_p), ("sweep_gamma", ctypes.c_void_p), ("prob", ctypes.c_void_p * MAXA),
        ("dpolicy", ctypes.c_void_p), ("grp_first", ctypes.c_void_p), ("grp_perm", ctypes.c_void_p),
        ("reward", ctypes.c_void_p), ("pi", ctypes.c_void_p),
        ("iters", ctypes.c_void_p), ("sweeps", ctypes.c_void_p), ("n_diff", ctypes.c_void_p),
        ("loss_all", ctypes.c_void_p), ("loss_mean", ctypes.c_void_p), ("loss_w", ctypes.c_void_p),
        ("gain_w", ctypes.c_void_p), ("v_w", ctypes.c_void_p), ("br_prob_w", ctypes.c_void_p),
        ("br_policy", ctypes.c_void_p), ("v_opt", ctypes.c_void_p), ("v_pi", ctypes.c_void_p),
    ]


SRN_MAX_LDS = 160 * 1024


class SampledResponseNoiseArgs(ctypes.Structure):
    """thrl_sampled_response_noise_args (include/thrl_response_noise.h)"""
    _fields_ = [
        ("n_games", ctypes.c_int32), ("n_tuples", ctypes.c_int32), ("n_prices", ctypes.c_int32), ("n_nodes", ctypes.c_int32),
        ("band_w", ctypes.c_int32), ("agents", ctypes.c_int32), ("max_sweeps", ctypes.c_int32), ("flags", ctypes.c_int32),
        ("reserved", ctypes.c_int32 * 2),
        ("kind", ctypes.c_int32 * MAXA), ("eps", ctypes.c_double * MAXA), ("gamma", ctypes.c_double * MAXA),
        ("eval_tol", ctypes.c_double), ("noise_prob", ctypes.c_double),
        ("eps_g", ctypes.c_void_p), ("sweep_gamma", ctypes.c_void_p), ("noise_prob_g", ctypes.c_void_p),
        ("prob", ctypes.c_void_p * MAXA), ("nprob", ctypes.c_void_p * MAXA),
        ("dpolicy", ctypes.c_void_p), ("npolicy", ctypes.c_void_p), ("grp_first", ctypes.c_void_p), ("grp_perm", ctypes.c_void_p),
        ("reward", ctypes.c_void_p), ("band_lo", ctypes.c_void_p), ("band", ctypes.c_void_p), ("noise_reward", ctypes.c_void_p),
        ("pi", ctypes.c_void_p),
        ("iters", ctypes.c_void_p), ("sweeps", ctypes.c_void_p), ("n_diff_prices", ctypes.c_void_p),
        ("n_diff_nodes", ctypes.c_void_p), ("loss_all", ctypes.c_void_p), ("loss_prices_mean", ctypes.c_void_p),
        ("loss_nodes_mean", ctypes.c_void_p), ("loss_w", ctypes.c_void_p), ("gain_w", ctypes.c_void_p), ("v_w", ctypes.c_void_p),
        ("br_prob_w", ctypes.c_void_p), ("br_policy", ctypes.c_void_p), ("v_opt", ctypes.c_void_p), ("v_pi", ctypes.c_void_p),
    ]


SD_POLICY = 1
SD_MAX_LDS = 160 * 1024


class SampledDeviationArgs(ctypes.Structure):
    """thrl_sampled_deviation_args (include/thrl_sampled_deviation.h)"""
    _fields_ = [
        ("n_games", ctypes.c_int32), ("n_tuples", ctypes.c_int32), ("n_prices", ctypes.c_int32), ("deviator", ctypes.c_int32),
        ("dev_len", ctypes.c_int32), ("n_steps", ctypes.c_int32), ("dev_action", ctypes.c_int32),
        ("row_begin", ctypes.c_int32), ("row_count", ctypes.c_int32), ("flags", ctypes.c_int32),
        ("reserved", ctypes.c_int32 * 2),
        ("kind", ctypes.c_int32 * MAXA), ("eps", ctypes.c_double * MAXA), ("gamma", ctypes.c_double),
        ("ret_tol", ctypes.c_double),
        ("eps_g", ctypes.c_void_p), ("sweep_gamma", ctypes.c_void_p), ("prob", ctypes.c_void_p * MAXA),
        ("dpolicy", ctypes.c_void_p), ("dev_policy", ctypes.c_void_p), ("grp_first", ctypes.c_void_p),
        ("grp_perm", ctypes.c_void_p), ("reward", ctypes.c_void_p), ("scaled", ctypes.c_void_p), ("price", ctypes.c_void_p),
        ("weights", ctypes.c_void_p),
        ("base_reward", ctypes.c_void_p), ("base_action", ctypes.c_void_p), ("base_price", ctypes.c_void_p),
        ("dev_share", ctypes.c_void_p), ("gain", ctypes.c_void_p), ("gain_dev", ctypes.c_void_p), ("low", ctypes.c_void_p),
        ("low_step", ctypes.c_void_p), ("ret_step", ctypes.c_void_p), ("dist", ctypes.c_void_p), ("mass", ctypes.c_void_p),
        ("reward_rows", ctypes.c_void_p), ("action_rows", ctypes.c_void_p), ("price_rows", ctypes.c_void_p),
        ("dist_rows", ctypes.c_void_p),
    ]


SDN_POLICY = 1
SDN_MAX_LDS = 160 * 1024


class SampledDeviationNoiseArgs(ctypes.Structure):
    """thrl_sampled_deviation_noise_args (include/thrl_sampled_deviation_noise.h)"""
    _fields_ = [
        ("n_games", ctypes.c_int32), ("n_tuples", ctypes.c_int32), ("n_prices", ctypes.c_int32), ("n_nodes", ctypes.c_int32),
        ("band_w", ctypes.c_int32), ("deviator", ctypes.c_int32), ("dev_len", ctypes.c_int32), ("n_steps", ctypes.c_int32),
        ("dev_action", ctypes.c_int32), ("row_begin", ctypes.c_int32), ("row_count", ctypes.c_int32), ("flags", ctypes.c_int32),
        ("reserved", ctypes.c_int32 * 2),
        ("kind", ctypes.c_int32 * MAXA), ("eps", ctypes.c_double * MAXA), ("gamma", ctypes.c_double),
        ("ret_tol", ctypes.c_double), ("noise_prob", ctypes.c_double),
        ("eps_g", ctypes.c_void_p), ("sweep_gamma", ctypes.c_void_p), ("noise_prob_g", ctypes.c_void_p),
        ("prob", ctypes.c_void_p * MAXA), ("nprob", ctypes.c_void_p * MAXA),
        ("dpolicy", ctypes.c_void_p), ("npolicy", ctypes.c_void_p), ("dev_policy", ctypes.c_void_p),
        ("grp_first", ctypes.c_void_p), ("grp_perm", ctypes.c_void_p), ("reward", ctypes.c_void_p), ("scaled", ctypes.c_void_p),
        ("price", ctypes.c_void_p), ("band_lo", ctypes.c_void_p), ("band", ctypes.c_void_p), ("noise_price", ctypes.c_void_p),
        ("noise_reward", ctypes.c_void_p), ("weights", ctypes.c_void_p),
        ("base_reward", ctypes.c_void_p), ("base_action", ctypes.c_void_p), ("base_price", ctypes.c_void_p),
        ("dev_share", ctypes.c_void_p), ("gain", ctypes.c_void_p), ("gain_dev", ctypes.c_void_p), ("low", ctypes.c_void_p),
        ("low_step", ctypes.c_void_p), ("ret_step", ctypes.c_void_p), ("dist", ctypes.c_void_p), ("mass", ctypes.c_void_p),
        ("reward_rows", ctypes.c_void_p), ("action_rows", ctypes.c_void_p), ("price_rows", ctypes.c_void_p),
        ("dist_rows", ctypes.c_void_p),
    ]


# every symbol include/thrl.h declares (tests check the library exports all of them)
SYMBOLS = [
    "thrl_version", "thrl_last_error", "thrl_build_info", "thrl_ablate_mask", "thrl_table_stride", "thrl_table_offset",
    "thrl_replay_mem_bytes", "thrl_workspace_bytes", "thrl_select_kernel", "thrl_wave_play_form", "thrl_training_cycle", "thrl_qtable_init",
    "thrl_qtable_episodes", "thrl_play_greedy", "thrl_op_sample_action", "thrl_op_encode", "thrl_op_scale",
    "thrl_op_env_step", "thrl_op_td_update",
    "thrl_nn_param_count", "thrl_nn_init", "thrl_nn_act", "thrl_nn_reinforce_train", "thrl_op_draws",
    "thrl_mixed_episodes", "thrl_mixed_policy_table_bytes", "thrl_ac_param_count", "thrl_ac_init", "thrl_ac_act", "thrl_ac_train",
    "thrl_cac_init", "thrl_cac_act", "thrl_cac_train", "thrl_group_stats", "thrl_ewm_rows", "thrl_deviation",
    "thrl_policy_track", "thrl_equilibrium", "thrl_crossplay", "thrl_attractors", "thrl_stationary",
    "thrl_equilibrium_noise", "thrl_deviation_noise",
    "thrl_tuple_policy", "thrl_tuple_walk", "thrl_tuple_deviation", "thrl_tuple_equilibrium",
    "thrl_tuple_attractors", "thrl_price_policy", "thrl_tuple_stationary", "thrl_tuple_equilibrium_noise", "thrl_tuple_deviation_noise", "thrl_price_probs", "thrl_sampled_chain",
    "thrl_sampled_noise_chain",
]
# every symbol include/thrl_response.h declares
RESPONSE_SYMBOLS = ["thrl_sampled_response"]
# every symbol include/thrl_response_noise.h declares
RESPONSE_NOISE_SYMBOLS = ["thrl_sampled_response_noise"]
# every symbol include/thrl_sampled_deviation.h declares
SAMPLED_DEVIATION_SYMBOLS = ["thrl_sampled_deviation"]
# every symbol include/thrl_sampled_deviation_noise.h declares
SAMPLED_DEVIATION_NOISE_SYMBOLS = ["thrl_sampled_deviation_noise"]
CAC_PARAMS = 1283

_lib = None


def _share_hip_runtime_with_torch():
    """PyTorch-ROCm bundles its own libamdhip64.so (SONAME libamdhip64.so.7).  Device
    pointers and streams are only meaningful inside ONE HIP runtime instance, so torch
    must be imported first and its runtime made globally visible; libthrl_hip.so's
    NEEDED libamdhip64.so.7 then binds to that same instance instead of /opt/rocm's."""
    try:
        import torch
    except ImportError as e:
        raise ThrlError("th_rl_amd needs PyTorch-ROCm (device memory / streams): %s" % e)
    cand = os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so")
    if os.path.exists(cand):
        ctypes.CDLL(cand, mode=ctypes.RTLD_GLOBAL)


def load():
    """Load libthrl_hip.so; raises ThrlError (never falls back) if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ThrlError(
            "th_rl_amd: %s not found. Build it with `python -m th_rl_amd.build` "
            "(hipcc, gfx950). There is no CPU fallback." % LIB_PATH)
    _share_hip_runtime_with_torch()
    try:
        L = ctypes.CDLL(LIB_PATH)
    except OSError as e:
        raise ThrlError("th_rl_amd: cannot load %s: %s" % (LIB_PATH, e))
    vp, i32, u64, dbl = ctypes.c_void_p, ctypes.c_int32, ctypes.c_uint64, ctypes.c_double
    cfgp = ctypes.POINTER(Cfg)
    L.thrl_version.restype = ctypes.c_int
    L.thrl_last_error.restype = ctypes.c_char_p
    L.thrl_build_info.restype = ctypes.c_char_p
    L.thrl_ablate_mask.restype = ctypes.c_int
    for n in ("thrl_table_stride", "thrl_replay_mem_bytes", "thrl_workspace_bytes"):
        getattr(L, n).restype = ctypes.c_size_t
        getattr(L, n).argtypes = [cfgp]
    L.thrl_table_offset.restype = ctypes.c_size_t
    L.thrl_table_offset.argtypes = [cfgp, ctypes.c_int]
    L.thrl_select_kernel.restype = ctypes.c_int
    L.thrl_select_kernel.argtypes = [cfgp, ctypes.c_int]
    if hasattr(L, "thrl_wave_play_form"):       # (an older build loaded through THRL_LIB for an A/B run lacks it)
        L.thrl_wave_play_form.restype = ctypes.c_int
        L.thrl_wave_play_form.argtypes = [cfgp, ctypes.POINTER(ctypes.c_int * 3)]
    L.thrl_training_cycle.restype = ctypes.c_int
    L.thrl_training_cycle.argtypes = [cfgp]
    L.thrl_qtable_init.restype = ctypes.c_int
    L.thrl_qtable_init.argtypes = [cfgp, vp, vp, vp, u64, u64, vp, vp]
    L.thrl_qtable_episodes.restype = ctypes.c_int
    L.thrl_qtable_episodes.argtypes = [cfgp, ctypes.POINTER(Buffers), ctypes.POINTER(Run), vp]
    L.thrl_play_greedy.restype = ctypes.c_int
    L.thrl_play_greedy.argtypes = [cfgp, vp, vp, i32, u64, u64, vp, vp, vp]
    L.thrl_op_sample_action.restype = ctypes.c_int
    # (choice: device int32 [G] since ABI v4 -- an int8 buffer here is read four games to the word)
    L.thrl_op_sample_action.argtypes = [cfgp, ctypes.c_int, vp, vp, dbl, vp, vp, ctypes.c_int, vp, vp]
    L.thrl_op_env_step.restype = ctypes.c_int
    L.thrl_op_env_step.argtypes = [cfgp, vp, vp, vp, vp, vp, vp]
    L.thrl_op_encode.restype = ctypes.c_int
    L.thrl_op_encode.argtypes = [cfgp, ctypes.c_int, vp, ctypes.c_int, vp, vp]
    L.thrl_op_scale.restype = ctypes.c_int
    L.thrl_op_scale.argtypes = [cfgp, ctypes.c_int, vp, vp, vp]
    L.thrl_op_td_update.restype = ctypes.c_int
    L.thrl_op_td_update.argtypes = [cfgp, ctypes.c_int, vp, vp, i32, vp, vp, vp, vp, vp, vp]
    L.thrl_nn_param_count.restype = ctypes.c_size_t
    L.thrl_nn_param_count.argtypes = [ctypes.c_int]
    L.thrl_nn_init.restype = ctypes.c_int
    L.thrl_nn_init.argtypes = [ctypes.c_int, ctypes.c_int, vp, u64, u64, ctypes.c_int, vp]
    L.thrl_nn_act.restype = ctypes.c_int
    L.thrl_nn_act.argtypes = [ctypes.c_int, ctypes.c_int, vp, vp, vp, vp, vp, vp]
    L.thrl_nn_reinforce_train.restype = ctypes.c_int
    L.thrl_nn_reinforce_train.argtypes = [ctypes.c_int, ctypes.c_int, vp, vp, vp, i32, i32, i32, vp, vp, vp,
                                          dbl, dbl, dbl, vp, vp, vp, vp, vp]
    L.thrl_op_draws.restype = ctypes.c_int
    # (choice_out: device int32 [N][G] since ABI v4)
    L.thrl_op_draws.argtypes = [cfgp, u64, u64, u64, i32, vp, vp, vp, vp, vp, vp]
    L.thrl_cac_init.restype = ctypes.c_int
    L.thrl_cac_init.argtypes = [ctypes.c_int, vp, u64, u64, ctypes.c_int, vp]
    L.thrl_cac_act.restype = ctypes.c_int
    L.thrl_cac_act.argtypes = [ctypes.c_int, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.thrl_cac_train.restype = ctypes.c_int
    L.thrl_cac_train.argtypes = [ctypes.c_int, vp, vp, vp, i32, i32, i32, vp, vp, vp, vp,
                                 ctypes.c_double, ctypes.c_double, ctypes.c_double, vp, vp, vp, vp]
    L.thrl_ac_param_count.restype = ctypes.c_size_t
    L.thrl_ac_param_count.argtypes = [ctypes.c_int]
    L.thrl_ac_init.restype = ctypes.c_int
    L.thrl_ac_init.argtypes = L.thrl_nn_init.argtypes
    L.thrl_ac_act.restype = ctypes.c_int
    L.thrl_ac_act.argtypes = L.thrl_nn_act.argtypes
    L.thrl_ac_train.restype = ctypes.c_int
    L.thrl_ac_train.argtypes = [ctypes.c_int, ctypes.c_int, vp, vp, vp, i32, i32, i32, vp, vp, vp, vp,
                                ctypes.c_double, ctypes.c_double, ctypes.c_double, vp, vp, vp, vp]
    L.thrl_mixed_policy_table_bytes.restype = ctypes.c_size_t
    L.thrl_mixed_policy_table_bytes.argtypes = [cfgp, ctypes.POINTER(Mixed)]
    L.thrl_mixed_episodes.restype = ctypes.c_int
    L.thrl_mixed_episodes.argtypes = [cfgp, ctypes.POINTER(Mixed), vp, vp, vp, ctypes.POINTER(Run), vp, vp, vp]
    L.thrl_group_stats.restype = ctypes.c_int
    L.thrl_group_stats.argtypes = [ctypes.POINTER(GroupStatsArgs), vp]
    L.thrl_ewm_rows.restype = ctypes.c_int
    L.thrl_ewm_rows.argtypes = [ctypes.POINTER(EwmRowsArgs), vp]
    L.thrl_deviation.restype = ctypes.c_int
    L.thrl_deviation.argtypes = [cfgp, vp, ctypes.POINTER(DeviationArgs), vp]
    L.thrl_policy_track.restype = ctypes.c_int
    L.thrl_policy_track.argtypes = [cfgp, vp, ctypes.POINTER(PolicyTrackArgs), vp]
    L.thrl_equilibrium.restype = ctypes.c_int
    L.thrl_equilibrium.argtypes = [cfgp, vp, ctypes.POINTER(EquilibriumArgs), vp]
    L.thrl_crossplay.restype = ctypes.c_int
    L.thrl_crossplay.argtypes = [cfgp, vp, ctypes.POINTER(CrossplayArgs), vp]
    L.thrl_attractors.restype = ctypes.c_int
    L.thrl_attractors.argtypes = [cfgp, vp, ctypes.POINTER(AttractorsArgs), vp]
    L.thrl_stationary.restype = ctypes.c_int
    L.thrl_stationary.argtypes = [cfgp, vp, ctypes.POINTER(StationaryArgs), vp]
    L.thrl_equilibrium_noise.restype = ctypes.c_int
    L.thrl_equilibrium_noise.argtypes = [cfgp, vp, ctypes.POINTER(EquilibriumNoiseArgs), vp]
    L.thrl_deviation_noise.restype = ctypes.c_int
    L.thrl_deviation_noise.argtypes = [cfgp, vp, ctypes.POINTER(DeviationNoiseArgs), vp]
    L.thrl_tuple_policy.restype = ctypes.c_int
    L.thrl_tuple_policy.argtypes = [cfgp, vp, ctypes.POINTER(TuplePolicyArgs), vp]
    L.thrl_tuple_walk.restype = ctypes.c_int
    L.thrl_tuple_walk.argtypes = [cfgp, ctypes.POINTER(TupleWalkArgs), vp]
    L.thrl_tuple_deviation.restype = ctypes.c_int
    L.thrl_tuple_deviation.argtypes = [cfgp, ctypes.POINTER(TupleDeviationArgs), vp]
    L.thrl_tuple_equilibrium.restype = ctypes.c_int
    L.thrl_tuple_equilibrium.argtypes = [cfgp, ctypes.POINTER(TupleEquilibriumArgs), vp]
    L.thrl_tuple_attractors.restype = ctypes.c_int
    L.thrl_tuple_attractors.argtypes = [cfgp, ctypes.POINTER(TupleAttractorsArgs), vp]
    L.thrl_price_policy.restype = ctypes.c_int
    L.thrl_price_policy.argtypes = [cfgp, vp, ctypes.POINTER(PricePolicyArgs), vp]
    L.thrl_tuple_stationary.restype = ctypes.c_int
    L.thrl_tuple_stationary.argtypes = [cfgp, ctypes.POINTER(TupleStationaryArgs), vp]
    L.thrl_tuple_equilibrium_noise.restype = ctypes.c_int
    L.thrl_tuple_equilibrium_noise.argtypes = [cfgp, ctypes.POINTER(TupleEquilibriumNoiseArgs), vp]
    L.thrl_tuple_deviation_noise.restype = ctypes.c_int
    L.thrl_tuple_deviation_noise.argtypes = [cfgp, ctypes.POINTER(TupleDeviationNoiseArgs), vp]
    L.thrl_price_probs.restype = ctypes.c_int
    L.thrl_price_probs.argtypes = [cfgp, ctypes.POINTER(PriceProbsArgs), vp]
    L.thrl_sampled_chain.restype = ctypes.c_int
    L.thrl_sampled_chain.argtypes = [cfgp, ctypes.POINTER(SampledChainArgs), vp]
    L.thrl_sampled_noise_chain.restype = ctypes.c_int
    L.thrl_sampled_noise_chain.argtypes = [cfgp, ctypes.POINTER(SampledNoiseChainArgs), vp]
    L.thrl_sampled_response.restype = ctypes.c_int
    L.thrl_sampled_response.argtypes = [cfgp, ctypes.POINTER(SampledResponseArgs), vp]
    L.thrl_sampled_response_noise.restype = ctypes.c_int
    L.thrl_sampled_response_noise.argtypes = [cfgp, ctypes.POINTER(SampledResponseNoiseArgs), vp]
    L.thrl_sampled_deviation.restype = ctypes.c_int
    L.thrl_sampled_deviation.argtypes = [cfgp, ctypes.POINTER(SampledDeviationArgs), vp]
    L.thrl_sampled_deviation_noise.restype = ctypes.c_int
    L.thrl_sampled_deviation_noise.argtypes = [cfgp, ctypes.POINTER(SampledDeviationNoiseArgs), vp]
    if L.thrl_version() != ABI_VERSION:
        raise ThrlError("th_rl_amd: ABI version mismatch (%d)" % L.thrl_version())
    _lib = L
    return L


def build_info():
    """dict(path, abi, ablate, src) of the loaded library (thrl_build_info)."""
    L = load()
    d = dict(kv.split("=", 1) for kv in L.thrl_build_info().decode().split(";"))
    return dict(path=LIB_PATH, abi=int(d["abi"]), ablate=int(d["ablate"]), src=d["src"], wave=d.get("wave"), nn=d.get("nn"))


def check(rc, what):
    if rc != 0:
        msg = load().thrl_last_error().decode("utf-8", "replace")
        err = ThrlError("%s failed (thrl_err %d): %s" % (what, rc, msg))
        err.code = rc
        raise err


# QTable.__init__ defaults (reference th_rl/agents.py:13-27) / NoisyPriceState (environments.py:5)
QTABLE_DEFAULTS = dict(states=16, actions=4, action_range=[0, 1], gamma=0.99, capacity=500,
                       max_state=10, alpha=0.1, eps_end=2e-2, epsilon=0.5, eps_step=5e-4,
                       min_memory=100)
ENV_DEFAULTS = dict(action_range=[0, 1], a=10, b=1, max_steps=1, noise_prob=0.05)


def cfg_from_config(config, n_games, q_dtype):
    """(Cfg, [epsilon_i]) from a reference-schema config dict whose agents are all QTable."""
    agents = config["agents"]
    if len(agents) > MAXA:
        raise ThrlError("at most %d agents per game" % MAXA)
    env = dict(ENV_DEFAULTS, **config["environment"])
    c = Cfg()
    c.n_games = int(n_games)
    c.n_agents = len(agents)
    c.max_steps = int(env["max_steps"])
    c.q_dtype = int(q_dtype)
    c.env_a = float(env["a"])
    c.env_b = float(env["b"])
    c.noise_prob = float(env["noise_prob"])
    eps = []
    for i, a in enumerate(agents):
        if a.get("name", "QTable") != "QTable":
            raise ThrlError("the batched device path handles QTable agents only, got %r" % a.get("name"))
        p = dict(QTABLE_DEFAULTS, **a)
        c.n_states[i] = int(p["states"]); c.n_actions[i] = int(p["actions"])
        c.min_memory[i] = int(p["min_memory"]); c.capacity[i] = int(p["capacity"])
        c.max_state[i] = float(p["max_state"]); c.gamma[i] = float(p["gamma"])
        c.alpha[i] = float(p["alpha"]); c.eps_end[i] = float(p["eps_end"])
        c.eps_step[i] = float(p["eps_step"])
        c.act_lo[i] = float(p["action_range"][0]); c.act_hi[i] = float(p["action_range"][1])
        eps.append(float(p["epsilon"]))
    return c, eps
