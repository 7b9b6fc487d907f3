"""ctypes mirrors of include/vilo_gpu.h / include/vilo_synth.h (plain C-ABI structs, no torch types)."""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_DIR = os.path.join(HERE, "lib")

F = 11  # VILO_MAX_FRAMES
MAX_PRIOR_BLOCKS = 40
MAX_PRIOR_DIM = 96

c_double_p = C.POINTER(C.c_double)
c_int32_p = C.POINTER(C.c_int32)
c_uint8_p = C.POINTER(C.c_uint8)
c_size_t_p = C.POINTER(C.c_size_t)


class Config(C.Structure):
    _fields_ = [
        ("acc_n", C.c_double), ("acc_n_z", C.c_double), ("acc_w", C.c_double), ("gyr_n", C.c_double), ("gyr_w", C.c_double),
        ("g_norm", C.c_double), ("phi_n", C.c_double), ("dphi_n", C.c_double), ("rho_c_n", C.c_double), ("rho_nc_n", C.c_double),
        ("v_n_min_xy", C.c_double), ("v_n_min_z", C.c_double), ("v_n_min", C.c_double), ("v_n_max", C.c_double),
        ("v_n_force_thres_ratio", C.c_double), ("v_n_term1_steep", C.c_double), ("v_n_term2_var_rescale", C.c_double),
        ("v_n_term3_distance_rescale", C.c_double), ("contact_sensor_type", C.c_int32), ("pad0", C.c_int32),
        ("rho_fix", C.c_double * 16), ("p_br", C.c_double * 3), ("R_br", C.c_double * 9),
        ("focal_length", C.c_double), ("huber_delta", C.c_double),
    ]


class Sample(C.Structure):
    _fields_ = [("dt", C.c_double), ("acc", C.c_double * 3), ("gyr", C.c_double * 3), ("phi", C.c_double * 12),
                ("dphi", C.c_double * 12), ("c", C.c_double * 4)]


SAMPLE_DOUBLES = 35
assert C.sizeof(Sample) == 8 * SAMPLE_DOUBLES


class Preint(C.Structure):
    _fields_ = [("sum_dt", C.c_double), ("delta_p", C.c_double * 3), ("delta_q", C.c_double * 4), ("delta_v", C.c_double * 3),
                ("delta_eps", C.c_double * 12), ("lin_ba", C.c_double * 3), ("lin_bg", C.c_double * 3), ("lin_rho", C.c_double * 4),
                ("jacobian", C.c_double * 961), ("covariance", C.c_double * 961)]


PREINT_DOUBLES = 33 + 2 * 961
assert C.sizeof(Preint) == 8 * PREINT_DOUBLES


class PreintImu(C.Structure):
    _fields_ = [("sum_dt", C.c_double), ("delta_p", C.c_double * 3), ("delta_q", C.c_double * 4), ("delta_v", C.c_double * 3),
                ("lin_ba", C.c_double * 3), ("lin_bg", C.c_double * 3), ("jacobian", C.c_double * 225), ("covariance", C.c_double * 225)]


PREINT_IMU_DOUBLES = 17 + 2 * 225
assert C.sizeof(PreintImu) == 8 * PREINT_IMU_DOUBLES


class Prior(C.Structure):
    _fields_ = [("n", C.c_int32), ("n_blocks", C.c_int32), ("block_id", C.c_int32 * MAX_PRIOR_BLOCKS),
                ("block_size", C.c_int32 * MAX_PRIOR_BLOCKS), ("block_idx", C.c_int32 * MAX_PRIOR_BLOCKS),
                ("x0", c_double_p), ("J0", c_double_p), ("r0", c_double_p), ("valid", C.c_int32), ("pad", C.c_int32)]


class WindowDesc(C.Structure):
    _fields_ = [("n_frames", C.c_int32), ("n_landmarks", C.c_int32), ("n_obs", C.c_int32), ("use_leg", C.c_int32),
                ("lm_start_frame", c_int32_p), ("lm_obs_offset", c_int32_p), ("obs", c_double_p), ("obs_is_stereo", c_uint8_p),
                ("preint", C.POINTER(Preint)), ("preint_imu", C.POINTER(PreintImu)), ("prior", C.POINTER(Prior)),
                ("leg_bias_const", C.c_int32), ("ex_const", C.c_int32), ("td_const", C.c_int32), ("pad", C.c_int32)]


class WindowState(C.Structure):
    _fields_ = [("pose", c_double_p), ("speed_bias", c_double_p), ("leg_bias", c_double_p), ("ex_pose", c_double_p),
                ("td", c_double_p), ("inv_depth", c_double_p)]


class SolveOpts(C.Structure):
    _fields_ = [("max_num_iterations", C.c_int32), ("fixed_iterations", C.c_int32),
                ("initial_trust_region_radius", C.c_double), ("max_trust_region_radius", C.c_double),
                ("min_trust_region_radius", C.c_double), ("min_relative_decrease", C.c_double),
                ("function_tolerance", C.c_double), ("gradient_tolerance", C.c_double), ("parameter_tolerance", C.c_double),
                ("min_lm_diagonal", C.c_double), ("max_lm_diagonal", C.c_double), ("jacobi_scaling", C.c_int32),
                ("max_solver_time_us", C.c_int32)]


class SolveSummary(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("num_successful", C.c_int32), ("termination", C.c_int32), ("pad", C.c_int32),
                ("initial_cost", C.c_double), ("final_cost", C.c_double), ("cost_trace", C.c_double * 64),
                ("radius_trace", C.c_double * 64)]


class CovOpts(C.Structure):
    """vilo_cov_opts (24 bytes)"""
    _fields_ = [("gauge", C.c_int32), ("pad0", C.c_int32), ("min_reciprocal_condition", C.c_double), ("want_poses", C.c_int32),
                ("pad1", C.c_int32)]


class ResidualOpts(C.Structure):
    """vilo_residual_opts (8 bytes)"""
    _fields_ = [("outlier_threshold_px", C.c_double)]


class WindowResidual(C.Structure):
    """vilo_window_residual (136 bytes)"""
    _fields_ = [("cost", C.c_double), ("prior_cost", C.c_double), ("imu_cost", C.c_double * 10), ("visual_cost", C.c_double),
                ("visual_cost_plain", C.c_double), ("n_visual_blocks", C.c_int32), ("n_huber_active", C.c_int32),
                ("n_outliers", C.c_int32), ("n_negative_depth", C.c_int32), ("status", C.c_int32), ("pad", C.c_int32)]


class WindowGradient(C.Structure):
    """vilo_window_gradient_record (48 bytes)"""
    _fields_ = [("max_norm", C.c_double), ("norm", C.c_double), ("scaled_max", C.c_double), ("argmax_kind", C.c_int32),
                ("argmax_index", C.c_int32), ("argmax_component", C.c_int32), ("n_free", C.c_int32), ("status", C.c_int32),
                ("pad", C.c_int32)]


class StepOpts(C.Structure):
    """vilo_step_opts (32 bytes)"""
    _fields_ = [("gauge", C.c_int32), ("pad0", C.c_int32), ("min_lm_diagonal", C.c_double), ("max_lm_diagonal", C.c_double),
                ("min_pivot", C.c_double)]


class WindowStepRecord(C.Structure):
    """vilo_window_step_record (40 bytes)"""
    _fields_ = [("model_cost_change", C.c_double), ("scaled_norm", C.c_double), ("norm", C.c_double), ("grad_dot_step", C.c_double),
                ("n_free", C.c_int32), ("status", C.c_int32)]


class DoglegOpts(C.Structure):
    """vilo_dogleg_opts (32 bytes: vilo_step_opts' fields)"""
    _fields_ = list(StepOpts._fields_)


class WindowDoglegRecord(C.Structure):
    """vilo_window_dogleg_record (80 bytes)"""
    _fields_ = [("alpha", C.c_double), ("gradient_norm", C.c_double), ("gauss_newton_norm", C.c_double), ("step_norm", C.c_double),
                ("beta", C.c_double), ("model_cost_change", C.c_double), ("grad_dot_step", C.c_double), ("norm", C.c_double),
                ("branch", C.c_int32), ("n_free", C.c_int32), ("status", C.c_int32), ("pad", C.c_int32)]


HV_MAX_VECTORS = 16  # VILO_HV_MAX_VECTORS


class HessVecRecord(C.Structure):
    """vilo_hess_vec_record (32 bytes)"""
    _fields_ = [("vHv", C.c_double), ("g_dot_v", C.c_double), ("model_cost_change", C.c_double), ("status", C.c_int32), ("pad", C.c_int32)]


TRIAL_MAX_STEPS = 16  # VILO_TRIAL_MAX_STEPS
TRIAL_OK, TRIAL_NUMERIC, TRIAL_INVALID, TRIAL_NOT_FINITE = 0, 1, 2, 3   # vilo_trial_record.status


class TrialRecord(C.Structure):
    """vilo_trial_record (48 bytes)"""
    _fields_ = [("cost", C.c_double), ("visual_cost", C.c_double), ("imu_cost", C.c_double), ("prior_cost", C.c_double),
                ("cost_change", C.c_double), ("n_negative_depth", C.c_int32), ("status", C.c_int32)]


class MaskOpts(C.Structure):
    """vilo_mask_opts (24 bytes)"""
    _fields_ = [("source", C.c_int32), ("combine", C.c_int32), ("flag_bits", C.c_uint32), ("pad", C.c_int32), ("outlier_threshold_px", C.c_double)]


class WindowMask(C.Structure):
    """vilo_window_mask_record (24 bytes)"""
    _fields_ = [("status", C.c_int32), ("n_landmarks", C.c_int32), ("n_masked", C.c_int32), ("n_newly_masked", C.c_int32),
                ("n_obs_left", C.c_int32), ("pad", C.c_int32)]


MASK_SOURCE = {"given": 0, "outlier_flags": 1, "clear": 2}   # VILO_MASK_GIVEN, _OUTLIER_FLAGS, _CLEAR
MASK_COMBINE = {"replace": 0, "or": 1}                        # VILO_MASK_REPLACE, _OR
MASK_OK, MASK_NO_LANDMARKS = 0, 1                             # vilo_window_mask_record.status


class TriangulateOpts(C.Structure):
    """vilo_triangulate_opts (24 bytes)"""
    _fields_ = [("init_depth", C.c_double), ("stereo", C.c_int32), ("select", C.c_int32), ("write", C.c_int32), ("pad", C.c_int32)]


TRI_SELECT = {"unset": 0, "all": 1, "mask": 2}   # VILO_TRI_*
TRI_SELECTED, TRI_STEREO, TRI_FALLBACK, TRI_NOT_FINITE = 1, 2, 4, 8   # bits of a landmark's flags

class PnpOpts(C.Structure):
    """vilo_pnp_opts (24 bytes)"""
    _fields_ = [("frame", C.c_int32), ("guess", C.c_int32), ("write", C.c_int32), ("max_iterations", C.c_int32),
                ("step_tolerance", C.c_double)]


class WindowPnpRecord(C.Structure):
    """vilo_window_pnp_record (32 bytes)"""
    _fields_ = [("final_cost", C.c_double), ("initial_cost", C.c_double), ("n_points", C.c_int32), ("iterations", C.c_int32),
                ("status", C.c_int32), ("pad", C.c_int32)]


PNP_GUESS = {"previous": 0, "current": 1}   # VILO_PNP_GUESS_*
PNP_OK, PNP_NOT_ENOUGH_POINTS, PNP_NO_CONVERGENCE, PNP_NUMERIC, PNP_NO_FRAME = 0, 1, 2, 3, 4   # a window's status (VILO_PNP_*)
MAX_FRAMES = 11   # VILO_MAX_FRAMES

class GyroOpts(C.Structure):
    """vilo_gyro_opts (8 bytes)"""
    _fields_ = [("linearization", C.c_int32), ("write", C.c_int32)]


class WindowGyroRecord(C.Structure):
    """vilo_window_gyro_record (24 bytes)"""
    _fields_ = [("initial_cost", C.c_double), ("model_cost", C.c_double), ("n_intervals", C.c_int32), ("status", C.c_int32)]


GYRO_LINEARIZATION = {"record": 0, "corrected": 1}   # VILO_GYRO_RECORD / VILO_GYRO_CORRECTED
GYRO_OK, GYRO_NO_INTERVALS, GYRO_SINGULAR, GYRO_NUMERIC = 0, 1, 2, 3   # a window's status (VILO_GYRO_*)

class PredictOpts(C.Structure):
    """vilo_predict_opts (8 bytes)"""
    _fields_ = [("mode", C.c_int32), ("pad", C.c_int32)]


class WindowPredictRecord(C.Structure):
    """vilo_window_predict_record (8 bytes)"""
    _fields_ = [("n_predicted", C.c_int32), ("status", C.c_int32)]


PREDICT_MODE = {"constant_velocity": 0, "given": 1}   # VILO_PREDICT_CONSTANT_VELOCITY / VILO_PREDICT_GIVEN
PREDICT_OK, PREDICT_TOO_FEW_FRAMES, PREDICT_NUMERIC = 0, 1, 2   # a window's status (VILO_PREDICT_*)
PREDICT_PREDICTED, PREDICT_BEHIND, PREDICT_NOT_FINITE, PREDICT_BEHIND_RIGHT = 1, 2, 4, 8   # bits of a landmark's flags

class DeadReckonOpts(C.Structure):
    """vilo_dead_reckon_opts (8 bytes)"""
    _fields_ = [("from_frame", C.c_int32), ("write", C.c_int32)]


class WindowDeadReckonRecord(C.Structure):
    """vilo_window_dead_reckon_record (8 bytes)"""
    _fields_ = [("n_steps", C.c_int32), ("status", C.c_int32)]


DR_OK, DR_NO_FRAME, DR_NUMERIC = 0, 1, 2   # a window's status (VILO_DR_*)
DR_STATE = 10   # P (3), quaternion x y z w, V (3)


class DrCovOpts(C.Structure):
    """vilo_dr_cov_opts (8 bytes)"""
    _fields_ = [("from_frame", C.c_int32), ("reserved", C.c_int32)]


class LegDeadReckonOpts(C.Structure):
    """vilo_leg_dead_reckon_opts (8 bytes)"""
    _fields_ = [("from_frame", C.c_int32), ("reserved", C.c_int32)]


class WindowLegDeadReckonRecord(C.Structure):
    """vilo_window_leg_dead_reckon_record (8 bytes)"""
    _fields_ = [("n_steps", C.c_int32), ("status", C.c_int32)]


LEG_DR_STATE, LEG_DR_LEGS, LEG_DR_TRAJ = 32, 12, 48   # doubles of a state_out, legs_out and trajectory row of a leg dead reckoning


class LegDrCovOpts(C.Structure):
    """vilo_leg_dr_cov_opts (8 bytes)"""
    _fields_ = [("from_frame", C.c_int32), ("reserved", C.c_int32)]


LEG_DR_COV_N = 31      # error-state coordinates of a leg dead-reckoned covariance: dp dtheta dv deps_1..4 dba dbg drho_1..4
LEG_DR_COV_IN = 19     # its cov_in: a frame block of Batch.covariance() (COV_FRAME)
LEG_DR_COV_POSE = 6    # the pose block of a pose_cov_trajectory row: dp, dtheta

DR_COV_N = 15     # error-state coordinates of a dead-reckoned covariance: dp, dtheta, dv, dba, dbg
DR_COV_POSE = 6   # the pose block of a trajectory row: dp, dtheta

class GaugeOpts(C.Structure):
    """vilo_gauge_opts (8 bytes)"""
    _fields_ = [("anchor", C.c_int32), ("reserved", C.c_int32)]


class WindowGaugeRecord(C.Structure):
    """vilo_window_gauge_record (16 bytes)"""
    _fields_ = [("yaw_diff_deg", C.c_double), ("singular", C.c_int32), ("status", C.c_int32)]


GAUGE_ANCHOR = {"uploaded": 0, "given": 1}   # VILO_GAUGE_ANCHOR_UPLOADED, VILO_GAUGE_ANCHOR_GIVEN
GAUGE_OK, GAUGE_NUMERIC = 0, 1   # a window's status (VILO_GAUGE_*)


class WindowFailureRecord(C.Structure):
    """vilo_window_failure_record (12 bytes)"""
    _fields_ = [("flags", C.c_int32), ("would_reboot", C.c_int32), ("status", C.c_int32)]


FAILURE_OK, FAILURE_NUMERIC = 0, 1   # a window's status (VILO_FAILURE_OK, VILO_FAILURE_NUMERIC)
FAILURE_FEW_TRACKS, FAILURE_BIG_BA, FAILURE_BIG_BG, FAILURE_BIG_TRANSLATION, FAILURE_BIG_Z, FAILURE_BIG_ANGLE = 1, 2, 4, 8, 16, 32   # bits of flags
FAILURE_VALUES = 6   # the compared quantities, in bit order

class RepropOpts(C.Structure):
    """vilo_reprop_opts (40 bytes)"""
    _fields_ = [("point", C.c_int32), ("select", C.c_int32), ("write", C.c_int32), ("pad", C.c_int32),
                ("ba_threshold", C.c_double), ("bg_threshold", C.c_double), ("rho_threshold", C.c_double)]


class IntervalRepropRecord(C.Structure):
    """vilo_interval_reprop_record (32 bytes)"""
    _fields_ = [("drift_ba", C.c_double), ("drift_bg", C.c_double), ("drift_rho", C.c_double), ("selected", C.c_int32),
                ("status", C.c_int32)]


REPROP_POINT = {"state": 0, "startup": 1, "given": 2}    # VILO_REPROP_POINT_*
REPROP_SELECT = {"all": 0, "drifted": 1, "mask": 2}      # VILO_REPROP_SELECT_*
REPROP_OK, REPROP_NOT_SELECTED, REPROP_NO_INTERVAL, REPROP_NO_SAMPLES, REPROP_NUMERIC = 0, 1, 2, 3, 4   # an interval's status (VILO_REPROP_*)
REPROP_THRESHOLDS = (0.10, 0.01, 0.01)   # vilo_default_reprop_opts: ba, bg, rho
PREPARED_DOUBLES = 126 + 961   # PreintPrepared: head + sqrt_info (Batch.fetch(15))

class RetractOpts(C.Structure):
    """vilo_retract_opts (8 bytes)"""
    _fields_ = [("base", C.c_int32), ("reserved", C.c_int32)]


class WindowRetractRecord(C.Structure):
    """vilo_window_retract_record (24 bytes)"""
    _fields_ = [("status", C.c_int32), ("n_applied", C.c_int32), ("step_norm", C.c_double), ("step_max", C.c_double)]


RETRACT_BASE = {"current": 0, "uploaded": 1}   # VILO_RETRACT_BASE_CURRENT, VILO_RETRACT_BASE_UPLOADED
RETRACT_OK, RETRACT_NUMERIC = 0, 1   # a window's status (VILO_RETRACT_*)

GRAD_STATE = 222  # pose 11 x 6, speed-bias 11 x 9, leg bias 11 x 4, extrinsics 2 x 6, td
IMU_RESIDUAL = 31  # entries of an interval's whitened residual (IMULegFactor; IMUFactor fills 0..14)

# vilo_debug_batch_path: code -> name per axis (include/vilo_gpu.h); "none": the step was not launched
PATH_AXES = (
    ("visual", {-1: "none", 0: "small_c", 1: "tpar_c", 2: "tpar", 3: "pc_imu", 4: "pc", 5: "single_c", 6: "single"}),
    ("imu", {-1: "none", 0: "fused", 1: "single", 2: "pair"}),
    ("imu_order", {-1: "none", 0: "last", 1: "first"}),
    ("assembly", {-1: "none", 0: "small", 1: "full", 2: "accept_wave"}),
    ("solver", {-1: "none", 0: "wave", 3: "split", 4: "mw8"}),
    ("rows", {0: "full", 1: "compact"}),
)

COV_GAUGES = {"frame0": 0, "none": 1}
COV_FRAME = 19     # dp dtheta v ba bg rho
COV_POSES = 79     # 11 poses, ex0, ex1, td


class SynthParams(C.Structure):
    _fields_ = [("seed", C.c_uint64), ("n_landmarks", C.c_int32), ("n_start_frames", C.c_int32), ("imu_rate_hz", C.c_double),
                ("frame_rate_hz", C.c_double), ("pixel_noise", C.c_double), ("sig_p", C.c_double), ("sig_theta", C.c_double),
                ("sig_v", C.c_double), ("sig_ba", C.c_double), ("sig_bg", C.c_double), ("sig_rho", C.c_double),
                ("sig_lambda_rel", C.c_double), ("lin_offset_ba", C.c_double), ("lin_offset_bg", C.c_double),
                ("lin_offset_rho", C.c_double), ("with_prior", C.c_int32), ("pad", C.c_int32)]


class SynthOut(C.Structure):
    _fields_ = [("lm_start_frame", c_int32_p), ("lm_obs_offset", c_int32_p), ("obs", c_double_p), ("obs_is_stereo", c_uint8_p),
                ("samples", C.POINTER(Sample)), ("sample_offsets", c_int32_p), ("lin", c_double_p),
                ("pose", c_double_p), ("speed_bias", c_double_p), ("leg_bias", c_double_p), ("ex_pose", c_double_p),
                ("td", c_double_p), ("inv_depth", c_double_p),
                ("truth_pose", c_double_p), ("truth_speed_bias", c_double_p), ("truth_leg_bias", c_double_p),
                ("truth_inv_depth", c_double_p), ("prior", C.POINTER(Prior))]


def dptr(a):
    assert a.dtype == np.float64 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(c_double_p)


def iptr(a):
    assert a.dtype == np.int32 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(c_int32_p)


def u8ptr(a):
    assert a.dtype == np.uint8 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(c_uint8_p)


def as_struct_ptr(a, ctype):
    """View a float64 numpy array as an array of `ctype` structs."""
    assert a.dtype == np.float64 and a.flags["C_CONTIGUOUS"]
    return C.cast(a.ctypes.data, C.POINTER(ctype))
