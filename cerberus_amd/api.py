"""Thin ctypes binding of the C-ABI in include/vilo_gpu.h (libvilo_gpu.so).

There is no CPU fallback: constructing a Context without the HIP library or without a GPU raises.
The methods mirror the reference's operator interface for the hot path:
  eval_* ........ ceres::CostFunction::Evaluate of the five factor classes (src/factor/*)
  preintegrate .. IMULegIntegrationBase ctor + push_back (imu_leg_integration_base.cpp:7-136)
  solve_windows . Estimator::optimization() solve half (estimator.cpp:1054-1245)
  marginalize ... Estimator::optimization() marginalisation half (estimator.cpp:1247-1455)
  Batch.retract ........ PoseLocalParameterization::Plus / Ceres' Euclidean Plus over a whole resident batch (vilo_batch_retract)
  window_retract ....... the same on host windows (vilo_window_retract)
  Batch.set_state ...... Estimator::vector2double for chosen windows of a resident batch (vilo_batch_set_state)
  Batch.save_state ..... the current state into the batch's snapshot slot (vilo_batch_save_state)
  Batch.restore_state .. the snapshot back, bit for bit (vilo_batch_restore_state)
  Batch.dead_reckon_covariance  IntegrationBase::midPointIntegration's F, V covariance recurrence beside dead_reckon's state (vilo_batch_dead_reckon_covariance)
  Batch.leg_dead_reckon  the nominal-state part of IMULegIntegrationBase::midPointIntegration with the fused leg position (vilo_batch_leg_dead_reckon)
  Batch.leg_dead_reckon_covariance  its 31 x 31 F, V covariance recurrence beside leg_dead_reckon's state (vilo_batch_leg_dead_reckon_covariance)
  Batch.gauss_newton_step  the step Ceres' linear solver computes, (H + mu D^2) delta = -g, per window (vilo_batch_gauss_newton_step)
"""
import collections
import ctypes as C
import os

import numpy as np

from . import _ctypes as T

_lib = None


class ViloError(RuntimeError):
    pass


def lib():
    global _lib
    if _lib is None:
        path = os.environ.get("VILO_GPU_LIB") or os.path.join(T.LIB_DIR, "libvilo_gpu.so")
        if not os.path.exists(path):
            raise ViloError("libvilo_gpu.so is missing (run __graft_entry__.build()); there is no CPU fallback")
        L = C.CDLL(path)
        L.vilo_last_error.restype = C.c_char_p
        L.vilo_last_solve_ms.restype = C.c_double
        L.vilo_last_covariance_ms.restype = C.c_double
        L.vilo_last_residuals_ms.restype = C.c_double
        L.vilo_last_gradient_ms.restype = C.c_double
        L.vilo_last_triangulate_ms.restype = C.c_double
        L.vilo_last_pnp_ms.restype = C.c_double
        L.vilo_last_gyro_align_ms.restype = C.c_double
        L.vilo_last_predict_ms.restype = C.c_double
        L.vilo_last_dead_reckon_ms.restype = C.c_double
        L.vilo_last_dr_cov_ms.restype = C.c_double
        L.vilo_last_leg_dead_reckon_ms.restype = C.c_double
        L.vilo_last_leg_dr_cov_ms.restype = C.c_double
        L.vilo_last_gauge_fix_ms.restype = C.c_double
        L.vilo_last_failure_detection_ms.restype = C.c_double
        L.vilo_last_repropagate_ms.restype = C.c_double
        L.vilo_last_mask_ms.restype = C.c_double
        L.vilo_last_retract_ms.restype = C.c_double
        L.vilo_last_set_state_ms.restype = C.c_double
        L.vilo_last_gn_step_ms.restype = C.c_double
        L.vilo_last_hess_vec_ms.restype = C.c_double
        L.vilo_last_dogleg_step_ms.restype = C.c_double
        L.vilo_last_trial_cost_ms.restype = C.c_double
        L.vilo_solve_wave_lds_bytes.restype = C.c_size_t
        _lib = L
    return _lib


def default_solve_opts(fixed_iterations=False, max_num_iterations=12):
    o = T.SolveOpts()
    lib().vilo_default_solve_opts(C.byref(o))
    o.fixed_iterations = 1 if fixed_iterations else 0
    o.max_num_iterations = max_num_iterations
    return o


def _p(a):
    return None if a is None else a.ctypes.data_as(T.c_double_p)


def _c(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def default_cov_opts():
    o = T.CovOpts()
    lib().vilo_default_cov_opts(C.byref(o))
    return o


def _cov_opts(gauge, poses, min_reciprocal_condition):
    if gauge not in T.COV_GAUGES:
        raise ValueError("gauge must be one of %s" % sorted(T.COV_GAUGES))
    o = default_cov_opts()
    o.gauge, o.want_poses, o.min_reciprocal_condition = T.COV_GAUGES[gauge], 1 if poses else 0, float(min_reciprocal_condition)
    return o


LandmarkCovariance = collections.namedtuple("LandmarkCovariance", "inv_depth_var points point_cov offsets status frames poses")


def _landmark_covariance(ctx, n_landmarks, gauge, frames, poses, min_reciprocal_condition, call):
    n = len(n_landmarks)
    o = _cov_opts(gauge, False, min_reciprocal_condition)
    offsets = np.zeros(n + 1, np.int64)
    offsets[1:] = np.cumsum(n_landmarks)
    L = int(offsets[-1])
    var, pts, pcov = np.zeros(L), np.zeros((L, 3)), np.zeros((L, 3, 3))
    status = np.zeros(n, np.int32)
    fr = np.zeros((n, T.F, T.COV_FRAME, T.COV_FRAME)) if frames else None
    pz = np.zeros((n, T.COV_POSES, T.COV_POSES)) if poses else None
    ctx._check(call(o, _p(fr), _p(pz), _p(var), _p(pts), _p(pcov), T.iptr(status)))
    return LandmarkCovariance(var, pts, pcov, offsets, status, fr, pz)


Residuals = collections.namedtuple("Residuals", "cost prior_cost imu_cost visual_cost visual_cost_plain n_visual_blocks n_huber_active "
                                                "n_outliers n_negative_depth status lm_cost lm_reproj_px lm_flags offsets obs_residuals "
                                                "imu_residuals")


def _residuals(ctx, descs, outlier_threshold_px, observations, imu, call):
    n = len(descs)
    o = T.ResidualOpts()
    lib().vilo_default_residual_opts(C.byref(o))
    o.outlier_threshold_px = float(outlier_threshold_px)
    offsets = np.zeros(n + 1, np.int64)
    offsets[1:] = np.cumsum([d.n_landmarks for d in descs])
    L = int(offsets[-1])
    rows = sum(d.n_obs for d in descs if d.n_landmarks > 0)   # (a window without landmarks has no observation rows)
    wr = (T.WindowResidual * n)()
    lm_cost, lm_px, lm_flags = np.zeros(L), np.zeros(L), np.zeros(L, np.uint8)
    obs = np.zeros((rows, 4)) if observations else None
    imr = np.zeros((n, 10, T.IMU_RESIDUAL)) if imu else None
    ctx._check(call(C.byref(o), wr, _p(lm_cost), _p(lm_px), T.u8ptr(lm_flags), _p(obs), _p(imr)))
    a = np.frombuffer(wr, dtype=np.dtype([(f, np.float64 if t is C.c_double else (np.float64, 10) if f == "imu_cost" else np.int32)
                                          for f, t in T.WindowResidual._fields_]), count=n).copy()
    return Residuals(a["cost"], a["prior_cost"], a["imu_cost"], a["visual_cost"], a["visual_cost_plain"], a["n_visual_blocks"],
                     a["n_huber_active"], a["n_outliers"], a["n_negative_depth"], a["status"], lm_cost, lm_px, lm_flags, offsets, obs, imr)


Gradient = collections.namedtuple("Gradient", "max_norm norm scaled_max argmax_kind argmax_index argmax_component n_free status "
                                              "state_grad state_diag lm_grad lm_diag offsets")


def _gradient(ctx, descs, state, diag, landmarks, call):
    n = len(descs)
    offsets = np.zeros(n + 1, np.int64)
    offsets[1:] = np.cumsum([d.n_landmarks for d in descs])
    L = int(offsets[-1])
    wg = (T.WindowGradient * n)()
    sg = np.zeros((n, T.GRAD_STATE)) if state else None
    sd = np.zeros((n, T.GRAD_STATE)) if (state and diag) else None
    lg = np.zeros(L) if landmarks else None
    ld = np.zeros(L) if (landmarks and diag) else None
    ctx._check(call(wg, _p(sg), _p(sd), _p(lg), _p(ld)))
    a = np.frombuffer(wg, dtype=np.dtype([(f, np.float64 if t is C.c_double else np.int32) for f, t in T.WindowGradient._fields_]),
                      count=n).copy()
    return Gradient(a["max_norm"], a["norm"], a["scaled_max"], a["argmax_kind"], a["argmax_index"], a["argmax_component"], a["n_free"],
                    a["status"], sg, sd, lg, ld, offsets)


Triangulation = collections.namedtuple("Triangulation", "depth flags offsets shift_inv_depth")


def triangulate_opts(n_landmarks, select="unset", mask=None, write=False, init_depth=5.0, stereo=True):
    """(T.TriangulateOpts, mask as a contiguous uint8 array or None) of a triangulate call over n_landmarks landmarks; needs no device.
    select: 'unset' (inverse depth not positive), 'all', or 'mask' with mask [n_landmarks] (non-zero: selected)."""
    if select not in T.TRI_SELECT:
        raise ValueError("select must be one of %s" % sorted(T.TRI_SELECT))
    if (select == "mask") != (mask is not None):
        raise ValueError("select='mask' and a mask go together")
    init_depth = float(init_depth)
    if not (np.isfinite(init_depth) and init_depth > 0.0):
        raise ValueError("init_depth must be finite and > 0")
    if mask is not None:
        mask = np.ascontiguousarray(np.asarray(mask) != 0, dtype=np.uint8)
        if mask.shape != (n_landmarks,):
            raise ValueError("mask must have one entry per landmark of the call (%d), got shape %s" % (n_landmarks, mask.shape))
    o = T.TriangulateOpts()
    o.init_depth, o.stereo, o.select, o.write, o.pad = init_depth, 1 if stereo else 0, T.TRI_SELECT[select], 1 if write else 0, 0
    return o, mask


def _triangulate(ctx, descs, select, mask, write, init_depth, stereo, shift, call):
    n = len(descs)
    offsets = np.zeros(n + 1, np.int64)
    offsets[1:] = np.cumsum([d.n_landmarks for d in descs])
    L = int(offsets[-1])
    o, mask = triangulate_opts(L, select, mask, write, init_depth, stereo)
    depth, flags = np.zeros(L), np.zeros(L, np.uint8)
    sh = np.zeros(L) if shift else None
    ctx._check(call(C.byref(o), None if mask is None else T.u8ptr(mask), _p(depth), T.u8ptr(flags), _p(sh)))
    return Triangulation(depth, flags, offsets, sh)


MaskRecords = collections.namedtuple("MaskRecords", "status n_landmarks n_masked n_newly_masked n_obs_left offsets")


def mask_opts(n_landmarks, source="given", mask=None, combine="replace", flag_bits=3, outlier_threshold_px=3.0):
    """(T.MaskOpts, mask as a contiguous uint8 array or None) of a mask_landmarks call over n_landmarks landmarks; needs no device.
    source: 'given' with mask [n_landmarks] (non-zero: masked), 'outlier_flags' (the residual call's landmark test, flag bytes
    intersecting flag_bits, at outlier_threshold_px) or 'clear'. combine: 'replace' or 'or' (added to the mask in force)."""
    if source not in T.MASK_SOURCE:
        raise ValueError("source must be one of %s" % sorted(T.MASK_SOURCE))
    if combine not in T.MASK_COMBINE:
        raise ValueError("combine must be one of %s" % sorted(T.MASK_COMBINE))
    if (source == "given") != (mask is not None):
        raise ValueError("source='given' and a mask go together")
    thr = float(outlier_threshold_px)
    if not (np.isfinite(thr) and thr >= 0.0):
        raise ValueError("outlier_threshold_px must be finite and >= 0")
    if mask is not None:
        mask = np.ascontiguousarray(np.asarray(mask) != 0, dtype=np.uint8)
        if mask.shape != (n_landmarks,):
            raise ValueError("mask must have one entry per landmark of the call (%d), got shape %s" % (n_landmarks, mask.shape))
    o = T.MaskOpts()
    o.source, o.combine, o.flag_bits, o.pad, o.outlier_threshold_px = T.MASK_SOURCE[source], T.MASK_COMBINE[combine], int(flag_bits) & 0xFF, 0, thr
    return o, mask


def _mask_landmarks(ctx, descs, source, mask, combine, flag_bits, outlier_threshold_px, call):
    n = len(descs)
    offsets = np.zeros(n + 1, np.int64)
    offsets[1:] = np.cumsum([d.n_landmarks for d in descs])
    L = int(offsets[-1])
    o, mask = mask_opts(L, source, mask, combine, flag_bits, outlier_threshold_px)
    out = np.zeros(L, np.uint8)
    rec = (T.WindowMask * n)()
    ctx._check(call(C.byref(o), None if mask is None else T.u8ptr(mask), T.u8ptr(out), rec))
    a = np.frombuffer(rec, dtype=np.dtype([(f, np.int32) for f, _ in T.WindowMask._fields_]), count=n).copy()
    return out, MaskRecords(a["status"], a["n_landmarks"], a["n_masked"], a["n_newly_masked"], a["n_obs_left"], offsets)


FramePose = collections.namedtuple("FramePose", "pose final_cost initial_cost n_points iterations status")


def pnp_opts(frame=-1, guess="previous", write=False, max_iterations=20, step_tolerance=1e-12):
    """T.PnpOpts of a frame_pose_pnp call; needs no device. frame: -1 (each window's last frame) or 1 .. T.MAX_FRAMES - 1; guess: 'previous'
    (the reference: start from frame k - 1's pose) or 'current' (frame k's own)."""
    if guess not in T.PNP_GUESS:
        raise ValueError("guess must be one of %s" % sorted(T.PNP_GUESS))
    if int(frame) != frame or frame < -1 or frame == 0 or frame > T.MAX_FRAMES - 1:
        raise ValueError("frame must be -1 (the last frame) or 1 .. %d" % (T.MAX_FRAMES - 1))
    if int(max_iterations) != max_iterations or not 1 <= max_iterations <= 64:
        raise ValueError("max_iterations must be 1 .. 64")
    step_tolerance = float(step_tolerance)
    if not (np.isfinite(step_tolerance) and step_tolerance >= 0.0):
        raise ValueError("step_tolerance must be finite and not negative")
    o = T.PnpOpts()
    o.frame, o.guess, o.write, o.max_iterations, o.step_tolerance = int(frame), T.PNP_GUESS[guess], 1 if write else 0, int(max_iterations), step_tolerance
    return o


def _frame_pose_pnp(ctx, n, frame, guess, write, max_iterations, step_tolerance, call):
    o = pnp_opts(frame, guess, write, max_iterations, step_tolerance)
    pose = np.zeros((n, 7))
    rec = (T.WindowPnpRecord * n)()
    ctx._check(call(C.byref(o), _p(pose), rec))
    a = np.frombuffer(rec, dtype=np.dtype([(f, np.float64 if t is C.c_double else np.int32) for f, t in T.WindowPnpRecord._fields_]),
                      count=n).copy()
    return FramePose(pose, a["final_cost"], a["initial_cost"], a["n_points"], a["iterations"], a["status"])


GyroAlignment = collections.namedtuple("GyroAlignment", "delta_bg initial_cost model_cost n_intervals status")


def gyro_opts(linearization="record", write=False):
    """T.GyroOpts of a gyro_bias_align call; needs no device. linearization: 'record' (the reference: the records' delta_q as they are) or
    'corrected' (delta_q corrected to first order for the state's gyro biases, as the IMU factors correct it)."""
    if linearization not in T.GYRO_LINEARIZATION:
        raise ValueError("linearization must be one of %s" % sorted(T.GYRO_LINEARIZATION))
    o = T.GyroOpts()
    o.linearization, o.write = T.GYRO_LINEARIZATION[linearization], 1 if write else 0
    return o


def _gyro_bias_align(ctx, n, linearization, write, call):
    o = gyro_opts(linearization, write)
    delta_bg = np.zeros((n, 3))
    rec = (T.WindowGyroRecord * n)()
    ctx._check(call(C.byref(o), _p(delta_bg), rec))
    a = np.frombuffer(rec, dtype=np.dtype([(f, np.float64 if t is C.c_double else np.int32) for f, t in T.WindowGyroRecord._fields_]),
                      count=n).copy()
    return GyroAlignment(delta_bg, a["initial_cost"], a["model_cost"], a["n_intervals"], a["status"])


NextFramePrediction = collections.namedtuple("NextFramePrediction", "pts_cam pts_cam_right flags offsets next_pose n_predicted status")


def predict_opts(mode="constant_velocity", next_pose=None, n_windows=None):
    """(T.PredictOpts, next_pose as a contiguous float64 array [W, 7] or None) of a predict_next_frame call; needs no device.
    mode: 'constant_velocity' (the reference: the last two frames' motion once more) or 'given' with next_pose, one row
    [px py pz qx qy qz qw] per window (n_windows of them, where that is given)."""
    if mode not in T.PREDICT_MODE:
        raise ValueError("mode must be one of %s" % sorted(T.PREDICT_MODE))
    if (mode == "given") != (next_pose is not None):
        raise ValueError("mode='given' and a next_pose go together")
    if next_pose is not None:
        next_pose = np.ascontiguousarray(next_pose, dtype=np.float64)
        if next_pose.ndim != 2 or next_pose.shape[1] != 7 or (n_windows is not None and next_pose.shape[0] != n_windows):
            raise ValueError("next_pose must have one row of 7 per window of the call%s, got shape %s"
                             % ("" if n_windows is None else " (%d)" % n_windows, next_pose.shape))
    o = T.PredictOpts()
    o.mode, o.pad = T.PREDICT_MODE[mode], 0
    return o, next_pose


def _predict_next_frame(ctx, descs, mode, next_pose, right, call):
    n = len(descs)
    o, given = predict_opts(mode, next_pose, n)
    offsets = np.zeros(n + 1, np.int64)
    offsets[1:] = np.cumsum([d.n_landmarks for d in descs])
    L = int(offsets[-1])
    pts, flags = np.zeros((L, 3)), np.zeros(L, np.uint8)
    ptr = np.zeros((L, 3)) if right else None
    pose = np.zeros((n, 7))
    rec = (T.WindowPredictRecord * n)()
    ctx._check(call(C.byref(o), _p(given), _p(pts), _p(ptr), T.u8ptr(flags), _p(pose), rec))
    a = np.frombuffer(rec, dtype=np.dtype([(f, np.int32) for f, _ in T.WindowPredictRecord._fields_]), count=n).copy()
    return NextFramePrediction(pts, ptr, flags, offsets, pose, a["n_predicted"], a["status"])


DeadReckoning = collections.namedtuple("DeadReckoning", "state trajectory step_offsets n_steps status")


def dead_reckon_opts(from_frame=-1, write=False):
    """T.DeadReckonOpts of a dead_reckon call; needs no device. from_frame: -1 (each window's last frame) or 0 .. T.MAX_FRAMES - 1;
    write=True (the result becomes the state of frame from_frame + 1) needs an explicit frame."""
    if int(from_frame) != from_frame or not -1 <= from_frame <= T.MAX_FRAMES - 1:
        raise ValueError("from_frame must be -1 (the last frame) or 0 .. %d" % (T.MAX_FRAMES - 1))
    if write and from_frame == -1:
        raise ValueError("write=True needs an explicit from_frame: the frame after a window's last does not exist")
    o = T.DeadReckonOpts()
    o.from_frame, o.write = int(from_frame), 1 if write else 0
    return o


def _dead_reckon(ctx, n, samples, offsets, from_frame, write, trajectory, call):
    o = dead_reckon_opts(from_frame, write)
    offsets = np.ascontiguousarray(offsets, dtype=np.int32)
    if offsets.shape != (n + 1,):
        raise ValueError("offsets must have one entry per window of the call and one more (%d), got shape %s" % (n + 1, offsets.shape))
    if offsets[0] != 0 or (np.diff(offsets) < 0).any():
        raise ValueError("offsets must start at 0 and must not decrease")
    samples = _c(samples).reshape(-1, T.SAMPLE_DOUBLES)
    if len(samples) < offsets[-1]:
        raise ValueError("offsets reach sample %d, samples holds %d" % (offsets[-1], len(samples)))
    step_offsets = np.zeros(n + 1, np.int64)
    step_offsets[1:] = np.cumsum(np.maximum(np.diff(offsets) - 1, 0))
    state = np.zeros((n, T.DR_STATE))
    traj = np.zeros((int(step_offsets[-1]), T.DR_STATE)) if trajectory else None
    rec = (T.WindowDeadReckonRecord * n)()
    ctx._check(call(C.byref(o), C.cast(samples.ctypes.data, C.POINTER(T.Sample)), T.iptr(offsets), _p(state), _p(traj), rec))
    a = np.frombuffer(rec, dtype=np.dtype([(f, np.int32) for f, _ in T.WindowDeadReckonRecord._fields_]), count=n).copy()
    return DeadReckoning(state, traj, step_offsets, a["n_steps"], a["status"])


LegDeadReckoning = collections.namedtuple("LegDeadReckoning", "state legs trajectory step_offsets n_steps status")


def leg_dead_reckon_opts(from_frame=-1):
    """T.LegDeadReckonOpts of a leg_dead_reckon call; needs no device. from_frame: -1 (each window's last frame) or 0 .. T.MAX_FRAMES - 1."""
    if int(from_frame) != from_frame or not -1 <= from_frame <= T.MAX_FRAMES - 1:
        raise ValueError("from_frame must be -1 (the last frame) or 0 .. %d" % (T.MAX_FRAMES - 1))
    o = T.LegDeadReckonOpts()
    o.from_frame, o.reserved = int(from_frame), 0
    return o


def _leg_dead_reckon(ctx, n, samples, offsets, from_frame, trajectory, call):
    o = leg_dead_reckon_opts(from_frame)
    offsets = np.ascontiguousarray(offsets, dtype=np.int32)
    if offsets.shape != (n + 1,):
        raise ValueError("offsets must have one entry per window of the call and one more (%d), got shape %s" % (n + 1, offsets.shape))
    if offsets[0] != 0 or (np.diff(offsets) < 0).any():
        raise ValueError("offsets must start at 0 and must not decrease")
    samples = _c(samples).reshape(-1, T.SAMPLE_DOUBLES)
    if len(samples) < offsets[-1]:
        raise ValueError("offsets reach sample %d, samples holds %d" % (offsets[-1], len(samples)))
    step_offsets = np.zeros(n + 1, np.int64)
    step_offsets[1:] = np.cumsum(np.maximum(np.diff(offsets) - 1, 0))
    state, legs = np.zeros((n, T.LEG_DR_STATE)), np.zeros((n, 4, 3))
    traj = np.zeros((int(step_offsets[-1]), T.LEG_DR_TRAJ)) if trajectory else None
    rec = (T.WindowLegDeadReckonRecord * n)()
    ctx._check(call(C.byref(o), C.cast(samples.ctypes.data, C.POINTER(T.Sample)), T.iptr(offsets), _p(state), _p(legs), _p(traj), rec))
    a = np.frombuffer(rec, dtype=np.dtype([(f, np.int32) for f, _ in T.WindowLegDeadReckonRecord._fields_]), count=n).copy()
    return LegDeadReckoning(state, legs, traj, step_offsets, a["n_steps"], a["status"])


DeadReckonedCovariance = collections.namedtuple("DeadReckonedCovariance", "state cov pose_cov_trajectory step_offsets n_steps status")


def dr_cov_opts(from_frame=-1):
    """T.DrCovOpts of a dead_reckon_covariance call; needs no device. from_frame: -1 (each window's last frame) or 0 .. T.MAX_FRAMES - 1."""
    if int(from_frame) != from_frame or not -1 <= from_frame <= T.MAX_FRAMES - 1:
        raise ValueError("from_frame must be -1 (the last frame) or 0 .. %d" % (T.MAX_FRAMES - 1))
    o = T.DrCovOpts()
    o.from_frame, o.reserved = int(from_frame), 0
    return o


def dr_cov_in(frames, n_frames, from_frame=-1):
    """cov_in [W, 15, 15] of a dead_reckon_covariance call, cut out of Batch.covariance()'s frames [W, 11, 19, 19]: for every window the
    leading 15 x 15 (dp, dtheta, dv, dba, dbg; the leg bias does not enter the IMU recurrence) of the block of frame from_frame, -1: the
    window's last, n_frames[w] - 1. Needs no device. A window that has no such frame gets zeros (the call reports it as NO_FRAME)."""
    frames = np.asarray(frames, dtype=np.float64)
    if frames.ndim != 4 or frames.shape[1:] != (T.F, T.COV_FRAME, T.COV_FRAME):
        raise ValueError("frames must have shape (W, %d, %d, %d), got %s" % (T.F, T.COV_FRAME, T.COV_FRAME, frames.shape))
    n_frames = np.asarray(n_frames)
    if n_frames.shape != (frames.shape[0],) or n_frames.dtype.kind not in "iu" or (n_frames < 1).any() or (n_frames > T.MAX_FRAMES).any():
        raise ValueError("n_frames must hold one frame count in 1 .. %d per window (%d)" % (T.MAX_FRAMES, frames.shape[0]))
    dr_cov_opts(from_frame)
    f = n_frames - 1 if from_frame == -1 else np.full(len(n_frames), int(from_frame))
    out = np.zeros((len(n_frames), T.DR_COV_N, T.DR_COV_N))
    have = f < n_frames
    out[have] = frames[np.nonzero(have)[0], f[have], :T.DR_COV_N, :T.DR_COV_N]
    return out


def _dead_reckon_covariance(ctx, n, samples, offsets, cov_in, from_frame, pose_trajectory, call):
    o = dr_cov_opts(from_frame)
    offsets = np.ascontiguousarray(offsets, dtype=np.int32)
    if offsets.shape != (n + 1,):
        raise ValueError("offsets must have one entry per window of the call and one more (%d), got shape %s" % (n + 1, offsets.shape))
    if offsets[0] != 0 or (np.diff(offsets) < 0).any():
        raise ValueError("offsets must start at 0 and must not decrease")
    samples = _c(samples).reshape(-1, T.SAMPLE_DOUBLES)
    if len(samples) < offsets[-1]:
        raise ValueError("offsets reach sample %d, samples holds %d" % (offsets[-1], len(samples)))
    if cov_in is not None:
        cov_in = _c(cov_in)
        if cov_in.shape != (n, T.DR_COV_N, T.DR_COV_N):
            raise ValueError("cov_in must have shape (%d, %d, %d), got %s" % (n, T.DR_COV_N, T.DR_COV_N, cov_in.shape))
    step_offsets = np.zeros(n + 1, np.int64)
    step_offsets[1:] = np.cumsum(np.maximum(np.diff(offsets) - 1, 0))
    state, cov = np.zeros((n, T.DR_STATE)), np.zeros((n, T.DR_COV_N, T.DR_COV_N))
    traj = np.zeros((int(step_offsets[-1]), T.DR_COV_POSE, T.DR_COV_POSE)) if pose_trajectory else None
    rec = (T.WindowDeadReckonRecord * n)()
    ctx._check(call(C.byref(o), C.cast(samples.ctypes.data, C.POINTER(T.Sample)), T.iptr(offsets), _p(cov_in), _p(state), _p(cov), _p(traj), rec))
    a = np.frombuffer(rec, dtype=np.dtype([(f, np.int32) for f, _ in T.WindowDeadReckonRecord._fields_]), count=n).copy()
    return DeadReckonedCovariance(state, cov, traj, step_offsets, a["n_steps"], a["status"])


LegDeadReckonedCovariance = collections.namedtuple("LegDeadReckonedCovariance",
                                                   "state legs cov pose_cov_trajectory leg_cov_trajectory step_offsets n_steps status")


def leg_dr_cov_opts(from_frame=-1):
    """T.LegDrCovOpts of a leg_dead_reckon_covariance call; needs no device. from_frame: -1 (each window's last frame) or 0 .. T.MAX_FRAMES - 1."""
    if int(from_frame) != from_frame or not -1 <= from_frame <= T.MAX_FRAMES - 1:
        raise ValueError("from_frame must be -1 (the last frame) or 0 .. %d" % (T.MAX_FRAMES - 1))
    o = T.LegDrCovOpts()
    o.from_frame, o.reserved = int(from_frame), 0
    return o


def leg_dr_cov_in(frames, n_frames, from_frame=-1):
    """cov_in [W, 19, 19] of a leg_dead_reckon_covariance call, cut out of Batch.covariance()'s frames [W, 11, 19, 19]: for every window the
    whole block (dp, dtheta, dv, dba, dbg, drho) of frame from_frame, -1: the window's last, n_frames[w] - 1. Needs no device. A window
    that has no such frame gets zeros (the call reports it as NO_FRAME)."""
    frames = np.asarray(frames, dtype=np.float64)
    if frames.ndim != 4 or frames.shape[1:] != (T.F, T.COV_FRAME, T.COV_FRAME):
        raise ValueError("frames must have shape (W, %d, %d, %d), got %s" % (T.F, T.COV_FRAME, T.COV_FRAME, frames.shape))
    n_frames = np.asarray(n_frames)
    if n_frames.shape != (frames.shape[0],) or n_frames.dtype.kind not in "iu" or (n_frames < 1).any() or (n_frames > T.MAX_FRAMES).any():
        raise ValueError("n_frames must hold one frame count in 1 .. %d per window (%d)" % (T.MAX_FRAMES, frames.shape[0]))
    leg_dr_cov_opts(from_frame)
    f = n_frames - 1 if from_frame == -1 else np.full(len(n_frames), int(from_frame))
    out = np.zeros((len(n_frames), T.LEG_DR_COV_IN, T.LEG_DR_COV_IN))
    have = f < n_frames
    out[have] = frames[np.nonzero(have)[0], f[have]]
    return out


def _leg_dead_reckon_covariance(ctx, n, samples, offsets, cov_in, from_frame, pose_trajectory, leg_trajectory, call):
    o = leg_dr_cov_opts(from_frame)
    offsets = np.ascontiguousarray(offsets, dtype=np.int32)
    if offsets.shape != (n + 1,):
        raise ValueError("offsets must have one entry per window of the call and one more (%d), got shape %s" % (n + 1, offsets.shape))
    if offsets[0] != 0 or (np.diff(offsets) < 0).any():
        raise ValueError("offsets must start at 0 and must not decrease")
    samples = _c(samples).reshape(-1, T.SAMPLE_DOUBLES)
    if len(samples) < offsets[-1]:
        raise ValueError("offsets reach sample %d, samples holds %d" % (offsets[-1], len(samples)))
    if cov_in is not None:
        cov_in = _c(cov_in)
        if cov_in.shape != (n, T.LEG_DR_COV_IN, T.LEG_DR_COV_IN):
            raise ValueError("cov_in must have shape (%d, %d, %d), got %s" % (n, T.LEG_DR_COV_IN, T.LEG_DR_COV_IN, cov_in.shape))
    step_offsets = np.zeros(n + 1, np.int64)
    step_offsets[1:] = np.cumsum(np.maximum(np.diff(offsets) - 1, 0))
    rows = int(step_offsets[-1])
    state, legs, cov = np.zeros((n, T.LEG_DR_STATE)), np.zeros((n, 4, 3)), np.zeros((n, T.LEG_DR_COV_N, T.LEG_DR_COV_N))
    pose = np.zeros((rows, T.LEG_DR_COV_POSE, T.LEG_DR_COV_POSE)) if pose_trajectory else None
    legc = np.zeros((rows, 4, 3, 3)) if leg_trajectory else None
    rec = (T.WindowLegDeadReckonRecord * n)()
    ctx._check(call(C.byref(o), C.cast(samples.ctypes.data, C.POINTER(T.Sample)), T.iptr(offsets), _p(cov_in), _p(state), _p(legs), _p(cov), _p(pose),
                    _p(legc), rec))
    a = np.frombuffer(rec, dtype=np.dtype([(f, np.int32) for f, _ in T.WindowLegDeadReckonRecord._fields_]), count=n).copy()
    return LegDeadReckonedCovariance(state, legs, cov, pose, legc, step_offsets, a["n_steps"], a["status"])


GaugeFix = collections.namedtuple("GaugeFix", "yaw_diff_deg singular status pose0_before")


def gauge_opts(anchor="uploaded", anchor_pose=None, n=None):
    """(T.GaugeOpts, anchor_pose [n, 7] or None) of a gauge_fix call; needs no device. anchor: 'uploaded' (frame 0's pose of the state the
    batch was created with) or 'given' (anchor_pose [n, 7] as [px py pz qx qy qz qw], one row per window of the call)."""
    if anchor not in T.GAUGE_ANCHOR:
        raise ValueError("anchor must be one of %s" % sorted(T.GAUGE_ANCHOR))
    if anchor == "given" and anchor_pose is None:
        raise ValueError("anchor='given' needs anchor_pose")
    if anchor != "given" and anchor_pose is not None:
        raise ValueError("anchor_pose needs anchor='given'")
    if anchor_pose is not None:
        anchor_pose = _c(anchor_pose)
        if anchor_pose.ndim != 2 or anchor_pose.shape[1] != 7 or (n is not None and anchor_pose.shape[0] != n):
            raise ValueError("anchor_pose must have shape (%s, 7), got %s" % ("W" if n is None else n, anchor_pose.shape))
    o = T.GaugeOpts()
    o.anchor, o.reserved = T.GAUGE_ANCHOR[anchor], 0
    return o, anchor_pose


def _gauge_fix(ctx, n, anchor, anchor_pose, pose0, call):
    o, anchor_pose = gauge_opts(anchor, anchor_pose, n)
    rec = (T.WindowGaugeRecord * n)()
    before = np.zeros((n, 7)) if pose0 else None
    ctx._check(call(C.byref(o), _p(anchor_pose), rec, _p(before)))
    a = np.frombuffer(rec, dtype=np.dtype([("yaw_diff_deg", np.float64), ("singular", np.int32), ("status", np.int32)]), count=n).copy()
    return GaugeFix(a["yaw_diff_deg"], a["singular"], a["status"], before)


FailureDetection = collections.namedtuple("FailureDetection", "flags would_reboot status values")


def failure_inputs(n, last_track_num=None, last_pose=None):
    """(last_track_num [n] int32 or None, last_pose [n, 7] or None) of a failure_detection call, checked; needs no device."""
    if last_track_num is not None:
        last_track_num = np.ascontiguousarray(last_track_num, dtype=np.int32)
        if last_track_num.shape != (n,):
            raise ValueError("last_track_num must have shape (%d,), got %s" % (n, last_track_num.shape))
    if last_pose is not None:
        last_pose = _c(last_pose)
        if last_pose.shape != (n, 7):
            raise ValueError("last_pose must have shape (%d, 7), got %s" % (n, last_pose.shape))
    return last_track_num, last_pose


def _failure_detection(ctx, n, last_track_num, last_pose, call):
    tracks, last_pose = failure_inputs(n, last_track_num, last_pose)
    rec = (T.WindowFailureRecord * n)()
    values = np.zeros((n, T.FAILURE_VALUES))
    ctx._check(call(T.iptr(tracks) if tracks is not None else None, _p(last_pose), rec, _p(values)))
    a = np.frombuffer(rec, dtype=np.dtype([(f, np.int32) for f, _ in T.WindowFailureRecord._fields_]), count=n).copy()
    return FailureDetection(a["flags"], a["would_reboot"], a["status"], values)


Repropagation = collections.namedtuple("Repropagation", "drift selected status")


def reprop_opts(point="state", select="all", write=True, lin=None, mask=None, thresholds=T.REPROP_THRESHOLDS, n_windows=None):
    """(T.RepropOpts, lin [W * 10, 10] or None, mask [W * 10] uint8 or None) of a repropagate call, checked; needs no device.
    point: 'state' (interval k at Ba_k, Bg_k, rho_k of the current state), 'startup' (0, Bg_{k+1}, rho_{k+1}: the reference's start-up
    loop) or 'given' with lin, one row ba bg rho per interval, [W, 10, 10] or [W * 10, 10]. select: 'all', 'drifted' (a drift above its
    threshold) or 'mask' with mask [W, 10] or [W * 10], non-zero = selected. thresholds: (ba, bg, rho), compared with the drifts."""
    if point not in T.REPROP_POINT:
        raise ValueError("point must be one of %s" % sorted(T.REPROP_POINT))
    if select not in T.REPROP_SELECT:
        raise ValueError("select must be one of %s" % sorted(T.REPROP_SELECT))
    if (point == "given") != (lin is not None):
        raise ValueError("point='given' and lin go together")
    if (select == "mask") != (mask is not None):
        raise ValueError("select='mask' and mask go together")
    th = np.asarray(thresholds, dtype=np.float64)
    if th.shape != (3,) or not np.isfinite(th).all() or (th < 0).any():
        raise ValueError("thresholds must be three finite numbers >= 0 (ba, bg, rho), got %r" % (thresholds,))
    if lin is not None:
        lin = _c(lin)
        if lin.shape[-1:] != (10,) or lin.ndim not in (2, 3) or (n_windows is not None and lin.size != 100 * n_windows):
            raise ValueError("lin must have a row of 10 per interval, 10 intervals per window%s, got shape %s"
                             % ("" if n_windows is None else " (%d windows)" % n_windows, lin.shape))
        lin = lin.reshape(-1, 10)
    if mask is not None:
        mask = np.ascontiguousarray(np.asarray(mask) != 0, dtype=np.uint8).reshape(-1)
        if mask.size % 10 or (n_windows is not None and mask.size != 10 * n_windows):
            raise ValueError("mask must have 10 entries per window%s, got %d" % ("" if n_windows is None else " (%d windows)" % n_windows, mask.size))
    o = T.RepropOpts()
    o.point, o.select, o.write, o.pad = T.REPROP_POINT[point], T.REPROP_SELECT[select], 1 if write else 0, 0
    o.ba_threshold, o.bg_threshold, o.rho_threshold = (float(x) for x in th)
    return o, lin, mask


def window_samples(windows):
    """(samples [n, 35], offsets [W * 10 + 1] int32) of the windows' own samples / sample_offsets in the layout vilo_batch_set_samples and
    vilo_batch_repropagate take: empty ranges for the intervals a window does not have."""
    parts, offs, base = [], [0], 0
    for w in windows:
        n = int(w.sample_offsets[-1])
        parts.append(w.samples[:n])
        offs.extend((w.sample_offsets[1:] + base).tolist())
        offs.extend([base + n] * (10 - (len(w.sample_offsets) - 1)))
        base += n
    return np.ascontiguousarray(np.concatenate(parts), dtype=np.float64), np.ascontiguousarray(offs, dtype=np.int32)


def _repropagate(ctx, n, samples, offsets, point, select, write, lin, mask, thresholds, call):
    o, lin, mask = reprop_opts(point, select, write, lin, mask, thresholds, n)
    if (samples is None) != (offsets is None):
        raise ValueError("samples and offsets go together")
    sp = op = None
    if samples is not None:
        offsets = np.ascontiguousarray(offsets, dtype=np.int32)
        if offsets.shape != (10 * n + 1,):
            raise ValueError("offsets must have 10 entries per window of the call and one more (%d), got shape %s" % (10 * n + 1, offsets.shape))
        samples = _c(samples).reshape(-1, T.SAMPLE_DOUBLES)
        if len(samples) < offsets.max():
            raise ValueError("offsets reach sample %d, samples holds %d" % (offsets.max(), len(samples)))
        sp, op = C.cast(samples.ctypes.data, C.POINTER(T.Sample)), T.iptr(offsets)
    rec = (T.IntervalRepropRecord * (10 * n))()
    ctx._check(call(sp, op, C.byref(o), _p(lin), T.u8ptr(mask) if mask is not None else None, rec))
    a = np.frombuffer(rec, dtype=np.dtype([(f, np.float64 if t is C.c_double else np.int32) for f, t in T.IntervalRepropRecord._fields_]),
                      count=10 * n).copy()
    drift = np.stack([a["drift_ba"], a["drift_bg"], a["drift_rho"]], axis=1).reshape(n, 10, 3)
    return Repropagation(drift, a["selected"].reshape(n, 10), a["status"].reshape(n, 10))


Retraction = collections.namedtuple("Retraction", "status n_applied step_norm step_max")


def retract_opts(n_windows, n_landmarks, base="current", state_step=None, lm_step=None, alpha=None):
    """(T.RetractOpts, state_step [n_windows, 222] or None, lm_step [n_landmarks] or None, alpha [n_windows] or None) of a retract call,
    checked and made contiguous float64; needs no device. base: 'current' (the step is applied to the current state) or 'uploaded' (to the
    state the batch was created with). state_step: vilo_batch_gradient's state_grad layout; lm_step: one entry per landmark of the call,
    window by window, in each window's own order; alpha: one step length per window, None for 1. A step that is None is a zero step."""
    if base not in T.RETRACT_BASE:
        raise ValueError("base must be one of %s" % sorted(T.RETRACT_BASE))
    if state_step is not None:
        state_step = _c(state_step)
        if state_step.shape != (n_windows, T.GRAD_STATE):
            raise ValueError("state_step must have shape (%d, %d), got %s" % (n_windows, T.GRAD_STATE, state_step.shape))
    if lm_step is not None:
        lm_step = _c(lm_step)
        if lm_step.shape != (n_landmarks,):
            raise ValueError("lm_step must have one entry per landmark of the call (%d), got shape %s" % (n_landmarks, lm_step.shape))
    if alpha is not None:
        alpha = _c(alpha)
        if alpha.shape != (n_windows,):
            raise ValueError("alpha must have one entry per window of the call (%d), got shape %s" % (n_windows, alpha.shape))
    o = T.RetractOpts()
    o.base, o.reserved = T.RETRACT_BASE[base], 0
    return o, state_step, lm_step, alpha


def _retract(ctx, descs, base, state_step, lm_step, alpha, call):
    n = len(descs)
    o, state_step, lm_step, alpha = retract_opts(n, sum(d.n_landmarks for d in descs), base, state_step, lm_step, alpha)
    rec = (T.WindowRetractRecord * n)()
    ctx._check(call(C.byref(o), _p(state_step), _p(lm_step), _p(alpha), rec))
    a = np.frombuffer(rec, dtype=np.dtype([(f, np.float64 if t is C.c_double else np.int32) for f, t in T.WindowRetractRecord._fields_]),
                      count=n).copy()
    return Retraction(a["status"], a["n_applied"], a["step_norm"], a["step_max"])


GaussNewtonStep = collections.namedtuple("GaussNewtonStep", "state_step lm_step offsets model_cost_change scaled_norm norm grad_dot_step "
                                                            "n_free status")


def gn_step_opts(n_windows, mu=None, gauge="none", min_lm_diagonal=1e-6, max_lm_diagonal=1e32, min_pivot=1e-14):
    """(T.StepOpts, mu [n_windows] contiguous float64 or None) of a gauss_newton_step call, checked; needs no device. mu: None (0), a scalar
    or one value per window, finite and >= 0. gauge: 'none' (the full system, what the solver solves) or 'frame0' (frame 0's position and
    its rotation about gravity held). The diagonal bounds are Ceres' min_lm_diagonal / max_lm_diagonal."""
    if gauge not in T.COV_GAUGES:
        raise ValueError("gauge must be one of %s" % sorted(T.COV_GAUGES))
    lo, hi, piv = float(min_lm_diagonal), float(max_lm_diagonal), float(min_pivot)
    if not (np.isfinite(lo) and np.isfinite(hi) and 0.0 <= lo <= hi):
        raise ValueError("0 <= min_lm_diagonal <= max_lm_diagonal < inf is required")
    if not (np.isfinite(piv) and piv >= 0.0):
        raise ValueError("min_pivot must be finite and >= 0")
    if mu is not None:
        mu = np.asarray(mu, dtype=np.float64)
        if mu.ndim == 0:
            mu = np.full(n_windows, float(mu))
        mu = _c(mu)
        if mu.shape != (n_windows,):
            raise ValueError("mu must be a scalar or have one entry per window of the call (%d), got shape %s" % (n_windows, mu.shape))
        if not np.isfinite(mu).all() or (mu < 0.0).any():
            raise ValueError("mu must be finite and >= 0")
    o = T.StepOpts()
    o.gauge, o.pad0, o.min_lm_diagonal, o.max_lm_diagonal, o.min_pivot = T.COV_GAUGES[gauge], 0, lo, hi, piv
    return o, mu


def _gn_step(ctx, descs, mu, gauge, state, landmarks, min_lm_diagonal, max_lm_diagonal, min_pivot, call):
    n = len(descs)
    o, mu = gn_step_opts(n, mu, gauge, min_lm_diagonal, max_lm_diagonal, min_pivot)
    offsets = np.zeros(n + 1, np.int64)
    offsets[1:] = np.cumsum([d.n_landmarks for d in descs])
    rec = (T.WindowStepRecord * n)()
    ss = np.zeros((n, T.GRAD_STATE)) if state else None
    ls = np.zeros(int(offsets[-1])) if landmarks else None
    ctx._check(call(C.byref(o), _p(mu), rec, _p(ss), _p(ls)))
    a = np.frombuffer(rec, dtype=np.dtype([(f, np.float64 if t is C.c_double else np.int32) for f, t in T.WindowStepRecord._fields_]),
                      count=n).copy()
    return GaussNewtonStep(ss, ls, offsets, a["model_cost_change"], a["scaled_norm"], a["norm"], a["grad_dot_step"], a["n_free"], a["status"])


DoglegStep = collections.namedtuple("DoglegStep", "state_step lm_step cauchy_state cauchy_lm offsets alpha gradient_norm gauss_newton_norm "
                                                  "step_norm beta model_cost_change grad_dot_step norm branch n_free status")


def dogleg_step_args(n_windows, radius, mu=None, gauge="none", min_lm_diagonal=1e-6, max_lm_diagonal=1e32, min_pivot=1e-14):
    """(T.DoglegOpts, radius [n_windows], mu [n_windows] or None) of a dogleg_step call, checked; needs no device. radius: a scalar or one
    value per window, finite and > 0; mu and the rest as gn_step_opts."""
    so, mu = gn_step_opts(n_windows, mu, gauge, min_lm_diagonal, max_lm_diagonal, min_pivot)
    radius = np.asarray(radius, dtype=np.float64)
    if radius.ndim == 0:
        radius = np.full(n_windows, float(radius))
    radius = _c(radius)
    if radius.shape != (n_windows,):
        raise ValueError("radius must be a scalar or have one entry per window of the call (%d), got shape %s" % (n_windows, radius.shape))
    if not np.isfinite(radius).all() or (radius <= 0.0).any():
        raise ValueError("radius must be finite and > 0")
    o = T.DoglegOpts()
    o.gauge, o.pad0, o.min_lm_diagonal, o.max_lm_diagonal, o.min_pivot = so.gauge, 0, so.min_lm_diagonal, so.max_lm_diagonal, so.min_pivot
    return o, radius, mu


def _dogleg_step(ctx, descs, radius, mu, gauge, cauchy, min_lm_diagonal, max_lm_diagonal, min_pivot, call):
    n = len(descs)
    o, radius, mu = dogleg_step_args(n, radius, mu, gauge, min_lm_diagonal, max_lm_diagonal, min_pivot)
    offsets = np.zeros(n + 1, np.int64)
    offsets[1:] = np.cumsum([d.n_landmarks for d in descs])
    rec = (T.WindowDoglegRecord * n)()
    ss, ls = np.zeros((n, T.GRAD_STATE)), np.zeros(int(offsets[-1]))
    cs, cl = (np.zeros((n, T.GRAD_STATE)), np.zeros(int(offsets[-1]))) if cauchy else (None, None)
    ctx._check(call(C.byref(o), _p(radius), _p(mu), rec, _p(ss), _p(ls), _p(cs), _p(cl)))
    a = np.frombuffer(rec, dtype=np.dtype([(f, np.float64 if t is C.c_double else np.int32) for f, t in T.WindowDoglegRecord._fields_]),
                      count=n).copy()
    return DoglegStep(ss, ls, cs, cl, offsets, a["alpha"], a["gradient_norm"], a["gauss_newton_norm"], a["step_norm"], a["beta"],
                      a["model_cost_change"], a["grad_dot_step"], a["norm"], a["branch"], a["n_free"], a["status"])


HessianVector = collections.namedtuple("HessianVector", "state_out lm_out offsets n_vec vHv g_dot_v model_cost_change status")


def hess_vec_args(descs, state_vec=None, lm_vec=None):
    """(K, squeeze, state_vec [W, K, 222] or None, lm_vec [K sum L] or None, offsets) of a hessian_vector call, checked; needs no device.
    state_vec: [W, 222] (one vector) or [W, K, 222]. lm_vec: the call's layout, 1-D of K * sum L entries — window w's block starts at
    K * offsets[w], vector k at + k * L_w inside it (hess_vec_lm_block views it) —, so [sum L] for one vector. At least one is needed."""
    n = len(descs)
    offsets = np.zeros(n + 1, np.int64)
    offsets[1:] = np.cumsum([d.n_landmarks for d in descs])
    n_lm = int(offsets[-1])
    if state_vec is None and lm_vec is None:
        raise ValueError("state_vec or lm_vec is needed")
    K, squeeze = None, False
    if state_vec is not None:
        state_vec = _c(state_vec)
        if state_vec.ndim == 2:
            state_vec, squeeze = state_vec[:, None, :], True
        if state_vec.ndim != 3 or state_vec.shape[0] != n or state_vec.shape[2] != T.GRAD_STATE:
            raise ValueError("state_vec must be [%d, %d] or [%d, K, %d], got %s" % (n, T.GRAD_STATE, n, T.GRAD_STATE, state_vec.shape))
        K = state_vec.shape[1]
        state_vec = _c(state_vec)
    if lm_vec is not None:
        lm_vec = _c(lm_vec)
        if lm_vec.ndim != 1:
            raise ValueError("lm_vec must be 1-D in the call's layout (K * sum L entries), got shape %s" % (lm_vec.shape,))
        if K is None:
            if n_lm == 0 or lm_vec.size % n_lm:
                raise ValueError("lm_vec must have K * sum L = K * %d entries, got %d" % (n_lm, lm_vec.size))
            K, squeeze = lm_vec.size // n_lm, lm_vec.size == n_lm
        elif lm_vec.size != K * n_lm:
            raise ValueError("lm_vec must have K * sum L = %d * %d entries, got %d" % (K, n_lm, lm_vec.size))
    if not 1 <= K <= T.HV_MAX_VECTORS:
        raise ValueError("1 <= K <= %d vectors per window are supported, got %d" % (T.HV_MAX_VECTORS, K))
    return K, squeeze, state_vec, lm_vec, offsets


def hess_vec_lm_block(lm, offsets, n_vec, w):
    """window w's [K, L_w] block of an lm_vec / lm_out array of a hessian_vector call (a view)"""
    a, b = n_vec * int(offsets[w]), n_vec * int(offsets[w + 1])
    return lm[a:b].reshape(n_vec, -1) if b > a else lm[a:b].reshape(n_vec, 0)


def _hess_vec(ctx, descs, state_vec, lm_vec, state, landmarks, call):
    n = len(descs)
    K, squeeze, sv, lv, offsets = hess_vec_args(descs, state_vec, lm_vec)
    rec = (T.HessVecRecord * (n * K))()
    so = np.zeros((n, K, T.GRAD_STATE)) if state else None
    lo = np.zeros(K * int(offsets[-1])) if landmarks else None
    ctx._check(call(K, _p(sv), _p(lv), rec, _p(so), _p(lo)))
    a = np.frombuffer(rec, dtype=np.dtype([(f, np.float64 if t is C.c_double else np.int32) for f, t in T.HessVecRecord._fields_]),
                      count=n * K).copy().reshape(n, K)
    if squeeze:
        a = a[:, 0]
        so = so[:, 0] if so is not None else None
    return HessianVector(so, lo, offsets, K, a["vHv"], a["g_dot_v"], a["model_cost_change"], a["status"])


TrialCost = collections.namedtuple("TrialCost", "cost visual_cost imu_cost prior_cost cost_change n_negative_depth status base best n_steps offsets")
TrialBase = collections.namedtuple("TrialBase", "cost visual_cost imu_cost prior_cost cost_change n_negative_depth status")


def trial_cost_args(descs, state_step=None, lm_step=None, alpha=None):
    """(K, squeeze, state_step [W, K, 222] or None, lm_step [K sum L] or None, alpha [W, K] or None, offsets) of a trial_cost call,
    checked; needs no device. state_step and lm_step as hess_vec_args takes its vectors ([W, 222] or [sum L]: one step); alpha [W, K], or
    [W] for one step, or None for 1."""
    n = len(descs)
    K, squeeze, sv, lv, offsets = hess_vec_args(descs, state_step, lm_step)
    if alpha is not None:
        alpha = _c(alpha)
        if alpha.ndim == 1 and K == 1:
            alpha = alpha[:, None]
        if alpha.shape != (n, K):
            raise ValueError("alpha must be [%d, %d]%s, got %s" % (n, K, " or [%d]" % n if K == 1 else "", alpha.shape))
        alpha = _c(alpha)
    return K, squeeze, sv, lv, alpha, offsets


def _trial_fields(rec, count):
    return np.frombuffer(rec, dtype=np.dtype([(f, np.float64 if t is C.c_double else np.int32) for f, t in T.TrialRecord._fields_]),
                         count=count).copy()


def _trial_cost(ctx, descs, state_step, lm_step, alpha, base, best, call):
    n = len(descs)
    K, squeeze, sv, lv, al, offsets = trial_cost_args(descs, state_step, lm_step, alpha)
    rec = (T.TrialRecord * (n * K))()
    brec = (T.TrialRecord * n)() if base else None
    bk = np.full(n, -2, np.int32) if best else None
    ctx._check(call(K, _p(sv), _p(lv), _p(al), brec, rec, T.iptr(bk) if best else None))
    a = _trial_fields(rec, n * K).reshape(n, K)
    if squeeze:
        a = a[:, 0]
    names = [f for f, _ in T.TrialRecord._fields_]
    b = TrialBase(*[_trial_fields(brec, n)[f] for f in names]) if base else None
    return TrialCost(*[a[f] for f in names], b, bk, K, offsets)


class Batch:
    """Device-resident batch of windows (vilo_batch)."""

    def __init__(self, ctx, windows):
        self.ctx, self.windows = ctx, windows
        n = len(windows)
        self._descs = (T.WindowDesc * n)()
        self._states = (T.WindowState * n)()
        for i, w in enumerate(windows):
            d, s = w.desc(T)
            self._descs[i], self._states[i] = d, s
        self.handle = C.c_void_p()
        ctx._check(lib().vilo_batch_create(ctx.h, n, self._descs, self._states, C.byref(self.handle)))

    def reset(self):
        self.ctx._check(lib().vilo_batch_reset(self.ctx.h, self.handle))

    def prepare(self):
        """sqrt_info of every preintegration record again (what the reference does per IMULegFactor::Evaluate), asynchronous."""
        self.ctx._check(lib().vilo_batch_prepare(self.ctx.h, self.handle))

    def set_samples(self, on=True):
        """BASELINE configs[2]: keep the windows' samples in HBM and integrate every interval again (repropagate) at the biases of
        every point the solver linearises; on=False goes back to records integrated once."""
        if not on:
            self.ctx._check(lib().vilo_batch_set_samples(self.ctx.h, self.handle, None, None))
            return
        samples, offsets = window_samples(self.windows)
        self.ctx._check(lib().vilo_batch_set_samples(self.ctx.h, self.handle, C.cast(samples.ctypes.data, C.POINTER(T.Sample)), T.iptr(offsets)))

    def repropagate(self, samples=None, offsets=None, point="state", select="all", write=True, lin=None, mask=None,
                    thresholds=T.REPROP_THRESHOLDS):
        """vilo_batch_repropagate: the selected intervals' preintegration records integrated again once, at the chosen point, and
        prepared again; the solves that follow run on them. Repropagation(drift [W, 10, 3] = |point - the record's lin_ba / lin_bg /
        lin_rho| of the records as they were, selected [W, 10], status [W, 10] (T.REPROP_*)). point / select / lin / mask / thresholds:
        see reprop_opts. write=False is the drift query: nothing is integrated and the batch is left as it was. samples [n, 35] and
        offsets [W * 10 + 1] as for vilo_batch_set_samples; with write and without samples they are built from the windows' samples /
        sample_offsets, exactly as set_samples builds them."""
        if write and samples is None and offsets is None:
            samples, offsets = window_samples(self.windows)
        return _repropagate(self.ctx, len(self._descs), samples, offsets, point, select, write, lin, mask, thresholds,
                            lambda *a: lib().vilo_batch_repropagate(self.ctx.h, self.handle, *a))

    def marginalize(self, modes, priors_out):
        """vilo_batch_marginalize at the batch's device state (call download() first: the windows' arrays are the host copy of it).
        priors_out: one synth.PriorData per window."""
        n = len(self.windows)
        m = (C.c_int * n)(*modes)
        outs = (T.Prior * n)()
        for i, p in enumerate(priors_out):
            p.rebind()
            outs[i] = p.struct
        self.ctx._check(lib().vilo_batch_marginalize(self.ctx.h, self.handle, n, self._descs, self._states, m, outs))
        for i, p in enumerate(priors_out):
            C.memmove(C.byref(p.struct), C.byref(outs[i]), C.sizeof(T.Prior))
            p.rebind()

    def covariance(self, gauge="frame0", poses=False, min_reciprocal_condition=1e-14):
        """vilo_batch_covariance at the batch's device state (normally right after solve()): (frames [W, 11, 19, 19], poses [W, 79, 79] or
        None, status [W]). gauge: 'frame0' (frame 0's position and world yaw held) or 'none' (H^-1). The batch is left as it was."""
        n = len(self.windows)
        o = _cov_opts(gauge, poses, min_reciprocal_condition)
        frames, status = np.zeros((n, T.F, T.COV_FRAME, T.COV_FRAME)), np.zeros(n, np.int32)
        pz = np.zeros((n, T.COV_POSES, T.COV_POSES)) if poses else None
        self.ctx._check(lib().vilo_batch_covariance(self.ctx.h, self.handle, C.byref(o), _p(frames), _p(pz), T.iptr(status)))
        return frames, pz, status

    def landmark_covariance(self, gauge="frame0", frames=False, poses=False, min_reciprocal_condition=1e-14):
        """vilo_batch_landmark_covariance at the batch's device state: LandmarkCovariance(inv_depth_var [sum L], points [sum L, 3],
        point_cov [sum L, 3, 3], offsets [W + 1] (window w's landmarks: offsets[w] .. offsets[w + 1], in its own order), status [W],
        frames [W, 11, 19, 19] or None, poses [W, 79, 79] or None). The batch is left as it was."""
        return _landmark_covariance(self.ctx, [d.n_landmarks for d in self._descs], gauge, frames, poses, min_reciprocal_condition,
                                    lambda o, *out: lib().vilo_batch_landmark_covariance(self.ctx.h, self.handle, C.byref(o), *out))

    def residuals(self, outlier_threshold_px=3.0, observations=False, imu=False):
        """vilo_batch_residuals at the batch's device state: Residuals(per-window cost, prior_cost, imu_cost [W, 10], visual_cost,
        visual_cost_plain, n_visual_blocks, n_huber_active, n_outliers, n_negative_depth, status, then lm_cost / lm_reproj_px / lm_flags
        [sum L] (window w's landmarks: offsets[w] .. offsets[w + 1], in its own order), offsets [W + 1], obs_residuals [sum n_obs, 4] or
        None, imu_residuals [W, 10, 31] or None). The batch is left as it was."""
        return _residuals(self.ctx, self._descs, outlier_threshold_px, observations, imu,
                          lambda o, *out: lib().vilo_batch_residuals(self.ctx.h, self.handle, o, *out))

    def mask_landmarks(self, source="given", mask=None, combine="replace", flag_bits=3, outlier_threshold_px=3.0):
        """vilo_batch_mask_landmarks: takes landmarks out of the resident batch on the device (removeOutlier): until the mask changes,
        solve / download / residuals / marginalize behave as on a batch built without them. Returns (mask [sum L] uint8: the mask in
        force, window w's landmarks at offsets[w] .. offsets[w + 1] in its own order, MaskRecords(status (T.MASK_*), n_landmarks,
        n_masked, n_newly_masked, n_obs_left, each [W], offsets [W + 1])). source / mask / combine / flag_bits: see mask_opts. A batch
        without landmarks comes back with records of zeros. covariance, landmark_covariance, gradient, triangulate, frame_pose_pnp and
        predict_next_frame raise (VILO_ERR_UNSUPPORTED) while a landmark is masked."""
        return _mask_landmarks(self.ctx, self._descs, source, mask, combine, flag_bits, outlier_threshold_px,
                               lambda *a: lib().vilo_batch_mask_landmarks(self.ctx.h, self.handle, *a))

    def clear_mask(self):
        """mask_landmarks(source='clear'): every landmark back, the flag image restored bit for bit."""
        return self.mask_landmarks(source="clear")

    def gradient(self, state=True, diag=True, landmarks=True):
        """vilo_batch_gradient at the batch's device state: Gradient(per-window max_norm, norm, scaled_max, argmax_kind, argmax_index,
        argmax_component, n_free, status [W], then state_grad / state_diag [W, 222] (pose 11 x 6, speed-bias 11 x 9, leg bias 11 x 4,
        extrinsics 2 x 6, td) or None, lm_grad / lm_diag [sum L] (window w's landmarks: offsets[w] .. offsets[w + 1], in its own order) or
        None, offsets [W + 1]). state / landmarks leave the arrays of that side out, diag the two diagonals. The batch is left as it was."""
        return _gradient(self.ctx, self._descs, state, diag, landmarks, lambda *out: lib().vilo_batch_gradient(self.ctx.h, self.handle, *out))

    def triangulate(self, select="unset", mask=None, write=False, init_depth=5.0, stereo=True, shift=False):
        """vilo_batch_triangulate at the batch's device state: Triangulation(depth [sum L], flags [sum L] (T.TRI_* bits), offsets [W + 1]
        (window w's landmarks: offsets[w] .. offsets[w + 1], in its own order), shift_inv_depth [sum L] or None). select: 'unset' (inverse
        depth not positive), 'all', 'mask' (mask [sum L] non-zero). write=True stores 1 / depth as the current inverse depth of the selected
        landmarks; otherwise the batch is left as it was."""
        return _triangulate(self.ctx, self._descs, select, mask, write, init_depth, stereo, shift,
                            lambda *a: lib().vilo_batch_triangulate(self.ctx.h, self.handle, *a))

    def frame_pose_pnp(self, frame=-1, guess="previous", write=False, max_iterations=20, step_tolerance=1e-12):
        """vilo_batch_frame_pose_pnp at the batch's device state: FramePose(pose [W, 7] as [px py pz qx qy qz qw], final_cost, initial_cost,
        n_points, iterations, status (T.PNP_*), each [W]) of frame `frame` (-1: each window's last) from the landmarks that have depth.
        write=True stores the pose of the windows with status T.PNP_OK as that frame's current pose; otherwise the batch is left as it was."""
        return _frame_pose_pnp(self.ctx, len(self._descs), frame, guess, write, max_iterations, step_tolerance,
                               lambda *a: lib().vilo_batch_frame_pose_pnp(self.ctx.h, self.handle, *a))

    def gyro_bias_align(self, linearization="record", write=False):
        """vilo_batch_gyro_bias_align at the batch's device state: GyroAlignment(delta_bg [W, 3], initial_cost, model_cost, n_intervals,
        status (T.GYRO_*), each [W]): the gyro-bias step that makes the records' preintegrated rotations agree with the poses
        (solveGyroscopeBias). write=True adds it to every frame's gyro bias of the windows with status T.GYRO_OK; otherwise the batch is
        left as it was."""
        return _gyro_bias_align(self.ctx, len(self._descs), linearization, write,
                                lambda *a: lib().vilo_batch_gyro_bias_align(self.ctx.h, self.handle, *a))

    def predict_next_frame(self, mode="constant_velocity", next_pose=None, right=False):
        """vilo_batch_predict_next_frame at the batch's device state: NextFramePrediction(pts_cam [sum L, 3], pts_cam_right [sum L, 3] or
        None, flags [sum L] (T.PREDICT_* bits), offsets [W + 1] (window w's landmarks: offsets[w] .. offsets[w + 1], in its own order),
        next_pose [W, 7], n_predicted, status (T.PREDICT_*), each [W]): the landmarks whose tracks reach the last frame, in the left (and
        with right=True the right) camera of the next frame, whose pose is the last two frames' motion applied once more
        (predictPtsInNextFrame) or, with mode='given', the caller's next_pose [W, 7]. The batch is left as it was."""
        return _predict_next_frame(self.ctx, self._descs, mode, next_pose, right,
                                   lambda *a: lib().vilo_batch_predict_next_frame(self.ctx.h, self.handle, *a))

    def dead_reckon(self, samples, offsets, from_frame=-1, write=False, trajectory=False):
        """vilo_batch_dead_reckon at the batch's device state: DeadReckoning(state [W, 10] as [P, qx qy qz qw, V], trajectory
        [sum n_steps, 10] or None, step_offsets [W + 1] (window w's trajectory rows: step_offsets[w] .. step_offsets[w + 1]), n_steps,
        status (T.DR_*), each [W]): frame from_frame (-1: each window's last) carried through the window's samples
        [offsets[w], offsets[w + 1]) of samples [n, 35] by the mid-point recurrence of processIMULeg, the first sample of a range playing
        (acc_0, gyr_0). The quaternion is not normalised. write=True stores the result as the pose and velocity of frame from_frame + 1 of
        the windows with status T.DR_OK; otherwise the batch is left as it was."""
        return _dead_reckon(self.ctx, len(self._descs), samples, offsets, from_frame, write, trajectory,
                            lambda *a: lib().vilo_batch_dead_reckon(self.ctx.h, self.handle, *a))

    def leg_dead_reckon(self, samples, offsets, from_frame=-1, trajectory=False):
        """vilo_batch_leg_dead_reckon at the batch's device state: LegDeadReckoning(state [W, 32]: sum_dt, delta_q x y z w, delta_v,
        delta_eps (12), sum_delta_eps, fused world position, the last step's contact flags (4), two zeros; legs [W, 4, 3], the legs' world
        positions; trajectory [sum n_steps, 48] or None: sum_dt, fused world position and velocity, flags (4), the legs' world velocities
        (12), weights (12), the feet in the world (12), a zero; step_offsets [W + 1]; n_steps and status (T.DR_*), each [W]): frame
        from_frame (-1: each window's last) dead-reckoned by leg odometry through the window's samples [offsets[w], offsets[w + 1])
        (the first sample of a range is the start sample). Nothing of the batch changes. A batch without leg factors raises."""
        return _leg_dead_reckon(self.ctx, len(self._descs), samples, offsets, from_frame, trajectory,
                                lambda *a: lib().vilo_batch_leg_dead_reckon(self.ctx.h, self.handle, *a))

    def dead_reckon_covariance(self, samples, offsets, cov_in=None, from_frame=-1, pose_trajectory=False):
        """vilo_batch_dead_reckon_covariance at the batch's device state: DeadReckonedCovariance(state [W, 10], bit for bit
        dead_reckon()'s; cov [W, 15, 15] over (dp, dtheta, dv, dba, dbg), bitwise symmetric; pose_cov_trajectory [sum n_steps, 6, 6] or
        None, the pose block after every step; step_offsets [W + 1]; n_steps and status (T.DR_*), each [W]): the covariance cov_in
        [W, 15, 15] (None: zero; only its upper triangle is read; dr_cov_in() cuts it out of covariance()'s frames) of frame from_frame
        (-1: each window's last) carried through the window's samples by Sigma <- F Sigma F^T + V Q V^T. The batch is left as it was."""
        return _dead_reckon_covariance(self.ctx, len(self._descs), samples, offsets, cov_in, from_frame, pose_trajectory,
                                       lambda *a: lib().vilo_batch_dead_reckon_covariance(self.ctx.h, self.handle, *a))

    def leg_dead_reckon_covariance(self, samples, offsets, cov_in=None, from_frame=-1, pose_trajectory=False, leg_trajectory=False):
        """vilo_batch_leg_dead_reckon_covariance at the batch's device state: LegDeadReckonedCovariance(state [W, 32] and legs [W, 4, 3],
        bit for bit leg_dead_reckon()'s; cov [W, 31, 31] over (dp, dtheta, dv, deps_1..4, dba, dbg, drho_1..4), dp dv deps in the world
        frame, bitwise symmetric; pose_cov_trajectory [sum n_steps, 6, 6] or None, the pose block after every step; leg_cov_trajectory
        [sum n_steps, 4, 3, 3] or None, the covariance of each leg's world position after every step; step_offsets [W + 1]; n_steps and
        status (T.DR_*), each [W]): the covariance cov_in [W, 19, 19] (None: zero; only its upper triangle is read; leg_dr_cov_in() cuts
        it out of covariance()'s frames) of frame from_frame (-1: each window's last) carried through the window's samples by
        Sigma <- F Sigma F^T + V Q V^T of IMULegIntegrationBase::midPointIntegration. The batch is left as it was. A batch without leg
        factors raises."""
        return _leg_dead_reckon_covariance(self.ctx, len(self._descs), samples, offsets, cov_in, from_frame, pose_trajectory, leg_trajectory,
                                           lambda *a: lib().vilo_batch_leg_dead_reckon_covariance(self.ctx.h, self.handle, *a))

    def gauge_fix(self, anchor="uploaded", anchor_pose=None, pose0_before=False):
        """vilo_batch_gauge_fix, in place on the batch's device state (normally right after solve()): double2vector's re-anchoring of yaw
        and position to frame 0 as it was before the solve, every velocity rotated, every pose and free extrinsic quaternion normalised.
        GaugeFix(yaw_diff_deg, singular, status (T.GAUGE_*), each [W], pose0_before [W, 7] or None: the solver's frame-0 pose that was
        replaced). anchor: 'uploaded' (frame 0 of the state the batch was created with) or 'given' (anchor_pose [W, 7]). download()
        afterwards gives the windows' arrays the fixed state, which is what marginalize() expects."""
        return _gauge_fix(self.ctx, len(self._descs), anchor, anchor_pose, pose0_before,
                          lambda *a: lib().vilo_batch_gauge_fix(self.ctx.h, self.handle, *a))

    def failure_detection(self, last_track_num=None, last_pose=None):
        """vilo_batch_failure_detection at the batch's device state: FailureDetection(flags (T.FAILURE_* bits), would_reboot, status
        (T.FAILURE_OK / T.FAILURE_NUMERIC), each [W], values [W, 6]: the compared quantities in bit order): every criterion of
        Estimator::failureDetection on each window's last frame. last_track_num [W] (bit 0) and last_pose [W, 7] (bits 3 to 5) are the
        caller's; None leaves their bits 0. The batch is left as it was."""
        return _failure_detection(self.ctx, len(self._descs), last_track_num, last_pose,
                                  lambda *a: lib().vilo_batch_failure_detection(self.ctx.h, self.handle, *a))

    def retract(self, state_step=None, lm_step=None, alpha=None, base="current"):
        """vilo_batch_retract, in place on the batch's device state: x <- x [+] alpha * step in the local coordinates gradient() reports
        (state_step [W, 222] as state_grad, lm_step [sum L] as lm_grad, alpha [W] or None for 1; see retract_opts). Pose and extrinsic
        blocks take PoseLocalParameterization::Plus (bit for bit Context.pose_plus), the others x + alpha * step, each product and sum
        rounded once. Constant blocks, the rows of absent frames and masked landmarks are not stepped and their step entries not read. A
        window with a non-finite alpha or applied step entry is left as it is (status T.RETRACT_NUMERIC). base='uploaded' steps the state
        the batch was created with (reset() and the step in one launch). Retraction(status (T.RETRACT_*), n_applied, step_norm, step_max,
        each [W]). reset(), the records, the mask and the summaries are not affected."""
        return _retract(self.ctx, self._descs, base, state_step, lm_step, alpha,
                        lambda *a: lib().vilo_batch_retract(self.ctx.h, self.handle, *a))

    def gauss_newton_step(self, mu=None, gauge="none", state=True, landmarks=True, min_lm_diagonal=1e-6, max_lm_diagonal=1e32,
                          min_pivot=1e-14):
        """vilo_batch_gauss_newton_step at the batch's device state: the solution delta of (H + mu D^2 / s^2) delta = -g (Ceres' Jacobi
        scale s and clamped D^2; see gn_step_opts and include/vilo_gpu.h), inverse depths included, in gradient()'s layouts, so that
        retract(r.state_step, r.lm_step) applies it. GaussNewtonStep(state_step [W, 222], lm_step [sum L], offsets, and per window
        model_cost_change, scaled_norm, norm, grad_dot_step, n_free, status). A window of status 1 or 2 reads NaN. The batch is left as
        it was."""
        return _gn_step(self.ctx, self._descs, mu, gauge, state, landmarks, min_lm_diagonal, max_lm_diagonal, min_pivot,
                        lambda *a: lib().vilo_batch_gauss_newton_step(self.ctx.h, self.handle, *a))

    def dogleg_step(self, radius, mu=None, gauge="none", cauchy=False, min_lm_diagonal=1e-6, max_lm_diagonal=1e32, min_pivot=1e-14):
        """vilo_batch_dogleg_step at the batch's device state: Ceres' traditional dogleg step for the trust-region radius `radius` (a
        scalar or [W], in the D-scaled space) and the damping mu of its Gauss-Newton point (gauss_newton_step's mu), from one
        linearisation; in gradient()'s layouts, so that trial_cost(r.state_step, r.lm_step) and retract(r.state_step, r.lm_step) take it.
        DoglegStep(state_step [W, 222], lm_step [sum L], cauchy_state, cauchy_lm (the Cauchy point -alpha s o (g^ / D); None unless
        cauchy=True), offsets, and per window alpha, gradient_norm, gauss_newton_norm, step_norm, beta, model_cost_change, grad_dot_step,
        norm, branch (0 Gauss-Newton, 1 Cauchy-limited, 2 interpolated), n_free, status). A window of status 1 or 2 reads NaN. The
        batch is left as it was."""
        return _dogleg_step(self.ctx, self._descs, radius, mu, gauge, cauchy, min_lm_diagonal, max_lm_diagonal, min_pivot,
                            lambda *a: lib().vilo_batch_dogleg_step(self.ctx.h, self.handle, *a))

    def hessian_vector(self, state_vec=None, lm_vec=None, state=True, landmarks=True):
        """vilo_batch_hessian_vector at the batch's device state: y = H v for K vectors per window, H the Gauss-Newton Hessian of
        gradient() and gauss_newton_step() (inverse depths part of the system, undamped, no gauge). state_vec [W, 222] or [W, K, 222],
        lm_vec [K sum L] (see hess_vec_args; None: zero). HessianVector(state_out [W, K, 222], lm_out [K sum L] (hess_vec_lm_block),
        offsets, n_vec, and per (window, vector) vHv, g_dot_v, model_cost_change = -g.v - vHv / 2, status); one vector given as
        [W, 222] returns [W, 222] and [W]. Entries of constant blocks and absent frames are not read and read 0 in the output. A
        vector with a non-finite read entry reads NaN (status 1), the others are untouched. The batch is left as it was."""
        return _hess_vec(self.ctx, self._descs, state_vec, lm_vec, state, landmarks,
                         lambda *a: lib().vilo_batch_hessian_vector(self.ctx.h, self.handle, *a))

    def set_state(self, window_ids, windows):
        """vilo_batch_set_state: the state arrays of windows[i] (synth.Window, or anything with desc()) replace the current device state
        of window window_ids[i]; the windows that are not named, and what reset() restores, stay as they are."""
        ids = np.ascontiguousarray(window_ids, dtype=np.int32)
        if ids.ndim != 1 or len(ids) != len(windows):
            raise ValueError("window_ids and windows must have the same length, got %s and %d" % (ids.shape, len(windows)))
        states = (T.WindowState * max(len(windows), 1))()
        for i, w in enumerate(windows):
            states[i] = w.desc(T)[1]
        self.ctx._check(lib().vilo_batch_set_state(self.ctx.h, self.handle, len(ids), T.iptr(ids), states))

    def trial_cost(self, state_step=None, lm_step=None, alpha=None, base=True, best=True):
        """vilo_batch_trial_cost: the cost at x [+] alpha[w][k] * step_k for K <= 16 steps per window, the batch left exactly as it is.
        state_step [W, K, 222] (or [W, 222]: one step), lm_step [K sum L] in hessian_vector's layout (hess_vec_lm_block views it), alpha
        [W, K] or None for 1 (see trial_cost_args). TrialCost(cost, visual_cost, imu_cost (the intervals' sum), prior_cost, cost_change
        (base cost - cost), n_negative_depth, status (T.TRIAL_*) [W, K] ([W] for one step given as [W, 222] / [sum L]), base (TrialBase
        of [W] arrays: the same at x itself) or None, best [W] (the lowest-cost OK step that lowers the cost, -1: none) or None, n_steps,
        offsets). The trial states are bit for bit what retract() would leave; commit a step with retract()."""
        return _trial_cost(self.ctx, self._descs, state_step, lm_step, alpha, base, best,
                           lambda *a: lib().vilo_batch_trial_cost(self.ctx.h, self.handle, *a))

    def save_state(self):
        """vilo_batch_save_state: the current device state into the batch's one snapshot slot (allocated at the first call)."""
        self.ctx._check(lib().vilo_batch_save_state(self.ctx.h, self.handle))

    def restore_state(self):
        """vilo_batch_restore_state: the saved state back, bit for bit; raises (VILO_ERR_UNSUPPORTED) before any save_state()."""
        self.ctx._check(lib().vilo_batch_restore_state(self.ctx.h, self.handle))

    def solve(self, opts):
        self.ctx._check(lib().vilo_batch_solve(self.ctx.h, self.handle, C.byref(opts)))
        return lib().vilo_last_solve_ms(self.ctx.h)

    def download(self):
        """Write the solver output into the windows' state arrays; returns the list of summaries."""
        n = len(self.windows)
        summ = (T.SolveSummary * n)()
        self.ctx._check(lib().vilo_batch_download(self.ctx.h, self.handle, self._states, summ))
        return list(summ)

    def path(self):
        """vilo_debug_batch_path: which form of each step the last solve() ran, by name (T.PATH_AXES), plus "replay" (the solve replayed
        the captured launch sequence) and "wave_order" (VILO_WAVE_ORDER at creation)."""
        out = np.zeros(8, np.int32)
        rc = lib().vilo_debug_batch_path(self.handle, T.iptr(out))
        if rc != 0:
            raise ViloError("vilo_debug_batch_path -> %d (no solve yet)" % rc)
        d = {name: codes[int(out[i])] for i, (name, codes) in enumerate(T.PATH_AXES)}
        d["replay"], d["wave_order"] = bool(out[6]), int(out[7])
        return d

    def device_bytes(self):
        """vilo_debug_batch_device_bytes: (bytes of the arena chunks the batch holds, bytes handed out of them)."""
        out = (C.c_size_t * 2)()
        self.ctx._check(lib().vilo_debug_batch_device_bytes(self.handle, C.cast(out, T.c_size_t_p)))
        return int(out[0]), int(out[1])

    def fetch(self, what, win=0, max_n=1 << 22):
        out = np.zeros(max_n)
        n = lib().vilo_debug_fetch(self.ctx.h, self.handle, what, win, _p(out), max_n)
        if n < 0:
            raise ViloError("vilo_debug_fetch(%d) -> %d" % (what, n))
        return out[:n].copy()

    def close(self):
        if self.handle:
            lib().vilo_batch_destroy(self.ctx.h, self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PreintStreams:
    """vilo_preint_streams: device-resident IMULegIntegrationBase objects updated by push_back as samples arrive."""

    def __init__(self, ctx, n, imu_only=False):
        self.ctx, self.n, self.imu_only = ctx, n, imu_only
        self.h = C.c_void_p()
        ctx._check((lib().vilo_preint_streams_create_imu if imu_only else lib().vilo_preint_streams_create)(ctx.h, n, C.byref(self.h)))

    def reset(self, ids, first, lin):
        ids, first, lin = np.ascontiguousarray(ids, np.int32), _c(first), _c(lin)
        self.ctx._check(lib().vilo_preint_streams_reset(self.ctx.h, self.h, len(ids), T.iptr(ids), C.cast(first.ctypes.data, C.POINTER(T.Sample)), _p(lin)))

    def push(self, ids, samples, offsets):
        ids, samples, offsets = np.ascontiguousarray(ids, np.int32), _c(samples), np.ascontiguousarray(offsets, np.int32)
        self.ctx._check(lib().vilo_preint_streams_push(self.ctx.h, self.h, len(ids), T.iptr(ids), C.cast(samples.ctypes.data, C.POINTER(T.Sample)),
                                                       T.iptr(offsets)))

    def read(self, ids):
        ids = np.ascontiguousarray(ids, np.int32)
        if self.imu_only:
            out = np.zeros((len(ids), T.PREINT_IMU_DOUBLES))
            self.ctx._check(lib().vilo_preint_streams_read_imu(self.ctx.h, self.h, len(ids), T.iptr(ids), C.cast(out.ctypes.data, C.POINTER(T.PreintImu))))
            return out
        out = np.zeros((len(ids), T.PREINT_DOUBLES))
        self.ctx._check(lib().vilo_preint_streams_read(self.ctx.h, self.h, len(ids), T.iptr(ids), C.cast(out.ctypes.data, C.POINTER(T.Preint))))
        return out

    def close(self):
        if self.h:
            lib().vilo_preint_streams_destroy(self.ctx.h, self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PriorPool:
    """vilo_prior_pool: last_marginalization_info objects whose J0 / r0 stay on the device between frames."""

    def __init__(self, ctx, n_slots):
        self.ctx, self.n = ctx, n_slots
        self.h = C.c_void_p()
        ctx._check(lib().vilo_prior_pool_create(ctx.h, n_slots, C.byref(self.h)))

    def upload(self, slot, prior):
        self.ctx._check(lib().vilo_prior_pool_upload(self.ctx.h, self.h, slot, C.byref(prior.struct) if prior is not None else None))

    def download(self, slot, prior_out):
        prior_out.rebind()
        self.ctx._check(lib().vilo_prior_pool_download(self.ctx.h, self.h, slot, C.byref(prior_out.struct)))
        return prior_out

    def dim(self, slot):
        return lib().vilo_prior_pool_dim(self.h, slot)

    def close(self):
        if self.h:
            lib().vilo_prior_pool_destroy(self.ctx.h, self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Context:
    def __init__(self, cfg, device=0):
        self.cfg = cfg
        self.h = C.c_void_p()
        rc = lib().vilo_create(C.byref(self.h), C.byref(cfg), device)
        if rc != 0:
            raise ViloError("vilo_create failed (%d): no usable HIP device %d; this library has no CPU path" % (rc, device))

    def close(self):
        if self.h:
            lib().vilo_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            raise ViloError("vilo error %d: %s" % (rc, lib().vilo_last_error(self.h).decode()))

    SOLVER_FORMS = {"auto": -1, "wave": 0, "split": 3, "mw8": 4}

    def set_solver_form(self, form):
        """vilo_set_solver_form: 'auto' (by batch size), 'wave', 'split' (bitwise equal to 'wave'), 'mw8'."""
        self._check(lib().vilo_set_solver_form(self.h, self.SOLVER_FORMS[form]))

    def set_gn_step_form(self, form):
        """vilo_set_gn_step_form: 'streamed' (default: the coupling through global memory, two workgroups per CU) or 'resident' (in LDS,
        one workgroup per CU); the same definition, kept for measurement."""
        self._check(lib().vilo_set_gn_step_form(self.h, {"streamed": 0, "resident": 1}[form]))

    def set_prior_form(self, form):
        """vilo_set_prior_form: 'eigen' (J0 = sqrt(S) V^T like the reference, default) or 'factor' (pivoted Cholesky factor where no
        eigenvalue would be dropped: same J0^T J0 / J0^T r0, a quarter of a single window's marginalisation time)."""
        self._check(lib().vilo_set_prior_form(self.h, {"eigen": 0, "factor": 1}[form]))

    def set_compact_rows(self, on):
        """vilo_set_compact_rows: batches created afterwards may / may not use the compact 16-column visual rows."""
        self._check(lib().vilo_set_compact_rows(self.h, 1 if on else 0))

    # ---- ceres::CostFunction-shaped batched evaluation ----
    def eval_proj(self, kind, obs, params, want_jac=True):
        """kind 0/1/2 = TwoFrameOneCam / TwoFrameTwoCam / OneFrameTwoCam; params: list of (n, size) arrays."""
        obs = _c(obs)
        n = obs.shape[0]
        params = [_c(p) for p in params]
        sizes = [[7, 7, 7, 1, 1], [7, 7, 7, 7, 1, 1], [7, 7, 1, 1]][kind]
        r = np.zeros((n, 2))
        Js = [np.zeros((n, 2, s)) for s in sizes] if want_jac else [None] * len(sizes)
        fn = [lib().vilo_eval_proj2f1c, lib().vilo_eval_proj2f2c, lib().vilo_eval_proj1f2c][kind]
        self._check(fn(self.h, n, _p(obs), *[_p(p) for p in params], _p(r), *[_p(j) for j in Js]))
        return r, Js

    def eval_imu_leg(self, preint, params, want_jac=True):
        preint = _c(preint)
        n = preint.shape[0]
        params = [_c(p) for p in params]
        sizes = [7, 9, 4, 7, 9, 4]
        r = np.zeros((n, 31))
        Js = [np.zeros((n, 31, s)) for s in sizes] if want_jac else [None] * 6
        self._check(lib().vilo_eval_imu_leg(self.h, n, C.cast(preint.ctypes.data, C.POINTER(T.Preint)), *[_p(p) for p in params],
                                            _p(r), *[_p(j) for j in Js]))
        return r, Js

    def eval_imu(self, preint, params, want_jac=True):
        preint = _c(preint)
        n = preint.shape[0]
        params = [_c(p) for p in params]
        sizes = [7, 9, 7, 9]
        r = np.zeros((n, 15))
        Js = [np.zeros((n, 15, s)) for s in sizes] if want_jac else [None] * 4
        self._check(lib().vilo_eval_imu(self.h, n, C.cast(preint.ctypes.data, C.POINTER(T.PreintImu)), *[_p(p) for p in params],
                                        _p(r), *[_p(j) for j in Js]))
        return r, Js

    def eval_prior(self, prior, params_concat, want_jac=True):
        """prior: synth.PriorData; params_concat: (n_eval, sum of global block sizes)."""
        pc = _c(params_concat)
        n_eval = pc.shape[0]
        n = prior.struct.n
        sg = sum(prior.struct.block_size[k] for k in range(prior.struct.n_blocks))
        r = np.zeros((n_eval, n))
        J = np.zeros((n_eval, n, sg)) if want_jac else None
        self._check(lib().vilo_eval_prior(self.h, n_eval, C.byref(prior.struct), _p(pc), _p(r), _p(J)))
        return r, J

    def pose_plus(self, x, d):
        x, d = _c(x), _c(d)
        out = np.zeros_like(x)
        self._check(lib().vilo_pose_plus(self.h, x.shape[0], _p(x), _p(d), _p(out)))
        return out

    # ---- preintegration ----
    def preintegrate(self, samples, offsets, lin):
        samples, lin = _c(samples), _c(lin)
        offsets = np.ascontiguousarray(offsets, dtype=np.int32)
        n = offsets.shape[0] - 1
        out = np.zeros((n, T.PREINT_DOUBLES))
        self._check(lib().vilo_preintegrate(self.h, n, C.cast(samples.ctypes.data, C.POINTER(T.Sample)), T.iptr(offsets), _p(lin),
                                            C.cast(out.ctypes.data, C.POINTER(T.Preint))))
        return out

    def preintegrate_imu(self, samples, offsets, lin6):
        samples, lin6 = _c(samples), _c(lin6)
        offsets = np.ascontiguousarray(offsets, dtype=np.int32)
        n = offsets.shape[0] - 1
        out = np.zeros((n, T.PREINT_IMU_DOUBLES))
        self._check(lib().vilo_preintegrate_imu(self.h, n, C.cast(samples.ctypes.data, C.POINTER(T.Sample)), T.iptr(offsets),
                                                _p(lin6), C.cast(out.ctypes.data, C.POINTER(T.PreintImu))))
        return out

    def preintegrate_window(self, w):
        """Fill w.preint (and w.preint_imu) from w.samples on the GPU."""
        w.preint[...] = self.preintegrate(w.samples, w.sample_offsets, w.lin)
        w.preint_imu[...] = self.preintegrate_imu(w.samples, w.sample_offsets, np.ascontiguousarray(w.lin[:, :6]))

    def preintegrate_windows(self, windows):
        """One launch for all intervals of all windows."""
        samples = np.concatenate([w.samples[: w.sample_offsets[-1]] for w in windows])
        offs, base = [0], 0
        for w in windows:
            offs.extend((w.sample_offsets[1:] + base).tolist())
            base += int(w.sample_offsets[-1])
        lin = np.concatenate([w.lin for w in windows])
        out = self.preintegrate(samples, np.array(offs, np.int32), lin)
        k = 0
        for w in windows:
            w.preint[...] = out[k:k + w.F - 1]
            k += w.F - 1

    # ---- solve ----
    def solve_windows(self, windows, opts=None):
        """Estimator::optimization() solve half on a list of windows; states updated in place."""
        opts = opts or default_solve_opts()
        n = len(windows)
        descs, states = (T.WindowDesc * n)(), (T.WindowState * n)()
        for i, w in enumerate(windows):
            descs[i], states[i] = w.desc(T)
        return self.solve_window_descs(descs, states, opts)

    def solve_window_descs(self, descs, states, opts):
        """vilo_solve_windows on descriptor arrays the caller built (and keeps alive); VILO_ERR_NUMERIC is a per-window outcome
        (termination 2 in that window's summary), everything else raises."""
        n = len(descs)
        summ = (T.SolveSummary * n)()
        rc = lib().vilo_solve_windows(self.h, n, descs, states, C.byref(opts), summ)
        if rc != -4:   # VILO_ERR_NUMERIC
            self._check(rc)
        return list(summ)

    def set_host_pipeline(self, lanes, sub_windows=1024):
        """vilo_set_host_pipeline: how vilo_solve_windows cuts a call with many host windows into sub-batches (lanes < 2: never)."""
        self._check(lib().vilo_set_host_pipeline(self.h, lanes, sub_windows))

    def gauge_fix(self, before_arrays, w):
        keep = [np.ascontiguousarray(a) for a in before_arrays]
        sb = T.WindowState()
        sb.pose, sb.speed_bias, sb.leg_bias, sb.ex_pose, sb.td, sb.inv_depth = [T.dptr(k) for k in keep]
        _, sa = w.desc(T)
        self._check(lib().vilo_gauge_fix(self.h, 1, C.byref(sb), C.byref(sa), w.F))

    def window_covariance(self, windows, gauge="frame0", poses=False, min_reciprocal_condition=1e-14):
        """vilo_window_covariance: the covariance of host windows at their current state arrays (see Batch.covariance)."""
        n = len(windows)
        descs, states = (T.WindowDesc * n)(), (T.WindowState * n)()
        for i, w in enumerate(windows):
            descs[i], states[i] = w.desc(T)
        o = _cov_opts(gauge, poses, min_reciprocal_condition)
        frames, status = np.zeros((n, T.F, T.COV_FRAME, T.COV_FRAME)), np.zeros(n, np.int32)
        pz = np.zeros((n, T.COV_POSES, T.COV_POSES)) if poses else None
        self._check(lib().vilo_window_covariance(self.h, n, descs, states, C.byref(o), _p(frames), _p(pz), T.iptr(status)))
        return frames, pz, status

    def window_landmark_covariance(self, windows, gauge="frame0", frames=False, poses=False, min_reciprocal_condition=1e-14):
        """vilo_window_landmark_covariance: the landmark covariance of host windows at their current state arrays (see
        Batch.landmark_covariance)."""
        n = len(windows)
        descs, states = (T.WindowDesc * n)(), (T.WindowState * n)()
        for i, w in enumerate(windows):
            descs[i], states[i] = w.desc(T)
        return _landmark_covariance(self, [d.n_landmarks for d in descs], gauge, frames, poses, min_reciprocal_condition,
                                    lambda o, *out: lib().vilo_window_landmark_covariance(self.h, n, descs, states, C.byref(o), *out))

    def window_residuals(self, windows, outlier_threshold_px=3.0, observations=False, imu=False):
        """vilo_window_residuals: the residuals of host windows at their current state arrays (see Batch.residuals)."""
        n = len(windows)
        descs, states = (T.WindowDesc * n)(), (T.WindowState * n)()
        for i, w in enumerate(windows):
            descs[i], states[i] = w.desc(T)
        return _residuals(self, descs, outlier_threshold_px, observations, imu,
                          lambda o, *out: lib().vilo_window_residuals(self.h, n, descs, states, o, *out))

    def window_mask_landmarks(self, windows, source="given", mask=None, combine="replace", flag_bits=3, outlier_threshold_px=3.0):
        """vilo_window_mask_landmarks: the mask and records of host windows at their current state arrays (see Batch.mask_landmarks);
        what it is for is source='outlier_flags', the device's selection."""
        n = len(windows)
        descs, states = (T.WindowDesc * n)(), (T.WindowState * n)()
        for i, w in enumerate(windows):
            descs[i], states[i] = w.desc(T)
        return _mask_landmarks(self, descs, source, mask, combine, flag_bits, outlier_threshold_px,
                               lambda *a: lib().vilo_window_mask_landmarks(self.h, n, descs, states, *a))

    def window_gradient(self, windows, state=True, diag=True, landmarks=True):
        """vilo_window_gradient: the gradient of host windows at their current state arrays (see Batch.gradient)."""
        n = len(windows)
        descs, states = (T.WindowDesc * n)(), (T.WindowState * n)()
        for i, w in enumerate(windows):
            descs[i], states[i] = w.desc(T)
        return _gradient(self, descs, state, diag, landmarks, lambda *out: lib().vilo_window_gradient(self.h, n, descs, states, *out))

    def window_triangulate(self, windows, select="unset", mask=None, write=False, init_depth=5.0, stereo=True, shift=False):
        """vilo_window_triangulate: the depths of host windows' landmarks at their current state arrays (see Batch.triangulate); with
        write=True the windows' inv_depth arrays receive the new values."""
        n = len(windows)
        descs, states = (T.WindowDesc * n)(), (T.WindowState * n)()
        for i, w in enumerate(windows):
            descs[i], states[i] = w.desc(T)
        return _triangulate(self, descs, select, mask, write, init_depth, stereo, shift,
                            lambda *a: lib().vilo_window_triangulate(self.h, n, descs, states, *a))

    def window_frame_pose_pnp(self, windows, frame=-1, guess="previous", write=False, max_iterations=20, step_tolerance=1e-12):
        """vilo_window_frame_pose_pnp: the PnP pose of a frame of host windows at their current state arrays (see Batch.frame_pose_pnp);
        with write=True the windows' pose arrays receive the new row."""
        n = len(windows)
        descs, states = (T.WindowDesc * n)(), (T.WindowState * n)()
        for i, w in enumerate(windows):
            descs[i], states[i] = w.desc(T)
        return _frame_pose_pnp(self, n, frame, guess, write, max_iterations, step_tolerance,
                               lambda *a: lib().vilo_window_frame_pose_pnp(self.h, n, descs, states, *a))

    def window_gyro_bias_align(self, windows, linearization="record", write=False):
        """vilo_window_gyro_bias_align: the gyro-bias alignment of host windows at their current state arrays (see Batch.gyro_bias_align);
        with write=True the windows' speed_bias arrays receive the new gyro biases."""
        n = len(windows)
        descs, states = (T.WindowDesc * n)(), (T.WindowState * n)()
        for i, w in enumerate(windows):
            descs[i], states[i] = w.desc(T)
        return _gyro_bias_align(self, n, linearization, write,
                                lambda *a: lib().vilo_window_gyro_bias_align(self.h, n, descs, states, *a))

    def window_predict_next_frame(self, windows, mode="constant_velocity", next_pose=None, right=False):
        """vilo_window_predict_next_frame: the next-frame prediction of host windows' landmarks at their current state arrays (see
        Batch.predict_next_frame)."""
        n = len(windows)
        descs, states = (T.WindowDesc * n)(), (T.WindowState * n)()
        for i, w in enumerate(windows):
            descs[i], states[i] = w.desc(T)
        return _predict_next_frame(self, descs, mode, next_pose, right,
                                   lambda *a: lib().vilo_window_predict_next_frame(self.h, n, descs, states, *a))

    def window_dead_reckon(self, windows, samples, offsets, from_frame=-1, write=False, trajectory=False):
        """vilo_window_dead_reckon: the dead reckoning of host windows at their current state arrays (see Batch.dead_reckon); with
        write=True the windows' pose and speed_bias arrays receive the new rows."""
        n = len(windows)
        descs, states = (T.WindowDesc * n)(), (T.WindowState * n)()
        for i, w in enumerate(windows):
            descs[i], states[i] = w.desc(T)
        return _dead_reckon(self, n, samples, offsets, from_frame, write, trajectory,
                            lambda *a: lib().vilo_window_dead_reckon(self.h, n, descs, states, *a))

    def window_leg_dead_reckon(self, windows, samples, offsets, from_frame=-1, trajectory=False):
        """vilo_window_leg_dead_reckon: Batch.leg_dead_reckon of host windows at their current state arrays."""
        n = len(windows)
        descs, states = (T.WindowDesc * n)(), (T.WindowState * n)()
        for i, w in enumerate(windows):
            descs[i], states[i] = w.desc(T)
        return _leg_dead_reckon(self, n, samples, offsets, from_frame, trajectory,
                                lambda *a: lib().vilo_window_leg_dead_reckon(self.h, n, descs, states, *a))

    def window_dead_reckon_covariance(self, windows, samples, offsets, cov_in=None, from_frame=-1, pose_trajectory=False):
        """vilo_window_dead_reckon_covariance: Batch.dead_reckon_covariance of host windows at their current state arrays."""
        n = len(windows)
        descs, states = (T.WindowDesc * n)(), (T.WindowState * n)()
        for i, w in enumerate(windows):
            descs[i], states[i] = w.desc(T)
        return _dead_reckon_covariance(self, n, samples, offsets, cov_in, from_frame, pose_trajectory,
                                       lambda *a: lib().vilo_window_dead_reckon_covariance(self.h, n, descs, states, *a))

    def window_leg_dead_reckon_covariance(self, windows, samples, offsets, cov_in=None, from_frame=-1, pose_trajectory=False, leg_trajectory=False):
        """vilo_window_leg_dead_reckon_covariance: Batch.leg_dead_reckon_covariance of host windows at their current state arrays."""
        n = len(windows)
        descs, states = (T.WindowDesc * n)(), (T.WindowState * n)()
        for i, w in enumerate(windows):
            descs[i], states[i] = w.desc(T)
        return _leg_dead_reckon_covariance(self, n, samples, offsets, cov_in, from_frame, pose_trajectory, leg_trajectory,
                                           lambda *a: lib().vilo_window_leg_dead_reckon_covariance(self.h, n, descs, states, *a))

    def window_gauge_fix(self, windows, anchor="given", anchor_pose=None, pose0_before=False):
        """vilo_window_gauge_fix: the gauge fix of host windows at their current state arrays, each with its own number of frames (see
        Batch.gauge_fix); the windows' pose, speed_bias and ex_pose arrays receive the fixed rows. anchor_pose [n, 7]: frame 0 as it was
        before the solve."""
        n = len(windows)
        descs, states = (T.WindowDesc * n)(), (T.WindowState * n)()
        for i, w in enumerate(windows):
            descs[i], states[i] = w.desc(T)
        return _gauge_fix(self, n, anchor, anchor_pose, pose0_before, lambda *a: lib().vilo_window_gauge_fix(self.h, n, descs, states, *a))

    def window_failure_detection(self, windows, last_track_num=None, last_pose=None):
        """vilo_window_failure_detection: the failure criteria of host windows at their current state arrays (see Batch.failure_detection)."""
        n = len(windows)
        descs, states = (T.WindowDesc * n)(), (T.WindowState * n)()
        for i, w in enumerate(windows):
            descs[i], states[i] = w.desc(T)
        return _failure_detection(self, n, last_track_num, last_pose,
                                  lambda *a: lib().vilo_window_failure_detection(self.h, n, descs, states, *a))

    def window_repropagate(self, windows, samples=None, offsets=None, point="state", select="all", write=True, lin=None, mask=None,
                           thresholds=T.REPROP_THRESHOLDS):
        """vilo_window_repropagate: the re-propagation of host windows' records at their current state arrays (see Batch.repropagate);
        with write=True the windows' preint (use_leg == 0: preint_imu) arrays receive the selected records."""
        n = len(windows)
        descs, states = (T.WindowDesc * n)(), (T.WindowState * n)()
        for i, w in enumerate(windows):
            descs[i], states[i] = w.desc(T)
        if write and samples is None and offsets is None:
            samples, offsets = window_samples(windows)
        return _repropagate(self, n, samples, offsets, point, select, write, lin, mask, thresholds,
                            lambda *a: lib().vilo_window_repropagate(self.h, n, descs, states, *a))

    def window_retract(self, windows, state_step=None, lm_step=None, alpha=None, base="current"):
        """vilo_window_retract: the step of host windows at their current state arrays (see Batch.retract); the windows' state arrays
        receive the stepped state."""
        n = len(windows)
        descs, states = (T.WindowDesc * n)(), (T.WindowState * n)()
        for i, w in enumerate(windows):
            descs[i], states[i] = w.desc(T)
        return _retract(self, descs, base, state_step, lm_step, alpha, lambda *a: lib().vilo_window_retract(self.h, n, descs, states, *a))

    def window_gauss_newton_step(self, windows, mu=None, gauge="none", state=True, landmarks=True, min_lm_diagonal=1e-6,
                                 max_lm_diagonal=1e32, min_pivot=1e-14):
        """vilo_window_gauss_newton_step: the step of host windows at their current state arrays (see Batch.gauss_newton_step)."""
        n = len(windows)
        descs, states = (T.WindowDesc * n)(), (T.WindowState * n)()
        for i, w in enumerate(windows):
            descs[i], states[i] = w.desc(T)
        return _gn_step(self, descs, mu, gauge, state, landmarks, min_lm_diagonal, max_lm_diagonal, min_pivot,
                        lambda *a: lib().vilo_window_gauss_newton_step(self.h, n, descs, states, *a))

    def window_dogleg_step(self, windows, radius, mu=None, gauge="none", cauchy=False, min_lm_diagonal=1e-6, max_lm_diagonal=1e32,
                           min_pivot=1e-14):
        """vilo_window_dogleg_step: the dogleg step of host windows at their current state arrays (see Batch.dogleg_step)."""
        n = len(windows)
        descs, states = (T.WindowDesc * n)(), (T.WindowState * n)()
        for i, w in enumerate(windows):
            descs[i], states[i] = w.desc(T)
        return _dogleg_step(self, descs, radius, mu, gauge, cauchy, min_lm_diagonal, max_lm_diagonal, min_pivot,
                            lambda *a: lib().vilo_window_dogleg_step(self.h, n, descs, states, *a))

    def window_trial_cost(self, windows, state_step=None, lm_step=None, alpha=None, base=True, best=True):
        """vilo_window_trial_cost: the trial costs of host windows at their current state arrays (see Batch.trial_cost)."""
        n = len(windows)
        descs, states = (T.WindowDesc * n)(), (T.WindowState * n)()
        for i, w in enumerate(windows):
            descs[i], states[i] = w.desc(T)
        return _trial_cost(self, descs, state_step, lm_step, alpha, base, best,
                           lambda *a: lib().vilo_window_trial_cost(self.h, n, descs, states, *a))

    def window_hessian_vector(self, windows, state_vec=None, lm_vec=None, state=True, landmarks=True):
        """vilo_window_hessian_vector: the products of host windows at their current state arrays (see Batch.hessian_vector)."""
        n = len(windows)
        descs, states = (T.WindowDesc * n)(), (T.WindowState * n)()
        for i, w in enumerate(windows):
            descs[i], states[i] = w.desc(T)
        return _hess_vec(self, descs, state_vec, lm_vec, state, landmarks,
                         lambda *a: lib().vilo_window_hessian_vector(self.h, n, descs, states, *a))

    def marginalize(self, w, mode, prior_out):
        d, s = w.desc(T)
        self._check(lib().vilo_marginalize(self.h, 1, C.byref(d), C.byref(s), mode, C.byref(prior_out.struct)))


def window_trial_cost(ctx, windows, state_step=None, lm_step=None, alpha=None, base=True, best=True):
    """Context.window_trial_cost as a function: the host-window form of Batch.trial_cost."""
    return ctx.window_trial_cost(windows, state_step, lm_step, alpha, base, best)
