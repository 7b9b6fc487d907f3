"""CPU: the numpy definition of vilo_batch_predict_next_frame (tests/predict_ref.py): the measured FP64 floor that sets the GPU tolerance
(predict_ref.TOL = 10 x predict_ref.FLOOR), the link to the oracle's ProjectionTwoFrameOneCam factor (which is pinned against
the reference's own source), the constant-velocity identity, the selection on ragged tracks, what the skew-extrinsics window is there for,
and the option parsing of the Python wrapper. tests/test_predict_gpu.py takes its windows and references from here."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import field_windows
import predict_ref
import tri_ref
from conftest import ROOT
from test_triangulate import SHAPES, shape_window, solved_window

FIELD = ("f40", "f70_chunks", "f60_partial8")
MODES = ("constant_velocity", "given")
# every predicted |pts_cam.z| of a parity case is at least this far from 0: bit 1 cannot flip by rounding
Z_CLEAR = 1000 * predict_ref.TOL


def skew_extrinsics(w):
    """the same window with both extrinsics replaced by skew rotations (tens of degrees about axes of their own) and translations of
    decimetres: at the generator's near-identity ric a transposed ric or a dropped tic is all but invisible"""
    t = w.twin()
    t.ex_pose[0] = [0.21, -0.13, 0.08] + list(np.array([0.3, -0.2, 0.25, 0.9]) / np.linalg.norm([0.3, -0.2, 0.25, 0.9]))
    t.ex_pose[1] = [0.19, 0.17, -0.06] + list(np.array([-0.15, 0.35, 0.1, 0.92]) / np.linalg.norm([-0.15, 0.35, 0.1, 0.92]))
    return t


def given_pose(w):
    """the pose a VILO_PREDICT_GIVEN parity case hands in: centimetres and about two degrees off the constant-velocity one (frame k's own
    pose where the window has two frames), its quaternion not normalised"""
    base = predict_ref.constant_velocity_pose(w) if w.F >= 3 else w.pose[w.F - 1].copy()
    dq = np.array([0.01, -0.02, 0.015, 1.0])
    return np.concatenate([base[:3] + [0.05, -0.03, 0.02], 1.7 * predict_ref.quat_mul(base[3:7], dq / np.linalg.norm(dq))])


@functools.lru_cache(maxsize=None)
def field_window(name, solved=False):
    from cerberus_amd import synth
    from oracle import oracle_py as O
    cfg = synth.default_config()
    w = field_windows.field_window(cfg, O.config_from(cfg), name)
    if solved:
        O.solve_window(O.config_from(cfg), w, O.default_opts(True, field_windows.ITERS))
    return w


def parity_cases():
    """(tag, window) of every window the GPU parity test runs, at the initial state and after a 4-iteration solve (the oracle's: the CPU
    stand-in for the state the device reaches; the two agree to 1e-8)"""
    out = []
    for state, solved in (("initial", False), ("solved", True)):
        for name in SHAPES:
            out.append(("%s %s" % (name, state), solved_window(name) if solved else shape_window(name)))
        for name in FIELD:
            out.append(("%s %s" % (name, state), field_window(name, solved)))
        out.append(("L70 skew extrinsics %s" % state, skew_extrinsics(solved_window("L70") if solved else shape_window("L70"))))
    return out


def _ulp_moved(w, g, rng):
    """the window (and the given pose) with every pose, extrinsic, observation point and inverse depth moved by one unit in the last
    place, up or down"""
    t = w.twin()
    t.obs = w.obs.copy()
    g = g.copy()
    for a in (t.pose, t.ex_pose, t.obs[:, 0:3], t.inv_depth, g):
        a[...] = np.nextafter(a, np.where(rng.random(a.shape) < 0.5, -np.inf, np.inf))
    return t, g


def _quat_of(R, like):
    """[x y z w] of the rotation matrix R, in the hemisphere of `like`"""
    w = 0.5 * np.sqrt(max(0.0, 1.0 + R[0, 0] + R[1, 1] + R[2, 2]))
    q = np.array([(R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w), w])
    return q if q @ like >= 0 else -q


def test_parity_cases_are_what_the_gpu_test_needs():
    """every case predicts some landmark, the field windows leave some out, and every predicted z is clear of zero in both cameras"""
    names = [t for t, _ in parity_cases()]
    assert len(set(names)) == len(names) == 2 * (len(SHAPES) + len(FIELD) + 1)
    for tag, w in parity_cases():
        for mode in MODES:
            r = predict_ref.window_prediction(w, mode, given_pose(w) if mode == "given" else None, right=True)
            assert r.status == predict_ref.OK and r.n_predicted > 0, tag
            assert r.n_predicted < w.L or not tag.startswith("f"), (tag, r.n_predicted, w.L)   # (a field window: ragged tracks)
            # in front of both cameras and finite; the skew copy's right camera looks away from some landmarks (bit 3: parity covers it)
            assert not (r.flags & ~np.uint8(predict_ref.PREDICTED | (predict_ref.BEHIND_RIGHT if "skew" in tag else 0))).any(), tag
            assert (np.abs(r.pts_cam[r.selected, 2]) >= Z_CLEAR).all() and (np.abs(r.pts_cam_right[r.selected, 2]) >= Z_CLEAR).all(), tag


def test_fp64_floor_measured():
    """Prints the floor of the definition over every parity case, both modes, both cameras: (a) one unit in the last place on the inputs,
    (b) the reference's 4 x 4 homogeneous product against the header's quaternion form; predict_ref.FLOOR must cover the largest.
    Measured (x86-64): points (a) 1.3e-15 (b) 6.0e-16; pose (a) 2.2e-16 (b) 1.1e-16."""
    rng = np.random.default_rng(11)
    pa = pb = qa = qb = 0.0
    for tag, w in parity_cases():
        for mode in MODES:
            g = given_pose(w)
            r = predict_ref.window_prediction(w, mode, g if mode == "given" else None, right=True)
            for _ in range(3):
                wm, gm = _ulp_moved(w, g, rng)
                m = predict_ref.window_prediction(wm, mode, gm if mode == "given" else None, right=True)
                assert (m.flags == r.flags).all(), tag
                pa = max(pa, predict_ref.point_error(m.pts_cam, r.pts_cam), predict_ref.point_error(m.pts_cam_right, r.pts_cam_right))
                qa = max(qa, predict_ref.pose_error(m.next_pose, r.next_pose))
        P4, R4 = predict_ref.constant_velocity_pose_4x4(w)
        pose = predict_ref.constant_velocity_pose(w)
        Rq = tri_ref.quat_R(pose[3:7])
        for cam in (0, 1):
            pb = max(pb, predict_ref.point_error(predict_ref.points(w, P4, R4, cam), predict_ref.points(w, pose[:3], Rq, cam)))
        qb = max(qb, predict_ref.pose_error(np.concatenate([P4, _quat_of(R4, pose[3:7])]), pose))
    print("MEASURED floor: points (a) %.1e (b) %.1e; pose (a) %.1e (b) %.1e; FLOOR %.0e, TOL %.0e"
          % (pa, pb, qa, qb, predict_ref.FLOOR, predict_ref.TOL))
    assert max(pa, pb, qa, qb) <= predict_ref.FLOOR
    assert predict_ref.TOL == 10 * predict_ref.FLOOR


def test_link_to_the_pinned_projection_factor(cfg, ocfg):
    """VILO_PREDICT_GIVEN with the pose of frame k itself: pts_cam.xy / pts_cam.z - point_k.xy of a predicted landmark is the unwhitened
    residual of the oracle's ProjectionTwoFrameOneCam between its start frame and frame k (tests/test_oracle_vs_reference.py pins that
    factor against the reference's source). The observations' cur_td is set to the window's td: the factor's time-offset term is zero."""
    from oracle import oracle_py as O
    sq = cfg.focal_length / 1.5
    for w0 in (shape_window("L70"), field_window("f40"), skew_extrinsics(shape_window("L70"))):
        w = w0.twin()
        w.obs = w0.obs.copy()
        w.obs[:, 10] = w.td[0]
        k = w.F - 1
        r = predict_ref.window_prediction(w, "given", w.pose[k])
        assert r.n_predicted > 0
        worst = 0.0
        for l in np.flatnonzero(r.selected):
            o0, s = int(w.lm_obs_offset[l]), int(w.lm_start_frame[l])
            f0, fk = w.obs[o0], w.obs[o0 + k - s]
            obs = np.concatenate([f0[0:3], fk[0:3], f0[6:8], fk[6:8], [f0[10], fk[10]]])
            res, _ = O.eval_proj(0, ocfg, obs, [w.pose[s], w.pose[k], w.ex_pose[0], w.inv_depth[l:l + 1], w.td], want_jac=False)
            worst = max(worst, np.abs(r.pts_cam[l, :2] / r.pts_cam[l, 2] - fk[0:2] - res / sq).max())
        print("MEASURED link to ProjectionTwoFrameOneCam: %.1e (bound %.0e)" % (worst, predict_ref.TOL))
        assert worst <= predict_ref.TOL


def test_constant_velocity_identity():
    """frame k set to T_{k-1} (T_{k-2}^-1 T_{k-1}): the window without its last frame predicts that pose"""
    w = shape_window("L70").twin()
    k = w.F - 1
    Ps, Rs, _, _ = tri_ref.poses(w)
    T1, T2 = np.eye(4), np.eye(4)
    T1[:3, :3], T1[:3, 3] = Rs[k - 1], Ps[k - 1]
    T2[:3, :3], T2[:3, 3] = Rs[k - 2], Ps[k - 2]
    Tk = T1 @ (np.linalg.inv(T2) @ T1)
    t = w.twin()
    t.F = k   # frames 0 .. k - 1
    pose = predict_ref.constant_velocity_pose(t)
    want = np.concatenate([Tk[:3, 3], _quat_of(Tk[:3, :3], pose[3:7])])
    e = predict_ref.pose_error(pose, want)
    print("MEASURED constant-velocity identity: %.1e (bound %.0e)" % (e, predict_ref.TOL))
    assert e <= predict_ref.TOL
    # and with that pose in the window, predicting once more moves on by the same motion: not the identity
    w.pose[k] = want
    assert predict_ref.pose_error(predict_ref.constant_velocity_pose(w), want) > 1e-3


def test_selection_on_ragged_tracks(cfg, ocfg):
    w = field_windows.field_window(cfg, ocfg, "f200")
    w.inv_depth[::9] = -1.0
    r = predict_ref.window_prediction(w, right=True)
    want = np.array([w.lm_start_frame[l] + (w.lm_obs_offset[l + 1] - w.lm_obs_offset[l]) - 1 == w.F - 1 and w.inv_depth[l] > 0
                     for l in range(w.L)])
    assert want.any() and (~want).any() and (want & (np.arange(w.L) % 9 != 0)).any()
    ends = np.array([w.lm_start_frame[l] + (w.lm_obs_offset[l + 1] - w.lm_obs_offset[l]) - 1 == w.F - 1 for l in range(w.L)])
    assert (ends & ~want).any() and (~ends).any()   # both reasons to be left out occur
    np.testing.assert_array_equal((r.flags & predict_ref.PREDICTED) != 0, want)
    np.testing.assert_array_equal(r.selected, want)
    assert r.n_predicted == want.sum()
    assert not r.pts_cam[~want].any() and not r.pts_cam_right[~want].any() and not r.flags[~want].any()
    assert np.abs(r.pts_cam[want]).min(axis=1).max() > 0.0


def test_skew_extrinsics_show_a_transposed_ric_or_a_dropped_tic():
    """either mistake moves pts_cam of the skew copy by at least 1000 x TOL, in both cameras"""
    w = skew_extrinsics(shape_window("L70"))
    pose = predict_ref.constant_velocity_pose(w)
    Pn, Rn = pose[:3], tri_ref.quat_R(pose[3:7])
    for cam in (0, 1):
        good = predict_ref.points(w, Pn, Rn, cam)
        for kw in (dict(ric_transposed=True), dict(tic_dropped=True)):
            e = np.abs(predict_ref.points(w, Pn, Rn, cam, **kw) - good).max(axis=1) / np.maximum(1.0, np.abs(good).max(axis=1))
            print("MEASURED skew copy, camera %d, %s: moves pts_cam by %.1e .. %.1e" % (cam, list(kw)[0], e.min(), e.max()))
            assert e.min() >= 1000 * predict_ref.TOL


def test_wrapper_options_need_no_device():
    from cerberus_amd import _ctypes as T
    from cerberus_amd import api
    assert C.sizeof(T.PredictOpts) == 8 and C.sizeof(T.WindowPredictRecord) == 8
    o, p = api.predict_opts()
    assert (o.mode, o.pad) == (0, 0) and p is None
    o, p = api.predict_opts("given", [[0, 0, 0, 0, 0, 0, 1]] * 3, 3)
    assert o.mode == 1 and p.dtype == np.float64 and p.shape == (3, 7) and p.flags["C_CONTIGUOUS"]
    assert api.predict_opts("given", np.zeros((5, 7)))[1].shape == (5, 7)
    for a in (("steady",), ("given",), ("constant_velocity", np.zeros((1, 7))), ("given", np.zeros((2, 7)), 3), ("given", np.zeros((3, 6)), 3),
              ("given", np.zeros(7), 1)):
        with pytest.raises(ValueError):
            api.predict_opts(*a)
    assert api.NextFramePrediction._fields == ("pts_cam", "pts_cam_right", "flags", "offsets", "next_pose", "n_predicted", "status")
    assert (T.PREDICT_OK, T.PREDICT_TOO_FEW_FRAMES, T.PREDICT_NUMERIC) == (predict_ref.OK, predict_ref.TOO_FEW_FRAMES, predict_ref.NUMERIC)
    # the header's structs, constants and the mirrors agree
    hdr = open(os.path.join(ROOT, "include", "vilo_gpu.h")).read()
    for struct, first, name in ((T.PredictOpts, "int32_t mode;", "vilo_predict_opts"), (T.WindowPredictRecord, "int32_t n_predicted;", "vilo_window_predict_record")):
        body = hdr[hdr.index("typedef struct {\n  " + first):hdr.index("} %s;" % name)]
        assert [f for f, _ in struct._fields_] == [ln.split(";")[0].split()[-1] for ln in body.splitlines()[1:] if ";" in ln]
    for name, v in (("CONSTANT_VELOCITY", T.PREDICT_MODE["constant_velocity"]), ("GIVEN", T.PREDICT_MODE["given"]), ("OK", T.PREDICT_OK),
                    ("TOO_FEW_FRAMES", T.PREDICT_TOO_FEW_FRAMES), ("NUMERIC", T.PREDICT_NUMERIC)):
        assert "#define VILO_PREDICT_%s %d\n" % (name, v) in hdr
