"""CPU: the numpy definition of vilo_batch_gyro_bias_align (tests/gyro_ref.py): the measured FP64 floor that sets the GPU tolerance
(gyro_ref.TOL = 10 x gyro_ref.FLOOR), the identity on IMU-propagated poses, recovery of a known bias, the quadratic
convergence of the corrected form, the option parsing of the Python wrapper, the struct sizes and the library's exports.
tests/test_gyro_align_gpu.py takes its cases from here."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import gyro_ref
from conftest import ROOT
from test_triangulate import SHAPES, shape_window


@functools.lru_cache(maxsize=None)
def kind_window(name, use_leg):
    """the packing shape's window for the factor kind: use_leg == 0 reads the IMU records, and holds the leg biases constant as a window
    without leg factors has none to estimate (tests/test_covariance_gpu.py's imu_only case)"""
    w = shape_window(name).twin()
    if not use_leg:
        w.use_leg, w.leg_bias_const = 0, 1
    return w


@functools.lru_cache(maxsize=None)
def solved_kind_window(name, use_leg):
    """after the oracle's 4-iteration solve: the CPU stand-in for the state the GPU parity test reaches"""
    from cerberus_amd import synth
    from oracle import oracle_py as O
    w = kind_window(name, use_leg).twin()
    O.solve_window(O.config_from(synth.default_config()), w, O.default_opts(True, 4))
    return w


def cases():
    """(tag, window) of every case: the four packing shapes (the six-frame window among them) x use_leg 1, 0 x initial, solved"""
    out = []
    for name in sorted(SHAPES):
        for use_leg in (1, 0):
            out.append(("%s use_leg %d initial" % (name, use_leg), kind_window(name, use_leg)))
            out.append(("%s use_leg %d solved" % (name, use_leg), solved_kind_window(name, use_leg)))
    return out


def _ulp_moved(p, rng):
    """the inputs with every pose quaternion, delta_q and Jacobian entry moved by one unit in the last place"""
    def mv(a):
        return np.nextafter(a, np.where(rng.random(a.shape) < 0.5, -np.inf, np.inf))
    return p._replace(q=mv(p.q), dq=mv(p.dq), J=mv(p.J))


def test_fp64_floor_measured():
    """Prints the floor of the definition over the cases and both linearizations: (a) one unit in the last place on every quaternion,
    delta_q and Jacobian entry, (b) numpy.linalg.solve on the normal equations against numpy.linalg.lstsq on the stacked rows.
    gyro_ref.FLOOR / FLOOR_COST must cover the larger. The synthetic robot keeps its attitude near the identity, so the vector parts of
    all quaternions are small and a unit in their last place is 1e-18: the residuals carry 1e-17 of rounding, which the step's
    sensitivity |A^-1 J^T| ~ 1 / sum_dt ~ 15 turns into 1e-16.
    Measured (x86-64, numpy's LAPACK): step (a) 1.5e-16 (b) 6.2e-17; initial_cost (a) 1.8e-13, model_cost (a) 1.8e-13 (relative)."""
    rng = np.random.default_rng(19)
    wa = wb = wc = wm = 0.0
    for tag, w in cases():
        p = gyro_ref.parts(w)
        for lin in ("record", "corrected"):
            r = gyro_ref.align_parts(p, lin)
            assert r.status == gyro_ref.OK and r.n_intervals == w.F - 1, tag
            for _ in range(4):
                m = gyro_ref.align_parts(_ulp_moved(p, rng), lin)
                wa = max(wa, gyro_ref.step_error(m.delta_bg, r.delta_bg))
                wc = max(wc, abs(m.initial_cost - r.initial_cost) / r.initial_cost)
                wm = max(wm, abs(m.model_cost - r.model_cost) / r.model_cost)
            wb = max(wb, gyro_ref.step_error(gyro_ref.align_lstsq(p, lin), r.delta_bg))
    print("MEASURED floor: step (a) %.1e (b) %.1e; initial_cost (a) %.1e, model_cost (a) %.1e" % (wa, wb, wc, wm))
    assert max(wa, wb) <= gyro_ref.FLOOR
    assert max(wc, wm) <= gyro_ref.FLOOR_COST
    assert gyro_ref.TOL == 10 * gyro_ref.FLOOR and 10 * gyro_ref.FLOOR_COST <= gyro_ref.TOL_COST == 1e-10


def test_linearizations_coincide_at_the_records_point():
    """state biases = the records' linearisation point: the correction is deltaQ(0), the identity"""
    for name in ("L9", "F6"):
        for use_leg in (1, 0):
            w = kind_window(name, use_leg).twin()
            p = gyro_ref.parts(w)
            w.speed_bias[:w.F - 1, 6:9] = p.lin_bg
            a, b = gyro_ref.align(w, "record"), gyro_ref.align(w, "corrected")
            assert a.delta_bg.tobytes() == b.delta_bg.tobytes() and a.initial_cost == b.initial_cost


def test_identity_on_propagated_poses():
    for tag, w in cases():
        t = gyro_ref.propagated(w)
        for lin in ("record", "corrected"):
            r = gyro_ref.align(t, lin)
            assert r.status == gyro_ref.OK, tag
            assert np.abs(r.delta_bg).max() <= gyro_ref.TOL, (tag, lin, r.delta_bg)


def _second_order_bound(ref, d):
    """what the linear model leaves of the true residual at d, carried through the least-squares solution: |pinv(J)| |r - J d|"""
    e = ref.r - np.einsum("kij,j->ki", ref.J, d)
    return float(np.linalg.norm(np.linalg.pinv(ref.J.reshape(-1, 3)), 2) * np.linalg.norm(e))


def test_recovers_a_known_bias():
    """Records rotated by Exp(-J_k d) on propagated poses return d up to what the linear model leaves. The inequality that carries the
    test is bound <= |d|^2 with bound = |pinv(J)| |r - J d|, the remainder of the true residual at d carried through the least-squares
    solution (measured 3.9e-13, the third-order term of 2 vec(Exp(theta)), against |d|^2 = 1e-6): a residual of the wrong sign, scale or
    block leaves r - J d of the order of |J d| = 7e-5 and a bound of 1e-3. err <= bound then holds by the algebra of least squares
    (delta_bg - d = pinv(J) (r - J d)) and only checks that align() solves the system it states."""
    d = 1e-3 * np.array([0.6, -0.48, 0.64])   # |d| = 1e-3 rad/s
    for tag, w in cases():
        t = gyro_ref.with_rotated_records(gyro_ref.propagated(w), d)
        r = gyro_ref.align(t)
        assert r.status == gyro_ref.OK, tag
        err = float(np.abs(r.delta_bg - d).max())
        bound = _second_order_bound(r, d) + gyro_ref.TOL
        print("MEASURED %s: |delta_bg - d| %.1e, second-order bound %.1e" % (tag, err, bound))
        assert bound <= np.dot(d, d), (tag, bound)
        assert err <= bound, (tag, err, bound)


def test_corrected_form_converges_quadratically():
    """write-back and a second call: |d2| <= QUADRATIC_K |d1|^2 + TOL with the fixed constant of gyro_ref (2 s/rad: the largest ratio
    measured here on the definition, 1.05, doubled). The record form, which does not see the written bias, returns the first step
    again and misses the same bound: the bound tells a correction from none."""
    K = gyro_ref.QUADRATIC_K
    worst = 0.0
    for tag, w in cases():
        first = gyro_ref.align(w, "corrected")
        assert first.status == gyro_ref.OK, tag
        t = gyro_ref.with_gyro_bias(w, first.delta_bg)
        second = gyro_ref.align(t, "corrected")
        n1, n2 = np.linalg.norm(first.delta_bg), np.linalg.norm(second.delta_bg)
        worst = max(worst, n2 / n1 ** 2)
        print("MEASURED %s: |d1| %.2e |d2| %.2e, |d2| / |d1|^2 %.2e (K = %.1f)" % (tag, n1, n2, n2 / n1 ** 2, K))
        assert n2 <= K * n1 ** 2 + gyro_ref.TOL, (tag, n1, n2)
        rec1, rec2 = gyro_ref.align(w, "record"), gyro_ref.align(t, "record")
        assert rec2.delta_bg.tobytes() == rec1.delta_bg.tobytes()
        m1 = np.linalg.norm(rec1.delta_bg)
        assert m1 > K * m1 ** 2 + gyro_ref.TOL, (tag, m1)
    print("MEASURED largest |d2| / |d1|^2: %.2e" % worst)
    assert worst <= 0.75 * K   # (the constant keeps its margin over what is measured)


def test_pose_quaternions_of_either_hemisphere():
    """q and -q are one rotation: negating stored pose quaternions changes no bit of the result (the reference forms q_ij from rotation
    matrices)"""
    for tag, w in cases():
        t = w.twin()
        t.pose[1:w.F:2, 3:7] *= -1.0
        for lin in ("record", "corrected"):
            a, b = gyro_ref.align(w, lin), gyro_ref.align(t, lin)
            assert a.delta_bg.tobytes() == b.delta_bg.tobytes() and a.initial_cost == b.initial_cost and a.model_cost == b.model_cost, tag
            assert (a.r == b.r).all()


def test_statuses_of_the_definition():
    w = kind_window("L9", 1)
    p = gyro_ref.parts(w)
    assert gyro_ref.align_parts(p._replace(J=np.zeros_like(p.J))).status == gyro_ref.SINGULAR
    bad = p.dq.copy()
    bad[3, 1] = np.nan
    r = gyro_ref.align_parts(p._replace(dq=bad))
    assert r.status == gyro_ref.NUMERIC and not r.delta_bg.any() and np.isnan(r.initial_cost)
    none = gyro_ref.Parts(p.q[:1], p.dq[:0], p.lin_bg[:0], p.J[:0], p.bg[:1])
    r = gyro_ref.align_parts(none)
    assert (r.status, r.n_intervals) == (gyro_ref.NO_INTERVALS, 0) and not r.delta_bg.any()
    # a two-frame window has one interval and a full-rank block
    two = gyro_ref.Parts(p.q[:2], p.dq[:1], p.lin_bg[:1], p.J[:1], p.bg[:2])
    assert gyro_ref.align_parts(two).status == gyro_ref.OK


def test_wrapper_options_need_no_device():
    from cerberus_amd import _ctypes as T
    from cerberus_amd import api
    o = api.gyro_opts()
    assert (o.linearization, o.write) == (0, 0)
    o = api.gyro_opts("corrected", True)
    assert (o.linearization, o.write) == (1, 1)
    with pytest.raises(ValueError):
        api.gyro_opts("exact")
    assert api.GyroAlignment._fields == ("delta_bg", "initial_cost", "model_cost", "n_intervals", "status")
    assert (T.GYRO_OK, T.GYRO_NO_INTERVALS, T.GYRO_SINGULAR, T.GYRO_NUMERIC) == \
        (gyro_ref.OK, gyro_ref.NO_INTERVALS, gyro_ref.SINGULAR, gyro_ref.NUMERIC)


def _header_struct(name):
    hdr = open(os.path.join(ROOT, "include", "vilo_gpu.h")).read()
    end = hdr.index("} %s;" % name)
    body = hdr[hdr.rindex("typedef struct {", 0, end):end]
    return [ln.split(";")[0].split() for ln in body.splitlines()[1:] if ";" in ln]


def test_struct_sizes_match_the_header():
    from cerberus_amd import _ctypes as T
    size = {"int32_t": 4, "double": 8}
    for name, mirror, want in (("vilo_gyro_opts", T.GyroOpts, 8), ("vilo_window_gyro_record", T.WindowGyroRecord, 24)):
        fields = _header_struct(name)
        assert [f for f, _ in mirror._fields_] == [f[-1] for f in fields]
        assert [C.sizeof(t) for _, t in mirror._fields_] == [size[f[0]] for f in fields]
        assert C.sizeof(mirror) == sum(size[f[0]] for f in fields) == want
    hdr = open(os.path.join(ROOT, "include", "vilo_gpu.h")).read()
    for k, v in (("RECORD", 0), ("CORRECTED", 1), ("OK", 0), ("NO_INTERVALS", 1), ("SINGULAR", 2), ("NUMERIC", 3)):
        assert re.search(r"#define VILO_GYRO_%s %d\b" % (k, v), hdr), k
    # the offsets gyro_ref reads the records at are the header's
    assert T.PREINT_DOUBLES == 33 + 2 * 31 * 31 and T.PREINT_IMU_DOUBLES == 17 + 2 * 15 * 15
    assert [n for n, _ in T.Preint._fields_][:7] == ["sum_dt", "delta_p", "delta_q", "delta_v", "delta_eps", "lin_ba", "lin_bg"]
    assert T.Preint.delta_q.offset == 8 * 4 and T.Preint.lin_bg.offset == 8 * 26 and T.Preint.jacobian.offset == 8 * 33
    assert T.PreintImu.delta_q.offset == 8 * 4 and T.PreintImu.lin_bg.offset == 8 * 14 and T.PreintImu.jacobian.offset == 8 * 17


def test_library_exports_the_entry_points():
    lib = C.CDLL(os.path.join(ROOT, "cerberus_amd", "lib", "libvilo_gpu.so"))
    for name in ("vilo_default_gyro_opts", "vilo_batch_gyro_bias_align", "vilo_window_gyro_bias_align", "vilo_last_gyro_align_ms"):
        assert hasattr(lib, name), name
    from cerberus_amd import _ctypes as T
    o = T.GyroOpts(7, 7)
    lib.vilo_default_gyro_opts(C.byref(o))   # host code: needs no device
    assert (o.linearization, o.write) == (0, 0)
