"""CPU, oracle only: the alternative configuration of tests/alt_config.py can SEE every field it changes.

For each changed field (one at a time) the field goes back to its default, the inputs stay as they are, and what the field feeds is
computed again with the oracle: the ten preintegration records of a 40-landmark window, an IMU-leg and a projection factor's residual and
Jacobian, and the f40 field window's cost, gradient, Gauss-Newton step and four-iteration solve. Each movement is expressed in units of
the parity bound tests/test_alt_config_gpu.py applies to that quantity. Each field has the list of quantities the GPU suite computes from
the DEVICE's own read of it (DEVICE_SEES); the best of those must reach 1000. A field below that is not being tested, whatever the GPU
test says.

Which quantity carries a field matters. acc_w, gyr_w, rho_c_n and rho_nc_n move the covariance by less than its bounds but the whitened
factors by 0.1 .. 0.7: the device sees them where its own records are whitened and solved ("solved states" 1e4 .. 4e6). phi_n and dphi_n
move no device-computed quantity by more than 4 bounds at this configuration (6e4 only in a whitened Jacobian on records the oracle
integrated, which the device is handed, not its own): they have a preintegration-only case of their own, alt_config.joint_noise_config,
held here by test_joint_noise_case_sees_phi_n_and_dphi_n.

Fields that act under one contact model only are measured under that one: v_n_min_xy and v_n_min_z under the flag-based model (type 0),
v_n_min, v_n_force_thres_ratio, v_n_term1_steep and the two rescale terms under the force-based one (type 2, forces in newtons)."""
import numpy as np
import pytest

import alt_config as A
import field_windows as FW
import resid_ref
from cerberus_amd import synth
from oracle import oracle_py as O
from test_oracle_factors import _proj_setup
from test_oracle_vs_reference import force_samples

# What the GPU suite computes from the DEVICE's own read of a field, by the name moved() gives it. Only these count: a quantity the device
# gets handed (the whitened factor of test_eval_imu_leg_and_imu runs on records the oracle integrated) says nothing about the kernel
# that reads the field.
_RECORD = ("record state", "record jacobian")                      # test_preintegrate, test_golden's alt records
_COV = ("record covariance", "record covariance entries")          # test_preintegrate
_SOLVED = ("solved cost", "solved states")                         # test_whole_path_with_the_devices_own_preintegration, test_solve_with_repropagation
DEVICE_SEES = {
    "R_br": _RECORD, "p_br": _RECORD, "rho_fix": _RECORD,
    "g_norm": ("imu residual", "imu jacobian") + _SOLVED,          # test_eval_imu_leg_and_imu: the factor kernel reads g_norm itself
    "focal_length": ("proj residual", "proj jacobian", "visual cost"),          # test_eval_proj, test_residuals
    "huber_delta": ("visual cost", "gauss-newton step") + _SOLVED,              # test_residuals, test_linearization_..., test_kernel_paths
    "acc_n": _COV, "acc_n_z": _COV, "gyr_n": _COV, "v_n_min_xy": _COV, "v_n_min_z": _COV, "v_n_max": _COV,
    "v_n_min": _COV, "v_n_force_thres_ratio": _COV, "v_n_term1_steep": _COV, "v_n_term2_var_rescale": _COV, "v_n_term3_distance_rescale": _COV,
    # below the covariance's bounds (it is compared relative to its largest or to its significant entries), 0.1 .. 0.7 of the whitened
    # factors: seen where the device whitens and solves on its own records
    "acc_w": _SOLVED, "gyr_w": _SOLVED, "rho_c_n": _SOLVED, "rho_nc_n": _SOLVED,
    # no device-visible quantity at alt_config: the dedicated case below (alt_config.joint_noise_config)
    "phi_n": (), "dphi_n": (),
}
JOINT_NOISE = ("phi_n", "dphi_n")
TYPE2_ONLY = ("v_n_min", "v_n_force_thres_ratio", "v_n_term1_steep", "v_n_term2_var_rescale", "v_n_term3_distance_rescale")
NEED = 1000.0


def _rel(a, b):
    return np.abs(a - b).max() / max(1e-300, np.abs(b).max())


class _Inputs:
    """Inputs generated ONCE at the alternative configuration, per contact model."""

    def __init__(self, alt, ctype):
        self.ctype = ctype
        self.w40 = synth.make_window(alt, n_landmarks=40, seed=7)
        self.f40 = FW.field_window(alt, O.config_from(alt), "f40")
        if ctype == 2:
            self.w40.samples = force_samples(self.w40.samples, 3)
            self.f40.samples = force_samples(self.f40.samples, 3)
        self.f40_state = self.f40.clone_state()
        rng = np.random.default_rng(100)
        self.proj = [_proj_setup(rng, kind) for kind in (0, 1, 2)]


def quantities(cfg, inp):
    """Everything a configuration feeds, from fixed inputs."""
    oc = O.config_from(A.with_type(cfg, inp.ctype))
    q = {}
    w = inp.w40
    O.fill_preint(oc, w)
    q["record"] = w.preint.copy()
    P = [w.pose[:-1], w.speed_bias[:-1], w.leg_bias[:-1], w.pose[1:], w.speed_bias[1:], w.leg_bias[1:]]
    r, J = O.eval_imu_leg(oc, w.preint[3], [p[3] for p in P])
    q["imu_r"], q["imu_J"] = r, np.hstack(J)
    q["proj"] = [O.eval_proj(kind, oc, obs, prm) for kind, (obs, prm) in enumerate(inp.proj)]
    f = inp.f40
    f.set_state(inp.f40_state)
    O.fill_preint(oc, f)
    H, g, cost = O.window_normal_eq(oc, f)
    act = np.flatnonzero(np.diag(H) > 0)
    Hs, gs = H[np.ix_(act, act)], g[act]
    s = 1.0 / (1.0 + np.sqrt(np.diag(Hs)))
    dh2 = np.clip(s * s * np.diag(Hs), 1e-6, 1e32) / (s * s)       # (tests/test_gpu_parity.py::_check_linearization)
    q["cost0"], q["grad"], q["step"] = cost, g, np.linalg.solve(Hs + 1e-8 * np.diag(dh2), gs)
    res = resid_ref.window_residuals(oc, f)
    q["visual_cost"], q["n_huber_active"] = res["visual_cost"], res["n_huber_active"]
    summ = O.solve_window(oc, f, O.default_opts(True, FW.ITERS))
    q["final_cost"], q["final_state"] = summ.final_cost, f.clone_state()
    f.set_state(inp.f40_state)
    return q


def moved(a, b):
    """{quantity: movement from b to a, in units of the GPU test's bound on it} (the bounds: tests/test_gpu_parity.py's test_preintegrate,
    test_eval_imu_leg_and_imu, test_eval_proj, _check_linearization and test_solve_parity)."""
    m = {}
    ra, rb = a["record"], b["record"]
    m["record state"] = float((np.abs(ra[:, :33] - rb[:, :33]) / (1e-14 + 1e-12 * np.abs(rb[:, :33]))).max())
    m["record jacobian"] = max(_rel(x[33:33 + 961], y[33:33 + 961]) for x, y in zip(ra, rb)) / 1e-11
    m["record covariance"] = max(_rel(x[33 + 961:], y[33 + 961:]) for x, y in zip(ra, rb)) / 1e-10
    sig = [np.abs(y[33 + 961:]) > 1e-6 * np.abs(y[33 + 961:]).max() for y in rb]       # (test_preintegrate's entry-wise check)
    m["record covariance entries"] = max(float(np.abs(x[33 + 961:][k] / y[33 + 961:][k] - 1).max()) for x, y, k in zip(ra, rb, sig)) / 1e-9
    m["imu residual"] = float((np.abs(a["imu_r"] - b["imu_r"]) / np.maximum(np.abs(b["imu_r"]), 1e-12 * np.abs(b["imu_r"]).max())).max()) / 1e-11
    m["imu jacobian"] = float((np.linalg.norm(a["imu_J"] - b["imu_J"], axis=1) / np.linalg.norm(b["imu_J"], axis=1)).max()) / 1e-13
    m["proj residual"] = max(float((np.abs(x[0] - y[0]) / (1e-11 + 1e-12 * np.abs(y[0]))).max()) for x, y in zip(a["proj"], b["proj"]))
    m["proj jacobian"] = max(float((np.abs(jx - jy) / (1e-11 * max(1.0, np.abs(jy).max()) + 1e-11 * np.abs(jy))).max())
                             for x, y in zip(a["proj"], b["proj"]) for jx, jy in zip(x[1], y[1]))
    m["window cost"] = abs(a["cost0"] - b["cost0"]) / (1e-10 * abs(b["cost0"]))
    m["visual cost"] = abs(a["visual_cost"] - b["visual_cost"]) / (1e-12 * max(1.0, abs(b["visual_cost"])))   # (tests/test_residuals_gpu.py)
    m["window gradient"] = float(np.abs(a["grad"] - b["grad"]).max() / (1e-9 * np.abs(b["grad"]).max()))
    m["gauss-newton step"] = float(np.abs(a["step"] - b["step"]).max() / (1e-7 * np.abs(b["step"]).max()))
    m["solved cost"] = abs(a["final_cost"] - b["final_cost"]) / (1e-8 * abs(b["final_cost"]))
    m["solved states"] = max(float(np.abs(x - y).max() / max(1.0, np.abs(y).max())) for x, y in zip(a["final_state"], b["final_state"])) / 1e-8
    return m


@pytest.fixture(scope="module")
def alt(cfg):
    return A.alt_config(cfg)


@pytest.fixture(scope="module")
def table(cfg, alt):
    """{field: {quantity: movement / bound}}: the field reverted against the alternative configuration."""
    out = {}
    for ctype in (0, 2):
        inp = _Inputs(alt, ctype)
        base = quantities(alt, inp)
        for f in A.FIELDS:
            if (f in TYPE2_ONLY) != (ctype == 2):
                continue
            out[f] = moved(quantities(A.revert(alt, cfg, f), inp), base)
    for f in A.FIELDS:
        seen = {q: out[f][q] for q in DEVICE_SEES[f]}
        best = max(seen, key=seen.get) if seen else "-"
        print("SENSITIVITY %-28s device sees best: %-26s %9.2e   " % (f, best, seen.get(best, 0.0)) + "  ".join("%s %.1e" % kv for kv in sorted(out[f].items())))
    return out


def test_the_rotation_is_proper_and_skew(alt):
    R = np.array(list(alt.R_br)).reshape(3, 3)
    assert np.abs(R @ R.T - np.eye(3)).max() <= 1e-15
    assert abs(np.linalg.det(R) - 1.0) <= 1e-15
    off = np.abs(R - R.T)[np.triu_indices(3, 1)]
    assert (off > 0.1).all(), off                      # a transposed read moves three entries by well over 0.1 each
    axis = np.array(A.RBR_ROTVEC) / np.linalg.norm(A.RBR_ROTVEC)
    assert np.abs(axis).max() < 0.9 and np.abs(axis).min() > 0.25   # no coordinate axis, none left out
    p = np.array(list(alt.p_br))
    assert (np.abs(p) >= 0.01).all() and (np.abs(p) <= 0.05).all() and len(set(np.abs(p).round(6))) == 3


def test_every_field_differs_from_its_default_and_its_neighbours(cfg, alt):
    for f in A.FIELDS:
        a, d = getattr(alt, f), getattr(cfg, f)
        if hasattr(a, "__len__"):
            assert all(x != y for x, y in zip(a, d)), f
        else:
            assert a != d, f
    fac = list(A.NOISE_FACTORS.values())
    assert len(set(fac)) == len(fac) and min(fac) >= 0.5 and max(fac) <= 2.0
    vals = [getattr(alt, f) for f in A.NOISE_FACTORS]
    assert len(set(vals)) == len(vals)                 # no swap of two noise fields is invisible
    shifts = [alt.rho_fix[i] - cfg.rho_fix[i] for i in range(16)]
    assert len(set(np.round(shifts, 9))) == 16 and all(2e-4 < abs(s) < 3e-3 for s in shifts)
    assert alt.contact_sensor_type == cfg.contact_sensor_type


def test_the_leg_inverse_kinematics_still_succeeds(alt):
    """synth.cpp's leg_ik at the shifted rho_fix: the window generates, and the oracle's forward kinematics of the generated joint
    angles give foot positions inside the leg's reach (a failed IK leaves NaN angles)."""
    w = synth.make_window(alt, n_landmarks=10, seed=3)
    assert np.isfinite(w.samples).all()
    for j in range(4):
        rf = np.array([alt.rho_fix[4 * j + k] for k in range(4)])
        for s in w.samples[::97]:
            f = O.kin(s[7 + 3 * j:10 + 3 * j], 0.21, rf)["f"]
            assert np.isfinite(f).all() and 0.1 < np.linalg.norm(f - np.array([rf[0], rf[1], 0.0])) < 0.45


def test_every_field_has_its_device_visible_quantities():
    assert set(DEVICE_SEES) == set(A.FIELDS)
    assert [f for f in A.FIELDS if not DEVICE_SEES[f]] == list(JOINT_NOISE)


@pytest.mark.parametrize("field", [f for f in A.FIELDS if f not in JOINT_NOISE])
def test_each_field_moves_what_the_device_computes_from_it(table, field):
    """The best of the quantities the GPU suite computes from the device's own read of the field (DEVICE_SEES), not of all quantities."""
    seen = {q: table[field][q] for q in DEVICE_SEES[field]}
    best = max(seen, key=seen.get)
    assert seen[best] >= NEED, (field, seen)


def _cov_moved(a, b):
    """two sets of records: movement of the covariance in units of test_preintegrate's two bounds (1e-10 of the largest entry; 1e-9 per
    significant entry)"""
    rel = max(_rel(x[33 + 961:], y[33 + 961:]) for x, y in zip(a, b)) / 1e-10
    sig = [np.abs(y[33 + 961:]) > 1e-6 * np.abs(y[33 + 961:]).max() for y in b]
    return rel, max(float(np.abs(x[33 + 961:][k] / y[33 + 961:][k] - 1).max()) for x, y, k in zip(a, b, sig)) / 1e-9


@pytest.mark.parametrize("ctype", [0, 2])
def test_joint_noise_case_sees_phi_n_and_dphi_n(cfg, alt, table, ctype):
    """At alt_config, phi_n and dphi_n (1e-5 rad, rad/s, times 0.7 and 1.35) move nothing the device computes from them by 1000 bounds:
    the largest is a covariance entry's 3.4 and 2.9, the foot-velocity noise being seven orders above them. That is a property of the
    reference's values, not of the factors: so a preintegration-only case raises the two by 1e3 and 3e3 (alt_config.joint_noise_config;
    tests/test_alt_config_gpu.py::test_preintegrate_joint_noise runs it on the device). There each of them, put back, and the two
    swapped move the significant covariance entries by more than 1000 of their 1e-9. Measured (types 0, 2): phi_n 6.6e6, 4.2e8;
    dphi_n 3.1e7, 6.3e8; swapped 4.9e7, 3.5e9. State and jacobian of the records do not read them."""
    import copy
    for f in JOINT_NOISE:
        assert max(table[f][q] for q in _RECORD + _COV + _SOLVED) < NEED   # (why the case exists; if this fails the case is not needed)
    jn = A.joint_noise_config(cfg)
    assert jn.phi_n != jn.dphi_n and jn.phi_n > 999 * cfg.phi_n and jn.dphi_n > 999 * cfg.dphi_n
    w = synth.make_window(alt, n_landmarks=40, seed=7)
    smp = force_samples(w.samples, 3) if ctype == 2 else w.samples

    def records(c):
        oc = O.config_from(A.with_type(c, ctype))
        return np.array([O.preintegrate_imu_leg(oc, smp[w.sample_offsets[k]:w.sample_offsets[k + 1]], w.lin[k]) for k in range(10)])
    base = records(jn)
    swapped = copy.copy(jn)
    swapped.phi_n, swapped.dphi_n = jn.dphi_n, jn.phi_n
    for name, c in (("phi_n", A.revert(jn, alt, "phi_n")), ("dphi_n", A.revert(jn, alt, "dphi_n")), ("swapped", swapped)):
        r = records(c)
        rel, ent = _cov_moved(r, base)
        print("SENSITIVITY joint noise, type %d, %-8s covariance %9.2e, significant entries %9.2e" % (ctype, name, rel, ent))
        assert ent >= NEED, (name, ent)
        np.testing.assert_array_equal(r[:, :33 + 961], base[:, :33 + 961])


def test_the_groups_of_fields_reach_the_quantities_the_issue_names(table):
    """R_br, p_br and rho_fix move the record itself (state, jacobian); the noise fields its covariance; g_norm the IMU factor;
    focal_length the projection factors; huber_delta the window's cost; and each family moves the four-iteration solve."""
    for f in ("R_br", "p_br", "rho_fix"):
        assert table[f]["record state"] >= NEED and table[f]["record jacobian"] >= NEED, f
    assert table["g_norm"]["imu residual"] >= NEED
    assert table["focal_length"]["proj residual"] >= NEED and table["focal_length"]["proj jacobian"] >= NEED
    assert table["huber_delta"]["visual cost"] >= NEED and table["huber_delta"]["gauss-newton step"] >= NEED
    for f in ("R_br", "p_br", "g_norm", "focal_length", "huber_delta", "acc_w", "gyr_w", "rho_c_n", "rho_nc_n"):
        assert max(table[f]["solved cost"], table[f]["solved states"]) >= NEED, f


def _visual_norms(ocfg, w):
    ob = resid_ref.window_residuals(ocfg, w)["obs_residuals"]
    s2 = np.concatenate([(ob[:, 0:2] ** 2).sum(1), (ob[:, 2:4] ** 2).sum(1)])
    return np.sqrt(s2[~np.isnan(s2)])


def test_huber_shares(cfg, alt):
    """On the field windows' initial states, at the alternative configuration: at least 10 % of the visual factors on each side of the
    new threshold, at least 1 % between it and the default 1.0 (where a hard-coded 1.0 gives another answer). Measured over the seven
    windows: 87 % above 0.6, 13 % below, 15 % between 0.6 and 1.0; per window 81 .. 95 %, 5 .. 20 % and 8 .. 18 %."""
    oa = O.config_from(alt)
    norms = [_visual_norms(oa, w) for w in FW.field_set(alt, oa).values()]
    n = np.concatenate(norms)
    d_new, d_old = alt.huber_delta, cfg.huber_delta
    above, below, between = (n > d_new).mean(), (n <= d_new).mean(), ((n > d_new) & (n <= d_old)).mean()
    print("HUBER SHARES above %.3f below %.3f between %.3f of %d factors" % (above, below, between, len(n)))
    assert above >= 0.10 and below >= 0.10 and between >= 0.01
    for x in norms:                                     # and no window without factors on each side and in between
        assert (x > d_new).any() and (x <= d_new).any() and ((x > d_new) & (x <= d_old)).mean() >= 0.01


def test_four_iterations_still_arrive(cfg, alt):
    """The leg samples are generated for R_br = I, p_br = 0, so the leg factors start with residuals of their own at the alternative
    configuration; the field windows' four iterations from the 0.3 start still come down from 1e10 to the visual terms' level (f40: 2.5e10,
    2.2e10, 1.5e10, 3.1e9, 251). f60_partial8 (leg biases constant, no prior) stays at its IMU terms' 1e10 under BOTH configurations."""
    oa, od = O.config_from(alt), O.config_from(cfg)
    for name, w in FW.field_set(alt, oa).items():
        s = O.solve_window(oa, w, O.default_opts(True, FW.ITERS))
        assert s.num_successful == FW.ITERS, name
        if name == "f60_partial8":
            sd = O.solve_window(od, FW.field_window(cfg, od, name), O.default_opts(True, FW.ITERS))
            assert s.final_cost > 1e9 and sd.final_cost > 1e9
        else:
            assert s.final_cost < 1e-6 * s.initial_cost and s.final_cost < 5.0 * w.n_obs, (name, s.final_cost)
