"""Test helper (no test in it): ONE configuration away from the shipped defaults, at which every value a kernel reads from vilo_config
differs from its default and from its neighbours. At the default point R_br is the identity, p_br is zero and huber_delta is 1.0: a
transposed read, a product on the wrong side, a dropped summand, `a` for `a * a` or a literal left over give the same bits there.
tests/test_alt_config.py holds, on a CPU and with the oracle alone, that each changed field moves what it feeds by 1000 times the parity
bound the GPU tests apply to it, and the Huber shares; tests/test_alt_config_gpu.py runs every config-reading call at this point."""
import copy

import numpy as np

# Rodrigues vector of R_br: 0.23 rad about (0.48, -0.30, 0.82): no coordinate axis; R and R^T differ by 0.37, 0.22 and 0.13 off the diagonal
RBR_ROTVEC = (0.11, -0.07, 0.19)
P_BR = (0.031, -0.017, 0.023)            # metres: three distinct, non-zero components
G_NORM, FOCAL, HUBER = 9.79, 380.0, 0.6
# every noise field times a factor of its own in [0.5, 2]: no two equal, and no two fields coincide afterwards
# (phi_n = dphi_n = 1e-5 by default -> 0.7e-5 and 1.35e-5; v_n_min_z = v_n_min = 0.005 -> 0.00375 and 0.009)
NOISE_FACTORS = {
    "acc_n": 1.30, "acc_n_z": 0.60, "acc_w": 1.70, "gyr_n": 0.80, "gyr_w": 1.45,
    "phi_n": 0.70, "dphi_n": 1.35, "rho_c_n": 1.90, "rho_nc_n": 0.55,
    "v_n_min_xy": 1.60, "v_n_min_z": 0.75, "v_n_min": 1.80, "v_n_max": 0.50,
    "v_n_force_thres_ratio": 0.90, "v_n_term1_steep": 1.20, "v_n_term2_var_rescale": 1.55, "v_n_term3_distance_rescale": 0.65,
}
# metres, one amount per entry of rho_fix (leg by leg: hip offset x, y, thigh offset, calf length): 0.4 .. 2.3 mm, all different
RHO_FIX_SHIFT = (0.0011, -0.0007, 0.0013, 0.0019, -0.0009, 0.0015, -0.0005, -0.0017,
                 0.0021, 0.0004, -0.0012, 0.0008, -0.0014, -0.0023, 0.0006, -0.0010)
# the fields alt_config changes, in the groups tests/test_alt_config.py reverts one at a time
FIELDS = ("R_br", "p_br", "g_norm", "focal_length", "huber_delta", "rho_fix") + tuple(NOISE_FACTORS)


def rotation(v):
    """Rodrigues' formula."""
    v = np.asarray(v, float)
    th = np.linalg.norm(v)
    k = v / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def alt_config(cfg):
    """A copy of cfg (the default configuration) with every field of FIELDS changed; contact_sensor_type is the caller's."""
    c = copy.copy(cfg)
    R = rotation(RBR_ROTVEC)
    for i in range(9):
        c.R_br[i] = R[i // 3, i % 3]          # row-major
    for i in range(3):
        c.p_br[i] = P_BR[i]
    c.g_norm, c.focal_length, c.huber_delta = G_NORM, FOCAL, HUBER
    for name, f in NOISE_FACTORS.items():
        setattr(c, name, getattr(cfg, name) * f)
    for i in range(16):
        c.rho_fix[i] = cfg.rho_fix[i] + RHO_FIX_SHIFT[i]
    return c


# A preintegration-only case for phi_n and dphi_n. Within [0.5, 2] of their defaults (1e-5) the joint-angle noise is seven orders below the
# foot-velocity noise and moves no covariance entry by more than 4e-9 relative: no bound sees it. Here the two are 1e3 and 3e3 times
# their defaults (distinct, so that a swap shows); everything else is alt_config's.
JOINT_NOISE_FACTORS = {"phi_n": 1.0e3, "dphi_n": 3.0e3}


def joint_noise_config(cfg):
    """alt_config(cfg) with phi_n and dphi_n raised to where the record's covariance carries them."""
    c = alt_config(cfg)
    for name, f in JOINT_NOISE_FACTORS.items():
        setattr(c, name, getattr(cfg, name) * f)
    return c


def with_type(cfg, contact_sensor_type):
    c = copy.copy(cfg)
    c.contact_sensor_type = contact_sensor_type
    return c


def revert(alt, default, field):
    """alt with one field of FIELDS back at its default."""
    c = copy.copy(alt)
    v = getattr(default, field)
    if hasattr(v, "__len__"):
        for i in range(len(v)):
            getattr(c, field)[i] = v[i]
    else:
        setattr(c, field, v)
    return c
