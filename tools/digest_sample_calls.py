#!/usr/bin/env python
"""One sha256 per call of the four sample-stream calls (dead_reckon, dead_reckon_covariance, leg_dead_reckon, leg_dead_reckon_covariance)
over every output of the call: state, legs, cov, every trajectory, step_offsets, n_steps and status; for dead_reckon with write also the
batch's state as downloaded afterwards. Two libraries that print the same lines compute the same bits (VILO_GPU_LIB selects the library
api.py loads; tools/build_variant.py builds one beside the tree's own).

The batch is 9 synthetic config-2 windows, NOT solved (the states are as synth makes them: no solve's rounding enters), with ranges of
0, 1, 2, 3, 7, 30, 30, 31 and 64 samples: quads, 16-lane groups and 32-lane groups of one wave hold ranges of different length, and nine
windows are more than one wave of either covariance kernel. Window 5's range has a NaN sample (NUMERIC) and window 4 has 5 frames, so the
explicit from_frame 7 is beyond them (NO_FRAME): both failure tails are digested. Every call runs from the last frame and from frame 7,
with and without cov_in, with and without trajectories, dead_reckon with write 0 and 1, under contact models 0, 1 and 2, each at the
default configuration and at one in which every value these kernels read of it is another. Needs a GPU; reads nothing outside the repository.
    python tools/digest_sample_calls.py > digests.txt"""
import copy
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RANGES = (0, 1, 2, 3, 7, 30, 30, 31, 64)
NAN_WINDOW, SHORT_WINDOW, SHORT_FRAMES, EXPLICIT = 5, 4, 5, 7


def other_config(cfg):
    """every scalar the four kernels read of the configuration, moved off its default"""
    c = copy.copy(cfg)
    c.g_norm = 9.79
    for name, k in (("acc_n", 1.5), ("acc_n_z", 3.0), ("acc_w", 2.0), ("gyr_n", 0.7), ("gyr_w", 0.5), ("phi_n", 2.0), ("dphi_n", 3.0),
                    ("rho_c_n", 1.7), ("rho_nc_n", 0.6), ("v_n_max", 0.8), ("v_n_min_xy", 1.3), ("v_n_min_z", 0.6), ("v_n_min", 1.2),
                    ("v_n_force_thres_ratio", 0.9), ("v_n_term1_steep", 1.1), ("v_n_term2_var_rescale", 1.4), ("v_n_term3_distance_rescale", 0.75)):
        setattr(c, name, k * getattr(c, name))
    for i in range(3):
        c.p_br[i] = c.p_br[i] + 0.01 * (i + 1)
    for i in range(16):
        c.rho_fix[i] = c.rho_fix[i] * (1.0 + 0.01 * (i % 4))
    return c


def short_window(base, F):
    """the first F frames of the window: its landmarks with two observations left, no prior"""
    w = base.twin()
    w.prior = w.prior.copy()
    keep = [l for l in range(w.L) if w.lm_start_frame[l] + 2 <= F]
    obs, st, off, sf = [], [], [0], []
    for l in keep:
        o0 = w.lm_obs_offset[l]
        K = min(w.lm_obs_offset[l + 1] - o0, F - w.lm_start_frame[l])
        obs.append(w.obs[o0:o0 + K]); st.append(w.obs_is_stereo[o0:o0 + K]); off.append(off[-1] + K); sf.append(w.lm_start_frame[l])
    w.L, w.n_obs, w.F = len(keep), off[-1], F
    w.lm_start_frame, w.lm_obs_offset = np.array(sf, np.int32), np.array(off, np.int32)
    w.obs, w.obs_is_stereo = np.ascontiguousarray(np.concatenate(obs)), np.ascontiguousarray(np.concatenate(st))
    w.inv_depth = np.ascontiguousarray(w.inv_depth[keep])
    w.prior.struct.valid = 0
    w.leg_bias_const = 1
    return w


def the_samples(base, model):
    rows = np.array(base.samples, dtype=np.float64, copy=True).reshape(-1, 35)
    if model == 2:   # foot forces for contact_sensor_type 2: 15 N + 140 N on a standing foot + noise
        rows[:, 31:35] = 15.0 + 140.0 * rows[:, 31:35] + 4.0 * np.random.default_rng(100).normal(size=(len(rows), 4))
    parts = [rows[(7 * i) % 16:(7 * i) % 16 + n].copy() for i, n in enumerate(RANGES)]
    parts[NAN_WINDOW][12, 5] = np.nan   # gyr[1] of a sample in mid-range: every chain reads it
    offsets = np.concatenate([[0], np.cumsum(RANGES)]).astype(np.int32)
    return np.ascontiguousarray(np.concatenate(parts)), offsets


def spd(n, W, seed):
    g = np.random.default_rng(seed)
    A = g.normal(size=(W, n, n))
    return np.ascontiguousarray(1e-4 * (A @ A.transpose(0, 2, 1) / n + np.eye(n)))


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(b"none" if a is None else np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def main():
    from cerberus_amd import api, synth
    W = len(RANGES)
    for model in (0, 1, 2):
        for cfg_name in ("default", "other"):
            cfg = copy.copy(synth.default_config())
            if cfg_name == "other":
                cfg = other_config(cfg)
            cfg.contact_sensor_type = model
            ctx = api.Context(cfg, 0)
            base = synth.make_window(cfg, params=synth.default_params(config=2, seed=20260925))
            ctx.preintegrate_window(base)
            samples, offsets = the_samples(base, model)
            b = api.Batch(ctx, [short_window(base, SHORT_FRAMES) if i == SHORT_WINDOW else base.twin() for i in range(W)])
            c15, c19 = spd(15, W, 15), spd(19, W, 19)
            tag = "model %d config %s" % (model, cfg_name)
            for f in (-1, EXPLICIT):
                for traj in (False, True):
                    r = b.dead_reckon(samples, offsets, f, False, trajectory=traj)
                    print("%s dead_reckon from %d traj %d: %s" % (tag, f, traj, digest(*r)))
                    r = b.leg_dead_reckon(samples, offsets, f, trajectory=traj)
                    print("%s leg_dead_reckon from %d traj %d: %s" % (tag, f, traj, digest(*r)))
                    for cin in (False, True):
                        r = b.dead_reckon_covariance(samples, offsets, c15 if cin else None, f, pose_trajectory=traj)
                        print("%s dead_reckon_covariance from %d traj %d cov_in %d: %s" % (tag, f, traj, cin, digest(*r)))
                        r = b.leg_dead_reckon_covariance(samples, offsets, c19 if cin else None, f, pose_trajectory=traj, leg_trajectory=traj)
                        print("%s leg_dead_reckon_covariance from %d traj %d cov_in %d: %s" % (tag, f, traj, cin, digest(*r)))
            # last: it changes the batch's state
            r = b.dead_reckon(samples, offsets, EXPLICIT, True, trajectory=True)
            b.download()
            print("%s dead_reckon from %d write 1, and the state downloaded: %s" % (tag, EXPLICIT, digest(*r, *[a for w in b.windows for a in w.state_arrays()])), flush=True)
            b.close()
            ctx.close()


if __name__ == "__main__":
    main()
