"""Test helper (no test in it) for the landmark mask of a resident batch (vilo_batch_mask_landmarks): the host window with landmarks
deleted, which is what a masked batch has to behave as; the masks the tests use; numpy counts for the call's records."""
import copy

import numpy as np

KINDS = ("one", "start_frame", "frame0", "all", "outliers", "empty")


def delete_landmarks(w, mask):
    """A new window over w's inputs with the landmarks mask != 0 deleted: lm_obs_offset, obs, obs_is_stereo, lm_start_frame and the
    inverse depths (state and truth) rebuilt; the camera-side state arrays are copies of w's, every other input is shared (as twin())."""
    mask = np.asarray(mask) != 0
    assert mask.shape == (w.L,)
    keep = np.flatnonzero(~mask)
    r = copy.copy(w)
    r.pose, r.speed_bias, r.leg_bias = w.pose.copy(), w.speed_bias.copy(), w.leg_bias.copy()
    r.ex_pose, r.td = w.ex_pose.copy(), w.td.copy()
    K = np.diff(w.lm_obs_offset)[keep]
    idx = (np.concatenate([np.arange(w.lm_obs_offset[l], w.lm_obs_offset[l + 1]) for l in keep]) if len(keep) else np.zeros(0, np.int64)).astype(np.int64)
    r.obs = np.ascontiguousarray(w.obs[idx]).reshape(len(idx), 11)
    r.obs_is_stereo = np.ascontiguousarray(w.obs_is_stereo[idx])
    r.lm_obs_offset = np.concatenate([[0], np.cumsum(K)]).astype(np.int32)
    r.lm_start_frame = np.ascontiguousarray(w.lm_start_frame[keep])
    r.inv_depth = np.ascontiguousarray(w.inv_depth[keep])
    r.truth_inv_depth = np.ascontiguousarray(w.truth_inv_depth[keep])
    r.L, r.n_obs = int(len(keep)), int(len(idx))
    return r


def make_mask(w, kind, outliers=None):
    """uint8 [w.L]. one: landmark 5; start_frame: every landmark of the most populated start frame other than 0 (a whole chunk);
    frame0: every landmark that starts at frame 0; all; outliers: the given selection; empty."""
    m = np.zeros(w.L, np.uint8)
    start = np.asarray(w.lm_start_frame)
    if kind == "one":
        m[5] = 1
    elif kind == "start_frame":
        counts = np.bincount(start, minlength=w.F)
        counts[0] = 0
        m[start == int(np.argmax(counts))] = 1
    elif kind == "frame0":
        m[start == 0] = 1
    elif kind == "all":
        m[:] = 1
    elif kind == "outliers":
        m[:] = np.asarray(outliers) != 0
    else:
        assert kind == "empty"
    return m


def record_counts(w, mask, before=None):
    """(status, n_landmarks, n_masked, n_newly_masked, n_obs_left) of vilo_window_mask_record for window w under `mask`, `before` the
    mask that was in force (None: none)."""
    mask = np.asarray(mask) != 0
    before = np.zeros(w.L, bool) if before is None else np.asarray(before) != 0
    K = np.diff(w.lm_obs_offset)
    n_masked = int(mask.sum())
    return (0 if w.L - n_masked > 0 else 1, w.L, n_masked, int((mask & ~before).sum()), int(K[~mask].sum()))
