"""Test helper (no test in it): one window for every frame count check_window accepts, 2 to 11 (cerberus_amd/csrc/batch_pack.hpp).
The frame count decides where the 6F-wide pose system ends inside its 16-column tiles (F = 8: on an edge; 3, 6, 11: just past one; 2, 5,
7, 9, 10: in the middle), the parity of the loops that walk the frames two at a time, which blocks every assembly pads with identity or
zero, where a window joins the four-windows-per-wave chain factorisation (chain_fact_groups runs to the wave's largest frame count), and
how many IMU intervals (F - 1) a window hands the IMU forms. The rest of the suite solves 4, 8 and 11 frames.
tests/test_frame_windows.py holds, on a CPU and with the oracle alone, that every window here meets the conditions the GPU comparison
relies on; tests/test_kernel_paths.py solves the set in every kernel form, tests/test_frame_counts_gpu.py runs every query call on it.

Every window is the generator's (cerberus_amd/host/synth.cpp), filled by the oracle's preintegration, its start perturbations scaled by
field_windows.START (the leg biases': SIG_RHO), cut to its first F frames by _paths_worker._truncate (no prior, leg biases constant). The generator hands out start
frames i % n_start_frames; with n_start_frames = F - 1 every landmark survives the cut and every start frame from 0 to F - 2 has one (at
F = 2 every landmark starts at frame 0). The default mask is the one the reference's Estimator::optimization() gives a window with
frame_count < WINDOW_SIZE: leg biases, extrinsics and td constant, no prior. The reference's shipped start-up solves only the full window
(it runs PnP and triangulation at every frame count); a partial solve is what the ABI offers any other caller."""
import numpy as np

import field_windows as FW

ITERS = FW.ITERS   # (tests/_paths_worker.py: the iteration count of every solve of these windows)
DEFAULT = dict(ex_const=1)   # (with _truncate's leg_bias_const = 1 and the generator's td_const = 1)

# Leg set (use_leg = 1), one batch kind.
#   name: (frames, landmarks, generator seed, shaper seed or None, flags)
# Landmark counts are odd or no multiple of the start-frame count, so the start-frame groups differ in size.
LEG = {
    "g2": (2, 17, 102, None, DEFAULT),
    "g3": (3, 23, 103, None, DEFAULT),
    "g4": (4, 29, 104, None, DEFAULT),
    "g5": (5, 33, 105, None, DEFAULT),
    "g6": (6, 37, 106, None, DEFAULT),
    "g7": (7, 41, 107, None, DEFAULT),
    "g8": (8, 47, 108, None, DEFAULT),
    "g9": (9, 53, 109, None, DEFAULT),
    "g10": (10, 59, 110, None, DEFAULT),
    "g11": (11, 60, 111, None, DEFAULT),                # the full window without a prior, under the partial windows' mask
    "g3_field": (3, 40, 123, 123, DEFAULT),             # ragged, part-mono, with outliers (field_windows.field_shape before the cut)
    "g6_field": (6, 50, 126, 126, DEFAULT),
    "g10_field": (10, 60, 130, 130, DEFAULT),
    "g5_exfree": (5, 35, 145, None, dict(ex_const=0)),  # the mask of the partial4 / partial8 specials of tests/_paths_worker.py
    "g7_exfree": (7, 43, 147, None, dict(ex_const=0)),
    "g10_exfree": (10, 57, 150, None, dict(ex_const=0)),
}
# IMU-only set (use_leg = 0), batches of its own (a batch holds one IMU factor kind).
#   name: (frames, landmarks, generator seed)
VINS = {
    "v2": (2, 19, 202),
    "v3": (3, 25, 203),
    "v5": (5, 31, 205),
    "v6": (6, 39, 206),
    "v7": (7, 44, 207),
    "v9": (9, 51, 209),
    "v10": (10, 58, 210),
}

# The leg biases start at their true value (sig_rho = 0), the one start scale that is not field_windows.START: a partial window keeps them
# constant, so a perturbed start stays in the cost as a constant 4e8 .. 1.4e10 of leg-factor residuals, and the steps that matter move the
# cost below its rounding (REJECTED). At the truth the cost comes down from 1e6 .. 1e7 and every step's decrease is 1e-6 of it or more.
SIG_RHO = 0.0
MIN_DECREASE = 1e-8   # of the cost, per step: 1e5 times the rounding of a sum of a few thousand terms, so no GPU decision turns on rounding

# Recipes tried and not kept: (names, recipe, the condition of tests/test_frame_windows.py it missed, the measured figure). No seed or
# landmark count had to go: every first seed meets every condition (step-quality ratios 0.998 .. 1.221).
REJECTED = [
    (tuple(LEG), "leg biases started sig_rho * field_windows.START off the truth, as every other block is",
     "each step's decrease at least MIN_DECREASE of the cost",
     "fourth step's relative decrease 2.0e-14 (g10) .. 3.7e-12 (g2), third 4.0e-13 .. 4.2e-11, of a cost of 4.5e8 .. 1.4e10 that the "
     "constant leg biases hold up; all steps successful, ratios 0.991 .. 1.221"),
]

# A batch's first 32 positions, repeated from there on. Every aligned group of four (the four windows chain_fact_groups puts in one wave,
# and a workgroup's neighbours in the other forms) holds four different frame counts; (2, 11, 3, 10) is positions 0 .. 3 and
# (10, 2, 9, 3) positions 16 .. 19: a window of 2 frames joins a wave that runs 11 or 10 frames, first and second in it.
LEG_ORDER = ["g2", "g11", "g3", "g10",
             "g5", "g8", "g6_field", "g4",
             "g7", "g9", "g10_field", "g3_field",
             "g5_exfree", "g7_exfree", "g10_exfree", "g6",
             "g10_field", "g2", "g9", "g3_field",
             "g11", "g4", "g7_exfree", "g5",
             "g6_field", "g8", "g10", "g3",
             "g7", "g5_exfree", "g6", "g10_exfree"]
# Seven windows in turn: any four consecutive ones differ, and 2 frames sit beside 10 and 9.
VINS_ORDER = ["v2", "v10", "v3", "v9", "v5", "v7", "v6"]


def _cut(cfg, ocfg, F, L, gseed, sseed):
    w = FW._filled(cfg, ocfg, L, gseed, prior=False, n_start_frames=max(F - 1, 1), sig_rho=SIG_RHO)
    if sseed is not None:
        FW.field_shape(w, sseed, focal=cfg.focal_length)
    return FW._truncate(w, F)   # (no prior, leg biases constant)


def leg_window(cfg, ocfg, name):
    F, L, gseed, sseed, flags = LEG[name]
    w = _cut(cfg, ocfg, F, L, gseed, sseed)
    for k, v in flags.items():
        setattr(w, k, v)
    return w


def vins_window(cfg, ocfg, name):
    F, L, gseed = VINS[name]
    w = _cut(cfg, ocfg, F, L, gseed, None)
    w.use_leg, w.leg_bias_const, w.ex_const = 0, 1, 1
    return w


def make(cfg, ocfg, name):
    return leg_window(cfg, ocfg, name) if name in LEG else vins_window(cfg, ocfg, name)


def leg_set(cfg, ocfg, names=None):
    """{name: window} of the leg set, oracle-filled, fresh objects (the oracle solves its own copies)."""
    return {n: leg_window(cfg, ocfg, n) for n in (names or LEG)}


def vins_set(cfg, ocfg, names=None):
    return {n: vins_window(cfg, ocfg, n) for n in (names or VINS)}


def order_of(S):
    return LEG_ORDER if "g2" in S else VINS_ORDER


def batch_of(S, W):
    """W windows of one set placed in turn along the set's order (field_windows.batch_of: the first occurrence the window itself, every
    later one a twin). Returns (windows, names by position). The 16 leg windows sit at two positions each in a batch of 32 (three each would
    take 48) and at three or more from 48 positions on; the 7 IMU-only windows at four or more."""
    return FW.batch_of(S, W, names=order_of(S))
