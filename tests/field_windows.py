"""Test helper (no test in it): synthetic windows in the shape a feature tracker hands over. The generator (cerberus_amd/host/synth.cpp)
sees every landmark in every frame from its start frame to the last one, every observation stereo, 0.5 px of noise and no outlier: in every
packed wave all lanes have the same track length. field_shape cuts the tracks to lengths of their own, clears stereo flags and adds
mismatches that stay on the Huber branch; field_set is the set of such windows the GPU tests share (tests/test_field_windows.py holds, on a
CPU and with the oracle alone, that the set has the properties the GPU tests rely on)."""
import numpy as np

ITERS = 4   # (tests/_paths_worker.py: the iteration count of every solve of these windows)


def field_shape(w, seed, mono=0.25, outlier=0.05, outlier_px=8.0, min_obs=2, focal=460.0):
    """Edits the filled synthetic window w in place (new observation arrays: twins made before keep theirs); one default_rng(seed).

    Track lengths: each landmark keeps its first K observations, K uniform in [min_obs, F - start frame]; obs, obs_is_stereo,
    lm_obs_offset and n_obs are rebuilt, inv_depth and lm_start_frame stay. Mono flags: obs_is_stereo is cleared on a `mono` share of
    the observations, first observations included (a cleared first observation: no one-frame-two-camera factor). Outliers: on an
    `outlier` share of the observations the left and the right image point get normal noise of outlier_px / focal.
    By construction, not by luck: in the largest start-frame group (the lowest start frame among equals) the first landmark keeps its
    full length and the second one two observations (one packed wave, lanes of different length), and the third one (any other landmark
    where the group has two) keeps two observations, both mono: exactly one two-residual factor.
    Returns the indices (full, short, one_factor)."""
    assert min_obs >= 2   # (a landmark without a factor is outside what the reference builds: used_num >= 2, feature_manager.cpp)
    rng = np.random.default_rng(seed)
    L = w.L
    start = np.asarray(w.lm_start_frame, np.int64)
    K0 = np.diff(w.lm_obs_offset).astype(np.int64)
    assert (K0 >= min_obs).all()
    K = rng.integers(min_obs, K0 + 1)
    groups = np.bincount(start, minlength=w.F)
    members = np.flatnonzero(start == int(np.argmax(groups)))
    assert len(members) >= 2 and K0[members[0]] > 2
    full, short = int(members[0]), int(members[1])
    one = int(members[2]) if len(members) > 2 else int(np.setdiff1d(np.arange(L), members[:2])[0])
    K[full], K[short], K[one] = K0[full], 2, 2
    off = np.concatenate([[0], np.cumsum(K)]).astype(np.int32)
    idx = np.concatenate([np.arange(w.lm_obs_offset[l], w.lm_obs_offset[l] + K[l]) for l in range(L)])
    obs = np.ascontiguousarray(w.obs[idx])
    stereo = np.ascontiguousarray(w.obs_is_stereo[idx])
    n = len(idx)
    stereo[rng.random(n) < mono] = 0
    hit = rng.random(n) < outlier
    noise = rng.normal(size=(n, 4)) * (outlier_px / focal)
    obs[hit, 0:2] += noise[hit, 0:2]
    obs[hit, 3:5] += noise[hit, 2:4]
    stereo[off[one]:off[one] + 2] = 0
    w.obs, w.obs_is_stereo, w.lm_obs_offset, w.n_obs = obs, stereo, off, n
    return full, short, one


def factor_counts(w):
    """Per landmark: the number of visual factors (a left-camera one per later observation, a two-camera one per stereo observation)."""
    K = np.diff(w.lm_obs_offset)
    st = np.add.reduceat(w.obs_is_stereo.astype(np.int64), w.lm_obs_offset[:-1]) if w.L else np.zeros(0, np.int64)
    return (K - 1) + st


START = 0.3   # the generator's start perturbations (sig_p ... sig_lambda_rel) are scaled by this, see field_set
_SIG = ("sig_p", "sig_theta", "sig_v", "sig_ba", "sig_bg", "sig_rho", "sig_lambda_rel")


def _filled(cfg, ocfg, L, seed, prior=True, **kw):
    from cerberus_amd import synth
    from oracle import oracle_py as O
    prm = synth.default_params(n_landmarks=L, seed=seed, with_prior=prior)
    for k in _SIG:
        setattr(prm, k, getattr(prm, k) * START)
    for k, v in kw.items():
        setattr(prm, k, v)
    w = synth.make_window(cfg, params=prm)
    O.fill_preint(ocfg, w)
    return w


def _truncate(w, F):
    from _paths_worker import _truncate as t
    return t(w, F)


#        name: (landmarks, generator seed, shaper seed, generator parameters, shaper parameters)
RECIPES = {
    "f40": (40, 7, 7, dict(), dict()),
    "f200": (200, 8, 8, dict(), dict()),                              # several start-frame groups of more than one lane each
    "f130_noprior": (130, 9, 9, dict(prior=False), dict()),
    "f70_chunks": (70, 10, 10, dict(n_start_frames=1), dict()),       # more than 64 lanes in one group: multi-chunk and ragged
    "f40_allmono": (40, 11, 117, dict(), dict(mono=1.0)),
    "f40_td": (40, 12, 112, dict(), dict()),                          # td_const = 0: the 23-column rows
    "f60_partial8": (60, 13, 13, dict(), dict()),                     # shaped, then the first 8 frames
}
FRAMES = {"f60_partial8": 8}
REJECTED_SHAPER_SEEDS = {"f40_allmono": 11, "f40_td": 12}        # tried first, see field_set; tests/test_field_windows.py shows why
BATCH_NAMES = [n for n in RECIPES if n != "f40_td"]                   # what shares a compact-row batch


def field_window(cfg, ocfg, name, shaper_seed=None):
    L, gseed, sseed, gen, shp = RECIPES[name]
    sseed = sseed if shaper_seed is None else shaper_seed
    w = _filled(cfg, ocfg, L, gseed, **gen)
    field_shape(w, sseed, focal=cfg.focal_length, **shp)
    if name == "f40_td":
        w.td_const = 0
    if name in FRAMES:
        _truncate(w, FRAMES[name])
    return w


def field_set(cfg, ocfg, names=None):
    """{name: window}, oracle-filled, fresh objects (the oracle solves its own copies).

    The start states are the generator's with its perturbations scaled by START = 0.3. From the generator's own start the oracle needs
    five iterations to come down from the IMU terms' 1e11 (measured, f40: 1.5e11, 1.5e11, 1.3e11, 7.9e10, 1.1e10, 295), so after ITERS = 4
    over 90 % of the visual factors still sit on the Huber branch, inliers included, and the cost holds nothing visual at 1e-8. From 0.3 of it
    the four iterations arrive (1.4e10, 1.2e10, 6.9e9, 7.7e8, 269: every step a large decrease, no decision near a threshold), the outliers
    alone stay on the Huber branch (17 % of the factors) and the visual terms are nearly all of the final cost.

    Shaper seeds 117 (f40_allmono) and 112 (f40_td) are not the first tried: with 11 and 12 the oracle's solve leaves a landmark with a mean
    reprojection error of 0.034 px and 0.004 px (a one-factor landmark has two residuals and one depth to fit them). That error is a
    difference of image coordinates near 1: one ulp of a coordinate is 1e-12 of an error of 0.05 px, so no evaluation of it, the numpy one
    included, holds the 1e-12 relative bound of tests/test_residuals_gpu.py there. tests/test_field_windows.py holds 0.1 px, and shows with numpy
    alone that two ways of writing the same sum differ by more than 1e-12 on those two landmarks and by less from 0.1 px on."""
    return {n: field_window(cfg, ocfg, n) for n in (names or RECIPES)}


def ragged_groups(w):
    """The start frames whose landmarks (the lanes of one packed wave, or of its chunks) differ in track length."""
    K = np.diff(w.lm_obs_offset)
    return [int(f) for f in np.unique(w.lm_start_frame) if len(set(K[w.lm_start_frame == f].tolist())) > 1]


MARG_NAMES = ["f40", "f200", "f130_noprior"]
MARG_NOTE = """The windows tests/test_gpu_parity.py marginalises. MARGIN_OLD drops frame 0 and its landmarks; frame 0 is the largest start-frame group,
so the full-length track, the one of two observations and the one-factor landmark are all among the dropped. With the oracle alone
(O.marginalize's A, m; O.window_normal_eq's H), each window beside its twin, the generator's window before field_shape:

                   cond(H), equilibrated      cond(Amm)                 numpy Schur complement    oracle's prior against the 60-digit
                   twin      field            twin      field           against the 60-digit one  one, blocks' diagonals (H, b)
    f40            8.7e11    8.3e11           2.0e11    3.9e15 (19000x) 1.4e-7    2.9e-7          2.1e-6, 2.8e-7
    f200           8.1e11    8.0e11           6.6e11    1.9e13 (28x)    3.8e-7    6.2e-6          3.1e-6, 2.6e-7
    f130_noprior   (singular: the gauge)      1.9e11    1.9e13 (100x)   1.1e-7    3.0e-6          7.3e-7, 1.8e-5 (twin: 0.25, 6.5e-5)

The whole window's H is no worse than its twin's; the dropped block Amm is, by its smallest eigenvalue (3.7e3 -> 0.20, 1.1e3 -> 41,
3.9e3 -> 39: the information two mono observations give on an inverse depth), and equilibrated it is not (8.5 for all six). It is the same
for every shaper seed and min_obs 2 .. 4, and 26 .. 27000x over eight generator seeds, since field_shape forces the two short tracks into
that group: no seed, min_obs or outlier size changes it. What it costs is the FP64 pinv of the unequilibrated Amm in test_marginalize's
numpy Schur complement: on f200 and f130_noprior that reference is itself 6e-6 and 3e-6 from the 60-digit one (2e-6 .. 6e-5 over those
seeds, none under 9e-7 on f200), more than the 1e-6 it is to hold, while the oracle stays 3e-8 and 9e-8 from the 60-digit one in the same
units. So MARGIN_OLD of f200 and f130_noprior leaves the numpy Schur complement out and keeps the others.
Without a prior the 60-digit comparison per block diagonal is left out as well. The prior is then by definition not the Schur complement:
A' is semi-definite, the reference drops every eigenvalue up to eps = 1e-8, and the 60-digit A' of f130_noprior has 13 eigenvalues below
that (9 for the twin) whose FP64 images are noise of 2e-9 (eps of the largest, 1e7) around the cut. One of the directions in question
carries a quarter of a diagonal entry of 0.5: where it is dropped, that entry is 0.25 of its diagonal off, where it is kept 7e-7. The
oracle drops it on the twin and on 4 of 20 shaper and generator seeds of the field window (not on seed 9); what holds there is the
comparison with the oracle at 1e-6 of the largest entry (tests/test_gpu_parity.py::test_marginalize_and_next_solve_without_leg_factors
does the same for its window without a prior). f40 in both modes and f200 in MARGIN_SECOND_NEW meet all three references;
MARGIN_SECOND_NEW of f130_noprior has no prior to carry over and leaves none."""

def batch_of(S, W, names=BATCH_NAMES, extra=None):
    """W windows: the named windows of S in turn, the first occurrence the window itself, every later one a twin; extra: {position: window}.
    Returns (windows, names by position)."""
    ws, at, seen = [], [], set()
    for p in range(W):
        if extra and p in extra:
            ws.append(extra[p][1]); at.append(extra[p][0]); continue
        nm = names[p % len(names)]
        ws.append(S[nm].twin() if nm in seen else S[nm]); at.append(nm); seen.add(nm)
    return ws, at
