// Host windows -> the tables of a batch, in two steps so that the caller can bring page-locked staging in between:
//   plan_batch  serial and light: every check of the (untrusted: include/vilo_window_io.h) tables, the landmark order, chunk and wave
//               tables, every offset and total;
//   fill_batch  one host thread per slice of windows: the heavy copies, into memory of the caller's.
// Plain C++17, no HIP: vilo_batch_create_refs (vilo_batch.hip) uploads what this leaves; tests/host_check/batch_pack_check.cpp runs it on
// a CPU under sanitizers, tests/test_batch_pack.py holds its output against a restatement of the layout. A window's resident references
// (device pools) are the caller's to resolve: the packer sees a PackWindow.
#pragma once
#include <algorithm>
#include <cstring>
#include <vector>

#include "batch_layout.hpp"
#include "launch_plan.hpp"
#include "worker_pool.hpp"

namespace vilo {

struct PackStatus { int code = VILO_OK; const char *msg = nullptr; };   // vilo_status; text for vilo_last_error (null: the code says it all — a missing pointer)

// What the caller resolved of window w's vilo_resident_refs (all defaults: a plain host window without a prior)
struct PackWindow {
  const vilo_prior *prior = nullptr;   // vilo_win_prior: the desc's, or the host mirror of a pool slot (J0 = null: stays on the device)
  double sum_dt[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};   // vilo_win_sum_dt of the intervals the window has
  bool resident_records = false;       // the preintegration records come out of a device pool: the desc needs none
  const char *refs_defect = nullptr;   // references this batch cannot take: refused as UNSUPPORTED with this message
};

struct PackPlan {
  std::vector<WinMeta> wins; std::vector<ChunkMeta> chunks; std::vector<WaveMeta> waves;
  std::vector<int> wave_order;      // launch order of the packed waves
  std::vector<int> perm;            // device order -> original landmark index (per window, concatenated)
  std::vector<int> obs_row;         // the caller's observation row of each landmark's first observation (device order, rows concatenated by window)
  std::vector<int> lm_off, L;       // per window
  std::vector<double> lam0;         // inverse depths, device order
  std::vector<unsigned char> lm_s;  // start frame per landmark (device order)
  int lm_total = 0, gram_total = 0, n_obs_rows = 0;
  size_t obs_total = 0, flags_total = 0;   // doubles of the observation image, bytes of its flags
  bool any_prior = false;
  int compact = 0;   // compact visual rows / Gram slots in the solve passes: td a constant block in every window (and the context allows it)
};

// Where fill_batch writes. obs / flags: PackPlan::obs_total doubles / flags_total bytes. Per window, zero when handed in: x0 [XSTRIDE],
// prior_map [96], prior_bsize / _bidx / _bxoff / _bstate [40], prior_x0 [280]. Per window, any content: imu_skip [10], J0 [96 * 96] (n x n
// packed) and r0 [96], of which only n x n / n of a window with a host prior are written.
struct PackOut {
  double *obs; unsigned char *flags; double *x0;
  int *prior_map, *prior_bsize, *prior_bidx, *prior_bxoff, *prior_bstate;
  double *prior_x0, *J0, *r0; unsigned char *imu_skip;
};

inline bool has_prior(const vilo_prior *p) { return p && p->valid && p->n > 0; }

// The kinds of parameter block a prior may keep (id = kind * 16 + index): global size, number of indices, first state double and first
// camera dimension of index 0 and their steps per index.
struct PriorBlockKind { int size, n_index, state0, state_step, cd0, cd_step; };
inline const PriorBlockKind &prior_block_kind(int kind) {   // VILO_BLK_POSE, _SB, _LB, _EX, _TD
  static const PriorBlockKind kinds[5] = {{7, VILO_MAX_FRAMES, XO_POSE, 7, 0, 6}, {9, VILO_MAX_FRAMES, XO_SB, 9, CD_B0, 13}, {4, VILO_MAX_FRAMES, XO_LB, 4, CD_B0 + 9, 13},
                                          {7, 2, XO_EX, 7, CD_EX0, 6}, {1, 1, XO_TD, 0, CD_TD, 0}};
  return kinds[kind];
}

// The block table of a prior (MarginalizationFactor, marginalization_factor.cpp:335-395): checked, and with `out` written as one
// window's rows of the device tables. A table that indexes outside the prior or names a block that does not exist is a bad argument
// (the assembly indexes its LDS image through these); a table that is sound but beyond what the solver takes — a block that is not
// camera-side (a feature), overlapping local ranges, more than 280 state doubles, speed / leg-bias blocks of two frames — is
// unsupported. bias_frame: the frame whose speed / leg-bias block the prior touches (-1: none).
inline PackStatus prior_blocks(const vilo_prior &p, const PackOut *out, int w, int *bias_frame) {
  if (p.n > VILO_MAX_PRIOR_DIM || p.n_blocks < 0 || p.n_blocks > VILO_MAX_PRIOR_BLOCKS) return {VILO_ERR_BAD_ARG, nullptr};
  auto local = [](int gs) { return gs == 7 ? 6 : gs; };   // a pose's local size
  auto camera_side = [](int id) { return id >= 0 && id < 16 * 5; };
  for (int k = 0; k < p.n_blocks; ++k) {
    const int id = p.block_id[k], idx = p.block_idx[k];
    if (!camera_side(id)) continue;   // (refused below, as unsupported)
    const PriorBlockKind &bk = prior_block_kind(id >> 4);
    if (p.block_size[k] != bk.size || (id & 15) >= bk.n_index || idx < 0 || idx + local(bk.size) > p.n) return {VILO_ERR_BAD_ARG, "prior block table out of range"};
  }
  int xo = 0, bframe = -1;
  for (int k = 0; k < p.n_blocks; ++k) {
    const int id = p.block_id[k], gs = p.block_size[k], ls = local(gs), idx = p.block_idx[k];
    if (!camera_side(id) || xo + gs > 280) return {VILO_ERR_UNSUPPORTED, "unsupported prior block"};
    for (int q = 0; q < k; ++q)   // local index ranges must not overlap
      if (idx < p.block_idx[q] + local(p.block_size[q]) && p.block_idx[q] < idx + ls) return {VILO_ERR_UNSUPPORTED, "unsupported prior block"};
    const PriorBlockKind &bk = prior_block_kind(id >> 4);
    const int cd = bk.cd0 + bk.cd_step * (id & 15);
    if (cd >= CD_B0) {
      const int fr = (cd - CD_B0) / 13;
      if (bframe >= 0 && bframe != fr) return {VILO_ERR_UNSUPPORTED, "prior couples speed/leg biases of two frames"};
      bframe = fr;
    }
    if (out) {
      const size_t b = (size_t)w * 40 + k;
      out->prior_bsize[b] = gs; out->prior_bidx[b] = idx; out->prior_bxoff[b] = xo; out->prior_bstate[b] = bk.state0 + bk.state_step * (id & 15);
      for (int c = 0; c < ls; ++c) out->prior_map[(size_t)w * 96 + idx + c] = cd + c;
      for (int c = 0; c < gs; ++c) out->prior_x0[(size_t)w * 280 + xo + c] = p.x0[xo + c];
    }
    xo += gs;
  }
  *bias_frame = bframe;
  return {};
}

// What a window must bring before any of its tables is walked. The observation table is indexed through lm_obs_offset: [0] = 0,
// non-decreasing, [L] = n_obs, and every start frame names a frame of the window — fill_batch reads obs[11 * (offset + t)] for t < K.
inline PackStatus check_window(const vilo_window_desc &d, const vilo_window_state &s, const PackWindow &r, const vilo_window_desc &first) {
  if (d.n_frames < 2 || d.n_frames > VILO_MAX_FRAMES || d.n_landmarks < 0 || d.n_landmarks > VILO_NUM_OF_F) return {VILO_ERR_BAD_ARG, "window sizes out of range"};
  if ((d.use_leg != 0) != (first.use_leg != 0)) return {VILO_ERR_UNSUPPORTED, "all windows of a batch must use the same IMU factor kind (use_leg)"};
  if (r.refs_defect) return {VILO_ERR_UNSUPPORTED, r.refs_defect};
  const int F = d.n_frames, L = d.n_landmarks;
  if (!(d.use_leg ? (const void *)d.preint : (const void *)d.preint_imu) && !r.resident_records) return {VILO_ERR_BAD_ARG, nullptr};
  if (!s.pose || !s.speed_bias || !s.leg_bias || !s.ex_pose || !s.td) return {VILO_ERR_BAD_ARG, nullptr};
  if (L > 0) {
    if (!s.inv_depth || !d.lm_start_frame || !d.lm_obs_offset || !d.obs || !d.obs_is_stereo) return {VILO_ERR_BAD_ARG, nullptr};
    bool ok = d.n_obs >= 0 && d.lm_obs_offset[0] == 0 && d.lm_obs_offset[L] == d.n_obs;
    for (int l = 0; ok && l < L; ++l) ok = d.lm_obs_offset[l + 1] >= d.lm_obs_offset[l] && d.lm_start_frame[l] >= 0 && d.lm_start_frame[l] < F;
    if (!ok) return {VILO_ERR_BAD_ARG, "landmark observation table: lm_obs_offset must start at 0, not decrease and end at n_obs; start frames must lie in the window"};
  }
  return {};
}

// Window w's landmarks in device order and its chunks: grouped by start frame (a stable counting sort: list order preserved inside a
// group), <= 64 per chunk. A chunk's landmarks are its lm_off .. lm_off + n entries of perm.
inline PackStatus plan_chunks(int w, const vilo_window_desc &d, const vilo_window_state &s, PackPlan &p) {
  const int F = d.n_frames, L = d.n_landmarks;
  int first[VILO_MAX_FRAMES + 1] = {0}, fill[VILO_MAX_FRAMES];
  for (int l = 0; l < L; ++l) ++first[d.lm_start_frame[l] + 1];
  for (int sf = 0; sf < F; ++sf) first[sf + 1] += first[sf];
  const size_t base = p.perm.size();
  p.perm.resize(base + L); p.lam0.resize(base + L); p.lm_s.resize(base + L); p.obs_row.resize(base + L);
  for (int sf = 0; sf < F; ++sf) fill[sf] = first[sf];
  for (int l = 0; l < L; ++l) {
    const int sf = d.lm_start_frame[l], at = fill[sf]++;
    p.perm[base + at] = l; p.lam0[base + at] = s.inv_depth[l]; p.lm_s[base + at] = (unsigned char)sf;
  }
  for (int i = 0; i < L; ++i) p.obs_row[base + i] = p.n_obs_rows + d.lm_obs_offset[p.perm[base + i]];
  if (L > 0) p.n_obs_rows += d.lm_obs_offset[L];
  for (int sf = 0; sf < F; ++sf)
    for (int c0 = first[sf]; c0 < first[sf + 1]; c0 += 64) {
      ChunkMeta cm = {};
      cm.win = w; cm.s = sf; cm.n = std::min(64, first[sf + 1] - c0); cm.lm_off = p.lm_total + c0; cm.lm_local = c0;
      for (int i = 0; i < cm.n; ++i) {
        const int l = p.perm[base + c0 + i], K = d.lm_obs_offset[l + 1] - d.lm_obs_offset[l];
        if (K < 1 || sf + K > F) return {VILO_ERR_BAD_ARG, "landmark observation range outside the window"};
        cm.kmax = std::max(cm.kmax, K);
      }
      cm.gram_off = p.gram_total;
      p.gram_total += cm.kmax;
      p.chunks.push_back(cm);
    }
  return {};
}

// The chunks from c on (one window's) packed into waves: consecutive chunks side by side, each at a lane multiple of 8, <= 4 per wave
inline void plan_waves(int w, int c, PackPlan &p) {
  while (c < (int)p.chunks.size()) {
    WaveMeta wv = {};
    wv.win = w;
    int lanes = 0;
    while (c < (int)p.chunks.size() && wv.nseg < 4) {
      const int pad = (p.chunks[c].n + 7) & ~7;
      if (lanes + pad > 64) break;
      wv.seg_chunk[wv.nseg] = c; wv.seg_lane0[wv.nseg] = lanes;
      wv.kmax = std::max(wv.kmax, p.chunks[c].kmax);
      lanes += pad; ++wv.nseg; ++c;
    }
    wv.n_lanes = lanes;
    wv.obs_off = (long long)p.obs_total;
    wv.flag_off = (long long)p.flags_total;
    p.obs_total += (size_t)wv.kmax * 11 * lanes;
    p.flags_total += (size_t)wv.kmax * lanes;
    p.waves.push_back(wv);
  }
}

// Launch order of the packed waves: by decreasing number of frames walked. A single-wave workgroup can only start on the SIMD the
// dispatcher's cyclic pointer names, so waves of mixed length in flight on one CU leave SIMDs idle behind a long one (measured: 2.7
// instead of 4 resident waves per CU); with equal lengths adjacent they retire in launch order and the longest ones do not form the tail.
inline std::vector<int> plan_wave_order(const std::vector<WaveMeta> &waves, int wave_order) {
  std::vector<int> order(waves.size());
  for (size_t i = 0; i < order.size(); ++i) order[i] = (int)i;
  if (wave_order >= 1) std::stable_sort(order.begin(), order.end(), [&](int a, int c) { return waves[a].kmax > waves[c].kmax; });
  if (wave_order == 2) {
    size_t g0 = 0; int gi = 0;
    while (g0 < order.size()) {
      size_t g1 = g0;
      while (g1 < order.size() && waves[order[g1]].kmax == waves[order[g0]].kmax) ++g1;
      if (g1 - g0 > 8) std::rotate(order.begin() + g0, order.begin() + g0 + (gi % 8), order.begin() + g1);
      g0 = g1; ++gi;
    }
  }
  return order;
}

// Step 1. res: [W], what the caller resolved of each window's references. The first defective window decides what is returned, except
// that a prior which is sound but unsupported (prior_blocks) is reported only if no window has a defect of any other kind.
inline PackStatus plan_batch(int W, const vilo_window_desc *in, const vilo_window_state *init, const PackWindow *res, bool compact_rows, const Tuning &t, PackPlan &p) {
  p = PackPlan();
  p.wins.resize(W); p.lm_off.resize(W); p.L.resize(W);
  p.compact = compact_rows ? 1 : 0;
  PackStatus unsupported_prior;
  for (int w = 0; w < W; ++w) {
    const vilo_window_desc &d = in[w];
    PackStatus st = check_window(d, init[w], res[w], in[0]);
    if (st.code != VILO_OK) return st;
    WinMeta &wm = p.wins[w];   // (zero: the vector's)
    wm.n_frames = d.n_frames; wm.L = d.n_landmarks; wm.use_leg = d.use_leg; wm.pad = -1;
    wm.lm_off = p.lm_total; wm.chunk_off = (int)p.chunks.size(); wm.gram_off = p.gram_total; wm.wave_off = (int)p.waves.size();
    // use_leg == 0: the leg-bias blocks are not part of the problem (estimator.cpp:1071-1072): masked like constant blocks
    wm.const_mask = ((d.leg_bias_const || !d.use_leg) ? CONST_LB : 0) | (d.ex_const ? CONST_EX : 0) | (d.td_const ? CONST_TD : 0);
    if (!(wm.const_mask & CONST_TD)) p.compact = 0;
    p.lm_off[w] = p.lm_total; p.L[w] = d.n_landmarks;
    st = plan_chunks(w, d, init[w], p);
    if (st.code != VILO_OK) return st;
    plan_waves(w, wm.chunk_off, p);
    wm.n_chunks = (int)p.chunks.size() - wm.chunk_off;
    wm.n_waves = (int)p.waves.size() - wm.wave_off;
    wm.n_gram = p.gram_total - wm.gram_off;
    p.lm_total += d.n_landmarks;
    if (has_prior(res[w].prior)) {
      int bias_frame;
      st = prior_blocks(*res[w].prior, nullptr, w, &bias_frame);
      if (st.code == VILO_ERR_BAD_ARG) return st;
      if (st.code != VILO_OK && unsupported_prior.code == VILO_OK) unsupported_prior = st;
      p.any_prior = true;
    }
  }
  p.wave_order = plan_wave_order(p.waves, t.wave_order);
  return unsupported_prior;
}

// One window of step 2: its state (vector2double layout; absent frames get the unit quaternion), its waves' observation image
// [t][11][lanes] and flags [t][lanes] (1 valid | 2 stereo), the intervals that carry no IMU factor (beyond the window, or sum_dt > 10 s:
// estimator.cpp:1118,1164) and its prior's rows (H = J0^T J0, b0 = J0^T r0, c0 = r0^T r0 are the device's to form, from J0 / r0).
inline void fill_window(int w, const vilo_window_desc &d, const vilo_window_state &s, const PackWindow &r, PackPlan &p, const PackOut &o) {
  WinMeta &wm = p.wins[w];
  const int F = d.n_frames;
  double *xw = o.x0 + (size_t)w * XSTRIDE;
  memcpy(xw + XO_POSE, s.pose, sizeof(double) * 7 * F);
  memcpy(xw + XO_SB, s.speed_bias, sizeof(double) * 9 * F);
  memcpy(xw + XO_LB, s.leg_bias, sizeof(double) * 4 * F);
  for (int k = F; k < VILO_MAX_FRAMES; ++k) xw[XO_POSE + 7 * k + 6] = 1.0;
  memcpy(xw + XO_EX, s.ex_pose, sizeof(double) * 14);
  xw[XO_TD] = s.td[0];
  for (int wi = wm.wave_off; wi < wm.wave_off + wm.n_waves; ++wi) {
    const WaveMeta &wv = p.waves[wi];
    const int lanes = wv.n_lanes;
    double *ob = o.obs + wv.obs_off;
    unsigned char *fl = o.flags + wv.flag_off;
    memset(ob, 0, sizeof(double) * (size_t)wv.kmax * 11 * lanes);
    memset(fl, 0, (size_t)wv.kmax * lanes);
    for (int g = 0; g < wv.nseg; ++g) {
      const ChunkMeta &cm = p.chunks[wv.seg_chunk[g]];
      const int *ids = p.perm.data() + cm.lm_off;   // the chunk's landmarks (window order)
      for (int i = 0; i < cm.n; ++i) {
        const int l = ids[i], lane = wv.seg_lane0[g] + i;
        const int o0 = d.lm_obs_offset[l], K = d.lm_obs_offset[l + 1] - o0;
        for (int t = 0; t < K; ++t) {
          for (int f = 0; f < 11; ++f) ob[((size_t)t * 11 + f) * lanes + lane] = d.obs[(size_t)(o0 + t) * 11 + f];
          fl[(size_t)t * lanes + lane] = (unsigned char)(1 | (d.obs_is_stereo[o0 + t] ? 2 : 0));
        }
      }
    }
  }
  for (int k = 0; k < 10; ++k) o.imu_skip[(size_t)w * 10 + k] = (k + 1 < F && !(r.sum_dt[k] > 10.0)) ? 0 : 1;
  if (!has_prior(r.prior)) return;
  const vilo_prior &pr = *r.prior;
  wm.prior_n = pr.n; wm.prior_nb = pr.n_blocks;
  (void)prior_blocks(pr, &o, w, &wm.pad);   // (checked by plan_batch)
  if (pr.J0) {   // a pool slot keeps J0 / r0 on the device
    memcpy(o.J0 + (size_t)w * 96 * 96, pr.J0, sizeof(double) * (size_t)pr.n * pr.n);
    memcpy(o.r0 + (size_t)w * 96, pr.r0, sizeof(double) * pr.n);
  }
}

// Step 2 (after plan_batch returned VILO_OK), on the host threads of `pool` (null: the library's shared ones)
inline void fill_batch(int W, const vilo_window_desc *in, const vilo_window_state *init, const PackWindow *res, PackPlan &p, const PackOut &o, WorkerPool *pool) {
  parallel_items(W, 8, [&](int w) { fill_window(w, in[w], init[w], res[w], p, o); }, pool);
}

}  // namespace vilo
