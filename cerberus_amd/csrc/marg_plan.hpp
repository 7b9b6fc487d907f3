// The host bookkeeping of a marginalisation call (Estimator::optimization(), estimator.cpp:1247-1455): which parameter blocks of a window
// take part, which are dropped and which kept, where each sits in the [dropped | kept] ordering the kernels build A and b in, and the
// kept-block table of the prior that comes out. Integer block ids (kind * 16 + index) stand where the reference keys on addresses
// (addr_shift, estimator.cpp:1358-1370).
//   plan_marginalization  per window: the MargWin the kernels read, the dropped landmarks, the kept blocks, skip / keep-the-old-prior;
//   assign_marg_scratch   where each window of the eigen path finds its scratch;
//   write_prior_meta / copy_prior_meta   the new prior's host side (everything but J0 / r0 of a computed one).
// Plain C++17, no HIP: kernels_marg.hip uploads what this leaves and runs the kernels; tests/host_check/marg_plan_check.cpp runs it on a
// CPU under sanitizers, tests/test_marg_plan.py holds its output against the oracle's marginalisation. What needs the batch or a window's
// resident references is the caller's to resolve: the planner sees a MargWindow.
#pragma once
#include <stddef.h>

#include <utility>

#include "batch_pack.hpp"

namespace vilo {

// One window as k_marginalize_lds / k_marginalize read it
struct MargWin {
  int m, n;             // dropped / kept local dims
  int n_drop_lm;        // landmarks among the dropped dims (they follow the 19 frame-0 dims; mode 0)
  int mode;
  int has_imu, prior_n;
  int general;          // 1: this window goes through the global-memory eigen path (set by the host from k_marginalize_lds' verdict)
  int pad1;
  long long scratch_off;  // doubles into the scratch arena
  int cdmap[CD_N];      // camera dim -> index in [dropped | kept] ordering, -1 if absent
};
static_assert(sizeof(MargWin) == 40 + 4 * CD_N && offsetof(MargWin, cdmap) == 40, "MargWin: 8 ints, scratch_off, cdmap (the kernels' view)");

// What the caller resolved of window w. The window has been through plan_batch: its tables are sound and its prior's blocks camera-side.
struct MargWindow {
  const vilo_window_desc *desc = nullptr;
  const vilo_prior *prior = nullptr;    // vilo_win_prior: the desc's, or the host mirror of a pool slot
  double sum_dt0 = 0.0;                 // vilo_win_sum_dt of interval 0 (read in mode 0 only)
  int L = 0;                            // the window's landmarks,
  const int *perm = nullptr;            // their device order -> original index (its slice of PackPlan::perm)
  const unsigned char *mask = nullptr;  // and its slice of the mask mirror (device order), or null: none masked
  int mode = 0;                         // 0 MARGIN_OLD, 1 MARGIN_SECOND_NEW, < 0 the window is skipped
};

// A block the new prior keeps: its id before the frame shift, its first local dim among the kept ones, its global size, its first state double
struct MargKept { int id, idx, size, state_off; };

struct MargPlan {
  std::vector<MargWin> wins;
  std::vector<int> drop_lm;   // [W][max_l0] dropped landmarks, device-order local index, ascending in original index
  int max_l0 = 1;
  std::vector<std::vector<MargKept>> kept;   // per window, ascending id
  std::vector<char> skip;                    // mode < 0: its output is left untouched
  std::vector<char> keep_prior;              // MARGIN_SECOND_NEW with nothing to marginalise: the old prior carries over
};

inline int local_size(const PriorBlockKind &bk) { return bk.size == 7 ? 6 : bk.size; }   // a pose's local size

// in[W]. VILO_ERR_UNSUPPORTED (no text) for a window beyond what the kernels take: more than VILO_MAX_PRIOR_DIM kept dims, more than
// VILO_MAX_PRIOR_BLOCKS kept blocks, more than 1200 dropped dims.
inline PackStatus plan_marginalization(int W, const MargWindow *in, MargPlan &p) {
  p = MargPlan();
  p.wins.resize(W); p.kept.resize(W); p.skip.assign(W, 0); p.keep_prior.assign(W, 0);
  std::vector<std::vector<int>> drops(W);
  for (int w = 0; w < W; ++w) {
    const vilo_window_desc &d = *in[w].desc;
    MargWin &M = p.wins[w];
    memset(&M, 0, sizeof(M));
    for (int i = 0; i < CD_N; ++i) M.cdmap[i] = -1;
    const int mode = in[w].mode;
    if (mode < 0) { p.skip[w] = 1; continue; }
    M.mode = mode;
    const int WS = d.n_frames - 1;
    const vilo_prior *prw = in[w].prior;
    const bool prior = has_prior(prw);
    M.prior_n = prior ? prw->n : 0;
    // which camera blocks take part (id = kind*16 + index), in the oracle's canonical order
    std::vector<int> present;   // block ids
    auto is_present = [&](int id) { return std::find(present.begin(), present.end(), id) != present.end(); };
    auto mark = [&](int id) { if (!is_present(id)) present.push_back(id); };
    if (prior)
      for (int k = 0; k < prw->n_blocks; ++k) mark(prw->block_id[k]);
    std::vector<int> dropped_ids;
    if (mode == 0) {
      const int nkind = d.use_leg ? 3 : 2;   // pose, speed/bias (, leg bias)
      M.has_imu = in[w].sum_dt0 < 10.0 ? 1 : 0;
      if (M.has_imu)
        for (int kind = 0; kind < nkind; ++kind) { mark(kind * 16 + 0); mark(kind * 16 + 1); }
      const int L = in[w].L, *perm = in[w].perm;
      // a masked landmark (vilo_batch_mask_landmarks) is the deleted one: in no residual block, so it marks no block and is not among
      // the eliminated landmarks (its E_l is 0: the inverse k_marginalize_lds takes of it would send the window to the eigen path)
      const unsigned char *msk = in[w].mask;
      for (int i = 0; i < L; ++i) {
        const int l = perm[i];
        if (d.lm_start_frame[l] != 0 || (msk && msk[i])) continue;
        const int K = d.lm_obs_offset[l + 1] - d.lm_obs_offset[l];
        mark(VILO_BLK_POSE * 16 + 0);
        for (int t = 1; t < K; ++t) mark(VILO_BLK_POSE * 16 + t);
        mark(VILO_BLK_EX * 16 + 0); mark(VILO_BLK_EX * 16 + 1); mark(VILO_BLK_TD * 16);
      }
      // dropped landmark list in ORIGINAL feature order (oracle: ascending parameter index)
      std::vector<std::pair<int, int>> dl;
      for (int i = 0; i < L; ++i)
        if (d.lm_start_frame[perm[i]] == 0 && !(msk && msk[i])) dl.push_back({perm[i], i});
      std::sort(dl.begin(), dl.end());
      for (auto &pr : dl) drops[w].push_back(pr.second);
      M.n_drop_lm = (int)drops[w].size();
      p.max_l0 = std::max(p.max_l0, M.n_drop_lm);
      for (int kind = 0; kind < 3; ++kind)
        if (is_present(kind * 16)) dropped_ids.push_back(kind * 16);
    } else {
      if (!prior || !is_present(VILO_BLK_POSE * 16 + (WS - 1))) {
        // estimator.cpp:1379-1380: nothing is marginalised and last_marginalization_info stays as it is
        p.keep_prior[w] = prior ? 1 : 0;
        continue;
      }
      dropped_ids.push_back(VILO_BLK_POSE * 16 + (WS - 1));
    }
    // the block's camera dims take the next local positions; returns its kind
    int pos = 0;
    auto place = [&](int id) -> const PriorBlockKind & {
      const PriorBlockKind &bk = prior_block_kind(id / 16);
      const int cd = bk.cd0 + bk.cd_step * (id % 16), ls = local_size(bk);
      for (int c = 0; c < ls; ++c) M.cdmap[cd + c] = pos + c;
      pos += ls;
      return bk;
    };
    std::sort(dropped_ids.begin(), dropped_ids.end());
    for (int id : dropped_ids) place(id);
    // (without an IMU factor on interval (0, 1) — sum_dt > 10 s — and without a prior on them, speed-bias / leg-bias of frame 0 are in no
    // residual block and are not marginalised: the dense dropped part is the pose alone, as in MarginalizationInfo::addResidualBlockInfo)
    pos += M.n_drop_lm;
    M.m = pos;
    std::vector<int> kept;
    for (int id : present)
      if (std::find(dropped_ids.begin(), dropped_ids.end(), id) == dropped_ids.end()) kept.push_back(id);
    std::sort(kept.begin(), kept.end());
    for (int id : kept) {
      const int idx = pos - M.m;
      const PriorBlockKind &bk = place(id);
      p.kept[w].push_back({id, idx, bk.size, bk.state0 + bk.state_step * (id % 16)});
    }
    M.n = pos - M.m;
    if (M.n > VILO_MAX_PRIOR_DIM || (int)kept.size() > VILO_MAX_PRIOR_BLOCKS || M.m > 1200) return {VILO_ERR_UNSUPPORTED, nullptr};
  }
  p.drop_lm.assign((size_t)W * p.max_l0, 0);
  for (int w = 0; w < W; ++w)
    for (size_t i = 0; i < drops[w].size(); ++i) p.drop_lm[(size_t)w * p.max_l0 + i] = drops[w][i];
  return {};
}

// scratch_off of the windows marked general (k_marginalize's layout: A | b | Amm | Vm | Ainv | tmp | Ar | V2 | br, A' kept behind it);
// returns the doubles they take together
inline size_t assign_marg_scratch(std::vector<MargWin> &wins) {
  size_t total = 0;
  for (MargWin &M : wins) {
    if (!M.general) continue;
    M.scratch_off = (long long)total;
    const size_t T = (size_t)M.m + M.n;
    total += T * T + T + 3 * (size_t)M.m * M.m + (size_t)M.n * M.m + 3 * (size_t)M.n * M.n + 2 * M.n + 64;
  }
  return total;
}

// The host side of the prior window w's marginalisation computed (J0 / r0 are the device's): the kept blocks with the frame shift —
// addr_shift: MARGIN_OLD frame k -> k - 1 (estimator.cpp:1358-1368); MARGIN_SECOND_NEW frame WS -> WS - 1 (:1413-1447) — and x0 from the
// state the window was linearised at (keep_block_data)
inline void write_prior_meta(const MargPlan &plan, int w, int n_frames, const vilo_window_state &s, vilo_prior &p) {
  const std::vector<MargKept> &kept = plan.kept[w];
  const int mode = plan.wins[w].mode, WS = n_frames - 1;
  p.n = plan.wins[w].n; p.n_blocks = (int)kept.size(); p.valid = 1;
  const double *xs[5] = {s.pose, s.speed_bias, s.leg_bias, s.ex_pose, s.td};
  int xo = 0;
  for (int k = 0; k < p.n_blocks; ++k) {
    const int kind = kept[k].id / 16, index = kept[k].id % 16;
    const bool shift = kind <= VILO_BLK_LB && (mode == 0 || index == WS);
    p.block_id[k] = shift ? kept[k].id - 1 : kept[k].id; p.block_size[k] = kept[k].size; p.block_idx[k] = kept[k].idx;
    const double *src = xs[kind] + prior_block_kind(kind).state_step * index;
    for (int c = 0; c < kept[k].size; ++c) p.x0[xo + c] = src[c];
    xo += kept[k].size;
  }
}

// The keep-the-old-prior case: q carries over into p (which may be q itself, or overlap it). A pooled prior's J0 / r0 stay on the device.
inline void copy_prior_meta(const vilo_prior &q, vilo_prior &p, bool pooled) {
  if (&p == &q) return;
  int sum_g = 0;
  for (int k = 0; k < q.n_blocks; ++k) { p.block_id[k] = q.block_id[k]; p.block_size[k] = q.block_size[k]; p.block_idx[k] = q.block_idx[k]; sum_g += q.block_size[k]; }
  p.n = q.n; p.n_blocks = q.n_blocks; p.valid = 1;
  memmove(p.x0, q.x0, sizeof(double) * sum_g);
  if (!pooled) {
    memmove(p.J0, q.J0, sizeof(double) * (size_t)q.n * q.n);
    memmove(p.r0, q.r0, sizeof(double) * q.n);
  }
}

}  // namespace vilo
