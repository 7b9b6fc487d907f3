// tests/test_marg_plan.py compiles this (under sanitizers) and runs it once per case: the host bookkeeping of a marginalisation call
// (cerberus_amd/csrc/marg_plan.hpp) on windows read from files (include/vilo_window_io.h, written by cerberus_amd/window_io.py), on a CPU.
//   marg_plan_check --mode M [--mask L,L,...] [--unpacked] FILE...
// M: 0 MARGIN_OLD, 1 MARGIN_SECOND_NEW, every window. --mask: landmarks (original indices) masked in every window that has them.
// --unpacked: plan_batch is not run (a window beyond what a batch takes); every landmark must start in frame 0, where the device order is
// the original one.
// Prints "status CODE" (plan_batch's, if it refuses, else plan_marginalization's) and, when the plan was accepted, per window w every
// table of the plan ("win_w", "cdmap_w", "perm_w", "drop_w", "kept_w"), the scratch offsets with every window that marginalises marked
// general ("scratch": offsets, then the total), and the prior the two write-out functions leave in exactly-sized heap buffers
// ("prior_w": n n_blocks valid; "block_id_w", "block_size_w", "block_idx_w", "x0_w").
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../cerberus_amd/csrc/marg_plan.hpp"
#include "../../include/vilo_window_io.h"

template <class T>
static void line(const std::string &name, const T *v, size_t n) {
  printf("%s", name.c_str());
  for (size_t i = 0; i < n; ++i) {
    if (sizeof(T) == sizeof(double)) printf(" %.17g", (double)v[i]);
    else printf(" %lld", (long long)v[i]);
  }
  printf("\n");
}

int main(int argc, char **argv) {
  int mode = -1;
  bool unpacked = false;
  std::vector<int> masked;
  std::vector<const char *> paths;
  for (int i = 1; i < argc; ++i) {
    if (!strcmp(argv[i], "--mode") && i + 1 < argc) mode = atoi(argv[++i]);
    else if (!strcmp(argv[i], "--unpacked")) unpacked = true;
    else if (!strcmp(argv[i], "--mask") && i + 1 < argc) {
      for (char *tok = strtok(argv[++i], ","); tok; tok = strtok(nullptr, ",")) masked.push_back(atoi(tok));
    } else paths.push_back(argv[i]);
  }
  const int W = (int)paths.size();
  if (W == 0 || (mode != 0 && mode != 1)) return 2;
  std::vector<vilo_window_file> files(W);
  for (int w = 0; w < W; ++w)
    if (vilo_window_read(paths[w], &files[w]) != 0) { fprintf(stderr, "cannot read %s\n", paths[w]); return 2; }
  std::vector<vilo_window_desc> in(W);
  std::vector<vilo_window_state> state(W);
  std::vector<vilo::PackWindow> res(W);
  for (int w = 0; w < W; ++w) {
    in[w] = files[w].desc; state[w] = files[w].before;
    res[w].prior = in[w].prior;
    for (int k = 0; k + 1 < in[w].n_frames; ++k) res[w].sum_dt[k] = in[w].use_leg ? in[w].preint[k].sum_dt : in[w].preint_imu[k].sum_dt;
  }
  // perm, L, lm_off: the batch's landmark order
  vilo::PackPlan P;
  if (unpacked) {
    for (int w = 0; w < W; ++w) {
      P.lm_off.push_back((int)P.perm.size()); P.L.push_back(in[w].n_landmarks);
      for (int l = 0; l < in[w].n_landmarks; ++l) {
        if (in[w].lm_start_frame[l] != 0) return 2;
        P.perm.push_back(l);
      }
    }
  } else {
    const vilo::PackStatus st = vilo::plan_batch(W, in.data(), state.data(), res.data(), true, vilo::tuning(), P);
    if (st.code != VILO_OK) { printf("status %d\n", st.code); return 0; }
  }
  // the mask mirror: device order, as vilo_batch_mask_landmarks leaves it
  std::vector<unsigned char> mirror(P.perm.size(), 0);
  for (int w = 0; w < W; ++w)
    for (int i = 0; i < P.L[w]; ++i)
      for (int l : masked)
        if (P.perm[P.lm_off[w] + i] == l) mirror[P.lm_off[w] + i] = 1;
  std::vector<vilo::MargWindow> mw(W);
  for (int w = 0; w < W; ++w) {
    mw[w].desc = &in[w]; mw[w].prior = in[w].prior; mw[w].sum_dt0 = res[w].sum_dt[0]; mw[w].mode = mode;
    mw[w].L = P.L[w]; mw[w].perm = P.perm.data() + P.lm_off[w]; mw[w].mask = masked.empty() ? nullptr : mirror.data() + P.lm_off[w];
  }
  vilo::MargPlan plan;
  const vilo::PackStatus st = vilo::plan_marginalization(W, mw.data(), plan);
  printf("status %d\n", st.code);
  if (st.code == VILO_OK) {
    for (int w = 0; w < W; ++w) {
      const std::string s = "_" + std::to_string(w);
      const vilo::MargWin &M = plan.wins[w];
      const long long head[9] = {M.m, M.n, M.n_drop_lm, M.mode, M.has_imu, M.prior_n, plan.skip[w], plan.keep_prior[w], plan.max_l0};
      line("win" + s, head, 9);
      line("cdmap" + s, M.cdmap, CD_N);
      line("perm" + s, mw[w].perm, (size_t)mw[w].L);
      line("drop" + s, plan.drop_lm.data() + (size_t)w * plan.max_l0, (size_t)M.n_drop_lm);
      std::vector<int> t;
      for (const vilo::MargKept &k : plan.kept[w]) t.insert(t.end(), {k.id, k.idx, k.size, k.state_off});
      line("kept" + s, t.data(), t.size());
    }
    std::vector<vilo::MargWin> gen = plan.wins;
    for (vilo::MargWin &M : gen) M.general = M.m > 0 && M.n > 0;
    std::vector<long long> so;
    const size_t total = vilo::assign_marg_scratch(gen);
    for (const vilo::MargWin &M : gen) so.push_back(M.general ? M.scratch_off : -1);
    so.push_back((long long)total);
    line("scratch", so.data(), so.size());
    for (int w = 0; w < W; ++w) {   // as the call's last step decides, every result taken as finite
      const std::string s = "_" + std::to_string(w);
      std::unique_ptr<double[]> x0(new double[7 * VILO_MAX_PRIOR_BLOCKS]), J0(new double[VILO_MAX_PRIOR_DIM * VILO_MAX_PRIOR_DIM]), r0(new double[VILO_MAX_PRIOR_DIM]);
      vilo_prior p;
      memset(&p, 0, sizeof(p));
      p.x0 = x0.get(); p.J0 = J0.get(); p.r0 = r0.get();
      if (plan.keep_prior[w]) vilo::copy_prior_meta(*in[w].prior, p, false);
      else if (plan.wins[w].m == 0 || plan.wins[w].n == 0) { p.valid = 0; p.n = 0; }
      else vilo::write_prior_meta(plan, w, in[w].n_frames, state[w], p);
      const long long head[3] = {p.n, p.n_blocks, p.valid};
      line("prior" + s, head, 3);
      int sum_g = 0;
      for (int k = 0; k < p.n_blocks; ++k) sum_g += p.block_size[k];
      line("block_id" + s, p.block_id, (size_t)p.n_blocks);
      line("block_size" + s, p.block_size, (size_t)p.n_blocks);
      line("block_idx" + s, p.block_idx, (size_t)p.n_blocks);
      line("x0" + s, p.x0, (size_t)sum_g);
    }
  }
  for (vilo_window_file &f : files) vilo_window_free(&f);
  return 0;
}
