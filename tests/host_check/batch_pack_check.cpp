// tests/test_batch_pack.py compiles this (under sanitizers) and runs it once per case: the host packing stage of a batch
// (cerberus_amd/csrc/batch_pack.hpp) on windows read from files (include/vilo_window_io.h, written by cerberus_amd/window_io.py), on a CPU.
//   batch_pack_check [--mutate WINDOW TABLE INDEX VALUE]... FILE...
// TABLE: lm_obs_offset, lm_start_frame, block_idx, block_size, block_id (one entry of that table of window WINDOW is overwritten after
// the read, as a corrupt file the reader lets through would have it), n_frames, use_leg (the desc's field; INDEX ignored).
// Prints "status CODE", "message TEXT" and, when the plan was accepted, every table plan_batch and fill_batch produce, one per line as
// "name v v v ...". Every output buffer is a heap block of exactly the size the plan states.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../cerberus_amd/csrc/batch_pack.hpp"
#include "../../include/vilo_window_io.h"

template <class T>
static void line(const char *name, const T *v, size_t n) {
  printf("%s", name);
  for (size_t i = 0; i < n; ++i) {
    if (sizeof(T) == sizeof(double)) printf(" %.17g", (double)v[i]);
    else printf(" %lld", (long long)v[i]);
  }
  printf("\n");
}

int main(int argc, char **argv) {
  struct Mutation { int win; std::string table; int index, value; };
  std::vector<Mutation> muts;
  std::vector<const char *> paths;
  for (int i = 1; i < argc; ++i) {
    if (!strcmp(argv[i], "--mutate") && i + 4 < argc) { muts.push_back({atoi(argv[i + 1]), argv[i + 2], atoi(argv[i + 3]), atoi(argv[i + 4])}); i += 4; }
    else paths.push_back(argv[i]);
  }
  const int W = (int)paths.size();
  if (W == 0) return 2;
  std::vector<vilo_window_file> files(W);
  for (int w = 0; w < W; ++w)
    if (vilo_window_read(paths[w], &files[w]) != 0) { fprintf(stderr, "cannot read %s\n", paths[w]); return 2; }
  for (const Mutation &m : muts) {
    if (m.win < 0 || m.win >= W) return 2;
    vilo_window_file &f = files[m.win];
    if (m.table == "lm_obs_offset") ((int32_t *)f.desc.lm_obs_offset)[m.index] = m.value;
    else if (m.table == "lm_start_frame") ((int32_t *)f.desc.lm_start_frame)[m.index] = m.value;
    else if (m.table == "block_idx") f.prior.block_idx[m.index] = m.value;
    else if (m.table == "block_size") f.prior.block_size[m.index] = m.value;
    else if (m.table == "block_id") f.prior.block_id[m.index] = m.value;
    else if (m.table == "n_frames") f.desc.n_frames = m.value;
    else if (m.table == "use_leg") f.desc.use_leg = m.value;
    else return 2;
  }
  std::vector<vilo_window_desc> in(W);
  std::vector<vilo_window_state> init(W);
  std::vector<vilo::PackWindow> res(W);
  for (int w = 0; w < W; ++w) {
    in[w] = files[w].desc; init[w] = files[w].before;
    res[w].prior = in[w].prior;
    const int F = files[w].desc.n_frames >= 2 && files[w].desc.n_frames <= VILO_MAX_FRAMES ? files[w].desc.n_frames : 0;
    for (int k = 0; k + 1 < F; ++k) res[w].sum_dt[k] = in[w].use_leg ? (in[w].preint ? in[w].preint[k].sum_dt : 0.0) : (in[w].preint_imu ? in[w].preint_imu[k].sum_dt : 0.0);
  }
  const char *cr = getenv("CHECK_COMPACT_ROWS");
  vilo::PackPlan P;
  const vilo::PackStatus st = vilo::plan_batch(W, in.data(), init.data(), res.data(), !cr || atoi(cr) != 0, vilo::tuning(), P);
  printf("status %d\nmessage %s\n", st.code, st.msg ? st.msg : "");
  if (st.code != VILO_OK) {
    for (vilo_window_file &f : files) vilo_window_free(&f);
    return 0;
  }
  const size_t Ws = (size_t)W;
  std::unique_ptr<double[]> obs(new double[P.obs_total]), x0(new double[Ws * XSTRIDE]()), px0(new double[Ws * 280]()), J0(new double[Ws * 96 * 96]), r0(new double[Ws * 96]);
  std::unique_ptr<unsigned char[]> flags(new unsigned char[P.flags_total]), iskip(new unsigned char[Ws * 10]);
  std::unique_ptr<int[]> pmap(new int[Ws * 96]()), pbs(new int[Ws * 40]()), pbi(new int[Ws * 40]()), pbx(new int[Ws * 40]()), pbst(new int[Ws * 40]());   // (zero when handed in: PackOut)
  vilo::fill_batch(W, in.data(), init.data(), res.data(), P, {obs.get(), flags.get(), x0.get(), pmap.get(), pbs.get(), pbi.get(), pbx.get(), pbst.get(), px0.get(), J0.get(), r0.get(), iskip.get()}, nullptr);
  const long long totals[9] = {P.lm_total, P.gram_total, (long long)P.obs_total, (long long)P.flags_total, P.n_obs_rows, P.any_prior, P.compact, (long long)P.chunks.size(), (long long)P.waves.size()};
  line("totals", totals, 9);
  static_assert(sizeof(WinMeta) == 14 * sizeof(int), "WinMeta: 14 ints");
  line("wins", (const int *)P.wins.data(), Ws * 14);
  std::vector<long long> t;
  for (const ChunkMeta &c : P.chunks) t.insert(t.end(), {c.win, c.s, c.n, c.kmax, c.lm_off, c.lm_local, c.gram_off});
  line("chunks", t.data(), t.size());
  t.clear();
  for (const WaveMeta &v : P.waves) {
    t.insert(t.end(), {v.win, v.nseg, v.n_lanes, v.kmax});
    for (int g = 0; g < 4; ++g) t.push_back(v.seg_chunk[g]);
    for (int g = 0; g < 4; ++g) t.push_back(v.seg_lane0[g]);
    t.insert(t.end(), {v.obs_off, v.flag_off});
  }
  line("waves", t.data(), t.size());
  line("wave_order", P.wave_order.data(), P.wave_order.size());
  line("perm", P.perm.data(), P.perm.size());
  line("lm_s", P.lm_s.data(), P.lm_s.size());
  line("obs_row", P.obs_row.data(), P.obs_row.size());
  line("lm_off", P.lm_off.data(), P.lm_off.size());
  line("L", P.L.data(), P.L.size());
  line("lam0", P.lam0.data(), P.lam0.size());
  line("obs", obs.get(), P.obs_total);
  line("flags", flags.get(), P.flags_total);
  line("x0", x0.get(), Ws * XSTRIDE);
  line("imu_skip", iskip.get(), Ws * 10);
  line("prior_map", pmap.get(), Ws * 96);
  line("prior_bsize", pbs.get(), Ws * 40);
  line("prior_bidx", pbi.get(), Ws * 40);
  line("prior_bxoff", pbx.get(), Ws * 40);
  line("prior_bstate", pbst.get(), Ws * 40);
  line("prior_x0", px0.get(), Ws * 280);
  for (int w = 0; w < W; ++w) {   // (only n x n / n of a window with a prior is written)
    const size_t n = (size_t)P.wins[w].prior_n;
    printf("J0_%d", w); line("", J0.get() + (size_t)w * 96 * 96, n * n);
    printf("r0_%d", w); line("", r0.get() + (size_t)w * 96, n);
  }
  for (vilo_window_file &f : files) vilo_window_free(&f);
  return 0;
}
