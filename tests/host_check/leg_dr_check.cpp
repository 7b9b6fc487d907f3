// tests/test_leg_dead_reckon.py compiles this with the address and undefined-behaviour sanitizers and runs it as a child process: the
// part of vilo_batch_leg_dead_reckon that needs no device (cerberus_amd/csrc/legdr_host.hpp) on a CPU. Without arguments: the argument
// checks, the packing and the call's blocks. With `in out`: the CPU path (leg_dead_reckon_window: legdr_step, the function the kernel
// calls, with the four legs owned by one thread) over the windows of file `in`, results to file `out`; the test compares them with the
// numpy definition (tests/leg_dr_model.py). Both files are plain doubles:
//   in   W, vilo_config (sizeof / 8 doubles, as bytes), then per window: n, pose (7), speed_bias (9), leg_bias (4), samples (35 n)
//   out  per window: status, n_steps, state (32), legs (12), the contact-force filter (36, O_FF layout), trajectory (48 n_steps)
// Prints what fails; exit status 0: nothing did.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../cerberus_amd/csrc/batch_call.hpp"
#include "../../cerberus_amd/csrc/legdr_host.hpp"
#include "../../cerberus_amd/csrc/sample_stream.hpp"

namespace {

int bad = 0;

void expect(bool ok, const char *what) {
  if (!ok) { printf("failed: %s\n", what); ++bad; }
}

vilo_leg_dead_reckon_opts opts(int from_frame, int reserved = 0) {
  vilo_leg_dead_reckon_opts o;
  o.from_frame = from_frame;
  o.reserved = reserved;
  return o;
}

void self_checks() {
  using namespace vilo;
  {
    const std::vector<int32_t> off = {0, 0, 1, 3, 6, 18};   // ranges of 0, 1, 2, 3 and 12 samples
    const int W = 5;
    std::vector<vilo_sample> s(18);
    std::vector<double> st(LEGDR_STATE * W), lg(LEGDR_LEGS * W);
    expect(!leg_dead_reckon_check(opts(-1), W, s.data(), off.data(), st.data(), lg.data()), "defaults pass");
    expect(!leg_dead_reckon_check(opts(0), W, s.data(), off.data(), st.data(), lg.data()), "frame 0 passes");
    expect(!leg_dead_reckon_check(opts(VILO_MAX_FRAMES - 1), W, s.data(), off.data(), st.data(), lg.data()), "the last frame passes");
    expect(leg_dead_reckon_check(opts(-2), W, s.data(), off.data(), st.data(), lg.data()) != nullptr, "from_frame -2");
    expect(leg_dead_reckon_check(opts(VILO_MAX_FRAMES), W, s.data(), off.data(), st.data(), lg.data()) != nullptr, "from_frame VILO_MAX_FRAMES");
    expect(leg_dead_reckon_check(opts(-1, 1), W, s.data(), off.data(), st.data(), lg.data()) != nullptr, "reserved 1");
    expect(leg_dead_reckon_check(opts(-1), W, s.data(), nullptr, st.data(), lg.data()) != nullptr, "NULL offsets");
    expect(leg_dead_reckon_check(opts(-1), W, s.data(), off.data(), nullptr, lg.data()) != nullptr, "NULL state_out");
    expect(leg_dead_reckon_check(opts(-1), W, s.data(), off.data(), st.data(), nullptr) != nullptr, "NULL legs_out");
    expect(leg_dead_reckon_check(opts(-1), W, nullptr, off.data(), st.data(), lg.data()) != nullptr, "NULL samples with samples to read");
    std::vector<int32_t> o1 = {1, 1, 2, 3, 6, 18};
    expect(leg_dead_reckon_check(opts(-1), W, s.data(), o1.data(), st.data(), lg.data()) != nullptr, "offsets[0] != 0");
    std::vector<int32_t> o2 = {0, 2, 1, 3, 6, 18};
    expect(leg_dead_reckon_check(opts(-1), W, s.data(), o2.data(), st.data(), lg.data()) != nullptr, "offsets decrease");
    std::vector<int32_t> o3 = {0, 3, 3, 3, 3, 2};
    expect(leg_dead_reckon_check(opts(-1), W, s.data(), o3.data(), st.data(), lg.data()) != nullptr, "the last offset decreases");
    const std::vector<int32_t> none = {0, 0, 0};
    expect(!leg_dead_reckon_check(opts(-1), 2, nullptr, none.data(), st.data(), lg.data()), "no samples at all: samples may be NULL");
    expect(!leg_dead_reckon_check(opts(-1), 0, nullptr, nullptr, nullptr, nullptr), "no windows: nothing to check but the options");
    expect(leg_dead_reckon_check(opts(-2), 0, nullptr, nullptr, nullptr, nullptr) != nullptr, "no windows: the options are checked all the same");
    std::vector<int32_t> step(W + 1, -7);
    expect(dead_reckon_step_offsets(W, off.data(), step.data()) == 14, "14 steps in all");
    expect(step == std::vector<int32_t>({0, 0, 0, 1, 3, 14}), "step offsets 0 0 0 1 3 14");
  }
  // the packing: dt acc gyr, then per leg phi dphi c; exactly n samples read and 35 n doubles written
  {
    const size_t n = 9;
    std::vector<vilo_sample> s(n);
    for (size_t i = 0; i < n; ++i) {
      double *d = (double *)&s[i];
      for (int k = 0; k < 35; ++k) d[k] = 100.0 * (double)i + k;
    }
    std::vector<double> rows(LEGDR_ROW * n, -1.0);
    leg_dead_reckon_pack(s.data(), n, rows.data());
    bool ok = true;
    for (size_t i = 0; i < n; ++i) {
      const double *r = rows.data() + LEGDR_ROW * i, b = 100.0 * (double)i;
      for (int k = 0; k < 7; ++k) ok = ok && r[k] == b + k;
      for (int j = 0; j < 4; ++j)
        for (int k = 0; k < 3; ++k) ok = ok && r[7 + 7 * j + k] == b + 7 + 3 * j + k && r[7 + 7 * j + 3 + k] == b + 19 + 3 * j + k;
      for (int j = 0; j < 4; ++j) ok = ok && r[7 + 7 * j + 6] == b + 31 + j;
    }
    expect(ok, "a packed row is dt acc gyr, then leg j's phi dphi c");
    expect(sizeof(vilo_sample) == 8 * LEGDR_ROW && offsetof(vilo_sample, phi) == 56 && offsetof(vilo_sample, dphi) == 152 && offsetof(vilo_sample, c) == 248,
           "vilo_sample's layout");
    leg_dead_reckon_pack(nullptr, 0, nullptr);
    std::vector<vilo_sample> part(s.begin() + 2, s.begin() + 5);
    std::vector<double> three(LEGDR_ROW * 3);
    leg_dead_reckon_pack(part.data(), 3, three.data());
    expect(three[0] == 200.0 && three[LEGDR_ROW * 2 + 34] == 434.0, "three samples");
  }
  // the call's blocks: packed samples | offsets | step offsets | states | legs | trajectory | records
  for (int c = 0; c < 3; ++c) {
    const size_t W = c == 0 ? 1 : (c == 1 ? 5 : 32768), n_s = c == 0 ? 0 : (c == 1 ? 18 : 30 * W), n_rows = c == 0 ? 0 : (c == 1 ? 14 : 29 * W);
    for (int traj = 0; traj < 2; ++traj) {
      CallLayout dev, host;
      const size_t o_s = dev.take<double>(LEGDR_ROW * n_s), o_o = dev.take<int32_t>(W + 1), o_t = dev.take<int32_t>(W + 1);
      const size_t o_x = dev.take<double>(LEGDR_STATE * W), o_l = dev.take<double>(LEGDR_LEGS * W);
      const size_t o_j = dev.take<double>(LEGDR_TRAJ * n_rows, traj != 0), o_c = dev.take<vilo_window_leg_dead_reckon_record>(W);
      const size_t h_s = host.take<double>(LEGDR_ROW * n_s), h_o = host.take<int32_t>(W + 1), h_t = host.take<int32_t>(W + 1);
      expect(o_s == 0 && h_s == 0 && o_o == h_o && o_t == h_t && host.bytes() == o_x, "the staging is laid out as the device blocks it goes to");
      const size_t offs[7] = {o_s, o_o, o_t, o_x, o_l, o_j, o_c};
      const size_t size[7] = {8 * LEGDR_ROW * n_s, 4 * (W + 1), 4 * (W + 1), 8 * LEGDR_STATE * W, 8 * LEGDR_LEGS * W, traj ? 8 * LEGDR_TRAJ * n_rows : 0, 8 * W};
      size_t end = 0;
      for (int i = 0; i < 7; ++i) {
        expect(offs[i] % 256 == 0 && offs[i] == end, "a block starts where the one before it ends, on a multiple of 256");
        end = offs[i] + (size[i] + 255) / 256 * 256;
      }
      expect(dev.bytes() == end, "the total");
    }
  }
}

int run_file(const char *in_path, const char *out_path) {
  using namespace vilo;
  FILE *fi = fopen(in_path, "rb");
  if (!fi) { printf("failed: cannot read %s\n", in_path); return 1; }
  std::vector<double> in;
  double buf[4096];
  size_t got;
  while ((got = fread(buf, sizeof(double), 4096, fi)) > 0) in.insert(in.end(), buf, buf + got);
  fclose(fi);
  constexpr size_t CFG_N = sizeof(vilo_config) / sizeof(double);
  static_assert(sizeof(vilo_config) % sizeof(double) == 0, "vilo_config is a whole number of doubles");
  if (in.size() < 1 + CFG_N) { printf("failed: short input\n"); return 1; }
  const int W = (int)in[0];
  vilo_config cfg;
  memcpy(&cfg, in.data() + 1, sizeof(cfg));
  size_t at = 1 + CFG_N;
  std::vector<double> out;
  for (int w = 0; w < W; ++w) {
    if (at + 21 > in.size()) { printf("failed: short input at window %d\n", w); return 1; }
    const int n = (int)in[at];
    const double *pose = in.data() + at + 1, *sb = pose + 7, *lb = sb + 9;
    at += 21;
    if (n < 0 || at + (size_t)35 * n > in.size()) { printf("failed: short input at window %d\n", w); return 1; }
    // the samples as the caller's vilo_sample array (a heap block of their own: a stray read is caught), packed as the call packs them
    std::vector<vilo_sample> smp(n);
    if (n) memcpy((void *)smp.data(), in.data() + at, sizeof(vilo_sample) * n);
    at += (size_t)35 * n;
    std::vector<double> rows((size_t)LEGDR_ROW * n);
    leg_dead_reckon_pack(smp.data(), n, rows.data());
    const int n_steps = n > 1 ? n - 1 : 0;
    std::vector<double> state(LEGDR_STATE, -1.0), legs(LEGDR_LEGS, -1.0), traj((size_t)LEGDR_TRAJ * n_steps, -1.0), ff(LEGDR_FF_N, -1.0);
    const int status = leg_dead_reckon_window(cfg, pose, sb, lb, rows.data(), n, state.data(), legs.data(), traj.data(), ff.data());
    // without the trajectory: the same state, bit for bit
    std::vector<double> state2(LEGDR_STATE, -1.0), legs2(LEGDR_LEGS, -1.0);
    const int status2 = leg_dead_reckon_window(cfg, pose, sb, lb, rows.data(), n, state2.data(), legs2.data(), nullptr, nullptr);
    expect(status2 == status && !memcmp(state.data(), state2.data(), 8 * LEGDR_STATE) && !memcmp(legs.data(), legs2.data(), 8 * LEGDR_LEGS),
           "with and without the trajectory: the same state_out and legs_out");
    if (status == VILO_DR_OK && n_steps) {
      const double *last = traj.data() + (size_t)LEGDR_TRAJ * (n_steps - 1);
      expect(!memcmp(last + LT_SUM_DT, state.data() + LS_SUM_DT, 8) && !memcmp(last + LT_POS, state.data() + LS_POS, 24) &&
                 !memcmp(last + LT_FLAG, state.data() + LS_FLAG, 32),
             "a window's last trajectory row agrees with its state_out");
    }
    out.push_back(status); out.push_back(n_steps);
    out.insert(out.end(), state.begin(), state.end());
    out.insert(out.end(), legs.begin(), legs.end());
    out.insert(out.end(), ff.begin(), ff.end());
    out.insert(out.end(), traj.begin(), traj.end());
  }
  FILE *fo = fopen(out_path, "wb");
  if (!fo || fwrite(out.data(), sizeof(double), out.size(), fo) != out.size()) { printf("failed: cannot write %s\n", out_path); return 1; }
  fclose(fo);
  return 0;
}

}  // namespace

int main(int argc, char **argv) {
  if (argc == 3) {
    if (run_file(argv[1], argv[2])) return 1;
  } else {
    self_checks();
  }
  if (bad) return 1;
  printf("ok\n");
  return 0;
}
