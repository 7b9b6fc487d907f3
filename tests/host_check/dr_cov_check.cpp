// tests/test_dr_covariance.py compiles this with the address and undefined-behaviour sanitizers and runs it: the host half of
// vilo_batch_dead_reckon_covariance that needs no device (cerberus_amd/csrc/drcov_host.hpp, with the step offsets and the packing of
// deadreckon_host.hpp as the call uses them) on a CPU. The argument checks accept what the header of include/vilo_gpu.h allows and name
// everything else; they read offsets[0 .. W] and nothing more (the arrays here are heap blocks of exactly that size). The element counts
// are those of the header's arrays, and the blocks of the call lie as vilo::CallLayout lays them, with and without cov_in and the
// trajectory, at W = 1, an odd shape and W = 32768. The noise diagonal is vilo_preintegrate_imu's. Prints what fails; exit status 0:
// nothing did.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../cerberus_amd/csrc/batch_call.hpp"
#include "../../cerberus_amd/csrc/drcov_host.hpp"
#include "../../cerberus_amd/csrc/sample_stream.hpp"

namespace {

int bad = 0;

void expect(bool ok, const char *what) {
  if (!ok) { printf("failed: %s\n", what); ++bad; }
}

vilo_dr_cov_opts opts(int from_frame, int reserved = 0) {
  vilo_dr_cov_opts o;
  o.from_frame = from_frame;
  o.reserved = reserved;
  return o;
}

}  // namespace

int main() {
  using namespace vilo;
  // ---- the argument checks ----
  {
    const std::vector<int32_t> off = {0, 0, 1, 3, 33};   // ranges of 0, 1, 2 and 30 samples
    const int W = 4;
    std::vector<vilo_sample> s(33);
    std::vector<double> st(DR_STATE * W), cov(DRC_N * DRC_N * W);
    expect(!dr_cov_check(opts(-1), W, s.data(), off.data(), st.data(), cov.data()), "defaults pass");
    expect(!dr_cov_check(opts(0), W, s.data(), off.data(), st.data(), cov.data()), "frame 0 passes");
    expect(!dr_cov_check(opts(VILO_MAX_FRAMES - 1), W, s.data(), off.data(), st.data(), cov.data()), "the last frame passes");
    expect(dr_cov_check(opts(-2), W, s.data(), off.data(), st.data(), cov.data()) != nullptr, "from_frame -2");
    expect(dr_cov_check(opts(VILO_MAX_FRAMES), W, s.data(), off.data(), st.data(), cov.data()) != nullptr, "from_frame VILO_MAX_FRAMES");
    expect(dr_cov_check(opts(3, 1), W, s.data(), off.data(), st.data(), cov.data()) != nullptr, "reserved 1");
    expect(dr_cov_check(opts(-1), W, s.data(), nullptr, st.data(), cov.data()) != nullptr, "NULL offsets");
    expect(dr_cov_check(opts(-1), W, s.data(), off.data(), nullptr, cov.data()) != nullptr, "NULL state_out");
    expect(dr_cov_check(opts(-1), W, s.data(), off.data(), st.data(), nullptr) != nullptr, "NULL cov_out");
    expect(dr_cov_check(opts(-1), W, nullptr, off.data(), st.data(), cov.data()) != nullptr, "NULL samples with samples to read");
    std::vector<int32_t> o1 = {1, 1, 2, 3, 33};
    expect(dr_cov_check(opts(-1), W, s.data(), o1.data(), st.data(), cov.data()) != nullptr, "offsets[0] != 0");
    std::vector<int32_t> o2 = {0, 2, 1, 3, 33};
    expect(dr_cov_check(opts(-1), W, s.data(), o2.data(), st.data(), cov.data()) != nullptr, "offsets decrease");
    std::vector<int32_t> o3 = {0, 3, 3, 3, 2};
    expect(dr_cov_check(opts(-1), W, s.data(), o3.data(), st.data(), cov.data()) != nullptr, "the last offset decreases");
    const std::vector<int32_t> none = {0, 0, 0};
    expect(!dr_cov_check(opts(-1), 2, nullptr, none.data(), st.data(), cov.data()), "no samples at all: samples may be NULL");
    expect(!dr_cov_check(opts(-1), 0, nullptr, nullptr, nullptr, nullptr), "no windows: nothing to check but the options");
    expect(dr_cov_check(opts(-2), 0, nullptr, nullptr, nullptr, nullptr) != nullptr, "no windows: the options are checked all the same");
    // the same ranges, the same step offsets as vilo_batch_dead_reckon's: the trajectory rows of the two calls correspond
    std::vector<int32_t> step(W + 1, -7);
    const int32_t n_rows = dead_reckon_step_offsets(W, off.data(), step.data());
    expect(n_rows == 30 && step == std::vector<int32_t>({0, 0, 0, 1, 30}), "step offsets 0 0 0 1 30");
    const DrCovCounts c = dr_cov_counts(W, n_rows);
    expect(c.cov == 225u * W && c.state == 10u * W && c.traj == 36u * 30 && c.rec == (size_t)W, "element counts of four windows, 30 steps");
    const DrCovCounts z = dr_cov_counts(0, 0);
    expect(z.cov == 0 && z.state == 0 && z.traj == 0 && z.rec == 0, "no windows: nothing");
  }
  // ---- the noise diagonal: vilo_preintegrate_imu's (ACC_N on all axes: acc_n_z does not enter) ----
  {
    vilo_config cfg;
    memset(&cfg, 0, sizeof cfg);
    cfg.acc_n = 3.0; cfg.acc_n_z = 1000.0; cfg.gyr_n = 5.0; cfg.acc_w = 7.0; cfg.gyr_w = 11.0;
    double q[DRC_NOISE + 1] = {-1, -1, -1, -1, -1, -1, -1};
    dr_cov_noise(cfg, q);
    expect(q[0] == 9.0 && q[1] == 25.0 && q[2] == 9.0 && q[3] == 25.0 && q[4] == 49.0 && q[5] == 121.0 && q[6] == -1.0, "acc_n^2 gyr_n^2 acc_n^2 gyr_n^2 acc_w^2 gyr_w^2");
  }
  // ---- the call's blocks: packed samples | offsets | step offsets | cov_in | states | covariances | trajectory | records, at W = 1
  // without samples, at a small odd shape and at W = 32768 with 30 samples each ----
  for (int c = 0; c < 3; ++c) {
    const size_t W = c == 0 ? 1 : (c == 1 ? 5 : 32768), n_s = c == 0 ? 0 : (c == 1 ? 33 : 30 * W);
    std::vector<int32_t> off(W + 1), step(W + 1);
    for (size_t w = 0; w <= W; ++w) off[w] = c == 2 ? (int32_t)(30 * w) : (w == W ? (int32_t)n_s : (int32_t)(w < 4 ? w : 3));
    const int32_t n_rows = dead_reckon_step_offsets((int)W, off.data(), step.data());
    expect((size_t)n_rows == (c == 0 ? 0 : (c == 1 ? 29 : 29 * W)), "the steps of the shape");
    const DrCovCounts cnt = dr_cov_counts((int)W, n_rows);
    for (int flags = 0; flags < 4; ++flags) {
      const bool traj = flags & 1, cin = flags & 2;
      CallLayout dev, host;
      const size_t o_s = dev.take<double>(DR_ROW * n_s), o_o = dev.take<int32_t>(W + 1), o_t = dev.take<int32_t>(W + 1);
      const size_t o_i = dev.take<double>(cnt.cov, cin), o_x = dev.take<double>(cnt.state), o_c = dev.take<double>(cnt.cov);
      const size_t o_j = dev.take<double>(cnt.traj, traj), o_r = dev.take<vilo_window_dead_reckon_record>(cnt.rec);
      const size_t h_s = host.take<double>(DR_ROW * n_s), h_o = host.take<int32_t>(W + 1), h_t = host.take<int32_t>(W + 1);
      expect(o_s == 0 && h_s == 0 && o_o == h_o && o_t == h_t && host.bytes() == o_i, "the staging is laid out as the device blocks it goes to");
      const size_t offs[8] = {o_s, o_o, o_t, o_i, o_x, o_c, o_j, o_r};
      const size_t size[8] = {8 * DR_ROW * n_s, 4 * (W + 1), 4 * (W + 1), cin ? 8 * 225 * W : 0, 8 * DR_STATE * W, 8 * 225 * W, traj ? 8 * 36 * (size_t)n_rows : 0, 8 * W};
      size_t end = 0;
      for (int i = 0; i < 8; ++i) {
        expect(offs[i] % 256 == 0 && offs[i] == end, "a block starts where the one before it ends, on a multiple of 256");
        end = offs[i] + (size[i] + 255) / 256 * 256;
      }
      expect(dev.bytes() == end, "the total");
      expect(o_x % 16 == 0 && (8 * DR_STATE) % 16 == 0, "state rows are 16-byte aligned");
    }
    // the packing of exactly the samples the ranges name
    std::vector<vilo_sample> s(n_s);
    for (size_t i = 0; i < n_s; ++i) { s[i].dt = (double)i; s[i].gyr[2] = -(double)i; }
    std::vector<double> rows(DR_ROW * n_s, -1.0);
    dead_reckon_pack(s.data(), n_s, rows.data());
    bool ok = true;
    for (size_t i = 0; i < n_s; ++i) ok = ok && rows[DR_ROW * i] == (double)i && rows[DR_ROW * i + 6] == -(double)i;
    expect(ok, "a packed row is dt, acc, gyr");
  }
  if (bad) return 1;
  printf("ok\n");
  return 0;
}
