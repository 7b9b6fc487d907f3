// tests/test_dead_reckon.py compiles this with the address and undefined-behaviour sanitizers and runs it: the host half of
// vilo_batch_dead_reckon that needs no device (cerberus_amd/csrc/deadreckon_host.hpp) on a CPU. The argument checks accept what the
// header of include/vilo_gpu.h allows and name everything else; they read offsets[0 .. W] and nothing more (the arrays here are heap
// blocks of exactly that size). The step offsets are max(0, n - 1) per range. The packing reads dt, acc, gyr of exactly n samples and
// writes exactly 7 n doubles. The blocks of the call lie as vilo::CallLayout lays them, host staging and device memory alike. Prints what
// fails; exit status 0: nothing did.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../cerberus_amd/csrc/batch_call.hpp"
#include "../../cerberus_amd/csrc/deadreckon_host.hpp"
#include "../../cerberus_amd/csrc/sample_stream.hpp"

namespace {

int bad = 0;

void expect(bool ok, const char *what) {
  if (!ok) { printf("failed: %s\n", what); ++bad; }
}

vilo_dead_reckon_opts opts(int from_frame, int write) {
  vilo_dead_reckon_opts o;
  o.from_frame = from_frame;
  o.write = write;
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
    std::vector<double> out(10 * W);
    expect(!dead_reckon_check(opts(-1, 0), W, s.data(), off.data(), out.data()), "defaults pass");
    expect(!dead_reckon_check(opts(0, 1), W, s.data(), off.data(), out.data()), "write with frame 0 passes");
    expect(!dead_reckon_check(opts(VILO_MAX_FRAMES - 1, 0), W, s.data(), off.data(), out.data()), "the last frame passes");
    expect(!dead_reckon_check(opts(VILO_MAX_FRAMES - 1, 1), W, s.data(), off.data(), out.data()), "write from the last frame is a status, not an argument error");
    expect(dead_reckon_check(opts(-2, 0), W, s.data(), off.data(), out.data()) != nullptr, "from_frame -2");
    expect(dead_reckon_check(opts(VILO_MAX_FRAMES, 0), W, s.data(), off.data(), out.data()) != nullptr, "from_frame VILO_MAX_FRAMES");
    expect(dead_reckon_check(opts(3, 2), W, s.data(), off.data(), out.data()) != nullptr, "write 2");
    expect(dead_reckon_check(opts(3, -1), W, s.data(), off.data(), out.data()) != nullptr, "write -1");
    expect(dead_reckon_check(opts(-1, 1), W, s.data(), off.data(), out.data()) != nullptr, "write without a frame");
    expect(dead_reckon_check(opts(-1, 0), W, s.data(), nullptr, out.data()) != nullptr, "NULL offsets");
    expect(dead_reckon_check(opts(-1, 0), W, s.data(), off.data(), nullptr) != nullptr, "NULL state_out");
    expect(dead_reckon_check(opts(-1, 0), W, nullptr, off.data(), out.data()) != nullptr, "NULL samples with samples to read");
    std::vector<int32_t> o1 = {1, 1, 2, 3, 33};
    expect(dead_reckon_check(opts(-1, 0), W, s.data(), o1.data(), out.data()) != nullptr, "offsets[0] != 0");
    std::vector<int32_t> o2 = {0, 2, 1, 3, 33};
    expect(dead_reckon_check(opts(-1, 0), W, s.data(), o2.data(), out.data()) != nullptr, "offsets decrease");
    std::vector<int32_t> o3 = {0, 3, 3, 3, 2};
    expect(dead_reckon_check(opts(-1, 0), W, s.data(), o3.data(), out.data()) != nullptr, "the last offset decreases");
    const std::vector<int32_t> none = {0, 0, 0};
    expect(!dead_reckon_check(opts(-1, 0), 2, nullptr, none.data(), out.data()), "no samples at all: samples may be NULL");
    expect(!dead_reckon_check(opts(-1, 0), 0, nullptr, nullptr, nullptr), "no windows: nothing to check but the options");
    expect(dead_reckon_check(opts(-1, 1), 0, nullptr, nullptr, nullptr) != nullptr, "no windows: the options are checked all the same");

    // ---- the step offsets ----
    std::vector<int32_t> step(W + 1, -7);
    expect(dead_reckon_step_offsets(W, off.data(), step.data()) == 30, "30 steps in all");
    expect(step == std::vector<int32_t>({0, 0, 0, 1, 30}), "step offsets 0 0 0 1 30");
    std::vector<int32_t> one(1, -7);
    expect(dead_reckon_step_offsets(0, off.data(), one.data()) == 0 && one[0] == 0, "no windows: one offset");
  }
  // ---- the packing ----
  {
    const size_t n = 37;
    std::vector<vilo_sample> s(n);
    for (size_t i = 0; i < n; ++i) {
      double *d = (double *)&s[i];
      for (int k = 0; k < 35; ++k) d[k] = 100.0 * (double)i + k;
    }
    std::vector<double> rows(DR_ROW * n, -1.0);
    dead_reckon_pack(s.data(), n, rows.data());
    bool ok = true;
    for (size_t i = 0; i < n; ++i)
      for (int k = 0; k < DR_ROW; ++k) ok = ok && rows[DR_ROW * i + k] == 100.0 * (double)i + k;   // dt acc gyr are doubles 0 .. 6
    expect(ok, "a packed row is dt, acc, gyr");
    expect(offsetof(vilo_sample, acc) == 8 && offsetof(vilo_sample, gyr) == 32 && sizeof(vilo_sample) == 280, "vilo_sample's layout");
    dead_reckon_pack(nullptr, 0, nullptr);   // nothing to pack: nothing is touched
    // a part of the array: the samples before and after are not read (their own heap block, so that a stray read would be caught)
    std::vector<vilo_sample> part(s.begin() + 5, s.begin() + 8);
    std::vector<double> three(DR_ROW * 3);
    dead_reckon_pack(part.data(), 3, three.data());
    expect(three[0] == 500.0 && three[DR_ROW * 2 + 6] == 706.0, "three samples");
  }
  // ---- the call's blocks: packed samples | offsets | step offsets | states | trajectory | records, at W = 1 without samples, at a small
  // odd shape and at W = 32768 with 30 samples each ----
  for (int c = 0; c < 3; ++c) {
    const size_t W = c == 0 ? 1 : (c == 1 ? 5 : 32768), n_s = c == 0 ? 0 : (c == 1 ? 33 : 30 * W), n_rows = c == 0 ? 0 : (c == 1 ? 29 : 29 * W);
    for (int traj = 0; traj < 2; ++traj) {
      CallLayout dev, host;
      const size_t o_s = dev.take<double>(DR_ROW * n_s), o_o = dev.take<int32_t>(W + 1), o_t = dev.take<int32_t>(W + 1);
      const size_t o_x = dev.take<double>(DR_STATE * W), o_j = dev.take<double>(DR_STATE * n_rows, traj != 0), o_c = dev.take<vilo_window_dead_reckon_record>(W);
      const size_t h_s = host.take<double>(DR_ROW * n_s), h_o = host.take<int32_t>(W + 1), h_t = host.take<int32_t>(W + 1);
      expect(o_s == 0 && h_s == 0 && o_o == h_o && o_t == h_t && host.bytes() == o_x, "the staging is laid out as the device blocks it goes to");
      const size_t offs[6] = {o_s, o_o, o_t, o_x, o_j, o_c};
      const size_t size[6] = {8 * DR_ROW * n_s, 4 * (W + 1), 4 * (W + 1), 8 * DR_STATE * W, traj ? 8 * DR_STATE * n_rows : 0, 8 * W};
      size_t end = 0;
      for (int i = 0; i < 6; ++i) {
        expect(offs[i] % 256 == 0 && offs[i] == end, "a block starts where the one before it ends, on a multiple of 256");
        end = offs[i] + (size[i] + 255) / 256 * 256;
      }
      expect(dev.bytes() == end, "the total");
      expect(o_j % 16 == 0 && (8 * DR_STATE) % 16 == 0, "trajectory rows are 16-byte aligned");
    }
  }
  if (bad) return 1;
  printf("ok\n");
  return 0;
}
