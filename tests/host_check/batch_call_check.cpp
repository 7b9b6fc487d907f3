// tests/test_batch_call.py compiles this with the address and undefined-behaviour sanitizers and runs it: the layout builder of the batch
// calls (vilo::CallLayout, cerberus_amd/csrc/batch_call.hpp) on a CPU. Every block's offset is a multiple of 256; the blocks lie in the
// order they were taken and do not overlap; a block that is not wanted, or empty, takes no bytes; the total is the sum of the blocks
// rounded up one by one (worked out here by division, not by the builder's mask). Prints what fails; exit status 0: nothing did.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../cerberus_amd/csrc/batch_call.hpp"
#include "../../include/vilo_gpu.h"

namespace {

struct Block { size_t off, bytes; };   // bytes 0: not wanted, or empty

struct Case {
  const char *name;
  vilo::CallLayout lay;
  std::vector<Block> blocks;
  template <class T>
  void take(size_t count, bool want = true) { blocks.push_back({lay.take<T>(count, want), want ? sizeof(T) * count : 0}); }
  int check() const {
    int bad = 0;
    size_t end = 0;   // where the blocks so far end, rounded up
    for (size_t i = 0; i < blocks.size(); ++i) {
      const Block &b = blocks[i];
      if (b.off % 256 != 0) { printf("%s: block %zu at %zu: not a multiple of 256\n", name, i, b.off); ++bad; }
      if (b.off != end) { printf("%s: block %zu at %zu, the blocks before it end at %zu\n", name, i, b.off, end); ++bad; }
      end = b.off + (b.bytes + 255) / 256 * 256;
    }
    if (lay.bytes() != end) { printf("%s: total %zu, the blocks end at %zu\n", name, lay.bytes(), end); ++bad; }
    return bad;
  }
};

struct Rec48 { char c[48]; };
struct Rec24 { char c[24]; };

// the blocks of a gradient-like call: records, two state arrays, two landmark arrays (empty without landmarks), an output not asked for
Case query(const char *name, size_t W, size_t n_lm, bool optional) {
  Case c{name, {}, {}};
  c.take<Rec48>(W);
  c.take<double>(222 * W);
  c.take<double>(222 * W, optional);
  c.take<double>(n_lm);
  c.take<unsigned char>(n_lm);
  c.take<unsigned char>(n_lm, optional);
  c.take<int>(W);
  return c;
}

// the gyroscope-bias alignment's: steps, records, and the copies of the batch's preintegration records and force filters
Case gyro(const char *name, size_t W, bool copies, bool filters) {
  Case c{name, {}, {}};
  c.take<double>(3 * W);
  c.take<Rec24>(W);
  c.take<vilo_preint>(10 * W, copies);
  c.take<double>(36 * 10 * W, copies && filters);
  return c;
}

}  // namespace

int main() {
  int bad = 0;
  const size_t W = 32768, n_lm = 6500000;
  bad += query("W 1, no landmarks", 1, 0, true).check();
  bad += query("W 1, no landmarks, nothing optional", 1, 0, false).check();
  bad += query("W 3, 7 landmarks", 3, 7, true).check();
  bad += query("W 32768, 6.5 M landmarks", W, n_lm, true).check();
  bad += gyro("gyro, no copies", W, false, true).check();
  bad += gyro("gyro, record copies", W, true, false).check();
  bad += gyro("gyro, record and filter copies", W, true, true).check();
  {
    // the totals, spelled out: one window without landmarks is four blocks of one granule (48, 4 bytes) and of 1776 bytes
    const size_t t = query("", 1, 0, true).lay.bytes();
    if (t != 256 + 2 * 1792 + 256) { printf("W 1, no landmarks: total %zu\n", t); ++bad; }
    const size_t u = query("", 1, 0, false).lay.bytes();
    if (u != 256 + 1792 + 256) { printf("W 1, no landmarks, nothing optional: total %zu\n", u); ++bad; }
    // the record copies alone are past 4 GiB: the offsets behind them need all of size_t
    const size_t rec = sizeof(vilo_preint) * 10 * W, head = 3 * 8 * W + 24 * W;   // (both heads are multiples of 256 at this W)
    if (rec <= ((size_t)1 << 32)) { printf("gyro: the record copies take %zu bytes, not more than 4 GiB\n", rec); ++bad; }
    const Case g = gyro("", W, true, true);
    const size_t want = head + (rec + 255) / 256 * 256 + 8 * 36 * 10 * W;
    if (g.lay.bytes() != want) { printf("gyro, record and filter copies: total %zu, expected %zu\n", g.lay.bytes(), want); ++bad; }
    if (g.blocks[3].off != head + (rec + 255) / 256 * 256) { printf("gyro: the filter copies lie at %zu\n", g.blocks[3].off); ++bad; }
    const Case q = query("", W, n_lm, true);
    const size_t lm8 = (8 * n_lm + 255) / 256 * 256, lm1 = (n_lm + 255) / 256 * 256;
    const size_t want_q = 48 * W + 2 * 8 * 222 * W + lm8 + 2 * lm1 + 4 * W;
    if (q.lay.bytes() != want_q) { printf("W 32768, 6.5 M landmarks: total %zu, expected %zu\n", q.lay.bytes(), want_q); ++bad; }
  }
  if (bad) return 1;
  printf("ok\n");
  return 0;
}
