// TEST INFRASTRUCTURE: the full batch's IMU linearisation (k_imu_raw + k_imu_linearize, cerberus_amd/csrc/kernels_solve.hip) emulated on
// the host with the product's own inline functions (cerberus_amd/csrc/factors.hpp): k_imu_raw's entry-major block pools over a batch of NF
// factors, the pair kernel's staging of two heads and two pools (IMU_STG_HEAD / IMU_STG_POOL, a lane's two 16-byte pool loads and two
// head loads per factor) and every lane's 24 operands through the shared helper (imu_lane_gather_load + imu_gather_operands). The result is
// the 32 x 48 operand image [J | r] of both factors of the pair, to be compared bit for bit with what imu_leg_raw / imu_raw write.
// Built as a shared library for tests/test_imu_pool_form.py, and with -DIMU_POOL_CHECK_MAIN as a stand-alone program (sanitizer builds).
#include <cmath>
#include <cstdio>
#include <vector>

#include "../../cerberus_amd/csrc/factors.hpp"
#include "../../include/vilo_gpu.h"

using namespace vilo;

namespace {
const ImuLaneGather g_lane[2] = {imu_lane_gather_table(false), imu_lane_gather_table(true)};

// heads: the NF records' heads; x: per factor [pose_i 7 | sb_i 9 | lb_i 4 | pose_j 7 | sb_j 9 | lb_j 4]. out: [2][32 * 48] of pair p.
void pair_image(int NF, int p, const PreintHead *heads, const double *x, int leg, double g_norm, double *out) {
  // k_imu_raw: one thread per factor, the whole batch (every other factor's entries lie between this pair's)
  std::vector<double> pool((size_t)IB_N * NF, std::nan(""));
  for (int f = 0; f < NF; ++f) {
    const double *s = x + 40 * (size_t)f;
    imu_blocks(heads[f], g_norm, leg != 0, s, s + 7, s + 16, s + 20, s + 27, s + 36, pool.data() + f, (size_t)NF);
  }
  // k_imu_linearize: the staging of pair p, lane by lane
  const int f0 = 2 * p;
  std::vector<double> lds(32 * 48, std::nan(""));
  for (int lane = 0; lane < 64; ++lane) {
    for (int h = 0; h < 2; ++h) {
      const double *hsrc = (const double *)&heads[f0 + h];
      lds[IMU_STG_HEAD(h) + lane] = hsrc[lane];
      lds[IMU_STG_HEAD(h) + 64 + lane] = (lane + 64 < 126) ? hsrc[lane + 64] : 0.0;
    }
    const double *p0 = pool.data() + (size_t)lane * NF + f0;   // the 16-byte load: both factors' entry `lane`
    lds[IMU_STG_POOL(0) + lane] = p0[0]; lds[IMU_STG_POOL(1) + lane] = p0[1];
    if (lane + 64 < IB_N) {
      const double *p1 = pool.data() + (size_t)(lane + 64) * NF + f0;
      lds[IMU_STG_POOL(0) + 64 + lane] = p1[0]; lds[IMU_STG_POOL(1) + 64 + lane] = p1[1];
    }
  }
  for (int h = 0; h < 2; ++h)
    for (int lane = 0; lane < 64; ++lane) {
      const int lr = lane & 15, lk = lane >> 4;
      unsigned gw[IMU_LANE_WORDS];
      double bv[8][3];
      imu_lane_gather_load(g_lane[leg ? 1 : 0], lane, gw);
      imu_gather_operands(gw, lds.data() + IMU_STG_HEAD(h), lds.data() + IMU_STG_POOL(h), bv);
      for (int kk = 0; kk < 8; ++kk)
        for (int J = 0; J < 3; ++J) out[(size_t)h * 32 * 48 + (4 * kk + lk) * 48 + 16 * J + lr] = bv[kk][J];
    }
}
}  // namespace

extern "C" {
// pre / pre_imu: NF records each (the kind `leg` selects is read). x: NF x 40 states. out: [2][32 x 48] row-major, the factors 2 p, 2 p + 1.
void hc_imu_pair_image(int NF, int p, const vilo_preint *pre, const vilo_preint_imu *pre_imu, int leg, double g_norm, const double *x,
                       double *out) {
  std::vector<PreintHead> heads(NF);
  for (int f = 0; f < NF; ++f) {
    if (leg) fill_preint_head(pre[f], heads[f]); else fill_preint_head_imu(pre_imu[f], heads[f]);
  }
  pair_image(NF, p, heads.data(), x, leg, g_norm, out);
}
// The lane-major table against the entry-major one it is built from: 0 when every lane's 24 words name the entries of its operand positions.
int hc_imu_lane_table_mismatches() {
  static const ImuGatherTable tabs[2] = {imu_gather_table(false), imu_gather_table(true)};
  int bad = 0;
  for (int leg = 0; leg < 2; ++leg)
    for (int lane = 0; lane < 64; ++lane)
      for (int i = 0; i < 24; ++i) {
        const unsigned g = (g_lane[leg].w[lane * IMU_LANE_WORDS + i / 2] >> (16 * (i & 1))) & 0xffffu;
        if (g != tabs[leg].e[(4 * (i / 3) + (lane >> 4)) * 48 + 16 * (i % 3) + (lane & 15)]) ++bad;
      }
  return bad;
}
}

#ifdef IMU_POOL_CHECK_MAIN
// Stand-alone: random heads and states for NF factors, every pair's image of both factor kinds against imu_leg_raw / imu_raw, entry by entry (==).
int main() {
  const int NF = 30;
  unsigned long long s = 88172645463325252ULL;
  auto rnd = [&]() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return (double)(s >> 11) / 9007199254740992.0 - 0.5; };
  std::vector<PreintHead> heads(NF);
  std::vector<double> x(40 * (size_t)NF);
  for (int f = 0; f < NF; ++f) {
    double *h = (double *)&heads[f];
    for (int i = 0; i < 126; ++i) h[i] = rnd();
    h[0] = 0.05 + 0.01 * f;
    double *q = heads[f].delta_q, n = 0;
    for (int i = 0; i < 4; ++i) n += q[i] * q[i];
    for (int i = 0; i < 4; ++i) q[i] /= std::sqrt(n);
    double *st = x.data() + 40 * (size_t)f;
    for (int i = 0; i < 40; ++i) st[i] = rnd();
    for (int e = 0; e < 2; ++e) {
      double *qq = st + 20 * e + 3, m = 0;
      for (int i = 0; i < 4; ++i) m += qq[i] * qq[i];
      for (int i = 0; i < 4; ++i) qq[i] /= std::sqrt(m);
    }
  }
  int bad = hc_imu_lane_table_mismatches();
  std::vector<double> img(2 * 32 * 48), want(32 * 48);
  for (int leg = 0; leg < 2; ++leg)
    for (int p = 0; p < NF / 2; ++p) {
      pair_image(NF, p, heads.data(), x.data(), leg, 9.805, img.data());
      for (int h = 0; h < 2; ++h) {
        const int f = 2 * p + h;
        const double *st = x.data() + 40 * (size_t)f;
        double r[31];
        std::fill(want.begin(), want.end(), 0.0);
        if (leg) imu_leg_raw(heads[f], 9.805, st, st + 7, st + 16, st + 20, st + 27, st + 36, r, true, want.data(), 48);
        else imu_raw(heads[f], 9.805, st, st + 7, st + 20, st + 27, r, true, want.data(), 48, 19);
        for (int i = 0; i < (leg ? 31 : 15); ++i) want[i * 48 + 38] = r[i];
        int diff = 0;   // (by value: imu_leg_raw writes -I3 as a block, its off-diagonal -0.0 are structural zeros of the table)
        for (int i = 0; i < 32 * 48; ++i) diff += !(want[i] == img[(size_t)h * 32 * 48 + i]);
        if (diff) {
          ++bad;
          std::printf("factor %d (leg %d): %d entries of the operand image differ\n", f, leg, diff);
        }
      }
    }
  std::printf("imu_pool_check: %d mismatches\n", bad);
  return bad ? 1 : 0;
}
#endif
