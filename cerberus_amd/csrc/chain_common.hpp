// The block-tridiagonal Cholesky chain of the speed / leg-bias part by one wave, with its coupling rows handed on through global memory:
//   S_k = A_kk + mu D_k - T_A(k+1)^T T_A(k+1),  L_k = chol(S_k),  M_k = L_k^-1,  T_A(k) = M_k A_{k,k-1},
//   V = [B_k | g_k] - T_A(k+1)^T T(k+1),  T(k) = M_k V   (13 x 80: columns 0..78 coupling rows, column 79 = rhs),  rhs_P -= T_B(k)^T t_g(k)
// for frames F-1 .. 0. The scalar part runs lane = row in the four 16-lane groups; T and V are FP64-MFMA tiles whose accumulator layout
// (register r of lane (lr, lk) = row lk + 4 r, column lr) is the operand layout of the next product — and of C -= T_B(k)^T T_B(k), which
// the caller does from Tout: [frame k][tile X][register kk][lane], tiles left of x_lo(k) neither written nor to be read.
// Used by k_chain_single (kernels_split.hip: two waves per SIMD; the form behind VILO_CHAIN_SINGLE).
//
// The default three-stage form cuts the chain once more (below): S_k, L_k, M_k and T_A(k) depend on nothing but the speed / leg-bias
// blocks, dhat^2 and mu, so k_chain_fact factorises FOUR windows per wave (chain_fact_groups: one window per 16-lane group, lane = row,
// pivots and columns broadcast inside the group by DPP row_newbcast) and k_chain keeps the MFMA recurrence of T (chain_recur_to_global),
// its M_k / T_A(k+1) operands read back from global memory a frame ahead. Entry by entry the arithmetic is chain_to_global's.
#pragma once
#include <type_traits>
#include <utility>
#include "wave_common.hpp"

// scratch (doubles, 704)
#define CH_LM 0         // 13 x 13: M_k = L_k^-1
#define CH_TA0 176
#define CH_TA1 352
#define CH_SN 528       // 13 x 13: S_{k-1} = A_{k-1,k-1} - T_A(k)^T T_A(k)
#define CH_TOTAL 704

__device__ __forceinline__ int chain_x_lo(int k, int kb) { return (k <= kb) ? 0 : max(0, (6 * (k - 1)) >> 4); }   // T(k) is zero left of pose k - 1 (dense from the prior's frame down)

// C -= T_B(k)^T T_B(k) for frames F-1 .. 0 on the pose system's 15 accumulator tiles (solve_wave_body's middle stage, kernels_wave.hip),
// the operands as k_chain left them in Tg ([frame k][tile X][register kk][lane], L2-resident): per frame the tiles (I, J) with
// J >= x_lo(k) in tile order, four kk steps each — k_solve_wave's sequence on the same values, so the tiles agree bitwise.
// The operands of a frame are in flight one frame ahead through unconditional loads with clamped addresses — no load sits under a branch,
// which would cost the compiler its count of loads in flight: the frame index is clamped at 0, a tile left of x_lo (never written) reads
// tile x_lo again, and the padding rows 13 .. 15 (register 3 of lanes beyond the first 16: never written) read row 12's lane group.
// One branch-free form of the MFMAs per x_lo (conditions between the MFMAs of a frame stall the stream). The sign of the A operand is
// flipped by the instruction (neg:[1,0,0], exact) instead of by 20 sign flips per frame in front of the MFMAs.
__device__ __forceinline__ void chain_rank_updates(mfma_d4 (&acc)[15], const double *Tg, int F, int kb, int lane) {
  const int lk = lane >> 4;
  const int lane3 = lk == 0 ? lane : (lane & 15);
  double tb[2][5][4];
  auto ldT = [&](int k, auto selc) {
    constexpr int sel = decltype(selc)::value;
    const int x_lo = chain_x_lo(k, kb);
#pragma unroll
    for (int X = 0; X < 5; ++X) {
      const double *src = Tg + 1280 * k + max(X, x_lo) * 256;
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {
        const double t = src[kk * 64 + (kk < 3 ? lane : lane3)];
        tb[sel][X][kk] = (kk < 3 || lk == 0) ? t : 0.0;   // (rows 13 .. 15: padding)
      }
    }
  };
  auto upd_x = [&](auto selc, auto xc) {
    constexpr int sel = decltype(selc)::value, XLO = decltype(xc)::value;
#pragma unroll
    for (int t = 0; t < 15; ++t) {
      if (c_tJ[t] >= XLO) {
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(tb[sel][c_tI[t]][kk], tb[sel][c_tJ[t]][kk], acc[t], 0, 0, 1);   // neg:[1,0,0]: -A, the sign flipped in the instruction
      }
    }
  };
  auto upd = [&](int k, auto selc) {
    switch (chain_x_lo(k, kb)) {
      case 0: upd_x(selc, std::integral_constant<int, 0>{}); break;
      case 1: upd_x(selc, std::integral_constant<int, 1>{}); break;
      case 2: upd_x(selc, std::integral_constant<int, 2>{}); break;
      default: upd_x(selc, std::integral_constant<int, 3>{}); break;
    }
  };
  std::integral_constant<int, 0> s0;
  std::integral_constant<int, 1> s1;
  ldT(max(F - 1, 0), s0);
  for (int k = F - 1; k >= 0; k -= 2) {
    ldT(max(k - 1, 0), s1);
    upd(k, s0);
    ldT(max(k - 2, 0), s0);
    if (k >= 1) upd(k - 1, s1);
  }
}

// DB / GB: dhat^2 and gradient of the 143 speed / leg-bias dimensions (LDS). Returns 1 when a pivot was not positive.
__device__ __forceinline__ int chain_to_global(const double *bimg, const double *gin, double *scr, const double *DB, const double *GB,
                                               double *Mg, double *TAg, double *Tout, double *vout, int F, int kb, double mu, int lane) {
  const int lr = lane & 15, lk = lane >> 4;
  int fX[5], oX[5];
#pragma unroll
  for (int X = 0; X < 5; ++X) { const int col = 16 * X + lr; fX[X] = col < 66 ? col / 6 : 99; oX[X] = col < 66 ? col - 6 * fX[X] : 0; }
  int fail = 0;
  {
    const int grp = lk, c = lr;
    const int row = c < 13 ? c : 0;
    double *LM = scr + CH_LM, *SN = scr + CH_SN;
    double *TAcur = scr + CH_TA0, *TAprev = scr + CH_TA1;
    mfma_d4 T[5];
    double yr[5];
#pragma unroll
    for (int X = 0; X < 5; ++X) { T[X] = mfma_d4{0.0, 0.0, 0.0, 0.0}; yr[X] = 0.0; }
    // this frame's blocks come from the assembled image one frame ahead of their use (registers nV / nrhs / nadn)
    auto load_blocks = [&](int k, mfma_d4 *Vn, double *rhsn, double *adnn) {
      // [B_k | g_k] in accumulator order: row lk + 4 r, column 16 X + lr (zero rows 13..15 in the image); column 79 carries the gradient
#pragma unroll
      for (int X = 0; X < 5; ++X) {
        const int df = fX[X] - k + 1;
        const bool on = df >= 0 && df <= 2;
        const double *src = bimg + BI_BS + (k * 16 + lk) * 18 + 6 * min(max(df, 0), 2) + oX[X];
#pragma unroll
        for (int r = 0; r < 4; ++r) Vn[X][r] = on ? src[72 * r] : 0.0;
      }
      if (k == kb) {
#pragma unroll
        for (int X = 0; X < 5; ++X)
#pragma unroll
          for (int r = 0; r < 4; ++r) Vn[X][r] += bimg[BI_BP + (lk + 4 * r) * 80 + 16 * X + lr];
      }
#pragma unroll
      for (int i = 0; i < 13; ++i) rhsn[i] = (k > 0) ? bimg[BI_AOT + (max(k - 1, 0) * 13 + row) * 13 + i] : 0.0;   // column `row` of A_{k,k-1}
#pragma unroll
      for (int r = 0; r < 4; ++r) adnn[r] = (k > 0 && lr < 13 && lk + 4 * r < 13) ? bimg[BI_AD + max(k - 1, 0) * 169 + (lk + 4 * r) * 13 + lr] : 0.0;   // A_{k-1,k-1}, accumulator order
    };
    mfma_d4 nV[5];
    double nrhs[13], nadn[4];
    load_blocks(F - 1, nV, nrhs, nadn);
    for (int k = F - 1; k >= 0; --k) {
      const int x_lo = chain_x_lo(k, kb);
      mfma_d4 V[5];
      double a[13], l[13], rhs[13], adn[4];
#pragma unroll
      for (int X = 0; X < 5; ++X) V[X] = nV[X];
#pragma unroll
      for (int i = 0; i < 13; ++i) rhs[i] = nrhs[i];
#pragma unroll
      for (int m = 0; m < 4; ++m) adn[m] = nadn[m];
      if (lr == 15) {
#pragma unroll
        for (int r = 0; r < 4; ++r) V[4][r] = (lk + 4 * r < 13) ? GB[13 * k + lk + 4 * r] : 0.0;
      }
      // S_k (lane = row): the top frame straight from A_kk, later frames from the update left by the previous step
      if (k == F - 1) {
#pragma unroll
        for (int j = 0; j < 13; ++j) a[j] = bimg[BI_AD + (k * 13 + row) * 13 + j];
      } else {
#pragma unroll
        for (int j = 0; j < 13; ++j) a[j] = SN[row * 13 + j];
      }
      {
        const double md = mu * DB[13 * k + row];
#pragma unroll
        for (int j = 0; j < 13; ++j) a[j] += (j == row) ? md : 0.0;
      }
      double myrinv = 1.0;
#pragma unroll
      for (int j = 0; j < 13; ++j) {
        double piv = readlane_d(a[j], j);
        if (!(piv > 0.0) || !isfinite(piv)) { fail = 1; piv = 1.0; }
        const double rinv = rsqrt(piv);
        const double lj = (c == j) ? piv * rinv : (c > j ? a[j] * rinv : 0.0);
        l[j] = lj;
        if (c == j) myrinv = rinv;
#pragma unroll
        for (int q = j + 1; q < 13; ++q) a[q] -= lj * readlane_d(lj, q);
      }
      // forward substitutions L x = rhs: T_A(k) columns (group 0), L^-1 columns (group 1); L broadcast from the owning lanes
      // (opaque copies: see chol16_tile)
#pragma unroll
      for (int j = 0; j < 13; ++j) asm volatile("" : "+v"(l[j]));
      double cl[13];
#pragma unroll
      for (int i = 0; i < 13; ++i) {
        double vv = (grp == 0) ? rhs[i] : ((i == c) ? 1.0 : 0.0);
#pragma unroll
        for (int q = 0; q < i; ++q) vv -= readlane_d(l[q], i) * cl[q];
        cl[i] = vv * readlane_d(myrinv, i);
        asm volatile("" : "+v"(cl[i]));
        __builtin_amdgcn_sched_barrier(0);   // (one row's v_readlane results at a time)
      }
      if (c < 13 && grp < 2) {
        if (grp == 0) {
#pragma unroll
          for (int i = 0; i < 13; ++i) { TAcur[i * 13 + c] = cl[i]; TAg[k * 169 + i * 13 + c] = cl[i]; }
        } else {
#pragma unroll
          for (int i = 0; i < 13; ++i) { LM[i * 13 + c] = cl[i]; Mg[k * 169 + i * 13 + c] = cl[i]; }
        }
      }
      lds_fence();
      // S_{k-1} = A_{k-1,k-1} - T_A(k)^T T_A(k): one 16 x 16 tile on the matrix cores (the operand serves as A and B)
      if (k > 0) {
        mfma_d4 sn = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
          const int q = 4 * kk + lk;
          const double ta = ((lr < 13) && (q < 13)) ? TAcur[min(q, 12) * 13 + min(lr, 12)] : 0.0;
          sn = __builtin_amdgcn_mfma_f64_16x16x4f64(ta, ta, sn, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (lr < 13 && lk + 4 * r < 13) SN[(lk + 4 * r) * 13 + lr] = adn[r] - sn[r];
      }
      // V -= T_A(k+1)^T T(k+1);  T(k) = M_k V
      double at[4], am[4];
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {
        const int q = 4 * kk + lk;
        const bool in = (lr < 13) && (q < 13);
        const double ta = TAprev[min(q, 12) * 13 + min(lr, 12)], m = LM[min(lr, 12) * 13 + min(q, 12)];
        at[kk] = (in && k < F - 1) ? -ta : 0.0;
        am[kk] = in ? m : 0.0;
      }
      if (k < F - 1) {
#pragma unroll
        for (int X = 0; X < 5; ++X)
          if (X >= x_lo) {
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) V[X] = __builtin_amdgcn_mfma_f64_16x16x4f64(at[kk], T[X][kk], V[X], 0, 0, 0);
          }
      }
#pragma unroll
      for (int X = 0; X < 5; ++X)
        if (X >= x_lo) {
          mfma_d4 n = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
          for (int kk = 0; kk < 4; ++kk) n = __builtin_amdgcn_mfma_f64_16x16x4f64(am[kk], V[X][kk], n, 0, 0, 0);
          T[X] = n;
        }
      // the next frame's blocks: in flight behind the rank update below (V, rhs and adn of this frame are dead)
      if (k > 0) load_blocks(k - 1, nV, nrhs, nadn);
      // t_g(k) (column 79) to every lane of its 16-lane row group; the pose system must not see it
      mfma_d4 T4 = T[4];
      double tg[4];
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {
        tg[kk] = __shfl(T[4][kk], (lane & 48) | 15, 64);
        if (lr == 15) T4[kk] = 0.0;
      }
      // T_B(k) out in operand order (tiles left of x_lo are zero and skipped on both sides): the middle stage's C -= T_B^T T_B;
      // rhs_P -= T_B^T t_g here
      {
        double *Tb = Tout + 1280 * k;
#pragma unroll
        for (int X = 0; X < 5; ++X)
          if (X >= x_lo) {
#pragma unroll
            for (int kk = 0; kk < 4; ++kk)
              if (kk < 3 || lk == 0) Tb[(X * 4 + kk) * 64 + lane] = (X == 4) ? T4[kk] : T[X][kk];   // (rows 13 .. 15 of the 16: padding, never read)
          }
      }
#pragma unroll
      for (int X = 0; X < 5; ++X)
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) yr[X] += ((X == 4) ? T4[kk] : T[X][kk]) * tg[kk];
      double *sw = TAcur; TAcur = TAprev; TAprev = sw;
      lds_fence();
    }
    // reduced right-hand side so far: g_P - sum_k T_B^T t_g
#pragma unroll
    for (int X = 0; X < 5; ++X) {
      yr[X] += __shfl_xor(yr[X], 16, 64);
      yr[X] += __shfl_xor(yr[X], 32, 64);
      if (lk == 0) vout[16 * X + lr] = gin[16 * X + lr] - yr[X];
    }
  }
  return fail;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// The factorisation on its own, and the recurrence that reads it back.

// fn(std::integral_constant<int, 0>{}) .. fn(std::integral_constant<int, N - 1>{}): a loop whose index is a constant expression (a DPP
// lane pattern is an immediate of the instruction)
template <class Fn, int... I>
__device__ __forceinline__ void chain_static_for(Fn &&fn, std::integer_sequence<int, I...>) { (fn(std::integral_constant<int, I>{}), ...); }
template <int N, class Fn>
__device__ __forceinline__ void chain_static_for(Fn &&fn) { chain_static_for(fn, std::make_integer_sequence<int, N>{}); }

// How lane SRC's value of a problem reaches the problem's other lanes: the broadcast policy of chain_factor_frame. BcRow16: one problem
// per 16-lane group (DPP row_newbcast: lane SRC of every row of 16 to the lanes of that row, no LDS round trip). chain_to_global and
// k_solve_wave keep their own inline text with v_readlane (one problem per wave, the two substitutions shared out over two groups): they
// are the forms this one is compared against, bit for bit and in time, and are left as they were measured.
struct BcRow16 {
  template <int SRC> static __device__ __forceinline__ double at(double v) { return dpp_move_d<0x150 + SRC, 0xf>(v); }
};

// One frame of the chain's scalar part, lane c = row c of the problem BC serves: L = chol(S) (a: row c of S in, destroyed), then both
// forward substitutions with L — clT: column c of T_A(k) = L^-1 rhs (rhs: column c of A_{k,k-1}), clM: column c of M_k = L^-1. The pivot
// sequence, the order of the multiply-adds and the contraction are chain_to_global's, where two groups of a wave take a substitution
// each. Branch-free: lanes of different problems go through it together. Returns 1 where the lane's problem met a pivot that was not
// positive and finite. between(): called once the factor stands, before the substitutions (loads whose registers the factorisation needs).
template <class BC, class Between>
__device__ __forceinline__ int chain_factor_frame(double (&a)[13], const double (&rhs)[13], int c, double (&clT)[13], double (&clM)[13], Between &&between) {
  int fail = 0;
  double l[13], myrinv = 1.0;
  chain_static_for<13>([&](auto jc) {
    constexpr int j = decltype(jc)::value;
    double piv = BC::template at<j>(a[j]);
    const bool bad = !(piv > 0.0) || !isfinite(piv);
    fail |= bad ? 1 : 0;
    piv = bad ? 1.0 : piv;
    const double rinv = rsqrt(piv);
    const double lj = (c == j) ? piv * rinv : (c > j ? a[j] * rinv : 0.0);
    l[j] = lj;
    myrinv = (c == j) ? rinv : myrinv;
    chain_static_for<12 - j>([&](auto qc) {
      constexpr int q = j + 1 + decltype(qc)::value;
      a[q] -= lj * BC::template at<q>(lj);
    });
  });
  // (opaque copies and one row's broadcasts at a time, as in chol16_tile: the broadcasts depend on nothing the substitution changes and
  // would all be emitted up front)
#pragma unroll
  for (int j = 0; j < 13; ++j) asm volatile("" : "+v"(l[j]));
  between();
  chain_static_for<13>([&](auto ic) {
    constexpr int i = decltype(ic)::value;
    double vT = rhs[i], vM = (i == c) ? 1.0 : 0.0;
    chain_static_for<i>([&](auto qc) {
      constexpr int q = decltype(qc)::value;
      const double liq = BC::template at<i>(l[q]);
      vT -= liq * clT[q];
      vM -= liq * clM[q];
    });
    const double ri = BC::template at<i>(myrinv);
    clT[i] = vT * ri;
    clM[i] = vM * ri;
    asm volatile("" : "+v"(clT[i]), "+v"(clM[i]));
    __builtin_amdgcn_sched_barrier(0);
  });
  return fail;
}

#define CHF_WIN 176           // doubles of LDS per window: T_A(k) while S_{k-1} is formed, then S_{k-1} in its place
#define CHF_TOTAL (4 * CHF_WIN)

// Windows first_win .. first_win + 3 by one wave, window g in the 16-lane group g: S_k, L_k, M_k, T_A(k) for frames F-1 .. 0, M_k to
// b.Lk and T_A(k) to b.TAg where chain_to_global writes them, SolverState::pad[1] = 1 / 0 (a pivot was not positive). The frame loop
// runs over the longest window of the four with the frame index shared: a window of fewer frames joins at its own top frame, a group
// whose window is finished, keeps its linearisation or does not exist computes on whatever lies there and stores nothing. Nothing in the
// loop branches on a group's condition: such a group reads uninitialised LDS and rows of Bimg no assembly wrote, so NaN and Inf may run
// through its lanes, but every store (LDS, Lk, TAg, pad[1]) and the fail flag are under the group's own `live` / `act`, a broadcast
// never leaves its row of 16, and the MFMA tiles are per window: nothing of it reaches a live window or memory. S_{k-1} = A_{k-1,k-1} - T_A(k)^T T_A(k) stays the one MFMA tile per window it is in
// chain_to_global (the same instruction on the same operands), window after window.
__device__ __forceinline__ void chain_fact_groups(const BatchDev &b, int first_win, double *scr, int lane) {
  const int c = lane & 15, grp = lane >> 4, lr = c, lk = grp;
  const int row = c < 13 ? c : 0;
  // every lane knows all four windows (wave-uniform), and its own
  int Fw[4], actw[4];
  const double *adw[4];
  int Fmax = 0;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    const int win = min(first_win + w, b.W - 1);
    const SolverState &sw = b.st[win];
    actw[w] = (first_win + w < b.W) && !sw.done && sw.need_lin;
    Fw[w] = b.win[win].n_frames;
    adw[w] = b.Bimg + (size_t)win * BI_N + BI_AD;
    Fmax = max(Fmax, actw[w] ? Fw[w] : 0);
  }
  if (Fmax == 0) return;   // (no live window in the wave)
  const int mywin = min(first_win + grp, b.W - 1);
  SolverState &st = b.st[mywin];
  const bool act = (first_win + grp < b.W) && !st.done && st.need_lin;
  const int F = b.win[mywin].n_frames;
  const double mu = st.mu;
  const double *bimg = b.Bimg + (size_t)mywin * BI_N;
  double *Mg = b.Lk + (size_t)mywin * 11 * 169, *TAg = b.TAg + (size_t)mywin * 11 * 169;
  double *my = scr + CHF_WIN * grp;
  // S of the window's top frame is A_kk itself
  if (act && c < 13) {
#pragma unroll
    for (int j = 0; j < 13; ++j) my[row * 13 + j] = bimg[BI_AD + (max(F - 1, 0) * 13 + row) * 13 + j];
  }
  int fail = 0;
  double nmd = mu * bimg[BI_DH2 + CD_B0 + 13 * (Fmax - 1) + row];
  lds_fence();
  for (int k = Fmax - 1; k >= 0; --k) {
    const bool live = act && k < F;
    const int kp = max(k - 1, 0);
    double a[13], rhs[13], clT[13], clM[13], adn[4][4];
    // column `row` of A_{k,k-1}
#pragma unroll
    for (int i = 0; i < 13; ++i) { const double v = bimg[BI_AOT + (kp * 13 + row) * 13 + i]; rhs[i] = (k > 0) ? v : 0.0; }
    // A_{k-1,k-1} of the four windows in accumulator order: in flight behind the substitutions, in the registers S_k leaves
    auto load_adn = [&]() {
#pragma unroll
      for (int w = 0; w < 4; ++w)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const double v = adw[w][kp * 169 + min(lk + 4 * r, 12) * 13 + min(lr, 12)];
          adn[w][r] = (k > 0 && lr < 13 && lk + 4 * r < 13) ? v : 0.0;
        }
    };
    const double md = nmd;
    nmd = mu * bimg[BI_DH2 + CD_B0 + 13 * kp + row];
#pragma unroll
    for (int j = 0; j < 13; ++j) a[j] = my[row * 13 + j];
#pragma unroll
    for (int j = 0; j < 13; ++j) a[j] += (j == row) ? md : 0.0;
    const int fk = chain_factor_frame<BcRow16>(a, rhs, c, clT, clM, load_adn);
    fail |= live ? fk : 0;
    if (live && c < 13) {
#pragma unroll
      for (int i = 0; i < 13; ++i) { my[i * 13 + c] = clT[i]; TAg[k * 169 + i * 13 + c] = clT[i]; Mg[k * 169 + i * 13 + c] = clM[i]; }
    }
    lds_fence();
    if (k > 0) {
      mfma_d4 sn[4];
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        sn[w] = mfma_d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
          const int q = 4 * kk + lk;
          const double t = scr[CHF_WIN * w + min(q, 12) * 13 + min(lr, 12)];
          const double ta = ((lr < 13) && (q < 13)) ? t : 0.0;
          sn[w] = __builtin_amdgcn_mfma_f64_16x16x4f64(ta, ta, sn[w], 0, 0, 0);
        }
      }
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        const bool livew = actw[w] && k < Fw[w];
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (livew && lr < 13 && lk + 4 * r < 13) scr[CHF_WIN * w + (lk + 4 * r) * 13 + lr] = adn[w][r] - sn[w][r];
      }
      lds_fence();
    }
  }
  if (act && c == 0) st.pad[1] = fail ? 0 : 1;
}

// The T recurrence of chain_to_global alone, for a window k_chain_fact has factorised: the operands M_k and -T_A(k+1) come from Mg / TAg
// in the order the MFMAs take them, one frame ahead of their use (unconditional, clamped loads), the gradient column from gin; no LDS.
__device__ __forceinline__ void chain_recur_to_global(const double *bimg, const double *gin, const double *Mg, const double *TAg, double *Tout,
                                                      double *vout, int F, int kb, int lane) {
  const int lr = lane & 15, lk = lane >> 4;
  int fX[5], oX[5];
#pragma unroll
  for (int X = 0; X < 5; ++X) { const int col = 16 * X + lr; fX[X] = col < 66 ? col / 6 : 99; oX[X] = col < 66 ? col - 6 * fX[X] : 0; }
  mfma_d4 T[5];
  double yr[5];
#pragma unroll
  for (int X = 0; X < 5; ++X) { T[X] = mfma_d4{0.0, 0.0, 0.0, 0.0}; yr[X] = 0.0; }
  auto load_blocks = [&](int k, mfma_d4 *Vn) {
    // [B_k | g_k] in accumulator order: row lk + 4 r, column 16 X + lr (zero rows 13..15 in the image); column 79 carries the gradient
#pragma unroll
    for (int X = 0; X < 5; ++X) {
      const int df = fX[X] - k + 1;
      const bool on = df >= 0 && df <= 2;
      const double *src = bimg + BI_BS + (k * 16 + lk) * 18 + 6 * min(max(df, 0), 2) + oX[X];
#pragma unroll
      for (int r = 0; r < 4; ++r) Vn[X][r] = on ? src[72 * r] : 0.0;
    }
    if (k == kb) {
#pragma unroll
      for (int X = 0; X < 5; ++X)
#pragma unroll
        for (int r = 0; r < 4; ++r) Vn[X][r] += bimg[BI_BP + (lk + 4 * r) * 80 + 16 * X + lr];
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const double gv = gin[CD_B0 + 13 * k + min(lk + 4 * r, 12)];
      if (lr == 15) Vn[4][r] = (lk + 4 * r < 13) ? gv : 0.0;
    }
  };
  // -T_A(k+1) (zero at the top frame) and M_k, operand order: register kk of lane (lr, lk) = entry (4 kk + lk, lr) / (lr, 4 kk + lk)
  auto load_factors = [&](int k, double *atn, double *amn) {
    const int kt = min(k + 1, F - 1);
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      const int q = 4 * kk + lk;
      const bool in = (lr < 13) && (q < 13);
      const double ta = TAg[kt * 169 + min(q, 12) * 13 + min(lr, 12)], m = Mg[k * 169 + min(lr, 12) * 13 + min(q, 12)];
      atn[kk] = (in && k < F - 1) ? -ta : 0.0;
      amn[kk] = in ? m : 0.0;
    }
  };
  mfma_d4 nV[5];
  double nat[4], nam[4];
  load_blocks(F - 1, nV);
  load_factors(F - 1, nat, nam);
  for (int k = F - 1; k >= 0; --k) {
    const int x_lo = chain_x_lo(k, kb);
    mfma_d4 V[5];
    double at[4], am[4];
#pragma unroll
    for (int X = 0; X < 5; ++X) V[X] = nV[X];
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) { at[kk] = nat[kk]; am[kk] = nam[kk]; }
    // V -= T_A(k+1)^T T(k+1);  T(k) = M_k V
    if (k < F - 1) {
#pragma unroll
      for (int X = 0; X < 5; ++X)
        if (X >= x_lo) {
#pragma unroll
          for (int kk = 0; kk < 4; ++kk) V[X] = __builtin_amdgcn_mfma_f64_16x16x4f64(at[kk], T[X][kk], V[X], 0, 0, 0);
        }
    }
#pragma unroll
    for (int X = 0; X < 5; ++X)
      if (X >= x_lo) {
        mfma_d4 n = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) n = __builtin_amdgcn_mfma_f64_16x16x4f64(am[kk], V[X][kk], n, 0, 0, 0);
        T[X] = n;
      }
    // the next frame's blocks and factors: in flight behind the rest of this frame
    {
      const int kn = max(k - 1, 0);
      load_blocks(kn, nV);
      load_factors(kn, nat, nam);
    }
    // t_g(k) (column 79) to every lane of its 16-lane row group; the pose system must not see it
    mfma_d4 T4 = T[4];
    double tg[4];
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      tg[kk] = __shfl(T[4][kk], (lane & 48) | 15, 64);
      if (lr == 15) T4[kk] = 0.0;
    }
    // T_B(k) out in operand order (tiles left of x_lo are zero and skipped on both sides); rhs_P -= T_B^T t_g
    {
      double *Tb = Tout + 1280 * k;
#pragma unroll
      for (int X = 0; X < 5; ++X)
        if (X >= x_lo) {
#pragma unroll
          for (int kk = 0; kk < 4; ++kk)
            if (kk < 3 || lk == 0) Tb[(X * 4 + kk) * 64 + lane] = (X == 4) ? T4[kk] : T[X][kk];   // (rows 13 .. 15 of the 16: padding, never read)
        }
    }
#pragma unroll
    for (int X = 0; X < 5; ++X)
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) yr[X] += ((X == 4) ? T4[kk] : T[X][kk]) * tg[kk];
  }
  // reduced right-hand side so far: g_P - sum_k T_B^T t_g
#pragma unroll
  for (int X = 0; X < 5; ++X) {
    yr[X] += __shfl_xor(yr[X], 16, 64);
    yr[X] += __shfl_xor(yr[X], 32, 64);
    if (lk == 0) vout[16 * X + lr] = gin[16 * X + lr] - yr[X];
  }
}
