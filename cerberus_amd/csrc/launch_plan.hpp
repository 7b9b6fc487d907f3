// Which kernels a batch runs: the tuning switches, and the one function that turns a batch's shape into the forms of a Gauss-Newton
// iteration. Plain C++17, no HIP: vilo_batch.hip asks it at create (frame-parallel form or not) and for the key of a captured
// launch sequence, host_pipeline.hip for the lane rule; vilo_solve_launch executes the plan it returns; tests/host_check/launch_plan_check.cpp pins it on a CPU.
// The codes are those of vilo_debug_batch_path (include/vilo_gpu.h).
#pragma once
#include <cstddef>
#include <cstdlib>
#include <cstring>

namespace vilo {

// Every switch that selects a kernel form or a launch parameter. Tuning aids and A/B runs: read once per process, at first use.
struct Tuning {
  // up to this many packed waves a batch takes the frame-parallel form of the visual linearisation (VILO_TPAR_MAX_WAVES; VILO_NO_TPAR = 0)
  size_t tpar_max_waves = 256;
  // k_assemble_s up to this many windows (one window per CU: measured 256 windows + 4 %, 384 - 8 % against three workgroups per CU)
  int asm_small_max = 256;     // VILO_ASM_SMALL_MAX_WINDOWS
  // the IMU workgroups inside the visual launch pay up to 2048 windows (768: + 5 %, 1024: + 2.6 %, 2048: + 0.9 %; at 4096 the two forms
  // take the same time and the full batch keeps its separate kernels); 0: never
  int fuse_max = 2048;         // VILO_SMALL_FUSE_MAX_WINDOWS
  // one wave per IMU factor while the batch leaves SIMDs idle (measured: 128 windows + 1 %, 256 equal, 512 - 3 %)
  int imu_single_max = 128;    // VILO_IMU_SINGLE_MAX_WINDOWS
  // k_visual_linearize_pc_imu's IMU workgroups first (1) or last (0); -1: by size, first up to 256 windows (measured in the captured launch
  // sequence: first 564 k / last 430 k window-iterations/s at 128 windows, 986 / 838 k at 256; 1018 / 1054 k at 384, 1227 / 1239 k at 512)
  int imu_first = -1;          // VILO_IMU_FIRST
  bool visual_pc = true;       // VILO_VISUAL_FORM=single keeps the one-wave compact form (false)
  // solver: as many waves per window as the batch leaves SIMDs for — eight up to two rounds of one window per CU (512 on an MI355X; measured
  // against the single wave with the two-kernel assembly: 320 windows + 5 %, 384 + 7 %, 512 + 4 %), the single wave beyond, in three
  // stages once the batch fills the two-waves-per-SIMD stages too
  int mw8_max = 512;           // VILO_MW8_MAX_WINDOWS
  int split_min = 1025;        // VILO_SPLIT_MIN_WINDOWS
  int wave_order = 1;          // VILO_WAVE_ORDER: launch order of the packed waves, 0 window order, 1 by length, 2 by length, groups rotated
  int debug_redo = 0;          // VILO_DEBUG_REDO (k_backsub)
  // the three-stage solver's chain as the one kernel it was (k_chain_single) instead of k_chain_fact + k_chain: A/B runs and the bitwise test
  bool chain_single = false;   // VILO_CHAIN_SINGLE
  long wave_lds = -1;          // VILO_WAVE_LDS: dynamic LDS bytes of k_solve_wave / k_solve_mid (occupancy experiments); -1: what they need
  bool no_graph = false;       // VILO_NO_GRAPH: plain launches, no captured launch sequence
  bool full_record_upload = false;   // VILO_FULL_RECORD_UPLOAD: vilo_batch_create uploads whole preintegration records

  static Tuning from_env() {
    Tuning t;
    auto num = [](const char *name, auto &v) { if (const char *e = getenv(name)) v = atol(e); };
    num("VILO_TPAR_MAX_WAVES", t.tpar_max_waves);
    if (getenv("VILO_NO_TPAR")) t.tpar_max_waves = 0;
    num("VILO_ASM_SMALL_MAX_WINDOWS", t.asm_small_max);
    num("VILO_SMALL_FUSE_MAX_WINDOWS", t.fuse_max);
    num("VILO_IMU_SINGLE_MAX_WINDOWS", t.imu_single_max);
    num("VILO_IMU_FIRST", t.imu_first);
    if (const char *e = getenv("VILO_VISUAL_FORM")) t.visual_pc = strcmp(e, "single") != 0;
    num("VILO_MW8_MAX_WINDOWS", t.mw8_max);
    num("VILO_SPLIT_MIN_WINDOWS", t.split_min);
    num("VILO_WAVE_ORDER", t.wave_order);
    num("VILO_DEBUG_REDO", t.debug_redo);
    t.chain_single = getenv("VILO_CHAIN_SINGLE") != nullptr;
    num("VILO_WAVE_LDS", t.wave_lds);
    t.no_graph = getenv("VILO_NO_GRAPH") != nullptr;
    t.full_record_upload = getenv("VILO_FULL_RECORD_UPLOAD") != nullptr;
    return t;
  }
};
inline const Tuning &tuning() {
  static const Tuning t = Tuning::from_env();
  return t;
}

enum { NO_FORM = -1 };
enum Visual { VIS_SMALL_C = 0, VIS_TPAR_C, VIS_TPAR, VIS_PC_IMU, VIS_PC, VIS_SINGLE_C, VIS_SINGLE };
enum Imu { IMU_FUSED = 0, IMU_SINGLE, IMU_PAIR };
enum Assembly { ASM_SMALL = 0, ASM_FULL, ASM_ACCEPT_WAVE };
enum Solver { SOLVER_WAVE = 0, SOLVER_SPLIT = 3, SOLVER_MW8 = 4 };   // VILO_SOLVER_*
enum Cost { COST_TPAR = 0, COST_WALK };
enum Chain { CHAIN_SINGLE = 0, CHAIN_FACT };   // SOLVER_SPLIT's chain: one kernel, or the factorisation four windows per wave + the recurrence

struct BatchShape {
  int W, n_waves;     // windows, packed waves
  bool compact;       // every window keeps td constant and the context allows the 16-column rows
  bool tpar;          // created with the frame-parallel buffers (shape_takes_tpar)
  bool full_regime;   // a lane's sub-batch: the kernel set of a full batch whatever its size
};
// few packed waves: one workgroup per (packed wave, frame) instead of per packed wave, so that the chip is not left to 3 waves per window
inline bool shape_takes_tpar(size_t n_waves, bool full_regime, const Tuning &t) { return n_waves <= t.tpar_max_waves && !full_regime; }

// One launch sequence. The six axes vilo_debug_batch_path reports, the kernel of the last candidate's visual cost and the form of the
// three-stage solver's chain (NO_FORM with any other solver).
struct SolvePlan {
  int visual = NO_FORM, imu = NO_FORM, imu_order = NO_FORM, assembly = NO_FORM, solver = NO_FORM, rows = 0, cost = NO_FORM, chain = NO_FORM;
  bool fuse_imu() const { return imu == IMU_FUSED; }            // extra workgroups of the visual launch linearise the IMU factors
  bool reduce_later() const { return visual == VIS_SMALL_C; }   // k_assemble_s's extra workgroups finish the frame-parallel form
  bool imu_single() const { return imu == IMU_SINGLE; }         // k_imu_linearize: one factor per wave (else a pair)
  bool operator==(const SolvePlan &o) const {
    return visual == o.visual && imu == o.imu && imu_order == o.imu_order && assembly == o.assembly && solver == o.solver && rows == o.rows && cost == o.cost &&
           chain == o.chain;
  }
  bool operator!=(const SolvePlan &o) const { return !(*this == o); }
};

// Which assembly a batch gets (compact slots: td a constant block in every window — all of the reference's configurations):
//   up to asm_small_max windows an iteration is a chain of kernel latencies, so the chain is kept short — the IMU factors are linearised by
//     extra workgroups of the visual launch, the bookkeeping, the assembly and the second half of the frame-parallel visual form share one
//     launch (k_assemble_s): three launches per iteration (linearise, bookkeeping + assemble, solve);
//   beyond: the assembly in two kernels by LDS footprint (kernels_asm_full.hip), the bookkeeping as the first phase of the pose part.
// Beyond the small form a batch with few packed waves runs the frame-parallel visual form with its own reduction kernel (only k_assemble_s
// has workgroups for that reduction), so its IMU factors are not fused. forced_solver_form: vilo_set_solver_form, -1 by size. A solve
// without iterations launches no step but the costs.
inline SolvePlan plan_solve(const BatchShape &s, int forced_solver_form, const Tuning &t, bool iterates = true) {
  SolvePlan p;
  p.rows = s.compact ? 1 : 0;
  if (s.n_waves > 0) p.cost = s.tpar ? COST_TPAR : COST_WALK;
  if (!iterates) return p;
  const bool asm_small = s.compact && !s.full_regime && s.W <= t.asm_small_max;
  const bool takes_imu = s.n_waves > 0 && s.compact && (s.tpar || t.visual_pc);
  const bool fuse = s.W <= t.fuse_max && takes_imu && (asm_small || !s.tpar);
  if (s.n_waves <= 0) p.visual = NO_FORM;
  else if (s.tpar) p.visual = s.compact ? (fuse ? VIS_SMALL_C : VIS_TPAR_C) : VIS_TPAR;
  else if (s.compact) p.visual = t.visual_pc ? (fuse ? VIS_PC_IMU : VIS_PC) : VIS_SINGLE_C;
  else p.visual = VIS_SINGLE;
  p.imu = fuse ? IMU_FUSED : (s.W <= t.imu_single_max ? IMU_SINGLE : IMU_PAIR);
  if (p.visual == VIS_SMALL_C) p.imu_order = 1;   // (its IMU workgroups are the first W x 10)
  else if (p.visual == VIS_PC_IMU) p.imu_order = t.imu_first >= 0 ? t.imu_first : (s.W <= 256 ? 1 : 0);
  p.assembly = asm_small ? ASM_SMALL : (s.compact ? ASM_FULL : ASM_ACCEPT_WAVE);
  p.solver = forced_solver_form >= 0 ? forced_solver_form : (s.W <= t.mw8_max ? SOLVER_MW8 : (s.W < t.split_min ? SOLVER_WAVE : SOLVER_SPLIT));
  if (p.solver == SOLVER_SPLIT) p.chain = t.chain_single ? CHAIN_SINGLE : CHAIN_FACT;
  return p;
}
// The one pass of vilo_marg_linearize (marginalisation, covariance): full 23-column rows with td, the IMU factors unfused, a pair per wave.
inline SolvePlan plan_marg_linearize(const BatchShape &s) {
  SolvePlan p;
  if (s.n_waves > 0) p.visual = s.tpar ? VIS_TPAR : VIS_SINGLE;
  p.imu = IMU_PAIR;
  return p;
}

// May a host call on many windows be cut into lanes? The lanes run the kernel set of a full batch (full_regime) and the forms agree to
// rounding, not bitwise, so only a call that as ONE batch would certainly be a full one too: more windows than the small assembly takes,
// more windows with landmarks (each at least one packed wave) than the frame-parallel form takes.
inline bool call_is_full_as_one_batch(int n_windows, int n_with_landmarks, const Tuning &t) {
  return n_windows > t.asm_small_max && !shape_takes_tpar((size_t)n_with_landmarks, false, t);
}

}  // namespace vilo
