// tests/test_launch_plan.py compiles this and runs it once per case, under the case's environment: the launch plan
// (cerberus_amd/csrc/launch_plan.hpp) of a batch shape as the library would compute it, on a CPU.
//   plan W n_waves compact full_regime forced_solver_form iterates -> visual imu imu_order assembly solver rows cost tpar wave_order no_graph
//   marg n_waves full_regime                                        -> the same ten numbers for the one pass of vilo_marg_linearize
//   lanes n_windows n_with_landmarks                                -> 1: the call may be cut into lanes
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../cerberus_amd/csrc/launch_plan.hpp"

int main(int argc, char **argv) {
  const vilo::Tuning &t = vilo::tuning();
  auto arg = [&](int i) { return i < argc ? atoi(argv[i]) : 0; };
  auto print = [&](const vilo::SolvePlan &p, bool tpar) {
    printf("%d %d %d %d %d %d %d %d %d %d\n", p.visual, p.imu, p.imu_order, p.assembly, p.solver, p.rows, p.cost, tpar ? 1 : 0, t.wave_order, t.no_graph ? 1 : 0);
  };
  if (argc == 8 && !strcmp(argv[1], "plan")) {
    vilo::BatchShape s{arg(2), arg(3), arg(4) != 0, false, arg(5) != 0};
    s.tpar = vilo::shape_takes_tpar((size_t)s.n_waves, s.full_regime, t);   // (what vilo_batch_create decides)
    print(vilo::plan_solve(s, arg(6), t, arg(7) != 0), s.tpar);
  } else if (argc == 4 && !strcmp(argv[1], "marg")) {
    vilo::BatchShape s{1, arg(2), true, false, arg(3) != 0};
    s.tpar = vilo::shape_takes_tpar((size_t)s.n_waves, s.full_regime, t);
    print(vilo::plan_marg_linearize(s), s.tpar);
  } else if (argc == 4 && !strcmp(argv[1], "lanes")) {
    printf("%d\n", vilo::call_is_full_as_one_batch(arg(2), arg(3), t) ? 1 : 0);
  } else {
    return 2;
  }
  return 0;
}
