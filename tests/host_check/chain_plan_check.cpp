// tests/test_chain_plan.py compiles this under sanitizers and runs it once per case, under the case's environment: the chain axis of
// the launch plan (cerberus_amd/csrc/launch_plan.hpp) as the library would compute it, on a CPU.
//   chain_plan_check W n_waves forced_solver_form iterates  ->  solver chain same_as_default
// same_as_default: 1 when the plan equals (operator==, the key of a captured launch sequence) the plan of the same shape under a Tuning
// with every switch at its default.
#include <cstdio>
#include <cstdlib>

#include "../../cerberus_amd/csrc/launch_plan.hpp"

int main(int argc, char **argv) {
  if (argc != 5) return 2;
  const vilo::Tuning &t = vilo::tuning();
  vilo::BatchShape s{atoi(argv[1]), atoi(argv[2]), true, false, false};
  s.tpar = vilo::shape_takes_tpar((size_t)s.n_waves, s.full_regime, t);
  const vilo::SolvePlan p = vilo::plan_solve(s, atoi(argv[3]), t, atoi(argv[4]) != 0);
  const vilo::Tuning d;
  vilo::BatchShape sd = s;
  sd.tpar = vilo::shape_takes_tpar((size_t)sd.n_waves, sd.full_regime, d);
  const vilo::SolvePlan pd = vilo::plan_solve(sd, atoi(argv[3]), d, atoi(argv[4]) != 0);
  printf("%d %d %d\n", p.solver, p.chain, p == pd ? 1 : 0);
  return 0;
}
