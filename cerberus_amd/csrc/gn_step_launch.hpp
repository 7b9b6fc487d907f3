// k_gn_step (kernels_step.hip) for the calls that run it: vilo_batch_gauss_newton_step and vilo_batch_dogleg_step. One launch function, so
// that the Gauss-Newton point of the dogleg is bitwise the step call's: the same kernel form (vilo_set_gn_step_form), the same chunks, the
// same blocks of the call's memory.
#pragma once
#include "batch_call.hpp"

// The blocks k_gn_step reads and writes, taken out of a call's layout before call.begin(): window records [W] | mu [W] (if given; the caller
// uploads it) | state step [W][222] | landmark step [sum L] | the kernel's per-window scratch of one chunk of windows.
struct GnStepBlocks {
  GnStepBlocks(vilo::CallLayout &lay, const BatchDev &bd, bool has_mu);
  bool has_mu;
  int chunk;
  size_t o_rec, o_mu, o_ss, o_ls, o_scr;
};

// vilo_step_opts' conditions (include/vilo_gpu.h)
bool vilo_step_opts_ok(const vilo_step_opts &o);
// k_gn_step on every window of the linearised batch `bd`, on ctx->stream. VILO_OK or VILO_ERR_HIP (ctx->err set).
int vilo_gn_step_launch(vilo_ctx *ctx, BatchCall &call, const BatchDev &bd, const GnStepBlocks &gb, const vilo_step_opts &o);
