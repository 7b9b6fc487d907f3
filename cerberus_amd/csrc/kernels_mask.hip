// Landmark mask of a resident batch (vilo_batch_mask_landmarks, include/vilo_gpu.h; Estimator::processImage's
// f_manager.removeOutlier(removeIndex), estimator.cpp:812-814; FeatureManager::removeOutlier, feature_manager.cpp).
//
// The solve's kernels, the marginalisation's linearisation and k_resid_landmarks skip an observation whose valid bit (flags[t][lane] & 1)
// is clear, so a landmark is taken out of a resident batch by clearing the valid bits of its lane's column of the flag image, and put back
// by copying the column back from the second copy of the image the batch keeps from its first mask call on. No kernel of the solve knows
// about the mask.
//
// Two launches (three with VILO_MASK_OUTLIER_FLAGS), one code path for every batch size; no atomics, no output depends on the batch a
// window shares or on its position:
//   k_resid_landmarks  (kernels_resid.hip, OUTLIER_FLAGS only) the reference's landmark test at the current state, flag bytes in caller order;
//   k_mask_landmarks   one wave per packed visual wave, lane = landmark (k_resid_landmarks' mapping, caller order through lm_perm): reads the
//                      wanted byte, writes the lane's column flags[t][lane], t < kmax, as the original with the valid bit cleared or as the
//                      original, the mask in force (device order for the next call, caller order for the caller), "newly masked" and the
//                      landmark's valid observations left;
//   k_mask_windows     one wave per window: the integer sums of a window's landmarks in caller order (exact in any order) and its record.
#include <hip/hip_runtime.h>

#include "batch_call.hpp"
#include "lin_common.hpp"

static_assert(sizeof(vilo_mask_opts) == 24, "vilo_mask_opts: 24 bytes (include/vilo_gpu.h)");
static_assert(sizeof(vilo_window_mask_record) == 24, "vilo_window_mask_record: 24 bytes (include/vilo_gpu.h)");

struct MaskArgs {
  const unsigned char *want;   // [n_lm] caller order: the caller's bytes (GIVEN) or k_resid_landmarks' flag bytes (OUTLIER_FLAGS); unread with CLEAR
  const unsigned char *orig;   // the flag image as uploaded
  unsigned char *mask;         // [n_lm] device order: the mask in force, read and rewritten
  unsigned char *out_mask, *out_new;   // [n_lm] caller order
  int *n_obs;                  // [n_lm] caller order: valid observations of the landmark that are left (0 when masked)
  int source, combine;
  unsigned flag_bits;
};

__global__ void __launch_bounds__(64) k_mask_landmarks(BatchDev b, MaskArgs a) {
  const WaveMeta wv = b.wave[blockIdx.x];
  const WinMeta wm = b.win[wv.win];
  const int lane = threadIdx.x;
  int cs[4], cn[4], ckm[4], cgo[4];
  const LaneSeg ls = lane_segment(wv, b.chunk, lane, cs, cn, ckm, cgo);
  if (!ls.active) return;   // (padding lanes: their flag bytes are zero in both copies)
  const int n = wv.n_lanes, gi = ls.gi, o = wm.lm_off + b.lm_perm[gi];
  const bool was = a.mask[gi] != 0;
  bool sel = false;
  if (a.source == VILO_MASK_GIVEN) sel = a.want[o] != 0;
  else if (a.source == VILO_MASK_OUTLIER_FLAGS) sel = (a.want[o] & a.flag_bits) != 0;
  const bool now = a.source != VILO_MASK_CLEAR && (sel || (a.combine == VILO_MASK_OR && was));   // (CLEAR: with either combine)
  const unsigned char *fo = a.orig + wv.flag_off;
  unsigned char *fl = b.flags + wv.flag_off;
  int cnt = 0;
  for (int t = 0; t < wv.kmax; ++t) {
    const unsigned char f = fo[(size_t)t * n + lane];
    cnt += f & 1;
    fl[(size_t)t * n + lane] = now ? (unsigned char)(f & ~1) : f;
  }
  a.mask[gi] = now ? 1 : 0;
  a.out_mask[o] = now ? 1 : 0;
  a.out_new[o] = (now && !was) ? 1 : 0;
  a.n_obs[o] = now ? 0 : cnt;
}

__global__ void __launch_bounds__(64) k_mask_windows(BatchDev b, const unsigned char *mask, const unsigned char *newly, const int *n_obs,
                                                     vilo_window_mask_record *out) {
  const int win = blockIdx.x, lane = threadIdx.x;
  const WinMeta wm = b.win[win];
  int nm = 0, nn = 0, no = 0;
  for (int l = lane; l < wm.L; l += 64) {
    const int o = wm.lm_off + l;
    nm += mask[o];
    nn += newly[o];
    no += n_obs[o];
  }
  // (integer counts: exact in any order)
  for (int off = 32; off > 0; off >>= 1) {
    nm += __shfl_down(nm, off, 64);
    nn += __shfl_down(nn, off, 64);
    no += __shfl_down(no, off, 64);
  }
  if (lane == 0) {
    vilo_window_mask_record r;
    r.status = (wm.L - nm > 0) ? VILO_MASK_OK : VILO_MASK_NO_LANDMARKS;
    r.n_landmarks = wm.L;
    r.n_masked = nm;
    r.n_newly_masked = nn;
    r.n_obs_left = no;
    r.pad = 0;
    out[win] = r;
  }
}

extern "C" void vilo_default_mask_opts(vilo_mask_opts *o) {
  if (!o) return;
  memset(o, 0, sizeof(*o));
  o->source = VILO_MASK_GIVEN;
  o->combine = VILO_MASK_REPLACE;
  o->flag_bits = 3;
  o->outlier_threshold_px = 3.0;
}

static int mask_check_opts(vilo_ctx *ctx, const vilo_mask_opts *opts, const uint8_t *mask_in, vilo_mask_opts *o) {
  if (opts) *o = *opts; else vilo_default_mask_opts(o);
  if (o->source != VILO_MASK_GIVEN && o->source != VILO_MASK_OUTLIER_FLAGS && o->source != VILO_MASK_CLEAR) {
    ctx->err = "vilo_batch_mask_landmarks: source must be VILO_MASK_GIVEN, VILO_MASK_OUTLIER_FLAGS or VILO_MASK_CLEAR";
    return VILO_ERR_BAD_ARG;
  }
  if (o->combine != VILO_MASK_REPLACE && o->combine != VILO_MASK_OR) {
    ctx->err = "vilo_batch_mask_landmarks: combine must be VILO_MASK_REPLACE or VILO_MASK_OR";
    return VILO_ERR_BAD_ARG;
  }
  if (o->source == VILO_MASK_CLEAR) o->combine = VILO_MASK_REPLACE;   // (CLEAR removes the mask whatever combine says)
  if (o->source == VILO_MASK_GIVEN && !mask_in) {
    ctx->err = "vilo_batch_mask_landmarks: VILO_MASK_GIVEN needs mask_in";
    return VILO_ERR_BAD_ARG;
  }
  if (o->source == VILO_MASK_OUTLIER_FLAGS && (!isfinite(o->outlier_threshold_px) || !(o->outlier_threshold_px >= 0.0))) {
    ctx->err = "vilo_batch_mask_landmarks: outlier_threshold_px must be finite and >= 0";
    return VILO_ERR_BAD_ARG;
  }
  return VILO_OK;
}

extern "C" int vilo_batch_mask_landmarks(vilo_ctx *ctx, vilo_batch *bt, const vilo_mask_opts *opts, const uint8_t *mask_in, uint8_t *mask_out,
                                         vilo_window_mask_record *records) {
  if (!ctx || !bt) return VILO_ERR_BAD_ARG;
  vilo_mask_opts o;
  const int rc = mask_check_opts(ctx, opts, mask_in, &o);
  if (rc != VILO_OK) return rc;
  ctx->last_mask_ms = 0.0;
  const BatchDev &bd = bt->d;
  const int W = bd.W, n_lm = bd.n_lm;
  if (n_lm <= 0 || bd.n_waves <= 0) return VILO_OK;   // nothing to mask: no array is touched
  VILO_HIP(hipSetDevice(ctx->device));
  BatchMask &ms = bt->mask;
  const int rs = ms.store(ctx, bt->arena, bd);   // (batch data, allocated at the first call: before the scope opens)
  if (rs != VILO_OK) return rs;
  const bool outl = o.source == VILO_MASK_OUTLIER_FLAGS;
  BatchCall call(ctx, bt, &vilo_ctx::last_mask_ms);
  // the call's device memory: wanted bytes | mask, newly masked (caller order) | observations left | window records | the residual kernel's other outputs
  const size_t o_want = call.lay.take<unsigned char>(n_lm), o_mask = call.lay.take<unsigned char>(n_lm), o_new = call.lay.take<unsigned char>(n_lm);
  const size_t o_nobs = call.lay.take<int>(n_lm), o_rec = call.lay.take<vilo_window_mask_record>(W);
  const size_t o_d3 = call.lay.take<double>(3 * (size_t)n_lm, outl), o_i2 = call.lay.take<int>(2 * (size_t)n_lm, outl);
  if (call.begin() != VILO_OK) return VILO_ERR_HIP;
  MaskArgs a;
  a.want = call.ptr<unsigned char>(o_want); a.orig = ms.d_flags_orig; a.mask = ms.d_mask;
  a.out_mask = call.ptr<unsigned char>(o_mask); a.out_new = call.ptr<unsigned char>(o_new); a.n_obs = call.ptr<int>(o_nobs);
  a.source = o.source; a.combine = o.combine; a.flag_bits = o.flag_bits;
  if (o.source == VILO_MASK_GIVEN) VILO_HIP(hipMemcpyAsync(call.ptr<unsigned char>(o_want), mask_in, (size_t)n_lm, hipMemcpyHostToDevice, ctx->stream));
  VILO_HIP(call.start());
  if (outl && vilo_resid_landmark_flags_launch(ctx, bd, o.outlier_threshold_px, call.ptr<double>(o_d3), call.ptr<int>(o_i2), call.ptr<unsigned char>(o_want)) != VILO_OK)
    return VILO_ERR_HIP;
  hipLaunchKernelGGL(k_mask_landmarks, dim3(bd.n_waves), dim3(64), 0, ctx->stream, bd, a);
  hipLaunchKernelGGL(k_mask_windows, dim3(W), dim3(64), 0, ctx->stream, bd, (const unsigned char *)a.out_mask, (const unsigned char *)a.out_new, (const int *)a.n_obs,
                     call.ptr<vilo_window_mask_record>(o_rec));
  // From here on the device's flag image and mask may have been rewritten. The host mirror (device order: what the marginalisation's host
  // tables and the refusing calls read) follows only once the mask has come down: a HIP error in between leaves the mirror marked stale,
  // and every call that reads it fails until a mask call has gone through.
  ms.changed(false);
  VILO_HIP(call.finish());
  std::vector<unsigned char> now((size_t)n_lm);
  VILO_HIP(call.down(now.data(), a.out_mask, (size_t)n_lm));
  const BatchLandmarks &lm = bt->lm;
  for (int w = 0; w < W; ++w)
    for (int i = 0; i < lm.L[w]; ++i) ms.mirror[lm.lm_off[w] + i] = now[lm.lm_off[w] + lm.perm[lm.lm_off[w] + i]];
  ms.changed(true);
  if (mask_out) memcpy(mask_out, now.data(), (size_t)n_lm);
  VILO_HIP(call.down(records, call.ptr<char>(o_rec), sizeof(vilo_window_mask_record) * (size_t)W));
  return VILO_OK;
}

extern "C" int vilo_window_mask_landmarks(vilo_ctx *ctx, int n_windows, const vilo_window_desc *in, const vilo_window_state *state,
                                          const vilo_mask_opts *opts, const uint8_t *mask_in, uint8_t *mask_out, vilo_window_mask_record *records) {
  if (!ctx || n_windows < 1 || !in || !state) return VILO_ERR_BAD_ARG;
  vilo_mask_opts o;
  const int rc = mask_check_opts(ctx, opts, mask_in, &o);
  if (rc != VILO_OK) return rc;
  return vilo_with_batch(ctx, n_windows, in, state, [&](vilo_batch *bt) { return vilo_batch_mask_landmarks(ctx, bt, opts, mask_in, mask_out, records); });
}

extern "C" double vilo_last_mask_ms(const vilo_ctx *ctx) { return ctx ? ctx->last_mask_ms : -1.0; }
