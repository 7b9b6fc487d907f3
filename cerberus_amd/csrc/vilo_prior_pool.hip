// The prior pool (include/vilo_gpu.h): last_marginalization_info of many windows kept between images as device slots — J0 / r0 in HBM
// (n x n packed, ld n), the block table and x0 in a host mirror. k_prior_scatter (kernels_marg.hip) writes a slot. Host code only.
#include "vilo_internal.hpp"

extern "C" int vilo_prior_pool_create(vilo_ctx *ctx, int n, vilo_prior_pool **out) {
  if (!ctx || n <= 0 || !out) return VILO_ERR_BAD_ARG;
  VILO_HIP(hipSetDevice(ctx->device));
  vilo_prior_pool *pl = new vilo_prior_pool();
  pl->n = n; pl->device = ctx->device; pl->dJ = pl->dr = nullptr;
  if (hipMalloc((void **)&pl->dJ, sizeof(double) * (size_t)n * 96 * 96) != hipSuccess || hipMalloc((void **)&pl->dr, sizeof(double) * (size_t)n * 96) != hipSuccess) {
    if (pl->dJ) (void)hipFree(pl->dJ);
    delete pl;
    ctx->err = "vilo_prior_pool_create: allocation failed";
    return VILO_ERR_HIP;
  }
  pl->meta.resize(n);
  pl->x0_store.assign((size_t)n * 7 * VILO_MAX_PRIOR_BLOCKS, 0.0);
  for (int i = 0; i < n; ++i) {
    memset(&pl->meta[i], 0, sizeof(vilo_prior));
    pl->meta[i].x0 = &pl->x0_store[(size_t)i * 7 * VILO_MAX_PRIOR_BLOCKS];
  }
  *out = pl;
  return VILO_OK;
}
extern "C" void vilo_prior_pool_destroy(vilo_ctx *ctx, vilo_prior_pool *pl) {
  if (!pl) return;
  (void)ctx;
  (void)hipSetDevice(pl->device);
  (void)hipFree(pl->dJ);
  (void)hipFree(pl->dr);
  delete pl;
}
extern "C" int vilo_prior_pool_dim(const vilo_prior_pool *pl, int slot) {
  if (!pl || slot < 0 || slot >= pl->n || !pl->meta[slot].valid) return 0;
  return pl->meta[slot].n;
}
extern "C" int vilo_prior_pool_upload(vilo_ctx *ctx, vilo_prior_pool *pl, int slot, const vilo_prior *p) {
  if (!ctx || !pl || slot < 0 || slot >= pl->n) return VILO_ERR_BAD_ARG;
  vilo_prior &m = pl->meta[slot];
  if (!p || !p->valid || p->n <= 0) { m.valid = 0; m.n = 0; m.n_blocks = 0; return VILO_OK; }
  if (p->n > VILO_MAX_PRIOR_DIM || p->n_blocks > VILO_MAX_PRIOR_BLOCKS || !p->x0 || !p->J0 || !p->r0) return VILO_ERR_BAD_ARG;
  VILO_HIP(hipSetDevice(ctx->device));
  double *x0 = m.x0;
  m = *p;
  m.x0 = x0; m.J0 = nullptr; m.r0 = nullptr;
  int sum_g = 0;
  for (int k = 0; k < p->n_blocks; ++k) sum_g += p->block_size[k];
  memcpy(m.x0, p->x0, sizeof(double) * sum_g);
  VILO_HIP(hipMemcpy(pl->dJ + (size_t)slot * 96 * 96, p->J0, sizeof(double) * (size_t)p->n * p->n, hipMemcpyHostToDevice));
  VILO_HIP(hipMemcpy(pl->dr + (size_t)slot * 96, p->r0, sizeof(double) * p->n, hipMemcpyHostToDevice));
  return VILO_OK;
}
extern "C" int vilo_prior_pool_download(vilo_ctx *ctx, vilo_prior_pool *pl, int slot, vilo_prior *out) {
  if (!ctx || !pl || !out || slot < 0 || slot >= pl->n) return VILO_ERR_BAD_ARG;
  const vilo_prior &m = pl->meta[slot];
  double *x0 = out->x0, *J0 = out->J0, *r0 = out->r0;
  if (!m.valid || m.n <= 0) { out->valid = 0; out->n = 0; out->n_blocks = 0; return VILO_OK; }
  if (!x0 || !J0 || !r0) return VILO_ERR_BAD_ARG;
  VILO_HIP(hipSetDevice(ctx->device));
  VILO_HIP(hipStreamSynchronize(ctx->stream));
  *out = m;
  out->x0 = x0; out->J0 = J0; out->r0 = r0;
  int sum_g = 0;
  for (int k = 0; k < m.n_blocks; ++k) sum_g += m.block_size[k];
  memcpy(x0, m.x0, sizeof(double) * sum_g);
  VILO_HIP(hipMemcpy(J0, pl->dJ + (size_t)slot * 96 * 96, sizeof(double) * (size_t)m.n * m.n, hipMemcpyDeviceToHost));
  VILO_HIP(hipMemcpy(r0, pl->dr + (size_t)slot * 96, sizeof(double) * m.n, hipMemcpyDeviceToHost));
  return VILO_OK;
}
