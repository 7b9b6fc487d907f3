// Device-resident batches of independent sliding windows: packing (host -> HBM layout), the solve driver and
// result download. Replaces the pack / unpack halves of Estimator::optimization():
//   vector2double  estimator.cpp:848-901   (para_* arrays, inverse depths in feature-list order)
//   problem build  estimator.cpp:1059-1216 (which residual blocks exist; here: landmark-major chunk tables)
//   double2vector  estimator.cpp:903-1003  (gauge fix: vilo_gauge_fix)
#include <algorithm>
#include <chrono>

#include "batch_pack.hpp"
#include "batch_state.hpp"

namespace {

// What the solver reads of an IMULegIntegrationBase record (vilo_preint, 1955 doubles): the 33 scalars, the bias columns 21 .. 30 of the
// Jacobian's rows 0 .. 20 (PreintHead, factors.hpp) and ONE triangle of the covariance (k_prepare_preint's Cholesky of the index-reversed
// matrix takes the source's upper triangle; the literal inverse() route reads all of it and keeps the full upload). Host windows bring
// their records up in this form — 739 doubles, 38 % of the bytes — and the device lays them out as the record the kernels index: the
// Jacobian entries no factor reads are zero in that copy, the covariance's lower triangle is the mirror of the upper.
#define REC_C_JAC 33
#define REC_C_TRI (33 + 21 * 10)
#define REC_C_N (REC_C_TRI + 31 * 32 / 2)   // 739
static inline int rec_tri_off(int r) { return r * 31 - r * (r - 1) / 2; }   // first entry of row r (columns r .. 30) of the packed upper triangle
static void rec_compact(const vilo_preint *src, double *dst) {
  memcpy(dst, src, sizeof(double) * 33);
  for (int r = 0; r < 21; ++r) memcpy(dst + REC_C_JAC + 10 * r, src->jacobian + r * 31 + 21, sizeof(double) * 10);
  for (int r = 0; r < 31; ++r) memcpy(dst + REC_C_TRI + rec_tri_off(r), src->covariance + r * 31 + r, sizeof(double) * (31 - r));
}
__global__ void __launch_bounds__(256) k_expand_records(int n, const double *comp, vilo_preint *out) {
  const int f = blockIdx.x;
  if (f >= n) return;
  const double *c = comp + (size_t)f * REC_C_N;
  double *o = (double *)(out + f);
  for (int e = threadIdx.x; e < (int)(sizeof(vilo_preint) / sizeof(double)); e += 256) {
    double v;
    if (e < 33) v = c[e];
    else if (e < 33 + 961) {
      const int r = (e - 33) / 31, q = (e - 33) - 31 * r;
      v = (r < 21 && q >= 21) ? c[REC_C_JAC + 10 * r + q - 21] : 0.0;
    } else {
      const int r = (e - 33 - 961) / 31, q = (e - 33 - 961) - 31 * r;
      const int a = min(r, q), b = max(r, q);
      v = c[REC_C_TRI + a * 31 - a * (a - 1) / 2 + (b - a)];
    }
    o[e] = v;
  }
}

// win_bad[w] = any live interval of window w whose covariance had no sqrt_info (prep_bad, written by the preparation)
__global__ void k_fold_win_bad(int W, const int *prep_bad, const unsigned char *imu_skip, int *win_bad) {
  const int w = blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= W) return;
  int bad = 0;
  for (int k = 0; k < 10; ++k) bad |= (!imu_skip[(size_t)w * 10 + k] && prep_bad[(size_t)w * 10 + k]) ? 1 : 0;
  win_bad[w] = bad;
}

// The tables of a batch are a dozen and a half small arrays: uploaded one by one, a window's batch pays a blocking copy for each (what a
// frame-by-frame caller pays per image). They are laid out in ONE host blob at the offsets of one device allocation and go up in one copy;
// the device pointers are set when the blob is flushed (nothing may read them before). Arrays of 256 KB and more keep their own copy
// straight from the caller's memory.
struct UploadBlob {
  struct Item { void **pp; size_t off; };
  std::vector<char> host;
  std::vector<Item> items;
  template <class T>
  int add(vilo_ctx *ctx, BatchArena &arena, T **p, const T *h, size_t n) {
    const size_t bytes = n * sizeof(T);
    if (bytes >= ((size_t)256 << 10)) return arena.upload_raw(ctx, p, h, n);
    const size_t off = (host.size() + 255) & ~(size_t)255;
    host.resize(off + std::max<size_t>(bytes, sizeof(T)));
    if (bytes) memcpy(host.data() + off, h, bytes);
    *p = nullptr;
    items.push_back({(void **)p, off});
    return VILO_OK;
  }
  int flush(vilo_ctx *ctx, BatchArena &arena) {
    if (items.empty()) return VILO_OK;
    void *base = nullptr;
    int rc = arena.alloc_bytes(ctx, &base, host.size());
    if (rc != VILO_OK) return rc;
    VILO_HIP(hipMemcpy(base, host.data(), host.size(), hipMemcpyHostToDevice));
    for (const Item &it : items) *it.pp = (char *)base + it.off;
    items.clear(); host.clear();
    return VILO_OK;
  }
};

// J0 / r0 of the windows whose prior lives in a pool slot: device-to-device into the staging k_prior_pack reads
__global__ void __launch_bounds__(256) k_prior_gather(int W, const WinMeta *win, const int *slot, const double *pJ, const double *pr, double *J0s, double *r0s) {
  const int w = blockIdx.x;
  if (w >= W || slot[w] < 0) return;
  const int n = win[w].prior_n;
  const double *sj = pJ + (size_t)slot[w] * 96 * 96, *sr = pr + (size_t)slot[w] * 96;
  for (int e = threadIdx.x; e < n * n; e += 256) J0s[(size_t)w * 96 * 96 + e] = sj[e];
  for (int e = threadIdx.x; e < n; e += 256) r0s[(size_t)w * 96 + e] = sr[e];
}

// MarginalizationFactor (marginalization_factor.cpp:335-395) in normal-equation form, per window: H = J0^T J0 (n x n, ld n),
// b0 = J0^T r0, c0 = r0^T r0, and H scattered into the solver's pre-assembled camera image (PD_* layout).
__global__ void __launch_bounds__(256) k_prior_pack(int W, const WinMeta *win, const double *J0s /*[W][96*96], n x n packed*/,
                                                    const double *r0s /*[W][96]*/, const int *pmap /*[W][96]*/, double *H /*[W][96*96]*/,
                                                    double *b0 /*[W][96]*/, double *c0 /*[W]*/, double *pdense /*[W][PD_N], zeroed*/) {
  extern __shared__ double Jl[];   // J0 of the window (n x n) + r0 (n): read once from HBM, every product out of LDS
  const int w = blockIdx.x, tid = threadIdx.x;
  const int n = win[w].prior_n;
  if (n <= 0) return;
  const double *J = J0s + (size_t)w * 96 * 96, *r = r0s + (size_t)w * 96;
  double *rl = Jl + 96 * 96;
  for (int e = tid; e < n * n; e += 256) Jl[e] = J[e];
  for (int e = tid; e < n; e += 256) rl[e] = r[e];
  __syncthreads();
  const int *pm = pmap + (size_t)w * 96;
  double *Hw = H + (size_t)w * 96 * 96, *pd = pdense + (size_t)w * PD_N;
  for (int e = tid; e < n * n; e += 256) {
    const int i = e / n, j = e % n;
    if (j > i) continue;
    double s = 0.0;
    for (int k = 0; k < n; ++k) s += Jl[k * n + i] * Jl[k * n + j];
    Hw[(size_t)i * n + j] = s;
    Hw[(size_t)j * n + i] = s;
    for (int rep = 0; rep < (i == j ? 1 : 2); ++rep) {
      const int ci = rep ? pm[j] : pm[i], cq = rep ? pm[i] : pm[j];
      if (ci < CD_B0 && cq < CD_B0) pd[PD_C + ci * PD_CLD + cq] = s;
      else if (ci >= CD_B0 && cq >= CD_B0) pd[PD_AD + ((ci - CD_B0) / 13) * 169 + ((ci - CD_B0) % 13) * 13 + (cq - CD_B0) % 13] = s;
      else if (ci >= CD_B0 && cq < CD_B0) pd[PD_BP + ((ci - CD_B0) % 13) * 80 + cq] = s;
    }
  }
  for (int i = tid; i < n; i += 256) {
    double s = 0.0;
    for (int k = 0; k < n; ++k) s += Jl[k * n + i] * rl[k];
    b0[(size_t)w * 96 + i] = s;
  }
  if (tid == 0) {
    double s = 0.0;
    for (int k = 0; k < n; ++k) s += rl[k] * rl[k];
    c0[w] = s;
  }
}

}  // namespace

// ---- the parts of a batch (batch_state.hpp) ----
int BatchArena::alloc_bytes(vilo_ctx *ctx, void **p, size_t bytes) {
  *p = nullptr;
  bytes = (std::max<size_t>(bytes, 1) + 255) & ~(size_t)255;
  if (cur_left < bytes) {
    const size_t want = std::max<size_t>(bytes, (size_t)64 << 20);
    int best = -1;
    for (int i = 0; i < (int)ctx->pool_free.size(); ++i)
      if (ctx->pool_free[i].second >= bytes && (best < 0 || ctx->pool_free[i].second < ctx->pool_free[best].second)) best = i;
    std::pair<void *, size_t> ch;
    if (best >= 0) {
      ch = ctx->pool_free[best];
      ctx->pool_free.erase(ctx->pool_free.begin() + best);
    } else {
      void *q = nullptr;
      VILO_HIP(hipMalloc(&q, want));
      ch = {q, want};
    }
    chunks.push_back(ch);
    cur = (char *)ch.first; cur_left = ch.second;
  }
  *p = cur;
  cur += bytes; cur_left -= bytes; used += bytes;
  return VILO_OK;
}

ArenaScope::ArenaScope(vilo_ctx *c, vilo_batch *b) : ctx(c), bt(b), n_chunks(b->arena.chunks.size()), cur_left(b->arena.cur_left), used(b->arena.used), cur(b->arena.cur) {}
ArenaScope::~ArenaScope() {
  (void)hipStreamSynchronize(ctx->stream);   // nothing of this call may still run when its memory is handed on
  BatchArena &a = bt->arena;
  for (size_t i = n_chunks; i < a.chunks.size(); ++i) ctx->pool_free.push_back(a.chunks[i]);
  a.chunks.resize(n_chunks);
  a.cur = cur; a.cur_left = cur_left; a.used = used;
}
void *ArenaScope::alloc(size_t bytes) {
  void *p = nullptr;
  return bt->arena.alloc_bytes(ctx, &p, bytes) == VILO_OK ? p : nullptr;
}

int BatchLandmarks::obs_rows(vilo_ctx *ctx, BatchArena &arena, const int **rows) {
  if (!d_obs_row) {
    int *d = nullptr;
    int rc = arena.upload(ctx, &d, obs_row);
    if (rc != VILO_OK) return rc;
    d_obs_row = d;
  }
  *rows = d_obs_row;
  return VILO_OK;
}

int BatchRecords::fold_win_bad(vilo_ctx *ctx, BatchDev &d) {
  hipLaunchKernelGGL(k_fold_win_bad, dim3((d.W + 255) / 256), dim3(256), 0, ctx->stream, d.W, d_prep_bad, d.imu_skip, d.win_bad);
  VILO_HIP(hipGetLastError());
  return VILO_OK;
}
int BatchRecords::replaced(vilo_ctx *ctx, BatchDev &d) {
  // (samples were in force once and may be again: the records vilo_batch_set_samples(NULL) brings back are these from here on)
  if (orig) VILO_HIP(hipMemcpyAsync(orig, d_pre, sizeof(vilo_preint) * (size_t)d.W * 10, hipMemcpyDeviceToDevice, ctx->stream));
  return d.win_bad ? fold_win_bad(ctx, d) : VILO_OK;
}

int BatchMask::store(vilo_ctx *ctx, BatchArena &arena, const BatchDev &d) {
  if (d_mask) return VILO_OK;
  // one block (flag copy | mask): either both exist or neither
  const size_t mask_at = (std::max<size_t>(flags_total, 1) + 255) & ~(size_t)255;
  unsigned char *fo = nullptr;
  const int rc = arena.alloc(ctx, &fo, mask_at + std::max<size_t>((size_t)d.n_lm, 1));
  if (rc != VILO_OK) return rc;
  unsigned char *mk = fo + mask_at;
  VILO_HIP(hipMemcpyAsync(fo, d.flags, std::max<size_t>(flags_total, 1), hipMemcpyDeviceToDevice, ctx->stream));
  VILO_HIP(hipMemsetAsync(mk, 0, std::max<size_t>((size_t)d.n_lm, 1), ctx->stream));
  d_flags_orig = fo; d_mask = mk;
  mirror.assign((size_t)d.n_lm, 0);
  return VILO_OK;
}
void BatchMask::changed(bool mirror_valid) {
  mirror_stale = !mirror_valid;
  if (mirror_valid) n_masked = (int)(mirror.size() - std::count(mirror.begin(), mirror.end(), 0));
}
int BatchMask::stale(vilo_ctx *ctx, const char *call) const {
  if (!mirror_stale) return VILO_OK;
  ctx->err = std::string(call) + ": the last vilo_batch_mask_landmarks on this batch failed after its kernels were launched, the mask in force is not known; run a mask call (VILO_MASK_CLEAR, or the mask wanted) first";
  return VILO_ERR_HIP;
}
int BatchMask::refuse(vilo_ctx *ctx, const char *call) const {
  if (mirror_stale) { (void)stale(ctx, call); return VILO_ERR_UNSUPPORTED; }
  if (n_masked <= 0) return VILO_OK;
  ctx->err = std::string(call) + ": a landmark mask is in force on this batch (vilo_batch_mask_landmarks) and this call does not honour it; clear the mask first";
  return VILO_ERR_UNSUPPORTED;
}

int BatchSnapshot::save(vilo_ctx *ctx, BatchArena &arena, const BatchDev &d) {
  const size_t nx = (size_t)d.W * XSTRIDE, nl = std::max<size_t>((size_t)std::max(d.n_lm, 0), 1);
  if (!d_x) {
    // one block (x | lam): either both exist or neither
    const size_t lam_at = (nx * sizeof(double) + 255) & ~(size_t)255;
    char *blk = nullptr;
    const int rc = arena.alloc(ctx, &blk, lam_at + nl * sizeof(double));
    if (rc != VILO_OK) return rc;
    d_x = (double *)blk; d_lam = (double *)(blk + lam_at);
  }
  saved = false;   // (a copy that fails leaves the slot without a state)
  VILO_HIP(hipMemcpyAsync(d_x, d.x, nx * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
  if (d.n_lm > 0) VILO_HIP(hipMemcpyAsync(d_lam, d.lam, (size_t)d.n_lm * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
  saved = true;
  return VILO_OK;
}
int BatchSnapshot::restore(vilo_ctx *ctx, const BatchDev &d) const {
  if (!saved) {
    ctx->err = "vilo_batch_restore_state: no state has been saved on this batch (vilo_batch_save_state first)";
    return VILO_ERR_UNSUPPORTED;
  }
  VILO_HIP(hipMemcpyAsync(d.x, d_x, (size_t)d.W * XSTRIDE * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
  if (d.n_lm > 0) VILO_HIP(hipMemcpyAsync(d.lam, d_lam, (size_t)d.n_lm * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
  return VILO_OK;
}

extern "C" int vilo_debug_batch_device_bytes(const vilo_batch *bt, size_t out[2]) {
  if (!bt || !out) return VILO_ERR_BAD_ARG;
  out[0] = 0;
  for (const auto &c : bt->arena.chunks) out[0] += c.second;
  out[1] = bt->arena.used;
  return VILO_OK;
}

extern "C" void vilo_batch_destroy(vilo_ctx *ctx, vilo_batch *bt) {
  if (!bt) return;
  if (ctx) (void)hipSetDevice(ctx->device);
  bt->graph.drop();
  if (ctx) {
    (void)hipStreamSynchronize(ctx->stream);   // nothing of this batch may still be running when its memory is handed on
    for (auto &c : bt->arena.chunks) ctx->pool_free.push_back(c);
  } else {
    for (auto &c : bt->arena.chunks) (void)hipFree(c.first);
  }
  delete bt;
}

int vilo_launch_preint_gather(vilo_ctx *ctx, const vilo_preint_streams *pool, int n, const int *d_ids, const int *d_dst, void *d_out);

extern "C" int vilo_batch_create(vilo_ctx *ctx, int W, const vilo_window_desc *in, const vilo_window_state *init, vilo_batch **out) {
  return vilo_batch_create_refs(ctx, W, in, nullptr, init, out);
}

namespace {

// The half-built batch of vilo_batch_create_refs: destroyed on every return but the last one
struct BatchGuard {
  vilo_ctx *ctx;
  vilo_batch *bt;
  ~BatchGuard() { if (bt) vilo_batch_destroy(ctx, bt); }
  vilo_batch *release() { vilo_batch *b = bt; bt = nullptr; return b; }
};

// What the packer (batch_pack.hpp) leaves on the host for one vilo_batch_create_refs call
struct HostPack {
  explicit HostPack(size_t W) : res(W), x0(W * XSTRIDE), px0(W * 280), pmap(W * 96), pbs(W * 40), pbi(W * 40), pbx(W * 40), pbst(W * 40), iskip(W * 10) {}
  vilo::PackPlan plan;
  std::vector<vilo::PackWindow> res;
  std::vector<double> x0, px0;
  std::vector<int> pmap, pbs, pbi, pbx, pbst;
  std::vector<unsigned char> iskip;
  // the context's reusable staging: J0 / r0 of the priors packed n x n per window for k_prior_pack (only n x n of a slot is read), the
  // wave-packed observation image and its flags
  double *pJ = nullptr, *pr0 = nullptr, *obs = nullptr;
  unsigned char *flags = nullptr;
};

// What the packer needs of window w's references (it sees no pool): whether this batch can take them, its prior, its intervals' sum_dt
vilo::PackWindow resolve_window(const vilo_window_desc &d, const vilo_resident_refs *rf, const vilo_resident_refs *rf0) {
  vilo::PackWindow r;
  if (rf && rf->preint_pool && ((d.use_leg != 0) == (rf->preint_pool->kind != 0) || !rf->preint_ids || !rf->preint_sum_dt || rf->preint_pool != rf0->preint_pool))
    r.refs_defect = "resident preintegration: pool kind must match use_leg, one pool per batch";
  else if (rf && rf->prior_pool && rf->prior_pool != rf0->prior_pool) r.refs_defect = "one prior pool per batch";
  if (r.refs_defect) return r;
  r.resident_records = rf && rf->preint_pool;
  r.prior = vilo_win_prior(d, rf);
  // (a window the packer refuses for its sizes or for a missing record array has no sum_dt to read)
  const bool have = r.resident_records || (d.use_leg ? (const void *)d.preint : (const void *)d.preint_imu) != nullptr;
  const int n_int = (have && d.n_frames >= 2 && d.n_frames <= VILO_MAX_FRAMES) ? d.n_frames - 1 : 0;
  for (int k = 0; k < n_int; ++k) r.sum_dt[k] = vilo_win_sum_dt(d, rf, k);
  return r;
}

// Every device buffer of a batch but the records', in arena order, each once: `up` a host table (the small ones go up in one blob at
// the flush; nothing may read their device pointers before), `dev` storage the kernels write, cleared where they rely on it.
int create_device_buffers(vilo_ctx *ctx, vilo_batch *bt, const HostPack &h) {
  BatchDev &D = bt->d;
  const vilo::PackPlan &P = h.plan;
  const size_t W = (size_t)D.W, lm = (size_t)P.lm_total;
  const bool CLEAR = true;
  UploadBlob blob;
  int rc = VILO_OK;
  auto up = [&](auto **p, const auto *src, size_t n) { if (rc == VILO_OK) rc = blob.add(ctx, bt->arena, p, src, n); };
  auto upv = [&](auto **p, const auto &v) { up(p, v.data(), v.size()); };
  auto dev = [&](auto **p, size_t n, bool clear = false) {
    if (rc == VILO_OK) rc = bt->arena.alloc(ctx, p, n);
    if (rc == VILO_OK && clear && hipMemsetAsync(*p, 0, sizeof(**p) * std::max<size_t>(n, 1), ctx->stream) != hipSuccess) rc = VILO_ERR_HIP;
  };
  upv(&D.win, P.wins); upv(&D.chunk, P.chunks); upv(&D.wave, P.waves); upv(&D.wave_order, P.wave_order);
  up(&D.obs, h.obs, P.obs_total); up(&D.flags, h.flags, P.flags_total);
  upv(&D.x0, h.x0); upv(&D.lam0, P.lam0); upv(&D.lm_s, P.lm_s); upv(&D.lm_perm, bt->lm.perm);
  dev(&D.x, W * XSTRIDE); dev(&D.xc, W * XSTRIDE);
  dev(&D.lam, lm); dev(&D.lamc, lm); dev(&D.lm_E, lm); dev(&D.lm_gbuf[0], lm); dev(&D.lm_gbuf[1], lm);
  dev(&D.lm_dh2, lm); dev(&D.lm_y, lm); dev(&D.lm_scale, lm); dev(&D.lm_einv, lm);
  // a landmark's coupling rows with the poses before its start frame are structural zeros: written here once, never again
  dev(&D.lm_w, lm * 80, CLEAR);
  // few windows: one workgroup per (packed wave, frame) instead of per packed wave, so that the chip is not left to 3 waves per window
  // (the landmark-side terms every such workgroup writes: all of them, zeros included — nothing reads an entry nobody wrote)
  D.lm_part = nullptr;
  D.full_regime = ctx->regime_full;
  if (vilo::shape_takes_tpar(P.waves.size(), ctx->regime_full != 0, vilo::tuning())) dev(&D.lm_part, lm * VILO_MAX_FRAMES * 2 * 21);
  dev(&D.gram, (size_t)P.gram_total * VILO_GRAM);
  dev(&D.chunk_cost, P.waves.size() * VILO_MAX_FRAMES);   // per (packed wave, frame offset) partial costs
  dev(&D.prep, W * 10); dev(&D.imu_lin, W * 10 * 31 * 39);
  // (k_imu_linearize's pair loads also bring the pool of a factor k_imu_raw skipped and the entries a plain IMU factor leaves out: never
  // used, but no kernel is to load memory nobody wrote)
  dev(&D.imu_raw, W * 10 * IB_N, CLEAR);
  dev(&D.imu_gram, W * 10 * 780); dev(&D.imu_cost, W * 10);
  upv(&D.imu_skip, h.iskip);
  dev(&D.prior_H, W * 96 * 96, CLEAR); dev(&D.prior_dense, W * PD_N, CLEAR); dev(&D.prior_hd, W * 96);
  dev(&D.prior_b0, W * 96, CLEAR); dev(&D.prior_c0, W, CLEAR);
  upv(&D.prior_x0, h.px0); upv(&D.prior_map, h.pmap);
  upv(&D.prior_bsize, h.pbs); upv(&D.prior_bidx, h.pbi); upv(&D.prior_bxoff, h.pbx); upv(&D.prior_bstate, h.pbst);
  if (rc == VILO_OK) rc = blob.flush(ctx, bt->arena);   // D.win ... D.prior_bstate are device pointers from here on
  dev(&D.cam_g, W * CD_N); dev(&D.cam_dh2, W * CD_N); dev(&D.cam_y, W * CD_N); dev(&D.cam_scale, W * CD_N);
  dev(&D.Lk, W * 11 * 169); dev(&D.TAg, W * 11 * 169); dev(&D.Cimg, W * 3840); dev(&D.Tk, W * TK_N);
  dev(&D.cam_gin, W * CD_N); dev(&D.Bimg, W * BI_N);
  dev(&D.st, W, CLEAR); dev(&D.status, 1, CLEAR); dev(&D.lin_cur, W);
  return rc;
}

// The priors' J0 / r0 (host staging; pool slots gathered on the device) -> H, b0, c0 and the pre-assembled image, by k_prior_pack
int upload_priors(vilo_ctx *ctx, vilo_batch *bt, const HostPack &h, const vilo_resident_refs *refs) {
  BatchDev &D = bt->d;
  const int W = D.W;
  double *d_J = nullptr, *d_r = nullptr;
  int rc = bt->arena.alloc(ctx, &d_J, (size_t)W * 96 * 96);
  if (rc == VILO_OK) rc = bt->arena.alloc(ctx, &d_r, (size_t)W * 96);
  if (rc != VILO_OK) return rc;
  if (hipMemcpyAsync(d_J, h.pJ, sizeof(double) * (size_t)W * 96 * 96, hipMemcpyHostToDevice, ctx->stream) != hipSuccess ||
      hipMemcpyAsync(d_r, h.pr0, sizeof(double) * (size_t)W * 96, hipMemcpyHostToDevice, ctx->stream) != hipSuccess) return VILO_ERR_HIP;
  if (refs && refs[0].prior_pool) {
    std::vector<int> slot(W, -1);
    for (int w = 0; w < W; ++w)
      if (refs[w].prior_pool && refs[w].prior_slot >= 0 && refs[w].prior_slot < refs[w].prior_pool->n && h.plan.wins[w].prior_n > 0) slot[w] = refs[w].prior_slot;
    int *d_slot = nullptr;
    rc = bt->arena.upload(ctx, &d_slot, slot);
    if (rc != VILO_OK) return rc;
    hipLaunchKernelGGL(k_prior_gather, dim3(W), dim3(256), 0, ctx->stream, W, D.win, d_slot, refs[0].prior_pool->dJ, refs[0].prior_pool->dr, d_J, d_r);
  }
  const size_t pp_lds = sizeof(double) * (96 * 96 + 96);
  if (!ctx->prior_attr_set) {
    if (hipFuncSetAttribute((const void *)k_prior_pack, hipFuncAttributeMaxDynamicSharedMemorySize, (int)pp_lds) != hipSuccess) return VILO_ERR_HIP;
    ctx->prior_attr_set = true;
  }
  hipLaunchKernelGGL(k_prior_pack, dim3(W), dim3(256), pp_lds, ctx->stream, W, D.win, d_J, d_r, D.prior_map, D.prior_H, D.prior_b0, D.prior_c0, D.prior_dense);
  return hipGetLastError() == hipSuccess ? VILO_OK : VILO_ERR_HIP;
}

// Host data to the device through the context's two page-locked staging chunks (slots 4 and 5, up to 32 MB each): the worker pool
// gathers chunk k + 1 into one while the DMA engine reads chunk k out of the other. gather(item, dst) writes one item's per_item bytes;
// copy(c0, cn, src) enqueues the copies of items c0 .. c0 + cn - 1 out of src; behind(c0, cn) enqueues what the device does with them.
template <class Gather, class Copy, class Behind>
int upload_through_ring(vilo_ctx *ctx, size_t n_items, size_t per_item, Gather gather, Copy copy, Behind behind) {
  const size_t chunk_n = std::max<size_t>(1, ((size_t)32 << 20) / per_item);
  char *ring[2] = {(char *)vilo_host_stage(ctx, 4, per_item * chunk_n), (char *)vilo_host_stage(ctx, 5, per_item * chunk_n)};
  if (!ctx->rec_ev[0]) { (void)hipEventCreateWithFlags(&ctx->rec_ev[0], hipEventDisableTiming); (void)hipEventCreateWithFlags(&ctx->rec_ev[1], hipEventDisableTiming); }
  if (!ring[0] || !ring[1] || !ctx->rec_ev[0] || !ctx->rec_ev[1]) return VILO_ERR_HIP;
  bool used[2] = {false, false};
  for (size_t c0 = 0, ci = 0; c0 < n_items; c0 += chunk_n, ++ci) {
    const int sl = (int)(ci & 1);
    const size_t cn = std::min(chunk_n, n_items - c0);
    if (used[sl] && hipEventSynchronize(ctx->rec_ev[sl]) != hipSuccess) return VILO_ERR_HIP;
    vilo::parallel_items((int)cn, 4, [&](int i) { gather(c0 + (size_t)i, ring[sl] + per_item * (size_t)i); }, ctx->pool);
    if (copy(c0, cn, ring[sl]) != VILO_OK || hipEventRecord(ctx->rec_ev[sl], ctx->stream) != hipSuccess) return VILO_ERR_HIP;
    used[sl] = true;
    behind(c0, cn);
  }
  return VILO_OK;
}

// The windows' preintegration records into d_pre ([W * 10] vilo_preint / vilo_preint_imu). Host records go through the staging ring (a
// staged host copy of W x 156 KB at once costs more than the copies; one hipMemcpyAsync per window straight from the caller's pageable
// arrays moved 640 MB of a 4096-window batch at 11.5 GB/s — the runtime's own bounce buffer, one thread); records of a device pool are
// gathered there. *compact_bytes: bytes that crossed the bus when not the full records'.
int upload_records(vilo_ctx *ctx, vilo_batch *bt, const vilo_window_desc *in, const vilo_resident_refs *refs, void *d_pre, size_t *compact_bytes) {
  const int W = bt->W;
  const bool leg = bt->rec.leg;
  const size_t rec = leg ? sizeof(vilo_preint) : sizeof(vilo_preint_imu);
  bool partial = false;
  for (int w = 0; w < W; ++w) partial = partial || in[w].n_frames < VILO_MAX_FRAMES;
  if (partial && hipMemsetAsync(d_pre, 0, rec * (size_t)W * 10, ctx->stream) != hipSuccess) return VILO_ERR_HIP;
  std::vector<int> g_ids, g_dst, host_rec;   // host_rec: windows whose records come out of the caller's arrays
  for (int w = 0; w < W; ++w) {
    if (!(refs && refs[w].preint_pool)) { host_rec.push_back(w); continue; }
    for (int k = 0; k + 1 < in[w].n_frames; ++k) {
      const int id = refs[w].preint_ids[k];
      if (id < 0 || id >= refs[w].preint_pool->n) return VILO_ERR_BAD_ARG;
      g_ids.push_back(id); g_dst.push_back(w * 10 + k);
    }
  }
  int rc = VILO_OK;
  if (leg && (int)host_rec.size() == W && ctx->sqrt_info_mode == 0 && !vilo::tuning().full_record_upload) {
    // every window's records from host memory, default sqrt_info route: the compact form (above); the device expands each chunk behind its copy
    const size_t per_win = sizeof(double) * REC_C_N * 10;
    void *d_comp = nullptr;
    if (bt->arena.alloc_bytes(ctx, &d_comp, per_win * (size_t)W) != VILO_OK) return VILO_ERR_HIP;
    *compact_bytes = per_win * (size_t)W;
    bt->rec.form = 1;
    rc = upload_through_ring(ctx, (size_t)W, per_win,
        [&](size_t w, char *to) {
          const int nr = in[w].n_frames - 1;
          double *dst = (double *)to;
          for (int k = 0; k < nr; ++k) rec_compact(in[w].preint + k, dst + (size_t)REC_C_N * k);
          if (nr < 10) memset(dst + (size_t)REC_C_N * nr, 0, sizeof(double) * REC_C_N * (size_t)(10 - nr));   // (intervals the window does not have: zero records)
        },
        [&](size_t c0, size_t cn, const char *src) {
          return hipMemcpyAsync((char *)d_comp + per_win * c0, src, per_win * cn, hipMemcpyHostToDevice, ctx->stream) == hipSuccess ? VILO_OK : VILO_ERR_HIP;
        },
        [&](size_t c0, size_t cn) {
          hipLaunchKernelGGL(k_expand_records, dim3((unsigned)(cn * 10)), dim3(256), 0, ctx->stream, (int)(cn * 10), (const double *)d_comp + (size_t)REC_C_N * 10 * c0,
                             (vilo_preint *)d_pre + 10 * c0);
        });
    if (rc == VILO_OK && hipGetLastError() != hipSuccess) rc = VILO_ERR_HIP;
  } else if (!host_rec.empty()) {
    const size_t per_win = rec * 10;
    rc = upload_through_ring(ctx, host_rec.size(), per_win,
        [&](size_t i, char *to) {
          const int w = host_rec[i];
          memcpy(to, leg ? (const void *)in[w].preint : (const void *)in[w].preint_imu, rec * (size_t)(in[w].n_frames - 1));
        },
        [&](size_t c0, size_t cn, const char *src) {   // consecutive windows of the chunk that are consecutive in the batch go up in one copy
          for (size_t i = 0, j; i < cn; i = j) {
            for (j = i + 1; j < cn && host_rec[c0 + j] == host_rec[c0 + j - 1] + 1 && in[host_rec[c0 + j - 1]].n_frames == VILO_MAX_FRAMES;) ++j;
            const size_t bytes_run = (j - i - 1) * per_win + rec * (size_t)(in[host_rec[c0 + j - 1]].n_frames - 1);
            if (hipMemcpyAsync((char *)d_pre + per_win * (size_t)host_rec[c0 + i], src + per_win * i, bytes_run, hipMemcpyHostToDevice, ctx->stream) != hipSuccess) return VILO_ERR_HIP;
          }
          return VILO_OK;
        },
        [](size_t, size_t) {});
  }
  if (rc == VILO_OK && !g_ids.empty()) {
    int *d_gi = nullptr, *d_gd = nullptr;
    bt->rec.from_pool = true;
    rc = bt->arena.upload(ctx, &d_gi, g_ids);
    if (rc == VILO_OK) rc = bt->arena.upload(ctx, &d_gd, g_dst);
    if (rc == VILO_OK) rc = vilo_launch_preint_gather(ctx, refs[0].preint_pool, (int)g_ids.size(), d_gi, d_gd, d_pre);
  }
  return rc;
}

// The records, their sqrt_info = chol(cov^-1)^T hoisted out of the iteration loop (the reference recomputes it on every
// IMULegFactor::Evaluate, imu_leg_factor.cpp:197-198) and the windows a record without one fails
int create_records(vilo_ctx *ctx, vilo_batch *bt, const vilo_window_desc *in, const vilo_resident_refs *refs, size_t *compact_bytes) {
  BatchDev &D = bt->d;
  const int W = bt->W;
  const bool leg = in[0].use_leg != 0;
  void *d_pre = nullptr;
  if (bt->arena.alloc_bytes(ctx, &d_pre, (leg ? sizeof(vilo_preint) : sizeof(vilo_preint_imu)) * (size_t)W * 10) != VILO_OK) return VILO_ERR_HIP;   // arena: lives as long as the batch
  bt->rec.d_pre = d_pre; bt->rec.leg = leg;
  int rc = upload_records(ctx, bt, in, refs, d_pre, compact_bytes);
  if (rc == VILO_OK) rc = bt->arena.alloc(ctx, &bt->rec.d_prep_bad, (size_t)W * 10);
  D.prep_bad = bt->rec.d_prep_bad;   // (per-interval flags of the records in force: the marginalisation looks at the intervals it uses)
  if (rc == VILO_OK) rc = vilo_batch_prepare(ctx, bt);
  // a covariance that is not positive definite has no sqrt_info: that window alone fails (termination FAILURE, like a non-finite
  // IterationZero); the flag is looked at for live intervals only — folded per window on the device (no round trip through the host:
  // a one-window batch is built for every image of a replay)
  if (rc == VILO_OK) rc = bt->arena.alloc(ctx, &D.win_bad, (size_t)W);
  if (rc == VILO_OK) rc = bt->rec.fold_win_bad(ctx, D);
  // (the uploads above came out of this call's host memory and the context's reusable staging: they are complete when it returns)
  if (rc == VILO_OK && hipStreamSynchronize(ctx->stream) != hipSuccess) rc = VILO_ERR_HIP;
  return rc;
}

}  // namespace

// refs (optional, [W]): device-resident preintegration objects / prior slots instead of the host records of the descs.
// plan -> staging -> fill (batch_pack.hpp) -> allocate and upload -> records -> prepare and reset
int vilo_batch_create_refs(vilo_ctx *ctx, int W, const vilo_window_desc *in, const vilo_resident_refs *refs, const vilo_window_state *init, vilo_batch **out) {
  if (!ctx || !in || !init || !out || W <= 0) return VILO_ERR_BAD_ARG;
  *out = nullptr;
  VILO_HIP(hipSetDevice(ctx->device));
  BatchGuard guard{ctx, new vilo_batch()};
  vilo_batch *bt = guard.bt;
  bt->W = W;
  memset(&bt->d, 0, sizeof(BatchDev));
  const bool timing = getenv("VILO_HOST_TIMING") != nullptr;
  auto now = [] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
  const double t_begin = now();
  HostPack h((size_t)W);
  vilo::PackPlan &P = h.plan;
  for (int w = 0; w < W; ++w) h.res[w] = resolve_window(in[w], refs ? refs + w : nullptr, refs);
  const vilo::PackStatus st = vilo::plan_batch(W, in, init, h.res.data(), ctx->compact_rows != 0, vilo::tuning(), P);
  if (st.code != VILO_OK) {
    if (st.msg) ctx->err = st.msg;
    return st.code;
  }
  const double t_plan = now() - t_begin;   // (the serial table pass's share of the packing time, for VILO_HOST_TIMING)
  h.pJ = (double *)vilo_host_stage(ctx, 0, sizeof(double) * (size_t)W * 96 * 96);
  h.pr0 = (double *)vilo_host_stage(ctx, 1, sizeof(double) * (size_t)W * 96);
  h.obs = (double *)vilo_host_stage(ctx, 2, sizeof(double) * std::max<size_t>(1, P.obs_total));
  h.flags = (unsigned char *)vilo_host_stage(ctx, 3, std::max<size_t>(1, P.flags_total));
  if (!h.pJ || !h.pr0 || !h.obs || !h.flags) return VILO_ERR_HIP;
  vilo::fill_batch(W, in, init, h.res.data(), P, {h.obs, h.flags, h.x0.data(), h.pmap.data(), h.pbs.data(), h.pbi.data(), h.pbx.data(), h.pbst.data(), h.px0.data(), h.pJ, h.pr0, h.iskip.data()},
                   ctx->pool);   // (worker_pool.hpp: host threads parked between batches)
  bt->lm.lm_off = std::move(P.lm_off); bt->lm.L = std::move(P.L); bt->lm.perm = std::move(P.perm);
  bt->lm.obs_row = std::move(P.obs_row); bt->lm.n_obs_rows = P.n_obs_rows;
  bt->mask.flags_total = P.flags_total;
  for (const WinMeta &wm : P.wins) bt->lm.max_win_waves = std::max(bt->lm.max_win_waves, wm.n_waves);
  const double t_packed = now();
  // a lane of vilo_solve_windows' pipeline: the uploads of the lanes go one after the other at the link's rate (side by side every lane's
  // solve would start when ALL uploads are through); held until this batch's uploads are complete, i.e. to the end of the call
  std::unique_lock<std::mutex> dma_turn;
  if (ctx->dma_turn) dma_turn = std::unique_lock<std::mutex>(*ctx->dma_turn);
  BatchDev &D = bt->d;
  D.W = W; D.n_chunks = (int)P.chunks.size(); D.n_lm = P.lm_total; D.n_gram = P.gram_total; D.n_waves = (int)P.waves.size();
  D.compact = P.compact;   // (vilo_set_compact_rows(ctx, 0) keeps the 23-column form)
  int rc = create_device_buffers(ctx, bt, h);
  if (rc == VILO_OK && P.any_prior) rc = upload_priors(ctx, bt, h, refs);
  if (rc != VILO_OK) return rc;
  const double t_uploaded = now();
  size_t rec_bytes_up = 0;
  rc = create_records(ctx, bt, in, refs, &rec_bytes_up);
  if (rc != VILO_OK) return rc;
  const double t_prep = now();
  rc = vilo_batch_reset(ctx, bt);
  if (rc != VILO_OK) return rc;
  ctx->last_create_ms[0] = now() - t_begin; ctx->last_create_ms[1] = t_packed - t_begin; ctx->last_create_ms[2] = t_uploaded - t_packed; ctx->last_create_ms[3] = t_prep - t_uploaded;
  ctx->last_create_bytes = (double)(sizeof(double) * (P.obs_total + (size_t)W * XSTRIDE + (P.any_prior ? (size_t)W * (96 * 96 + 96) : 0)) + P.flags_total +
                                    (rec_bytes_up ? rec_bytes_up : (in[0].use_leg ? sizeof(vilo_preint) : sizeof(vilo_preint_imu)) * (size_t)W * 10));
  if (timing)
    fprintf(stderr, "[vilo_batch_create] W=%d pack %.2f ms (of which the serial table pass %.2f) alloc+upload %.2f ms preint %.2f ms reset %.2f ms\n", W, t_packed - t_begin, t_plan,
            t_uploaded - t_packed, t_prep - t_uploaded, now() - t_prep);
  *out = guard.release();
  return VILO_OK;
}

// sqrt_info = chol(cov^-1)^T of every live interval of the batch (asynchronous, on the context's stream)
extern "C" int vilo_batch_prepare(vilo_ctx *ctx, vilo_batch *bt) {
  if (!ctx || !bt || !bt->rec.d_pre) return VILO_ERR_BAD_ARG;
  VILO_HIP(hipSetDevice(ctx->device));
  BatchDev &D = bt->d;
  const BatchRecords &R = bt->rec;
  VILO_HIP(hipMemsetAsync(R.d_prep_bad, 0, sizeof(int) * (size_t)bt->W * 10, ctx->stream));
  const bool timed = ctx->profile == 1 || ctx->profile == 2 + 11;   // (kind 11 = k_prepare_preint, vilo_kernel_name)
  if (timed) {
    for (hipEvent_t &e : ctx->prep_ev) if (!e) VILO_HIP(hipEventCreate(&e));
    VILO_HIP(hipEventRecord(ctx->prep_ev[0], ctx->stream));
  }
  int rc = R.leg ? vilo_launch_prepare_preint(ctx, bt->W * 10, (const vilo_preint *)R.d_pre, D.prep, R.d_prep_bad, D.imu_skip, 1)
                 : vilo_launch_prepare_preint_imu(ctx, bt->W * 10, (const vilo_preint_imu *)R.d_pre, D.prep, R.d_prep_bad, D.imu_skip, 1);
  if (rc == VILO_OK && !R.leg) rc = vilo_launch_embed_sqrt15(ctx, D);
  if (timed) {
    VILO_HIP(hipEventRecord(ctx->prep_ev[1], ctx->stream));
    ctx->prep_pending = true;
  }
  return rc;
}

// a vilo_batch_set_samples that fails: nothing of a set of samples may stay referenced by the launch sequence, captured or not
static int samples_failed(vilo_batch *bt, int rc) {
  BatchDev &D = bt->d;
  D.rp_on = 0; D.rp_samples = nullptr; D.rp_terms = nullptr; D.rp_offsets = nullptr;
  bt->graph.drop();
  return rc;
}

// BASELINE configs[2]: keep the samples behind the batch's IMU-leg records in HBM and integrate every live interval again
// (IMULegIntegrationBase::repropagate, imu_leg_integration_base.cpp:62-86) at the biases of each point the solver linearises
extern "C" int vilo_batch_set_samples(vilo_ctx *ctx, vilo_batch *bt, const vilo_sample *samples, const int32_t *offsets) {
  if (!ctx || !bt) return VILO_ERR_BAD_ARG;
  BatchDev &D = bt->d;
  BatchRecords &R = bt->rec;
  const size_t n = (size_t)bt->W * 10;
  if (!samples) {   // back to records integrated once
    if (!D.rp_on) return VILO_OK;
    D.rp_on = 0;
    bt->graph.drop();
    // d_pre holds what the last re-integration left (the records at the last candidate point): the records the batch was created with come
    // back from their copy, their sqrt_info is prepared again and win_bad is folded again from the flags of that preparation — a covariance
    // without sqrt_info fails its window again, as it did before the samples were set. All of it is complete when the call returns.
    VILO_HIP(hipSetDevice(ctx->device));
    if (R.orig) VILO_HIP(hipMemcpyAsync(R.d_pre, R.orig, sizeof(vilo_preint) * n, hipMemcpyDeviceToDevice, ctx->stream));
    int rc = vilo_batch_prepare(ctx, bt);
    if (rc == VILO_OK && D.win_bad) rc = R.fold_win_bad(ctx, D);
    if (rc != VILO_OK) return rc;
    VILO_HIP(hipStreamSynchronize(ctx->stream));
    return VILO_OK;
  }
  if (!offsets) return VILO_ERR_BAD_ARG;
  if (!R.leg || !R.d_pre) { ctx->err = "vilo_batch_set_samples: the batch has no IMU-leg preintegration records"; return VILO_ERR_UNSUPPORTED; }
  VILO_HIP(hipSetDevice(ctx->device));
  std::vector<unsigned char> skip(n);
  VILO_HIP(hipMemcpy(skip.data(), D.imu_skip, n, hipMemcpyDeviceToHost));
  if (offsets[0] < 0) return VILO_ERR_BAD_ARG;
  for (size_t f = 0; f < n; ++f)
    if (offsets[f + 1] < offsets[f] || (!skip[f] && offsets[f + 1] - offsets[f] < 2)) {
      // (one sample = the constructor's: nothing is integrated and the covariance stays zero, which has no sqrt_info)
      ctx->err = "vilo_batch_set_samples: a live interval needs at least two samples";
      return VILO_ERR_BAD_ARG;
    }
  if (!R.rp_s || R.rp_cap < (size_t)offsets[n]) {
    R.rp_cap = (size_t)offsets[n];
    int rc = bt->arena.alloc(ctx, &R.rp_s, R.rp_cap);
    if (rc == VILO_OK && !R.rp_o) rc = bt->arena.alloc(ctx, &R.rp_o, n + 1);
    if (rc == VILO_OK) rc = bt->arena.alloc(ctx, &R.rp_t, R.rp_cap * (size_t)(4 * VILO_LEG_REC));   // 4 legs x one record per sample
    if (rc != VILO_OK) {
      R.rp_s = nullptr; R.rp_cap = 0;
      return samples_failed(bt, rc);
    }
  }
  if (!R.orig) {   // the records the batch was created with (vilo_batch_set_samples(NULL) brings them back)
    int rc = bt->arena.alloc(ctx, &R.orig, n);
    if (rc != VILO_OK) return rc;
    VILO_HIP(hipMemcpyAsync(R.orig, R.d_pre, sizeof(vilo_preint) * n, hipMemcpyDeviceToDevice, ctx->stream));
    VILO_HIP(hipStreamSynchronize(ctx->stream));
  }
  // the records are integrated again before every linearisation from here on: the flags of the records the batch was created with no
  // longer describe them (k_accept / the marginalisation read prep_bad of the records in force)
  if (D.win_bad) VILO_HIP(hipMemset(D.win_bad, 0, sizeof(int) * (size_t)bt->W));
  VILO_HIP(hipMemcpy(R.rp_s, samples, sizeof(vilo_sample) * (size_t)offsets[n], hipMemcpyHostToDevice));
  VILO_HIP(hipMemcpy(R.rp_o, offsets, sizeof(int) * (n + 1), hipMemcpyHostToDevice));
  D.rp_samples = R.rp_s; D.rp_terms = R.rp_t; D.rp_offsets = R.rp_o; D.rp_pre = R.d_pre; D.prep_bad = R.d_prep_bad; D.leg = 1; D.rp_on = 1;
  // Every interval is one IMULegIntegrationBase object that integrated its samples once (the record the batch was created with); the
  // solver's re-integrations are repropagate() calls on it, and repropagate() leaves the contact-force filter of contact_sensor_type 2 as
  // the previous pass left it (imu_leg_integration_base.cpp:62-86). The filter state after the original integration depends on the
  // samples only: that pass is run here once (mode 2: at the records' own linearisation point, which reproduces the records).
  if (!R.rp_ff) { int rc = bt->arena.alloc(ctx, &R.rp_ff, n * VILO_FF_N); if (rc != VILO_OK) return samples_failed(bt, rc); }
  D.rp_ff = R.rp_ff;
  VILO_HIP(hipMemsetAsync(R.rp_ff, 0, sizeof(double) * n * VILO_FF_N, ctx->stream));
  if (ctx->cfg.contact_sensor_type == 2) {
    int rc = vilo_repropagate_launch(ctx, D, 2, 0);
    if (rc != VILO_OK) return samples_failed(bt, rc);
    // a reset batch is the batch as it was after this call: the filter state the first integration left, not the one the last solve's
    // re-integrations left (reset + solve is then repeatable bit for bit: bench steps, Monte-Carlo restarts, graph replays)
    if (!R.rp_ff0) { rc = bt->arena.alloc(ctx, &R.rp_ff0, n * VILO_FF_N); if (rc != VILO_OK) return samples_failed(bt, rc); }
    VILO_HIP(hipMemcpyAsync(R.rp_ff0, R.rp_ff, sizeof(double) * n * VILO_FF_N, hipMemcpyDeviceToDevice, ctx->stream));
  }
  bt->graph.drop();   // the captured launch sequence changes
  return VILO_OK;
}

extern "C" int vilo_batch_reset(vilo_ctx *ctx, vilo_batch *bt) {
  if (!ctx || !bt) return VILO_ERR_BAD_ARG;
  VILO_HIP(hipSetDevice(ctx->device));
  VILO_HIP(hipMemcpyAsync(bt->d.x, bt->d.x0, sizeof(double) * (size_t)bt->W * XSTRIDE, hipMemcpyDeviceToDevice, ctx->stream));
  if (bt->d.n_lm > 0)
    VILO_HIP(hipMemcpyAsync(bt->d.lam, bt->d.lam0, sizeof(double) * (size_t)bt->d.n_lm, hipMemcpyDeviceToDevice, ctx->stream));
  if (bt->d.rp_on && bt->rec.rp_ff0 && ctx->cfg.contact_sensor_type == 2)   // the contact-force filters of the intervals' objects as set_samples left them
    VILO_HIP(hipMemcpyAsync(bt->rec.rp_ff, bt->rec.rp_ff0, sizeof(double) * (size_t)bt->W * 10 * VILO_FF_N, hipMemcpyDeviceToDevice, ctx->stream));
  return VILO_OK;
}

extern "C" int vilo_batch_solve(vilo_ctx *ctx, vilo_batch *bt, const vilo_solve_opts *opts) {
  if (!ctx || !bt || !opts) return VILO_ERR_BAD_ARG;
  if (opts->max_num_iterations < 0 || opts->max_num_iterations > 63) return VILO_ERR_BAD_ARG;
  if (bt->mask.stale(ctx, "vilo_batch_solve") != VILO_OK) return VILO_ERR_HIP;
  VILO_HIP(hipSetDevice(ctx->device));
  int rc = VILO_OK;
  const vilo::SolvePlan plan = vilo::plan_solve(vilo_batch_shape(bt->d), ctx->solver_form, vilo::tuning(), opts->max_num_iterations > 0);
  SolveGraph &G = bt->graph;
  const bool want_graph = !ctx->profile && !G.failed && bt->n_solves >= 1 && !vilo::tuning().no_graph;
  if (opts->max_solver_time_us < 0) { ctx->err = "vilo_solve_opts.max_solver_time_us < 0 (fill the struct with vilo_default_solve_opts)"; return VILO_ERR_BAD_ARG; }
  const SolveGraph::Key key{*opts, ctx->sqrt_info_mode, bt->d.rp_on, ctx->initial_mu, plan};   // what the launch sequence depends on
  if (want_graph && !(G.exec && G.key == key)) {
    G.drop();
    hipGraph_t g = nullptr;
    if (hipStreamBeginCapture(ctx->stream, hipStreamCaptureModeThreadLocal) == hipSuccess) {
      rc = vilo_solve_launch(ctx, bt->d, opts, plan);
      const hipError_t e = hipStreamEndCapture(ctx->stream, &g);
      if (rc != VILO_OK || e != hipSuccess || !g || hipGraphInstantiate(&G.exec, g, nullptr, nullptr, 0) != hipSuccess) G.exec = nullptr;
      if (g) (void)hipGraphDestroy(g);
    }
    if (!G.exec) { G.failed = true; (void)hipGetLastError(); ctx->err.clear(); }
    else G.key = key;
    rc = VILO_OK;
  }
  VILO_HIP(hipEventRecord(ctx->ev0, ctx->stream));
  if (want_graph && G.exec) {
    VILO_HIP(hipGraphLaunch(G.exec, ctx->stream));
    bt->path[6] = 1;
  } else {
    rc = vilo_solve_launch(ctx, bt->d, opts, plan);
    if (rc != VILO_OK) return rc;
    bt->path[6] = 0;
  }
  const int32_t forms[6] = {plan.visual, plan.imu, plan.imu_order, plan.assembly, plan.solver, plan.rows};
  memcpy(bt->path, forms, sizeof(forms));
  bt->path[7] = vilo::tuning().wave_order;
  ++bt->n_solves;
  VILO_HIP(hipEventRecord(ctx->ev1, ctx->stream));
  VILO_HIP(hipEventSynchronize(ctx->ev1));
  float ms = 0.f;
  VILO_HIP(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
  ctx->last_solve_ms = ms;
  if (ctx->prep_pending) {   // (recorded on this stream before ev1: complete)
    float t = 0.f;
    if (hipEventElapsedTime(&t, ctx->prep_ev[0], ctx->prep_ev[1]) == hipSuccess) { ctx->kernel_ms[VILO_K_PREPARE_PREINT] += t; ctx->kernel_launches[VILO_K_PREPARE_PREINT] += 1; }
    ctx->prep_pending = false;
  }
  if (ctx->profile) {
    for (size_t i = 0; i < ctx->pev_kind.size(); ++i) {
      float t = 0.f;
      if (hipEventElapsedTime(&t, ctx->pev[2 * i], ctx->pev[2 * i + 1]) == hipSuccess) {
        ctx->kernel_ms[ctx->pev_kind[i]] += t;
        ctx->kernel_launches[ctx->pev_kind[i]] += 1;
      }
    }
  }
  return VILO_OK;
}

extern "C" int vilo_debug_batch_path(const vilo_batch *bt, int32_t out[8]) {
  if (!bt || !out || bt->n_solves < 1) return VILO_ERR_BAD_ARG;
  memcpy(out, bt->path, sizeof(bt->path));
  return VILO_OK;
}

extern "C" int vilo_batch_download(vilo_ctx *ctx, vilo_batch *bt, vilo_window_state *out, vilo_solve_summary *summ) {
  if (!ctx || !bt) return VILO_ERR_BAD_ARG;
  VILO_HIP(hipSetDevice(ctx->device));
  const int W = bt->W;
  const auto t_dl0 = std::chrono::steady_clock::now();
  struct DlTimer { vilo_ctx *c; std::chrono::steady_clock::time_point t0; ~DlTimer() { c->last_download_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); } } dl_timer{ctx, t_dl0};
  VILO_HIP(hipStreamSynchronize(ctx->stream));
  if (out) {
    std::vector<double> x((size_t)W * XSTRIDE), lam((size_t)std::max(1, bt->d.n_lm));
    VILO_HIP(hipMemcpy(x.data(), bt->d.x, sizeof(double) * x.size(), hipMemcpyDeviceToHost));
    if (bt->d.n_lm > 0) VILO_HIP(hipMemcpy(lam.data(), bt->d.lam, sizeof(double) * (size_t)bt->d.n_lm, hipMemcpyDeviceToHost));
    std::vector<WinMeta> wins(W);
    VILO_HIP(hipMemcpy(wins.data(), bt->d.win, sizeof(WinMeta) * W, hipMemcpyDeviceToHost));
    for (int w = 0; w < W; ++w) {
      const double *xw = &x[(size_t)w * XSTRIDE];
      const int F = wins[w].n_frames;
      memcpy(out[w].pose, xw + XO_POSE, sizeof(double) * 7 * F);
      memcpy(out[w].speed_bias, xw + XO_SB, sizeof(double) * 9 * F);
      memcpy(out[w].leg_bias, xw + XO_LB, sizeof(double) * 4 * F);
      memcpy(out[w].ex_pose, xw + XO_EX, sizeof(double) * 14);
      out[w].td[0] = xw[XO_TD];
      for (int i = 0; i < bt->lm.L[w]; ++i) out[w].inv_depth[bt->lm.perm[bt->lm.lm_off[w] + i]] = lam[bt->lm.lm_off[w] + i];
    }
  }
  if (summ) {
    std::vector<SolverState> st(W);
    VILO_HIP(hipMemcpy(st.data(), bt->d.st, sizeof(SolverState) * W, hipMemcpyDeviceToHost));
    for (int w = 0; w < W; ++w) {
      vilo_solve_summary &s = summ[w];
      memset(&s, 0, sizeof(s));
      s.iterations = st[w].iter; s.num_successful = st[w].num_successful; s.termination = st[w].termination;
      s.initial_cost = st[w].cost_trace[0]; s.final_cost = st[w].x_cost;
      memcpy(s.cost_trace, st[w].cost_trace, sizeof(s.cost_trace));
      memcpy(s.radius_trace, st[w].radius_trace, sizeof(s.radius_trace));
    }
  }
  return VILO_OK;
}

// host wall time inside the last vilo_batch_create of this context: [0] total, [1] packing, [2] allocation + upload of observations /
// states / priors, [3] preintegration records up + sqrt_info; and the bytes it moved to the device
extern "C" int vilo_last_create_ms(const vilo_ctx *ctx, double out_ms[4], double *bytes_up) {
  if (!ctx || !out_ms) return VILO_ERR_BAD_ARG;
  for (int i = 0; i < 4; ++i) out_ms[i] = ctx->last_create_ms[i];
  if (bytes_up) *bytes_up = ctx->last_create_bytes;
  return VILO_OK;
}
extern "C" double vilo_last_download_ms(const vilo_ctx *ctx) { return ctx ? ctx->last_download_ms : -1.0; }

// Test / profiling hook: copy an internal device array of window `win` to the host. Not part of the
// reference's interface. what: 0 gram slots, 1 lm_E, 2 lm_g, 3 lm_w (80 x L), 4 cam_g, 5 cam_dh2, 6 cam_y,
// 7 imu_lin, 8 lm_y, 9 lm_dh2, 10 SolverState scalars + cost trace (24 + 64 doubles), 11 landmark permutation (as doubles),
// 13 the preintegration records (10 x vilo_preint), 14 lm_g of the buffer the current linearisation does NOT use (after an accepted last
// step whose candidate was only costed: the gradients that go with lm_E and lm_w, which have one buffer; what 2 reads is unwritten then),
// 15 the prepared records (10 x PreintPrepared), 16 the records of an IMU-only batch (10 x vilo_preint_imu), 17 [records' form, from a pool]
extern "C" int vilo_debug_fetch(vilo_ctx *ctx, vilo_batch *bt, int what, int win, double *out, int max_n) {
  if (!ctx || !bt || win < 0 || win >= bt->W || !out) return VILO_ERR_BAD_ARG;
  VILO_HIP(hipSetDevice(ctx->device));
  VILO_HIP(hipStreamSynchronize(ctx->stream));
  WinMeta wm;
  VILO_HIP(hipMemcpy(&wm, bt->d.win + win, sizeof(WinMeta), hipMemcpyDeviceToHost));
  const double *src = nullptr;
  size_t n = 0;
  switch (what) {
    case 0: src = bt->d.gram + (size_t)wm.gram_off * VILO_GRAM; n = (size_t)wm.n_gram * VILO_GRAM; break;
    case 1: src = bt->d.lm_E + wm.lm_off; n = wm.L; break;
    case 2:
    case 14: {
      SolverState sst;
      VILO_HIP(hipMemcpy(&sst, bt->d.st + win, sizeof(SolverState), hipMemcpyDeviceToHost));
      src = bt->d.lm_gbuf[(sst.cur ^ (what == 14)) & 1] + wm.lm_off; n = wm.L; break;
    }
    case 3: src = bt->d.lm_w + 80 * (size_t)wm.lm_off; n = (size_t)80 * wm.L; break;
    case 4: src = bt->d.cam_g + (size_t)win * CD_N; n = CD_N; break;
    case 5: src = bt->d.cam_dh2 + (size_t)win * CD_N; n = CD_N; break;
    case 6: src = bt->d.cam_y + (size_t)win * CD_N; n = CD_N; break;
    case 7: src = bt->d.imu_lin + (size_t)win * 10 * 31 * 39; n = 10 * 31 * 39; break;
    case 8: src = bt->d.lm_y + wm.lm_off; n = wm.L; break;
    case 9: src = bt->d.lm_dh2 + wm.lm_off; n = wm.L; break;
    case 10: src = (const double *)(bt->d.st + win); n = 24 + 64; break;
    case 12: src = (const double *)(bt->d.st + win) + 24 + 128 + 1; n = 63; break;   // phase_clk (int64 bit patterns)
    case 13:   // the window's preintegration records as they stand (vilo_preint x 10; with vilo_batch_set_samples: the last re-integration)
      if (!bt->rec.leg || !bt->rec.d_pre) return VILO_ERR_UNSUPPORTED;
      src = (const double *)((const vilo_preint *)bt->rec.d_pre + (size_t)win * 10); n = 10 * sizeof(vilo_preint) / sizeof(double); break;
    case 15:   // the window's prepared records (10 x PreintPrepared: head + sqrt_info), entries of intervals without a factor as they lie
      src = (const double *)(bt->d.prep + (size_t)win * 10); n = 10 * sizeof(PreintPrepared) / sizeof(double); break;
    case 16:   // what 13 is for a batch of IMU-only windows (vilo_preint_imu x 10)
      if (bt->rec.leg || !bt->rec.d_pre) return VILO_ERR_UNSUPPORTED;
      src = (const double *)((const vilo_preint_imu *)bt->rec.d_pre + (size_t)win * 10); n = 10 * sizeof(vilo_preint_imu) / sizeof(double); break;
    case 17: {   // BatchRecords::form of the records (0 full, 1 compact upload, 2 mixed) and whether they came from a pool
      if (max_n < 2) return VILO_ERR_BAD_ARG;
      out[0] = bt->rec.form; out[1] = bt->rec.from_pool ? 1.0 : 0.0;
      return 2;
    }
    // the bias chain's hand-over buffers as the last linearisation left them: M_k, T_A(k) ([11][13][13]), T(k) in MFMA operand order + the
    // reduced right-hand side ([TK_N]: tiles left of chain_x_lo and the padding rows are never written)
    case 18: src = bt->d.Lk + (size_t)win * 11 * 169; n = 11 * 169; break;
    case 19: src = bt->d.TAg + (size_t)win * 11 * 169; n = 11 * 169; break;
    case 20: src = bt->d.Tk + (size_t)win * TK_N; n = TK_N; break;
    case 11: {
      n = wm.L;
      if ((int)n > max_n) return VILO_ERR_BAD_ARG;
      for (size_t i = 0; i < n; ++i) out[i] = bt->lm.perm[bt->lm.lm_off[win] + i];
      return (int)n;
    }
    default: return VILO_ERR_BAD_ARG;
  }
  if ((long long)n > max_n) return VILO_ERR_BAD_ARG;
  if (n) VILO_HIP(hipMemcpy(out, src, n * sizeof(double), hipMemcpyDeviceToHost));
  return (int)n;
}
