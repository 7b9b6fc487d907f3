// The resident batch (vilo_batch) as every .hip file of the library sees it: the device tables the kernels read (BatchDev) and six parts,
// each with the state of one concern and the few operations on it. State that outlives a call goes into a part; state of one call goes
// into its BatchCall (batch_call.hpp). Members without a body here live in vilo_batch.hip.
#pragma once
#include <algorithm>

#include "solver_types.hpp"

// Device memory of a batch: bump allocation out of 64 MB (or larger) chunks, which come from and go back to ctx->pool_free
struct BatchArena {
  std::vector<std::pair<void *, size_t>> chunks;
  char *cur = nullptr;
  size_t cur_left = 0, used = 0;   // used: bytes handed out of the chunks (vilo_debug_batch_device_bytes)
  int alloc_bytes(vilo_ctx *ctx, void **p, size_t bytes);   // 256-byte aligned
  template <class T> int alloc(vilo_ctx *ctx, T **p, size_t n) {
    void *q = nullptr;
    int rc = alloc_bytes(ctx, &q, std::max<size_t>(n, 1) * sizeof(T));
    *p = (T *)q;
    return rc;
  }
  template <class T> int upload_raw(vilo_ctx *ctx, T **p, const T *h, size_t n) {
    int rc = alloc(ctx, p, n);
    if (rc != VILO_OK) return rc;
    if (n) VILO_HIP(hipMemcpy(*p, h, n * sizeof(T), hipMemcpyHostToDevice));
    return VILO_OK;
  }
  template <class T> int upload(vilo_ctx *ctx, T **p, const std::vector<T> &h) { return upload_raw(ctx, p, h.data(), h.size()); }
};
// Per-call device memory of a batch call: bump-allocated out of the batch's arena, all of it given back when the scope closes, on every
// return path. Closing waits for the context's stream first (batch uploads are null-stream copies, which do not wait for it), then hands
// the arena chunks taken since opening back to ctx->pool_free and rewinds the bump pointer. Bump allocation never moves what it has handed
// out, so a buffer may be sized partway through a call. The rule: nothing that must outlive the call is allocated inside a scope. The
// calls that query a resident batch do not open one by hand: batch_call.hpp's BatchCall owns the scope, allocates the blocks its
// CallLayout lists in one piece, and carries the timed region and the downloads around the call's kernels.
struct ArenaScope {
  ArenaScope(vilo_ctx *ctx, vilo_batch *bt);
  ~ArenaScope();
  ArenaScope(const ArenaScope &) = delete;
  ArenaScope &operator=(const ArenaScope &) = delete;
  void *alloc(size_t bytes);   // 256-byte aligned; null (ctx->err set) when the device has no memory left
  vilo_ctx *ctx;
  vilo_batch *bt;
  size_t n_chunks, cur_left, used;
  char *cur;
};

// The host's landmark tables, concatenated by window in device order
struct BatchLandmarks {
  std::vector<int> lm_off;   // per window: where its landmarks start
  std::vector<int> perm;     // device order -> original landmark index within its window
  std::vector<int> L;        // per window
  int max_win_waves = 0;     // most packed visual waves of one window (vilo_batch_frame_pose_pnp sizes its LDS by it)
  // the caller's observation row of each landmark's first observation (a window without landmarks has none); on the device from the
  // first obs_rows() on: batch data, uploaded outside any call's scope
  std::vector<int> obs_row;
  int n_obs_rows = 0;
  int *d_obs_row = nullptr;
  int obs_rows(vilo_ctx *ctx, BatchArena &arena, const int **rows);
};

// The preintegration records in force ([W * 10] vilo_preint when leg, else vilo_preint_imu) and where they came from
struct BatchRecords {
  void *d_pre = nullptr;
  bool leg = true;
  bool from_pool = false;       // gathered from a vilo_preint_streams pool
  // 0 full records, 1 uploaded in the compact 739-double form (entries no factor reads are zero, the covariance's lower triangle mirrors
  // the upper), 2 such a batch after a re-propagation that left some records in that form
  int form = 0;
  int *d_prep_bad = nullptr;    // [W * 10] covariance of this record not positive definite
  vilo_preint *orig = nullptr;  // [W * 10] the records vilo_batch_set_samples(NULL) brings back, kept from the first vilo_batch_set_samples on
  // sample buffers of vilo_batch_set_samples: reused by later calls while they are large enough (the arena cannot free)
  vilo_sample *rp_s = nullptr; int *rp_o = nullptr; double *rp_t = nullptr; size_t rp_cap = 0;
  double *rp_ff = nullptr;      // [W * 10][VILO_FF_N]
  double *rp_ff0 = nullptr;     // the same right after the objects' first integration: what vilo_batch_reset brings back (contact_sensor_type 2)
  // win_bad[w] = any live interval of window w whose covariance had no sqrt_info (prep_bad, written by the preparation): one launch on
  // the context's stream
  int fold_win_bad(vilo_ctx *ctx, BatchDev &d);
  // records were overwritten and prepared again (prep_bad of each rewritten): they are what vilo_batch_set_samples(NULL) brings back from
  // here on, and win_bad is folded again (asynchronous on the context's stream); then, once the caller knows: all_live = no live record
  // is left in the compact form
  int replaced(vilo_ctx *ctx, BatchDev &d);
  void full(bool all_live) { if (form) form = all_live ? 0 : 2; }
};

// vilo_batch_mask_landmarks (kernels_mask.hip): the flag image as uploaded and the mask in force (device order), one arena block from the
// first store() on (batch data, outside any call's scope), and the mask's host mirror (device order, as BatchLandmarks::perm: what the
// marginalisation's host tables read)
struct BatchMask {
  size_t flags_total = 0;
  unsigned char *d_flags_orig = nullptr, *d_mask = nullptr;
  std::vector<unsigned char> mirror;
  int n_masked = 0;            // landmarks the mirror masks
  bool mirror_stale = false;   // a mask call failed after its kernels were launched: the mirror may not be the device's mask
  int store(vilo_ctx *ctx, BatchArena &arena, const BatchDev &d);
  // the mirror was rewritten (mirror_valid), or the device's mask may have been and the mirror was not (a HIP error inside a mask call):
  // stale() then fails (VILO_ERR_HIP, vilo_last_error set) until a mask call has gone through, and so does refuse()
  void changed(bool mirror_valid);
  int stale(vilo_ctx *ctx, const char *call) const;
  // VILO_ERR_UNSUPPORTED with vilo_last_error set while any landmark is masked (the calls that do not honour a mask)
  int refuse(vilo_ctx *ctx, const char *call) const;
  // the mirror from landmark lm_off on (a window's BatchLandmarks::lm_off) while any landmark is masked, else null
  const unsigned char *host(int lm_off) const { return n_masked > 0 ? mirror.data() + lm_off : nullptr; }
};

// vilo_batch_save_state / vilo_batch_restore_state (kernels_retract.hip): the one snapshot slot of a batch, a second copy of x and lam,
// one arena block from the first save() on (batch data, outside any call's scope)
struct BatchSnapshot {
  double *d_x = nullptr, *d_lam = nullptr;   // [W][XSTRIDE], [n_lm]
  bool saved = false;                        // a save has gone through: the slot holds a state
  int save(vilo_ctx *ctx, BatchArena &arena, const BatchDev &d);
  // VILO_ERR_UNSUPPORTED with vilo_last_error set before the first save
  int restore(vilo_ctx *ctx, const BatchDev &d) const;
};

// The launch sequence of one solve (5 + 7 x max_num_iterations kernels) as a hipGraph, captured when the same resident batch is solved a
// second time (vilo_batch_reset + vilo_batch_solve loops: replays, Monte-Carlo seeds, bench), and everything that sequence depends on
struct SolveGraph {
  struct Key {
    vilo_solve_opts opts; int sqrt_info_mode, rp_on; double initial_mu; vilo::SolvePlan plan;
    bool operator==(const Key &o) const {   // (the options byte by byte, padding included)
      return memcmp(&opts, &o.opts, sizeof(opts)) == 0 && sqrt_info_mode == o.sqrt_info_mode && rp_on == o.rp_on && initial_mu == o.initial_mu && plan == o.plan;
    }
  };
  hipGraphExec_t exec = nullptr;
  bool failed = false;   // a capture did not come through: this batch launches kernel by kernel from then on
  Key key;               // what exec was captured with
  void drop() { if (exec) { (void)hipGraphExecDestroy(exec); exec = nullptr; } }
};

struct vilo_batch {
  BatchDev d;
  int W, n_solves = 0;
  int32_t path[8] = {-1, -1, -1, -1, -1, -1, -1, -1};   // vilo_debug_batch_path: the plan of the last solve, replay or not, the wave order
  BatchArena arena;
  BatchLandmarks lm;
  BatchRecords rec;
  BatchMask mask;
  BatchSnapshot snap;
  SolveGraph graph;
};
