// C ABI (include/nrms_hip.h): argument validation, workspace carving and the
// stage order of the NRMS encoders. Every call only enqueues work on the
// caller's stream (no allocation, no synchronisation); the only globals are the
// process-wide GEMM arithmetic and the once-per-(device, kernel) LDS attribute.
#include "nrms_common.hpp"
#include "titles.hpp"

#include <atomic>
#include <cstdlib>
#include <mutex>
#include <set>
#include <tuple>

namespace nrms {

static thread_local int32_t g_last_hip = 0;
void set_last_hip_error(hipError_t e) { g_last_hip = (int32_t)e; }

static int initial_gemm_arith() {
  const char* e = env_knob("NRMS_GEMM");
  if (e && (e[0] == 'f' || e[0] == 'F')) return NRMS_GEMM_F32;
  if (e && (e[0] == 'x' || e[0] == 'X')) return NRMS_GEMM_SPLIT_BF16X6;
  return NRMS_GEMM_SPLIT_F16X3;
}
static std::atomic<int> g_gemm_arith{initial_gemm_arith()};
// test only (tests/test_gpu_parity.py): classification half A in the pack
// launch but no tail jobs in the projection, so the news launch classifies
// again itself -- the fallback nrms_forward takes when the projection leaves
// its fragment path after the pack
static const bool g_skip_classify_tail = [] {
  const char* e = env_knob("NRMS_TEST_SKIP_CLASSIFY_TAIL");
  return e && e[0] == '1';
}();
static thread_local int32_t t_gemm_arith = -1;   // nrms_set_thread_gemm_arith (-1: none)
int gemm_arith() {
  const int32_t t = t_gemm_arith;
  return t >= 0 ? t : g_gemm_arith.load(std::memory_order_relaxed);
}

void ensure_dynamic_lds(const void* fn, int bytes) {
  static std::mutex mu;
  static std::set<std::tuple<int, const void*, int>> done;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return;
  std::lock_guard<std::mutex> lock(mu);
  if (done.insert(std::make_tuple(dev, fn, bytes)).second)
    (void)hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
}

namespace {

constexpr int kDK = 20;   // d_k = D / H supported by the attention kernel
constexpr int kQMax = 208;

size_t align_up(size_t x) { return (x + 255) & ~(size_t)255; }

// Bump allocator over the caller's workspace. Every workspace and state
// buffer has one layout routine, which takes a Carve and returns the named
// pointers: run over() the caller's buffer it carves; run measuring (no base:
// only off advances) it gives the size that buffer needs.
struct Carve {
  char* base;
  size_t cap, off = 0;
  bool ok = true;
  static Carve over(void* buf, size_t bytes) { return Carve{static_cast<char*>(buf), buf ? bytes : 0}; }
  float* floats(size_t n) {
    const size_t need = align_up(n * sizeof(float));
    if (need > cap - off) { ok = false; return nullptr; }
    float* p = base ? reinterpret_cast<float*>(base + off) : nullptr;
    off += need;
    return p;
  }
};
template <class Layout>
size_t measure(Layout&& layout) {
  Carve cv{nullptr, SIZE_MAX};
  layout(cv);
  return cv.off;
}

bool weights_ok(const nrms_encoder_weights_t* w) {
  if (!w) return false;
  if (!w->w_q || !w->b_q || !w->w_k || !w->b_k || !w->w_v || !w->b_v || !w->w_add ||
      !w->b_add || !w->q_add)
    return false;
  return w->d_model > 0 && w->n_heads > 0 && w->query_dim > 0;
}

int32_t shape_ok(const nrms_encoder_weights_t* w) {
  if (!weights_ok(w)) return NRMS_ERR_INVALID_ARG;
  if (w->d_model % w->n_heads != 0) return NRMS_ERR_INVALID_ARG;  // multihead_self.py:31
  if (w->d_model / w->n_heads != kDK || w->n_heads != 15) return NRMS_ERR_UNSUPPORTED;
  if (w->query_dim > kQMax || w->d_model % 4 != 0) return NRMS_ERR_UNSUPPORTED;
  return NRMS_OK;
}

WeightRows qkv_rows(const nrms_encoder_weights_t* w) {
  WeightRows r{};
  r.w[0] = w->w_q; r.w[1] = w->w_k; r.w[2] = w->w_v;
  r.b[0] = w->b_q; r.b[1] = w->b_k; r.b[2] = w->b_v;
  r.seg_rows = w->d_model;
  r.nseg = 3;
  return r;
}

// one bias-free segment of `rows` rows (the backward GEMMs' transposed weights)
WeightRows one_segment(const float* w, int rows, int accumulate) {
  WeightRows r{};
  r.w[0] = w;
  r.seg_rows = rows;
  r.nseg = 1;
  r.accumulate = accumulate;
  return r;
}

// q|k|v row stride of the hot path (nrms_qkv_row_stride; 3D since round 3)
int64_t hot_ld(bool fused, int32_t D) { return fused ? qkv_row_stride(D) : 3 * (int64_t)D; }
int64_t news_ld(const nrms_encoder_weights_t* w, int32_t L) {
  return hot_ld(fused_news_supported(L, w->d_model, w->n_heads, w->query_dim), w->d_model);
}
int64_t user_ld(const nrms_encoder_weights_t* w, int32_t N) {
  return hot_ld(fused_user_supported(N, w->d_model, w->n_heads, w->query_dim), w->d_model);
}

bool use_folded(int32_t mode, int64_t n_tok, int64_t V) {
  if (mode == NRMS_PROJ_FOLDED) return true;
  if (mode == NRMS_PROJ_DIRECT) return false;
  return n_tok > V;
}

// One encoder's workspace (nrms_news_encode[_folded], nrms_user_encode, and
// both inside the forward's).
struct EncodeWs {
  float* qkv;      // projected rows, nrms_qkv_row_stride apart
  float* ctx;      // stage kernels: attention context [rows][D]
  float* scores;   // ... and additive scores [rows]
  float* wap;      // the fused tail's workspace (packed W_add first)
  float* pack;     // split Q|K|V weights (proj_x6_pack_floats)
};
// rows: tokens (news) or clicked titles (user). qkv_rows: their own rows, V (the
// folded table), or 0 with pack_floats 0 (the table is the caller's:
// nrms_news_encode_folded; the state's: the prepared folded forward).
EncodeWs encode_layout(Carve& cv, size_t qkv_rows, size_t rows, int32_t D, size_t wap_floats, size_t pack_floats) {
  EncodeWs z{};
  z.qkv = cv.floats(qkv_rows * (size_t)qkv_row_stride(D));
  z.ctx = cv.floats(rows * (size_t)D);
  z.scores = cv.floats(rows);
  z.wap = cv.floats(wap_floats);
  z.pack = cv.floats(pack_floats);
  return z;
}
EncodeWs news_encode_layout(Carve& cv, int64_t n_titles, int32_t L, int64_t qkv_rows, int32_t D) {
  return encode_layout(cv, qkv_rows, (size_t)n_titles * (size_t)L, D, fused_news_workspace_floats(n_titles),
                       proj_x6_pack_floats());
}
EncodeWs user_encode_layout(Carve& cv, int64_t B, int32_t N, int32_t D) {
  return encode_layout(cv, (size_t)B * N, (size_t)B * N, D, fused_user_packed_b_floats(), proj_x6_pack_floats());
}

// nrms_forward[_prepared]'s workspace: both encoders', the news and user
// vectors between them, and the UserEncoder's row list and dispatch order.
// (A prepared step carves the buffers its state replaces all the same.)
struct ForwardWs {
  EncodeWs n;
  float* news;   // [clicked B*N | candidates B*C] x D
  float* user;   // [B][D]
  EncodeWs u;
  int64_t* ulist;    // [B*N] launch_user_row_list's rows
  int32_t* uorder;   // [B] user dispatch order
};
ForwardWs forward_layout(Carve& cv, int64_t B, int32_t C, int32_t N, int32_t L, int64_t qkv_rows, int32_t D) {
  const int64_t n_all = B * (C + N);
  ForwardWs z{};
  z.n = news_encode_layout(cv, n_all, L, qkv_rows, D);
  z.news = cv.floats((size_t)n_all * D);
  z.user = cv.floats((size_t)B * D);
  z.u = user_encode_layout(cv, B, N, D);
  z.ulist = reinterpret_cast<int64_t*>(cv.floats((size_t)B * N * 2));
  z.uorder = reinterpret_cast<int32_t*>(cv.floats((size_t)B));
  return z;
}
size_t forward_bytes(int64_t B, int32_t C, int32_t N, int32_t L, int64_t qkv_rows, int32_t D) {
  if (B < 0 || C < 0 || N <= 0 || L <= 0 || qkv_rows < 0 || D <= 0) return 0;
  return measure([&](Carve& cv) { forward_layout(cv, B, C, N, L, qkv_rows, D); });
}

// The weight-derived buffers of a forward: the folded table, both encoders'
// split Q|K|V weights and both packed W_add -- carved from a caller's state
// buffer (nrms_forward_prepare / nrms_forward_prepared) or part of
// nrms_forward's own workspace.
struct WeightState {
  float* table;   // [V][ld] (null: none)
  float* pack;    // news Q|K|V (proj_x6_pack_floats)
  float* upack;   // user Q|K|V
  float* nwap;    // news W_add planes + the zero / NaN rows (fused_news_packed_floats)
  float* uwap;    // user W_add (fused_user_packed_b_floats)
};
WeightState state_layout(Carve& cv, int64_t V, int32_t D, bool with_table) {
  WeightState ws{};
  if (with_table) ws.table = cv.floats((size_t)V * (size_t)qkv_row_stride(D));
  ws.pack = cv.floats(proj_x6_pack_floats());
  ws.upack = cv.floats(proj_x6_pack_floats());
  ws.nwap = cv.floats(fused_news_packed_floats());
  ws.uwap = cv.floats(fused_user_packed_b_floats());
  return ws;
}

// The training calls' workspaces.
struct AdditiveBackwardWs {
  float *dz, *waT, *part_rows, *part_tn;
};
AdditiveBackwardWs additive_backward_layout(Carve& cv, int64_t n_seq, int32_t L, int32_t D, int32_t Q) {
  return {cv.floats((size_t)n_seq * L * Q), cv.floats((size_t)D * Q),   // (braces: in this order)
          cv.floats(additive_backward_part_floats(n_seq, Q)), cv.floats(gemm_tn_part_floats(Q, D))};
}
struct ProjectBackwardWs {
  float *wT, *part_tn;
};
ProjectBackwardWs project_backward_layout(Carve& cv, int32_t D) {
  return {cv.floats((size_t)3 * D * D), cv.floats(gemm_tn_part_floats(3 * D, D))};
}

AdditiveWeights additive(const nrms_encoder_weights_t* w) { return AdditiveWeights{w->w_add, w->b_add, w->q_add}; }

// Q|K|V projection of the encoders: the pre-split-W kernel (proj_x6.hip) when
// the shape and arithmetic allow, packing w into o.pack first unless the
// caller already did (o.packed, with the same arith); the staged GEMM
// otherwise (x6: bitwise the same rows; f16x3: the kernel's scaled split-f16
// arithmetic, the staged GEMM's x6 rows only within rounding).
Launched project_qkv(const ProjRows& in, const nrms_encoder_weights_t* w, float* Y, int64_t ld, hipStream_t s,
                     const ProjOpts& o) {
  const int D = w->d_model;
  const WeightRows wr = qkv_rows(w);
  const int arith = o.arith < 0 ? gemm_arith() : o.arith;
  const bool h3 = arith == NRMS_GEMM_SPLIT_F16X3;
  if (o.pack && arith != NRMS_GEMM_F32 && proj_x6_supported(D, 3 * D, wr) && ((uintptr_t)Y % 16) == 0 &&
      ld % 4 == 0) {
    if (!o.packed)
      if (int32_t st = launch_proj_x6_pack(wr, o.pack, nullptr, nullptr, h3, s)) return st;
    Launched did = launch_proj_x6(in.X, in.n_rows_x, in.ar, in.row_ids, in.M, o.pack, Y, ld, o.list_count, h3, s,
                                  o.tail);
    did.tail_done = did.st == NRMS_OK && o.tail != nullptr;
    return did;
  }
  if (o.list_count)
    return launch_gemm_store_list(in.X, in.n_rows_x, in.row_ids, o.list_count, in.M, D, wr, 3 * D, Y, ld, s);
  return launch_gemm_store_rows(in.X, in.n_rows_x, in.ar, in.row_ids, in.M, D, wr, 3 * D, Y, ld, s);
}

// attention + additive pooling from projected rows (shared by news and user
// paths). o.wap non-null: use the fused news kernel when the geometry allows.
Launched encode_from_qkv(const QkvRows& qkv, TitleIds ids, int32_t L, const nrms_encoder_weights_t* w, float* out,
                         hipStream_t s, const EncodeOpts& o) {
  const int D = w->d_model;
  if (o.wap && fused_news_supported(L, D, w->n_heads, w->query_dim))
    return launch_fused_news(qkv, ids, additive(w), o.wap, out, s, o.news);
  if (o.news.preclassified) return NRMS_ERR_INVALID_ARG;
  if (o.news.direct_rows) ids.a = ids.b = nullptr;   // per-token rows: the ids only classify (fused kernel)
  // stage kernels: any row stride >= 3D (packed rows, or the folded table's
  // rows of nrms_qkv_row_stride)
  int32_t st = launch_mhsa(qkv.p, qkv.ld, qkv.n_rows, ids.a, ids.n_a, ids.b, ids.n, L, w->n_heads, kDK, o.ctx, s);
  if (st) return st;
  st = launch_gemm_additive_score(o.ctx, ids.n * L, D, w->w_add, w->b_add, w->q_add, w->query_dim, o.scores, s);
  if (st) return st;
  return launch_additive_pool(o.ctx, o.scores, ids.n, L, D, out, s);
}

}  // namespace
}  // namespace nrms

using namespace nrms;

extern "C" {

int32_t nrms_abi_version(void) { return NRMS_ABI_VERSION; }

int32_t nrms_set_gemm_arith(int32_t mode) {
  if (mode != NRMS_GEMM_SPLIT_BF16X6 && mode != NRMS_GEMM_F32 && mode != NRMS_GEMM_SPLIT_F16X3)
    return -NRMS_ERR_INVALID_ARG;
  return g_gemm_arith.exchange(mode);
}

int32_t nrms_get_gemm_arith(void) { return gemm_arith(); }

int32_t nrms_set_title_dedupe(int32_t on) { return set_title_dedupe(on); }

int32_t nrms_set_token_compaction(int32_t on) { return set_token_compaction(on); }

int32_t nrms_set_thread_gemm_arith(int32_t mode) {
  if (mode != -1 && mode != NRMS_GEMM_SPLIT_BF16X6 && mode != NRMS_GEMM_F32 && mode != NRMS_GEMM_SPLIT_F16X3)
    return -NRMS_ERR_INVALID_ARG;
  const int32_t prev = t_gemm_arith;
  t_gemm_arith = mode;
  return prev;
}

int32_t nrms_set_thread_title_dedupe(int32_t on) {
  if (on < -1) return -NRMS_ERR_INVALID_ARG;
  return set_thread_title_dedupe(on);
}

int32_t nrms_set_thread_token_compaction(int32_t on) {
  if (on < -1) return -NRMS_ERR_INVALID_ARG;
  return set_thread_token_compaction(on);
}

const char* nrms_status_string(int32_t st) {
  switch (st) {
    case NRMS_OK: return "ok";
    case NRMS_ERR_INVALID_ARG: return "invalid argument";
    case NRMS_ERR_UNSUPPORTED: return "unsupported shape or alignment";
    case NRMS_ERR_WORKSPACE: return "workspace missing or too small";
    case NRMS_ERR_HIP: return "HIP launch failed";
    default: return "unknown status";
  }
}

int32_t nrms_last_hip_error(void) { return g_last_hip; }

int32_t nrms_embedding_gather(const int64_t* ids, int64_t n_tok, const float* table, int64_t V,
                              int32_t D, float* out, hipStream_t stream) {
  if (n_tok < 0 || V < 0 || D <= 0) return NRMS_ERR_INVALID_ARG;
  if (n_tok > 0 && (!ids || !table || !out)) return NRMS_ERR_INVALID_ARG;
  return launch_gather(ids, n_tok, table, V, D, out, stream);
}

int32_t nrms_qkv_row_stride(int32_t D) { return D > 0 ? (int32_t)qkv_row_stride(D) : 0; }

int32_t nrms_qkv_project(const float* x, int64_t n_rows_x, const int64_t* row_ids, int64_t M,
                         const nrms_encoder_weights_t* w, float* qkv, int64_t ld_qkv,
                         hipStream_t stream) {
  if (M < 0 || n_rows_x < 0) return NRMS_ERR_INVALID_ARG;
  if (int32_t st = shape_ok(w)) return st;
  if (M > 0 && (!x || !qkv)) return NRMS_ERR_INVALID_ARG;
  const int D = w->d_model;
  if (ld_qkv == 0) ld_qkv = 3 * D;
  if (ld_qkv < 3 * D) return NRMS_ERR_INVALID_ARG;
  return launch_gemm_store(x, n_rows_x, row_ids, M, D, qkv_rows(w), 3 * D, qkv, ld_qkv, stream);
}

size_t nrms_qkv_project_workspace_size(int32_t D) {
  return D > 0 ? measure([](Carve& cv) { cv.floats(proj_x6_pack_floats()); }) : 0;
}

int32_t nrms_qkv_project_ws(const float* x, int64_t n_rows_x, const int64_t* row_ids, int64_t M,
                            const nrms_encoder_weights_t* w, float* qkv, int64_t ld_qkv, void* workspace,
                            size_t workspace_bytes, hipStream_t stream) {
  if (M < 0 || n_rows_x < 0) return NRMS_ERR_INVALID_ARG;
  if (int32_t st = shape_ok(w)) return st;
  if (M > 0 && (!x || !qkv)) return NRMS_ERR_INVALID_ARG;
  const int D = w->d_model;
  if (ld_qkv == 0) ld_qkv = 3 * D;
  if (ld_qkv < 3 * D) return NRMS_ERR_INVALID_ARG;
  if (M == 0) return NRMS_OK;
  Carve cv = Carve::over(workspace, workspace_bytes);
  float* pack = cv.floats(proj_x6_pack_floats());
  if (!cv.ok) return NRMS_ERR_WORKSPACE;
  return project_qkv({x, n_rows_x, contiguous_rows(D), row_ids, M}, w, qkv, ld_qkv, stream, {.pack = pack}).st;
}

int32_t nrms_self_attention(const float* qkv, int64_t n_rows_qkv, const int64_t* tok_ids,
                            int64_t n_seq_a, const int64_t* tok_ids_b, int64_t n_seq, int32_t L,
                            const nrms_encoder_weights_t* w, float* ctx, hipStream_t stream) {
  if (n_seq < 0 || n_seq_a < 0 || L <= 0) return NRMS_ERR_INVALID_ARG;
  if (int32_t st = shape_ok(w)) return st;
  if (n_seq > 0 && (!qkv || !ctx)) return NRMS_ERR_INVALID_ARG;
  return launch_mhsa(qkv, 3 * (int64_t)w->d_model, n_rows_qkv, tok_ids, n_seq_a, tok_ids_b, n_seq, L, w->n_heads, kDK, ctx,
                     stream);
}

int32_t nrms_additive_attention(const float* x, int64_t n_seq, int32_t L,
                                const nrms_encoder_weights_t* w, float* scores_ws, float* out,
                                hipStream_t stream) {
  if (n_seq < 0 || L <= 0) return NRMS_ERR_INVALID_ARG;
  if (int32_t st = shape_ok(w)) return st;
  if (n_seq > 0 && (!x || !scores_ws || !out)) return NRMS_ERR_INVALID_ARG;
  const int D = w->d_model;
  int32_t st = launch_gemm_additive_score(x, n_seq * L, D, w->w_add, w->b_add, w->q_add,
                                          w->query_dim, scores_ws, stream);
  if (st) return st;
  return launch_additive_pool(x, scores_ws, n_seq, L, D, out, stream);
}

int32_t nrms_additive_scores(const float* x, int64_t n_rows, const nrms_encoder_weights_t* w,
                             float* scores, hipStream_t stream) {
  if (n_rows < 0) return NRMS_ERR_INVALID_ARG;
  if (int32_t st = shape_ok(w)) return st;
  if (n_rows > 0 && (!x || !scores)) return NRMS_ERR_INVALID_ARG;
  return launch_gemm_additive_score(x, n_rows, w->d_model, w->w_add, w->b_add, w->q_add,
                                    w->query_dim, scores, stream);
}

int32_t nrms_additive_pool(const float* x, const float* scores, int64_t n_seq, int32_t L,
                           int32_t D, float* out, hipStream_t stream) {
  if (n_seq < 0 || L <= 0 || D <= 0) return NRMS_ERR_INVALID_ARG;
  if (n_seq > 0 && (!x || !scores || !out)) return NRMS_ERR_INVALID_ARG;
  return launch_additive_pool(x, scores, n_seq, L, D, out, stream);
}

size_t nrms_news_attention_pool_workspace_size(int64_t n_titles, int32_t L, int32_t D) {
  if (n_titles < 0 || L <= 0 || D <= 0) return 0;
  // (the context stays on chip)
  return measure([&](Carve& cv) { cv.floats(fused_news_workspace_floats(n_titles)); });
}

int32_t nrms_news_attention_pool(const float* qkv, int64_t ld_qkv, int64_t n_rows_qkv,
                                 const int64_t* tok_ids, int64_t n_seq_a, const int64_t* tok_ids_b,
                                 int64_t n_titles, int32_t L, const nrms_encoder_weights_t* w,
                                 float* out, void* workspace, size_t workspace_bytes,
                                 hipStream_t stream) {
  if (n_titles < 0 || n_seq_a < 0 || L <= 0) return NRMS_ERR_INVALID_ARG;
  if (int32_t st = shape_ok(w)) return st;
  if (!fused_news_supported(L, w->d_model, w->n_heads, w->query_dim)) return NRMS_ERR_UNSUPPORTED;
  if (n_titles == 0) return NRMS_OK;
  if (!qkv || !out) return NRMS_ERR_INVALID_ARG;
  Carve cv = Carve::over(workspace, workspace_bytes);
  float* wap = cv.floats(fused_news_workspace_floats(n_titles));
  if (!cv.ok) return NRMS_ERR_WORKSPACE;
  if (ld_qkv == 0) ld_qkv = 3 * (int64_t)w->d_model;
  return launch_fused_news({qkv, ld_qkv, n_rows_qkv}, {tok_ids, n_seq_a, tok_ids_b, n_titles}, additive(w), wap, out,
                           stream).st;
}

size_t nrms_news_encode_workspace_size(int64_t n_titles, int32_t L, int64_t V, int32_t D,
                                       int32_t proj_mode) {
  if (n_titles < 0 || L <= 0 || V < 0 || D <= 0) return 0;
  const int64_t qkv_rows = use_folded(proj_mode, n_titles * L, V) ? V : n_titles * L;
  return measure([&](Carve& cv) { news_encode_layout(cv, n_titles, L, qkv_rows, D); });
}

int32_t nrms_news_encode(const int64_t* ids, int64_t n_titles, int32_t L, const float* table,
                         int64_t V, const nrms_encoder_weights_t* w, int32_t proj_mode, float* out,
                         void* workspace, size_t workspace_bytes, hipStream_t stream) {
  if (n_titles < 0 || L <= 0 || V <= 0) return NRMS_ERR_INVALID_ARG;
  if (int32_t st = shape_ok(w)) return st;
  if (n_titles == 0) return NRMS_OK;
  if (!ids || !table || !out) return NRMS_ERR_INVALID_ARG;
  const int D = w->d_model;
  // Vocabulary-level projection: one GEMM over the table, then rows gathered by
  // id; or per-token projection with the embedding gather fused into the
  // A-operand load.
  const bool folded = use_folded(proj_mode, n_titles * L, V);
  const int64_t ld = news_ld(w, L), rows = folded ? V : n_titles * L;
  Carve cv = Carve::over(workspace, workspace_bytes);
  const EncodeWs z = news_encode_layout(cv, n_titles, L, rows, D);
  if (!cv.ok) return NRMS_ERR_WORKSPACE;
  const ProjRows in{table, V, contiguous_rows(D), folded ? nullptr : ids, rows};
  if (int32_t st = project_qkv(in, w, z.qkv, ld, stream, {.pack = z.pack}).st) return st;
  EncodeOpts eo{z.ctx, z.scores, z.wap};
  eo.news.direct_rows = !folded;
  return encode_from_qkv({z.qkv, ld, rows}, {ids, n_titles, nullptr, n_titles}, L, w, out, stream, eo).st;
}

size_t nrms_news_encode_folded_workspace_size(int64_t n_titles, int32_t L, int32_t D) {
  if (n_titles < 0 || L <= 0 || D <= 0) return 0;
  return measure([&](Carve& cv) { encode_layout(cv, 0, (size_t)n_titles * L, D, fused_news_workspace_floats(n_titles), 0); });
}

int32_t nrms_news_encode_folded(const int64_t* ids, int64_t n_titles, int32_t L,
                                const float* qkv_table, int64_t ld_qkv, int64_t V,
                                const nrms_encoder_weights_t* w, float* out, void* workspace,
                                size_t workspace_bytes, hipStream_t stream) {
  if (n_titles < 0 || L <= 0 || V <= 0) return NRMS_ERR_INVALID_ARG;
  if (int32_t st = shape_ok(w)) return st;
  if (n_titles == 0) return NRMS_OK;
  if (!ids || !qkv_table || !out) return NRMS_ERR_INVALID_ARG;
  Carve cv = Carve::over(workspace, workspace_bytes);
  const EncodeWs z = encode_layout(cv, 0, (size_t)n_titles * L, w->d_model, fused_news_workspace_floats(n_titles), 0);
  if (!cv.ok) return NRMS_ERR_WORKSPACE;
  if (ld_qkv == 0) ld_qkv = 3 * (int64_t)w->d_model;
  return encode_from_qkv({qkv_table, ld_qkv, V}, {ids, n_titles, nullptr, n_titles}, L, w, out, stream,
                         {z.ctx, z.scores, z.wap})
      .st;
}

size_t nrms_user_encode_workspace_size(int64_t B, int32_t N, int32_t D) {
  if (B < 0 || N <= 0 || D <= 0) return 0;
  return measure([&](Carve& cv) { user_encode_layout(cv, B, N, D); });
}

size_t nrms_user_attention_pool_workspace_size(int64_t B, int32_t N, int32_t D) {
  if (B < 0 || N <= 0 || D <= 0) return 0;
  return measure([](Carve& cv) { cv.floats(fused_user_packed_b_floats()); });
}

int32_t nrms_user_attention_pool(const float* qkv, int64_t ld_qkv, int64_t B, int32_t N,
                                 const nrms_encoder_weights_t* w, float* out, void* workspace,
                                 size_t workspace_bytes, hipStream_t stream) {
  if (B < 0 || N <= 0) return NRMS_ERR_INVALID_ARG;
  if (int32_t st = shape_ok(w)) return st;
  if (!fused_user_supported(N, w->d_model, w->n_heads, w->query_dim)) return NRMS_ERR_UNSUPPORTED;
  if (B == 0) return NRMS_OK;
  if (!qkv || !out) return NRMS_ERR_INVALID_ARG;
  Carve cv = Carve::over(workspace, workspace_bytes);
  float* wap = cv.floats(fused_user_packed_b_floats());
  if (!cv.ok) return NRMS_ERR_WORKSPACE;
  if (ld_qkv == 0) ld_qkv = 3 * (int64_t)w->d_model;
  return launch_fused_user({qkv, ld_qkv}, B, N, additive(w), wap, out, stream);
}

int32_t nrms_user_attention_pool_padded(const float* qkv, int64_t ld_qkv, int64_t B, int32_t N,
                                        const uint8_t* pad_flags, const nrms_encoder_weights_t* w, float* out,
                                        void* workspace, size_t workspace_bytes, hipStream_t stream) {
  if (B < 0 || N <= 0) return NRMS_ERR_INVALID_ARG;
  if (int32_t st = shape_ok(w)) return st;
  if (!fused_user_supported(N, w->d_model, w->n_heads, w->query_dim)) return NRMS_ERR_UNSUPPORTED;
  if (B == 0) return NRMS_OK;
  if (!qkv || !out || !pad_flags) return NRMS_ERR_INVALID_ARG;
  Carve cv = Carve::over(workspace, workspace_bytes);
  float* wap = cv.floats(fused_user_packed_b_floats());
  if (!cv.ok) return NRMS_ERR_WORKSPACE;
  if (ld_qkv == 0) ld_qkv = 3 * (int64_t)w->d_model;
  const bool compact = token_compaction() && N <= 64;
  const PaddingGroups pg{pad_flags, nullptr, nullptr};   // (no rep: every flagged row was projected)
  return launch_fused_user({qkv, ld_qkv}, B, N, additive(w), wap, out, stream,
                           {.pg = compact ? &pg : nullptr, .compact = compact});
}

int32_t nrms_user_encode(const float* clicked, int64_t B, int32_t N, int64_t stride_b,
                         int64_t stride_n, const nrms_encoder_weights_t* w, float* out,
                         void* workspace, size_t workspace_bytes, hipStream_t stream) {
  if (B < 0 || N <= 0 || stride_b < 0 || stride_n < 0) return NRMS_ERR_INVALID_ARG;
  if (int32_t st = shape_ok(w)) return st;
  if (B == 0) return NRMS_OK;
  if (!clicked || !out) return NRMS_ERR_INVALID_ARG;
  const int D = w->d_model;
  const int64_t rows = B * N;
  Carve cv = Carve::over(workspace, workspace_bytes);
  const int64_t ld = user_ld(w, N);
  const EncodeWs z = user_encode_layout(cv, B, N, D);
  if (!cv.ok) return NRMS_ERR_WORKSPACE;
  // the [B, N, D] view is read in place (e.g. the transpose(0, 1) of
  // src/evaluate.py:220-224: stride_b = D, stride_n = B * D)
  const ARows ar = (stride_b == (int64_t)N * D && stride_n == D) ? contiguous_rows(D)
                                                                 : ARows{N, stride_b, stride_n};
  if (int32_t st = project_qkv({clicked, rows, ar, nullptr, rows}, w, z.qkv, ld, stream, {.pack = z.pack}).st) return st;
  if (fused_user_supported(N, D, w->n_heads, w->query_dim) && ((uintptr_t)out % 16) == 0)
    return launch_fused_user({z.qkv, ld}, B, N, additive(w), z.wap, out, stream);
  return encode_from_qkv({z.qkv, ld, rows}, {nullptr, B, nullptr, B}, N, w, out, stream, {z.ctx, z.scores}).st;
}

int32_t nrms_score(const float* news, int64_t B, int32_t C, int64_t stride_b, int64_t stride_c,
                   const float* user, int64_t stride_u, int32_t D, float* out,
                   hipStream_t stream) {
  if (B < 0 || C < 0 || D <= 0) return NRMS_ERR_INVALID_ARG;
  if (B * C > 0 && (!news || !user || !out)) return NRMS_ERR_INVALID_ARG;
  return launch_score(news, B, C, stride_b, stride_c, user, stride_u, D, out, stream);
}

int32_t nrms_score_pairs(const float* news, int64_t n_news, const float* user, int64_t n_users,
                         const int64_t* news_idx, const int64_t* user_idx, int64_t n_pairs,
                         int32_t D, float* out, hipStream_t stream) {
  if (n_pairs < 0 || n_news < 0 || n_users < 0 || D <= 0) return NRMS_ERR_INVALID_ARG;
  if (n_pairs > 0 && (!news || !user || !news_idx || !user_idx || !out)) return NRMS_ERR_INVALID_ARG;
  return launch_score_pairs(news, n_news, user, n_users, news_idx, user_idx, n_pairs, D, out, stream);
}

// ---- Exp1: category views and position embedding (views.hip)
static int32_t views_weights_status(const nrms_views_weights_t* w) {
  if (!w) return NRMS_ERR_INVALID_ARG;
  if (w->n_cat < 0 || w->emb_dim <= 0 || w->d_model <= 0 || w->query_dim <= 0) return NRMS_ERR_INVALID_ARG;
  if (!w->emb_cat || !w->emb_sub || !w->w_cat || !w->b_cat || !w->w_sub || !w->b_sub || !w->w_fin || !w->b_fin ||
      !w->q_fin)
    return NRMS_ERR_INVALID_ARG;
  if (w->n_cat > ((int64_t)1 << 24) || w->query_dim > kQMax || (int64_t)w->emb_dim + w->d_model > 12280)
    return NRMS_ERR_UNSUPPORTED;
  return NRMS_OK;
}

size_t nrms_views_state_size(int64_t n_cat, int32_t D) {
  if (n_cat < 0 || n_cat > ((int64_t)1 << 24) || D <= 0 || D > 12280) return 0;
  return (size_t)n_cat * (2 * (size_t)D + 2) * sizeof(float);
}

int32_t nrms_views_prepare(const nrms_views_weights_t* w, void* state, size_t state_bytes, hipStream_t stream) {
  if (int32_t st = views_weights_status(w)) return st;
  if (w->n_cat == 0) return NRMS_OK;
  if (!state) return NRMS_ERR_INVALID_ARG;
  if (state_bytes < nrms_views_state_size(w->n_cat, w->d_model)) return NRMS_ERR_WORKSPACE;
  return launch_views_prepare(*w, static_cast<float*>(state), stream);
}

size_t nrms_news_views_fuse_workspace_size(int64_t n) {
  return n <= 0 ? 0 : align_up((size_t)n * sizeof(float));
}

int32_t nrms_news_views_fuse(const float* title_vec, int64_t n, const int64_t* category,
                             const int64_t* subcategory, const nrms_views_weights_t* w, const void* state,
                             float* out, void* workspace, size_t workspace_bytes, hipStream_t stream) {
  if (n < 0) return NRMS_ERR_INVALID_ARG;
  if (int32_t st = views_weights_status(w)) return st;
  if (n == 0) return NRMS_OK;
  if (!title_vec || !category || !subcategory || !state || !out) return NRMS_ERR_INVALID_ARG;
  if (!workspace || workspace_bytes < nrms_news_views_fuse_workspace_size(n)) return NRMS_ERR_WORKSPACE;
  if (w->d_model % 4 != 0 || (uintptr_t)title_vec % 16 || (uintptr_t)state % 16 || (uintptr_t)out % 16 ||
      (uintptr_t)w->w_fin % 16 || (uintptr_t)workspace % 4)
    return NRMS_ERR_UNSUPPORTED;
  float* logit = static_cast<float*>(workspace);
  int32_t st = launch_gemm_additive_score(title_vec, n, w->d_model, w->w_fin, w->b_fin, w->q_fin, w->query_dim,
                                          logit, stream);
  if (st) return st;
  return launch_views_combine(title_vec, logit, n, category, subcategory, static_cast<const float*>(state),
                              w->n_cat, w->d_model, out, stream);
}

int32_t nrms_rows_add_position(const float* src, int64_t n_src_rows, const int64_t* rows, int64_t B,
                               int32_t N, int64_t stride_b, int64_t stride_n, const float* pos, int32_t D,
                               float* out, hipStream_t stream) {
  if (B < 0 || N <= 0 || D <= 0 || n_src_rows < 0 || stride_b < 0 || stride_n < 0) return NRMS_ERR_INVALID_ARG;
  if (B == 0) return NRMS_OK;
  if (!src || !pos || !out) return NRMS_ERR_INVALID_ARG;
  if ((int64_t)N * D > INT32_MAX || B > INT32_MAX / (int64_t)N) return NRMS_ERR_UNSUPPORTED;
  return launch_rows_add_position(src, n_src_rows, rows, B, N, stride_b, stride_n, pos, D, out, stream);
}

size_t nrms_recommend_topk_workspace_size(int64_t n_users, int64_t n_news, int32_t D, int32_t K,
                                          int32_t n_excl) {
  if (n_users < 0 || n_news < 0 || n_news > INT32_MAX || D != 300 || K < 1 || K > 256 || n_excl < 0 ||
      n_excl > 256)
    return 0;
  return topk_workspace_bytes(n_users, n_news, K, n_excl);
}

int32_t nrms_recommend_topk(const float* news, int64_t n_news, const float* user, int64_t n_users,
                            int32_t D, const int64_t* exclude, int32_t n_excl, int32_t K,
                            int64_t* out_idx, float* out_score, void* workspace, size_t workspace_bytes,
                            hipStream_t stream) {
  if (n_news < 0 || n_users < 0 || n_excl < 0) return NRMS_ERR_INVALID_ARG;
  if (D != 300 || K < 1 || K > 256 || n_excl > 256 || n_news > INT32_MAX) return NRMS_ERR_UNSUPPORTED;
  if (n_users == 0) return NRMS_OK;
  if (!user || !out_idx || !out_score || !workspace || (n_news > 0 && !news) || (n_excl > 0 && !exclude))
    return NRMS_ERR_INVALID_ARG;
  if (((uintptr_t)news % 16) != 0 || ((uintptr_t)user % 16) != 0 || ((uintptr_t)workspace % 8) != 0)
    return NRMS_ERR_UNSUPPORTED;
  return launch_topk(news, n_news, user, n_users, exclude, n_excl, K, out_idx, out_score, workspace,
                     workspace_bytes, stream);
}

int32_t nrms_rank_impressions(const float* news, int64_t n_news, const float* user, int64_t n_users,
                              const int64_t* news_idx, const int64_t* imp_user, const int64_t* offsets,
                              int64_t n_imp, int32_t D, int32_t tie_mode, float* out_score,
                              int32_t* out_rank, hipStream_t stream) {
  if (n_imp < 0 || n_news < 0 || n_users < 0 || D <= 0) return NRMS_ERR_INVALID_ARG;
  if (tie_mode != NRMS_RANK_ORDER && tie_mode != NRMS_RANK_SHARED) return NRMS_ERR_INVALID_ARG;
  if (n_imp > 0 && (!news || !user || !news_idx || !imp_user || !offsets || !out_score || !out_rank))
    return NRMS_ERR_INVALID_ARG;
  return launch_rank_impressions(news, n_news, user, n_users, news_idx, imp_user, offsets, n_imp, D,
                                 tie_mode, out_score, out_rank, stream);
}

int32_t nrms_impression_metrics(const float* scores, const int32_t* labels,
                                const int64_t* offsets, int64_t n_imp, double* out,
                                hipStream_t stream) {
  if (n_imp < 0) return NRMS_ERR_INVALID_ARG;
  if (n_imp > 0 && (!scores || !labels || !offsets || !out)) return NRMS_ERR_INVALID_ARG;
  return launch_impression_metrics(scores, labels, offsets, n_imp, out, stream);
}

size_t nrms_forward_workspace_size(int64_t B, int32_t C, int32_t N, int32_t L, int64_t V,
                                   int32_t D, int32_t proj_mode) {
  if (V < 0) return 0;
  const int64_t n_tok = B * (C + N) * L;
  return forward_bytes(B, C, N, L, use_folded(proj_mode, n_tok, V) ? V : n_tok, D);
}

size_t nrms_forward_state_size(int64_t V, int32_t D, int32_t with_folded_table) {
  if (V < 0 || D <= 0) return 0;
  return measure([&](Carve& cv) { state_layout(cv, V, D, with_folded_table != 0); });
}

}  // extern "C"

namespace {

// The checks nrms_forward_prepare and every forward share.
int32_t encoders_ok(int64_t V, const nrms_encoder_weights_t* news_w, const nrms_encoder_weights_t* user_w) {
  if (V <= 0) return NRMS_ERR_INVALID_ARG;
  if (int32_t st = shape_ok(news_w)) return st;
  if (int32_t st = shape_ok(user_w)) return st;
  return news_w->d_model == user_w->d_model ? NRMS_OK : NRMS_ERR_INVALID_ARG;
}
// both encoders' Q|K|V are split once into packs (proj_x6.hip) under this arithmetic
bool qkv_packs(int arith, const nrms_encoder_weights_t* news_w) {
  return arith != NRMS_GEMM_F32 && proj_x6_supported(news_w->d_model, 3 * news_w->d_model, qkv_rows(news_w));
}

// A forward call's arguments (prepared: nrms_forward_prepared[_timed], which
// read the weight-derived buffers from `state`).
struct ForwardArgs {
  const int64_t *cand_ids, *clicked_ids;
  int64_t B;
  int32_t C, N, L;
  const float* table;
  int64_t V;
  const nrms_encoder_weights_t *news_w, *user_w;
  int32_t proj_mode;
  float* logits;
  void* workspace;
  size_t workspace_bytes;
  const nrms_forward_state_t* state;
  bool prepared;
};

// Everything a forward step decides before its first launch (pipeline.py's
// ForwardPlan picks the shapes; this, the launches). What the launches
// themselves report (Launched) stays with the run.
struct StepLaunchPlan {
  bool empty;   // B == 0: nothing to launch
  int D, arith;
  int64_t n_clk, n_all;
  bool folded;
  ForwardWs ws;
  // The weight-derived buffers: the step's own workspace, which its first
  // launches fill with the step's classification folded into them
  // (fill_weights: nrms_forward); or the caller's state wherever it has them,
  // the step then starting with the classification's own two launches.
  WeightState wt;
  bool fill_weights;
  float* qkv;        // the news rows: wt.table (folded) or per-token rows
  int64_t ld, uld;   // news / user q|k|v row strides
  float* step_ws;    // the news launch's own part of ws.n.wap
  bool packed;       // both encoders' Q|K|V come from packs
  bool prepacked;    // ... and both W_add are packed before the news launch
  bool user_fused;
  // with the UserEncoder's row-list projection the clicked padding titles'
  // vectors are never read, and the scorer reads a copied candidate from the
  // rep group: no copies are written, and the news kernel lists the
  // UserEncoder's rows in its prologue
  bool user_rows_here;
  // the titles' classification without the atomics (titles.hpp): the first
  // half with the counter reset and the second (classify_tail) in the
  // vocabulary projection's tail or a launch of its own; without the second
  // half the news launch classifies the titles itself
  bool split_cls, classify_tail;
  tl::ClassifyJob cjob;
  tl::TailJobs ntail;
  // if the news launch classifies: UserEncoder token compaction
  // (user_fused.hip: a user's padding positions, one news vector, collapse into
  // one row carrying their count), and the users' longest-first dispatch order
  // in the UserEncoder projection's tail (titles.hpp)
  bool user_compact, order_tail;
  // the click scores in the fused UserEncoder launch (bitwise the score
  // kernel's; its stage is then empty)
  bool score_fold;
};

// Everything of a forward that reads weights only, enqueued on the stream into
// p.wt: prepacked: all four packings in one launch; else, packed: the two
// Q|K|V packs; folded: the vocabulary projection into wt.table. nrms_forward's
// plan folds its step's classification into these launches (split_cls: the
// counter reset and half A in the pack launch; classify_tail: half B in the
// projection's tail); nrms_forward_prepare's has none, so nothing there
// depends on an id.
Launched prepare_weights(const ForwardArgs& a, const StepLaunchPlan& p, hipStream_t stream) {
  const WeightRows nwr = qkv_rows(a.news_w), uwr = qkv_rows(a.user_w);
  const bool h3 = p.arith == NRMS_GEMM_SPLIT_F16X3;
  if (p.prepacked) {
    if (int32_t st = launch_forward_pack(nwr, p.wt.pack, uwr, p.wt.upack, a.news_w->w_add, p.wt.nwap, h3,
                                         a.user_w->w_add, p.wt.uwap, stream, p.split_cls ? &p.cjob : nullptr,
                                         reinterpret_cast<int32_t*>(p.step_ws)))
      return st;
  } else if (p.packed) {
    if (int32_t st = launch_proj_x6_pack(nwr, p.wt.pack, &uwr, p.wt.upack, h3, stream)) return st;
  }
  if (!p.folded) return NRMS_OK;
  return project_qkv({a.table, a.V, contiguous_rows(p.D), nullptr, a.V}, a.news_w, p.wt.table, p.ld, stream,
                     {.pack = p.wt.pack,
                      .packed = p.packed,
                      .arith = p.arith,
                      .tail = p.classify_tail ? &p.ntail : nullptr});
}

// Host only: no HIP call, no launch.
int32_t plan_forward_step(const ForwardArgs& a, StepLaunchPlan* plan) {
  StepLaunchPlan& p = *plan;
  const nrms_encoder_weights_t *nw = a.news_w, *uw = a.user_w;
  if (a.B < 0 || a.C < 0 || a.N <= 0 || a.L <= 0) return NRMS_ERR_INVALID_ARG;
  if (int32_t st = encoders_ok(a.V, nw, uw)) return st;
  const int D = p.D = nw->d_model;
  p.n_clk = a.B * a.N;
  p.n_all = a.B * (a.C + a.N);
  p.folded = use_folded(a.proj_mode, p.n_all * a.L, a.V);
  p.arith = gemm_arith();
  p.packed = qkv_packs(p.arith, nw);
  // what is ready before the step (NRMS_STATE_*), and where
  p.fill_weights = !a.prepared;
  WeightState sw{};
  uint32_t have = 0;
  if (a.prepared) {
    const nrms_forward_state_t* state = a.state;
    if (!state || !state->buffer || state->V != a.V || state->D != D || state->gemm_arith != p.arith)
      return NRMS_ERR_INVALID_ARG;
    have = state->flags;
    if (p.folded && !(have & NRMS_STATE_FOLDED_TABLE)) return NRMS_ERR_INVALID_ARG;
    if (state->ld_qkv != qkv_row_stride(D)) return NRMS_ERR_INVALID_ARG;
    Carve sc = Carve::over(state->buffer, state->bytes);
    sw = state_layout(sc, a.V, D, (have & NRMS_STATE_FOLDED_TABLE) != 0);
    if (!sc.ok) return NRMS_ERR_WORKSPACE;
  } else {
    // (the step's own first launches: the fused news tail takes folded + L = 20)
    have = (p.packed ? NRMS_STATE_QKV_PACKS : 0) | (p.folded ? NRMS_STATE_FOLDED_TABLE | NRMS_STATE_ADD_PACKS : 0);
  }
  p.empty = a.B == 0;
  if (p.empty) return NRMS_OK;
  // (the prepared folded table lives in the state: the workspace has no rows then)
  const bool state_table = !p.fill_weights && p.folded;
  if (!a.cand_ids || !a.clicked_ids || !a.logits || (!a.table && !state_table)) return NRMS_ERR_INVALID_ARG;
  Carve cv = Carve::over(a.workspace, a.workspace_bytes);
  p.ws = forward_layout(cv, a.B, a.C, a.N, a.L, state_table ? 0 : (p.folded ? a.V : p.n_all * a.L), D);
  if (!cv.ok) return NRMS_ERR_WORKSPACE;
  // (the state's packs were made under this arithmetic: the Q|K|V packs are
  // there exactly when this step would make them)
  if (p.packed != ((have & NRMS_STATE_QKV_PACKS) != 0)) return NRMS_ERR_INVALID_ARG;
  p.user_fused = fused_user_supported(a.N, D, uw->n_heads, uw->query_dim) && ((uintptr_t)p.ws.user % 16) == 0;
  p.user_rows_here = p.user_fused && p.arith != NRMS_GEMM_F32;
  p.prepacked = p.packed && p.user_fused && fused_news_supported(a.L, D, nw->n_heads, nw->query_dim) &&
                (have & NRMS_STATE_ADD_PACKS) != 0;
  p.wt = WeightState{nullptr, p.ws.n.pack, p.ws.u.pack, p.ws.n.wap, p.ws.u.wap};
  if (!p.fill_weights) {
    // both W_add from the state, or both packed by this step's own launches
    // into its workspace: a step writes nothing into the state
    if (p.packed) { p.wt.pack = sw.pack; p.wt.upack = sw.upack; }
    if (p.prepacked) { p.wt.nwap = sw.nwap; p.wt.uwap = sw.uwap; }
  }
  p.qkv = state_table ? sw.table : p.ws.n.qkv;
  if (p.folded) p.wt.table = p.qkv;
  p.ld = state_table ? a.state->ld_qkv : news_ld(nw, a.L);
  p.uld = user_ld(uw, a.N);
  p.step_ws = p.ws.n.wap + fused_news_packed_floats();
  p.split_cls = p.prepacked && p.folded &&
                fused_news_classify_split(p.step_ws, a.clicked_ids, p.n_clk, a.cand_ids, p.n_all, a.V, &p.cjob, &p.ntail.sc);
  p.classify_tail = p.split_cls && !g_skip_classify_tail;
  p.user_compact = p.user_fused && token_compaction() && a.N <= 64;
  p.order_tail = p.user_compact && user_lpt() && a.B * a.N <= INT32_MAX;
  p.score_fold = p.user_fused && a.C > 0 && ((uintptr_t)(p.ws.news + (size_t)p.n_clk * D) % 16) == 0;
  return NRMS_OK;
}

// The launches of a planned step. ev (optional, NRMS_FORWARD_STAGES + 1
// events): recorded on the stream before each stage and after the last.
int32_t run_forward_step(const ForwardArgs& a, const StepLaunchPlan& p, hipStream_t stream, hipEvent_t* ev) {
  const nrms_encoder_weights_t *nw = a.news_w, *uw = a.user_w;
  const ForwardWs& ws = p.ws;
  const int D = p.D;
  const int64_t n_clk = p.n_clk, n_all = p.n_all;
  auto rec = [&](int i) -> int32_t {
    if (ev && hipEventRecord(ev[i], stream) != hipSuccess) return launch_status();
    return NRMS_OK;
  };
  int32_t st;
  if ((st = rec(0))) return st;
  bool tail_done = false;
  if (p.fill_weights) {
    const Launched w = prepare_weights(a, p, stream);
    if (w.st) return w.st;
    tail_done = w.tail_done;
  } else if (p.prepacked) {
    if ((st = launch_forward_classify(p.split_cls ? &p.cjob : nullptr, reinterpret_cast<int32_t*>(p.step_ws), stream)))
      return st;
    if (p.classify_tail) {
      if ((st = launch_forward_scatter(p.ntail.sc, stream))) return st;
      tail_done = true;
    }
  }
  EncodeOpts eo{ws.n.ctx, ws.n.scores, p.wt.nwap};   // (W_add: read-only when prepacked)
  eo.news.prepacked = p.prepacked;
  eo.news.step_ws = p.step_ws;
  int64_t n_rows = a.V;
  if (p.folded) {
    if ((st = rec(1))) return st;
    eo.news.broadcast_from = p.user_rows_here ? n_all : 0;
    eo.news.user_list = p.user_rows_here ? ws.ulist : nullptr;
    eo.news.user_rows = n_clk;
    eo.news.preclassified = p.split_cls && tail_done;
  } else {
    const ProjOpts po{.pack = p.wt.pack, .packed = p.packed, .arith = p.arith};
    const ARows rows = contiguous_rows(D);
    if ((st = project_qkv({a.table, a.V, rows, a.clicked_ids, n_clk * a.L}, nw, p.qkv, p.ld, stream, po).st)) return st;
    if ((st = project_qkv({a.table, a.V, rows, a.cand_ids, a.B * a.C * a.L}, nw, p.qkv + (size_t)n_clk * a.L * p.ld,
                          p.ld, stream, po)
                  .st))
      return st;
    if ((st = rec(1))) return st;
    // (the ids only classify the tokens: the rows are per token)
    eo.news.direct_rows = true;
    n_rows = n_all * a.L;
  }
  const Launched nl =
      encode_from_qkv({p.qkv, p.ld, n_rows}, {a.clicked_ids, n_clk, a.cand_ids, n_all}, a.L, nw, ws.news, stream, eo);
  if (nl.st) return nl.st;
  if ((st = rec(2))) return st;
  // (the direct mode has no ids to deduplicate by downstream: the all-padding
  // titles' copies are written for every title, so the UserEncoder and the
  // scorer read plain rows)
  const bool deduped = p.folded && nl.deduped;
  // UserEncoder (src/model/NRMS/user_encoder.py:15-26) over the clicked news
  // vectors. After a deduplicating news launch, the clicked titles of copied
  // all-padding groups have the rep group's vectors (bitwise; not written out
  // here, see user_rows_here), so their q|k|v rows are the rep rows': only the
  // other rows are projected (row-list GEMM, listed by the news kernel's
  // prologue) and the fused tail reads copied positions from the rep rows.
  // Bitwise the same logits as projecting every row.
  const bool user_dedupe = deduped && p.user_rows_here;
  const bool user_compact = p.user_compact && nl.classified;
  const bool order_tail = p.order_tail && user_compact;
  const PaddingGroups groups = fused_news_padding_groups(p.step_ws, n_all);   // (valid where nl.classified)
  tl::TailJobs utail{};
  if (order_tail) utail.uo = tl::UserOrder{groups.pad_title, ws.uorder, a.B, a.N};
  const Launched up = project_qkv({ws.news, n_clk, contiguous_rows(D), user_dedupe ? ws.ulist : nullptr, n_clk}, uw,
                                  ws.u.qkv, p.uld, stream,
                                  {.pack = p.wt.upack,
                                   .packed = p.packed,
                                   .list_count = user_dedupe ? groups.user_count : nullptr,
                                   .arith = p.arith,
                                   .tail = order_tail ? &utail : nullptr});
  if (up.st) return up.st;
  if ((st = rec(3))) return st;
  const float* cand_news = ws.news + (size_t)n_clk * D;
  const PaddingGroups none{nullptr, nullptr, nullptr};
  const ScoreFold sfold{cand_news, a.logits, user_dedupe ? groups : none, n_clk, a.C};
  if (p.user_fused)
    st = launch_fused_user({ws.u.qkv, p.uld}, a.B, a.N, additive(uw), p.wt.uwap, ws.user, stream,
                           {.pg = (user_dedupe || user_compact) ? &groups : nullptr,
                            .prepacked = p.prepacked,
                            .copied = user_dedupe,
                            .compact = user_compact,
                            .order = ws.uorder,
                            .order_ready = up.tail_done,
                            .score = p.score_fold ? &sfold : nullptr});
  else
    st = encode_from_qkv({ws.u.qkv, p.uld, n_clk}, {nullptr, a.B, nullptr, a.B}, a.N, uw, ws.user, stream,
                         {ws.u.ctx, ws.u.scores})
             .st;
  if (st) return st;
  if ((st = rec(4))) return st;
  if (!p.score_fold) {
    st = launch_score(cand_news, a.B, a.C, (int64_t)a.C * D, D, ws.user, D, D, a.logits, stream);
    if (st) return st;
  }
  return rec(5);
}

int32_t forward_step(const ForwardArgs& a, hipStream_t stream, hipEvent_t* ev) {
  StepLaunchPlan p{};
  if (int32_t st = plan_forward_step(a, &p)) return st;
  return p.empty ? NRMS_OK : run_forward_step(a, p, stream, ev);
}

}  // namespace

extern "C" {

int32_t nrms_forward(const int64_t* cand_ids, const int64_t* clicked_ids, int64_t B, int32_t C,
                     int32_t N, int32_t L, const float* table, int64_t V,
                     const nrms_encoder_weights_t* news_w, const nrms_encoder_weights_t* user_w,
                     int32_t proj_mode, float* logits, void* workspace, size_t workspace_bytes,
                     hipStream_t stream) {
  return forward_step({cand_ids, clicked_ids, B, C, N, L, table, V, news_w, user_w, proj_mode, logits, workspace,
                       workspace_bytes, nullptr, false},
                      stream, nullptr);
}

int32_t nrms_forward_prepare(const float* table, int64_t V, const nrms_encoder_weights_t* news_w,
                             const nrms_encoder_weights_t* user_w, int32_t with_folded_table, void* state_buf,
                             size_t state_bytes, nrms_forward_state_t* state, hipStream_t stream) {
  if (!state) return NRMS_ERR_INVALID_ARG;
  *state = nrms_forward_state_t{};   // (unusable until this call succeeds)
  if (!table) return NRMS_ERR_INVALID_ARG;
  if (int32_t st = encoders_ok(V, news_w, user_w)) return st;
  // the weight phase of a step with no ids: a plan of its own
  ForwardArgs a{};
  a.table = table, a.V = V, a.news_w = news_w, a.user_w = user_w;
  StepLaunchPlan p{};
  const int D = p.D = news_w->d_model;
  p.folded = with_folded_table != 0;
  Carve cv = Carve::over(state_buf, state_bytes);
  p.wt = state_layout(cv, V, D, p.folded);
  if (!cv.ok) return NRMS_ERR_WORKSPACE;
  p.arith = gemm_arith();
  p.packed = qkv_packs(p.arith, news_w);
  // (the W_add packs are those of the fused tails: any title length / history
  // length they take has the same packs)
  p.prepacked = p.packed && fused_news_supported(tl::FL, D, news_w->n_heads, news_w->query_dim) &&
                fused_user_supported(1, D, user_w->n_heads, user_w->query_dim);
  p.ld = qkv_row_stride(D);
  if (int32_t st = prepare_weights(a, p, stream).st) return st;
  state->buffer = state_buf;
  state->bytes = state_bytes;
  state->V = V;
  state->D = D;
  state->ld_qkv = (int32_t)p.ld;
  state->gemm_arith = p.arith;
  state->flags = (p.folded ? NRMS_STATE_FOLDED_TABLE : 0) | (p.packed ? NRMS_STATE_QKV_PACKS : 0) |
                 (p.prepacked ? NRMS_STATE_ADD_PACKS : 0);
  return NRMS_OK;
}

size_t nrms_forward_prepared_workspace_size(int64_t B, int32_t C, int32_t N, int32_t L, int32_t D) {
  return forward_bytes(B, C, N, L, B * (C + N) * L, D);
}

size_t nrms_forward_prepared_folded_workspace_size(int64_t B, int32_t C, int32_t N, int32_t L, int32_t D) {
  return forward_bytes(B, C, N, L, 0, D);
}

int32_t nrms_forward_prepared(const int64_t* cand_ids, const int64_t* clicked_ids, int64_t B, int32_t C,
                              int32_t N, int32_t L, const float* table, int64_t V,
                              const nrms_encoder_weights_t* news_w, const nrms_encoder_weights_t* user_w,
                              int32_t proj_mode, float* logits, void* workspace, size_t workspace_bytes,
                              hipStream_t stream, const nrms_forward_state_t* state) {
  return forward_step({cand_ids, clicked_ids, B, C, N, L, table, V, news_w, user_w, proj_mode, logits, workspace,
                       workspace_bytes, state, true},
                      stream, nullptr);
}

int32_t nrms_forward_prepared_timed(const int64_t* cand_ids, const int64_t* clicked_ids, int64_t B, int32_t C,
                                    int32_t N, int32_t L, const float* table, int64_t V,
                                    const nrms_encoder_weights_t* news_w, const nrms_encoder_weights_t* user_w,
                                    int32_t proj_mode, float* logits, void* workspace, size_t workspace_bytes,
                                    hipStream_t stream, const nrms_forward_state_t* state,
                                    hipEvent_t* stage_events, int32_t n_events) {
  if (n_events != 0 && (n_events != NRMS_FORWARD_STAGES + 1 || !stage_events))
    return NRMS_ERR_INVALID_ARG;
  return forward_step({cand_ids, clicked_ids, B, C, N, L, table, V, news_w, user_w, proj_mode, logits, workspace,
                       workspace_bytes, state, true},
                      stream, n_events ? stage_events : nullptr);
}

int32_t nrms_forward_timed(const int64_t* cand_ids, const int64_t* clicked_ids, int64_t B, int32_t C,
                           int32_t N, int32_t L, const float* table, int64_t V,
                           const nrms_encoder_weights_t* news_w, const nrms_encoder_weights_t* user_w,
                           int32_t proj_mode, float* logits, void* workspace, size_t workspace_bytes,
                           hipStream_t stream, hipEvent_t* stage_events, int32_t n_events) {
  if (n_events != 0 && (n_events != NRMS_FORWARD_STAGES + 1 || !stage_events))
    return NRMS_ERR_INVALID_ARG;
  return forward_step({cand_ids, clicked_ids, B, C, N, L, table, V, news_w, user_w, proj_mode, logits, workspace,
                       workspace_bytes, nullptr, false},
                      stream, n_events ? stage_events : nullptr);
}

const char* nrms_forward_stage_name(int32_t i) {
  static const char* names[NRMS_FORWARD_STAGES] = {"qkv_news", "news_fused", "qkv_user", "user_fused",
                                                   "score"};
  return (i >= 0 && i < NRMS_FORWARD_STAGES) ? names[i] : nullptr;
}


// ---------------------------------------------------------------------------
// Training kernels (train-mode forward pieces, backward, optimizer step).

int32_t nrms_dropout(const float* x, float* y, int64_t n, float p, uint64_t seed,
                     hipStream_t stream) {
  if (n < 0 || !(p >= 0.f && p < 1.f)) return NRMS_ERR_INVALID_ARG;
  if (n > 0 && (!x || !y)) return NRMS_ERR_INVALID_ARG;
  return launch_dropout(x, y, n, p, seed, stream);
}

int32_t nrms_additive_forward_train(const float* x, int64_t n_seq, int32_t L,
                                    const nrms_encoder_weights_t* w, float* y_tanh, float* scores,
                                    float* out, hipStream_t stream) {
  if (n_seq < 0 || L <= 0) return NRMS_ERR_INVALID_ARG;
  if (!weights_ok(w)) return NRMS_ERR_INVALID_ARG;
  if (n_seq == 0) return NRMS_OK;
  if (!x || !y_tanh || !scores || !out) return NRMS_ERR_INVALID_ARG;
  int32_t st = launch_gemm_additive_score_y(x, n_seq * L, w->d_model, w->w_add, w->b_add, w->q_add,
                                            w->query_dim, scores, y_tanh, stream);
  if (st) return st;
  return launch_additive_pool(x, scores, n_seq, L, w->d_model, out, stream);
}

size_t nrms_additive_backward_workspace_size(int64_t n_seq, int32_t L, int32_t D, int32_t Q) {
  if (n_seq < 0 || L <= 0 || D <= 0 || Q <= 0) return 0;
  return measure([&](Carve& cv) { additive_backward_layout(cv, n_seq, L, D, Q); });
}

int32_t nrms_additive_backward(const float* x, int64_t n_seq, int32_t L,
                               const nrms_encoder_weights_t* w, const float* y_tanh,
                               const float* scores, const float* dout, float* dx, float* d_w_add,
                               float* d_b_add, float* d_q_add, void* workspace,
                               size_t workspace_bytes, hipStream_t stream) {
  if (n_seq < 0 || L <= 0) return NRMS_ERR_INVALID_ARG;
  if (!weights_ok(w)) return NRMS_ERR_INVALID_ARG;
  if (n_seq == 0) return NRMS_OK;
  if (!x || !y_tanh || !scores || !dout || !dx || !d_w_add || !d_b_add || !d_q_add)
    return NRMS_ERR_INVALID_ARG;
  const int D = w->d_model, Q = w->query_dim;
  if (D % 4 != 0 || Q % 4 != 0) return NRMS_ERR_UNSUPPORTED;
  Carve cv = Carve::over(workspace, workspace_bytes);
  const AdditiveBackwardWs z = additive_backward_layout(cv, n_seq, L, D, Q);
  if (!cv.ok) return NRMS_ERR_WORKSPACE;
  float *dz = z.dz, *waT = z.waT;
  int32_t st = launch_additive_backward_rows(x, y_tanh, scores, w->q_add, dout, n_seq, L, D, Q, dx,
                                             dz, d_q_add, d_b_add, z.part_rows, stream);
  if (st) return st;
  const float* wa[1] = {w->w_add};
  st = launch_transpose(wa, 1, Q, D, waT, stream);   // [Q, D] -> [D, Q]
  if (st) return st;
  st = launch_gemm_store_f32(dz, n_seq * L, Q, one_segment(waT, D, 1), D, dx, D, stream);   // dx += dz W_add
  if (st) return st;
  return launch_gemm_tn(dz, n_seq * L, Q, x, D, d_w_add, nullptr, z.part_tn, stream);   // dW += dz^T x
}

int32_t nrms_self_attention_backward(const float* qkv, const float* dctx, int64_t n_seq,
                                     int32_t L, const nrms_encoder_weights_t* w, float* dqkv,
                                     hipStream_t stream) {
  if (n_seq < 0 || L <= 0) return NRMS_ERR_INVALID_ARG;
  if (int32_t st = shape_ok(w)) return st;
  if (n_seq == 0) return NRMS_OK;
  if (!qkv || !dctx || !dqkv) return NRMS_ERR_INVALID_ARG;
  return launch_mhsa_backward(qkv, dctx, n_seq, L, w->d_model, w->n_heads, dqkv, stream);
}

size_t nrms_qkv_project_backward_workspace_size(int32_t D) {
  if (D <= 0) return 0;
  return measure([&](Carve& cv) { project_backward_layout(cv, D); });
}

int32_t nrms_qkv_project_backward(const float* x, int64_t rows, const nrms_encoder_weights_t* w,
                                  const float* dqkv, float* dx, float* d_w_qkv, float* d_b_qkv,
                                  void* workspace, size_t workspace_bytes, hipStream_t stream) {
  if (rows < 0) return NRMS_ERR_INVALID_ARG;
  if (!weights_ok(w)) return NRMS_ERR_INVALID_ARG;
  if (rows == 0) return NRMS_OK;
  if (!x || !dqkv || !d_w_qkv || !d_b_qkv) return NRMS_ERR_INVALID_ARG;
  const int D = w->d_model;
  int32_t st;
  Carve cv = Carve::over(workspace, workspace_bytes);
  const ProjectBackwardWs z = project_backward_layout(cv, D);
  if (!cv.ok) return NRMS_ERR_WORKSPACE;
  if (dx) {
    const float* ws3[3] = {w->w_q, w->w_k, w->w_v};
    st = launch_transpose(ws3, 3, D, D, z.wT, stream);   // [3D, D] -> [D, 3D]
    if (st) return st;
    st = launch_gemm_store_f32(dqkv, rows, 3 * D, one_segment(z.wT, D, 0), D, dx, D, stream);   // dx = dqkv [Wq; Wk; Wv]
    if (st) return st;
  }
  return launch_gemm_tn(dqkv, rows, 3 * D, x, D, d_w_qkv, d_b_qkv, z.part_tn, stream);
}

int32_t nrms_score_backward(const float* news, int64_t B, int32_t C, int64_t stride_b,
                            int64_t stride_c, const float* user, int64_t stride_u, int32_t D,
                            const float* dlogits, float* dnews, float* duser, hipStream_t stream) {
  if (B < 0 || C < 0 || D <= 0) return NRMS_ERR_INVALID_ARG;
  if (B * C > 0 && (!news || !user || !dlogits || !dnews || !duser)) return NRMS_ERR_INVALID_ARG;
  return launch_score_backward(news, B, C, stride_b, stride_c, user, stride_u, D, dlogits, dnews,
                               duser, stream);
}

int32_t nrms_train_batch_gather(const int64_t* titles, int64_t n_title_rows, int32_t L,
                                const int32_t* sample_rows, int64_t n_samples, int32_t C, int32_t N,
                                const int64_t* sample_idx, int64_t B, int64_t* cand_ids,
                                int64_t* clicked_ids, hipStream_t stream) {
  if (n_title_rows < 0 || n_samples < 0 || B < 0 || L <= 0 || C < 0 || N < 0) return NRMS_ERR_INVALID_ARG;
  if (B == 0 || C + N == 0) return NRMS_OK;
  if (!sample_idx || (C > 0 && !cand_ids) || (N > 0 && !clicked_ids)) return NRMS_ERR_INVALID_ARG;
  if ((n_samples > 0 && !sample_rows) || (n_title_rows > 0 && !titles)) return NRMS_ERR_INVALID_ARG;
  return launch_train_batch_gather(titles, n_title_rows, L, sample_rows, n_samples, C, N, sample_idx, B,
                                   cand_ids, clicked_ids, stream);
}

int32_t nrms_train_batch_sample_gather(const int64_t* titles, int64_t n_title_rows, int32_t L,
                                       const int32_t* pos_row, const int32_t* pos_imp, int64_t n_samples,
                                       const int64_t* neg_off, int64_t n_imps, const int32_t* neg_rows,
                                       int64_t n_neg, const int32_t* imp_hist, const int32_t* hist_rows,
                                       int64_t n_hists, int32_t K, int32_t N, const int64_t* sample_idx, int64_t B,
                                       uint64_t seed, int64_t epoch, int64_t* cand_ids, int64_t* clicked_ids,
                                       hipStream_t stream) {
  if (n_title_rows < 0 || n_samples < 0 || n_imps < 0 || n_neg < 0 || n_hists < 0 || B < 0 || L <= 0 || N < 0)
    return NRMS_ERR_INVALID_ARG;
  if (K < 0 || K > 15) return NRMS_ERR_UNSUPPORTED;
  if (B == 0) return NRMS_OK;
  if (!sample_idx || !cand_ids || (N > 0 && !clicked_ids)) return NRMS_ERR_INVALID_ARG;
  if ((n_samples > 0 && (!pos_row || !pos_imp)) || (n_title_rows > 0 && !titles)) return NRMS_ERR_INVALID_ARG;
  if (n_imps > 0 && (!neg_off || !imp_hist)) return NRMS_ERR_INVALID_ARG;
  if ((n_neg > 0 && !neg_rows) || (n_hists > 0 && N > 0 && !hist_rows)) return NRMS_ERR_INVALID_ARG;
  return launch_train_batch_sample_gather(titles, n_title_rows, L, pos_row, pos_imp, n_samples, neg_off, n_imps,
                                          neg_rows, n_neg, imp_hist, hist_rows, n_hists, K, N, sample_idx, B, seed,
                                          epoch, cand_ids, clicked_ids, stream);
}

int32_t nrms_xent_class0(const float* logits, int64_t B, int32_t C, float* dlogits, float* loss_out,
                         hipStream_t stream) {
  if (B <= 0 || C <= 0) return NRMS_ERR_INVALID_ARG;
  if (!logits || !dlogits || !loss_out) return NRMS_ERR_INVALID_ARG;
  return launch_xent_class0(logits, B, C, dlogits, loss_out, stream);
}

int32_t nrms_embedding_backward(const int64_t* ids, int64_t n_tok, const float* dx, int64_t V,
                                int32_t D, int64_t padding_idx, float* dtable,
                                hipStream_t stream) {
  if (n_tok < 0 || V <= 0 || D <= 0) return NRMS_ERR_INVALID_ARG;
  if (n_tok > 0 && (!ids || !dx || !dtable)) return NRMS_ERR_INVALID_ARG;
  return launch_embedding_backward(ids, n_tok, dx, V, D, padding_idx, dtable, stream);
}

size_t nrms_embedding_backward_workspace_size(int64_t n_tok, int64_t V) {
  if (n_tok < 0 || V <= 0) return 0;
  return embedding_backward_sorted_bytes(n_tok, V);
}

int32_t nrms_embedding_backward_ws(const int64_t* ids, int64_t n_tok, const float* dx, int64_t V, int32_t D,
                                   int64_t padding_idx, float* dtable, void* workspace, size_t workspace_bytes,
                                   hipStream_t stream) {
  if (n_tok < 0 || V <= 0 || D <= 0) return NRMS_ERR_INVALID_ARG;
  if (n_tok > 0 && (!ids || !dx || !dtable)) return NRMS_ERR_INVALID_ARG;
  return launch_embedding_backward_sorted(ids, n_tok, dx, V, D, padding_idx, dtable, workspace, workspace_bytes,
                                          stream);
}

int32_t nrms_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq,
                       int64_t n, float lr, float beta1, float beta2, float eps, int64_t step,
                       hipStream_t stream) {
  if (n < 0 || step < 1) return NRMS_ERR_INVALID_ARG;
  if (n > 0 && (!param || !grad || !exp_avg || !exp_avg_sq)) return NRMS_ERR_INVALID_ARG;
  return launch_adam(param, grad, exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps, step, stream);
}

int32_t nrms_adam_step_multi(const nrms_adam_tensor_t* tensors, int32_t n, float lr, float beta1,
                             float beta2, float eps, int64_t step, hipStream_t stream) {
  if (n < 0 || step < 1) return NRMS_ERR_INVALID_ARG;
  if (n > 0 && !tensors) return NRMS_ERR_INVALID_ARG;
  for (int32_t i = 0; i < n; ++i) {
    const nrms_adam_tensor_t& t = tensors[i];
    if (t.numel < 0) return NRMS_ERR_INVALID_ARG;
    if (t.numel > 0 && (!t.param || !t.grad || !t.exp_avg || !t.exp_avg_sq))
      return NRMS_ERR_INVALID_ARG;
  }
  return launch_adam_multi(tensors, n, lr, beta1, beta2, eps, step, stream);
}

static int32_t check_flat_tensors(const nrms_flat_tensor_t* tensors, int32_t n, const float* flat) {
  if (n < 0 || (n > 0 && !tensors)) return NRMS_ERR_INVALID_ARG;
  for (int32_t i = 0; i < n; ++i) {
    const nrms_flat_tensor_t& t = tensors[i];
    if (t.numel < 0 || t.offset < 0) return NRMS_ERR_INVALID_ARG;
    if (t.numel > 0 && (!t.data || !flat)) return NRMS_ERR_INVALID_ARG;
  }
  return NRMS_OK;
}

int32_t nrms_params_pack(const nrms_flat_tensor_t* tensors, int32_t n, float* flat, hipStream_t stream) {
  if (int32_t st = check_flat_tensors(tensors, n, flat)) return st;
  return launch_params_pack(tensors, n, flat, stream);
}

int32_t nrms_params_unpack_div(const nrms_flat_tensor_t* tensors, int32_t n, const float* flat,
                               float divisor, hipStream_t stream) {
  if (divisor == 0.0f || divisor != divisor) return NRMS_ERR_INVALID_ARG;     // 0 and NaN
  if (int32_t st = check_flat_tensors(tensors, n, flat)) return st;
  return launch_params_unpack_div(tensors, n, flat, divisor, stream);
}

}  // extern "C"
