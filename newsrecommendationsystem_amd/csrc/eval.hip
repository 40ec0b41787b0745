// Eval-semantics scoring (src/evaluate.py:171-272) on the GPU:
//  * pair scorer: logits of ragged impressions from cached news / user
//    vectors (evaluate.py:251-260: get_prediction per impression), one wave
//    per (candidate, user) pair — every impression of a split in one launch
//    instead of a Python loop with a device->host sync per impression;
//  * the same scores with every candidate's rank inside its impression, one
//    workgroup per impression (nrms_rank_impressions: the reference's unused
//    value2rank, evaluate.py:45-48, for MIND prediction files);
//  * per-impression ranking metrics (evaluate.py:24-42,160-168): AUC (the
//    Mann-Whitney statistic with ties counted 1/2, which is what
//    sklearn.metrics.roc_auc_score computes for binary labels), MRR, nDCG@5,
//    nDCG@10, one wave per impression, fp64 accumulation. Edge cases follow
//    the reference as it runs against scikit-learn 1.7 (pinned by
//    tests/golden/nrms_flow_golden.npz): a non-finite score makes
//    roc_auc_score raise, so all four are NaN (the ValueError branch,
//    evaluate.py:167-168); a single-class impression gets AUC = NaN (sklearn
//    warns instead of raising) while MRR / nDCG keep numpy's arithmetic:
//    all-negative -> 0/0 = NaN, all-positive -> MRR = mean(1/rank), nDCG = 1.
#include "nrms_common.hpp"

namespace nrms {
namespace {

constexpr int kThreads = 256;

__global__ __launch_bounds__(kThreads) void score_pairs_kernel(
    const float* __restrict__ news, int64_t n_news, const float* __restrict__ user,
    int64_t n_users, const int64_t* __restrict__ news_idx, const int64_t* __restrict__ user_idx,
    int64_t n_pairs, int D, float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t k = (int64_t)blockIdx.x * (kThreads / kWave) + (threadIdx.x >> 6);
  if (k >= n_pairs) return;
  const int64_t a = news_idx[k], b = user_idx[k];
  if ((uint64_t)a >= (uint64_t)n_news || (uint64_t)b >= (uint64_t)n_users) {
    if (lane == 0) out[k] = qnan();
    return;
  }
  const float* nv = news + a * D;
  const float* uv = user + b * D;
  const UserRegs none{};
  const float acc = (D & 3) == 0 ? wave_dot<true, false>(nv, uv, D, lane, none)
                                 : wave_dot<false, false>(nv, uv, D, lane, none);
  if (lane == 0) out[k] = acc;
}

// ---------------------------------------------------------------------------
// Fused per-impression score + rank (nrms_rank_impressions): one workgroup per
// impression. Its waves (four; NRMS_RANK_WAVES for measurements, see
// profiles/predict_bench.txt) stride over the candidates, each candidate one
// wave_dot against the impression's user vector (held in registers: the
// lane's float4s are loaded once), and lane 0 writes the score and, while the
// impression fits kRankLds, its order key into LDS. After one barrier thread t
// ranks candidates t, t + 256, ... by counting over the keys: a uniform loop of
// broadcast 16-byte LDS reads, four VALU per key.
//
// An impression of more than kRankLds candidates takes the chunked path:
// the keys are rebuilt from the out_score values this workgroup wrote
// (workgroup barrier in between), kRankLds at a time through the same LDS
// array, and every thread adds each chunk's count to its candidates'
// out_rank, which it alone reads and writes. n^2 / 256 compares per thread as
// on the fast path, plus n / kRankLds re-reads of out_score and out_rank.
//
// Order key: the order-preserving bit flip of the fp32 score with -0 folded
// into +0 and every NaN mapped to the top, 0xffffffff, above +inf. No key is 0
// (-inf gives 0x007fffff), so key_j >= key_c is key_j > key_c - 1.
constexpr int kRankLds = NRMS_RANK_LDS_CANDIDATES;

__device__ __forceinline__ uint32_t rank_key(float s) {
  uint32_t b = __float_as_uint(s);
  if (s != s) return 0xffffffffu;
  if (b == 0x80000000u) b = 0u;
  return b ^ ((uint32_t)((int32_t)b >> 31) | 0x80000000u);
}

// #{j < m : key[j] > kc, or key[j] == kc and j > cr and ties by order}; key is
// 16-B aligned, cr (the candidate's own position relative to key[0]) may lie
// outside [0, m).
__device__ __forceinline__ int count_above(const uint32_t* __restrict__ key, int m, int64_t cr, uint32_t kc,
                                           bool order) {
  const uint32_t kge = kc - (order ? 1u : 0u);
  int cnt = 0, j = 0;
  for (; j + 4 <= m; j += 4) {
    const uint4 k4 = *reinterpret_cast<const uint4*>(key + j);
    cnt += k4.x > (j > cr ? kge : kc);
    cnt += k4.y > (j + 1 > cr ? kge : kc);
    cnt += k4.z > (j + 2 > cr ? kge : kc);
    cnt += k4.w > (j + 3 > cr ? kge : kc);
  }
  for (; j < m; ++j) cnt += key[j] > (j > cr ? kge : kc);
  return cnt;
}

template <bool VEC, int THREADS>
__global__ __launch_bounds__(THREADS) void rank_impressions_kernel(
    const float* __restrict__ news, int64_t n_news, const float* __restrict__ user, int64_t n_users,
    const int64_t* __restrict__ news_idx, const int64_t* __restrict__ imp_user,
    const int64_t* __restrict__ offsets, int D, int tie_mode, float* out_score, int32_t* out_rank) {
  __shared__ __attribute__((aligned(16))) uint32_t s_key[kRankLds];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t imp = blockIdx.x;
  const int64_t b = offsets[imp];
  const int64_t n = offsets[imp + 1] - b;
  if (n <= 0) return;
  const int64_t u = imp_user[imp];
  const bool u_ok = (uint64_t)u < (uint64_t)n_users;
  const float* uv = user + (u_ok ? u : 0) * D;
  UserRegs ur{};
  if (VEC && u_ok) ur = load_user_regs(uv, D, lane);
  const bool in_lds = n <= kRankLds;
  float* sc = out_score + b;
  int32_t* rk = out_rank + b;

  int64_t a = news_idx[b + (wave < n ? wave : 0)];
  for (int64_t c = wave; c < n; c += THREADS / kWave) {
    const int64_t cn = c + THREADS / kWave;
    const int64_t a_next = news_idx[b + (cn < n ? cn : c)];   // the next row's index, ahead of this dot
    float s = qnan();
    if (u_ok && (uint64_t)a < (uint64_t)n_news) s = wave_dot<VEC, true>(news + a * D, uv, D, lane, ur);
    if (lane == 0) {
      sc[c] = s;
      if (in_lds) s_key[c] = rank_key(s);
    }
    a = a_next;
  }
  __syncthreads();   // (workgroup scope: the scores written above are visible to every wave below)

  const bool order = tie_mode == NRMS_RANK_ORDER;
  if (in_lds) {
    const int m = (int)n;
    for (int c = tid; c < m; c += THREADS) rk[c] = 1 + count_above(s_key, m, c, s_key[c], order);
    return;
  }
  for (int64_t j0 = 0; j0 < n; j0 += kRankLds) {
    const int m = n - j0 < kRankLds ? (int)(n - j0) : kRankLds;
    if (j0) __syncthreads();   // the previous chunk's readers are done
    for (int j = tid; j < m; j += THREADS) s_key[j] = rank_key(sc[j0 + j]);
    __syncthreads();
    for (int64_t c = tid; c < n; c += THREADS) {
      const int cnt = count_above(s_key, m, c - j0, rank_key(sc[c]), order);
      rk[c] = (j0 ? rk[c] : 1) + cnt;
    }
  }
}

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// Rank of candidate c under the reference's order: np.argsort(y_score)[::-1]
// (descending score; among equal scores the larger index comes first, i.e. a
// stable ascending sort reversed). rank = 1 + #{j : s_j > s_c or (s_j == s_c and j > c)}.
__global__ __launch_bounds__(kThreads) void impression_metrics_kernel(
    const float* __restrict__ scores, const int32_t* __restrict__ labels,
    const int64_t* __restrict__ offsets, int64_t n_imp, double* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t imp = (int64_t)blockIdx.x * (kThreads / kWave) + (threadIdx.x >> 6);
  if (imp >= n_imp) return;
  const int64_t b = offsets[imp], e = offsets[imp + 1];
  const int n = (int)(e - b);
  const float* s = scores + b;
  const int32_t* y = labels + b;

  // class counts and non-finite check (sklearn's check_array rejects NaN / inf)
  double npos = 0.0, nbad = 0.0;
  for (int c = lane; c < n; c += kWave) {
    npos += (y[c] == 1) ? 1.0 : 0.0;
    nbad += __builtin_isfinite(s[c]) ? 0.0 : 1.0;
  }
  npos = wave_sum_d(npos);
  nbad = wave_sum_d(nbad);
  const double nneg = (double)n - npos;
  double* o = out + imp * 4;
  if (n == 0 || npos == 0.0 || nbad > 0.0) {   // all-negative: every metric is 0/0
    if (lane < 4) o[lane] = __builtin_nan("");
    return;
  }
  double auc_num = 0.0, rr = 0.0, dcg5 = 0.0, dcg10 = 0.0;
  for (int c = lane; c < n; c += kWave) {
    if (y[c] != 1) continue;
    const float sc = s[c];
    int higher = 0;
    double wins = 0.0;
    for (int j = 0; j < n; ++j) {
      const float sj = s[j];
      higher += (sj > sc || (sj == sc && j > c)) ? 1 : 0;
      if (y[j] != 1) wins += (sc > sj) ? 1.0 : (sc == sj ? 0.5 : 0.0);
    }
    const int rank = higher + 1;
    auc_num += wins;
    rr += 1.0 / rank;
    const double disc = 1.0 / log2((double)rank + 1.0);
    if (rank <= 5) dcg5 += disc;
    if (rank <= 10) dcg10 += disc;
  }
  auc_num = wave_sum_d(auc_num);
  rr = wave_sum_d(rr);
  dcg5 = wave_sum_d(dcg5);
  dcg10 = wave_sum_d(dcg10);
  // ideal DCG: the positives occupy ranks 1..npos (evaluate.py:32-35)
  double idcg5 = 0.0, idcg10 = 0.0;
  const int np_i = (int)npos;
  for (int r = 1; r <= np_i && r <= 10; ++r) {
    const double d = 1.0 / log2((double)r + 1.0);
    if (r <= 5) idcg5 += d;
    idcg10 += d;
  }
  if (lane == 0) {
    const bool one_class = nneg == 0.0;   // all positive: identical DCG arrays, ratio 1
    o[0] = one_class ? __builtin_nan("") : auc_num / (npos * nneg);
    o[1] = rr / npos;
    o[2] = one_class ? 1.0 : dcg5 / idcg5;
    o[3] = one_class ? 1.0 : dcg10 / idcg10;
  }
}

}  // namespace

int32_t launch_score_pairs(const float* news, int64_t n_news, const float* user, int64_t n_users,
                           const int64_t* news_idx, const int64_t* user_idx, int64_t n_pairs,
                           int D, float* out, hipStream_t s) {
  if (n_pairs == 0) return NRMS_OK;
  const int per = kThreads / kWave;
  const int64_t blocks = (n_pairs + per - 1) / per;
  if (blocks > INT32_MAX) return NRMS_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(score_pairs_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, s, news,
                     n_news, user, n_users, news_idx, user_idx, n_pairs, D, out);
  return launch_status();
}

// NRMS_RANK_WAVES in the environment (measurement only, read once): waves per
// impression's workgroup, 1, 2 or 4 (default). The outputs do not depend on it.
int rank_waves_knob() {
  static const int knob = [] {
    const char* e = env_knob("NRMS_RANK_WAVES");
    return e ? atoi(e) : 4;
  }();
  return knob;
}

int32_t launch_rank_impressions(const float* news, int64_t n_news, const float* user, int64_t n_users,
                                const int64_t* news_idx, const int64_t* imp_user, const int64_t* offsets,
                                int64_t n_imp, int D, int tie_mode, float* out_score, int32_t* out_rank,
                                hipStream_t s) {
  if (n_imp == 0) return NRMS_OK;
  if (n_imp > INT32_MAX) return NRMS_ERR_UNSUPPORTED;
  const dim3 grid((unsigned)n_imp);
  const bool vec = (D & 3) == 0;
#define NRMS_RANK_LAUNCH(V, T)                                                                          \
  hipLaunchKernelGGL((rank_impressions_kernel<V, T>), grid, dim3(T), 0, s, news, n_news, user, n_users, \
                     news_idx, imp_user, offsets, D, tie_mode, out_score, out_rank)
  switch (rank_waves_knob()) {
    case 1: if (vec) NRMS_RANK_LAUNCH(true, 64); else NRMS_RANK_LAUNCH(false, 64); break;
    case 2: if (vec) NRMS_RANK_LAUNCH(true, 128); else NRMS_RANK_LAUNCH(false, 128); break;
    default: if (vec) NRMS_RANK_LAUNCH(true, 256); else NRMS_RANK_LAUNCH(false, 256); break;
  }
#undef NRMS_RANK_LAUNCH
  return launch_status();
}

int32_t launch_impression_metrics(const float* scores, const int32_t* labels,
                                  const int64_t* offsets, int64_t n_imp, double* out,
                                  hipStream_t s) {
  if (n_imp == 0) return NRMS_OK;
  const int per = kThreads / kWave;
  const int64_t blocks = (n_imp + per - 1) / per;
  if (blocks > INT32_MAX) return NRMS_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(impression_metrics_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, s,
                     scores, labels, offsets, n_imp, out);
  return launch_status();
}

}  // namespace nrms
