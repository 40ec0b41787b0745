// The Exp1 model's additions to the NRMS path (src/model/Exp1/news_encoder.py:
// 36-43,95-111, src/model/Exp1/user_encoder.py:27-28): the category /
// subcategory element encoders folded into a per-id table, the final additive
// attention over the three views of an article, and the position embedding of
// the user history. All three are small or HBM-bound: 16-B lanes, each row read
// by consecutive lanes, output written fully contiguous (as gather.hip).
#include "nrms_common.hpp"

namespace nrms {
namespace {

constexpr int kViewThreads = 256;
constexpr int kViewWaves = kViewThreads / kWave;
constexpr int kRowsPerBlock = 64;
constexpr int kUnroll = 4;

// relu as torch computes it: NaN stays NaN, everything else below or at zero is +0
__device__ __forceinline__ float relu_f(float v) { return (v > 0.f || v != v) ? v : 0.f; }

// dot of two [n] rows by one wave: lane-strided FMA chain, then the xor tree
__device__ __forceinline__ float wave_row_dot(const float* __restrict__ a, const float* __restrict__ b, int n,
                                              int lane) {
  float acc = 0.f;
  for (int i = lane; i < n; i += kWave) acc = fmaf(a[i], b[i], acc);
  return wave_sum(acc);
}

// One workgroup per (category id, element encoder): blockIdx.x = 2 c + which.
//   vec[c]   = relu(emb[c] W^T + b)                     [D]
//   logit[c] = q_fin . tanh(W_fin vec[c] + b_fin)       (additive.py:35-38)
// LDS: the embedding row [E], the view vector [D], one partial per wave.
__global__ __launch_bounds__(kViewThreads) void views_prepare_kernel(nrms_views_weights_t w, float* __restrict__ state) {
  extern __shared__ float lds[];
  const int E = w.emb_dim, D = w.d_model, Q = w.query_dim;
  const int64_t C = w.n_cat;
  float* e_row = lds;
  float* v_row = lds + E;
  float* part = v_row + D;
  const int64_t c = blockIdx.x >> 1;
  const int which = blockIdx.x & 1;
  const float* emb = (which ? w.emb_sub : w.emb_cat) + c * E;
  const float* W = which ? w.w_sub : w.w_cat;
  const float* b = which ? w.b_sub : w.b_cat;
  float* vec = state + ((int64_t)which * C + c) * D;
  float* logit = state + 2 * C * D + (int64_t)which * C + c;
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;

  for (int i = threadIdx.x; i < E; i += kViewThreads) e_row[i] = emb[i];
  __syncthreads();
  for (int d = wave; d < D; d += kViewWaves) {
    const float v = relu_f(wave_row_dot(W + (int64_t)d * E, e_row, E, lane) + b[d]);
    if (lane == 0) {
      v_row[d] = v;
      vec[d] = v;
    }
  }
  __syncthreads();
  float acc = 0.f;   // every lane of a wave carries the wave's partial
  for (int q = wave; q < Q; q += kViewWaves)
    acc = fmaf(w.q_fin[q], tanhf(wave_row_dot(w.w_fin + (int64_t)q * D, v_row, D, lane) + w.b_fin[q]), acc);
  if (lane == 0) part[wave] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    float s = 0.f;
    for (int i = 0; i < kViewWaves; ++i) s += part[i];
    *logit = s;
  }
}

// Final attention over (title, category, subcategory) and the weighted sum,
// 64 rows per workgroup. The first 64 threads turn their row's three logits
// into softmax weights (maximum subtracted); all threads then stream the rows.
// title and out may be the same buffer: every element is read and written by
// one thread, the read first.
__global__ __launch_bounds__(kViewThreads) void views_combine_kernel(
    const float4* title, const float* __restrict__ title_logit, int64_t n, const int64_t* __restrict__ category,
    const int64_t* __restrict__ subcategory, const float4* __restrict__ cat_vec, const float4* __restrict__ sub_vec,
    const float* __restrict__ cat_logit, const float* __restrict__ sub_logit, int64_t C, int D4, float4* out) {
  __shared__ float w_t[kRowsPerBlock], w_c[kRowsPerBlock], w_s[kRowsPerBlock];
  __shared__ int64_t off_c[kRowsPerBlock], off_s[kRowsPerBlock];   // first float4 of the view's row; -1: id out of range
  const int64_t r0 = (int64_t)blockIdx.x * kRowsPerBlock;
  const int rows = (int)min<int64_t>(kRowsPerBlock, n - r0);
  if ((int)threadIdx.x < rows) {
    const int r = threadIdx.x;
    const int64_t ic = category[r0 + r], is = subcategory[r0 + r];
    const bool ok = (uint64_t)ic < (uint64_t)C && (uint64_t)is < (uint64_t)C;
    float wt = qnan(), wc = qnan(), ws = qnan();
    if (ok) {
      const float lt = title_logit[r0 + r], lc = cat_logit[ic], ls = sub_logit[is];
      const float m = fmaxf(lt, fmaxf(lc, ls));
      const float et = expf(lt - m), ec = expf(lc - m), es = expf(ls - m);
      const float sum = et + ec + es;
      wt = et / sum;
      wc = ec / sum;
      ws = es / sum;
    }
    w_t[r] = wt;
    w_c[r] = wc;
    w_s[r] = ws;
    off_c[r] = ok ? ic * D4 : -1;
    off_s[r] = ok ? is * D4 : -1;
  }
  __syncthreads();
  const int total = rows * D4;
  const float4* t_blk = title + r0 * D4;
  float4* out_blk = out + r0 * D4;
  for (int base = threadIdx.x; base < total; base += kViewThreads * kUnroll) {
    float4 v[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const int i = base + u * kViewThreads;
      if (i < total) {
        const int r = i / D4;
        const int c = i - r * D4;
        const int64_t oc = off_c[r];
        if (oc < 0) {
          v[u] = nan4();
        } else {
          const float4 t = t_blk[i], a = cat_vec[oc + c], b = sub_vec[off_s[r] + c];
          const float wt = w_t[r], wc = w_c[r], ws = w_s[r];
          // (w_t t + w_c cat) + w_s sub, one rounding per step
          v[u] = make_float4(fmaf(ws, b.x, fmaf(wc, a.x, wt * t.x)), fmaf(ws, b.y, fmaf(wc, a.y, wt * t.y)),
                             fmaf(ws, b.z, fmaf(wc, a.z, wt * t.z)), fmaf(ws, b.w, fmaf(wc, a.w, wt * t.w)));
        }
      }
    }
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const int i = base + u * kViewThreads;
      if (i < total) out_blk[i] = v[u];
    }
  }
}

// Where row R = b N + i of the [B, N, D] input lives: rows != null: row rows[R]
// of the [n_src_rows, D] table; else the view's (b, i) at b stride_b + i
// stride_n floats. -1: out of range (a NaN row).
__device__ __forceinline__ int64_t position_src_offset(const int64_t* __restrict__ rows, int64_t n_src_rows, int64_t R,
                                                       int N, int64_t stride_b, int64_t stride_n, int D) {
  if (rows) {
    const int64_t id = rows[R];
    return (uint64_t)id < (uint64_t)n_src_rows ? id * D : -1;
  }
  return (R / N) * stride_b + (R % N) * stride_n;
}

// out[R, :] = x[R, :] + pos[R % N, :], 64 rows per workgroup, float4 lanes
// (D = 4 D4, src / pos / out 16-B aligned, strides multiples of 4).
__global__ __launch_bounds__(kViewThreads) void rows_add_position_kernel(
    const float* __restrict__ src, int64_t n_src_rows, const int64_t* __restrict__ rows, int64_t n_rows, int N,
    int64_t stride_b, int64_t stride_n, const float4* __restrict__ pos, int D4, float4* __restrict__ out) {
  __shared__ int64_t off_x[kRowsPerBlock];   // in float4 units; -1: a NaN row
  __shared__ int off_p[kRowsPerBlock];
  const int64_t r0 = (int64_t)blockIdx.x * kRowsPerBlock;
  const int cnt = (int)min<int64_t>(kRowsPerBlock, n_rows - r0);
  if ((int)threadIdx.x < cnt) {
    const int64_t R = r0 + threadIdx.x;
    const int64_t o = position_src_offset(rows, n_src_rows, R, N, stride_b, stride_n, 4 * D4);
    off_x[threadIdx.x] = o < 0 ? -1 : o / 4;
    off_p[threadIdx.x] = (int)(R % N) * D4;
  }
  __syncthreads();
  const float4* src4 = reinterpret_cast<const float4*>(src);
  const int total = cnt * D4;
  float4* out_blk = out + r0 * D4;
  for (int base = threadIdx.x; base < total; base += kViewThreads * kUnroll) {
    float4 v[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const int i = base + u * kViewThreads;
      if (i < total) {
        const int r = i / D4;
        const int c = i - r * D4;
        const int64_t o = off_x[r];
        if (o < 0) {
          v[u] = nan4();
        } else {
          const float4 x = src4[o + c], p = pos[off_p[r] + c];
          v[u] = make_float4(x.x + p.x, x.y + p.y, x.z + p.z, x.w + p.w);
        }
      }
    }
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const int i = base + u * kViewThreads;
      if (i < total) out_blk[i] = v[u];
    }
  }
}

// Generic D and alignment: one workgroup per row, scalar lanes.
__global__ __launch_bounds__(kViewThreads) void rows_add_position_scalar_kernel(
    const float* __restrict__ src, int64_t n_src_rows, const int64_t* __restrict__ rows, int N, int64_t stride_b,
    int64_t stride_n, const float* __restrict__ pos, int D, float* __restrict__ out) {
  const int64_t R = blockIdx.x;
  const int64_t o = position_src_offset(rows, n_src_rows, R, N, stride_b, stride_n, D);
  const float* p = pos + (R % N) * D;
  for (int c = threadIdx.x; c < D; c += kViewThreads) out[R * D + c] = o < 0 ? qnan() : src[o + c] + p[c];
}

}  // namespace

size_t views_prepare_lds_bytes(int E, int D) { return ((size_t)E + D + kViewWaves) * sizeof(float); }

int32_t launch_views_prepare(const nrms_views_weights_t& w, float* state, hipStream_t s) {
  if (w.n_cat == 0) return NRMS_OK;
  hipLaunchKernelGGL(views_prepare_kernel, dim3((unsigned)(2 * w.n_cat)), dim3(kViewThreads),
                     views_prepare_lds_bytes(w.emb_dim, w.d_model), s, w, state);
  return launch_status();
}

int32_t launch_views_combine(const float* title, const float* title_logit, int64_t n, const int64_t* category,
                             const int64_t* subcategory, const float* state, int64_t C, int D, float* out,
                             hipStream_t s) {
  if (n == 0) return NRMS_OK;
  const int64_t blocks = (n + kRowsPerBlock - 1) / kRowsPerBlock;
  const float* sub_vec = state + C * D;
  const float* cat_logit = state + 2 * C * D;
  hipLaunchKernelGGL(views_combine_kernel, dim3((unsigned)blocks), dim3(kViewThreads), 0, s,
                     reinterpret_cast<const float4*>(title), title_logit, n, category, subcategory,
                     reinterpret_cast<const float4*>(state), reinterpret_cast<const float4*>(sub_vec), cat_logit,
                     cat_logit + C, C, D / 4, reinterpret_cast<float4*>(out));
  return launch_status();
}

int32_t launch_rows_add_position(const float* src, int64_t n_src_rows, const int64_t* rows, int64_t B, int N,
                                 int64_t stride_b, int64_t stride_n, const float* pos, int D, float* out,
                                 hipStream_t s) {
  const int64_t n_rows = B * N;
  if (n_rows == 0) return NRMS_OK;
  const bool aligned = D % 4 == 0 && (uintptr_t)src % 16 == 0 && (uintptr_t)pos % 16 == 0 && (uintptr_t)out % 16 == 0 &&
                       (rows || (stride_b % 4 == 0 && stride_n % 4 == 0));
  if (aligned) {
    const int64_t blocks = (n_rows + kRowsPerBlock - 1) / kRowsPerBlock;
    hipLaunchKernelGGL(rows_add_position_kernel, dim3((unsigned)blocks), dim3(kViewThreads), 0, s, src, n_src_rows,
                       rows, n_rows, N, stride_b, stride_n, reinterpret_cast<const float4*>(pos), D / 4,
                       reinterpret_cast<float4*>(out));
  } else {
    hipLaunchKernelGGL(rows_add_position_scalar_kernel, dim3((unsigned)n_rows), dim3(kViewThreads), 0, s, src,
                       n_src_rows, rows, N, stride_b, stride_n, pos, D, out);
  }
  return launch_status();
}

}  // namespace nrms
