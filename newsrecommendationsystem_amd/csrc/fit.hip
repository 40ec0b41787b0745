// Kernels under the fit loop (newsrecommendationsystem_amd/fit.py): the batch
// assembly of BaseDataset.__getitem__ + default collate (src/dataset.py:64-85)
// from a device-resident training set, and CrossEntropyLoss against class 0
// with its gradient (src/train.py:205-206) in one launch.
#include <math.h>

#include "nrms_common.hpp"

namespace nrms {
namespace {

constexpr int kBatchGatherThreads = 256;

// One 8-byte element per lane: element e of the batch is word l of title
// t = e / L, titles [0, B C) being the candidates and [B C, B (C + N)) the
// clicked ones. Consecutive lanes write consecutive words (each output is one
// contiguous run) and read consecutive words of a title row; rows of odd L
// are only 8-byte aligned, so nothing wider than one word is moved. An index
// outside its table is never dereferenced: the words it addresses are zeros.
__global__ __launch_bounds__(kBatchGatherThreads) void train_batch_gather_kernel(
    const int64_t* __restrict__ titles, int64_t n_title_rows, int L, const int32_t* __restrict__ sample_rows,
    int64_t n_samples, int C, int N, const int64_t* __restrict__ sample_idx, int64_t B,
    int64_t* __restrict__ cand_ids, int64_t* __restrict__ clicked_ids) {
  const int64_t n_cand = B * C * L;
  const int64_t total = n_cand + B * N * L;
  const int64_t e = (int64_t)blockIdx.x * kBatchGatherThreads + threadIdx.x;
  if (e >= total) return;
  int64_t b, w;   // sample of the batch, word within the sample's C (or N) titles
  int j0;
  int64_t* out;
  if (e < n_cand) {
    b = e / ((int64_t)C * L);
    w = e - b * C * L;
    j0 = 0;
    out = cand_ids + e;
  } else {
    const int64_t r = e - n_cand;
    b = r / ((int64_t)N * L);
    w = r - b * N * L;
    j0 = C;
    out = clicked_ids + r;
  }
  const int j = (int)(w / L);
  const int l = (int)(w - (int64_t)j * L);
  int64_t v = 0;
  const int64_t s = sample_idx[b];
  if ((uint64_t)s < (uint64_t)n_samples) {
    const int64_t row = sample_rows[s * (C + N) + j0 + j];
    if ((uint64_t)row < (uint64_t)n_title_rows) v = titles[row * L + l];
  }
  *out = v;
}

constexpr int kXentWaves = 16;

// One workgroup; wave w takes rows w, w + 16, ... in turn, lanes stride over
// the C classes. Row maximum subtracted first (torch's log_softmax): a row
// holding +inf or NaN gives NaN. The per-row losses are added in fp64, each
// wave's in row order and the 16 partial sums in wave order, so the mean is
// the same bits on every call (no atomics).
__global__ __launch_bounds__(kXentWaves * kWave) void xent_class0_kernel(
    const float* __restrict__ logits, int64_t B, int C, float* __restrict__ dlogits,
    float* __restrict__ loss_out) {
  __shared__ double part[kXentWaves];
  const int lane = threadIdx.x & (kWave - 1);
  const int w = threadIdx.x / kWave;
  const float fB = (float)B;
  double acc = 0.0;
  for (int64_t b = w; b < B; b += kXentWaves) {
    const float* z = logits + b * C;
    float m = -INFINITY;
    for (int c = lane; c < C; c += kWave) m = nan_max(m, z[c]);
    m = wave_max_nan(m);
    float s = 0.f;
    for (int c = lane; c < C; c += kWave) s += expf(z[c] - m);
    s = wave_sum(s);
    acc += (double)(logf(s) - (z[0] - m));
    float* dz = dlogits + b * C;
    for (int c = lane; c < C; c += kWave) dz[c] = (expf(z[c] - m) / s - (c == 0 ? 1.f : 0.f)) / fB;
  }
  if (lane == 0) part[w] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int i = 0; i < kXentWaves; ++i) t += part[i];
    loss_out[0] = (float)(t / (double)B);
  }
}

}  // namespace

int32_t launch_train_batch_gather(const int64_t* titles, int64_t n_title_rows, int L, const int32_t* sample_rows,
                                  int64_t n_samples, int C, int N, const int64_t* sample_idx, int64_t B,
                                  int64_t* cand_ids, int64_t* clicked_ids, hipStream_t s) {
  const int64_t total = B * ((int64_t)C + N) * L;
  if (total == 0) return NRMS_OK;
  const int64_t blocks = (total + kBatchGatherThreads - 1) / kBatchGatherThreads;
  if (blocks > INT32_MAX) return NRMS_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(train_batch_gather_kernel, dim3((unsigned)blocks), dim3(kBatchGatherThreads), 0, s, titles,
                     n_title_rows, L, sample_rows, n_samples, C, N, sample_idx, B, cand_ids, clicked_ids);
  return launch_status();
}

int32_t launch_xent_class0(const float* logits, int64_t B, int C, float* dlogits, float* loss_out,
                           hipStream_t s) {
  hipLaunchKernelGGL(xent_class0_kernel, dim3(1), dim3(kXentWaves * kWave), 0, s, logits, B, C, dlogits,
                     loss_out);
  return launch_status();
}

}  // namespace nrms
