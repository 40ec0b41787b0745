// FedAvg exchange (train.FedAvg): the model's parameters to and from one
// contiguous fp32 buffer, the buffer an all-reduce averages.
//   pack        flat[offset_t + i] = data_t[i]
//   unpack_div  data_t[i] = flat[offset_t + i] / divisor
// Both are streaming copies over every parameter in one launch per 32 tensors
// (the descriptors travel by value in the kernel arguments, as Adam's do:
// train.hip, AdamChunk), so the only floor is HBM traffic: 2 x 4 bytes per
// parameter per kernel.
//
// The quotient is the correctly rounded IEEE fp32 one (hipcc's default for
// `/`; this file must not be built with fast-math or
// -fno-hip-fp32-correctly-rounded-divide-sqrt): every rank computes the same
// bits numpy does, whatever the world size. divisor == 1 copies the bits.
#include <hip/hip_runtime.h>

#include "nrms_common.hpp"

namespace nrms {
namespace {

constexpr int kFlatChunk = 32;          // descriptors per launch: 32 x (24 + 8) B = 1 KB of kernarg
constexpr int kFlatThreads = 256;
constexpr int kFlatVecs = 4;            // float4 per thread of a full block
constexpr int64_t kFlatBlock = (int64_t)kFlatThreads * 4 * kFlatVecs;   // floats per block (4096)

struct FlatChunk {
  nrms_flat_tensor_t t[kFlatChunk];
  int64_t first_block[kFlatChunk];
};

template <bool kDiv>
__device__ __forceinline__ float4 quot(float4 v, float d) {
  if (kDiv) {
    v.x = v.x / d;
    v.y = v.y / d;
    v.z = v.z / d;
    v.w = v.w / d;
  }
  return v;
}

// One block moves floats [start, start + cnt) of its tensor, cnt <= kFlatBlock.
// start is a multiple of kFlatBlock, so the 16-byte alignment of both sides is
// that of the two bases: block-uniform. Aligned: float4 loads and stores (all
// loads of a full block issued before its stores), then a scalar tail of
// cnt % 4 floats; otherwise scalar throughout.
template <bool kDiv>
__device__ __forceinline__ void move_block(const float* __restrict__ src, float* __restrict__ dst,
                                           int64_t cnt, float divisor) {
  const int tid = threadIdx.x;
  const bool aligned = ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15) == 0;
  if (aligned) {
    const float4* s4 = reinterpret_cast<const float4*>(src);
    float4* d4 = reinterpret_cast<float4*>(dst);
    if (cnt == kFlatBlock) {
      float4 v[kFlatVecs];
#pragma unroll
      for (int k = 0; k < kFlatVecs; ++k) v[k] = s4[k * kFlatThreads + tid];
#pragma unroll
      for (int k = 0; k < kFlatVecs; ++k) d4[k * kFlatThreads + tid] = quot<kDiv>(v[k], divisor);
      return;
    }
    const int64_t n4 = cnt >> 2;
    for (int64_t i = tid; i < n4; i += kFlatThreads) d4[i] = quot<kDiv>(s4[i], divisor);
    const int64_t i = (n4 << 2) + tid;
    if (i < cnt) dst[i] = kDiv ? src[i] / divisor : src[i];
    return;
  }
  for (int64_t i = tid; i < cnt; i += kFlatThreads) dst[i] = kDiv ? src[i] / divisor : src[i];
}

// kUnpack: flat -> tensors (divided when kDiv), else tensors -> flat.
template <bool kUnpack, bool kDiv>
__global__ __launch_bounds__(kFlatThreads) void flat_kernel(const FlatChunk c, int n, float* flat,
                                                            float divisor) {
  const int64_t b = blockIdx.x;
  int t = 0;
  while (t + 1 < n && c.first_block[t + 1] <= b) ++t;
  const nrms_flat_tensor_t d = c.t[t];
  const int64_t start = (b - c.first_block[t]) * kFlatBlock;
  if (start >= d.numel) return;
  const int64_t cnt = d.numel - start < kFlatBlock ? d.numel - start : kFlatBlock;
  float* p = d.data + start;
  float* f = flat + d.offset + start;
  if (kUnpack)
    move_block<kDiv>(f, p, cnt, divisor);
  else
    move_block<false>(p, f, cnt, 1.0f);
}

template <bool kUnpack, bool kDiv>
int32_t launch_flat(const nrms_flat_tensor_t* ts, int n, float* flat, float divisor, hipStream_t s) {
  for (int base = 0; base < n; base += kFlatChunk) {
    FlatChunk c{};
    const int k = n - base < kFlatChunk ? n - base : kFlatChunk;
    int64_t blocks = 0;
    for (int i = 0; i < k; ++i) {
      c.t[i] = ts[base + i];
      c.first_block[i] = blocks;          // numel == 0: an empty range, never selected
      blocks += (ts[base + i].numel + kFlatBlock - 1) / kFlatBlock;
    }
    if (blocks == 0) continue;
    if (blocks > INT32_MAX) return NRMS_ERR_UNSUPPORTED;
    hipLaunchKernelGGL((flat_kernel<kUnpack, kDiv>), dim3((unsigned)blocks), dim3(kFlatThreads), 0, s, c, k,
                       flat, divisor);
    if (int32_t st = launch_status()) return st;
  }
  return NRMS_OK;
}

}  // namespace

int32_t launch_params_pack(const nrms_flat_tensor_t* ts, int n, float* flat, hipStream_t s) {
  return launch_flat<false, false>(ts, n, flat, 1.0f, s);
}

int32_t launch_params_unpack_div(const nrms_flat_tensor_t* ts, int n, const float* flat, float divisor,
                                 hipStream_t s) {
  float* f = const_cast<float*>(flat);    // read only on this route
  return divisor == 1.0f ? launch_flat<true, false>(ts, n, f, divisor, s)
                         : launch_flat<true, true>(ts, n, f, divisor, s);
}

}  // namespace nrms
