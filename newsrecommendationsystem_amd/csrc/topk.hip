// Catalogue-wide top-K recommendation (nrms_recommend_topk): a tiled
// users x news GEMM on the matrix cores with a per-user running top-K' fused
// into the epilogue. The [n_users, n_news] score matrix is never written;
// only K' = K + n_excl survivors per (user, news chunk) leave the kernel, and
// a second small kernel merges the chunks' lists, drops the excluded rows and
// writes the sorted [n_users, K] result.
//
// Arithmetic (nrms_get_gemm_arith at enqueue time):
//   F32                         v_mfma_f32_16x16x4_f32, exact fp32 products;
//   SPLIT_BF16X6 / SPLIT_F16X3  split-bf16 x6 on v_mfma_f32_16x16x32_bf16: the
//     exact three-plane split (split3x2) of both operands while they are staged
//     into LDS and the six products with i + j <= 2, the scheme of
//     gemm_x6_kernel (gemm_f32.hip).
// There is no fp16-plane form: news and user vectors carry no range guarantee,
// and fp16 planes would need a range recheck pass this operation does not
// justify, so SPLIT_F16X3 runs the bf16 planes here. (An infinite operand
// splits into inf + NaN: in the split modes its scores are NaN, as in every
// split GEMM of this library.)
//
// Structure: one workgroup (4 waves as 2 x 2, wave tile 32 x 96) owns 64 users
// and one chunk of the news rows, streamed in 192-row tiles through the
// K-staged loop of gemm_x6_tile. Workgroups that share a chunk get contiguous
// logical ids (xcd_remap), so they stream it through one XCD's L2.
//
// Order: candidates are compared as one 64-bit key. High word: the
// order-preserving bit flip of the score, -0 folded into +0 and every NaN
// mapped to 0, below -inf. Low word: ~row, so equal scores prefer the smaller
// row. Keys of distinct rows are distinct, 0 is the empty slot.
//
// Filter: each user row keeps a threshold (its K'-th best key so far) in LDS
// and a candidate buffer of kCap keys in the workspace. A score that passes
// the fp32 pre-test against the threshold's score and then the exact key
// compare is appended (LDS counter, one 8-byte store). A tile appends at most
// 192 keys per user, so a buffer holding more than kCap - 192 after a tile is
// reduced before the next one: one wave per user finds the K'-th largest key
// by bitwise binary search over ballot counts, keeps exactly the K' keys at
// or above it and raises the threshold. A threshold is always the K'-th best
// of keys already seen, so no member of the chunk's true top K' is dropped
// and the survivors do not depend on the order of appends, on the chunking
// or on the grid. Excluded rows are dropped in the merge only: they displace
// at most n_excl of the K' survivors.
//
// Resources (gfx950): the split kernel 187 VGPRs,
// 50 KB of LDS, no scratch, two workgroups per CU; under a three-per-CU
// bound it spilled 22 VGPRs with a reload in every k step and ran 8 % slower.
#include "nrms_common.hpp"

namespace nrms {
namespace {

constexpr int kD = 300;
constexpr int kThreads = 256;
constexpr int UT = 64;        // users per workgroup
constexpr int NT = 192;       // news rows per tile
constexpr int BK = 32;        // k depth of one staged chunk
constexpr int XLD = 32;       // bf16 per LDS row (split planes)
constexpr int FLD = 40;       // floats per LDS row (f32 path), as gemm_xwt_f32_kernel
constexpr int kCapSmall = 512, kCapLarge = 1024;   // candidate slots per user
constexpr int kKpSmall = 128;                      // K' up to here: kCapSmall
constexpr int kMergeMax = 4096;                    // keys one merge block holds in LDS
constexpr int kMaxChunks = 64;
constexpr int kTargetWgs = 2048;                   // 8 per CU: chunk count for few users

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ int xsw(int r) { return ((r >> 3) & 1) << 1; }   // gemm_f32.hip

__device__ __forceinline__ void split4(const float4 v, bf16x4& h, bf16x4& m, bf16x4& l) {
  uint32_t h0, m0, l0, h1, m1, l1;
  split3x2(v.x, v.y, h0, m0, l0);
  split3x2(v.z, v.w, h1, m1, l1);
  h = __builtin_bit_cast(bf16x4, make_uint2(h0, h1));
  m = __builtin_bit_cast(bf16x4, make_uint2(m0, m1));
  l = __builtin_bit_cast(bf16x4, make_uint2(l0, l1));
}

__device__ __forceinline__ uint32_t key_hi(float s) {
  uint32_t b = __float_as_uint(s);
  if (s != s) return 0u;
  if (b == 0x80000000u) b = 0u;
  return b ^ ((uint32_t)((int32_t)b >> 31) | 0x80000000u);
}
__device__ __forceinline__ float key_score(uint32_t hi) {
  if (hi == 0u) return qnan();
  return __uint_as_float((hi & 0x80000000u) ? (hi ^ 0x80000000u) : ~hi);
}

// Staging sources of one tile: user rows u0 .. u0 + 63 (A) and news rows
// n0 .. n0 + 191 below n_end (B); rows outside are staged as zeros. a / b
// point at this thread's first row and k column (row tid >> 3, k 4 (tid & 7));
// its other rows lie 32 rows further each.
struct TileSrc {
  const float* a;
  const float* b;
  int a_rows, b_rows;   // valid rows of the tile
};
__device__ __forceinline__ TileSrc tile_src(const float* __restrict__ user, int64_t n_users, int64_t u0,
                                            const float* __restrict__ news, int64_t n0, int64_t n_end,
                                            int tid) {
  TileSrc t;
  const int off = (tid >> 3) * kD + (tid & 7) * 4;
  t.a = user + u0 * kD + off;
  t.b = news + n0 * kD + off;
  t.a_rows = n_users - u0 < UT ? (int)(n_users - u0) : UT;
  t.b_rows = n_end - n0 < NT ? (int)(n_end - n0) : NT;
  return t;
}

__device__ __forceinline__ void gload(const TileSrc& t, int kc, int lrow, int lc4, float4 (&ra)[2],
                                      float4 (&rb)[6]) {
  const bool kin = kc * BK + lc4 * 4 < kD;
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    ra[p] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (kin && lrow + 32 * p < t.a_rows) ra[p] = *reinterpret_cast<const float4*>(t.a + 32 * p * kD + kc * BK);
  }
#pragma unroll
  for (int p = 0; p < 6; ++p) {
    rb[p] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (kin && lrow + 32 * p < t.b_rows) rb[p] = *reinterpret_cast<const float4*>(t.b + 32 * p * kD + kc * BK);
  }
}

// acc[mt][nt][r]: user row 32 wm + 16 mt + 4 (lane >> 4) + r, news row
// 96 wn + 16 nt + (lane & 15) of the tile. Every element accumulates its k
// terms in the same order wherever it sits in a tile, a chunk or the grid.
// nt_live: N tiles of this wave that hold rows below n_end (wave-uniform).
__device__ __forceinline__ void x6_tile(const TileSrc& t, int nt_live, floatx4 (&acc)[2][6],
                                        __bf16* __restrict__ As, __bf16* __restrict__ Bs) {
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave & 1, wn = wave >> 1;
  const int lrow = tid >> 3, lc4 = tid & 7;
  float4 ra[2], rb[6];
  auto lstore = [&]() {
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      bf16x4 h, m, l;
      split4(ra[p], h, m, l);
      const int r = lrow + 32 * p;
      __bf16* d = As + r * XLD + (((lc4 >> 1) ^ xsw(r)) << 3) + (lc4 & 1) * 4;
      *reinterpret_cast<bf16x4*>(d) = h;
      *reinterpret_cast<bf16x4*>(d + UT * XLD) = m;
      *reinterpret_cast<bf16x4*>(d + 2 * UT * XLD) = l;
    }
#pragma unroll
    for (int p = 0; p < 6; ++p) {
      bf16x4 h, m, l;
      split4(rb[p], h, m, l);
      const int r = lrow + 32 * p;
      __bf16* d = Bs + r * XLD + (((lc4 >> 1) ^ xsw(r)) << 3) + (lc4 & 1) * 4;
      *reinterpret_cast<bf16x4*>(d) = h;
      *reinterpret_cast<bf16x4*>(d + NT * XLD) = m;
      *reinterpret_cast<bf16x4*>(d + 2 * NT * XLD) = l;
    }
  };
  const int lm = lane & 15, kq = lane >> 4;
  const __bf16* Aw = As + (32 * wm + lm) * XLD + ((kq ^ xsw(lm)) << 3);
  const __bf16* Bw = Bs + (96 * wn + lm) * XLD + ((kq ^ xsw(lm)) << 3);
  constexpr int nk = (kD + BK - 1) / BK;
  gload(t, 0, lrow, lc4, ra, rb);
  lstore();
  __syncthreads();
  for (int kc = 0; kc < nk; ++kc) {
    if (kc + 1 < nk) gload(t, kc + 1, lrow, lc4, ra, rb);
    bf16x8 a[2][3];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int pl = 0; pl < 3; ++pl)
        a[mt][pl] = *reinterpret_cast<const bf16x8*>(Aw + pl * UT * XLD + 16 * mt * XLD);
#pragma unroll
    for (int nt = 0; nt < 6; ++nt) {
      if (nt >= nt_live) break;
      bf16x8 b[3];
#pragma unroll
      for (int pl = 0; pl < 3; ++pl)
        b[pl] = *reinterpret_cast<const bf16x8*>(Bw + pl * NT * XLD + 16 * nt * XLD);
      // the six products with i + j <= 2, smallest first
#define NRMS_X6(PA, PB)                                                                             \
  _Pragma("unroll") for (int mt = 0; mt < 2; ++mt)                                                   \
      acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[mt][PA], b[PB], acc[mt][nt], 0, 0, 0);
      NRMS_X6(2, 0) NRMS_X6(1, 1) NRMS_X6(0, 2) NRMS_X6(1, 0) NRMS_X6(0, 1) NRMS_X6(0, 0)
#undef NRMS_X6
    }
    __syncthreads();
    if (kc + 1 < nk) {
      lstore();
      __syncthreads();
    }
  }
}

// The same tile on v_mfma_f32_16x16x4_f32: MFMA step (c, t) gives lane group
// kq the k index 16 c + 4 kq + t for A and B alike (gemm_tile, gemm_f32.hip).
__device__ __forceinline__ void f32_tile(const TileSrc& t, int nt_live, floatx4 (&acc)[2][6],
                                         float* __restrict__ As, float* __restrict__ Bs) {
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave & 1, wn = wave >> 1;
  const int lrow = tid >> 3, lc4 = tid & 7;
  float4 ra[2], rb[6];
  auto lstore = [&]() {
#pragma unroll
    for (int p = 0; p < 2; ++p) *reinterpret_cast<float4*>(&As[(lrow + 32 * p) * FLD + lc4 * 4]) = ra[p];
#pragma unroll
    for (int p = 0; p < 6; ++p) *reinterpret_cast<float4*>(&Bs[(lrow + 32 * p) * FLD + lc4 * 4]) = rb[p];
  };
  const int lm = lane & 15, kq = lane >> 4;
  const float* Aw = As + (32 * wm + lm) * FLD + 4 * kq;
  const float* Bw = Bs + (96 * wn + lm) * FLD + 4 * kq;
  constexpr int nk = (kD + BK - 1) / BK;
  gload(t, 0, lrow, lc4, ra, rb);
  lstore();
  __syncthreads();
  for (int kc = 0; kc < nk; ++kc) {
    if (kc + 1 < nk) gload(t, kc + 1, lrow, lc4, ra, rb);
#pragma unroll
    for (int c = 0; c < BK / 16; ++c) {
      if (kc * BK + 16 * c >= kD) break;   // the zero-padded half chunk past k = 300
      float4 a[2];
#pragma unroll
      for (int mt = 0; mt < 2; ++mt) a[mt] = *reinterpret_cast<const float4*>(Aw + 16 * mt * FLD + 16 * c);
#pragma unroll
      for (int nt = 0; nt < 6; ++nt) {
        if (nt >= nt_live) break;
        const float4 b = *reinterpret_cast<const float4*>(Bw + 16 * nt * FLD + 16 * c);
#define NRMS_F4(F)                                                                              \
  _Pragma("unroll") for (int mt = 0; mt < 2; ++mt)                                               \
      acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[mt].F, b.F, acc[mt][nt], 0, 0, 0);
        NRMS_F4(x) NRMS_F4(y) NRMS_F4(z) NRMS_F4(w)
#undef NRMS_F4
      }
    }
    __syncthreads();
    if (kc + 1 < nk) {
      lstore();
      __syncthreads();
    }
  }
}

__device__ __forceinline__ int wave_count(bool p) { return __popcll(__ballot(p)); }

// One wave reduces one user's n > kp candidate keys (buf[0 .. n), n <= 64 EPL)
// to the kp largest, compacted into buf[0 .. kp); returns the kp-th largest
// key's high word (the new threshold; its low word in *tlo).
template <int EPL>
__device__ __forceinline__ uint32_t reduce_user(uint64_t* __restrict__ buf, int n, int kp, uint32_t* tlo) {
  const int lane = threadIdx.x & 63;
  uint32_t hi[EPL], lo[EPL];
#pragma unroll
  for (int e = 0; e < EPL; ++e) {
    const int i = e * 64 + lane;
    const uint64_t k = i < n ? buf[i] : 0ull;
    hi[e] = (uint32_t)(k >> 32);
    lo[e] = (uint32_t)k;
  }
  // largest Th with #{hi >= Th} >= kp (empty slots are hi = 0, never counted: c >= 1)
  uint32_t th = 0;
  for (int b = 31; b >= 0; --b) {
    const uint32_t c = th | (1u << b);
    int cnt = 0;
#pragma unroll
    for (int e = 0; e < EPL; ++e) cnt += wave_count(hi[e] >= c);
    if (cnt >= kp) th = c;
  }
  int gt = 0, eq = 0;
#pragma unroll
  for (int e = 0; e < EPL; ++e) {
    gt += wave_count(hi[e] > th);
    eq += wave_count(hi[e] == th && lo[e] != 0u);
  }
  const int need = kp - gt;   // >= 1 of the eq keys at the threshold score survive
  uint32_t tl = 0;
  if (eq != need) {
    for (int b = 31; b >= 0; --b) {
      const uint32_t c = tl | (1u << b);
      int cnt = 0;
#pragma unroll
      for (int e = 0; e < EPL; ++e) cnt += wave_count(hi[e] == th && lo[e] >= c);
      if (cnt >= need) tl = c;
    }
  }
  int base = 0;
#pragma unroll
  for (int e = 0; e < EPL; ++e) {
    const bool keep = hi[e] > th || (hi[e] == th && lo[e] != 0u && lo[e] >= tl);
    const uint64_t m = __ballot(keep);
    const int pos = base + __popcll(m & ((1ull << lane) - 1ull));
    if (keep && pos < kp) buf[pos] = ((uint64_t)hi[e] << 32) | lo[e];
    base += __popcll(m);
  }
  *tlo = tl;
  return th;
}

template <bool F32>
__global__ __launch_bounds__(kThreads, 2) void topk_scan_kernel(
    const float* __restrict__ news, int64_t n_news, const float* __restrict__ user, int64_t n_users,
    int kp, int cap, int64_t chunk_rows, int n_tiles, uint64_t* __restrict__ ws_buf,
    int32_t* __restrict__ ws_cnt) {
  __shared__ __attribute__((aligned(16))) char smem[F32 ? (UT + NT) * FLD * 4 : 3 * (UT + NT) * XLD * 2];
  __shared__ int s_cnt[UT];
  __shared__ uint64_t s_thr[UT];
  __shared__ float s_thrf[UT];

  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave & 1, wn = wave >> 1;
  const int lm = lane & 15, kq = lane >> 4;
  const int wg = xcd_remap(blockIdx.x, gridDim.x);
  const int chunk = wg / n_tiles, tile = wg % n_tiles;
  const int64_t u0 = (int64_t)tile * UT;
  const int64_t c_lo = (int64_t)chunk * chunk_rows;
  const int64_t c_hi = c_lo + chunk_rows < n_news ? c_lo + chunk_rows : n_news;
  const int64_t slot0 = ((int64_t)chunk * n_tiles + tile) * UT;
  uint64_t* __restrict__ buf = ws_buf + slot0 * cap;

  if (tid < UT) {
    s_cnt[tid] = 0;
    s_thr[tid] = 0ull;
    s_thrf[tid] = u0 + tid < n_users ? -__builtin_inff() : __builtin_inff();
  }
  __syncthreads();

  for (int64_t n0 = c_lo; n0 < c_hi; n0 += NT) {
    floatx4 acc[2][6];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int nt = 0; nt < 6; ++nt) acc[mt][nt] = floatx4{0.f, 0.f, 0.f, 0.f};
    int nt_live;
    {
      const int64_t live = (c_hi - (n0 + 96 * wn) + 15) / 16;
      nt_live = live < 0 ? 0 : (live < 6 ? (int)live : 6);
    }
    const TileSrc src = tile_src(user, n_users, u0, news, n0, c_hi, tid);
    if constexpr (F32)
      f32_tile(src, nt_live, acc, reinterpret_cast<float*>(smem), reinterpret_cast<float*>(smem) + UT * FLD);
    else
      x6_tile(src, nt_live, acc, reinterpret_cast<__bf16*>(smem), reinterpret_cast<__bf16*>(smem) + 3 * UT * XLD);

    // filter: fp32 pre-test against the threshold's score (a NaN passes it),
    // then the exact key compare
    float tf[2][4];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int r = 0; r < 4; ++r) tf[mt][r] = s_thrf[32 * wm + 16 * mt + 4 * kq + r];
#pragma unroll
    for (int nt = 0; nt < 6; ++nt) {
      if (nt >= nt_live) break;
      const int64_t col = n0 + 96 * wn + 16 * nt + lm;
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float s = acc[mt][nt][r];
          if (!(s < tf[mt][r]) && col < c_hi) {
            const int ul = 32 * wm + 16 * mt + 4 * kq + r;
            if (u0 + ul < n_users) {
              const uint64_t key = ((uint64_t)key_hi(s) << 32) | (uint32_t)~(uint32_t)col;
              if (key > s_thr[ul]) {
                const int slot = atomicAdd(&s_cnt[ul], 1);
                if (slot < cap) buf[ul * cap + slot] = key;
              }
            }
          }
        }
    }
    __syncthreads();
    // a tile appends at most NT keys per user: reduce what could overflow next
    const bool last = n0 + NT >= c_hi;
    for (int i = 0; i < UT / 4; ++i) {
      const int ul = wave * (UT / 4) + i;
      const int n = __builtin_amdgcn_readfirstlane(s_cnt[ul]);
      if (n > (last ? kp : cap - NT)) {
        uint32_t tl;
        uint64_t* b = buf + (int64_t)ul * cap;
        const int nn = n < cap ? n : cap;
        const uint32_t th = cap <= kCapSmall ? reduce_user<kCapSmall / 64>(b, nn, kp, &tl)
                                             : reduce_user<kCapLarge / 64>(b, nn, kp, &tl);
        if (lane == 0) {
          s_cnt[ul] = kp;
          s_thr[ul] = ((uint64_t)th << 32) | tl;
          s_thrf[ul] = th == 0u ? -__builtin_inff() : key_score(th);
        }
      }
    }
    __syncthreads();
  }
  if (tid < UT) {
    const int n = s_cnt[tid];
    ws_cnt[slot0 + tid] = n < kp ? n : kp;
  }
}

// One block per user: gather the chunks' survivors, drop the excluded rows,
// rank the rest by counting and write the K best in order, then the padding.
__global__ __launch_bounds__(kThreads) void topk_merge_kernel(
    const uint64_t* __restrict__ ws_buf, const int32_t* __restrict__ ws_cnt, int n_chunks, int n_tiles,
    int kp, int cap, int64_t n_news, const int64_t* __restrict__ exclude, int n_excl, int K,
    int64_t* __restrict__ out_idx, float* __restrict__ out_score) {
  __shared__ uint64_t s_key[kMergeMax];
  __shared__ uint32_t s_ex[256];
  __shared__ int s_valid;
  const int64_t u = blockIdx.x;
  const int tid = threadIdx.x;
  const int M = n_chunks * kp;
  if (tid == 0) s_valid = 0;
  for (int i = tid; i < n_excl; i += kThreads) {
    const int64_t v = exclude[u * n_excl + i];
    s_ex[i] = (v >= 0 && v < n_news) ? (uint32_t)v : 0xffffffffu;   // out of range: matches no row
  }
  __syncthreads();
  int mine = 0;
  for (int m = tid; m < M; m += kThreads) {
    const int c = m / kp, j = m - c * kp;
    const int64_t slot = ((int64_t)c * n_tiles + u / UT) * UT + u % UT;
    uint64_t key = j < ws_cnt[slot] ? ws_buf[slot * cap + j] : 0ull;
    const uint32_t row = ~(uint32_t)key;
    for (int i = 0; i < n_excl; ++i)
      if (s_ex[i] == row) key = 0ull;
    s_key[m] = key;
    mine += key != 0ull;
  }
  if (mine) atomicAdd(&s_valid, mine);
  __syncthreads();
  for (int m = tid; m < M; m += kThreads) {
    const uint64_t key = s_key[m];
    if (key == 0ull) continue;
    int rank = 0;
    for (int j = 0; j < M; ++j) rank += s_key[j] > key;
    if (rank < K) {
      out_idx[u * K + rank] = (int64_t)(uint32_t)~(uint32_t)key;
      out_score[u * K + rank] = key_score((uint32_t)(key >> 32));
    }
  }
  for (int j = s_valid + tid; j < K; j += kThreads) {
    out_idx[u * K + j] = -1;
    out_score[u * K + j] = qnan();
  }
}

// NRMS_TOPK_CHUNK in the environment (read once): news rows per chunk, so that
// tests can force several chunks at a small n_news.
int64_t topk_chunk_knob() {
  static const int64_t knob = [] {
    const char* e = env_knob("NRMS_TOPK_CHUNK");
    const int64_t v = e ? (int64_t)atoll(e) : (int64_t)0;
    return v > 0 ? v : (int64_t)0;
  }();
  return knob;
}

// News rows per chunk. Default: one chunk when the user tiles alone fill the
// CUs several times over, else enough chunks for about kTargetWgs workgroups,
// in whole tiles. Never more chunks than one merge block can hold (kMergeMax
// keys, kMaxChunks).
int64_t topk_chunk_rows(int64_t tiles, int64_t n_news, int kp) {
  if (n_news <= 0) return NT;
  int64_t max_chunks = kMergeMax / kp;
  if (max_chunks > kMaxChunks) max_chunks = kMaxChunks;
  int64_t rows = topk_chunk_knob();
  if (rows == 0) {
    int64_t want = tiles >= kTargetWgs * 3 / 4 ? 1 : (kTargetWgs + tiles - 1) / (tiles > 0 ? tiles : 1);
    if (want > max_chunks) want = max_chunks;
    rows = (n_news + want - 1) / want;
    if (rows < 2 * NT) rows = 2 * NT;
    rows = (rows + NT - 1) / NT * NT;
  }
  if ((n_news + rows - 1) / rows > max_chunks) rows = ((n_news + max_chunks - 1) / max_chunks + 63) / 64 * 64;
  return rows;
}

// The workspace: one count and `cap` keys per (chunk, user tile, user) slot.
// It is sized for a bound on chunks x tiles that depends on n_users alone and
// grows with it (the chunk count itself shrinks as users are added), so the
// size is monotone in n_users and in K: tiles x chunks < tiles + kTargetWgs by
// the default policy, <= kMaxChunks tiles always.
struct TopkPlan {
  int kp, cap, n_tiles, n_chunks;
  int64_t chunk_rows;
  size_t cnt_bytes, buf_bytes;
};
TopkPlan topk_plan(int64_t n_users, int64_t n_news, int K, int n_excl) {
  TopkPlan p;
  p.kp = K + n_excl;
  p.cap = p.kp <= kKpSmall ? kCapSmall : kCapLarge;
  const int64_t tiles = (n_users + UT - 1) / UT;
  p.n_tiles = (int)tiles;
  p.chunk_rows = topk_chunk_rows(tiles, n_news, p.kp);
  p.n_chunks = (int)((n_news + p.chunk_rows - 1) / p.chunk_rows);
  int64_t bound = tiles * kMaxChunks;
  if (topk_chunk_knob() == 0 && tiles + kTargetWgs - 1 < bound) bound = tiles + kTargetWgs - 1;
  if (bound < 1) bound = 1;
  const size_t slots = (size_t)bound * UT;
  p.cnt_bytes = (slots * sizeof(int32_t) + 255) & ~(size_t)255;
  p.buf_bytes = slots * (size_t)p.cap * sizeof(uint64_t);
  return p;
}

}  // namespace

size_t topk_workspace_bytes(int64_t n_users, int64_t n_news, int K, int n_excl) {
  const TopkPlan p = topk_plan(n_users, n_news, K, n_excl);
  return p.cnt_bytes + p.buf_bytes;
}

int32_t launch_topk(const float* news, int64_t n_news, const float* user, int64_t n_users,
                    const int64_t* exclude, int n_excl, int K, int64_t* out_idx, float* out_score,
                    void* ws, size_t ws_bytes, hipStream_t s) {
  const TopkPlan p = topk_plan(n_users, n_news, K, n_excl);
  if (ws_bytes < p.cnt_bytes + p.buf_bytes) return NRMS_ERR_WORKSPACE;
  if (n_users > INT32_MAX || (int64_t)p.n_chunks * p.n_tiles > INT32_MAX) return NRMS_ERR_UNSUPPORTED;
  if ((size_t)p.n_chunks * (size_t)p.n_tiles * UT * (size_t)p.cap * sizeof(uint64_t) > p.buf_bytes)
    return NRMS_ERR_WORKSPACE;   // (the plan never exceeds its own bound)
  int32_t* cnt = reinterpret_cast<int32_t*>(ws);
  uint64_t* buf = reinterpret_cast<uint64_t*>(reinterpret_cast<char*>(ws) + p.cnt_bytes);
  if (p.n_chunks > 0) {
    const dim3 grid((unsigned)(p.n_chunks * p.n_tiles));
    if (gemm_arith() == NRMS_GEMM_F32)
      hipLaunchKernelGGL(topk_scan_kernel<true>, grid, dim3(kThreads), 0, s, news, n_news, user, n_users,
                         p.kp, p.cap, p.chunk_rows, p.n_tiles, buf, cnt);
    else
      hipLaunchKernelGGL(topk_scan_kernel<false>, grid, dim3(kThreads), 0, s, news, n_news, user, n_users,
                         p.kp, p.cap, p.chunk_rows, p.n_tiles, buf, cnt);
    if (int32_t st = launch_status()) return st;
  }
  hipLaunchKernelGGL(topk_merge_kernel, dim3((unsigned)n_users), dim3(kThreads), 0, s, buf, cnt, p.n_chunks,
                     p.n_tiles, p.kp, p.cap, n_news, exclude, n_excl, K, out_idx, out_score);
  return launch_status();
}

}  // namespace nrms
