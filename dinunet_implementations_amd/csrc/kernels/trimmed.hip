// Coordinate-wise trimmed mean / median over the sites' gradients (ops.trimmed.TrimmedState):
// rows[w * stride + i] is site w's value of coordinate i; of the W values of a coordinate the b
// smallest and the b largest are dropped and the rest averaged.  ops.reference.trimmed_mean is
// the numpy mirror, same bits:
//
//   key(x)   u = bits(x); u ^ 0x80000000 when the sign bit is clear, else ~u: unsigned order of
//            the keys is the IEEE total order (-NaN < -inf < ... < -0 < +0 < ... < +inf < +NaN)
//   order    the W entries ascending by (key, site): one 64-bit word (key << 4) | site each,
//            all distinct, so the order is strict and depends on the values alone
//   value    s = v[b]; s = s + v[b+1]; ...; s = s + v[W-1-b] in sorted order (fp32 adds), then
//            out = s * inv (inv = 1 / (W - 2b), made on the host) unless W - 2b == 1: no
//            division, no fused multiply-add
//   counts   trimmed[w] += the coordinates at which site w sat at a sorted position < b or
//            >= W - b (64-bit integer counters, cumulative)
//
//   tm_kernel<W>   each thread takes 4 consecutive coordinates per round (one 16-byte load from
//                  each of the W rows, one 16-byte store), grid-stride; the last n % 4 coordinates
//                  go one each to the first threads.  A coordinate is sorted by Batcher's odd-even
//                  merge network, fully unrolled on W register pairs (no LDS, no divergence); the
//                  value of a position is rebuilt from its key.  Which sites were trimmed is one
//                  W-bit mask per coordinate, added to W per-thread counters; at the end every
//                  thread adds its counters to the workgroup's LDS tallies, and the workgroup adds
//                  each non-zero tally with ONE 64-bit integer atomic: order-independent, so
//                  the counters are exact and a captured graph replays them.
//
// Sizes (W, n, b) are launch arguments; the rows are read from device memory at every launch.
#include <utility>

#include "common.h"

namespace {

constexpr int TM_THREADS = 256;
constexpr int TM_MAXW = 16;        // the peer exchange's limit (site index: 4 bits of the word)
constexpr int TM_BLOCKS_PER_CU = 4;

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned long long u64;

// Batcher's odd-even merge sort on the next power of two, the comparators that touch a wire
// >= W left out: those wires would hold +infinity pads, which no comparator moves
struct TmNet {
  int n;
  int a[80], b[80];
};

constexpr TmNet tm_make_net(int W) {
  TmNet net{};
  int P = 1;
  while (P < W) P *= 2;
  for (int p = 1; p < P; p *= 2)
    for (int k = p; k >= 1; k /= 2)
      for (int j = k % p; j + k < P; j += 2 * k)
        for (int i = 0; i < k && i + j + k < P; ++i)
          if ((i + j) / (2 * p) == (i + j + k) / (2 * p) && i + j + k < W) {
            net.a[net.n] = i + j;
            net.b[net.n] = i + j + k;
            ++net.n;
          }
  return net;
}

template <int W>
struct TmSort {
  static constexpr TmNet NET = tm_make_net(W);

  template <int A, int B>
  static __device__ __forceinline__ void ce(u64 (&k)[W]) {
    const u64 x = k[A], y = k[B];
    const bool lt = x < y;
    k[A] = lt ? x : y;
    k[B] = lt ? y : x;
  }

  template <size_t... I>
  static __device__ __forceinline__ void run(u64 (&k)[W], std::index_sequence<I...>) {
    (ce<NET.a[I], NET.b[I]>(k), ...);
  }

  static __device__ __forceinline__ void sort(u64 (&k)[W]) {
    run(k, std::make_index_sequence<(size_t)NET.n>{});
  }
};

__device__ __forceinline__ uint32_t tm_key(uint32_t u) {
  return (u & 0x80000000u) ? ~u : (u ^ 0x80000000u);
}
__device__ __forceinline__ uint32_t tm_unkey(uint32_t k) {
  return (k & 0x80000000u) ? (k ^ 0x80000000u) : ~k;
}

// one coordinate: bits[w] = site w's value; returns the trimmed mean, `mask` = the trimmed sites
template <int W>
__device__ __forceinline__ float tm_coord(const uint32_t (&bits)[W], int b, float inv,
                                          uint32_t& mask) {
  u64 k[W];
#pragma unroll
  for (int w = 0; w < W; ++w) k[w] = ((u64)tm_key(bits[w]) << 4) | (u64)w;
  TmSort<W>::sort(k);
  const int last = W - 1 - b;
  float s = 0.f;
  mask = 0u;
#pragma unroll
  for (int p = 0; p < W; ++p) {
    const float v = __uint_as_float(tm_unkey((uint32_t)(k[p] >> 4)));
    const uint32_t bit = 1u << ((uint32_t)k[p] & 15u);
    const bool kept = p >= b && p <= last;
    const float sum = __fadd_rn(s, v);
    s = kept ? (p == b ? v : sum) : s;
    mask |= kept ? 0u : bit;
  }
  return W - 2 * b == 1 ? s : __fmul_rn(s, inv);
}

template <int W>
__global__ void __launch_bounds__(TM_THREADS)
tm_kernel(const uint32_t* __restrict__ rows, long stride, long n, int b, float inv,
          float* __restrict__ out, u64* __restrict__ trimmed) {
  __shared__ unsigned int tally[TM_MAXW];
  if (threadIdx.x < TM_MAXW) tally[threadIdx.x] = 0u;
  __syncthreads();
  uint32_t cnt[W];
#pragma unroll
  for (int w = 0; w < W; ++w) cnt[w] = 0u;

  const long nvec = n >> 2;
  const long gtid = (long)blockIdx.x * TM_THREADS + threadIdx.x;
  const long gsz = (long)gridDim.x * TM_THREADS;
  for (long v = gtid; v < nvec; v += gsz) {
    u32x4 x[W];
#pragma unroll
    for (int w = 0; w < W; ++w)
      x[w] = *reinterpret_cast<const u32x4*>(rows + (long)w * stride + 4 * v);
    f32x4 r;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      uint32_t bits[W], mask;
#pragma unroll
      for (int w = 0; w < W; ++w) bits[w] = x[w][c];
      r[c] = tm_coord<W>(bits, b, inv, mask);
#pragma unroll
      for (int w = 0; w < W; ++w) cnt[w] += (mask >> w) & 1u;
    }
    *reinterpret_cast<f32x4*>(out + 4 * v) = r;
  }
  // the last n % 4 coordinates, one each to the first threads of the grid
  const long i = 4 * nvec + gtid;
  if (gtid < 4 && i < n) {
    uint32_t bits[W], mask;
#pragma unroll
    for (int w = 0; w < W; ++w) bits[w] = rows[(long)w * stride + i];
    out[i] = tm_coord<W>(bits, b, inv, mask);
#pragma unroll
    for (int w = 0; w < W; ++w) cnt[w] += (mask >> w) & 1u;
  }

#pragma unroll
  for (int w = 0; w < W; ++w)
    if (cnt[w]) atomicAdd(&tally[w], cnt[w]);
  __syncthreads();
  if (threadIdx.x < W && tally[threadIdx.x])
    atomicAdd(&trimmed[threadIdx.x], (u64)tally[threadIdx.x]);
}

int g_tm_max_blocks = 0;  // 0: from the CU count (dn_trimmed_set_max_blocks)

int tm_cus() {
  static int cus = 0;
  if (cus <= 0) {
    int dev = 0, c = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&c, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
        c <= 0) {
      (void)hipGetLastError();
      return 256;  // (not cached: asked again at the next launch)
    }
    cus = c;
  }
  return cus;
}

template <int W>
void tm_launch(const void* rows, long stride, long n, int b, float inv, float* out, void* trimmed,
               hipStream_t st) {
  // the grid is bounded by the CU count, never by n alone: every n runs the grid-stride loop
  const long items = (n >> 2) > 4 ? (n >> 2) : 4;  // (4 threads at the least: the scalar tail)
  long cap = (long)tm_cus() * TM_BLOCKS_PER_CU;
  if (g_tm_max_blocks > 0 && g_tm_max_blocks < cap) cap = g_tm_max_blocks;
  long blocks = (items + TM_THREADS - 1) / TM_THREADS;
  if (blocks > cap) blocks = cap;
  hipLaunchKernelGGL(tm_kernel<W>, dim3((unsigned)blocks), dim3(TM_THREADS), 0, st,
                     reinterpret_cast<const uint32_t*>(rows), stride, n, b, inv, out,
                     reinterpret_cast<u64*>(trimmed));
}

}  // namespace

DN_API int dn_trimmed_max_sites() { return TM_MAXW; }

// Bounds the launch's workgroups (0: the default, 4 per CU): the grid-stride loop can then be
// made to wrap at a small n.  Returns the previous bound.
DN_API int dn_trimmed_set_max_blocks(int blocks) {
  const int old = g_tm_max_blocks;
  g_tm_max_blocks = blocks > 0 ? blocks : 0;
  return old;
}

// rows: W rows of n fp32, `row_stride` elements apart (a multiple of 4, >= n) -> out (n fp32,
// every element written) = the mean of the W - 2b middle values per coordinate, inv = 1 / (W -
// 2b); trimmed_u64[w] (W 64-bit counters) += the coordinates at which site w was dropped
DN_API int dn_trimmed_mean(const void* rows, int W, long row_stride, long n, int b, float inv,
                           float* out, void* trimmed_u64, hipStream_t st) {
  if (n <= 0 || n >= (1L << 31) || W < 1 || W > TM_MAXW || b < 0 || 2 * b >= W || !rows || !out ||
      !trimmed_u64)
    return DN_BAD_SHAPE;
  if (row_stride < n || (row_stride & 3)) return DN_BAD_SHAPE;
  if (((uintptr_t)rows & 15) || ((uintptr_t)out & 15) || ((uintptr_t)trimmed_u64 & 7))
    return DN_BAD_SHAPE;
  switch (W) {
#define TM_CASE(w) \
  case w: tm_launch<w>(rows, row_stride, n, b, inv, out, trimmed_u64, st); break;
    TM_CASE(1) TM_CASE(2) TM_CASE(3) TM_CASE(4) TM_CASE(5) TM_CASE(6) TM_CASE(7) TM_CASE(8)
    TM_CASE(9) TM_CASE(10) TM_CASE(11) TM_CASE(12) TM_CASE(13) TM_CASE(14) TM_CASE(15) TM_CASE(16)
#undef TM_CASE
    default: return DN_BAD_SHAPE;
  }
  return dn_launch_status();
}
