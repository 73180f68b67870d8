// Top-k sparsified gradient release with error feedback (ops.topk.TopKState): of acc = g + err
// the k entries of largest magnitude leave the site as (index, value) pairs in ascending index
// order, the rest stay in err; every site then sums the gathered pairs into the dense gradient.
// All of it is integer selection logic on key(i) = bits(acc[i]) & 0x7fffffff (NaN > inf >
// finite, +-0 tie, the lower index wins a tie), so ops.reference.topk_select / topk_combine
// give the same bits.
//
//   tk_pass<0..3>   radix select of the k-th largest key, 8 bits per pass from the top: an LDS
//                   histogram of the digit over the keys that still match the prefix, then one
//                   integer atomic per non-empty bin and workgroup.  Pass 0 forms acc = g + err
//                   and leaves it in err.  Pass p > 0 first resolves pass p - 1's histogram
//                   (every workgroup for itself, from the finished counts: no workgroup waits for
//                   another); workgroup 0 records the result and clears the histogram two
//                   passes back, so the scratch is all zero again after a release.
//   tk_pass<4>      resolves the last digit: threshold key T and `need`, the number of keys == T
//                   that are taken (k - need keys are > T); every workgroup counts the keys > T
//                   and == T of its contiguous index range.
//   tk_write        exclusive sums of those counts over the workgroups before it, then per tile
//                   of 1024 indices one block scan: element i goes to slot (#keys > T before i)
//                   + min(#keys == T before i, need) when key > T, or key == T with fewer than
//                   `need` equal keys before it.  idx / val ascending, err[i] = +0 where taken.
//   tk_combine      each workgroup owns 2048 consecutive indices in LDS (+0), lower-bounds every
//                   rank's sorted index list for its range and adds the ranks' values in rank
//                   order (one rank's indices are distinct: no two lanes meet), then stores the
//                   range.  No float atomics: the sum order is rank order whatever the geometry.
//
// Sizes (n, k) are launch arguments fixed when the state is built; everything that changes from
// release to release is read from device memory, so a captured graph replays on fresh gradients.
#include "common.h"

namespace {

constexpr int TK_THREADS = 256;
constexpr int TK_TILE = 1024;    // indices per workgroup and round (4 per thread)
constexpr int TK_MAXG = 1024;    // workgroups of the count / write launches at the most
// ... of a digit pass: each adds up to 256 bins to the one histogram, and those same-address
// atomics are what a pass costs (1.06 M keys: select 56 us at 1024 workgroups, 34 at 256, 33 at
// 128, 40 at 64; profiles/topk_bench.md)
constexpr int TK_MAXH = 256;
constexpr int TK_RANGE = 2048;   // indices per workgroup of the combine launch
// scratch words: hist[4][256], sel[4][2] {prefix, remaining}, cnt[TK_MAXG][2] {> T, == T}
constexpr int TK_HIST = 0, TK_SEL = 4 * 256, TK_CNT = TK_SEL + 8;
constexpr int TK_SCRATCH = TK_CNT + 2 * TK_MAXG;

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ uint32_t tk_key(uint32_t bits) { return bits & 0x7fffffffu; }

// exclusive prefix sum of v over the 256 threads (thread order) and the total; red: 4 words
__device__ __forceinline__ int tk_scan(int v, int* red, int& total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int u = __shfl_up(inc, o, 64);
    if (lane >= o) inc += u;
  }
  __syncthreads();  // (red may still be read from the previous scan)
  if (lane == 63) red[w] = inc;
  __syncthreads();
  int base = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) base += j < w ? red[j] : 0;
  total = red[0] + red[1] + red[2] + red[3];
  return base + inc - v;
}

// The digit of the k-th largest key among those counted in hist (256 bins), `rem` of them still
// to take from the top: the bin d with (#keys in bins > d) < rem <= (#keys in bins >= d).
// Returns the prefix with d at `shift` and leaves rem - (#keys in bins > d) in rem.
__device__ __forceinline__ uint32_t tk_resolve(const int* __restrict__ hist, uint32_t prefix,
                                               int shift, int& rem, int* red, int* pick) {
  const int h = hist[threadIdx.x];
  if (threadIdx.x == 0) pick[0] = 0, pick[1] = 1;  // (never kept: one bin always qualifies)
  int total;
  const int below = tk_scan(h, red, total);  // keys in bins < d
  const int above = total - below - h;       // keys in bins > d
  if (above < rem && rem <= above + h) {     // exactly one thread (total >= rem >= 1)
    pick[0] = (int)threadIdx.x;
    pick[1] = rem - above;
  }
  __syncthreads();
  rem = pick[1];
  return prefix | ((uint32_t)pick[0] << shift);
}

// four consecutive words at i0 (zeros past n; `ok` lanes are inside)
__device__ __forceinline__ u32x4 tk_load4(const uint32_t* __restrict__ p, long i0, long n) {
  if (i0 + 4 <= n) return *reinterpret_cast<const u32x4*>(p + i0);
  u32x4 v = u32x4{0u, 0u, 0u, 0u};
#pragma unroll
  for (int e = 0; e < 4; ++e)
    if (i0 + e < n) v[e] = p[i0 + e];
  return v;
}

// the state a pass starts from: what pass P - 1's histogram resolves to
template <int P>
__device__ __forceinline__ uint32_t tk_enter(int* __restrict__ scratch, int k, int& rem, int* red,
                                             int* pick) {
  uint32_t prefix = 0u;
  rem = k;
  if (P >= 2) {
    prefix = (uint32_t)scratch[TK_SEL + 2 * (P - 2)];
    rem = scratch[TK_SEL + 2 * (P - 2) + 1];
  }
  if (P >= 1) {
    prefix = tk_resolve(scratch + TK_HIST + 256 * (P - 1), prefix, 24 - 8 * (P - 1), rem, red,
                        pick);
    if (blockIdx.x == 0) {
      if (threadIdx.x == 0) {
        scratch[TK_SEL + 2 * (P - 1)] = (int)prefix;
        scratch[TK_SEL + 2 * (P - 1) + 1] = rem;
      }
      // (no launch after pass P - 1 reads the histogram of pass P - 2)
      if (P >= 2) scratch[TK_HIST + 256 * (P - 2) + threadIdx.x] = 0;
    }
  }
  return prefix;
}

template <int P>
__global__ void __launch_bounds__(TK_THREADS)
tk_pass(const float* __restrict__ g, uint32_t* __restrict__ acc, long n, int k,
        int* __restrict__ scratch, long chunk) {
  __shared__ int lh[256];
  __shared__ int red[4];
  __shared__ int pick[2];
  lh[threadIdx.x] = 0;
  int rem;
  const uint32_t prefix = tk_enter<P>(scratch, k, rem, red, pick);
  __syncthreads();
  if constexpr (P < 4) {
    const long stride = (long)gridDim.x * TK_TILE;
    for (long i0 = (long)blockIdx.x * TK_TILE + 4 * threadIdx.x; i0 < n; i0 += stride) {
      u32x4 a;
      if constexpr (P == 0) {
        const u32x4 gb = tk_load4(reinterpret_cast<const uint32_t*>(g), i0, n);
        const u32x4 eb = tk_load4(acc, i0, n);
#pragma unroll
        for (int e = 0; e < 4; ++e)
          a[e] = __float_as_uint(__uint_as_float(gb[e]) + __uint_as_float(eb[e]));
        if (i0 + 4 <= n) {
          *reinterpret_cast<u32x4*>(acc + i0) = a;
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (i0 + e < n) acc[i0 + e] = a[e];
        }
      } else {
        a = tk_load4(acc, i0, n);
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (i0 + e >= n) continue;
        const uint32_t key = tk_key(a[e]);
        if constexpr (P == 0) {
          atomicAdd(&lh[key >> 24], 1);
        } else {
          constexpr int up = 32 - 8 * P;  // bits below the resolved prefix
          if ((key >> up) == (prefix >> up)) atomicAdd(&lh[(key >> (up - 8)) & 255u], 1);
        }
      }
    }
    __syncthreads();
    const int c = lh[threadIdx.x];
    if (c) atomicAdd(&scratch[TK_HIST + 256 * P + threadIdx.x], c);
  } else {
    // T = prefix: the keys > T and == T of this workgroup's contiguous range
    const long lo = (long)blockIdx.x * chunk;
    const long hi = lo + chunk < n ? lo + chunk : n;
    int cg = 0, ce = 0;
    for (long i0 = lo + 4 * threadIdx.x; i0 < hi; i0 += TK_TILE) {
      const u32x4 a = tk_load4(acc, i0, hi);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (i0 + e >= hi) continue;
        const uint32_t key = tk_key(a[e]);
        cg += key > prefix;
        ce += key == prefix;
      }
    }
    int tg, te;
    tk_scan(cg, red, tg);
    tk_scan(ce, red, te);
    if (threadIdx.x == 0) {
      scratch[TK_CNT + 2 * blockIdx.x] = tg;
      scratch[TK_CNT + 2 * blockIdx.x + 1] = te;
    }
  }
}

__global__ void __launch_bounds__(TK_THREADS)
tk_write(uint32_t* __restrict__ acc, long n, int k, int* __restrict__ scratch, long chunk,
         uint32_t* __restrict__ idx, uint32_t* __restrict__ val, int idx_float) {
  __shared__ int red[4];
  const uint32_t T = (uint32_t)scratch[TK_SEL + 6];
  const int need = scratch[TK_SEL + 7];
  if (blockIdx.x == 0) scratch[TK_HIST + 256 * 3 + threadIdx.x] = 0;
  // keys > T and == T in the ranges before this one
  int bg = 0, be = 0;
  for (int j = 4 * threadIdx.x; j < 4 * (int)threadIdx.x + 4; ++j) {
    if (j < (int)blockIdx.x) {
      bg += scratch[TK_CNT + 2 * j];
      be += scratch[TK_CNT + 2 * j + 1];
    }
  }
  int base_g, base_e;
  tk_scan(bg, red, base_g);
  tk_scan(be, red, base_e);
  const long lo = (long)blockIdx.x * chunk;
  const long hi = lo + chunk < n ? lo + chunk : n;
  for (long t0 = lo; t0 < hi; t0 += TK_TILE) {
    const long i0 = t0 + 4 * threadIdx.x;
    const u32x4 a = tk_load4(acc, i0, hi);
    int pk = 0;  // keys > T in the low half, == T in the high half (at most 4 each)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (i0 + e >= hi) continue;
      const uint32_t key = tk_key(a[e]);
      pk += (key > T) + ((key == T) << 16);
    }
    int tot;
    const int ex = tk_scan(pk, red, tot);
    int ng = base_g + (ex & 0xffff), ne = base_e + (ex >> 16);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (i0 + e >= hi) continue;
      const uint32_t key = tk_key(a[e]);
      const bool gt = key > T, eq = key == T;
      if (gt || (eq && ne < need)) {
        const long pos = (long)ng + (ne < need ? ne : need);
        if (pos < k) {  // (always: exactly k elements qualify)
          const long i = i0 + e;
          idx[pos] = idx_float ? __float_as_uint((float)i) : (uint32_t)i;
          val[pos] = a[e];
          acc[i] = 0u;
        }
      }
      ng += gt;
      ne += eq;
    }
    base_g += tot & 0xffff;
    base_e += tot >> 16;
  }
}

__device__ __forceinline__ long tk_index(const uint32_t* __restrict__ p, int j, int idx_float) {
  return idx_float ? (long)__uint_as_float(p[j]) : (long)p[j];
}

// pairs: rank w's k indices at pairs + w * stride, its k values k words further on
__global__ void __launch_bounds__(TK_THREADS)
tk_combine(const uint32_t* __restrict__ pairs, int W, long stride, int k, int idx_float,
           float* __restrict__ out, long n) {
  __shared__ float tile[TK_RANGE];
  __shared__ int bound[2];
  const long lo = (long)blockIdx.x * TK_RANGE;
  const long hi = lo + TK_RANGE < n ? lo + TK_RANGE : n;
  for (int j = threadIdx.x; j < TK_RANGE; j += TK_THREADS) tile[j] = 0.f;
  for (int w = 0; w < W; ++w) {
    const uint32_t* ix = pairs + (long)w * stride;
    if (threadIdx.x < 2) {  // first position with index >= lo (thread 0), >= hi (thread 1)
      const long want = threadIdx.x ? hi : lo;
      int a = 0, b = k;
      while (a < b) {
        const int m = a + (b - a) / 2;
        if (tk_index(ix, m, idx_float) < want) a = m + 1; else b = m;
      }
      bound[threadIdx.x] = a;
    }
    __syncthreads();  // (also: the previous rank's adds are done)
    const int p1 = bound[1];
    for (int j = bound[0] + threadIdx.x; j < p1; j += TK_THREADS) {
      const long i = tk_index(ix, j, idx_float);
      if (i >= lo && i < hi) tile[i - lo] += __uint_as_float(ix[k + j]);
    }
    __syncthreads();
  }
  for (long i0 = lo + 4 * threadIdx.x; i0 < hi; i0 += 4 * TK_THREADS) {
    if (i0 + 4 <= hi) {
      *reinterpret_cast<f32x4*>(out + i0) = *reinterpret_cast<const f32x4*>(tile + (i0 - lo));
    } else {
      for (long i = i0; i < hi; ++i) out[i] = tile[i - lo];
    }
  }
}

long tk_chunk(long n) {
  const long per = (n + TK_MAXG - 1) / TK_MAXG;
  return (per + TK_TILE - 1) / TK_TILE * TK_TILE;
}

}  // namespace

DN_API int dn_topk_scratch_words() { return TK_SCRATCH; }

// g, err (n fp32) -> err = g + err with the k selected entries moved to send: k index words
// (int32, or fp32 values with idx_float) then k value words, ascending index.  scratch:
// dn_topk_scratch_words() int32 words, all zero before the first release (left all zero).
DN_API int dn_topk_select(const float* g, float* err, long n, int k, void* send, int idx_float,
                          void* scratch, hipStream_t st) {
  if (n <= 0 || n >= (1L << 31) || k < 1 || k > n || !g || !err || !send || !scratch)
    return DN_BAD_SHAPE;
  if (idx_float && n > (1L << 24)) return DN_BAD_SHAPE;  // indices exact in fp32
  if (((uintptr_t)g & 15) || ((uintptr_t)err & 15) || ((uintptr_t)send & 3) ||
      ((uintptr_t)scratch & 3))
    return DN_BAD_SHAPE;
  uint32_t* acc = reinterpret_cast<uint32_t*>(err);
  int* sc = reinterpret_cast<int*>(scratch);
  const long chunk = tk_chunk(n);
  const unsigned G = (unsigned)((n + chunk - 1) / chunk);  // <= TK_MAXG
  const long tiles = (n + TK_TILE - 1) / TK_TILE;
  const unsigned H = (unsigned)(tiles < TK_MAXH ? tiles : TK_MAXH);
  const dim3 blk(TK_THREADS);
  hipLaunchKernelGGL(tk_pass<0>, dim3(H), blk, 0, st, g, acc, n, k, sc, chunk);
  hipLaunchKernelGGL(tk_pass<1>, dim3(H), blk, 0, st, g, acc, n, k, sc, chunk);
  hipLaunchKernelGGL(tk_pass<2>, dim3(H), blk, 0, st, g, acc, n, k, sc, chunk);
  hipLaunchKernelGGL(tk_pass<3>, dim3(H), blk, 0, st, g, acc, n, k, sc, chunk);
  hipLaunchKernelGGL(tk_pass<4>, dim3(G), blk, 0, st, g, acc, n, k, sc, chunk);
  uint32_t* ix = reinterpret_cast<uint32_t*>(send);
  hipLaunchKernelGGL(tk_write, dim3(G), blk, 0, st, acc, n, k, sc, chunk, ix, ix + k, idx_float);
  return dn_launch_status();
}

// pairs: W ranks' send blocks, `stride` words apart -> out (n fp32, every element written):
// out[i] = ((+0 + v_0) + v_1) + ... over the ranks that hold i, in rank order
DN_API int dn_topk_combine(const void* pairs, int W, long stride, int k, int idx_float, float* out,
                           long n, hipStream_t st) {
  if (n <= 0 || n >= (1L << 31) || k < 1 || k > n || W < 1 || stride < 2L * k || !pairs || !out)
    return DN_BAD_SHAPE;
  if (((uintptr_t)pairs & 3) || ((uintptr_t)out & 15)) return DN_BAD_SHAPE;
  const long G = (n + TK_RANGE - 1) / TK_RANGE;
  hipLaunchKernelGGL(tk_combine, dim3((unsigned)G), dim3(TK_THREADS), 0, st,
                     reinterpret_cast<const uint32_t*>(pairs), W, stride, k, idx_float, out, n);
  return dn_launch_status();
}
