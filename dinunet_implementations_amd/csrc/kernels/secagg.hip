// Secure aggregation (ops.secagg.SecAggState): the site's flat gradient as a pairwise-masked
// fixed-point image, so that the sum over the parties is exact and no party sees another's
// gradient.  Three stream-ordered launches per release -- no atomics, no grid-wide wait:
//
//   sa_mask_kernel  one thread per ChaCha20 block (8 elements): two float4 loads, q =
//                   int64(rint(clamp(g, +-2^18) * 2^40)), then for every peer j the 20-round block
//                   function at (key k_j, block b, release t + 1, domain word) with the 16-word
//                   state in registers; the 8 uint64 masks are added (j > rank) or subtracted
//                   (j < rank) mod 2^64 and the 64 bytes leave in four 16-byte stores.  Every
//                   workgroup leaves its {saturated, non-finite} counts in the state block;
//   sa_tail_kernel  one wave sums those partials in the fixed order and writes the masked tail
//                   block [non-finite 0/1, saturated, 0 x 6] at word n (ChaCha block ceil(n/8));
//   sa_open_kernel  after the exchange: mean = fp32(double(int64(sum)) * c), all NaN when the
//                   summed non-finite word is not 0; the counts; t += 1.
//
// Everything mutable (t, the keys, the domain word, c) is read from the device block, so a
// captured graph replays releases with fresh masks and no host work.  Keys are read at a
// wave-uniform index (scalar loads); every store is a vector store.
//
// ops.reference.secagg_mask / secagg_open are the host mirror (same bits).
#include "common.h"

namespace {

constexpr int SA_MAXW = 16;
constexpr int SA_PARTS = 1024;  // workgroups of the mask launch at the most (four per CU)
constexpr int SA_TAIL = 8;

struct SaState {
  int W, rank;
  uint32_t domain;              // ChaCha state word 15: fold * 4096 + phase * 2048
  uint32_t pad0;
  unsigned long long t;         // releases opened so far (the next mask is release t + 1)
  long long saturated;          // clamped elements, all parties, all releases
  long long nonfinite;          // releases with a non-finite element at any party
  long long last_saturated;     // clamped elements of the last release, all parties
  double c;                     // 2^-40 / W (host-written)
  uint32_t key[SA_MAXW][8];     // k_{rank, j} (row `rank` unused)
  int part[SA_PARTS][2];        // per-workgroup {saturated, non-finite} of the mask launch
};

typedef unsigned long long u64;
typedef u64 u64x2 __attribute__((ext_vector_type(2)));

#define SA_QR(a, b, c, d)                                \
  a += b; d ^= a; d = __builtin_rotateleft32(d, 16);     \
  c += d; b ^= c; b = __builtin_rotateleft32(b, 12);     \
  a += b; d ^= a; d = __builtin_rotateleft32(d, 8);      \
  c += d; b ^= c; b = __builtin_rotateleft32(b, 7);

// acc[0..8) +-= the 8 masks of ChaCha block `blk` under key k (neg: all ones to subtract)
__device__ __forceinline__ void sa_block(const uint32_t (&k)[8], uint32_t blk, uint32_t tl,
                                         uint32_t th, uint32_t dom, u64 neg, u64 (&acc)[8]) {
  uint32_t x0 = 0x61707865u, x1 = 0x3320646eu, x2 = 0x79622d32u, x3 = 0x6b206574u;
  uint32_t x4 = k[0], x5 = k[1], x6 = k[2], x7 = k[3], x8 = k[4], x9 = k[5], x10 = k[6],
           x11 = k[7];
  uint32_t x12 = blk, x13 = tl, x14 = th, x15 = dom;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    SA_QR(x0, x4, x8, x12) SA_QR(x1, x5, x9, x13) SA_QR(x2, x6, x10, x14) SA_QR(x3, x7, x11, x15)
    SA_QR(x0, x5, x10, x15) SA_QR(x1, x6, x11, x12) SA_QR(x2, x7, x8, x13) SA_QR(x3, x4, x9, x14)
  }
  x0 += 0x61707865u; x1 += 0x3320646eu; x2 += 0x79622d32u; x3 += 0x6b206574u;
  x4 += k[0]; x5 += k[1]; x6 += k[2]; x7 += k[3];
  x8 += k[4]; x9 += k[5]; x10 += k[6]; x11 += k[7];
  x12 += blk; x13 += tl; x14 += th; x15 += dom;
#define SA_ACC(m, lo, hi) acc[m] += ((((u64)(hi) << 32) | (u64)(lo)) ^ neg) - neg;
  SA_ACC(0, x0, x1) SA_ACC(1, x2, x3) SA_ACC(2, x4, x5) SA_ACC(3, x6, x7)
  SA_ACC(4, x8, x9) SA_ACC(5, x10, x11) SA_ACC(6, x12, x13) SA_ACC(7, x14, x15)
#undef SA_ACC
}

// every peer's masks of block `blk` onto acc
__device__ __forceinline__ void sa_masks(const SaState* __restrict__ ds, int W, int rank,
                                         uint32_t blk, uint32_t tl, uint32_t th, uint32_t dom,
                                         u64 (&acc)[8]) {
  for (int j = 0; j < W; ++j) {
    if (j == rank) continue;
    uint32_t k[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) k[i] = ds->key[j][i];
    sa_block(k, blk, tl, th, dom, j > rank ? 0ull : ~0ull, acc);
  }
}

// one element: clamp, count, quantise (the fp32 scaling by 2^40 and rintf are exact)
__device__ __forceinline__ u64 sa_quant(float g, int& sat, int& nf) {
  const uint32_t bits = __float_as_uint(g);
  if ((bits & 0x7f800000u) == 0x7f800000u) {  // inf or NaN: signalled through the tail block
    nf = 1;
    return 0ull;
  }
  const float lim = 262144.f;  // 2^18
  if (__builtin_fabsf(g) > lim) {
    sat += 1;
    g = __builtin_copysignf(lim, g);
  }
  return (u64)(long long)rintf(g * 1099511627776.f);  // 2^40
}

__global__ void __launch_bounds__(256)
sa_mask_kernel(const float* __restrict__ g, long n, u64* __restrict__ wire,
               const SaState* __restrict__ ds, int (*__restrict__ part)[2]) {
  __shared__ int red[2][4];
  const int W = ds->W, rank = ds->rank;
  const u64 t = ds->t + 1;  // this release (1-based)
  const uint32_t tl = (uint32_t)t, th = (uint32_t)(t >> 32), dom = ds->domain;
  const long nb = (n + 7) / 8;
  const long stride = (long)gridDim.x * blockDim.x;
  int sat = 0, nf = 0;
  for (long b = blockIdx.x * (long)blockDim.x + threadIdx.x; b < nb; b += stride) {
    const bool full = 8 * b + 8 <= n;  // else n % 8 == 4: the last block holds 4 elements
    const f32x4 lo = reinterpret_cast<const f32x4*>(g)[2 * b];
    f32x4 hi = f32x4{0.f, 0.f, 0.f, 0.f};
    if (full) hi = reinterpret_cast<const f32x4*>(g)[2 * b + 1];
    u64 acc[8];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      acc[e] = sa_quant(lo[e], sat, nf);
      acc[4 + e] = sa_quant(hi[e], sat, nf);
    }
    sa_masks(ds, W, rank, (uint32_t)b, tl, th, dom, acc);
    u64x2* out = reinterpret_cast<u64x2*>(wire + 8 * b);
    out[0] = u64x2{acc[0], acc[1]};
    out[1] = u64x2{acc[2], acc[3]};
    if (full) {
      out[2] = u64x2{acc[4], acc[5]};
      out[3] = u64x2{acc[6], acc[7]};
    }
  }
  // the workgroup's counts, summed in lane and wave order
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    sat += __shfl_xor(sat, o, 64);
    nf |= __shfl_xor(nf, o, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    red[0][threadIdx.x >> 6] = sat;
    red[1][threadIdx.x >> 6] = nf;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    part[blockIdx.x][0] = red[0][0] + red[0][1] + red[0][2] + red[0][3];
    part[blockIdx.x][1] = red[1][0] | red[1][1] | red[1][2] | red[1][3];
  }
}

// one wave: the partials of the `parts` workgroups of the mask launch in the fixed order, the
// masked tail block at word n
__global__ void __launch_bounds__(64)
sa_tail_kernel(long n, u64* __restrict__ wire, const SaState* __restrict__ ds, int parts) {
  long long sat = 0;
  int nf = 0;
  for (int p = threadIdx.x; p < parts; p += 64) {
    sat += ds->part[p][0];
    nf |= ds->part[p][1];
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    sat += __shfl_xor(sat, o, 64);
    nf |= __shfl_xor(nf, o, 64);
  }
  const u64 t = ds->t + 1;
  u64 acc[8] = {(u64)(nf != 0), (u64)sat, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull};
  sa_masks(ds, ds->W, ds->rank, (uint32_t)((n + 7) / 8), (uint32_t)t, (uint32_t)(t >> 32),
           ds->domain, acc);
  if (threadIdx.x == 0) {
    u64x2* out = reinterpret_cast<u64x2*>(wire + n);
    out[0] = u64x2{acc[0], acc[1]};
    out[1] = u64x2{acc[2], acc[3]};
    out[2] = u64x2{acc[4], acc[5]};
    out[3] = u64x2{acc[6], acc[7]};
  }
}

// the summed wire -> the fp32 mean; four elements per thread and round
__global__ void __launch_bounds__(256)
sa_open_kernel(const u64* __restrict__ sum, long n4, float* __restrict__ g,
               SaState* __restrict__ ds) {
  const long n = 4 * n4;
  const u64 bad = sum[n];  // parties with a non-finite element
  const long long sat = (long long)sum[n + 1];
  const double c = ds->c;
  const long stride = (long)gridDim.x * blockDim.x;
  long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (bad != 0ull) {  // every site alike: the release carries nothing
    const float q = __builtin_nanf("");
    for (; i < n4; i += stride) reinterpret_cast<f32x4*>(g)[i] = f32x4{q, q, q, q};
  } else {
    for (; i < n4; i += stride) {
      const u64x2 a = reinterpret_cast<const u64x2*>(sum)[2 * i];
      const u64x2 b = reinterpret_cast<const u64x2*>(sum)[2 * i + 1];
      f32x4 o;
      o[0] = (float)((double)(long long)a[0] * c);
      o[1] = (float)((double)(long long)a[1] * c);
      o[2] = (float)((double)(long long)b[0] * c);
      o[3] = (float)((double)(long long)b[1] * c);
      reinterpret_cast<f32x4*>(g)[i] = o;
    }
  }
  // (no thread of this launch reads these; the next mask launch is stream-ordered after it)
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    ds->t += 1;
    ds->last_saturated = sat;
    ds->saturated += sat;
    if (bad != 0ull) ds->nonfinite += 1;
  }
}

int sa_check(const void* g, long n, const void* wire, const void* state) {
  // the ChaCha block index (tail block included) is a 32-bit word
  if (n <= 0 || n % 4 || (n + 7) / 8 >= 0xFFFFFFFFL || !g || !wire || !state) return DN_BAD_SHAPE;
  if (((uintptr_t)g & 15) || ((uintptr_t)wire & 15) || ((uintptr_t)state & 7)) return DN_BAD_SHAPE;
  return DN_OK;
}

int sa_mask_grid(long n) {
  const long b = ((n + 7) / 8 + 255) / 256;
  return (int)(b < SA_PARTS ? (b > 0 ? b : 1) : SA_PARTS);
}

}  // namespace

DN_API long dn_secagg_state_size() { return (long)sizeof(SaState); }
DN_API int dn_secagg_parts() { return SA_PARTS; }
DN_API int dn_secagg_maxw() { return SA_MAXW; }

// g (n fp32, n % 4 == 0) -> wire (n + 8 uint64): this party's masked release t + 1
DN_API int dn_secagg_mask(const float* g, long n, void* wire, void* state, hipStream_t st) {
  const int rc = sa_check(g, n, wire, state);
  if (rc != DN_OK) return rc;
  const int grid = sa_mask_grid(n);
  SaState* ds = reinterpret_cast<SaState*>(state);
  // (the keys and the partials through pointers of their own: the launch only reads the former,
  // so they stay scalar loads)
  hipLaunchKernelGGL(sa_mask_kernel, dim3(grid), dim3(256), 0, st, g, n,
                     reinterpret_cast<u64*>(wire), (const SaState*)ds, ds->part);
  hipLaunchKernelGGL(sa_tail_kernel, dim3(1), dim3(64), 0, st, n, reinterpret_cast<u64*>(wire),
                     (const SaState*)ds, grid);
  return dn_launch_status();
}

// sum (n + 8 uint64, the parties' wires added mod 2^64) -> g (n fp32): the mean; t advanced
DN_API int dn_secagg_open(const void* sum, long n, float* g, void* state, hipStream_t st) {
  const int rc = sa_check(g, n, sum, state);
  if (rc != DN_OK) return rc;
  const long b = (n / 4 + 255) / 256;
  hipLaunchKernelGGL(sa_open_kernel, dim3((unsigned)(b < 1024 ? b : 1024)), dim3(256), 0, st,
                     reinterpret_cast<const u64*>(sum), n / 4, g,
                     reinterpret_cast<SaState*>(state));
  return dn_launch_status();
}
