// Differentially private gradient release (ops.dp.DPState): the site's flat gradient clipped to
// an L2 norm c and Gaussian noise of standard deviation sigma * c added, on the device, before any
// byte of it leaves the site.  Two stream-ordered launches per release -- no atomics, no
// grid-wide wait, no "last workgroup" ticket:
//
//   dp_norm_kernel       the SQNORM_PARTS fp64 partial sums of g^2 (sqnorm.h, as the clipped Adam
//                        forms them) and the release counter t += 1;
//   dp_privatize_kernel  every wave sums the partials in the fixed order, G = sqrt(sum),
//                        coef = fp32(min(1, c / (G + 1e-6))), and g = coef * g + (sigma c) z with
//                        z from Philox4x32-10 at counter (float4 index, t_lo, t_hi, stream), key
//                        (seed_lo, seed_hi): the counter lives on the device, so a captured graph
//                        replays the release with no host work and never repeats a draw.
//
// ops.reference.dp_privatize is the fp64 host mirror (same Philox bits, same mapping).
#include "common.h"
#include "sqnorm.h"

namespace {

struct DpState {
  double part[SQNORM_PARTS];  // partial sums of g^2 (every one rewritten by every norm launch)
  float clip;                 // threshold c (host-written; read here, so captured graphs follow it)
  float sigma;                // noise multiplier (host-written, read here)
  uint32_t seed_lo, seed_hi;  // generator key
  uint32_t stream;            // generator stream word (site / fold / phase)
  uint32_t pad0;
  unsigned long long t;       // releases so far
  float norm;                 // last pre-clip norm G
  int clipped;                // releases with G > c
  int nonfinite;              // releases with a non-finite G
  int pad1;
};

__global__ void __launch_bounds__(256)
dp_norm_kernel(const float* __restrict__ g, long n4, DpState* __restrict__ ds) {
  sqnorm_partial(g, n4, ds->part);
  // the release number of the privatise launch that follows on the stream (nobody in this
  // launch reads it)
  if (blockIdx.x == 0 && threadIdx.x == 0) ds->t += 1;
}

// Philox4x32-10 (Salmon et al., SC'11), the state in named registers.
__device__ __forceinline__ void philox_round(uint32_t& c0, uint32_t& c1, uint32_t& c2, uint32_t& c3,
                                             uint32_t k0, uint32_t k1) {
  const uint32_t h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
  const uint32_t h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
  c0 = h1 ^ c1 ^ k0;
  c1 = l1;
  c2 = h0 ^ c3 ^ k1;
  c3 = l0;
}

__device__ __forceinline__ void philox4x32_10(uint32_t& c0, uint32_t& c1, uint32_t& c2, uint32_t& c3,
                                              uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    philox_round(c0, c1, c2, c3, k0, k1);
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
}

// 24-bit uniform in (0, 1]
__device__ __forceinline__ float dp_uniform(uint32_t x) {
  return (float)((x >> 8) + 1u) * 5.9604644775390625e-08f;  // 2^-24, exact
}

// Box-Muller from two independent uniforms: precise logf, exactly range-reduced sin / cos of
// 2 pi u (sinpif / cospif of 2u, exact in fp32)
__device__ __forceinline__ void dp_normal_pair(uint32_t xa, uint32_t xb, float& za, float& zb) {
  const float r = sqrtf(-2.0f * logf(dp_uniform(xa)));
  const float a = 2.0f * dp_uniform(xb);
  za = r * cospif(a);
  zb = r * sinpif(a);
}

__global__ void __launch_bounds__(256)
dp_privatize_kernel(float* __restrict__ g, long n4, DpState* __restrict__ ds) {
  const double G = sqrt(sqnorm_total(ds->part));
  const float c = ds->clip, sigma = ds->sigma;
  const float Gf = (float)G;
  const bool bad = !(fabsf(Gf) <= 3.402823466e+38f);  // inf or NaN
  const float coef = (float)fmin(1.0, (double)c / (G + 1e-6));  // G <= c: exactly 1
  const unsigned long long t = ds->t;  // (the norm launch left it: 1-based)
  const uint32_t k0 = ds->seed_lo, k1 = ds->seed_hi, sw = ds->stream;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    ds->norm = Gf;
    if (bad) ds->nonfinite += 1;
    else if (G > (double)c) ds->clipped += 1;
  }
  const long stride = (long)gridDim.x * blockDim.x;
  long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (bad) {  // the release carries nothing
    const float q = __builtin_nanf("");
    for (; i < n4; i += stride) reinterpret_cast<f32x4*>(g)[i] = f32x4{q, q, q, q};
    return;
  }
  if (sigma == 0.f) {  // no generator; coef == 1 gives the gradient back bit for bit
    if (coef == 1.f) return;
    for (; i < n4; i += stride) {
      f32x4 gg = reinterpret_cast<f32x4*>(g)[i];
#pragma unroll
      for (int e = 0; e < 4; ++e) gg[e] = coef * gg[e];
      reinterpret_cast<f32x4*>(g)[i] = gg;
    }
    return;
  }
  const float sc = sigma * c;
  const uint32_t tl = (uint32_t)t, th = (uint32_t)(t >> 32);
  for (; i < n4; i += stride) {
    f32x4 gg = reinterpret_cast<f32x4*>(g)[i];
    uint32_t x0 = (uint32_t)i, x1 = tl, x2 = th, x3 = sw;
    philox4x32_10(x0, x1, x2, x3, k0, k1);
    float z0, z1, z2, z3;
    dp_normal_pair(x0, x1, z0, z1);
    dp_normal_pair(x2, x3, z2, z3);
    gg[0] = coef * gg[0] + sc * z0;
    gg[1] = coef * gg[1] + sc * z1;
    gg[2] = coef * gg[2] + sc * z2;
    gg[3] = coef * gg[3] + sc * z3;
    reinterpret_cast<f32x4*>(g)[i] = gg;
  }
}

// one float4 per thread and round, at most one workgroup per CU's worth of rounds
int dp_grid(long n4) {
  const long b = (n4 + 255) / 256;
  return (int)(b < SQNORM_PARTS ? (b > 0 ? b : 1) : SQNORM_PARTS);
}

int dp_check(const float* g, long n, const void* state) {
  // the float4 index is a 32-bit counter word
  if (n <= 0 || n % 4 || n / 4 > 0xFFFFFFFFL || !g || !state) return DN_BAD_SHAPE;
  if (((uintptr_t)g & 15) || ((uintptr_t)state & 7)) return DN_BAD_SHAPE;
  return DN_OK;
}

}  // namespace

DN_API long dn_dp_state_size() { return (long)sizeof(DpState); }
DN_API int dn_dp_parts() { return SQNORM_PARTS; }

// the norm launch alone: partials of g^2 into the state, release counter advanced
DN_API int dn_dp_norm(const float* g, long n, void* state, hipStream_t st) {
  const int rc = dp_check(g, n, state);
  if (rc != DN_OK) return rc;
  hipLaunchKernelGGL(dp_norm_kernel, dim3(SQNORM_PARTS), dim3(256), 0, st, g, n / 4,
                     reinterpret_cast<DpState*>(state));
  return dn_launch_status();
}

// the privatise launch alone (the state's partials and counter are those of a norm launch on g)
DN_API int dn_dp_apply(float* g, long n, void* state, hipStream_t st) {
  const int rc = dp_check(g, n, state);
  if (rc != DN_OK) return rc;
  hipLaunchKernelGGL(dp_privatize_kernel, dim3(dp_grid(n / 4)), dim3(256), 0, st, g, n / 4,
                     reinterpret_cast<DpState*>(state));
  return dn_launch_status();
}

// one release of g in place: both launches, stream-ordered
DN_API int dn_dp_privatize(float* g, long n, void* state, hipStream_t st) {
  const int rc = dn_dp_norm(g, n, state, st);
  return rc != DN_OK ? rc : dn_dp_apply(g, n, state, st);
}
