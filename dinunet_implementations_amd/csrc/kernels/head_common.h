// Helpers shared by the fused MLP-head kernels (mlp_head.hip: batch <= 64, head_big.hip:
// any batch): dropout hash, LDS transpose fragment reads, column sums of MFMA accumulators.
#pragma once
#include "common.h"

namespace {

typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) s16x4 lds_s16x4;

__host__ __device__ constexpr int rup32(int v) { return (v + 31) & ~31; }

// 32-bit counter hash (Wellons' lowbias32 finaliser over idx ^ key(seed, layer)): two 32-bit
// multiplies per hash.  The former 64-bit splitmix finaliser (six 64-bit multiplies, each a
// chain of quarter-rate 32-bit ones) made the layer-0 dropout the longest phase of the forward.
__device__ __forceinline__ uint32_t hmix(uint64_t seed, uint32_t layer, uint32_t idx) {
  const uint32_t key = (uint32_t)seed * 0x9E3779B9u ^ (uint32_t)(seed >> 32) * 0x85EBCA6Bu ^
                       (layer + 1u) * 0xC2B2AE35u;
  uint32_t x = idx ^ key;
  x ^= x >> 16;
  x *= 0x7FEB352Du;
  x ^= x >> 15;
  x *= 0x846CA68Bu;
  x ^= x >> 16;
  return x;
}

// Keep decision of element (m, k) of a [.][K] activation: one hash serves the element PAIR
// idx / 2 (16 uniform bits each: low half for even idx, high half for odd), so a lane holding
// consecutive elements (every kernel's vector loads) hashes once per two -- the quarter-rate
// multiplies of the layer-0 input dropout were ~2 us of the replicated head's prologue.  Keep
// probabilities resolve to 2^-16.
__device__ __forceinline__ bool hkeep(uint64_t seed, int layer, int m, int k, int K, float p) {
  const uint32_t idx = (uint32_t)(m * K + k);
  const uint32_t h = hmix(seed, (uint32_t)layer, idx >> 1);
  const uint32_t u = (idx & 1u) ? (h >> 16) : (h & 0xffffu);
  return (float)u * (1.f / 65536.f) >= p;
}

// sum over the four lanes holding one accumulator column (l, l^16, l^32, l^48)
__device__ __forceinline__ float colsum4(float v) {
  v += __shfl_xor(v, 16);
  v += __shfl_xor(v, 32);
  return v;
}

// ---- LayerNorm (norm mode 3) arithmetic shared by mlp_head.hip and head_rep.hip -----------------
// Both kernels reduce in ONE order with pinned roundings (explicit fma / unfused multiplies), so
// the one-launch and the three-launch heads agree bitwise:
//  * along a row: per 16-column tile a butterfly over the tile's 16 lanes (lane & 15 = column in
//    the tile, the MFMA accumulator layout), then the tiles added in tile order;
//  * down a column: rows 16 mt + 4 q + r, each q's rows added in (mt, r) order, then
//    (q0 + q1) + (q2 + q3) (= a per-lane register sum followed by colsum4).
// a * b rounded to fp32 on its own.  The kernels are built with -ffp-contract=fast, which fuses a
// multiply into a neighbouring add wherever the backend likes (and ignores contract pragmas), so
// the product is taken by an instruction the optimiser cannot look into.
__device__ __forceinline__ float mul_rn(float a, float b) {
  float r;
  asm("v_mul_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}

__device__ __forceinline__ float tile16_sum(float v) {
  v += __shfl_xor(v, 1);
  v += __shfl_xor(v, 2);
  v += __shfl_xor(v, 4);
  v += __shfl_xor(v, 8);
  return v;
}

// s + the four tile sums of one 64-column chunk (lane -> column of the chunk), in tile order
__device__ __forceinline__ float ln_add_tiles(float s, float t) {
  t = tile16_sum(t);
#pragma unroll
  for (int g = 0; g < 4; ++g) s += __shfl(t, 16 * g);
  return s;
}

__device__ __forceinline__ float ln_xhat(float z, float mean, float rstd) {
  return mul_rn(z - mean, rstd);
}

__device__ __forceinline__ float ln_y(float gamma, float xhat, float beta) {
  return __builtin_fmaf(gamma, xhat, beta);
}

// dz = rstd (g - mean(g) - xhat mean(g xhat)), g = dy gamma
__device__ __forceinline__ float ln_dz(float rstd, float g, float m1, float xhat, float m2) {
  return mul_rn(rstd, __builtin_fmaf(-xhat, m2, g - m1));
}

// Fragment with lane i <- column c0 + (i & 15) and element j <- row k0 + 8 * (i >> 4) + j of a
// row-major LDS image (row stride S elements): two hardware-transposed 4x16 reads.
__device__ __forceinline__ bf16x8 tr_frag(const bf16* img, int S, int c0, int k0, int lane) {
  const int g = lane >> 4, i = lane & 15, q = i >> 2, p = i & 3;
  const bf16* a0 = img + (k0 + 8 * g + q) * S + c0 + 4 * p;
  const s16x4 x0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(a0));
  const s16x4 x1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(a0 + 4 * S));
  return __builtin_bit_cast(bf16x8, __builtin_shufflevector(x0, x1, 0, 1, 2, 3, 4, 5, 6, 7));
}

}  // namespace
// Any-batch head (head_big.hip): same arguments and workspace contract as dn_head_layout /
// dn_head_fwd / dn_head_bwd, which forward here for batches above the single-workgroup kernels.
int headb_layout(int nl, const int* dims, const int* flags, int B, long* out);
int headb_fwd(int nl, const int* dims, const int* flags, const float* drops, const float* bnp,
              void* const* ptrs, const float* x, long ldx, int B, const long long* y, float* out,
              float* loss, long long* pred, unsigned long long* rng, void* ws, int train,
              int log_out, const float* lossp, hipStream_t st);
int headb_bwd(int nl, const int* dims, const int* flags, const float* drops, const float* bnp,
              void* const* ptrs, int B, void* ws, const float* dloss, float* dx, long lddx,
              int lw, hipStream_t st);
