// Loss heads: fused (log-)softmax + cross-entropy/NLL + argmax + input gradient, one launch.
//   ICA head (comps/icalstm/__init__.py:60-63): prob = softmax(z), loss = CE(z, y), pred = argmax
//   FS  head (comps/fs/__init__.py:54-57):      out = log_softmax(z), loss = NLL(out, y), pred
// Both share d loss / d z = (softmax(z) - onehot(y)) / B, computed in the same pass so the
// backward is a single scale.  One 256-thread workgroup; rows strided over waves, classes over
// lanes, wave64 shuffles for the row max / sum; loss reduced deterministically in LDS.
#include "common.h"
#include "loss_opt.h"

namespace {

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max_nan(v, __shfl_xor(v, o, 64));
  return v;
}
// equal for the argmax: the same value, or both NaN
__device__ __forceinline__ bool same_rank(float a, float b) { return a == b || (a != a && b != b); }
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// LW: the loss options are on (lossp: the block of loss_opt.h with C weights)
template <bool LW>
__global__ void __launch_bounds__(256)
softmax_xent_kernel(const float* __restrict__ z, const long* __restrict__ y, int B, int C,
                    int log_out, float* __restrict__ out, float* __restrict__ dz,
                    float* __restrict__ loss, long* __restrict__ pred,
                    const float* __restrict__ lossp) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  __shared__ float red[4];
  float lsum = 0.f;
  // loss options: D = sum_i w[y_i] first (rows over threads, waves merged in wave order), since
  // every dz is divided by it.  A label outside [0, C) keeps weight 1, as with the options off.
  LossOpt lo{1.f, 0.f, 0.f};
  const float* wts = LW ? lossp + DN_LOSS_W0 : nullptr;
  float D = (float)B;
  if constexpr (LW) {
    lo = lo_load(lossp);
    float d = 0.f;
    for (int r = threadIdx.x; r < B; r += 256) {
      const long lab = y[r];
      d += (lab >= 0 && lab < C) ? wts[lab] : 1.f;
    }
    d = wave_sum(d);
    if (lane == 0) red[wid] = d;
    __syncthreads();
    D = red[0] + red[1] + red[2] + red[3];
    __syncthreads();
  }
  for (int r = wid; r < B; r += 4) {
    const float* zr = z + (long)r * C;
    float mx = -INFINITY;
    for (int c = lane; c < C; c += 64) mx = max_nan(mx, zr[c]);
    mx = wave_max(mx);
    float s = 0.f;
    for (int c = lane; c < C; c += 64) s += __expf(zr[c] - mx);
    s = wave_sum(s);
    const float lse = mx + __logf(s);
    const long lab = y[r];
    // argmax as torch.argmax: the first index of the largest value, NaN the largest of all.  A
    // lane without a class keeps (-inf, INT_MAX) and loses every comparison to a lane with one.
    float bv = -INFINITY;
    int bi = 0x7fffffff;
    for (int c = lane; c < C; c += 64) {
      const float v = zr[c];
      if (argmax_takes(v, bv) || (same_rank(v, bv) && c < bi)) { bv = v; bi = c; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(bv, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      if (argmax_takes(ov, bv) || (same_rank(ov, bv) && oi < bi)) { bv = ov; bi = oi; }
    }
    if constexpr (LW) {
      const bool inr = lab >= 0 && lab < C;
      const float awy = lo_mul(lo.a, inr ? wts[lab] : 1.f);
      const float coef = awy + lo.eW;
      float S = 0.f;
      for (int c = lane; c < C; c += 64) {
        const float lp = zr[c] - lse;
        const float p = __expf(lp);
        const float wc = wts[c];
        out[(long)r * C + c] = log_out ? lp : p;
        dz[(long)r * C + c] = lo_grad(p, c == lab, awy, coef, lo_mul(lo.e, wc)) / D;
        S += lo_mul(wc, lse - zr[c]);
      }
      S = wave_sum(S);
      if (lane == 0) {
        pred[r] = bi;
        lsum += lo_row(lo, inr ? awy : 0.f, inr ? (lse - zr[lab]) : 0.f, S);
      }
      continue;
    }
    for (int c = lane; c < C; c += 64) {
      const float lp = zr[c] - lse;
      const float p = __expf(lp);
      out[(long)r * C + c] = log_out ? lp : p;
      dz[(long)r * C + c] = (p - (c == lab ? 1.f : 0.f)) / (float)B;
    }
    if (lane == 0) {
      pred[r] = bi;
      lsum += (lab >= 0 && lab < C) ? (lse - zr[lab]) : 0.f;
    }
  }
  if (lane == 0) red[wid] = lsum;
  __syncthreads();
  if (threadIdx.x == 0) *loss = (red[0] + red[1] + red[2] + red[3]) / D;
}

}  // namespace

// lossp: the loss-option block of loss_opt.h with C weights (device memory), or null for the
// plain mean cross-entropy.
DN_API int dn_softmax_xent_lw(const float* z, const long* y, int B, int C, int log_out, float* out,
                              float* dz, float* loss, long* pred, const float* lossp,
                              hipStream_t st) {
  if (B <= 0 || C <= 0) return DN_BAD_SHAPE;
  if (lossp)
    hipLaunchKernelGGL(softmax_xent_kernel<true>, dim3(1), dim3(256), 0, st, z, y, B, C, log_out,
                       out, dz, loss, pred, lossp);
  else
    hipLaunchKernelGGL(softmax_xent_kernel<false>, dim3(1), dim3(256), 0, st, z, y, B, C, log_out,
                       out, dz, loss, pred, lossp);
  return dn_launch_status();
}

DN_API int dn_softmax_xent(const float* z, const long* y, int B, int C, int log_out, float* out,
                           float* dz, float* loss, long* pred, hipStream_t st) {
  return dn_softmax_xent_lw(z, y, B, C, log_out, out, dz, loss, pred, nullptr, st);
}
