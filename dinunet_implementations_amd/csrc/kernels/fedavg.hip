// Federated averaging with local steps (ops.fedavg.FedAvgState): what a site runs around the one
// site mean of a round.  p: parameters, a: the anchor (the model every site held after the last
// round), g: the flat gradient buffer (all zero between updates), u: the server momentum.
//
//   fedavg_delta_kernel   g = (p - a) * w, and the fp64 partials of sum (p - a)^2 (unweighted):
//                         one per workgroup, every slot of the state rewritten by every launch;
//   (the site mean of g, parallel.engines)
//   fedavg_adopt_kernel   u = beta * u + g (momentum on), a = a + eta * (u or g), p = a, g = 0;
//                         its first wave sums the partials in the fixed order of sqnorm.h and
//                         leaves drift = sqrt(sum).
//
// Every fp32 operation is rounded on its own, so a numpy float32 mirror reproduces the bits:
// __fsub_rn / __fmul_rn / __fadd_rn say so, and this file is compiled with -ffp-contract=off
// (csrc/build.py FILE_FLAGS) -- the library's -ffp-contract=fast fuses a multiply and an add even
// through these intrinsics, which hipcc's math header defines as the plain operators.
// 16-byte loads and stores, a scalar tail for the n % 4 last elements, a grid-stride loop; no
// atomics, and no workgroup waits for another.
#include "common.h"
#include "sqnorm.h"

namespace {

constexpr int FEDAVG_GRID = 2048;                       // the cap of optim.hip grid_for
constexpr int FEDAVG_GROUPS = FEDAVG_GRID / SQNORM_PARTS;  // sqnorm_total sums SQNORM_PARTS slots

struct FedAvgWork {
  double part[FEDAVG_GRID];  // partial sums of (p - a)^2; slots past the grid are written 0
  double drift;              // sqrt of their sum, left by the adopt launch
};

__global__ void __launch_bounds__(256)
fedavg_delta_kernel(const float* __restrict__ p, const float* __restrict__ a,
                    float* __restrict__ g, long n, float w, FedAvgWork* __restrict__ fw) {
  const long n4 = n >> 2;
  const long stride = (long)gridDim.x * blockDim.x;
  double acc = 0.0;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n4; i += stride) {
    const f32x4 pp = reinterpret_cast<const f32x4*>(p)[i];
    const f32x4 aa = reinterpret_cast<const f32x4*>(a)[i];
    f32x4 d;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float t = __fsub_rn(pp[e], aa[e]);
      acc += (double)t * (double)t;
      d[e] = __fmul_rn(t, w);
    }
    reinterpret_cast<f32x4*>(g)[i] = d;
  }
  const long j = 4 * n4 + threadIdx.x;  // the scalar tail: at most 3 elements, workgroup 0
  if (blockIdx.x == 0 && j < n) {
    const float t = __fsub_rn(p[j], a[j]);
    acc += (double)t * (double)t;
    g[j] = __fmul_rn(t, w);
  }
  sqnorm_block_sum(acc, fw->part + blockIdx.x);
  if (threadIdx.x == 0)
    for (int s = blockIdx.x + gridDim.x; s < FEDAVG_GRID; s += gridDim.x) fw->part[s] = 0.0;
}

template <bool MOM>
__device__ __forceinline__ float adopt_one(float m, float aa, float& uu, float eta, float beta) {
  float s = m;
  if (MOM) {
    uu = __fadd_rn(__fmul_rn(beta, uu), m);
    s = uu;
  }
  return __fadd_rn(aa, __fmul_rn(eta, s));
}

template <bool MOM>
__global__ void __launch_bounds__(256)
fedavg_adopt_kernel(float* __restrict__ p, float* __restrict__ a, float* __restrict__ g,
                    float* __restrict__ u, long n, float eta, float beta,
                    FedAvgWork* __restrict__ fw) {
  if (blockIdx.x == 0 && threadIdx.x < 64) {  // one whole wave: sqnorm_total needs all 64 lanes
    double tot = 0.0;
#pragma unroll
    for (int k = 0; k < FEDAVG_GROUPS; ++k) tot += sqnorm_total(fw->part + k * SQNORM_PARTS);
    if (threadIdx.x == 0) fw->drift = sqrt(tot);
  }
  const long n4 = n >> 2;
  const long stride = (long)gridDim.x * blockDim.x;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n4; i += stride) {
    const f32x4 mm = reinterpret_cast<const f32x4*>(g)[i];
    f32x4 aa = reinterpret_cast<const f32x4*>(a)[i];
    f32x4 uu = {0.f, 0.f, 0.f, 0.f};
    if (MOM) uu = reinterpret_cast<const f32x4*>(u)[i];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float ue = uu[e];
      aa[e] = adopt_one<MOM>(mm[e], aa[e], ue, eta, beta);
      uu[e] = ue;
    }
    if (MOM) reinterpret_cast<f32x4*>(u)[i] = uu;
    reinterpret_cast<f32x4*>(a)[i] = aa;
    reinterpret_cast<f32x4*>(p)[i] = aa;
    reinterpret_cast<f32x4*>(g)[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  const long j = 4 * n4 + threadIdx.x;
  if (blockIdx.x == 0 && j < n) {
    float ue = MOM ? u[j] : 0.f;
    const float an = adopt_one<MOM>(g[j], a[j], ue, eta, beta);
    if (MOM) u[j] = ue;
    a[j] = an;
    p[j] = an;
    g[j] = 0.f;
  }
}

// one float4 per thread and round, the grid capped as optim.hip grid_for caps it
int fedavg_grid(long n4) {
  const long b = (n4 + 255) / 256;
  return (int)(b < FEDAVG_GRID ? (b > 0 ? b : 1) : FEDAVG_GRID);
}

bool misaligned(const void* q) { return ((uintptr_t)q & 15) != 0; }

}  // namespace

DN_API long dn_fedavg_work_size() { return (long)sizeof(FedAvgWork); }
DN_API int dn_fedavg_parts() { return FEDAVG_GRID; }

// g = (p - a) * w and the drift partials into work
DN_API int dn_fedavg_delta(const float* p, const float* a, float* g, long n, float w, void* work,
                           hipStream_t st) {
  if (n <= 0 || !p || !a || !g || !work) return DN_BAD_SHAPE;
  if (misaligned(p) || misaligned(a) || misaligned(g) || ((uintptr_t)work & 7)) return DN_BAD_SHAPE;
  hipLaunchKernelGGL(fedavg_delta_kernel, dim3(fedavg_grid(n / 4)), dim3(256), 0, st, p, a, g, n, w,
                     reinterpret_cast<FedAvgWork*>(work));
  return dn_launch_status();
}

// the adopt rule on the site mean in g; u null: no server momentum (beta is not read)
DN_API int dn_fedavg_adopt(float* p, float* a, float* g, float* u, long n, float eta, float beta,
                           void* work, hipStream_t st) {
  if (n <= 0 || !p || !a || !g || !work) return DN_BAD_SHAPE;
  if (misaligned(p) || misaligned(a) || misaligned(g) || (u && misaligned(u))
      || ((uintptr_t)work & 7))
    return DN_BAD_SHAPE;
  const dim3 grid(fedavg_grid(n / 4));
  FedAvgWork* fw = reinterpret_cast<FedAvgWork*>(work);
  if (u)
    hipLaunchKernelGGL(fedavg_adopt_kernel<true>, grid, dim3(256), 0, st, p, a, g, u, n, eta, beta,
                       fw);
  else
    hipLaunchKernelGGL(fedavg_adopt_kernel<false>, grid, dim3(256), 0, st, p, a, g, u, n, eta,
                       beta, fw);
  return dn_launch_status();
}
