// Fused optimizer kernels over ONE flat fp32 parameter buffer (all of a model's tensors are views
// into it), so a whole optimizer step is a single launch regardless of the parameter count.
#include "common.h"
#include "prologue.h"
#include "sqnorm.h"

namespace {

// ---------------------------------------------------------------------------------------------
// Global-norm gradient clipping (FusedAdam max_grad_norm).  grad_sqnorm_kernel leaves CLIP_PARTS
// fp64 partial sums of g^2 (a fixed grid, so every partial is rewritten by every launch and the
// same data always gives the same bits); the Adam launch that follows sums them in the prologue of
// every updating wave -- no finalize launch, no float atomics, no "last workgroup" ticket.
constexpr int CLIP_PARTS = SQNORM_PARTS;  // (sqnorm.h: the partials and their fixed order)
struct ClipState {
  double part[CLIP_PARTS];
  float max_norm;  // threshold c (host-written; read here, so a captured graph follows it)
  float norm;      // last G = grad_scale * ||g||_2
  int skipped;     // updates skipped for a non-finite G
  int pad;
};

__global__ void __launch_bounds__(256)
grad_sqnorm_kernel(const float* __restrict__ g, long n4, ClipState* __restrict__ cs) {
  sqnorm_partial(g, n4, cs->part);
}

// Prologue of a clipped update (all 64 lanes of the wave active): the partials summed in one
// fixed order, G = grad_scale * sqrt(sum), and torch.nn.utils.clip_grad_norm_'s coefficient folded
// into the gradient scale, rounded to fp32 once.  G <= c gives grad_scale back exactly.  A
// non-finite G sets skip; workgroup 0 records G and counts the skip.
__device__ __forceinline__ float clip_coef(ClipState* __restrict__ cs, float grad_scale, bool& skip) {
  const double s = sqnorm_total(cs->part);
  const double G = (double)grad_scale * sqrt(s);
  const float Gf = (float)G;
  skip = !(fabsf(Gf) <= 3.402823466e+38f);  // inf or NaN
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    cs->norm = Gf;
    if (skip) cs->skipped += 1;
  }
  return (float)((double)grad_scale * fmin(1.0, (double)cs->max_norm / (G + 1e-6)));
}

// ---------------------------------------------------------------------------------------------
// Learning-rate schedule (FusedAdam lr_schedule).  The rate is a function of the update number t
// the bias corrections use, evaluated in the prologue of every updating wave from a small device
// block, so a captured graph follows the schedule -- and a host write to base / scale -- with no
// recapture and no extra launch.
enum LrKind { LR_CONSTANT = 0, LR_LINEAR = 1, LR_COSINE = 2 };
struct LrState {
  float base;       // host-written: the base rate (FusedAdam.lr)
  float scale;      // host-written: the plateau multiplier (FusedAdam.lr_scale)
  float lr_min;     // host-written: the rate the decay ends at
  int kind;         // host-written: LrKind
  int warmup;       // host-written: W, warmup length in updates
  int decay_steps;  // host-written: T, total schedule length (<= W: no decay yet)
  float applied;    // kernel-written: the rate the last update used
  int pad;
};

//   w(t) = t < W ? t / W : 1
//   u(t) = clamp((t - W) / (T - W), 0, 1)
//   d(t) = 1 | 1 - (1 - r) u | r + (1 - r) 0.5 (1 + cos(pi u)),   r = lr_min / base
//   lr(t) = (float)(((base * scale) * w) * d)
// in double, rounded to fp32 once (FusedAdam.lr_at is the host mirror, same order of operations).
// Constant, W = 0, scale = 1 gives base back exactly.  Workgroup 0 records the rate.
__device__ __forceinline__ float sched_lr(LrState* __restrict__ ls, int t) {
  const double base = (double)ls->base, td = (double)t;
  const int W = ls->warmup, T = ls->decay_steps, kind = ls->kind;
  const double w = t < W ? td / (double)W : 1.0;
  double d = 1.0;
  if (kind != LR_CONSTANT && T > W) {
    const double u = fmin(fmax((td - (double)W) / (double)(T - W), 0.0), 1.0);
    const double r = base > 0.0 ? (double)ls->lr_min / base : 1.0;
    d = kind == LR_LINEAR ? 1.0 - (1.0 - r) * u
                          : r + (1.0 - r) * 0.5 * (1.0 + cos(3.14159265358979323846 * u));
  }
  const float lr = (float)(((base * (double)ls->scale) * w) * d);
  if (blockIdx.x == 0 && threadIdx.x == 0) ls->applied = lr;
  return lr;
}

// ---------------------------------------------------------------------------------------------
// Exponential moving average of the parameters (FusedAdam ema_decay): e += (1 - d_t) (p - e) right
// after the update, from the registers that hold the new p -- one more fp32 stream in and out of
// the same launch.  The decay of update t (the number the bias corrections use) is
//   d_t = warmup ? min(decay, (1 + t) / (10 + t)) : decay
// in double; 1 - d_t is rounded to fp32 once (FusedAdam.ema_decay_at is the host mirror).  A
// skipped update and a priming launch neither read nor write e.  Workgroup 0 records d_t.
struct EmaState {
  float decay;    // host-written: the cap (FusedAdam.ema_decay)
  int warmup;     // host-written: the (1 + t) / (10 + t) ramp on / off
  float applied;  // kernel-written: the decay the last average used
  int pad;
};

__device__ __forceinline__ float ema_omd(EmaState* __restrict__ es, int t) {
  const double dec = (double)es->decay, td = (double)t;
  const double d = es->warmup ? fmin(dec, (1.0 + td) / (10.0 + td)) : dec;
  if (blockIdx.x == 0 && threadIdx.x == 0) es->applied = (float)d;
  return (float)(1.0 - d);
}

// torch.optim.Adam semantics (L2 weight decay, no amsgrad):
//   g += wd * p;  m = b1 m + (1-b1) g;  v = b2 v + (1-b2) g^2
//   p -= lr / bc1 * m / (sqrt(v) / sqrt(bc2) + eps)
// grad_scale folds the dSGD mean (1/world) or loss scaling into the same pass.
//
// what the element rule takes from the prologue of a launch
struct AdamCoef {
  float grad_scale, step, inv_sqrt_bc2, omd;  // step = lr / bc1, omd = 1 - d_t
};

// Prologue of every updating wave.  The update number is t = *tdev + tofs (tdev null: tofs is the
// host's step number, and bc1 / inv_sqrt_bc2 are the host's corrections).  `update` clear on
// entry is a priming launch (adam_pack_kernel): the recorded rate and decay are left alone.
// CLIP: the gradient scale comes from clip_coef (cs non-null), and its skip clears `update`.
// SCHED: lr comes from sched_lr at t (ls non-null); a skipped update still evaluates and records
// it.
// EMA: 1 - d_t of t (es non-null); a priming launch and a skipped update leave the average, and
// its recorded decay, alone.
template <bool CLIP, bool SCHED, bool EMA>
__device__ __forceinline__ AdamCoef adam_begin(float lr, float bc1, float inv_sqrt_bc2,
                                               float grad_scale, const int* __restrict__ tdev,
                                               int tofs, double b1d, double b2d,
                                               ClipState* __restrict__ cs, LrState* __restrict__ ls,
                                               EmaState* __restrict__ es, int& update) {
  const int t = tdev ? *tdev + tofs : tofs;
  if constexpr (SCHED) {
    if (update) lr = sched_lr(ls, t);
  }
  if constexpr (CLIP) {
    bool skip;
    grad_scale = clip_coef(cs, grad_scale, skip);
    if (skip) update = 0;  // p, m, v (and the average) untouched
  }
  float omd = 0.f;
  if (update) {
    if constexpr (EMA) omd = ema_omd(es, t);
    if (tdev) {  // graph-replayable forms: the step number lives on the device (adam_bump_kernel,
                 // gemm.hip group_bump); double math as on the host, so every form rounds to the
                 // same fp32 corrections
      const double td = (double)t;
      bc1 = (float)(1.0 - pow(b1d, td));
      inv_sqrt_bc2 = (float)(1.0 / sqrt(1.0 - pow(b2d, td)));
    }
  }
  return AdamCoef{grad_scale, lr / bc1, inv_sqrt_bc2, omd};
}

// The update of one element, and the average e after it from the register that holds the new p:
// the one place the rule is written, for adam_kernel's float4 loop and scalar tail and for
// adam_pack_kernel's loop, so the step forms agree bit for bit by construction.  The float4 loads
// and stores around it stay in the kernels: moved into a function of their own (by reference or
// by value), the compiler orders the two products of gr the other way round and contracts the
// other one into the sum, which moves m and v by an ulp (tests/test_adam_bits_gpu.py).
template <bool EMA>
__device__ __forceinline__ void adam_elem(float& p, float g, float& m, float& v, float& e,
                                          float grad_scale, float wd, float b1, float b2,
                                          float step, float inv_sqrt_bc2, float eps, float omd) {
  const float gr = g * grad_scale + wd * p;
  m = b1 * m + (1.f - b1) * gr;
  v = b2 * v + (1.f - b2) * gr * gr;
  p -= step * m / (sqrtf(v) * inv_sqrt_bc2 + eps);
  if constexpr (EMA) e = __builtin_fmaf(omd, p - e, e);
}

template <bool CLIP, bool SCHED, bool EMA>
__global__ void __launch_bounds__(256)
adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
            float* __restrict__ v, long n, float lr, float b1, float b2, float eps, float wd,
            float bc1, float inv_sqrt_bc2, float grad_scale, const int* __restrict__ tdev,
            double b1d, double b2d, int tofs, long long* __restrict__ cursor,
            ClipState* __restrict__ cs, LrState* __restrict__ ls, float* __restrict__ ema,
            EmaState* __restrict__ es) {
  // the device-fed batch cursor (prologue.h) advances once per update; no workgroup of this
  // launch reads it
  if (cursor && blockIdx.x == 0 && threadIdx.x == 0) *cursor += 1;
  int update = 1;
  const AdamCoef c = adam_begin<CLIP, SCHED, EMA>(lr, bc1, inv_sqrt_bc2, grad_scale, tdev, tofs, b1d,
                                                  b2d, cs, ls, es, update);
  if (!update) return;  // skipped: the step number still advances
  const long n4 = n >> 2;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
    f32x4 pp = reinterpret_cast<f32x4*>(p)[i];
    f32x4 gg = reinterpret_cast<const f32x4*>(g)[i];
    f32x4 mm = reinterpret_cast<f32x4*>(m)[i];
    f32x4 vv = reinterpret_cast<f32x4*>(v)[i];
    f32x4 ee = f32x4{0.f, 0.f, 0.f, 0.f};
    if constexpr (EMA) ee = reinterpret_cast<f32x4*>(ema)[i];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float p_ = pp[e], m_ = mm[e], v_ = vv[e], e_ = ee[e];
      adam_elem<EMA>(p_, gg[e], m_, v_, e_, c.grad_scale, wd, b1, b2, c.step, c.inv_sqrt_bc2, eps,
                     c.omd);
      pp[e] = p_, mm[e] = m_, vv[e] = v_, ee[e] = e_;
    }
    reinterpret_cast<f32x4*>(p)[i] = pp;
    reinterpret_cast<f32x4*>(m)[i] = mm;
    reinterpret_cast<f32x4*>(v)[i] = vv;
    if constexpr (EMA) reinterpret_cast<f32x4*>(ema)[i] = ee;
  }
  // scalar tail
  const long t = (n4 << 2) + blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (blockIdx.x == 0 && t < n) {
    float none = 0.f;
    adam_elem<EMA>(p[t], g[t], m[t], v[t], EMA ? ema[t] : none, c.grad_scale, wd, b1, b2, c.step,
                   c.inv_sqrt_bc2, eps, c.omd);
  }
}

// ---------------------------------------------------------------------------------------------
// Fused Adam that also emits the NEXT step's operands: every updated
// parameter element is written, rounded to bf16, straight into the packed images the step's
// kernels read (the LSTM W_ih / W_hh / W_hh^T kernel layouts, the encoder's bf16 weight copy) and
// the split LSTM bias images (b_ih, b_hh: dn_lstm_fwd bias_split); the gradient is zeroed as it is
// consumed; and the next step's batch is gathered from the HBM-resident dataset at cursor + gofs
// (prologue.h).  The step then starts at its encoder GEMM, which advances the step counter and the
// cursor (gemm.hip group_bump): this launch READS both, so it cannot advance them itself.
// update = 0: pack + gather only (priming the persistent images before the first such step).
enum PackKind { PK_NONE = 0, PK_CAST = 1, PK_WIH = 2, PK_WHH = 3, PK_BIAS = 4 };
constexpr int PACK_SEGS = 16;
struct PackSeg {
  long off;    // flat offset, multiple of 4
  int n;       // elements (reference layout)
  int kind, d; // PackKind, LSTM direction
  void* dst;   // bf16 image (CAST / WIH / WHH), fp32 image (BIAS)
  void* dst2;  // WHH: the W_hh^T image
};
struct PackPlan {
  PackSeg s[PACK_SEGS];
  int cnt;
  int I, Hd, HD;  // LSTM input size, hidden, padded hidden
};

// fragment-linear position of (row, col) in a [rows][KS*32] image (lstm.hip frag_rc inverse)
__device__ __forceinline__ int frag_index(int row, int col, int KS) {
  const int T = row >> 4, n = row & 15, ks = col >> 5, q = (col >> 3) & 3, e = col & 7;
  return ((T * KS + ks) * 64 + q * 16 + n) * 8 + e;
}

__device__ __forceinline__ void pack_store(const PackPlan& pl, const PackSeg& sg, int j, float v) {
  const int GP = 4 * pl.HD;
  switch (sg.kind) {
    case PK_CAST:
      reinterpret_cast<bf16*>(sg.dst)[j] = (bf16)v;
      break;
    case PK_WIH: {
      const int row = j / pl.I, k = j - row * pl.I;
      const int g = row / pl.Hd, u = row - g * pl.Hd;
      reinterpret_cast<bf16*>(sg.dst)[(sg.d * GP + 4 * u + g) * pl.I + k] = (bf16)v;
      break;
    }
    case PK_WHH: {
      const int row = j / pl.Hd, k = j - row * pl.Hd;
      const int g = row / pl.Hd, u = row - g * pl.Hd, m = 4 * u + g;
      const int base = sg.d * GP * pl.HD;
      int a, b;
      if (pl.HD > 192) {
        a = frag_index(m, k, pl.HD / 32);
        b = frag_index(k, m, GP / 32);
      } else {
        a = m * pl.HD + k;
        b = k * GP + m;
      }
      reinterpret_cast<bf16*>(sg.dst)[base + a] = (bf16)v;
      reinterpret_cast<bf16*>(sg.dst2)[base + b] = (bf16)v;
      break;
    }
    case PK_BIAS: {
      const int g = j / pl.Hd, u = j - g * pl.Hd;
      reinterpret_cast<float*>(sg.dst)[sg.d * GP + 4 * u + g] = v;
      break;
    }
    default: break;
  }
}

// 4 consecutive elements j0 .. j0 + 3 of one segment (j0 % 4 == 0, j0 + 3 < sg.n): one index
// decode per thread and one 8-byte store wherever the destination keeps them consecutive (the
// cast images, W_ih rows, the W_hh row image; the transposed W_hh image stays per element) --
// per element, each with its integer divisions and a 2-byte store, the packing was ~6.4 of the
// launch's 14.5 us at B = 32 (profiles/r6_adam_pack_probe.txt).  Same values as pack_store.
__device__ __forceinline__ void pack_store4(const PackPlan& pl, const PackSeg& sg, int j0,
                                            const f32x4& v) {
  const int GP = 4 * pl.HD;
  bf16x4 h;
#pragma unroll
  for (int e = 0; e < 4; ++e) h[e] = (bf16)v[e];
  const bool a8 = (((uintptr_t)sg.dst) & 7) == 0;
  switch (sg.kind) {
    case PK_CAST:
      if (a8) {
        *reinterpret_cast<bf16x4*>(reinterpret_cast<bf16*>(sg.dst) + j0) = h;
        return;
      }
      break;
    case PK_WIH:
      if (a8 && (pl.I & 3) == 0) {
        const int row = j0 / pl.I, k = j0 - row * pl.I;
        const int g = row / pl.Hd, u = row - g * pl.Hd;
        *reinterpret_cast<bf16x4*>(reinterpret_cast<bf16*>(sg.dst) +
                                   (long)(sg.d * GP + 4 * u + g) * pl.I + k) = h;
        return;
      }
      break;
    case PK_WHH:
      if (a8 && pl.HD <= 192 && (pl.Hd & 3) == 0 && (pl.HD & 3) == 0) {
        const int row = j0 / pl.Hd, k = j0 - row * pl.Hd;
        const int g = row / pl.Hd, u = row - g * pl.Hd, m = 4 * u + g;
        const int base = sg.d * GP * pl.HD;
        *reinterpret_cast<bf16x4*>(reinterpret_cast<bf16*>(sg.dst) + base + m * pl.HD + k) = h;
#pragma unroll
        for (int e = 0; e < 4; ++e)
          reinterpret_cast<bf16*>(sg.dst2)[base + (k + e) * GP + m] = h[e];
        return;
      }
      break;
    default:
      break;
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) pack_store(pl, sg, j0 + e, v[e]);
}

// ---------------------------------------------------------------------------------------------
// Split-K slab sources (FusedAdam.step_pack with the step's deferred weight-gradient launch
// armed, ops._grad.arm_slabs): the gradient of a segment is not read from g but summed here from
// the fp32 partials [splits][M][N] the grouped weight-gradient GEMM left (gemm.hip
// dn_gemm_grouped defer_reduce), operation for operation what gemm_splitk_reduce + epi_store4 /
// epi_store would have stored into g -- the reduce launch and its pass over g disappear.
//   SRC_ROWS  segment element j = (row, k) of [rows][N]: slab element (m, k), 16-B loads
//             (N % 4 == 0); splits summed four at a time, v += ((a0 + a1) + a2) + a3, then the
//             rest one by one (the reduce's vector path)
//   SRC_COL   segment element j = row of a column sum (a bias gradient as its own a^T @ ones
//             problem, one column stored): slab element (m, 0); splits summed in order (the
//             reduce's scalar path)
//   SRC_GATE  m = 4u + g of reference row g * Hd + u (the inverse of the LSTM row map, which
//             pack_store4 computes too), else m = row
// then v *= alpha and v += beta * 0: the reduce accumulated into the zero this kernel wrote one
// step earlier, and the add is kept so that a -0 sum ends as the +0 it did there.
enum SlabMode { SRC_ROWS = 1, SRC_COL = 2, SRC_GATE = 4 };
struct SlabSrc {
  const float* slab;  // null: the segment reads g
  long elems;         // fp32 elements the allocation holds from `slab` on (host check)
  int M, N, splits, mode;
  float alpha, beta;
};
struct SlabPlan {
  SlabSrc s[PACK_SEGS];  // by segment
};

// the gradient of segment elements j0 .. j0 + 3 (j0 % 4 == 0, j0 + 3 < sg.n, sg.n % 4 == 0)
__device__ __forceinline__ f32x4 slab_grad(const PackPlan& pl, const SlabSrc& sr, int j0) {
  const long mn = (long)sr.M * sr.N;
  const bool gate = (sr.mode & SRC_GATE) != 0;
  f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
  if (sr.mode & SRC_COL) {
    long at[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      int r = j0 + e;
      if (gate) {
        const int g = r / pl.Hd, u = r - g * pl.Hd;
        r = 4 * u + g;
      }
      at[e] = (long)r * sr.N;
    }
    for (int s = 0; s < sr.splits; ++s) {  // the four rows' loads of a split issue together
      const float* b = sr.slab + (long)s * mn;
      const float a0 = b[at[0]], a1 = b[at[1]], a2 = b[at[2]], a3 = b[at[3]];
      v[0] += a0;
      v[1] += a1;
      v[2] += a2;
      v[3] += a3;
    }
  } else {
    int row = j0 / sr.N;
    const int k = j0 - row * sr.N;
    if (gate) {
      const int g = row / pl.Hd, u = row - g * pl.Hd;
      row = 4 * u + g;
    }
    const float* b = sr.slab + (long)row * sr.N + k;
    int s = 0;
    for (; s + 4 <= sr.splits; s += 4) {  // four slab loads in flight per round
      const f32x4 a0 = *reinterpret_cast<const f32x4*>(b + (long)s * mn);
      const f32x4 a1 = *reinterpret_cast<const f32x4*>(b + (long)(s + 1) * mn);
      const f32x4 a2 = *reinterpret_cast<const f32x4*>(b + (long)(s + 2) * mn);
      const f32x4 a3 = *reinterpret_cast<const f32x4*>(b + (long)(s + 3) * mn);
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] += ((a0[e] + a1[e]) + a2[e]) + a3[e];
    }
    // the remainder (the headline's 3 splits are all remainder): loads issued together, added
    // one by one in split order
    const int rem = sr.splits - s;
    if (rem == 3) {
      const f32x4 a0 = *reinterpret_cast<const f32x4*>(b + (long)s * mn);
      const f32x4 a1 = *reinterpret_cast<const f32x4*>(b + (long)(s + 1) * mn);
      const f32x4 a2 = *reinterpret_cast<const f32x4*>(b + (long)(s + 2) * mn);
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = ((v[e] + a0[e]) + a1[e]) + a2[e];
    } else if (rem == 2) {
      const f32x4 a0 = *reinterpret_cast<const f32x4*>(b + (long)s * mn);
      const f32x4 a1 = *reinterpret_cast<const f32x4*>(b + (long)(s + 1) * mn);
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = (v[e] + a0[e]) + a1[e];
    } else if (rem == 1) {
      const f32x4 a0 = *reinterpret_cast<const f32x4*>(b + (long)s * mn);
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] += a0[e];
    }
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    v[e] *= sr.alpha;
    if (sr.beta != 0.f) v[e] += sr.beta * 0.f;
  }
  return v;
}

// Per-step train-metric record of a device-fed epoch (runtime.feed.DeviceFeed): the step's score
// column out[b][col] (ICA: prob[:, 1], reference comps/icalstm/__init__.py:64-65) and its loss
// land in rings indexed by the batch cursor, so an epoch of K-step graph replays yields the exact
// per-sample (score, label) pairs for the train AUC and the per-step losses for the train average
// with no host work between steps.  Slot c = (*cursor + cofs) mod n.
struct StepRecord {
  const float* out;
  long ld;
  int col, B;
  const float* loss;
  float* rs;  // [n][B] scores
  float* rl;  // [n] losses
  long n;
  const long long* cursor;
  const long long* pred;  // col < 0: the score is the predicted class (FS: hard labels)
};

__device__ __forceinline__ void record_step(const StepRecord& r, int cofs) {
  long c = (*r.cursor + cofs) % r.n;
  if (c < 0) c += r.n;
  for (int b = threadIdx.x; b < r.B; b += blockDim.x)
    r.rs[c * r.B + b] = r.col < 0 ? (float)r.pred[b] : r.out[b * r.ld + r.col];
  if (threadIdx.x == 0) r.rl[c] = *r.loss;
}

__global__ void __launch_bounds__(256) record_kernel(StepRecord r, int cofs) { record_step(r, cofs); }

// SLAB: some segments take their gradient from split-K slabs (sl; slab_grad above).  Never with
// CLIP: the norm needs the finished gradient before this launch.
template <bool CLIP, bool SCHED, bool EMA, bool SLAB = false>
__global__ void __launch_bounds__(256)
adam_pack_kernel(float* __restrict__ p, float* __restrict__ g, float* __restrict__ m,
                 float* __restrict__ v, long n, float lr, float b1, float b2, float eps, float wd,
                 float grad_scale, const int* __restrict__ tdev, double b1d, double b2d, int update,
                 int zero_grad, PackPlan pl, StepPrologue sp, int gofs, int ublocks, StepRecord rec,
                 ClipState* __restrict__ cs, LrState* __restrict__ ls, SlabPlan sl,
                 float* __restrict__ ema, EmaState* __restrict__ es) {
  // the step's train record (rec.out set): the LAST workgroup; the cursor was advanced by this
  // step's encoder GEMM, so it names the batch this step trained on
  if (rec.out && blockIdx.x == gridDim.x - 1) {
    record_step(rec, 0);
    return;
  }
  // blocks [0, ublocks) update the parameters (one float4 per thread and round), the rest gather
  // the next batch: no divergent work mix inside a wave, every load of a round issued at once
  if ((int)blockIdx.x >= ublocks) {
    const long c = (*sp.cursor + gofs) % sp.nb;
    const long ng = sp.ux + sp.ny;
    const long stride = (long)(gridDim.x - ublocks - (rec.out ? 1 : 0)) * blockDim.x;
    for (long i = (blockIdx.x - ublocks) * (long)blockDim.x + threadIdx.x; i < ng; i += stride)
      prologue_item(sp, i, c);  // sp.ug == 0: the zeroing rides in the update below
    return;
  }
  // the encoder GEMM of this step advanced *tdev (prebumped form: tofs 0); CLIP is launched with
  // update set only, and a skip clears it: images from the unchanged parameters, gradient still
  // zeroed
  const AdamCoef c = adam_begin<CLIP, SCHED, EMA>(lr, 1.f, 1.f, grad_scale, tdev, 0, b1d, b2d, cs, ls,
                                                  es, update);
  const long n4 = n >> 2, stride = (long)ublocks * blockDim.x;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n4; i += stride) {
    f32x4 pp = reinterpret_cast<f32x4*>(p)[i];
    const long e0 = i << 2;
    int s = 0;
    if constexpr (SLAB) {  // the element's segment first: it says where the gradient comes from
      while (s < pl.cnt && e0 >= pl.s[s].off + pl.s[s].n) ++s;
    }
    if (update) {
      f32x4 gg;
      if constexpr (SLAB) {
        if (s < pl.cnt && e0 >= pl.s[s].off && sl.s[s].slab)
          gg = slab_grad(pl, sl.s[s], (int)(e0 - pl.s[s].off));
        else
          gg = reinterpret_cast<const f32x4*>(g)[i];
      } else {
        gg = reinterpret_cast<const f32x4*>(g)[i];
      }
      f32x4 mm = reinterpret_cast<f32x4*>(m)[i];
      f32x4 vv = reinterpret_cast<f32x4*>(v)[i];
      f32x4 ee = f32x4{0.f, 0.f, 0.f, 0.f};
      if constexpr (EMA) ee = reinterpret_cast<f32x4*>(ema)[i];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float p_ = pp[e], m_ = mm[e], v_ = vv[e], e_ = ee[e];
        adam_elem<EMA>(p_, gg[e], m_, v_, e_, c.grad_scale, wd, b1, b2, c.step, c.inv_sqrt_bc2,
                       eps, c.omd);
        pp[e] = p_, mm[e] = m_, vv[e] = v_, ee[e] = e_;
      }
      reinterpret_cast<f32x4*>(p)[i] = pp;
      reinterpret_cast<f32x4*>(m)[i] = mm;
      reinterpret_cast<f32x4*>(v)[i] = vv;
      if constexpr (EMA) reinterpret_cast<f32x4*>(ema)[i] = ee;
    }
    if (zero_grad) reinterpret_cast<f32x4*>(g)[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    if constexpr (!SLAB) {
      while (s < pl.cnt && e0 >= pl.s[s].off + pl.s[s].n) ++s;
    }
    if (s < pl.cnt && e0 >= pl.s[s].off) {
      const PackSeg& sg = pl.s[s];
      const int j0 = (int)(e0 - sg.off);
      if (j0 + 4 <= sg.n) {
        pack_store4(pl, sg, j0, pp);
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (j0 + e < sg.n) pack_store(pl, sg, j0 + e, pp[e]);
      }
    }
  }
}

__global__ void adam_bump_kernel(int* __restrict__ tdev) { *tdev += 1; }

// plain SGD with momentum (torch.optim.SGD semantics, dampening 0, no nesterov)
__global__ void __launch_bounds__(256)
sgd_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf, long n,
           float lr, float momentum, float wd, float grad_scale, int first) {
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    float d = g[i] * grad_scale + wd * p[i];
    if (momentum != 0.f) {
      float b = first ? d : momentum * buf[i] + d;
      buf[i] = b;
      d = b;
    }
    p[i] -= lr * d;
  }
}

// out = in * scale, fp32 -> bf16 (grad payload compression for precision_bits = 16)
__global__ void cast_scale_bf16_kernel(const float* __restrict__ in, bf16* __restrict__ out, long n,
                                       float scale) {
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
    out[i] = (bf16)(in[i] * scale);
}

__global__ void cast_scale_f32_kernel(const bf16* __restrict__ in, float* __restrict__ out, long n,
                                      float scale) {
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
    out[i] = (float)in[i] * scale;
}

int grid_for(long n) {
  long b = (n + 255) / 256;
  return (int)(b < 2048 ? (b > 0 ? b : 1) : 2048);
}

}  // namespace

// The squared-norm partials of g for the clipped update that follows on the same stream.
DN_API int dn_clip_parts() { return CLIP_PARTS; }
DN_API long dn_clip_state_size() { return (long)sizeof(ClipState); }
DN_API int dn_grad_sqnorm(const float* g, long n, void* clip, hipStream_t st) {
  if (n <= 0 || n % 4 || !clip) return DN_BAD_SHAPE;
  if (((uintptr_t)g & 15) || ((uintptr_t)clip & 7)) return DN_BAD_SHAPE;
  hipLaunchKernelGGL(grad_sqnorm_kernel, dim3(CLIP_PARTS), dim3(256), 0, st, g, n / 4,
                     reinterpret_cast<ClipState*>(clip));
  return dn_launch_status();
}

DN_API long dn_lr_state_size() { return (long)sizeof(LrState); }
DN_API long dn_ema_state_size() { return (long)sizeof(EmaState); }

// The argument block of every Adam launcher (ops/optim.py _AdamArgs is the host mirror), by
// address across the C ABI; the launchers hand its fields to the kernels.
struct AdamArgs {
  float *p, *g, *m, *v;
  float* ema;  // the average (null: off; with es)
  long n;
  float lr, b1, b2, eps, wd, grad_scale;
  float bc1, inv_sqrt_bc2;  // the host's bias corrections (tdev null)
  double b1d, b2d;          // the betas as the host holds them (tdev non-null)
  int* tdev;                // device step counter, null: tofs is the host's step number
  int tofs, pad;            // this update's number is *tdev + tofs
  long long* cursor;        // adam_kernel: the device-fed batch cursor to advance (null: none)
  ClipState* cs;            // non-null: the clipped update (CLIP)
  LrState* ls;              // non-null: the scheduled rate (SCHED)
  EmaState* es;             // non-null: the average follows (EMA)
};
static_assert(sizeof(AdamArgs) == 144, "ops/optim.py _AdamArgs mirrors this layout");

// The instantiations by flag bits, 1 CLIP | 2 SCHED | 4 EMA (| 8 SLAB): the state pointers of a
// launch (null = off) pick one.  There is no CLIP with SLAB (refused on the host).
using AdamKernel = decltype(&adam_kernel<false, false, false>);
using AdamPackKernel = decltype(&adam_pack_kernel<false, false, false>);
static constexpr AdamKernel ADAM_KERNELS[8] = {
    adam_kernel<false, false, false>, adam_kernel<true, false, false>,
    adam_kernel<false, true, false>,  adam_kernel<true, true, false>,
    adam_kernel<false, false, true>,  adam_kernel<true, false, true>,
    adam_kernel<false, true, true>,   adam_kernel<true, true, true>};
static constexpr AdamPackKernel ADAM_PACK_KERNELS[16] = {
    adam_pack_kernel<false, false, false>,       adam_pack_kernel<true, false, false>,
    adam_pack_kernel<false, true, false>,        adam_pack_kernel<true, true, false>,
    adam_pack_kernel<false, false, true>,        adam_pack_kernel<true, false, true>,
    adam_pack_kernel<false, true, true>,         adam_pack_kernel<true, true, true>,
    adam_pack_kernel<false, false, false, true>, nullptr,
    adam_pack_kernel<false, true, false, true>,  nullptr,
    adam_pack_kernel<false, false, true, true>,  nullptr,
    adam_pack_kernel<false, true, true, true>,   nullptr};
static int adam_flags(const AdamArgs& a) { return (a.cs ? 1 : 0) | (a.ls ? 2 : 0) | (a.es ? 4 : 0); }

// What every Adam launch requires of its block: p, g, m, v and the average 16-byte aligned, the
// state blocks word aligned, and ema / es both null (off) or both set (the average is as long as
// p).  cs is a ClipState dn_grad_sqnorm filled for this gradient.
DN_API long dn_adam_args_size() { return (long)sizeof(AdamArgs); }
static bool adam_args_ok(const AdamArgs& a) {
  if (((uintptr_t)a.p | (uintptr_t)a.g | (uintptr_t)a.m | (uintptr_t)a.v | (uintptr_t)a.ema) & 15)
    return false;
  if (((uintptr_t)a.ls | (uintptr_t)a.es) & 3) return false;
  return !a.ema == !a.es;
}

// One adam_kernel launch.  tdev null: update number tofs and the bias corrections come from the
// host.  tdev non-null: the number is *tdev + tofs (*tdev = completed steps), so the launch is
// capturable in a HIP graph and replayed every step with the right bias corrections; `bump`: the
// one-thread launch that advances *tdev follows (tofs 1), else the caller's step prologue
// advanced it already (tofs 0).
DN_API int dn_adam(const AdamArgs* args, int bump, hipStream_t st) {
  if (!args || (bump && !args->tdev)) return DN_BAD_SHAPE;
  const AdamArgs& a = *args;
  if (a.n <= 0) return DN_OK;
  if (!adam_args_ok(a)) return DN_BAD_SHAPE;
  hipLaunchKernelGGL(ADAM_KERNELS[adam_flags(a)], dim3(grid_for(a.n / 4 + 1)), dim3(256), 0, st,
                     a.p, a.g, a.m, a.v, a.n, a.lr, a.b1, a.b2, a.eps, a.wd, a.bc1, a.inv_sqrt_bc2,
                     a.grad_scale, a.tdev, a.b1d, a.b2d, a.tofs, a.cursor, a.cs, a.ls, a.ema, a.es);
  if (bump) hipLaunchKernelGGL(adam_bump_kernel, dim3(1), dim3(1), 0, st, a.tdev);
  return dn_launch_status();
}

// adam_pack_kernel launch.  segs: host PackSeg-compatible rows {off, n, kind, d, dst, dst2} sorted
// by offset (cnt <= 16); the device-fed gather (gx ... yd) is optional (gx null: none).
DN_API long dn_pack_seg_size() { return (long)sizeof(PackSeg); }
DN_API long dn_slab_src_size() { return (long)sizeof(SlabSrc); }

// A slab source against its segment: every index slab_grad forms from a segment element stays
// inside [splits][M][N], and that lies inside what the caller says the allocation holds.
static bool slab_src_ok(const SlabSrc& r, const PackSeg& s, int Hd, int HD) {
  if (((uintptr_t)r.slab & 15) || r.M <= 0 || r.N <= 0 || r.splits < 2 || r.splits > 64) return false;
  if ((long)r.splits * r.M * r.N > r.elems || s.n % 4) return false;
  const bool gate = (r.mode & SRC_GATE) != 0;
  const int shape = r.mode & (SRC_ROWS | SRC_COL);
  if ((r.mode & ~(SRC_ROWS | SRC_COL | SRC_GATE)) || (shape != SRC_ROWS && shape != SRC_COL))
    return false;
  // gate rows: reference row g * Hd + u < 4 Hd -> slab row 4 u + g < 4 Hd <= 4 HD = M
  if (gate && (Hd <= 0 || HD < Hd || r.M != 4 * HD)) return false;
  const long rows = gate ? 4L * Hd : r.M;
  if (shape == SRC_ROWS) return r.N % 4 == 0 && s.n == rows * r.N;
  return s.n == rows;
}

static bool record_ok(const StepRecord& r) {
  return r.out && r.loss && r.rs && r.rl && r.cursor && r.n > 0 && r.B > 0 &&
         (r.col < 0 ? r.pred != nullptr : r.ld > r.col);
}

// args: the update's block (tofs 0: the step's encoder GEMM advanced *tdev; update = 0 leaves the
// average alone).  srcs: null, or cnt SlabSrc rows by segment (slab null: that segment reads g)
// -- only with an unclipped update.
DN_API int dn_adam_pack(const AdamArgs* args, int update, int zero_grad, const void* segs, int cnt,
                        int I, int Hd, int HD, const void* gx, int gx_bf16, long row_elems,
                        const long long* gy, const long long* order, long nb,
                        const long long* cursor, int B, void* xb, long long* yd, long long* sd,
                        int gofs, const void* record, const void* srcs, hipStream_t st) {
  if (!args) return DN_BAD_SHAPE;
  const AdamArgs& a = *args;
  const long n = a.n;
  if (n <= 0 || n % 4 || cnt < 0 || cnt > PACK_SEGS) return DN_BAD_SHAPE;
  if (!adam_args_ok(a)) return DN_BAD_SHAPE;
  if (a.cs && !update) return DN_BAD_SHAPE;  // the partials belong to an update's gradient
  if (srcs && (a.cs || !update)) return DN_BAD_SHAPE;
  StepRecord rec{};
  if (record && update) {
    rec = *reinterpret_cast<const StepRecord*>(record);
    if (!record_ok(rec)) return DN_BAD_SHAPE;
  }
  if (update && !a.tdev) return DN_BAD_SHAPE;
  PackPlan pl{};
  pl.cnt = cnt;
  pl.I = I;
  pl.Hd = Hd;
  pl.HD = HD;
  const PackSeg* hs = reinterpret_cast<const PackSeg*>(segs);
  for (int k = 0; k < cnt; ++k) {
    pl.s[k] = hs[k];
    const PackSeg& s = pl.s[k];
    if (s.off % 4 || s.n <= 0 || s.off + s.n > n || !s.dst) return DN_BAD_SHAPE;
    if (k && s.off < pl.s[k - 1].off + pl.s[k - 1].n) return DN_BAD_SHAPE;  // sorted, disjoint
    if ((s.kind == PK_WIH || s.kind == PK_WHH || s.kind == PK_BIAS) && (Hd <= 0 || HD < Hd || I <= 0))
      return DN_BAD_SHAPE;
    if (s.kind == PK_WHH && !s.dst2) return DN_BAD_SHAPE;
  }
  SlabPlan sl{};
  bool slabs = false;
  if (srcs) {
    const SlabSrc* hr = reinterpret_cast<const SlabSrc*>(srcs);
    for (int k = 0; k < cnt; ++k) {
      if (!hr[k].slab) continue;
      if (!slab_src_ok(hr[k], pl.s[k], Hd, HD)) return DN_BAD_SHAPE;
      sl.s[k] = hr[k];
      slabs = true;
    }
  }
  StepPrologue sp{};
  if (gx) {
    const int rc = prologue_gather(sp, gx, gx_bf16, row_elems, gy, order, nb, cursor, B, xb, yd,
                                   a.g, 0, nullptr, sd);
    if (rc != DN_OK) return rc;
  }
  // one item per thread up to 4096 workgroups per part (the chip holds ~2048 at a time; the
  // rest start as the first retire)
  auto parts = [](long items) { return (int)((items + 255) / 256 < 4096 ? (items + 255) / 256 : 4096); };
  const int ub = parts(n / 4), gb = sp.gx ? parts(sp.ux + sp.ny) : 0;
  const AdamPackKernel kernel = ADAM_PACK_KERNELS[adam_flags(a) | (slabs ? 8 : 0)];
  if (!kernel) return DN_BAD_SHAPE;  // (CLIP with SLAB: refused above already)
  hipLaunchKernelGGL(kernel,
                     dim3(ub + gb + (rec.out ? 1 : 0)), dim3(256), 0, st, a.p, a.g, a.m, a.v, n,
                     a.lr, a.b1, a.b2, a.eps, a.wd, a.grad_scale, a.tdev, a.b1d, a.b2d, update,
                     zero_grad, pl, sp, gofs, ub, rec, a.cs, a.ls, sl, a.ema, a.es);
  return dn_launch_status();
}

// the standalone record (eager steps, and steps whose update is not the packing Adam): slot
// (*cursor + cofs) mod n, cofs = -1 after an update that advanced the cursor
DN_API long dn_step_record_size() { return (long)sizeof(StepRecord); }
DN_API int dn_step_record(const void* record, int cofs, hipStream_t st) {
  if (!record) return DN_BAD_SHAPE;
  const StepRecord r = *reinterpret_cast<const StepRecord*>(record);
  if (!record_ok(r)) return DN_BAD_SHAPE;
  hipLaunchKernelGGL(record_kernel, dim3(1), dim3(256), 0, st, r, cofs);
  return dn_launch_status();
}

DN_API int dn_sgd(float* p, const float* g, float* buf, long n, float lr, float momentum, float wd,
                  float grad_scale, int first, hipStream_t st) {
  if (n <= 0) return DN_OK;
  hipLaunchKernelGGL(sgd_kernel, dim3(grid_for(n)), dim3(256), 0, st, p, g, buf, n, lr, momentum,
                     wd, grad_scale, first);
  return dn_launch_status();
}

DN_API int dn_cast_f32_bf16(const float* in, void* out, long n, float scale, hipStream_t st) {
  if (n <= 0) return DN_OK;
  hipLaunchKernelGGL(cast_scale_bf16_kernel, dim3(grid_for(n)), dim3(256), 0, st, in, (bf16*)out, n,
                     scale);
  return dn_launch_status();
}

DN_API int dn_cast_bf16_f32(const void* in, float* out, long n, float scale, hipStream_t st) {
  if (n <= 0) return DN_OK;
  hipLaunchKernelGGL(cast_scale_f32_kernel, dim3(grid_for(n)), dim3(256), 0, st, (const bf16*)in,
                     out, n, scale);
  return dn_launch_status();
}
