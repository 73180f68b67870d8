// Batch boundary of a device-fed evaluation pass (runtime.evalfeed.EvalFeed).
//
// A validation / test pass walks a split RESIDENT in HBM in its stored order, batch after batch,
// inside captured HIP graphs.  Between two batches ONE launch of this kernel
//   * files the finished batch: its out[b][:C], pred[b] and scalar loss go to the pass-level
//     arrays out_all [N][C], pred_all [N], loss_b [nb] at the row / batch the device cursor names;
//   * advances the cursor (first row of the batch in the static input, batches finished);
//   * gathers the next batch -- up to `cap` rows, fewer at the end of the split -- and its labels
//     from the resident split into the static input the next forward reads.  The two
//     source / destination modes of the training prologue's gather (prologue.h): bf16 -> bf16
//     (ICA), fp32 -> fp32 unrounded (the padded FS features).
// The pass starts with a launch that has no finished batch (n_prev = 0) on a zeroed cursor.
//
// Every workgroup needs the cursor's value from BEFORE this launch, and one of them has to store
// the new one.  Each workgroup reads it and then takes a ticket (one integer atomic); the
// workgroup that draws the last ticket knows every other one has read, stores the new cursor
// and resets the ticket.  Nobody waits for anybody, so the launch needs no co-residency.
#include "common.h"

namespace {

struct EvalBoundary {
  const float* out;       // finished batch [n_prev][ld] (fp32), or null when n_prev == 0
  const long long* pred;  // [n_prev]
  const float* loss;      // its scalar loss
  float* out_all;         // [N][C]
  long long* pred_all;    // [N]
  float* loss_b;          // [nb]
  long long* cursor;      // [2]: first row of the batch in the static input, batches finished
  unsigned* ticket;       // workgroups of this launch that have read the cursor (0 between launches)
  const void* gx;         // resident split [N][f8 * 8]: bf16 (mode 1) or fp32 (mode 2)
  const long long* gy;    // [N] labels
  void* xb;               // static input [cap][f8 * 8], the element type of gx
  long long* yd;          // [cap]
  long N, nb, ld;
  int C, n_prev, cap, f8, mode;
};

__global__ void __launch_bounds__(256) eval_boundary_kernel(EvalBoundary e) {
  __shared__ long long s_cur[2];
  if (threadIdx.x == 0) {
    const long long row = __hip_atomic_load(&e.cursor[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const long long bat = __hip_atomic_load(&e.cursor[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    s_cur[0] = row;
    s_cur[1] = bat;
    __threadfence();  // both reads have returned before the ticket is taken
    const unsigned t = __hip_atomic_fetch_add(e.ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    if (t == gridDim.x - 1) {  // every workgroup has read the cursor
      e.cursor[0] = row + e.n_prev;
      e.cursor[1] = bat + (e.n_prev > 0 ? 1 : 0);
      *e.ticket = 0u;
    }
  }
  __syncthreads();
  const long row0 = (long)s_cur[0], bat = (long)s_cur[1];
  if (row0 < 0 || bat < 0) return;  // a cursor nobody zeroed: touch nothing
  const long next0 = row0 + e.n_prev;  // first row of the next batch
  long rem = e.N - next0;
  const int n_next = rem <= 0 ? 0 : (rem < e.cap ? (int)rem : e.cap);
  const long ux = (long)n_next * e.f8;          // 8-element units of the gather
  const long nout = (long)e.n_prev * e.C;
  const long total = ux + n_next + nout + e.n_prev + 1;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total;
       i += (long)gridDim.x * blockDim.x) {
    long j = i;
    if (j < ux) {
      const int b = (int)(j / e.f8), u = (int)(j - (long)b * e.f8);
      const long s = (next0 + b) * e.f8 + u;
      if (e.mode == 1) {
        reinterpret_cast<bf16x8*>(e.xb)[j] = reinterpret_cast<const bf16x8*>(e.gx)[s];
      } else {
        const f32x4* sp = reinterpret_cast<const f32x4*>(e.gx) + 2 * s;
        f32x4* dp = reinterpret_cast<f32x4*>(e.xb) + 2 * j;
        dp[0] = sp[0];
        dp[1] = sp[1];
      }
    } else if ((j -= ux) < n_next) {
      e.yd[j] = e.gy[next0 + j];
    } else if ((j -= n_next) < nout) {
      const int b = (int)(j / e.C), c = (int)(j - (long)b * e.C);
      if (row0 + b < e.N) e.out_all[(row0 + b) * e.C + c] = e.out[(long)b * e.ld + c];
    } else if ((j -= nout) < e.n_prev) {
      if (row0 + j < e.N) e.pred_all[row0 + j] = e.pred[j];
    } else if (e.n_prev > 0 && bat < e.nb) {
      e.loss_b[bat] = *e.loss;
    }
  }
}

}  // namespace

DN_API long dn_eval_boundary_size() { return (long)sizeof(EvalBoundary); }

// eb: a host EvalBoundary (copied into the launch).  A launch whose cursor already stands at the
// end of the split gathers nothing; rows and batches past N / nb are never written.
DN_API int dn_eval_boundary(const void* eb, hipStream_t st) {
  if (!eb) return DN_BAD_SHAPE;
  const EvalBoundary e = *reinterpret_cast<const EvalBoundary*>(eb);
  if (!e.out_all || !e.pred_all || !e.loss_b || !e.cursor || !e.ticket || !e.gx || !e.gy ||
      !e.xb || !e.yd)
    return DN_BAD_SHAPE;
  if (e.N <= 0 || e.nb <= 0 || e.C <= 0 || e.cap <= 0 || e.f8 <= 0 || e.n_prev < 0 ||
      e.n_prev > e.cap || (e.mode != 1 && e.mode != 2))
    return DN_BAD_SHAPE;
  if (e.n_prev > 0 && (!e.out || !e.pred || !e.loss || e.ld < e.C)) return DN_BAD_SHAPE;
  if (((uintptr_t)e.gx | (uintptr_t)e.xb) & 15) return DN_BAD_SHAPE;
  if (((uintptr_t)e.cursor | (uintptr_t)e.gy | (uintptr_t)e.yd | (uintptr_t)e.pred_all) & 7)
    return DN_BAD_SHAPE;
  if ((long)e.cap * e.f8 >= (1L << 31) || (long)e.cap * e.C >= (1L << 31)) return DN_BAD_SHAPE;
  const long items = (long)e.cap * e.f8 + e.cap + (long)e.n_prev * e.C + e.n_prev + 1;
  const long blocks = (items + 255) / 256;
  hipLaunchKernelGGL(eval_boundary_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)),
                     dim3(256), 0, st, e);
  return dn_launch_status();
}
