// Per-utterance forms of the adaptive sampler's device passes (Engine::ode_sample_each): every utterance of a batch, uniform or
// ragged, is integrated with its own step size, stage times and accept / reject decisions, while each network evaluation is still
// one launch sequence over the whole batch.  Grid (blocks, B): blockIdx.y is the utterance, blockIdx.x the workgroup INSIDE it, and
// the bodies of kernels_ode.h run over the utterance's own range of elements -- the same arithmetic, element order and summation
// order as the batch-wide kernels launched for that utterance alone, so its result does not depend on the rest of the batch.
//
// Scalar table: [B][ODE_ROWS][ODE_STRIDE] doubles, utterance b's rows 0..6 as in kernels_ode.h (its own h), and row 7 the
// utterance's state of this round:
//   [0] selector s (0 or 1): the accepted state is xbuf[s], an attempt's end point goes to xbuf[1 - s]; K_0 = kbuf[s], K_6 = kbuf[1 - s].
//       An accepted attempt flips s on the host ("first same as last"), a rejected one leaves it: no copy pass.
//   [1] active (1 / 0): a finished utterance is frozen -- its workgroups return at once and nothing of it is written.
// Reductions: partial [B][ODE_NBLK][ODE_NSUM], result [B][ODE_NSUM] (entries of frozen utterances are left as they are).
#pragma once
#include "kernels_ode.h"

namespace sgmse {

constexpr int ODE_ROW_STATE = 7;     // table row of the selector and the active flag

struct OdeEachArgs {
  OdeArgs a;                 // pointers: batch bases (utterance b at its offset); x, k[0], k[6] are resolved from the selector
  float* xbuf[2];            // the two state buffers
  float* kbuf[2];            // the two buffers K_0 / K_6 alternate between
  const long long* rag_off;  // ragged batch: [B + 1] complex-element prefix of the packed utterances (null: `per` elements each)
  long long per;
  int kout_sel;              // slope written by this pass: 0 -> K_0, 6 -> K_6, otherwise a.kout (stage kernel; the error pass writes K_6)
  int to_new_state;          // stage kernel: xnext also goes to the utterance's xbuf[1 - s] (the attempt's end point)
  int d2;                    // init-norms kernel: 1 -> the d2 pass (K_6 - K_0), 0 -> the d0 / d1 pass (x, K_0)
};

// utterance b's view of the arguments; false: the utterance is frozen
__device__ __forceinline__ bool ode_each_resolve(const OdeEachArgs& e, int b, OdeArgs* o, const double** tab, int* sel) {
  const double* t = e.a.table + (size_t)b * ODE_ROWS * ODE_STRIDE;
  if (t[ODE_ROW_STATE * ODE_STRIDE + 1] == 0.0) return false;
  const int s = t[ODE_ROW_STATE * ODE_STRIDE] != 0.0 ? 1 : 0;
  const long long off = e.rag_off ? e.rag_off[b] : (long long)b * e.per;          // complex elements
  const long long len = e.rag_off ? e.rag_off[b + 1] - e.rag_off[b] : e.per;
  const size_t fo = (size_t)off * 2;                                              // floats
  OdeArgs a = e.a;
  a.nfl = 2 * len;
  a.x = e.xbuf[s] + fo;
  if (a.xs) a.xs += fo;
  a.y += fo; a.score += fo;
  if (a.kout) a.kout += fo;
  if (a.xnext) a.xnext += fo;
  if (a.xnew) a.xnew += fo;
#pragma unroll
  for (int j = 1; j < 6; ++j) a.k[j] += fo;
  a.k[0] = e.kbuf[s] + fo;
  a.k[6] = e.kbuf[1 - s] + fo;
  a.partial = e.a.partial + (size_t)b * ODE_NBLK * ODE_NSUM;
  a.result = e.a.result + (size_t)b * ODE_NSUM;
  *o = a; *tab = t; *sel = s;
  return true;
}

__global__ __launch_bounds__(256) void ode_stage_each_kernel(OdeEachArgs e) {
  OdeArgs a; const double* tab; int s;
  if (!ode_each_resolve(e, blockIdx.y, &a, &tab, &s)) return;
  if (!e.a.xs) a.xs = a.x;                                                         // (the first evaluation: at the state itself)
  if (e.kout_sel == 0) a.kout = const_cast<float*>(a.k[0]);
  else if (e.kout_sel == 6) a.kout = const_cast<float*>(a.k[6]);
  float* x2 = e.to_new_state ? e.xbuf[1 - s] + (a.x - e.xbuf[s]) : nullptr;
  ode_stage_body(a, tab + (size_t)(a.row >= 0 ? a.row : *a.step_ptr) * ODE_STRIDE, x2, blockIdx.x, gridDim.x);
}

__global__ __launch_bounds__(256) void ode_error_each_kernel(OdeEachArgs e) {
  OdeArgs a; const double* tab; int s;
  if (!ode_each_resolve(e, blockIdx.y, &a, &tab, &s)) return;
  a.xnew = e.xbuf[1 - s] + (a.x - e.xbuf[s]);
  a.kout = const_cast<float*>(a.k[6]);
  ode_error_body(a, tab + (size_t)(a.row >= 0 ? a.row : *a.step_ptr) * ODE_STRIDE, blockIdx.x, gridDim.x);
}

__global__ __launch_bounds__(256) void ode_init_norms_each_kernel(OdeEachArgs e) {
  OdeArgs a; const double* tab; int s;
  if (!ode_each_resolve(e, blockIdx.y, &a, &tab, &s)) return;
  if (e.d2) { a.k[1] = a.k[0]; a.k[0] = a.k[6]; }
  else a.k[1] = nullptr;
  ode_init_norms_body(a, blockIdx.x, gridDim.x);
}

// one wave per utterance (grid B)
__global__ __launch_bounds__(64) void ode_reduce_final_each_kernel(const double* table, const double* partial, double* result) {
  const int b = blockIdx.x;
  if (table[((size_t)b * ODE_ROWS + ODE_ROW_STATE) * ODE_STRIDE + 1] == 0.0) return;
  ode_reduce_final_body(partial + (size_t)b * ODE_NBLK * ODE_NSUM, result + (size_t)b * ODE_NSUM);
}

}  // namespace sgmse
