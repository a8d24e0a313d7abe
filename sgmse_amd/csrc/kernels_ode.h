// Device side of the adaptive probability-flow sampler (Engine::ode_run): Dormand-Prince 5(4) with scipy's step control
// (scipy/integrate/_ivp/rk.py RK45, common.py select_initial_step) over the OUVE probability-flow drift
//   f(x, t) = theta (y - x) - 1/2 g(t)^2 score(x, y, t)            (sdes.py: rsde.sde(...)[0] with probability_flow=True).
// The state, the seven stage slopes K_0..K_6 and the error estimate stay on the device as complex64; every pass below is
// element-wise over the 2n floats of the n complex elements (real and imaginary parts follow the same arithmetic, only the error
// norm looks at complex magnitudes), 16 bytes per access in the stage and error passes that run for every evaluation (the
// initial-step norms, twice per call, read one complex element, 8 bytes, per access).
//
// The batch is integrated as G controller GROUPS, each a contiguous range of elements with its own step size, stage times, error
// norm and accept / reject decisions, while each network evaluation is still one launch sequence over the whole batch: G = 1, the
// whole rectangular batch under one error norm as scipy sees the flattened state, or G = B, one group per utterance of a uniform or
// ragged batch.  Grid (blocks, G): blockIdx.y is the group, blockIdx.x the workgroup INSIDE it, and the bodies run over the group's
// own range -- arithmetic, element order and summation order depend on the group alone, so an utterance's result does not depend on
// the rest of its batch and equals the G = 1 run on it alone.
//
// Scalar table: [G][ODE_ROWS][ODE_STRIDE] doubles written by the host for one attempted step of every group (the group's own h); the
// row is the device step counter the network reads its time-embedding row by.
//   row e (0..5) = evaluation e of the attempt (scipy's stage e + 1):  [0] = g(t_e)^2 / 2,
//                  e < 4: [1 + j] = h A[e+2][j], j <= e+1    (input of the next stage)
//                  e = 4: [1 + j] = h B[j], j <= 5           (the step's end point y_new)
//                  e = 5: [1 + j] = h E[j], j <= 6           (error estimate)
//   row 6: [1] = h A[1][0]: the first stage's input, formed before the attempt's first evaluation (OdeArgs::row = 6)
//   row 7 (ODE_ROW_STATE): the group's state of this round
//     [0] selector s (0 or 1): the accepted state is xbuf[s], an attempt's end point goes to xbuf[1 - s]; K_0 = kbuf[s], K_6 = kbuf[1 - s].
//         An accepted attempt flips s on the host ("first same as last"), a rejected one leaves it: no copy pass.
//     [1] active (1 / 0): a finished group is frozen -- its workgroups return at once and nothing of it is written.
// Reductions: partial [G][ODE_NBLK][ODE_NSUM], result [G][ODE_NSUM] (entries of frozen groups are left as they are).
// Sums of products of the fp32 slopes are formed in double and rounded once, as scipy forms them in complex128.
#pragma once
#include <sgmse_devrt.h>
#include "kernels_norm_fir.h"

namespace sgmse {

constexpr int ODE_STRIDE = 8;        // doubles per table row
constexpr int ODE_ROWS = 8;          // rows of a group's table
constexpr int ODE_ROW_STATE = 7;     // table row of the selector and the active flag
constexpr int ODE_NBLK = 256;        // workgroups of a reduction pass: fixed, so the summation order never depends on the shape
constexpr int ODE_NSUM = 2;          // sums a reduction pass produces

// one group's view of a pass (ode_each_resolve)
struct OdeArgs {
  const float* x;          // state at the start of the step
  const float* xs;         // where the score was evaluated (the stage input)
  const float* y;
  const float* score;
  float* kout;             // K of this evaluation (null: no drift, combination only)
  const float* k[7];       // slopes entering the combination; k[self] is taken from registers
  float* xnext;            // x + sum_j c_j K_j (null: none)
  const double* table; const int* step_ptr;
  int row;                 // table row; < 0: the device step counter
  int self;                // index of the slope computed here
  int nterms;              // slopes in the combination: j < nterms
  float theta;
  long long nfl;           // floats: 2 n
  // reduction passes
  double atol, rtol;
  const float* xnew;       // error pass: the step's end point (= xs)
  double* partial;         // [ODE_NBLK][ODE_NSUM]
  double* result;          // [ODE_NSUM]
};

__device__ __forceinline__ float ode_drift1(float theta, float g2h, float y, float x, float s) { return fmaf(-g2h, s, theta * (y - x)); }

// The passes are bodies over one group's contiguous range of p.nfl floats that workgroup `blk` of `nblk` (counted inside the group)
// works on.

// Fused drift + next stage: K_self = f(xs, t_row) from the score the network just left, xnext = x + sum_j c_j K_j
// (xnext2: a second copy of xnext, or null).
__device__ __forceinline__ void ode_stage_body(const OdeArgs& p, const double* row, float* xnext2, unsigned blk, unsigned nblk) {
  const float g2h = (float)row[0];
  double c[7];
#pragma unroll
  for (int j = 0; j < 7; ++j) c[j] = j < p.nterms ? row[1 + j] : 0.0;
  const long long nq = p.nfl >> 2;
  for (long long q = (long long)blk * 256 + threadIdx.x; q < nq; q += (long long)nblk * 256) {
    float kv[4] = {0.f, 0.f, 0.f, 0.f};
    if (p.kout) {
      const float4 xs = reinterpret_cast<const float4*>(p.xs)[q], yv = reinterpret_cast<const float4*>(p.y)[q];
      const float4 sv = reinterpret_cast<const float4*>(p.score)[q];
      kv[0] = ode_drift1(p.theta, g2h, yv.x, xs.x, sv.x); kv[1] = ode_drift1(p.theta, g2h, yv.y, xs.y, sv.y);
      kv[2] = ode_drift1(p.theta, g2h, yv.z, xs.z, sv.z); kv[3] = ode_drift1(p.theta, g2h, yv.w, xs.w, sv.w);
      reinterpret_cast<float4*>(p.kout)[q] = make_float4(kv[0], kv[1], kv[2], kv[3]);
    }
    if (!p.xnext) continue;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int j = 0; j < 7; ++j) {
      if (j >= p.nterms || c[j] == 0.0) continue;       // (uniform: B[1] = 0 costs no load)
      float4 kj;
      if (p.kout && j == p.self) kj = make_float4(kv[0], kv[1], kv[2], kv[3]);
      else kj = reinterpret_cast<const float4*>(p.k[j])[q];
      acc[0] += c[j] * (double)kj.x; acc[1] += c[j] * (double)kj.y; acc[2] += c[j] * (double)kj.z; acc[3] += c[j] * (double)kj.w;
    }
    const float4 xv = reinterpret_cast<const float4*>(p.x)[q];
    const float4 xo = make_float4((float)((double)xv.x + acc[0]), (float)((double)xv.y + acc[1]),
                                  (float)((double)xv.z + acc[2]), (float)((double)xv.w + acc[3]));
    reinterpret_cast<float4*>(p.xnext)[q] = xo;
    if (xnext2) reinterpret_cast<float4*>(xnext2)[q] = xo;
  }
  // tail: one complex element when n is odd
  if ((p.nfl & 3) && blk == 0 && threadIdx.x < (unsigned)(p.nfl & 3)) {
    const long long i = (nq << 2) + threadIdx.x;
    float kv = 0.f;
    if (p.kout) { kv = ode_drift1(p.theta, g2h, p.y[i], p.xs[i], p.score[i]); p.kout[i] = kv; }
    if (p.xnext) {
      double acc = 0.0;
      for (int j = 0; j < p.nterms; ++j) if (c[j] != 0.0) acc += c[j] * (double)((p.kout && j == p.self) ? kv : p.k[j][i]);
      const float xo = (float)((double)p.x[i] + acc);
      p.xnext[i] = xo;
      if (xnext2) xnext2[i] = xo;
    }
  }
}

// block-level sum of ODE_NSUM doubles in a fixed order: butterfly inside the wave, the four waves in sequence
__device__ __forceinline__ void ode_block_sums(double s0, double s1, double* partial, unsigned blk) {
  __shared__ double s_w[4 * ODE_NSUM];
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) { s0 += drt_shfl_xor_f64(s0, m); s1 += drt_shfl_xor_f64(s1, m); }
  if ((threadIdx.x & 63) == 0) { s_w[(threadIdx.x >> 6) * ODE_NSUM] = s0; s_w[(threadIdx.x >> 6) * ODE_NSUM + 1] = s1; }
  __syncthreads();
  if (threadIdx.x == 0) {
    partial[(size_t)blk * ODE_NSUM] = (s_w[0] + s_w[2]) + (s_w[4] + s_w[6]);
    partial[(size_t)blk * ODE_NSUM + 1] = (s_w[1] + s_w[3]) + (s_w[5] + s_w[7]);
  }
}

__device__ __forceinline__ double ode_abs(double re, double im) { return sqrt(re * re + im * im); }

// Last pass of an attempted step: K_6 = f(y_new, t + h) from the score at y_new, err = sum_j (h E_j) K_j,
// scale = atol + max(|x|, |y_new|) rtol, partial sums of |err / scale|^2 over complex elements (sum 0; sum 1 = 0).
__device__ __forceinline__ void ode_error_body(const OdeArgs& p, const double* row, unsigned blk, unsigned nblk) {
  const float g2h = (float)row[0];
  double c[7];
#pragma unroll
  for (int j = 0; j < 7; ++j) c[j] = row[1 + j];
  const long long npair = p.nfl >> 2, nc = p.nfl >> 1;      // 16-byte items (two complex elements), complex elements
  double sum = 0.0;
  for (long long q = (long long)blk * 256 + threadIdx.x; q < npair; q += (long long)nblk * 256) {
    const float4 xn = reinterpret_cast<const float4*>(p.xnew)[q], yv = reinterpret_cast<const float4*>(p.y)[q];
    const float4 sv = reinterpret_cast<const float4*>(p.score)[q], xv = reinterpret_cast<const float4*>(p.x)[q];
    const float k6[4] = {ode_drift1(p.theta, g2h, yv.x, xn.x, sv.x), ode_drift1(p.theta, g2h, yv.y, xn.y, sv.y),
                         ode_drift1(p.theta, g2h, yv.z, xn.z, sv.z), ode_drift1(p.theta, g2h, yv.w, xn.w, sv.w)};
    reinterpret_cast<float4*>(p.kout)[q] = make_float4(k6[0], k6[1], k6[2], k6[3]);
    double e[4] = {c[6] * (double)k6[0], c[6] * (double)k6[1], c[6] * (double)k6[2], c[6] * (double)k6[3]};
#pragma unroll
    for (int j = 0; j < 6; ++j) {
      if (c[j] == 0.0) continue;                           // (E[1] = 0)
      const float4 kj = reinterpret_cast<const float4*>(p.k[j])[q];
      e[0] += c[j] * (double)kj.x; e[1] += c[j] * (double)kj.y; e[2] += c[j] * (double)kj.z; e[3] += c[j] * (double)kj.w;
    }
    const double sa = p.atol + fmax(ode_abs(xv.x, xv.y), ode_abs(xn.x, xn.y)) * p.rtol;
    const double sb = p.atol + fmax(ode_abs(xv.z, xv.w), ode_abs(xn.z, xn.w)) * p.rtol;
    sum += (e[0] * e[0] + e[1] * e[1]) / (sa * sa) + (e[2] * e[2] + e[3] * e[3]) / (sb * sb);
  }
  if ((nc & 1) && blk == 0 && threadIdx.x == 0) {
    const long long i = npair << 2;
    double e[2];
    for (int r = 0; r < 2; ++r) {
      const float k6 = ode_drift1(p.theta, g2h, p.y[i + r], p.xnew[i + r], p.score[i + r]);
      p.kout[i + r] = k6;
      e[r] = c[6] * (double)k6;
      for (int j = 0; j < 6; ++j) if (c[j] != 0.0) e[r] += c[j] * (double)p.k[j][i + r];
    }
    const double s = p.atol + fmax(ode_abs(p.x[i], p.x[i + 1]), ode_abs(p.xnew[i], p.xnew[i + 1])) * p.rtol;
    sum += (e[0] * e[0] + e[1] * e[1]) / (s * s);
  }
  ode_block_sums(sum, 0.0, p.partial, blk);
}

// The norms of the initial-step rule with scale = atol + |x| rtol:
//   sum 0 = sum |x / scale|^2 (d0; skipped when k[1] is given),  sum 1 = sum |(k[0] - k[1]) / scale|^2  (d1: k[1] null; d2: k[1] = K_0)
__device__ __forceinline__ void ode_init_norms_body(const OdeArgs& p, unsigned blk, unsigned nblk) {
  const long long nc = p.nfl >> 1;
  const float2* x = reinterpret_cast<const float2*>(p.x);
  const float2* a = reinterpret_cast<const float2*>(p.k[0]);
  const float2* b = reinterpret_cast<const float2*>(p.k[1]);
  double s0 = 0.0, s1 = 0.0;
  for (long long i = (long long)blk * 256 + threadIdx.x; i < nc; i += (long long)nblk * 256) {
    const float2 xv = x[i], av = a[i];
    const double sc = p.atol + ode_abs(xv.x, xv.y) * p.rtol;
    double dr = av.x, di = av.y;
    if (b) { const float2 bv = b[i]; dr -= (double)bv.x; di -= (double)bv.y; }
    else s0 += ((double)xv.x * xv.x + (double)xv.y * xv.y) / (sc * sc);
    s1 += (dr * dr + di * di) / (sc * sc);
  }
  ode_block_sums(s0, s1, p.partial, blk);
}

// second stage of every reduction: one wave adds the ODE_NBLK partial sums in a fixed order
__device__ __forceinline__ void ode_reduce_final_body(const double* partial, double* result) {
  double s0 = 0.0, s1 = 0.0;
  for (int k = threadIdx.x; k < ODE_NBLK; k += 64) { s0 += partial[(size_t)k * ODE_NSUM]; s1 += partial[(size_t)k * ODE_NSUM + 1]; }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) { s0 += drt_shfl_xor_f64(s0, m); s1 += drt_shfl_xor_f64(s1, m); }
  if (threadIdx.x == 0) { result[0] = s0; result[1] = s1; }
}

// ---- the launches: grid (blocks, G)

struct OdeEachArgs {
  OdeArgs a;                 // pointers: batch bases (group g at its offset); x, k[0], k[6] are resolved from the selector
  float* xbuf[2];            // the two state buffers
  float* kbuf[2];            // the two buffers K_0 / K_6 alternate between
  const long long* rag_off;  // ragged batch: [G + 1] complex-element prefix of the packed utterances (null: `per` elements per group)
  long long per;
  int kout_sel;              // slope written by this pass: 0 -> K_0, 6 -> K_6, otherwise a.kout (stage kernel; the error pass writes K_6)
  int to_new_state;          // stage kernel: xnext also goes to the group's xbuf[1 - s] (the attempt's end point)
  int d2;                    // init-norms kernel: 1 -> the d2 pass (K_6 - K_0), 0 -> the d0 / d1 pass (x, K_0)
};

// group b's view of the arguments; false: the group is frozen
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

// one wave per group (grid G)
__global__ __launch_bounds__(64) void ode_reduce_final_each_kernel(const double* table, const double* partial, double* result) {
  const int b = blockIdx.x;
  if (table[((size_t)b * ODE_ROWS + ODE_ROW_STATE) * ODE_STRIDE + 1] == 0.0) return;
  ode_reduce_final_body(partial + (size_t)b * ODE_NBLK * ODE_NSUM, result + (size_t)b * ODE_NSUM);
}

}  // namespace sgmse
