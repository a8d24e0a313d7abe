// STFT / iSTFT front-end and the spectrogram amplitude transforms.
//
// Replaces torch.stft / torch.istft as configured by reference sgmse/data_module.py:190-218 (center=True with
// reflect padding, one-sided, no normalisation, periodic Hann / sqrt-Hann window) and spec_fwd / spec_back
// (data_module.py:162-188).  n_fft = 510 = 2*3*5*17 and 1534 = 2*13*59 are not powers of two and the whole
// front-end is < 0.01 % of the run time, so both transforms are direct DFTs against an fp64-generated twiddle table
// (SURVEY Appendix C gives the exact framing / envelope rules reproduced here).
#pragma once
#include <sgmse_devrt.h>

namespace sgmse {

struct StftArgs {
  const float* sig;      // [B][L]
  const float* window;   // [n_fft]
  const float2* twiddle; // [n_fft]: (cos, sin)(2*pi*m/n_fft)
  float2* spec;          // [B][F][K], F = n_fft/2+1, K = L/hop+1
  int L, n_fft, hop, F, K;
};

constexpr int kMaxNfft = 2048;

// grid = (K, B): one workgroup per frame; thread f computes bin f.
__global__ __launch_bounds__(256) void stft_kernel(StftArgs p) {
  __shared__ float s_fr[kMaxNfft];
  __shared__ float2 s_tw[kMaxNfft];
  const int k = blockIdx.x, b = blockIdx.y, N = p.n_fft, half = N / 2;
  const float* sig = p.sig + (size_t)b * p.L;
  for (int n = threadIdx.x; n < N; n += 256) {
    int idx = k * p.hop + n - half;          // position in the un-padded signal
    if (idx < 0) idx = -idx;                 // reflect (no edge repeat)
    if (idx >= p.L) idx = 2 * (p.L - 1) - idx;
    s_fr[n] = sig[idx] * p.window[n];
    s_tw[n] = p.twiddle[n];
  }
  __syncthreads();
  for (int f = threadIdx.x; f < p.F; f += 256) {
    float re = 0.f, im = 0.f;
    int m = 0;
    for (int n = 0; n < N; ++n) {
      const float2 w = s_tw[m];
      const float v = s_fr[n];
      re = fmaf(v, w.x, re);
      im = fmaf(-v, w.y, im);
      m += f;
      if (m >= N) m -= N;
    }
    p.spec[((size_t)b * p.F + f) * p.K + k] = make_float2(re, im);
  }
}

struct IstftArgs {
  const float2* spec;    // [B][F][K]
  const float* window; const float2* twiddle;
  float* out;            // [B][length]
  int n_fft, hop, F, K, length;
};

// One thread per output sample: inverse one-sided DFT of every frame that covers it, windowed, overlap-added and
// divided by the window-square envelope (torch.istft semantics incl. center crop).  grid = (ceil(length/256), B)
__global__ __launch_bounds__(256) void istft_kernel(IstftArgs p) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= p.length) return;
  const int b = blockIdx.y, N = p.n_fft, half = N / 2;
  const int pos = j + half;                       // position in the padded (centered) signal
  const float2* spec = p.spec + (size_t)b * p.F * p.K;
  int k_hi = pos / p.hop; if (k_hi > p.K - 1) k_hi = p.K - 1;
  int k_lo = (pos - N + p.hop) / p.hop; if (pos - N + 1 <= 0) k_lo = 0;
  if (k_lo < 0) k_lo = 0;
  float acc = 0.f, env = 0.f;
  const float invN = 1.0f / (float)N;
  for (int k = k_lo; k <= k_hi; ++k) {
    const int n = pos - k * p.hop;
    if (n < 0 || n >= N) continue;
    const float w = p.window[n];
    // irfft sample n: (X0 + (-1)^n X_{N/2} + 2 sum_{f=1}^{N/2-1} Re(X_f e^{+2 pi i f n / N})) / N   (N even)
    float s = spec[(size_t)0 * p.K + k].x;
    if ((N & 1) == 0) s += ((n & 1) ? -1.f : 1.f) * spec[(size_t)half * p.K + k].x;
    float t = 0.f;
    int m = n % N;
    const int fend = (N & 1) ? half + 1 : half;   // odd N: bins 1..half all doubled
    int mm = m;
    for (int f = 1; f < fend; ++f) {
      const float2 X = spec[(size_t)f * p.K + k];
      const float2 tw = p.twiddle[mm];
      t += X.x * tw.x - X.y * tw.y;
      mm += m;
      if (mm >= N) mm -= N;
    }
    acc += (s + 2.f * t) * invN * w;
    env += w * w;
  }
  p.out[(size_t)b * p.length + j] = acc / env;
}

// spec_fwd / spec_back, transform_type in {exponent=0, log=1, none=2}; element-wise on complex data.
struct SpecXformArgs { const float2* in; float2* out; size_t n; int type; float factor, exponent; int inverse; };

// The arithmetic of one element (reference data_module.py:162-188); the stand-alone transform and the window kernels below share it.
__device__ __forceinline__ float2 spec_xform(float2 v, int type, float factor, float exponent, int inverse) {
  if (!inverse) {
    if (type == 0) {
      if (exponent != 1.f) {
        const float mag = sqrtf(v.x * v.x + v.y * v.y);
        const float g = mag > 0.f ? powf(mag, exponent) / mag : 0.f;
        v.x *= g; v.y *= g;
      }
      v.x *= factor; v.y *= factor;
    } else if (type == 1) {
      const float mag = sqrtf(v.x * v.x + v.y * v.y);
      const float g = mag > 0.f ? log1pf(mag) / mag : 0.f;
      v.x *= g * factor; v.y *= g * factor;
    }
  } else {
    if (type == 0) {
      v.x /= factor; v.y /= factor;
      if (exponent != 1.f) {
        const float mag = sqrtf(v.x * v.x + v.y * v.y);
        const float g = mag > 0.f ? powf(mag, 1.0f / exponent) / mag : 0.f;
        v.x *= g; v.y *= g;
      }
    } else if (type == 1) {
      v.x /= factor; v.y /= factor;
      const float mag = sqrtf(v.x * v.x + v.y * v.y);
      const float g = mag > 0.f ? (expf(mag) - 1.f) / mag : 0.f;
      v.x *= g; v.y *= g;
    }
  }
  return v;
}

__global__ __launch_bounds__(256) void spec_xform_kernel(SpecXformArgs p) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= p.n) return;
  p.out[i] = spec_xform(p.in[i], p.type, p.factor, p.exponent, p.inverse);
}

// Windows of a long spectrogram (sgmse_spec_split / sgmse_spec_merge).  spec is [F][K]; window j holds the frames
// [start[j], start[j] + frames[j]) as its own [F][frames[j]] block, the blocks packed one after the other: block j begins at element
// F * col0[j], col0[j] = frames[0] + ... + frames[j-1] (the layout of a ragged batch).  tab = start[n] | frames[n] | col0[n].  The host
// has checked the plan: starts and ends strictly increasing, no gap, every frame under one or two windows.  Frames are fastest in
// both layouts and an element is 8 bytes, so a wave reads and writes consecutive 8-byte words.
struct SpecWinArgs { const float2* src; float2* dst; const int* tab; int F, K, n, type; float factor, exponent; };

// grid = (ceil(max_j frames[j] / 256), F, n): thread t of window j, row f.  A gather: windows[j][f][t] = spec_fwd(spec[f][start[j] + t]).
__global__ __launch_bounds__(256) void spec_split_kernel(SpecWinArgs p) {
  const int t = blockIdx.x * 256 + threadIdx.x, f = blockIdx.y, j = blockIdx.z;
  const int Tj = p.tab[p.n + j];
  if (t >= Tj) return;
  const float2 v = p.src[(size_t)f * p.K + p.tab[j] + t];
  p.dst[(size_t)p.F * p.tab[2 * p.n + j] + (size_t)f * Tj + t] = spec_xform(v, p.type, p.factor, p.exponent, 0);
}

// grid = (ceil(K / 256), F): one thread per output element (f, k), no atomics.  j = the last window that starts at or before k covers
// k; window j - 1 covers it too when it ends behind k, and the two are cross-faded linearly over their overlap AFTER spec_back.
__global__ __launch_bounds__(256) void spec_merge_kernel(SpecWinArgs p) {
  const int k = blockIdx.x * 256 + threadIdx.x, f = blockIdx.y;
  if (k >= p.K) return;
  const int* start = p.tab; const int* frames = p.tab + p.n; const int* col0 = p.tab + 2 * p.n;
  int lo = 0, hi = p.n - 1;                  // start[0] = 0 <= k
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (start[mid] <= k) lo = mid; else hi = mid - 1;
  }
  const int j = lo, sj = start[j], Tj = frames[j];
  float2 b = spec_xform(p.src[(size_t)p.F * col0[j] + (size_t)f * Tj + (k - sj)], p.type, p.factor, p.exponent, 1);
  if (j > 0) {
    const int si = start[j - 1], Ti = frames[j - 1], ov = si + Ti - sj;      // overlap [sj, si + Ti)
    if (k < si + Ti) {
      const float2 a = spec_xform(p.src[(size_t)p.F * col0[j - 1] + (size_t)f * Ti + (k - si)], p.type, p.factor, p.exponent, 1);
      const float w = ((float)(k - sj) + 0.5f) / (float)ov;
      b.x = fmaf(w, b.x - a.x, a.x);
      b.y = fmaf(w, b.y - a.y, a.y);
    }
  }
  p.dst[(size_t)f * p.K + k] = b;
}

// Windows of ONE width W over a recording [F][K] (sgmse_window_gather / sgmse_window_blend, the windowed score of
// Engine::set_windows): window j holds the frames [start[j], start[j] + W) as block j of [n][F][W].  No transform.  The host has
// checked the plan (window_plan_error): start[0] = 0, starts strictly increasing, no gap, start[n-1] + W = K, every frame under at
// most three windows.
struct WinArgs { const float2* src; float2* dst; const int* start; int F, K, W, n; };

// grid = (ceil(W / 256), F, slots): win[j][f][t] = src[f][start[j] + t] for the `slots` table entries start[0 .. slots).  (The engine's
// table repeats the last window in the filler slots of the last chunk.)
__global__ __launch_bounds__(256) void window_gather_kernel(WinArgs p) {
  const int t = blockIdx.x * 256 + threadIdx.x, f = blockIdx.y, j = blockIdx.z;
  if (t >= p.W) return;
  p.dst[((size_t)j * p.F + f) * p.W + t] = p.src[(size_t)f * p.K + p.start[j] + t];
}

// weight of window j at its local frame t: 1 inside, rising over the overlap with window j - 1 (L_j frames), falling over the
// overlap with window j + 1
__device__ __forceinline__ float window_weight(const int* start, int n, int W, int j, int t) {
  float w = 1.0f;
  if (j > 0) w = fminf(w, ((float)t + 0.5f) / (float)(start[j - 1] + W - start[j]));
  if (j < n - 1) w = fminf(w, ((float)(W - t) - 0.5f) / (float)(start[j] + W - start[j + 1]));
  return w;
}

// grid = (ceil(K / 256), F): one thread per output element (f, k), no atomics.  The windows over frame k are j0, the first whose end
// lies behind k (binary search: ends increase), and up to two successors that start at or before k.  With a the first one's value and
// S the sum of the weights (ascending j): out = a, then out = fmaf(w_j / S, v_j - a, out) for each later one -- a frame under one
// window is that window's value bit for bit, windows that agree give their common value bit for bit.
__global__ __launch_bounds__(256) void window_blend_kernel(WinArgs p) {
  const int k = blockIdx.x * 256 + threadIdx.x, f = blockIdx.y;
  if (k >= p.K) return;
  const int* start = p.start;
  int lo = 0, hi = p.n - 1;                  // start[n-1] + W = K > k
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (start[mid] + p.W > k) hi = mid; else lo = mid + 1;
  }
  const int j0 = lo;
  float w[3];
  float2 v[3];
  int m = 0;
  float S = 0.f;
  for (int j = j0; j < p.n && m < 3 && start[j] <= k; ++j, ++m) {
    const int t = k - start[j];
    w[m] = window_weight(start, p.n, p.W, j, t);
    v[m] = p.src[((size_t)j * p.F + f) * p.W + t];
    S += w[m];
  }
  float2 out = v[0];
  for (int i = 1; i < m; ++i) {
    const float r = w[i] / S;
    out.x = fmaf(r, v[i].x - v[0].x, out.x);
    out.y = fmaf(r, v[i].y - v[0].y, out.y);
  }
  p.dst[(size_t)f * p.K + k] = out;
}

}  // namespace sgmse
