// 3x3 convolution of the wide U-Net levels: fp16x2 operand split + 1-D Winograd F(4,3) along the frame axis.
//
// kernels_conv_wino.h (F(2,3)) is bound by the energy of its MFMAs; F(4,3) computes FOUR neighbouring output columns from 6 transformed
// inputs x 6 transformed weights: 18 MFMA K-steps per 4 outputs and kernel row against F(2,3)'s 24 (3/4 of the matrix work, of the hi/lo
// split arithmetic and of the LDS operand stores) and 1.5 accumulators per output instead of 2.  Interpolation points 0, +-1, +-2, inf:
//
//     d0..d5 = producer output at columns 4m-1 .. 4m+4 (zero outside the image), g0..g2 = the weights of one kernel row
//     V0 = 4 d0 - 5 d2 + d4            V1 = (d4 - 4 d2) + (d3 - 4 d1)      V2 = (d4 - 4 d2) - (d3 - 4 d1)
//     V3 = (d4 - d2) + 2 (d3 - d1)     V4 = (d4 - d2) - 2 (d3 - d1)        V5 = 4 d1 - 5 d3 + d5          (fp32, one fixed order, then hi + lo)
//     U0 = g0/4   U1 = -(g0+g1+g2)/6   U2 = -(g0-g1+g2)/6   U3 = g0/24 + g1/12 + g2/6   U4 = g0/24 - g1/12 + g2/6   U5 = g2   (fp64 at pack time)
//     M_k = sum over input channels and kernel rows of U_k V_k                            (6 implicit GEMMs, fp32 accumulation)
//     y(4m)   = M0 + M1 + M2 + M3 + M4           y(4m+1) = (M1 - M2) + 2 (M3 - M4)
//     y(4m+2) = (M1 + M2) + 4 (M3 + M4)          y(4m+3) = (M1 - M2) + 8 (M3 - M4) + M5
//
// Range: |V| <= 10 max|d|, so the input's power-of-two scale puts the producer's bound into [2^10, 2^11) (F(2,3): [2^13, 2^14));
// |U| <= max|g|.  Every extra factor is a power of two and exact.
//
// Layout: as kernels_conv_wino.h (one workgroup = 128 co x ROWS x 32 px, 8 waves, one workgroup per CU) with these differences:
//   * a GEMM column is a POSITION (image row, column QUAD); an MFMA B fragment = 32 positions = 4 rows x 8 quads; a tile holds ROWS/4
//     position fragments.  Wave (cf, kh) owns channel fragment cf and the components {3 kh, 3 kh + 1, 3 kh + 2}: 3 x ROWS/4 accumulators
//     (96 registers for ROWS = 8), every weight fragment private to one wave.
//   * B operand in LDS: [row][quad][k 6][k-group][split], 25 x 16 B per (row, quad) (24 + 1: the 16 lanes of an LDS cycle hit 16
//     distinct bank quads); two stages double-buffered (2 x 31.25 KB, + 8 KB of producer coefficients).  What sizes the LDS
//     allocation of the 8-row shape is the epilogue's exchange area (128 KB, laid over the dead stage buffers behind the loop's last
//     barrier; 4-row shape: 70.5 KB): it fits the CU's 160 KB and, like F(2,3)'s 132 KB, rules out a second workgroup per CU.
//   * staging: a lane holds an ALIGNED column quad (x0 - 4 + 4 j .. + 3), j = 0..9, of 4 channels (one 16-byte load per channel); 10
//     lanes = one (4-channel group, tile row), 6 such rows per wave pass, one pass per wave.  The transform needs the last column of
//     lane - 1 and the first of lane + 1: the same two whole-wave DPP shifts per channel as F(2,3).  The width must be a multiple of 4.
//     In the K loop the item of the NEXT stage is cut into 56 units of whole elements (Wino43Units below) that sit BETWEEN the MFMAs
//     of the first STG taps of a stage (A-waves) or of its last STG taps (B-waves): MFMA, units, MFMA, units, ...  Measured
//     (DESIGN.md section 8, round 13): the gaps hide little of the item; the form is 1.2-1.6 % faster per launch than two halves
//     behind the MFMAs of two taps through shorter waits at the stage barriers and 7 % fewer vector instructions.
//   * A operand: [co block][stage][dy 3][k 6][split 2][cf 4][lane 64] fragments (18 pairs per stage), ring of three, two taps ahead.
//   * epilogue: A-waves form {M0 + (M1 + M2), M1 - M2, M1 + M2}, B-waves {s, 2 t, 4 s, 8 t + M5} (s = M3 + M4, t = M3 - M4); the
//     partners swap half through LDS behind one barrier, the A-wave finishes rows 0-3 and the B-wave rows 4-7 (4-row shape: the A-wave
//     everything).  y_i = pA_i + pB_i whoever finishes and the factors 2, 4, 8 are exact, so the 4-row and the 8-row shape give the
//     same bits.  A lane ends with the 4 columns of a quad of 16 channels: two 8-byte stores per channel, GroupNorm partials per
//     4 rows x 32 columns and the range bound exactly as conv3x3_wino_kernel emits them.
//   * no folded shortcut: the 1x1 shortcut runs as its own launch (conv1x1_split_kernel) and arrives here as the residual.
#pragma once
#include "kernels_conv_wino.h"
#include <utility>

// Taps of a K-stage over which a wave spreads the staging of the next stage's item (2: the item in two halves BEHIND the MFMAs of a
// fragment slot, the placement up to round 12; 3, 4: in units between the MFMAs).  One value per library; the others are for A/B runs of
// a measurement build (HIPCC_COMPILE_FLAGS_APPEND=-DSGMSE_WINO43_STG=2 make ABLATION=1).  The LDS image does not depend on it.
#ifndef SGMSE_WINO43_STG
#define SGMSE_WINO43_STG 3
#endif
// How the K loop's MFMAs get their operands, a bit mask (one value per library; 0 = the instruction order up to round 13, for A/B runs
// of one source as above).  No bit changes a value or an address, only when a load or read is issued:
//   1  B fragments one fragment slot ahead: fragment 0 of tap t + 1 is read from LDS in front of the MFMAs of the last fragment of
//      tap t; only the first fragment of a stage is read at the top of its tap, behind the stage barrier
//   2  A fragments through a raw buffer view of the weight block: per-lane offset in one register computed before the loop, (stage,
//      dy, k, split) in the scalar offset -- no address arithmetic on the vector ALU in the loop
//   4  (reserved: exact vmcnt waits behind a wave's raw look-ahead loads; not built)
//   8  the first two taps of the weight ring are loaded beside the other prologue loads, in front of the staging of item 0
// 3 ships.  Bit 8 measured inside the run-to-run spread on the headline and stays off.
#ifndef SGMSE_WINO43_FEED
#define SGMSE_WINO43_FEED 3
#endif

namespace sgmse {

template <class F, int... I>
__device__ __forceinline__ void wino43_unroll(F&& f, std::integer_sequence<int, I...>) { (f(std::integral_constant<int, I>{}), ...); }
template <int N, class F>
__device__ __forceinline__ void wino43_unroll(F&& f) { wino43_unroll(f, std::make_integer_sequence<int, N>{}); }    // f(0_c) ... f((N-1)_c)

// The staging item of one thread (4 channels x an aligned column quad -> 6 transformed values per channel -> fp16 hi/lo pairs -> 12
// 8-byte LDS stores) as 56 units in dependency order, each a few instructions of whole elements:
//   channel c (11 units): E0 E1 F0 F1 E2 E3 F2 F3 Ta Tb Tc    E = affine (+ the exponential of SiLU) of one element, F = its reciprocal,
//                                                             product and mask; Ta, Tb, Tc = the transform {V1 V2}, {V0 V3 V4}, {V5}
//   item: channel 0, channel 1, S0(k = 0..5), channel 2, channel 3, S1(k = 0..5)
//                                                             S0 = hi/lo split of channels 0,1 of component k (kept in registers),
//                                                             S1 = split of channels 2,3 + the two 8-byte stores of component k
// cost() = issue cycles (transcendental 8, other VALU 4, LDS store 4 + the exec mask around the pair); gap() deals the units out over
// the G = 3 NF STG MFMA gaps of the staging taps in proportion to it, in order.
template <int ACT>
struct Wino43Units {
  static constexpr int NCH = 11, NU = 4 * NCH + 12;
  enum Kind { E, F, TA, TB, TC, S0, S1 };
  static constexpr bool in_chan(int u) { return u < 2 * NCH || (u >= 2 * NCH + 6 && u < 4 * NCH + 6); }
  static constexpr int chan_pos(int u) { return u < 2 * NCH ? u : u - 6; }                    // (channel units only)
  static constexpr int chan(int u) { return chan_pos(u) / NCH; }
  static constexpr int first_unit(int c) { return c < 2 ? c * NCH : c * NCH + 6; }
  static constexpr Kind kind(int u) {
    if (!in_chan(u)) return u < 2 * NCH + 6 ? S0 : S1;
    const int j = chan_pos(u) % NCH;
    return j >= 8 ? (j == 8 ? TA : j == 9 ? TB : TC) : (j & 2) ? F : E;
  }
  static constexpr int elem(int u) { const int j = chan_pos(u) % NCH; return (j & 1) + 2 * (j >> 2); }      // (E, F)
  static constexpr int comp(int u) { return u < 2 * NCH + 6 ? u - 2 * NCH : u - (4 * NCH + 6); }            // (S0, S1)
  static constexpr int cost(int u) {
    const Kind k = kind(u);
    return k == E ? (ACT ? 16 : 4) : k == F ? (ACT ? 20 : 4) : k == TA ? 24 : k == TB ? 20 : k == TC ? 12 : k == S0 ? 16 : 28;
  }
  static constexpr int before(int u) { int s = 0; for (int i = 0; i < u; ++i) s += cost(i); return s; }
  static constexpr int gap(int u, int G) { return (2 * before(u) + cost(u)) * G / (2 * before(NU)); }         // monotone in u, < G
};

template <int ROWS_>
struct Wino43Geom {
  static constexpr int KC = 16, ROWS = ROWS_, TROWS = ROWS_ + 2, NF = ROWS_ / 4, NK = 6;
  static constexpr int PV = 25;                       // u32x4 per (row, quad): 6 k x 2 k-groups x 2 splits, + 1 (bank spread)
  static constexpr int ROW_V = 8 * PV;
  static constexpr int STAGE_V = TROWS * ROW_V;
  static constexpr int NSROW = 4 * TROWS;             // staging rows: (4-channel group q, tile row r), q fastest
  static constexpr int NPASS = (NSROW + 5) / 6;       // wave passes of 6 staging rows x 10 lanes (one per wave)
  static constexpr int CO_V = 512;                    // producer coefficient table, u32x4 per input channel
  static constexpr int NDIR = ROWS_ == 4 ? 1 : 2;     // epilogue exchange: B-waves -> A-waves only (4 rows), or both ways
  static constexpr int XCH_V = 4 * NDIR * 16 * 64;    // ... [channel fragment][direction][register][lane] float4
  static constexpr int LDS_V = (2 * STAGE_V + CO_V) > XCH_V ? (2 * STAGE_V + CO_V) : XCH_V;
  static_assert(NPASS <= 8, "one staging pass per wave");
};

// Weight packing.  src: OIHW fp32 [Cout][Cin][3][3]; dst: u32x4 [nCoBlk][Cin/16][dy 3][k 6][split 2][cf 4][lane 64], followed by
// nCoBlk * 128 floats: per output channel the factor 2^-e that undoes its weights' scale.  One thread per 16-byte fragment element.
inline size_t packed_wino43_frags(int cin, int cout) { return (size_t)((cout + 127) / 128) * (cin / 16) * 18 * 2 * 4 * 64; }
inline size_t packed_wino43_bytes(int cin, int cout) { return packed_wino43_frags(cin, cout) * 16 + (size_t)((cout + 127) / 128) * 128 * 4; }

__device__ __forceinline__ double wino43_u(double g0, double g1, double g2, int k) {
  return k == 0 ? 0.25 * g0 : k == 1 ? -(g0 + g1 + g2) / 6.0 : k == 2 ? -(g0 - g1 + g2) / 6.0
       : k == 3 ? g0 / 24.0 + g1 / 12.0 + g2 / 6.0 : k == 4 ? g0 / 24.0 - g1 / 12.0 + g2 / 6.0 : g2;
}
// max |transformed weight| of output channel co (<= max |g|): the channel's power-of-two scale.  One wave per channel: the lanes share the
// cin * 3 kernel rows and reduce by shuffles (a maximum does not depend on the order)
__global__ __launch_bounds__(64) void wino43_co_scale_kernel(const float* src, int cin, int cout, int cout_pad, float* inv_scale, float* scale) {
  const int co = blockIdx.x;
  if (co >= cout_pad) return;
  float m = 0.f;
  if (co < cout) {
    for (int i = threadIdx.x; i < cin * 3; i += 64) {
      const float* g = src + ((size_t)co * cin * 3 + i) * 3;
      m = fmaxf(m, fmaxf(0.25f * fabsf(g[0]), fabsf(g[2])));                  // |U0|, |U5|
      for (int k = 1; k < 5; ++k) m = fmaxf(m, fabsf((float)wino43_u(g[0], g[1], g[2], k)));
    }
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
  if (threadIdx.x == 0) {
    const float s = co < cout ? h2_weight_scale(m) : 1.f;
    scale[co] = s; inv_scale[co] = 1.f / s;
  }
}
__global__ __launch_bounds__(256) void pack_weights_wino43_kernel(PackWinoArgs p, const float* co_scale) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= p.total) return;
  const int lane = (int)(e & 63);
  size_t r = e >> 6;
  const int cf = (int)(r & 3); r >>= 2;
  const int split = (int)(r & 1); r >>= 1;
  const int k = (int)(r % 6); r /= 6;
  const int dy = (int)(r % 3); r /= 3;
  const int nst = p.cin / 16;
  const int st = (int)(r % nst);
  const int blk = (int)(r / nst);
  const int co = blk * 128 + cf * 32 + (lane & 31);
  const int c0 = st * 16 + 8 * (lane >> 5);
  const double ws = co < p.cout ? (double)co_scale[co] : 1.0;
  u32x4 o;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    uint32_t part[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int c = c0 + 2 * q + h;
      double u = 0.0;
      if (co < p.cout) {
        const float* g = p.src + (((size_t)co * p.cin + c) * 3 + dy) * 3;
        u = wino43_u(g[0], g[1], g[2], k);
      }
      u *= ws;
      const uint32_t hi = drt_f32_to_f16((float)u);
      const uint32_t lo = drt_f32_to_f16((float)(u - (double)drt_f16_to_f32(hi)));
      part[h] = split ? lo : hi;
    }
    o[q] = part[0] | (part[1] << 16);
  }
  reinterpret_cast<u32x4*>(p.dst)[e] = o;
}

// One 16-byte A fragment element through a raw buffer view (SGMSE_WINO43_FEED bit 2): drt_buf_load4 of sgmse_devrt.h; the CPU
// emulator's form of it lives here, next to its only use
#ifndef SGMSE_EMULATOR
__device__ __forceinline__ u32x4 wino43_buf_load4(const drt_buf& b, unsigned voff, unsigned soff) { return drt_buf_load4(b, voff, soff); }
#else
static inline u32x4 wino43_buf_load4(const drt_buf& b, unsigned voff, unsigned soff) { u32x4 v; memcpy(&v, b.p + voff + soff, 16); return v; }
#endif

// ACT: SiLU behind the GroupNorm affine of the fused producer (1) or the affine only (0).
// TRACE (measurement only, sgmse_bench_conv in an ABLATION build): phase time stamps per workgroup, 32 words as conv3x3_wino_kernel's
// ([0] placement, [1] start, [2] loop, [3] epilogue, [4] end, [5], [7]-[10] epilogue steps from [3], [6] stage barriers), the nine tap
// positions + barrier time of thread 0 (A-wave) in [11]-[20] and of thread 256 (B-wave) in [21]-[30]; tools/analyze_trace.py FILE wino43.
template <int ROWS, int ACT, int TRACE = 0>
__global__ __launch_bounds__(512, 1) void conv3x3_wino43_kernel(ConvArgs p) {
  using G = Wino43Geom<ROWS>;
  using T = WinoTile<ROWS>;
  using S = SplitH2;
  constexpr int NF = G::NF, PV = G::PV, NS = 2;
  __shared__ u32x4 s_all[G::LDS_V];
  u32x4* const s_in0 = s_all;
  u32x4* const s_in1 = s_all + G::STAGE_V;
  f32x4* const s_co = reinterpret_cast<f32x4*>(s_all + 2 * G::STAGE_V);

  const int tid = threadIdx.x;
  const int wave = drt_uniform(tid >> 6), lane = tid & 63, l31 = lane & 31, kg = lane >> 5;
  const int cf = wave & 3, kh = wave >> 2;
  unsigned long long* trace = nullptr;
  if constexpr (TRACE) {
    if (tid == 0 && p.trace) {
      trace = p.trace + 32 * (size_t)(blockIdx.y * gridDim.x + blockIdx.x);
      trace[0] = (unsigned long long)drt_hw_id() | ((unsigned long long)drt_xcc_id() << 32);
      trace[1] = drt_clock();
    }
  }
  const int Cin = p.C1 + p.C2;
  const int tiles_xg = (p.W + 31) >> 5;
  const int tiles_y = (p.H + ROWS - 1) / ROWS;
  int b, ty, tx;
  conv_tile_of(p, (int)blockIdx.x, (int)gridDim.x, tiles_xg, tiles_y, b, ty, tx);
  if (p.rag_w) { if (!conv_ragged_adjust(p, b, tx)) return; }
  const int H = p.H, W = p.W;
  const int tiles_x = (W + 31) >> 5;
  const int co_blk = blockIdx.y;
  const int x0 = tx * 32, y0 = ty * ROWS;
  const unsigned HW = (unsigned)H * (unsigned)W;

  // prologue loads, all issued before the first is waited for (as conv3x3_wino_kernel)
  float xb_raw = 0.f;
  if (p.xbound) xb_raw = p.xbound[b * kAmaxSpread + (tid & (kAmaxSpread - 1))];
  const bool cld = p.in_scale != nullptr && tid < Cin;
  const float csc = cld ? p.in_scale[b * Cin + (tid < Cin ? tid : 0)] : 1.f;
  const float csh = cld ? p.in_shift[b * Cin + (tid < Cin ? tid : 0)] : 0.f;

  // the staging item of this thread: staging row (q, r) = 6 wave + lane / 10, aligned column quad j = lane % 10
  const int it_sub = lane / 10, it_j = lane - 10 * it_sub;
  const int it_rr = 6 * wave + it_sub;
  const bool it_live = it_sub < 6 && it_rr < G::NSROW;
  const int it_q = it_rr & 3, it_r = it_live ? it_rr >> 2 : 0;
  const int it_gy = y0 - 1 + it_r, it_gx = x0 - 4 + 4 * it_j;
  const bool it_ok = it_live && it_gy >= 0 && it_gy < H && it_gx >= 0 && it_gx < W;     // (W % 4 == 0: a whole quad is in or out)
  const unsigned it_boff = ((unsigned)(4 * it_q) * HW + (it_ok ? (unsigned)(it_gy * W + it_gx) : 0u)) * 4u;
  const int it_woff = ((it_r * 8 + (it_j - 1)) * PV + (it_q >> 1) * NS) * 2 + (it_q & 1);   // in 8-byte units: entry (r, quad j - 1, k-group q / 2), half q % 2
  const bool it_wr = it_live && it_j >= 1 && it_j <= 8;
  const bool it_run = 6 * wave < G::NSROW;                                              // wave-uniform
  float rin[16];
  auto load_item = [&](int c0) {
    const bool first = c0 < p.C1;
    const float* base = first ? p.src1 + ((size_t)b * p.C1 + c0) * HW : p.src2 + ((size_t)b * p.C2 + (c0 - p.C1)) * HW;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const float4 v = *reinterpret_cast<const float4*>(reinterpret_cast<const char*>(base + (size_t)c * HW) + it_boff);
      rin[4 * c] = v.x; rin[4 * c + 1] = v.y; rin[4 * c + 2] = v.z; rin[4 * c + 3] = v.w;
    }
  };
  float V[6][4];
  auto produce_co = [&](float x, const f32x4& co) -> float {
    float o = x * co[0] + co[1];
    if constexpr (ACT == 1) {
      const float u = x * co[2] + co[3];
      o = o * __builtin_amdgcn_rcpf(1.0f + drt_exp2(u));
    }
    return it_ok ? o : 0.f;
  };
  // input transform of channel c of the item: the quad (d1..d4), the last column of lane - 1 (d0) and the first of lane + 1 (d5)
  auto stage_chan_co = [&](int c, const f32x4& co) {
    const float d1 = produce_co(rin[4 * c], co), d2 = produce_co(rin[4 * c + 1], co);
    const float d3 = produce_co(rin[4 * c + 2], co), d4 = produce_co(rin[4 * c + 3], co);
    const float d0 = drt_wave_shr1(d4), d5 = drt_wave_shl1(d1);
    const float a = d4 - d2, bb = d3 - d1;
    const float c4 = d4 - 4.f * d2, c3 = d3 - 4.f * d1;
    V[0][c] = 4.f * (d0 - d2) + a;
    V[1][c] = c4 + c3;
    V[2][c] = c4 - c3;
    V[3][c] = a + 2.f * bb;
    V[4][c] = a - 2.f * bb;
    V[5][c] = (d5 - d3) - 4.f * bb;
  };
  auto flush_item = [&](u32x4* sbuf) {
    if (it_wr) {
      uint2* w = reinterpret_cast<uint2*>(sbuf) + it_woff;
#pragma unroll
      for (int k = 0; k < 6; ++k) {
        uint32_t d01[2], d23[2];
        S::split2(V[k][0], V[k][1], d01);
        S::split2(V[k][2], V[k][3], d23);
        w[k * 8] = make_uint2(d01[0], d23[0]);          // (k: 4 u32x4 = 8 halves; split: 1 u32x4 = 2 halves)
        w[k * 8 + 2] = make_uint2(d01[1], d23[1]);
      }
    }
  };

  const int nst = Cin / G::KC;
  const float* cs_tab = p.co_scale + (size_t)co_blk * 128;
  float acc_raw[16];
  conv_acc_raw<T>(p, b, co_blk, cf, kg, acc_raw);
  auto load_cs = [&](float (&cs)[16]) {
#pragma unroll
    for (int r = 0; r < 16; ++r) cs[r] = cs_tab[cf * 32 + 4 * kg + (r & 3) + 8 * (r >> 2)];
  };
  if (it_run) load_item(0);
  float kx = 1.f;
  if (p.xbound) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) xb_raw = fmaxf(xb_raw, __shfl_xor(xb_raw, o));
    kx = h2_weight_scale(xb_raw) * 0.125f;              // |V| <= 10 max|d| < 10 * 2^11
  }
  const float inv_kx = 1.f / kx;
  if (tid < Cin) {
    constexpr float nl2e = -1.4426950408889634f;
    f32x4 v;
    v[0] = csc * kx; v[1] = csh * kx; v[2] = csc * nl2e; v[3] = csh * nl2e;
    s_co[tid] = v;
  }
  // accumulators: [component kk of this wave: k = 3 kh + kk][position fragment].  M1 enters every one of the four outputs with the
  // factor 1: the additive terms (bias + time-embedding row, in accumulator units) start there
  f32x16 acc[3][NF];
#pragma unroll
  for (int kk = 0; kk < 3; ++kk) {
    float init[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) init[r] = 0.f;
    if (kk == 1 && kh == 0) {
      float cs_inv[16];
      load_cs(cs_inv);
#pragma unroll
      for (int r = 0; r < 16; ++r) init[r] = acc_raw[r] * (kx / cs_inv[r]);
    }
#pragma unroll
    for (int f = 0; f < NF; ++f)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[kk][f][r] = init[r];
  }

  // A fragments of this wave: tap (dy, kk) of stage st -> [st][dy][3 kh + kk][split][cf][lane]
  const u32x4* wblk = reinterpret_cast<const u32x4*>(p.w) + (size_t)co_blk * nst * 18 * NS * 4 * 64;
  const unsigned a_boff = (unsigned)((cf * 64 + lane) * 16);
  constexpr int FEED = SGMSE_WINO43_FEED;
  constexpr bool B_AHEAD = (FEED & 1) != 0, A_BUF = (FEED & 2) != 0, A_EARLY = (FEED & 8) != 0;
  static_assert((FEED & ~11) == 0, "SGMSE_WINO43_FEED: bits 1, 2 and 8");
  // (A_BUF: a co block's fragments end below nst * 18 * NS * 4 * 64 * 16 bytes = 4.5 MB at 512 input channels, far below the view's 2^31)
  const drt_buf wbuf = drt_make_buf(reinterpret_cast<const float*>(wblk));
  auto load_a = [&](int st, int tap, u32x4 (&a)[NS]) {
    const int dy = tap / 3, k = 3 * kh + (tap - 3 * dy);
    if constexpr (A_BUF) {
      const unsigned soff = (unsigned)((st * 3 + dy) * 6 + k) * (unsigned)(NS * 4 * 64 * 16);
#pragma unroll
      for (int s = 0; s < NS; ++s) a[s] = wino43_buf_load4(wbuf, a_boff, soff + (unsigned)(s * 4 * 64 * 16));
    } else {
      const u32x4* q = wblk + (size_t)((st * 3 + dy) * 6 + k) * NS * 4 * 64;
#pragma unroll
      for (int s = 0; s < NS; ++s) a[s] = *reinterpret_cast<const u32x4*>(reinterpret_cast<const char*>(q + s * 4 * 64) + a_boff);
    }
  };
  // B fragment base of this lane: position (row 4 f + (l31 >> 3) [+ dy], quad l31 & 7), k-group kg
  const int b_lane = l31 * PV + kg * NS;

  // one unit of the next stage's item (Wino43Units): the expressions of produce_co, stage_chan_co and flush_item, element by element
  using U = Wino43Units<ACT>;
  constexpr int STG = SGMSE_WINO43_STG, NGAP = 3 * NF * STG;
  static_assert(STG >= 2 && 2 * STG < 9, "the two waves of a SIMD never stage in the same tap");
  struct Item {                // (every field is written once per stage, by one unit, before the units that read it)
    f32x4 co[4];
    float o[4][4], e[4][4], d[4][4], a[4], bb[4];     // an element between E and F; d1..d4 of a channel; a, bb of its transform
    float V[6][4];
    uint32_t h[6][2];                                 // hi / lo halves of channels 0,1 until channels 2,3 are there
  };
  // The units sit in conditional blocks (a wave stages or does not) and hand their values on through an Item.  At the join behind a
  // block the value "from the other side" has to be SOMETHING: an uninitialised variable becomes a zero the compiler materialises on
  // the path every wave runs (one v_mov per value), a variable that lives across stages a register held around the whole loop.
  // fresh() in front of the block gives the variable a register and no instruction; the block then writes into that register.
  auto fresh = [&](auto& x) __attribute__((always_inline)) {
#ifndef SGMSE_EMULATOR
    asm volatile("" : "=v"(x));
#else
    (void)x;
#endif
  };
  auto fresh_outputs = [&](auto u_c, Item& it) __attribute__((always_inline)) {
    constexpr int u = decltype(u_c)::value;
    constexpr auto kind = U::kind(u);
    if constexpr (kind == U::E) { fresh(it.o[U::chan(u)][U::elem(u)]); if constexpr (ACT == 1) fresh(it.e[U::chan(u)][U::elem(u)]); }
    else if constexpr (kind == U::F) fresh(it.d[U::chan(u)][U::elem(u)]);
    else if constexpr (kind == U::TA) { fresh(it.a[U::chan(u)]); fresh(it.bb[U::chan(u)]); fresh(it.V[1][U::chan(u)]); fresh(it.V[2][U::chan(u)]); }
    else if constexpr (kind == U::TB) { fresh(it.V[0][U::chan(u)]); fresh(it.V[3][U::chan(u)]); fresh(it.V[4][U::chan(u)]); }
    else if constexpr (kind == U::TC) fresh(it.V[5][U::chan(u)]);
    else if constexpr (kind == U::S0) { fresh(it.h[U::comp(u)][0]); fresh(it.h[U::comp(u)][1]); }
  };
  auto unit = [&](auto u_c, Item& it, u32x4* nxt) __attribute__((always_inline)) {
    constexpr int u = decltype(u_c)::value;
    constexpr auto kind = U::kind(u);
    if constexpr (kind == U::E) {
      constexpr int c = U::chan(u), e = U::elem(u);
      it.o[c][e] = rin[4 * c + e] * it.co[c][0] + it.co[c][1];
      if constexpr (ACT == 1) it.e[c][e] = drt_exp2(rin[4 * c + e] * it.co[c][2] + it.co[c][3]);
    } else if constexpr (kind == U::F) {
      constexpr int c = U::chan(u), e = U::elem(u);
      float o = it.o[c][e];
      if constexpr (ACT == 1) o = o * __builtin_amdgcn_rcpf(1.0f + it.e[c][e]);
      it.d[c][e] = it_ok ? o : 0.f;
    } else if constexpr (kind == U::TA) {
      constexpr int c = U::chan(u);
      it.a[c] = it.d[c][3] - it.d[c][1]; it.bb[c] = it.d[c][2] - it.d[c][0];
      const float c4 = it.d[c][3] - 4.f * it.d[c][1], c3 = it.d[c][2] - 4.f * it.d[c][0];
      it.V[1][c] = c4 + c3;
      it.V[2][c] = c4 - c3;
    } else if constexpr (kind == U::TB) {
      constexpr int c = U::chan(u);
      const float d0 = drt_wave_shr1(it.d[c][3]);
      it.V[0][c] = 4.f * (d0 - it.d[c][1]) + it.a[c];
      it.V[3][c] = it.a[c] + 2.f * it.bb[c];
      it.V[4][c] = it.a[c] - 2.f * it.bb[c];
    } else if constexpr (kind == U::TC) {
      constexpr int c = U::chan(u);
      const float d5 = drt_wave_shl1(it.d[c][0]);
      it.V[5][c] = (d5 - it.d[c][2]) - 4.f * it.bb[c];
    } else if constexpr (kind == U::S0) {
      constexpr int k = U::comp(u);
      S::split2(it.V[k][0], it.V[k][1], it.h[k]);
    } else {
      constexpr int k = U::comp(u);
      uint32_t d23[2];
      S::split2(it.V[k][2], it.V[k][3], d23);
      if (it_wr) {
        uint2* w = reinterpret_cast<uint2*>(nxt) + it_woff;
        w[k * 8] = make_uint2(it.h[k][0], d23[0]);
        w[k * 8 + 2] = make_uint2(it.h[k][1], d23[1]);
      }
    }
  };

  // one tap = component k of kernel row dy: NF position fragments x 3 split products.  SLOT >= 0: the SLOT-th of this wave's STG staging
  // taps -- behind each MFMA the units of that gap, in a conditional block of their own (stage_here: this wave stages in this tap), whose
  // ends also fence them: the scheduler moves nothing across (STG = 2: behind each fragment's three MFMAs half of the item's channels
  // 2 SLOT, 2 SLOT + 1, and the LDS writes at the end of slot 1)
  // B_AHEAD: a fragment is read one fragment slot ahead of its MFMAs, across taps too -- fragment 0 of tap t + 1 in front of the MFMAs
  // of the last fragment of tap t; read_b(., 0, 0) behind the stage barrier (the other buffer is written until then), tap 8 reads
  // nothing ahead.  Slot of (tap, f) in bq: f at NF = 2, tap & 1 at NF = 1 (tap 8 and the next stage's tap 0 both 0: that read sits
  // behind tap 8's MFMAs and the barrier)
  u32x4 bq[2][NS];
  auto read_b = [&](const u32x4* sbuf, auto tap_c, auto f_c) __attribute__((always_inline)) {
    constexpr int tap = decltype(tap_c)::value, f = decltype(f_c)::value;
    constexpr int dy = tap / 3, kk = tap - 3 * dy, slot = NF > 1 ? (f & 1) : (tap & 1);
    const u32x4* q = sbuf + b_lane + dy * G::ROW_V + (3 * kh + kk) * 4 + f * 4 * G::ROW_V;
#pragma unroll
    for (int s = 0; s < NS; ++s) bq[slot][s] = q[s];
  };
  auto compute_tap = [&](auto slot_c, auto tap_c, bool stage_here, Item& it, const u32x4* sbuf, const u32x4 (&a)[NS], int c0n, u32x4* nxt) __attribute__((always_inline)) {
    constexpr int SLOT = decltype(slot_c)::value;
    constexpr int tap = decltype(tap_c)::value;
    constexpr bool SPREAD = SLOT >= 0 && STG > 2;
    constexpr int dy = tap / 3, kk = tap - 3 * dy;
    const u32x4* sb = sbuf + b_lane + dy * G::ROW_V + (3 * kh + kk) * 4;
    if constexpr (SPREAD) {
      wino43_unroll<4>([&](auto c_c) __attribute__((always_inline)) {       // the coefficients of the channels that begin in this tap
        constexpr int c = decltype(c_c)::value;
        if constexpr (U::gap(U::first_unit(c), NGAP) / (3 * NF) == SLOT) {
          fresh(it.co[c]);
          if (stage_here) it.co[c] = s_co[c0n + 4 * it_q + c];
        }
      });
    } else if constexpr (SLOT >= 0) {
      if (stage_here) {
#pragma unroll
        for (int c = 0; c < 2; ++c) it.co[c] = s_co[c0n + 4 * it_q + 2 * SLOT + c];
      }
    }
    if constexpr (!B_AHEAD) {
#pragma unroll
      for (int s = 0; s < NS; ++s) bq[0][s] = sb[s];
    }
    wino43_unroll<NF>([&](auto f_c) __attribute__((always_inline)) {
      constexpr int f = decltype(f_c)::value;
      constexpr int bs = B_AHEAD && NF == 1 ? (tap & 1) : (f & 1);
      if constexpr (f + 1 < NF) {
        if constexpr (B_AHEAD) {
          read_b(sbuf, tap_c, std::integral_constant<int, f + 1>{});
        } else {
          const u32x4* q = sb + (f + 1) * 4 * G::ROW_V;
#pragma unroll
          for (int s = 0; s < NS; ++s) bq[(f + 1) & 1][s] = q[s];
        }
      } else if constexpr (B_AHEAD && tap + 1 < 9) {
        read_b(sbuf, std::integral_constant<int, tap + 1>{}, std::integral_constant<int, 0>{});
      }
      __builtin_amdgcn_sched_barrier(SGMSE_SPLIT_FENCE);
      wino43_unroll<S::NP>([&](auto k_c) __attribute__((always_inline)) {
        constexpr int k = decltype(k_c)::value;
        acc[kk][f] = S::mfma(a[S::pa(k)], bq[bs][S::pb(k)], acc[kk][f]);
        if constexpr (SPREAD) {
          constexpr int gap = (SLOT * NF + f) * S::NP + k;
          wino43_unroll<U::NU>([&](auto u_c) __attribute__((always_inline)) {
            if constexpr (U::gap(decltype(u_c)::value, NGAP) == gap) fresh_outputs(u_c, it);
          });
          if (stage_here) {
            wino43_unroll<U::NU>([&](auto u_c) __attribute__((always_inline)) {
              if constexpr (U::gap(decltype(u_c)::value, NGAP) == gap) unit(u_c, it, nxt);
            });
          }
        }
      });
      if constexpr (SLOT >= 0 && !SPREAD) {
        if (stage_here) {
          constexpr int CPF = 2 / NF;                 // channels per fragment slot (1 for 8 rows, 2 for 4)
#pragma unroll
          for (int c = 0; c < CPF; ++c) stage_chan_co(2 * SLOT + f * CPF + c, it.co[f * CPF + c]);
          if (SLOT == 1 && f == NF - 1) flush_item(nxt);
        }
      }
      __builtin_amdgcn_sched_barrier(SGMSE_SPLIT_FENCE);
    });
  };

  constexpr int AR = 3, AD = AR - 1, NTAP = 9;
  u32x4 ar[AR][NS];
  if constexpr (A_EARLY) {  // the ring's first two taps: issued behind item 0's raw loads (vmcnt retires in order), their L2 latency under its staging
#pragma unroll
    for (int t = 0; t < AD; ++t) load_a(0, t, ar[t]);
  }
  __syncthreads();          // s_co visible
  if (it_run) {
#pragma unroll
    for (int c = 0; c < 4; ++c) stage_chan_co(c, s_co[4 * it_q + c]);
    flush_item(s_in0);
    load_item((nst > 1 ? 1 : 0) * G::KC);        // raw inputs one full stage ahead
  }
  __syncthreads();

  if constexpr (TRACE) { if (trace) trace[2] = drt_clock(); }
  unsigned long long tbar = 0, ttap[NTAP] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  const bool tracer = TRACE && p.trace && (tid == 0 || tid == 256);       // one lane of an A-wave and of a B-wave time their taps
  if constexpr (!A_EARLY) {
#pragma unroll
    for (int t = 0; t < AD; ++t) load_a(0, t, ar[t]);
  }
#pragma unroll 1
  for (int st = 0; st < nst; ++st) {
    const int stn = st + 1 < nst ? st + 1 : st;
    const int stl = st + 2 < nst ? st + 2 : nst - 1;
    const u32x4* cur = (st & 1) ? s_in1 : s_in0;
    u32x4* nxt = (st & 1) ? s_in0 : s_in1;
    // staging of the next stage's item: the A-waves in the FIRST STG taps, the B-waves in the LAST STG (the two waves of a SIMD are
    // (cf, 0) and (cf, 1): de-phased, one wave's producer arithmetic issues beside the other's MFMAs); the last stage stages nothing
    // and the last two load nothing.  The raw inputs two stages ahead are fetched behind the last unit that reads rin.
    // (one item per role, declared here: its registers are live over that role's staging taps only)
    const bool stage_a = it_run && kh == 0 && st + 1 < nst, stage_b = it_run && kh == 1 && st + 1 < nst;
    Item item_a, item_b;
    wino43_unroll<NTAP>([&](auto tap_c) __attribute__((always_inline)) {
      constexpr int tap = decltype(tap_c)::value;
      unsigned long long tc0 = 0;
      if constexpr (TRACE) tc0 = drt_clock();
      constexpr int ntap = (tap + AD) % NTAP;
      const int nstg = tap + AD < NTAP ? st : stn;
      if constexpr (B_AHEAD && tap == 0) {             // the stage's first fragment: behind the barrier, ahead of the ring's address work
        read_b(cur, tap_c, std::integral_constant<int, 0>{});
        __builtin_amdgcn_sched_barrier(0);
      }
      load_a(nstg, ntap, ar[(tap + AD) % AR]);        // issued before the raw loads below: vmcnt retires in order
      __builtin_amdgcn_sched_barrier(0);
      constexpr bool ca = tap < STG;
      constexpr int slot = ca ? tap : tap >= NTAP - STG ? tap - (NTAP - STG) : -1;
      const bool stage_here = slot >= 0 && (ca ? stage_a : stage_b);
      compute_tap(std::integral_constant<int, slot>{}, tap_c, stage_here, ca ? item_a : item_b, cur, ar[tap % AR], stn * G::KC, nxt);
      if (slot == STG - 1 && stage_here && st + 2 < nst) load_item(stl * G::KC);
      if constexpr (TRACE) { __builtin_amdgcn_sched_barrier(0); ttap[tap] += drt_clock() - tc0; }
    });
    if constexpr (TRACE) {
      const unsigned long long tb = drt_clock();
      __syncthreads();
      tbar += drt_clock() - tb;
    } else {
      __syncthreads();
    }
  }
  if constexpr (TRACE) {
    if (trace) { trace[3] = drt_clock(); trace[6] = tbar; }
    if (tracer) {
      unsigned long long* tq = p.trace + 32 * (size_t)(blockIdx.y * gridDim.x + blockIdx.x) + (tid == 0 ? 11 : 21);
#pragma unroll
      for (int i = 0; i < NTAP; ++i) tq[i] = ttap[i];
      tq[NTAP] = tbar;
    }
  }

  // ---- output transform + epilogue in the accumulators' own (position) layout ---------------------------------------------------
  // (the loop's last barrier has passed: nobody reads the stage buffers any more)
  constexpr bool ALL_TO_A = ROWS == 4;
  const bool fin_wave = !ALL_TO_A || kh == 0;
  const int ef = ALL_TO_A ? 0 : kh;                        // the fragment (4 rows) this wave finishes
  int tid_e = (int)threadIdx.x;
  DRT_PIN_INT(tid_e);
  const int lane_e = tid_e & 63, l31_e = lane_e & 31, kg_e = lane_e >> 5;
  const int yy_raw = y0 + 4 * ef + (l31_e >> 3), x = x0 + 4 * (l31_e & 7);
  const bool okc = x < W;
  const bool inside = x0 + 32 <= W && y0 + ROWS <= H;      // workgroup-uniform: no access of the tile needs a guard
  const size_t ubase = (size_t)b * p.Cout * HW;
  const int co_l = co_blk * 128 + cf * 32 + 4 * kg_e;        // + (r & 3) + 8 (r >> 2)
  const int yy = yy_raw < H ? yy_raw : H - 1;              // (clamped into the image: guarded accesses never use the value)
  const unsigned lane_boff = (((unsigned)co_l * (unsigned)H + (unsigned)yy) * (unsigned)W + (unsigned)(okc ? x : 0)) * 4u;
  auto soff = [&](int r) -> unsigned { return (unsigned)((r & 3) + 8 * (r >> 2)) * HW * 4u; };
  const drt_buf obuf = drt_make_buf(p.out + ubase), rbuf = drt_make_buf(p.res ? p.res + ubase : p.out);
  const bool has_res = p.res != nullptr;
  float2 rr[16][2];
  if (fin_wave && has_res) {
#pragma unroll
    for (int r = 0; r < 16; ++r) { rr[r][0] = drt_buf_load2(rbuf, lane_boff, soff(r)); rr[r][1] = drt_buf_load2(rbuf, lane_boff + 8u, soff(r)); }
  }
  if constexpr (TRACE) { if (trace) trace[7] = drt_clock() - trace[3]; }       // residual loads issued
  float yv[4][16];
  {
    // exchange slots: [channel fragment][direction: 0 = for the A-wave, 1 = for the B-wave][register][lane] float4
    float4* xs = reinterpret_cast<float4*>(s_all);
    auto slot = [&](int dir, int r) -> float4* { return xs + (((cf * G::NDIR + dir) * 16 + r) * 64 + lane_e); };
    auto part_a = [&](int f, int r) -> float4 {
      const float m1 = acc[1][f][r], m2 = acc[2][f][r];
      const float sp = m1 + m2, sm = m1 - m2;
      return make_float4(acc[0][f][r] + sp, sm, sp, sm);
    };
    auto part_b = [&](int f, int r) -> float4 {
      const float m3 = acc[0][f][r], m4 = acc[1][f][r];
      const float s = m3 + m4, t = m3 - m4;
      return make_float4(s, 2.f * t, 4.f * s, 8.f * t + acc[2][f][r]);
    };
    if (kh == 0) {
      if constexpr (!ALL_TO_A) {
#pragma unroll
        for (int r = 0; r < 16; ++r) *slot(1, r) = part_a(NF - 1, r);
      }
    } else {
#pragma unroll
      for (int r = 0; r < 16; ++r) *slot(0, r) = part_b(0, r);
    }
    if constexpr (TRACE) { if (trace) trace[8] = drt_clock() - trace[3]; }     // partial sums written
    __syncthreads();
    if constexpr (TRACE) { if (trace) trace[9] = drt_clock() - trace[3]; }     // barrier passed
    if (!fin_wave) return;
    if (kh == 0) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float4 pb = *slot(0, r), pa = part_a(0, r);
        yv[0][r] = pa.x + pb.x; yv[1][r] = pa.y + pb.y; yv[2][r] = pa.z + pb.z; yv[3][r] = pa.w + pb.w;
      }
    } else {
      if constexpr (!ALL_TO_A) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float4 pa = *slot(1, r), pb = part_b(NF - 1, r);
          yv[0][r] = pa.x + pb.x; yv[1][r] = pa.y + pb.y; yv[2][r] = pa.z + pb.z; yv[3][r] = pa.w + pb.w;
        }
      }
    }
  }
  if constexpr (TRACE) { if (trace) trace[5] = drt_clock() - trace[3]; }
  auto finish = [&](auto guard_tag) {
    constexpr bool GUARD = decltype(guard_tag)::value;
    float cs_inv[16];
    load_cs(cs_inv);
    float s1[16], s2[16], vmax = 0.f;
    const bool ok = !GUARD || (okc && yy_raw < H);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      float v[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i] = yv[i][r] * cs_inv[r] * inv_kx;      // exact powers of two
      if (has_res) { v[0] += rr[r][0].x; v[1] += rr[r][0].y; v[2] += rr[r][1].x; v[3] += rr[r][1].y; }
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i] *= p.out_scale;
      if (ok) {
        drt_buf_store2(obuf, make_float2(v[0], v[1]), lane_boff, soff(r));
        drt_buf_store2(obuf, make_float2(v[2], v[3]), lane_boff + 8u, soff(r));
      }
      if (GUARD) {
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = ok ? v[i] : 0.f;
      }
      vmax = fmaxf(fmaxf(vmax, fmaxf(fabsf(v[0]), fabsf(v[1]))), fmaxf(fabsf(v[2]), fabsf(v[3])));
      s1[r] = (v[0] + v[1]) + (v[2] + v[3]);
      s2[r] = (v[0] * v[0] + v[1] * v[1]) + (v[2] * v[2] + v[3] * v[3]);
    }
    DRT_PIN_HERE(vmax);
    if constexpr (TRACE) { if (trace) trace[10] = drt_clock() - trace[3]; }    // outputs stored (issued)
    if (p.stats_out && y0 + 4 * ef < H) {
      // {sum, sum of squares} of the wave's 4-row x 32-column sub-tile per channel (the butterfly of conv3x3_wino_kernel)
      auto butterfly = [&](float (&sv)[16]) -> float {
        float a[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) a[k] = drt_xadd<16>(sv[k], sv[k + 8]);
        float c[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) c[k] = drt_xadd<8>(a[k], a[k + 4]);
        const float d0 = drt_xadd<7>(c[0], c[2]), d1 = drt_xadd<7>(c[1], c[3]);
        return drt_add_xor2(drt_xadd<1>(d0, d1));
      };
      const float e2 = butterfly(s2);
      __builtin_amdgcn_sched_barrier(0);
      const float e1 = butterfly(s1);
      const int r = ((l31_e >> 4) & 1) * 8 + ((l31_e >> 3) & 1) * 4 + ((l31_e >> 2) & 1) * 2 + (l31_e & 1);
      const int co = co_l + (r & 3) + 8 * (r >> 2);
      float* so = p.stats_out + ((size_t)(b * p.Cout + co) * p.stats_nsub + (size_t)((y0 + 4 * ef) >> 2) * tiles_x + tx) * 2;
      so[0] = e1; so[1] = e2;
    }
    if (p.amax_out) {
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) vmax = fmaxf(vmax, __shfl_xor(vmax, o));
      if (lane_e == 0) drt_atomic_max_nonneg(p.amax_out + b * kAmaxSpread + ((blockIdx.x * 8 + wave) & (kAmaxSpread - 1)), vmax);
    }
    DRT_CODE_MARKER(GUARD);
  };
  if (inside) finish(std::false_type{}); else finish(std::true_type{});
  if constexpr (TRACE) { if (trace) trace[4] = drt_clock(); }
}

}  // namespace sgmse
