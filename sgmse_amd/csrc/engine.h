// Host-side engine: weight store (reference state_dict names), activation arena, the NCSN++ forward as a static
// kernel sequence, and the predictor-corrector / probability-flow sampler loop (hipGraph-captured per step).
//
// Mirrors, by behaviour, reference sgmse/backbones/ncsnpp.py:50-253 (module list) and :256-419 (forward),
// ncsnpp_48k.py (ordering deltas), layerspp.py:62-91,212-274 (AttnBlockpp, ResnetBlockBigGANpp),
// sampling/__init__.py:52-68 (pc_sampler) with predictors.py:56-65 and correctors.py:60-81, and sdes.py:72-89,
// 130-135,188-229 (OUVE discretisation).  Nothing here is numerics except index bookkeeping: all arithmetic is in
// the kernels.
#pragma once
#include <algorithm>
#include <map>
#include <string>
#include <vector>
#include <cstdio>
#include <stdexcept>

#include <deque>
#include <sgmse_devrt.h>
#include "dev_memory.h"
#include "kernels_conv.h"
#include "conv_launch.h"
#include "kernels_norm_fir.h"
#include "kernels_attn_misc.h"
#include "kernels_ode.h"
#include "ode_control.h"
#include "kernels_stft.h"
#include "../../include/sgmse_hip.h"     // sgmse_sampler_cfg, sgmse_ode_cfg: the samplers take the public structs

namespace sgmse {

struct NetCfg {
  int variant = 0;            // 0: ncsnpp, 1: ncsnpp_48k
  int nf = 128;
  int n_levels = 7;
  int ch_mult[8] = {1, 1, 2, 2, 2, 2, 2, 0};
  int num_res_blocks = 2;
  int n_attn = 1;
  int attn_res[8] = {16, 0, 0, 0, 0, 0, 0, 0};
  int image_size = 256;
  int progressive = 1;        // 0 none, 1 output_skip
  int progressive_input = 1;  // 0 none, 1 input_skip
  int scale_by_sigma = 1;
};

// ---- module layout (order and names of reference all_modules, ncsnpp.py:107-253) ---------------------------
struct Mod {
  enum Kind { FOURIER, LINEAR, CONV3, RES, ATTN, COMBINE, GN } kind;
  int idx, cin, cout;
  bool up, down;
  int res;                    // resolution (rows) of the level the module runs at; 0 for the time-embedding modules
};

inline bool cfg_has_attn(const NetCfg& c, int res) {
  for (int i = 0; i < c.n_attn; ++i) if (c.attn_res[i] == res) return true;
  return false;
}

inline std::vector<Mod> build_layout(const NetCfg& c) {
  std::vector<Mod> mods;
  int res = 0;                // of the level being laid out
  auto add = [&](Mod::Kind k, int cin, int cout, bool up = false, bool down = false) {
    mods.push_back(Mod{k, (int)mods.size(), cin, cout, up, down, res});
  };
  const int nf = c.nf, L = c.n_levels, temb = 4 * nf, channels = 4;
  add(Mod::FOURIER, 0, nf);
  add(Mod::LINEAR, 2 * nf, temb);
  add(Mod::LINEAR, temb, temb);
  res = c.image_size;
  add(Mod::CONV3, channels, nf);
  std::vector<int> hs_c{nf};
  int in_ch = nf;
  for (int l = 0; l < L; ++l) {
    res = c.image_size >> l;
    for (int r = 0; r < c.num_res_blocks; ++r) {
      const int out_ch = nf * c.ch_mult[l];
      add(Mod::RES, in_ch, out_ch);
      in_ch = out_ch;
      if (cfg_has_attn(c, res)) add(Mod::ATTN, in_ch, in_ch);
      hs_c.push_back(in_ch);
    }
    if (l != L - 1) {
      add(Mod::RES, in_ch, in_ch, false, true);
      if (c.progressive_input == 1) add(Mod::COMBINE, channels, in_ch);
      hs_c.push_back(in_ch);
    }
  }
  in_ch = hs_c.back();
  add(Mod::RES, in_ch, in_ch);
  add(Mod::ATTN, in_ch, in_ch);
  add(Mod::RES, in_ch, in_ch);
  for (int l = L - 1; l >= 0; --l) {
    res = c.image_size >> l;
    for (int r = 0; r < c.num_res_blocks + 1; ++r) {
      const int out_ch = nf * c.ch_mult[l];
      const int cin = in_ch + hs_c.back();
      hs_c.pop_back();
      add(Mod::RES, cin, out_ch);
      in_ch = out_ch;
    }
    if (cfg_has_attn(c, res)) add(Mod::ATTN, in_ch, in_ch);
    if (c.progressive == 1) { add(Mod::GN, in_ch, in_ch); add(Mod::CONV3, in_ch, channels); }
    if (l != 0) add(Mod::RES, in_ch, in_ch, true, false);
  }
  SG_REQUIRE(hs_c.empty(), "layout: skip stack not empty");
  if (c.progressive != 1) { add(Mod::GN, in_ch, in_ch); add(Mod::CONV3, in_ch, channels); }
  return mods;
}

// What launch_attn_core cannot run of a layout, as the text of the refusal, or "" (sgmse_configure refuses such a configuration as an
// invalid argument, before weights are loaded: the first forward is too late to find out).
inline std::string attn_config_error(const std::vector<Mod>& layout) {
  for (const Mod& m : layout)
    if (m.kind == Mod::ATTN && !attn_width_supported(m.cin))
      return "attention block at resolution " + std::to_string(m.res) + " has " + std::to_string(m.cin) +
             " channels; the attention kernel runs " + attn_widths_text() + " (choose ch_mult / attn_resolutions accordingly)";
  return "";
}

// expected parameter names and element counts, in named_parameters() order
inline std::vector<std::pair<std::string, size_t>> param_manifest(const NetCfg& c) {
  std::vector<std::pair<std::string, size_t>> out;
  out.push_back({"output_layer.weight", 8});
  out.push_back({"output_layer.bias", 2});
  const int temb = 4 * c.nf;
  for (const Mod& m : build_layout(c)) {
    const std::string p = "all_modules." + std::to_string(m.idx) + ".";
    auto put = [&](const char* k, size_t n) { out.push_back({p + k, n}); };
    switch (m.kind) {
      case Mod::FOURIER: put("W", c.nf); break;
      case Mod::LINEAR: put("weight", (size_t)m.cout * m.cin); put("bias", m.cout); break;
      case Mod::CONV3: put("weight", (size_t)m.cout * m.cin * 9); put("bias", m.cout); break;
      case Mod::GN: put("weight", m.cin); put("bias", m.cin); break;
      case Mod::COMBINE: put("Conv_0.weight", (size_t)m.cout * m.cin); put("Conv_0.bias", m.cout); break;
      case Mod::ATTN:
        put("GroupNorm_0.weight", m.cin); put("GroupNorm_0.bias", m.cin);
        for (int i = 0; i < 4; ++i) {
          out.push_back({p + "NIN_" + std::to_string(i) + ".W", (size_t)m.cin * m.cin});
          out.push_back({p + "NIN_" + std::to_string(i) + ".b", (size_t)m.cin});
        }
        break;
      case Mod::RES:
        put("GroupNorm_0.weight", m.cin); put("GroupNorm_0.bias", m.cin);
        put("Conv_0.weight", (size_t)m.cout * m.cin * 9); put("Conv_0.bias", m.cout);
        put("Dense_0.weight", (size_t)m.cout * temb); put("Dense_0.bias", m.cout);
        put("GroupNorm_1.weight", m.cout); put("GroupNorm_1.bias", m.cout);
        put("Conv_1.weight", (size_t)m.cout * m.cout * 9); put("Conv_1.bias", m.cout);
        if (m.cin != m.cout || m.up || m.down) { put("Conv_2.weight", (size_t)m.cout * m.cin); put("Conv_2.bias", m.cout); }
        break;
    }
  }
  return out;
}

// ---- weight packing on the device --------------------------------------------------------------------------
// dst[blk][c][tap][j] = W(co = blk*co_t + j, c, tap); the logical weight is the channel-concatenation of up to three
// sources, each either OIHW [cout_s][cin][taps] (io = 0) or NIN's [cin][cout_s] (io = 1, taps = 1).
struct PackArgs { const float* src[3]; int nsrc, cout_per_src, io, cin, taps, cout, co_t; float* dst; size_t total; };

__global__ __launch_bounds__(256) void pack_weights_kernel(PackArgs p) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= p.total) return;
  const int j = (int)(e % p.co_t);
  size_t r = e / p.co_t;
  const int t = (int)(r % p.taps); r /= p.taps;
  const int c = (int)(r % p.cin);
  const int blk = (int)(r / p.cin);
  const int co = blk * p.co_t + j;
  float v = 0.f;
  if (co < p.cout) {
    const int s = co / p.cout_per_src, cj = co % p.cout_per_src;
    v = p.io ? p.src[s][(size_t)c * p.cout_per_src + cj] : p.src[s][((size_t)cj * p.cin + c) * p.taps + t];
  }
  p.dst[e] = v;
}

// OIHW weights with the input channels zero-padded from cin to cin_pad (entry convolution on the MFMA kernels)
__global__ __launch_bounds__(256) void pad_cin_kernel(const float* src, float* dst, int cout, int cin, int cin_pad, int taps) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (size_t)cout * cin_pad * taps) return;
  const int t = (int)(e % taps);
  const int c = (int)((e / taps) % cin_pad);
  const int co = (int)(e / ((size_t)taps * cin_pad));
  dst[e] = c < cin ? src[((size_t)co * cin + c) * taps + t] : 0.f;
}

__global__ __launch_bounds__(256) void zero_floats_kernel(float* p, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) p[i] = 0.f;
}

__global__ __launch_bounds__(256) void fill_random_kernel(float* dst, size_t n, uint32_t seed) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  uint32_t h = (uint32_t)i * 2654435761u ^ seed;
  h ^= h >> 16; h *= 0x7feb352du; h ^= h >> 15; h *= 0x846ca68bu; h ^= h >> 16;
  dst[i] = (float)(h >> 8) * (2.0f / 16777216.0f) - 1.0f;
}

// Measurement only (sgmse_calib_stream): a stream of KNOWN size for calibrating the FETCH_SIZE / WRITE_SIZE counters in the run that
// reads them (MI355X_MICROARCH.md, HBM: gfx950's FETCH_SIZE under-reports coalesced streams by a width-dependent factor).  VEC = floats
// per lane and access (2: the 8-byte column pairs of the Winograd kernel's staging, 4: its 16-byte weight fragments); consecutive lanes
// read consecutive elements, a workgroup walks a contiguous chunk.  WRITE = 1: the same stream stored instead of loaded.
template <int VEC, int WRITE>
__global__ __launch_bounds__(256) void calib_stream_kernel(float* buf, size_t nvec, float* sink) {
  struct alignas(VEC * 4) vec_t { float v[VEC]; };
  vec_t* p = reinterpret_cast<vec_t*>(buf);
  const size_t per = (nvec + gridDim.x - 1) / gridDim.x;
  const size_t lo = (size_t)blockIdx.x * per, hi = lo + per < nvec ? lo + per : nvec;
  float acc = 0.f;
  for (size_t i = lo + threadIdx.x; i < hi; i += 256) {
    if constexpr (WRITE) { vec_t v; for (int k = 0; k < VEC; ++k) v.v[k] = (float)(i & 1023); p[i] = v; }
    else { const vec_t v = p[i]; for (int k = 0; k < VEC; ++k) acc += v.v[k]; }
  }
  if (!WRITE && acc == 123456.789f) sink[0] = acc;
}

// Test hook (SGMSE_POISON_LDS=1): fill the whole LDS of every CU with NaN bit patterns in front of every launch of an eager forward, so
// that a kernel reading LDS it never wrote -- whose result then depends on what the PREVIOUS workgroup on that CU left there, i.e. on what
// else runs on the device -- shows up as a changed result (round 6: tools/probes/concurrency_bits_probe.py).  One workgroup owns a CU.
__global__ __launch_bounds__(256) void lds_poison_kernel(unsigned* sink, unsigned salt) {
  __shared__ unsigned s[40960];                    // 160 KiB
  for (int i = threadIdx.x; i < 40960; i += 256) s[i] = 0x7FC00000u | ((unsigned)i + salt);
  __syncthreads();
  if (s[(threadIdx.x * 97 + salt) % 40960] == 0x12345678u) sink[0] = 1u;
}

// [cin][cout] -> [cout][cin]
__global__ __launch_bounds__(256) void transpose_io_kernel(const float* src, float* dst, int cin, int cout) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= cin * cout) return;
  const int co = e / cin, c = e % cin;
  dst[e] = src[(size_t)c * cout + co];
}

// ---- arena ---------------------------------------------------------------------------------------------------
// Deterministic first-fit pool over one device allocation.  In "measure" mode nothing is backed by memory and only
// the high-water mark is tracked (used to size the real arena before the first run / graph capture).
class Arena {
 public:
  void reset() { free_.clear(); free_.push_back({0, cap_}); live_.clear(); deferring_ = false; deferred_.clear(); }
  void configure(char* base, size_t cap) { base_ = base; cap_ = cap; live_.clear(); reset(); }
  // measure mode hands out addresses from an unmapped fake range; they are never dereferenced (dry run)
  void measure_mode() { base_ = reinterpret_cast<char*>(uintptr_t(1) << 44); cap_ = size_t(1) << 42; high_ = 0; reset(); live_.clear(); }
  size_t high_water() const { return high_; }
  float* alloc(size_t nfloats) {
    size_t bytes = (nfloats * 4 + 255) / 256 * 256;
    if (bytes == 0) bytes = 256;
    for (size_t i = 0; i < free_.size(); ++i) {
      if (free_[i].second >= bytes) {
        const size_t off = free_[i].first;
        free_[i].first += bytes; free_[i].second -= bytes;
        if (free_[i].second == 0) free_.erase(free_.begin() + i);
        live_[off] = bytes;
        if (off + bytes > high_) high_ = off + bytes;
        return reinterpret_cast<float*>(base_ + off);
      }
    }
    throw EngineError("activation arena exhausted");
  }
  // Deferred releases (side branches of the forward on a second stream, Engine::side_begin): a buffer released by the side branch, or
  // by the main chain while the side branch may still read it, goes back to the pool only at the join -- nothing enqueued in between
  // can be handed memory that an unfinished kernel of the other stream still uses.
  void defer_begin() { deferring_ = true; }
  void defer_end() { deferring_ = false; std::vector<float*> d; d.swap(deferred_); for (float* p : d) release(p); }
  void release(float* p) {
    if (!p) return;
    if (deferring_) { deferred_.push_back(p); return; }
    const size_t off = size_t(reinterpret_cast<char*>(p) - base_);
    auto it = live_.find(off);
    SG_REQUIRE(it != live_.end(), "arena: bad release");
    size_t bytes = it->second;
    live_.erase(it);
    size_t i = 0;
    while (i < free_.size() && free_[i].first < off) ++i;
    free_.insert(free_.begin() + i, {off, bytes});
    if (i + 1 < free_.size() && free_[i].first + free_[i].second == free_[i + 1].first) {
      free_[i].second += free_[i + 1].second; free_.erase(free_.begin() + i + 1);
    }
    if (i > 0 && free_[i - 1].first + free_[i - 1].second == free_[i].first) {
      free_[i - 1].second += free_[i].second; free_.erase(free_.begin() + i);
    }
  }
 private:
  char* base_ = nullptr;
  size_t cap_ = 0, high_ = 0;
  std::vector<std::pair<size_t, size_t>> free_;
  std::map<size_t, size_t> live_;
  bool deferring_ = false;
  std::vector<float*> deferred_;
};

// st: [B][C][nsub][2] GroupNorm partial sums; amax: [B] upper bounds of |x| per utterance (null: unknown range)
// srows: image rows per statistics sub-tile (1: the fp32 kernels, 4: the split kernels; ConvArgs::stats_rows)
struct Tensor { float* p = nullptr; int C = 0, H = 0, W = 0; float* st = nullptr; int nsub = 0; float* amax = nullptr; int srows = 1; };

struct ConvW {            // one convolution's parameters on the device
  const float* oihw = nullptr;   // [cout][cin][ks][ks] (for NIN: transposed copy)
  const float* packed = nullptr; // MFMA layout (null if the shape is not MFMA-eligible)
  const float* packed32 = nullptr; // second MFMA layout with 32-channel output tiles: 4x more workgroups for launches that
                                   // would otherwise leave most CUs idle (the 16x32 ... 4x8 levels of the U-Net)
  const float* packed_thin = nullptr;  // [ci][tap][4 co] of the C -> 4 layers (kernels_conv_thin.h)
  const float* packed_split = nullptr; // split-kernel fragment layout (kernels_conv_split.h) in the engine's split mode,
                                       // 3x3 with cout % 128 == 0, cin % 16 == 0
  const float* split_scale = nullptr;  // fp16x2: per output channel the factor undoing its weights' power-of-two scale (table behind the fragments)
  int split_mode = 0;                  // 1 bf16x3, 2 fp16x2 (0: no split layout)
  const float* packed_wino = nullptr;  // Winograd x fp16x2 fragment layout in the engine's ONE form (wino_form), 3x3 with cout % 128 == 0, cin % 16 == 0
  const float* wino_scale = nullptr;   // ... and the per-output-channel factors behind it
  WinoForm wino_form = WinoForm::F23;  // F43 (kernels_conv_wino43.h) where SGMSE_WINO43 selects it, else F23 (kernels_conv_wino.h)
  const float* bias = nullptr;
  int ks = 1, cin = 0, cout = 0, co_t = 0;
};

struct ResW { const float *g0w, *g0b, *g1w, *g1b; ConvW c0, c1, c2; bool has_c2; int temb_off; };
struct AttnW { const float *gw, *gb; ConvW qkv, proj; };

class Engine {
 public:
  explicit Engine(int device, void* stream) : device_(device) {
    SG_CHECK(drt::set_device(device));
    stream_ = reinterpret_cast<drt::stream_t>(stream);
    read_knobs();
  }
  ~Engine() {      // (buffers and events: released by their holders)
    if (graph_valid_ || graph_stale_) drt::graph_destroy(&graph_);
    if (side_stream_ready_) drt::stream_destroy(side_stream_);
  }

  drt::stream_t stream() const { return stream_; }
  void set_stream(void* s) { stream_ = reinterpret_cast<drt::stream_t>(s); }  // a captured graph can be launched on any stream

  // ---- weights ----------------------------------------------------------------------------------------------
  void set_config(const NetCfg& c) {
    std::vector<Mod> layout = build_layout(c);
    const std::string bad = attn_config_error(layout);
    SG_REQUIRE(bad.empty(), bad);
    cfg_ = c; layout_ = std::move(layout); weights_ready_ = false; invalidate_graph(); read_knobs();
  }
  const NetCfg& config() const { return cfg_; }

  void load_weights(const char* const* names, const void* const* ptrs, const long long* numels, int n, int on_device) {
    invalidate_graph();            // a captured graph refers to the old weight buffers
    weights_ready_ = false;
    release_weights();
    auto manifest = param_manifest(cfg_);
    std::map<std::string, size_t> want;
    size_t total = 0;
    for (auto& kv : manifest) { want[kv.first] = kv.second; total += (kv.second + 63) / 64 * 64; }
    float* blob = keep(fresh(total * 4));
    std::map<std::string, std::pair<const void*, long long>> given;
    for (int i = 0; i < n; ++i) given[names[i]] = {ptrs[i], numels[i]};
    size_t off = 0;
    W_.clear();
    for (auto& kv : manifest) {
      auto it = given.find(kv.first);
      if (it == given.end()) throw EngineError("load_weights: missing parameter " + kv.first);
      if ((size_t)it->second.second != kv.second)
        throw EngineError("load_weights: size mismatch for " + kv.first + " (got " + std::to_string(it->second.second) +
                          ", want " + std::to_string(kv.second) + ")");
      if (on_device) SG_CHECK(drt::memcpy_d2d(blob + off, it->second.first, kv.second * 4, stream_));
      else SG_CHECK(drt::memcpy_h2d(blob + off, it->second.first, kv.second * 4, stream_));
      W_[kv.first] = blob + off;
      off += (kv.second + 63) / 64 * 64;
    }
    if (!on_device) SG_CHECK(drt::stream_sync(stream_));  // host buffers may be released by the caller
    read_knobs();                  // (kernel-family knobs are per load, so one process can compare settings)
    finalize_weights();
  }

  size_t param_count() const { size_t n = 0; for (auto& kv : param_manifest(cfg_)) n += kv.second; return n; }

  // ---- network forward ----------------------------------------------------------------------------------------
  // x: complex64 [B][1][F][T] with batch stride xbs (complex elements), y likewise; t: device fp32.
  // out: complex64 [B][1][F][T] = sign * NCSNpp(cat[x,y], t).
  struct FwdCtl {
    const float* bias_table; int bias_bstride, bias_sstride; const int* step_ptr;
    const float* tvals; int t_bstride, t_sstride; float sign;
    const float* coef = nullptr; int coef_bstride = 0, coef_sstride = 0;   // score-wrapper rows {gamma, alpha, beta, -} or null
    const int* bias_step = nullptr;   // step counter the convolutions read for their bias row (null: row 0 / per-utterance rows)
    int y_plane = 0;     // ragged launches: y of utterance b lies y_plane * F * T_b elements behind its x-relative position (entry_kernel)
  };

  void forward_xy(const float2* xy, const float* t_dev, float2* out, int B, int F, int T) {
    // public single-evaluation entry: xy is [B][2][F][T]; t is a device array [B]
    require_ready();
    ensure_shape(B, F, T, /*nrows=*/B);
    compute_temb(t_dev, B);
    FwdCtl ctl{bias_table_, tot_temb_, 0, nullptr, t_dev, 1, 0, 1.0f};
    const long long FT = (long long)F * T;
    arena_.reset();
    if (ragged()) {          // xy: utterance after utterance, each [2][F][T_b]; out: each [F][T_b]
      ctl.y_plane = 1;
      run_forward(xy, 2, xy, 2, out, B, F, T, ctl);
    } else {
      run_forward(xy, 2 * FT, xy + FT, 2 * FT, out, B, F, T, ctl);
    }
  }

  // ---- sampler --------------------------------------------------------------------------------------------------
  // what a captured step depends on.  The Philox seed is NOT part of it: the sampler kernels read it from a device word
  // (upload_tables), so one capture serves every utterance / batch of a run (the Python samplers draw a fresh seed per call)
  struct GraphKey {
    int B, F, T, corr, ncorr, pred, pf; const void* y; const void* noise; float theta; int dps;
    int win = 0;      // serial number of the window plan the step evaluates the network under (set_windows), 0: none
    bool operator==(const GraphKey& o) const {
      return B == o.B && F == o.F && T == o.T && corr == o.corr && ncorr == o.ncorr && pred == o.pred && pf == o.pf && y == o.y &&
             noise == o.noise && theta == o.theta && dps == o.dps && win == o.win;
    }
  };
  // What the fixed-step samplers share in front of their loop.  fill(i, row) writes step i's row of the step table (row[SC_T] = its
  // time); in_scale / alpha / beta are the score wrapper's host arrays [N], all three or none.  Tables and seed -> device (no host
  // synchronisation: pinned staging), time embeddings of the N steps, y -> the engine-owned copy (a captured graph never refers to
  // caller memory).  Returns the device seed words and the network's control block; ctl.coef is set iff the wrapper was given.
  struct StepSetup { const unsigned long long* seed; FwdCtl ctl; };
  template <class Fill>
  StepSetup begin_steps(const char* who, const float2* Y, size_t n, int B, int N, unsigned long long seed, Fill&& fill,
                        const float* in_scale, const float* alpha, const float* beta) {
    std::vector<float> tab((size_t)N * SC_STRIDE, 0.f), tv(N), cf;
    for (int i = 0; i < N; ++i) { float* r = &tab[(size_t)i * SC_STRIDE]; fill(i, r); tv[i] = r[SC_T]; }
    const bool affine = in_scale && alpha && beta;
    SG_REQUIRE(affine || (!in_scale && !alpha && !beta), std::string(who) + ": give all three score-wrapper arrays or none");
    if (affine) {
      cf.assign((size_t)N * 4, 0.f);
      for (int i = 0; i < N; ++i) { cf[4 * i] = in_scale[i]; cf[4 * i + 1] = alpha[i]; cf[4 * i + 2] = beta[i]; }
    }
    const unsigned long long* seed_dev = upload_tables(tab, tv, cf, seed, B);
    compute_temb(tsteps_, N);
    SG_CHECK(drt::memcpy_d2d(sy_, Y, n * 8, stream_));
    FwdCtl ctl{bias_table_, 0, tot_temb_, step_ctr_, tsteps_, 0, 1, -1.0f};
    if (affine) { ctl.coef = coef_table_; ctl.coef_bstride = 0; ctl.coef_sstride = 1; }
    return {seed_dev, ctl};
  }
  // N times the step `body`: as replays of the engine's ONE captured graph (captured anew, or updated in place, when `key` is not the
  // captured step's), or eagerly
  template <class Body>
  void run_steps(int N, const GraphKey& key, bool use_graph, Body&& body) {
    if (use_graph && drt::graphs_supported()) {
      if (!graph_valid_ || !(key == graph_key_)) {
        invalidate_graph();
        capture_step(body);
        graph_key_ = key;
      }
      for (int i = 0; i < N; ++i) SG_CHECK(drt::graph_launch(&graph_, stream_));
    } else {
      for (int i = 0; i < N; ++i) body();
    }
  }
  // prior: sx_ = sy_ + std1 z over the n packed elements, z = noise (replayed, draw 0) or the Philox stream of the seed words
  void draw_prior(const float2* noise, const unsigned long long* seed_dev, float std1, size_t n, int B, int per) {
    SamplerArgs sa{};
    sa.x = sx_; sa.y = sy_; sa.noise = noise; sa.seed = seed_dev; sa.std1 = std1; sa.n = (int)n; sa.B = B; sa.per = per;
    sa.rag_off = rag_off0();
    DRT_LAUNCH(sampler_prior_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), stream_, sa);
  }

  void pc_sample(const float2* Y, float2* out, int B, int F, int T, const sgmse_sampler_cfg& sc, const float2* noise,
                 unsigned long long seed) {
    require_ready();
    SG_REQUIRE(sc.N >= 1 && sc.t && sc.dt && sc.G && sc.G2, "pc_sample: step table missing");
    SG_REQUIRE(sc.corrector != 1 || (sc.ald_eps && sc.ald_noise), "pc_sample: ALD table missing");
    if (windowed()) win_begin("pc_sample", B, F, T, sc.N);
    else ensure_shape(B, F, T, sc.N);
    take_noise_frames("pc_sample", B, T, noise);
    SG_REQUIRE(!ragged() || sc.corrector != 2, "ragged batches: the Langevin corrector with the step size of the batch couples the utterances (correctors.py:50-52) "
                                               "and is not supported; corrector = 3 takes the step size per utterance");
    const size_t n = ragged() ? rag_[0].pix : (size_t)B * F * T;     // complex elements of Y / the result, utterance after utterance
    const StepSetup st = begin_steps("pc_sample", Y, n, B, sc.N, seed, [&](int i, float* r) {
      r[SC_T] = sc.t[i]; r[SC_DT] = sc.dt[i]; r[SC_G] = sc.G[i]; r[SC_G2] = sc.G2[i];
      if (sc.corrector == 1) { r[SC_ALD_EPS] = sc.ald_eps[i]; r[SC_ALD_NOISE] = sc.ald_noise[i]; }
    }, sc.in_scale, sc.score_alpha, sc.score_beta);
    const FwdCtl& ctl = st.ctl;

    const int ncorr = sc.corrector ? sc.corrector_steps : 0;
    const bool langevin = sc.corrector == 2 || sc.corrector == 3;       // 3: step size per utterance (lang_scal_: [B][2])
    const bool pred_noise = sc.predictor == 1 && !sc.probability_flow;
    const int draws_per_step = ncorr + (pred_noise ? 1 : 0);

    SamplerArgs sa{};
    sa.x = sx_; sa.x_mean = sxm_; sa.y = sy_; sa.score = sscore_; sa.noise = noise; sa.seed = st.seed;
    sa.table = step_table_; sa.step_ptr = step_ctr_; sa.theta = sc.theta; sa.std1 = sc.std1; sa.n = (int)n;
    sa.score_w = sc.probability_flow ? 0.5f : 1.0f;
    sa.snr = sc.snr; sa.B = B; sa.per = F * T; sa.partial = lang_partial_; sa.lang = lang_scal_;
    sa.rag_off = rag_off0();
    const dim3 eg((unsigned)((n + 255) / 256));

    draw_prior(noise, st.seed, sc.std1, n, B, F * T);
    SG_CHECK(drt::memcpy_d2d(sxm_, sx_, n * 8, stream_));
    DRT_LAUNCH(step_set_kernel, dim3(1), dim3(64), stream_, step_ctr_.get(), 0);
    if (windowed()) win_gather_y(F);

    auto step_body = [&]() {
      for (int cs = 0; cs < ncorr; ++cs) {
        eval_score(B, F, T, ctl);
        SamplerArgs a = sa; a.draw_base = 1 + cs; a.draw_per_step = draws_per_step;
        if (sc.corrector == 3) {
          DRT_LAUNCH(sampler_langevin_norms_each_kernel, dim3(LANG_NBLK, B), dim3(256), stream_, a);
          DRT_LAUNCH(sampler_langevin_scalars_each_kernel, dim3(1), dim3(64), stream_, a);
          DRT_LAUNCH(sampler_langevin_each_kernel, eg, dim3(256), stream_, a);
        } else if (sc.corrector == 2) {
          DRT_LAUNCH(sampler_langevin_norms_kernel, dim3(LANG_NBLK, B), dim3(256), stream_, a);
          DRT_LAUNCH(sampler_langevin_scalars_kernel, dim3(1), dim3(64), stream_, a);
          DRT_LAUNCH(sampler_langevin_kernel, eg, dim3(256), stream_, a);
        } else {
          DRT_LAUNCH(sampler_ald_kernel, eg, dim3(256), stream_, a);
        }
      }
      if (sc.predictor == 1) {
        eval_score(B, F, T, ctl);
        SamplerArgs a = sa; a.draw_base = 1 + ncorr; a.draw_per_step = draws_per_step; a.add_noise = pred_noise ? 1 : 0;
        DRT_LAUNCH(sampler_revdiff_kernel, eg, dim3(256), stream_, a);
      }
      // NonePredictor.update_fn returns (x, x) (predictors.py:69-76): xt_mean := xt also after a corrector moved them apart
      if (sc.predictor == 0 && ncorr > 0) SG_CHECK(drt::memcpy_d2d(sxm_, sx_, n * 8, stream_));
      DRT_LAUNCH(step_inc_kernel, dim3(1), dim3(64), stream_, step_ctr_.get());
    };
    run_steps(sc.N, GraphKey{B, F, T, sc.corrector, ncorr, sc.predictor, sc.probability_flow + (ctl.coef ? 2 : 0), (const void*)sy_, (const void*)noise,
                             sc.theta + 1000.f * sc.snr * langevin, draws_per_step, win_key()},      // (set_frames invalidates the graph itself)
              sc.use_graph, step_body);
    SG_CHECK(drt::memcpy_d2d(out, sc.denoise ? sxm_ : sx_, n * 8, stream_));
    nfe_ = sc.N * (ncorr + 1);   // the reference counts N*(corrector.n_steps+1) whatever the predictor (sampling/__init__.py:67)
  }
  // get_sb_sampler(...)() (sampling/__init__.py:145-249): N steps of  x <- w_prev x + w_est model(x, y, t) + w_y y + w_z z,
  // x_0 = y.  Host arrays [N]; coef (in_scale / alpha / beta, [N] each or all null) = the ScoreModel.forward wrapper.
  void sb_sample(const float2* Y, float2* out, int B, int F, int T, int N, const float* t, const float* w_prev, const float* w_est,
                 const float* w_y, const float* w_z, const float* in_scale, const float* alpha, const float* beta, int stochastic,
                 const float2* noise, unsigned long long seed, int use_graph) {
    require_ready();
    SG_REQUIRE(N >= 1 && t && w_prev && w_est && w_y && w_z, "sb_sample: step table missing");
    if (windowed()) win_begin("sb_sample", B, F, T, N);
    else ensure_shape(B, F, T, N);
    take_noise_frames("sb_sample", B, T, noise);
    const size_t n = ragged() ? rag_[0].pix : (size_t)B * F * T;     // complex elements of Y / the result, utterance after utterance
    const StepSetup st = begin_steps("sb_sample", Y, n, B, N, seed, [&](int i, float* r) {
      r[SC_T] = t[i]; r[SB_WPREV] = w_prev[i]; r[SB_WEST] = w_est[i]; r[SB_WY] = w_y[i]; r[SB_WZ] = w_z[i];
    }, in_scale, alpha, beta);
    const FwdCtl& ctl = st.ctl;
    SG_CHECK(drt::memcpy_d2d(sx_, Y, n * 8, stream_));          // x_0 = y
    DRT_LAUNCH(step_set_kernel, dim3(1), dim3(64), stream_, step_ctr_.get(), 0);

    SamplerArgs sa{};
    sa.x = sx_; sa.x_mean = sxm_; sa.y = sy_; sa.score = sscore_; sa.noise = noise; sa.seed = st.seed;
    sa.table = step_table_; sa.step_ptr = step_ctr_; sa.n = (int)n; sa.add_noise = stochastic ? 1 : 0; sa.B = B; sa.per = F * T;
    sa.draw_base = 0; sa.draw_per_step = 1; sa.rag_off = rag_off0();
    const dim3 eg((unsigned)((n + 255) / 256));
    if (windowed()) win_gather_y(F);
    auto step_body = [&]() {
      eval_score(B, F, T, ctl);
      DRT_LAUNCH(sampler_sb_kernel, eg, dim3(256), stream_, sa);
      DRT_LAUNCH(step_inc_kernel, dim3(1), dim3(64), stream_, step_ctr_.get());
    };
    run_steps(N, GraphKey{B, F, T, 100 + stochastic, 0, 0, ctl.coef ? 2 : 0, nullptr, (const void*)noise, 0.f, 1, win_key()}, use_graph, step_body);
    SG_CHECK(drt::memcpy_d2d(out, sx_, n * 8, stream_));
    nfe_ = N;
  }
  // the reference's fp32 expressions: g = sigma_min (sigma_max / sigma_min)^t sqrt(2 lambda); 0.5 g^2
  static double ode_g2half(const sgmse_ode_cfg& oc, float tf) {
    const double lam = std::log((double)oc.sigma_max / (double)oc.sigma_min);
    const float g = (float)((double)oc.sigma_min * std::pow((double)oc.sigma_max / (double)oc.sigma_min, (double)tf) * std::sqrt(2.0 * lam));
    return (double)(g * g * 0.5f);
  }
  // get_ode_sampler(..., denoise=False)() (sampling/__init__.py:96-143) with the solver inside the library: scipy's RK45
  // (Dormand-Prince 5(4), scipy/integrate/_ivp/rk.py) and its step control (common.py select_initial_step, RungeKutta._step_impl),
  // one controller (ode_control.h) per GROUP of the batch (kernels_ode.h).  State, slopes and error estimates stay on the device; the
  // host runs the step control in double and reads one scalar, the error norm, per group and attempted step.
  //   batch control (sgmse_ode_sample): G = 1, the flattened rectangular batch -- ONE error norm for all B*F*T complex elements, as
  //     scipy sees the state, so the utterances of a batch are coupled exactly as in the reference; the evaluation count is scipy's nfev.
  //   per-utterance control (sgmse_ode_sample_each): G = B, group g = utterance g of a uniform or ragged (sgmse_set_frames: packed
  //     tensors, as pc_sample takes them) batch, each with its own initial step, stage times, error norm, accept / reject decisions
  //     and end of integration, all fed by ONE batch evaluation per stage.  Utterance b's result, evaluation count, step counts and
  //     accepted times are those of batch control on that utterance alone: it is the same code with another number of groups.  A
  //     finished utterance is frozen: the network still evaluates its slot (at its last stage input, at t = eps), nothing of it is
  //     written.  max_nfe caps every utterance's own count; last_nfe() is the number of batch evaluations (the largest utterance's).
  // A "round" is one attempted step of every unfinished group: six batch evaluations at 6 G time-embedding rows (row = stage * G +
  // group), one table of [G][ODE_ROWS][ODE_STRIDE] doubles up, G error sums back.  coef_fn is called once per upload with its nt G
  // times STAGE-MAJOR (t[stage * G + g]): nt = 1 for f0 and for the probe of select_initial_step, 6 for a round.
  // Prior: x0 (given start state), else y + std1 z with z = noise (replayed, [B][F][T]) or the Philox stream of (seed, streams).
  void ode_run(const float2* Y, float2* out, int B, int F, int T, const sgmse_ode_cfg& oc, const float2* noise, const float2* x0,
               unsigned long long seed, bool per_utterance) {
    require_ready();
    const std::string who = per_utterance ? "ode_sample_each" : "ode_sample";
    if (windowed()) throw EngineArgError(who + ": a window plan (sgmse_set_windows) is not supported by the adaptive solver; withdraw it (n = 0)");
    SG_REQUIRE(per_utterance || !ragged(), "ode_sample: ragged batches are not supported: the solver's error norm couples the utterances of a batch "
                                           "(call sgmse_set_frames with n = 0 and pass a rectangular batch)");
    // (rtol, atol, first_step, max_step, max_nfe: checked once, at the C boundary)
    SG_REQUIRE(oc.t_end != oc.eps && oc.eps > 0 && oc.t_end > 0, who + ": bad time span");
    SG_REQUIRE(oc.sigma_min > 0 && oc.sigma_max > oc.sigma_min, who + ": bad sigma range");
    SG_REQUIRE(oc.first_step <= std::fabs(oc.eps - oc.t_end), who + ": `first_step` exceeds bounds");
    SG_REQUIRE(!per_utterance || B <= kOdeEachMaxB, "ode_sample_each: batch too large");
    const int G = per_utterance ? B : 1;
    ensure_shape(B, F, T, ODE_ROWS * G);
    take_noise_frames(who, B, T, noise);
    const size_t n = ragged() ? rag_[0].pix : (size_t)B * F * T;     // complex elements, utterance after utterance
    const size_t per = per_utterance ? (size_t)F * T : n;            // ... of a group (ragged: of the longest)
    for (DevArray<float2>& k : ode_k_) grow(k, n * 8);
    grow(ode_xs_, n * 8);
    grow(ode_table_, sizeof(double) * G * ODE_ROWS * ODE_STRIDE);
    grow(ode_partial_, sizeof(double) * G * ODE_NBLK * ODE_NSUM);
    grow(ode_result_, sizeof(double) * G * ODE_NSUM);
    ode_host_.ensure(sizeof(double) * G * ODE_NSUM);
    ode_ctl_.assign(G, OdeControl());
    ode_rounds_ = ode_wasted_ = 0; nfe_ = 0;
    std::vector<OdeControl>& cs = ode_ctl_;
    std::vector<size_t> goff(G), glen(G);                            // the groups' ranges, in complex elements
    for (int g = 0; g < G; ++g) {
      goff[g] = ragged() ? (size_t)F * rag_prefix(g) : (size_t)g * per;
      glen[g] = ragged() ? (size_t)F * rag_T_[g] : per;
      cs[g].start(oc.t_end, oc.eps, oc.max_step, (double)glen[g]);
    }

    // prior
    const std::vector<float> one_row(SC_STRIDE, 0.f), one_t(1, (float)oc.t_end);
    const unsigned long long* seed_dev = upload_tables(one_row, one_t, std::vector<float>(), seed, B);    // (also consumes the noise-stream ids)
    SG_CHECK(drt::memcpy_d2d(sy_, Y, n * 8, stream_));
    if (x0) SG_CHECK(drt::memcpy_d2d(sx_, x0, n * 8, stream_));
    else draw_prior(noise, seed_dev, oc.std1, n, B, F * T);

    // time-embedding / time / wrapper rows: row = stage * G + group; the network's batch stride over them is 1 row when every
    // utterance is a group and 0 when the batch is one
    const int bs = per_utterance ? 1 : 0;
    FwdCtl ctl{bias_table_, bs * tot_temb_, G * tot_temb_, step_ctr_, tsteps_, bs, G, -1.0f};
    if (oc.coef_fn) { ctl.coef = coef_table_; ctl.coef_bstride = bs; ctl.coef_sstride = G; }
    const long long FT = ragged() ? 1 : (long long)F * T;            // batch stride of x / y (ragged: multiplier of the utterance's offset)
    const unsigned egrid = (unsigned)std::min<size_t>((per / 2 + 255) / 256 + 1, 4096);      // per group
    std::vector<int> sel(G, 0);                                        // host copy of the selectors (kernels_ode.h)
    auto base_args = [&]() {
      OdeEachArgs e{};
      OdeArgs& a = e.a;
      a.y = (const float*)sy_.get(); a.score = (const float*)sscore_.get();
      for (int j = 1; j < 6; ++j) a.k[j] = (const float*)ode_k_[j].get();
      a.table = ode_table_; a.step_ptr = step_ctr_; a.row = -1; a.theta = oc.theta;
      a.atol = oc.atol; a.rtol = oc.rtol; a.partial = ode_partial_; a.result = ode_result_;
      e.xbuf[0] = (float*)sx_.get(); e.xbuf[1] = (float*)sxm_.get(); e.kbuf[0] = (float*)ode_k_[0].get(); e.kbuf[1] = (float*)ode_k_[6].get();
      e.rag_off = rag_off0(); e.per = (long long)per; e.kout_sel = -1;
      return e;
    };
    const size_t tab_doubles = (size_t)G * ODE_ROWS * ODE_STRIDE;
    std::vector<double> table(tab_doubles), times((size_t)ODE_ROWS * G);
    std::vector<float> tf((size_t)ODE_ROWS * G), cf((size_t)ODE_ROWS * G * 4), ga((size_t)ODE_ROWS * G), al(ga.size()), be(ga.size());
    // one round's table (rows 0..6 of the active groups filled by the caller; row 7 = selector, active flag), nt * G stage times
    // (times[e * G + g]) and wrapper rows -> device through the pinned staging buffer; time embedding rows; step counter to row 0
    auto upload = [&](int nt, const std::vector<char>& active) {
      const int rows = nt * G;
      for (int g = 0; g < G; ++g) {
        double* tb = &table[(size_t)g * ODE_ROWS * ODE_STRIDE];
        for (int e = 0; e < nt; ++e) { tf[(size_t)e * G + g] = (float)times[(size_t)e * G + g]; tb[e * ODE_STRIDE] = ode_g2half(oc, tf[(size_t)e * G + g]); }
        tb[ODE_ROW_STATE * ODE_STRIDE] = (double)sel[g]; tb[ODE_ROW_STATE * ODE_STRIDE + 1] = active[g] ? 1.0 : 0.0;
      }
      if (oc.coef_fn) {
        oc.coef_fn(oc.coef_user, rows, tf.data(), ga.data(), al.data(), be.data());
        for (int r = 0; r < rows; ++r) {
          SG_REQUIRE(std::isfinite(ga[r]) && std::isfinite(al[r]) && std::isfinite(be[r]), who + ": the score-wrapper callback returned a non-finite coefficient");
          cf[4 * (size_t)r] = ga[r]; cf[4 * (size_t)r + 1] = al[r]; cf[4 * (size_t)r + 2] = be[r]; cf[4 * (size_t)r + 3] = 0.f;
        }
      }
      const size_t nb_tab = sizeof(double) * tab_doubles, nb_t = sizeof(float) * rows, nb_c = sizeof(float) * 4 * rows;
      char* hs = stage_.acquire(nb_tab + nb_t + nb_c);
      memcpy(hs, table.data(), nb_tab); memcpy(hs + nb_tab, tf.data(), nb_t); memcpy(hs + nb_tab + nb_t, cf.data(), nb_c);
      SG_CHECK(drt::memcpy_h2d(ode_table_, hs, nb_tab, stream_));
      SG_CHECK(drt::memcpy_h2d(tsteps_, hs + nb_tab, nb_t, stream_));
      if (oc.coef_fn) SG_CHECK(drt::memcpy_h2d(coef_table_, hs + nb_tab + nb_t, nb_c, stream_));
      stage_.commit(stream_);
      compute_temb(tsteps_, rows);
      DRT_LAUNCH(step_set_kernel, dim3(1), dim3(64), stream_, step_ctr_.get(), 0);
    };
    auto evaluate = [&](const float2* at) {      // one batch evaluation at the step counter's time rows
      arena_.reset();
      run_forward(at, FT, sy_, FT, sscore_, B, F, T, ctl);
      ++nfe_;
    };
    auto read_sums = [&]() {                     // second stage of a reduction + the one transfer of a round: G x ODE_NSUM doubles
      DRT_LAUNCH(ode_reduce_final_each_kernel, dim3(G), dim3(64), stream_, (const double*)ode_table_, (const double*)ode_partial_, ode_result_.get());
      SG_CHECK(drt::memcpy_d2h(ode_host_, ode_result_, sizeof(double) * G * ODE_NSUM, stream_));
      SG_CHECK(drt::stream_sync(stream_));
      check_launch();
    };
    const auto subject = [&](int g) { return who + (per_utterance ? ": utterance " + std::to_string(g) : std::string(": the solver")); };
    auto count = [&](int g, int k) {             // checked before the evaluations run
      SG_REQUIRE(cs[g].nfe + k <= oc.max_nfe, subject(g) + " needs more than max_nfe = " + std::to_string(oc.max_nfe) + " evaluations (t = " +
                 std::to_string(cs[g].last_time(oc.t_end)) + ")");
      cs[g].nfe += k;
    };
    const dim3 sgrid(egrid, G), rgrid(ODE_NBLK, G);
    std::vector<char> active(G, 1);

    // f0 = f(t0, y0): every selector is 0, the state of the whole batch is sx_
    for (int g = 0; g < G; ++g) count(g, 1);
    std::fill(table.begin(), table.end(), 0.0);
    for (int g = 0; g < G; ++g) times[g] = oc.t_end;
    upload(1, active);
    evaluate(sx_);
    { OdeEachArgs e = base_args(); e.kout_sel = 0; e.a.self = 0; DRT_LAUNCH(ode_stage_each_kernel, sgrid, dim3(256), stream_, e); }

    if (oc.first_step > 0) {
      for (int g = 0; g < G; ++g) cs[g].h_abs = oc.first_step;
    } else {      // select_initial_step, per group: the probe evaluation at the group's own t0 + h0
      for (int g = 0; g < G; ++g) count(g, 1);
      { OdeEachArgs e = base_args(); e.d2 = 0; DRT_LAUNCH(ode_init_norms_each_kernel, rgrid, dim3(256), stream_, e); }
      read_sums();
      std::fill(table.begin(), table.end(), 0.0);
      for (int g = 0; g < G; ++g) {
        const double h0 = cs[g].probe_step(ode_host_[g * ODE_NSUM], ode_host_[g * ODE_NSUM + 1]);
        table[((size_t)g * ODE_ROWS + 6) * ODE_STRIDE + 1] = h0 * cs[g].dir;
        times[g] = cs[g].t + h0 * cs[g].dir;
      }
      upload(1, active);
      { OdeEachArgs e = base_args(); e.a.row = 6; e.a.nterms = 1; e.a.xnext = (float*)ode_xs_.get(); DRT_LAUNCH(ode_stage_each_kernel, sgrid, dim3(256), stream_, e); }
      evaluate(ode_xs_);
      { OdeEachArgs e = base_args(); e.a.xs = (const float*)ode_xs_.get(); e.kout_sel = 6; e.a.self = 6; DRT_LAUNCH(ode_stage_each_kernel, sgrid, dim3(256), stream_, e); }
      { OdeEachArgs e = base_args(); e.d2 = 1; DRT_LAUNCH(ode_init_norms_each_kernel, rgrid, dim3(256), stream_, e); }
      read_sums();
      for (int g = 0; g < G; ++g) cs[g].first_step_from_probe(ode_host_[g * ODE_NSUM + 1]);
    }

    for (;;) {
      int nactive = 0;
      for (int g = 0; g < G; ++g) { active[g] = cs[g].done() ? 0 : 1; nactive += active[g]; }
      if (!nactive) break;
      // ---- one round: an attempted step of every unfinished group; six batch evaluations, G scalars back
      std::fill(table.begin(), table.end(), 0.0);
      for (int g = 0; g < G; ++g) {
        if (!active[g]) { for (int e = 0; e < 6; ++e) times[(size_t)e * G + g] = cs[g].t; continue; }      // (frozen: any valid time)
        SG_REQUIRE(cs[g].begin_attempt(), (per_utterance ? subject(g) : who) + ": required step size is less than spacing between numbers (t = " +
                   std::to_string(cs[g].t) + ")");
        count(g, 6);
        double tm[6];
        cs[g].fill_attempt(tm, &table[(size_t)g * ODE_ROWS * ODE_STRIDE], ODE_STRIDE);
        for (int e = 0; e < 6; ++e) times[(size_t)e * G + g] = tm[e];
      }
      ++ode_rounds_; ode_wasted_ += 6 * (G - nactive);
      upload(6, active);
      { OdeEachArgs e = base_args(); e.a.row = 6; e.a.nterms = 1; e.a.xnext = (float*)ode_xs_.get(); DRT_LAUNCH(ode_stage_each_kernel, sgrid, dim3(256), stream_, e); }
      for (int st = 0; st < 5; ++st) {
        evaluate(ode_xs_);
        OdeEachArgs e = base_args();
        e.a.xs = (const float*)ode_xs_.get(); e.a.kout = (float*)ode_k_[st + 1].get(); e.a.self = st + 1; e.a.nterms = st + 2;
        e.a.xnext = (float*)ode_xs_.get();              // (in place: each thread reads its elements before it writes them)
        e.to_new_state = st == 4 ? 1 : 0;         // y_new: to the stage-input buffer for the network AND to the group's other state buffer
        DRT_LAUNCH(ode_stage_each_kernel, sgrid, dim3(256), stream_, e);
        DRT_LAUNCH(step_inc_kernel, dim3(1), dim3(64), stream_, step_ctr_.get());
      }
      evaluate(ode_xs_);
      { OdeEachArgs e = base_args(); DRT_LAUNCH(ode_error_each_kernel, rgrid, dim3(256), stream_, e); }
      read_sums();
      for (int g = 0; g < G; ++g)
        if (active[g] && cs[g].finish_attempt(ode_host_[g * ODE_NSUM])) sel[g] ^= 1;      // first same as last
    }
    for (int g = 0; g < G; ++g) SG_CHECK(drt::memcpy_d2d(out + goff[g], (sel[g] ? sxm_ : sx_) + goff[g], glen[g] * 8, stream_));
  }
  // group b of the last ode_run (per-utterance control: utterance b; batch control: b = 0, the batch)
  void ode_stats_each(int b, int* nfe, int* accepted, int* rejected, double* t_accepted, int cap, int* rounds, int* wasted) const {
    SG_REQUIRE(b >= 0 && b < (int)ode_ctl_.size(), "ode_stats_each: no such utterance in the last run");
    const OdeControl& c = ode_ctl_[b];
    if (nfe) *nfe = c.nfe;
    if (accepted) *accepted = c.n_accepted;
    if (rejected) *rejected = c.n_rejected;
    for (int i = 0; t_accepted && i < cap && i < (int)c.t_accepted.size(); ++i) t_accepted[i] = c.t_accepted[i];
    if (rounds) *rounds = ode_rounds_;
    if (wasted) *wasted = ode_wasted_;
  }
  size_t rag_prefix(int b) const { size_t s = 0; for (int i = 0; i < b; ++i) s += (size_t)rag_T_[i]; return s; }      // frames before utterance b
  void ode_stats(int* accepted, int* rejected, double* t_accepted, int cap) const {      // group 0 of the last ode_run
    if (!ode_ctl_.empty()) ode_stats_each(0, nullptr, accepted, rejected, t_accepted, cap, nullptr, nullptr);
    else { if (accepted) *accepted = 0; if (rejected) *rejected = 0; }
  }
  void set_noise_streams(const unsigned long long* ids, int n) { streams_next_.assign(ids, ids + n); }
  void set_noise_frames(const int* first, const int* total, int n) {
    frames_next_.assign(first, first + n);
    frames_next_.insert(frames_next_.end(), total, total + n);
  }
  // The noise geometry of the sampler call `who` over B utterances of T frames (ragged: the frame table's) -> geom_call_, which
  // upload_tables puts behind the stream ids.  A pending table of B entries is consumed and checked -- a refusal also drops the
  // pending stream ids, which belonged to the same call --, one of another size is dropped like stream ids of another size.
  void take_noise_frames(const std::string& who, int B, int T, const float2* noise) {
    std::vector<int> g;
    g.swap(frames_next_);
    geom_call_.clear();
    if ((int)g.size() != 2 * B) return;
    std::string bad;
    if (noise) bad = who + ": a noise geometry (sgmse_set_noise_frames) applies to in-kernel noise, not to replayed noise";
    for (int b = 0; b < B && bad.empty(); ++b) {
      const int Tb = ragged() ? rag_T_[b] : T;
      const long long first = g[b], total = g[B + b];
      if (first < 0 || first + Tb > total)
        bad = who + ": utterance " + std::to_string(b) + ": noise frames [" + std::to_string(first) + ", " + std::to_string(first + Tb) +
              ") do not lie inside the recording's [0, " + std::to_string(total) + ")";
      geom_call_.insert(geom_call_.end(), {g[b], g[B + b], Tb});
    }
    if (!bad.empty()) { geom_call_.clear(); streams_next_.clear(); throw EngineArgError(bad); }
  }
  void set_ragged_frames(const int* frames, int n) { set_frames(frames, n); }     // sgmse_set_frames

  // ---- windowed score (sgmse_set_windows): ONE reverse process over a long recording, only the network runs on windows ------------
  // With a plan in force pc_sample / sb_sample take B = 1, T = K and keep their state (sx_, sxm_, sy_, sscore_) at F * K elements,
  // K any length; every score evaluation (eval_score) cuts the current state into the plan's n windows of W frames, runs the network
  // on them in C = ceil(n / max_batch) chunks of Bc = ceil(n / C) windows and blends the windows' scores into the recording's
  // (window_gather_kernel / window_blend_kernel).  The up to C - 1 empty slots of the last chunk evaluate its last window again
  // (their scores are not blended), so the network runs at ONE shape and the whole step is one captured graph.  Sticky like
  // set_frames; n = 0 withdraws the plan.  The plan's serial number is part of the captured step's key: the same plan given again
  // (also after a withdrawal) keeps it.
  static std::string window_plan_error(int K, int W, const int* start, int n) {
    if (K < 1 || W < 1 || n < 1 || !start) return "a window plan needs K >= 1, W >= 1 and n >= 1 starts";
    if (n > 32767) return "more than 32767 windows";      // (grid.z of the gather: up to C * Bc < 2 n slots)
    for (int j = 0; j < n; ++j) {
      if (start[j] < 0 || (long long)start[j] + W > K) return "window " + std::to_string(j) + " does not lie inside [0, K)";
      if (j > 0 && start[j] <= start[j - 1]) return "window starts must be strictly increasing";
      if (j == 0 ? start[0] != 0 : start[j] > start[j - 1] + W) return "the windows leave a gap: they must cover [0, K)";
      if (j > 2 && start[j] < start[j - 3] + W) return "a frame lies under four windows";
    }
    if (start[n - 1] + W != K) return "the windows leave a gap: they must cover [0, K)";
    return "";
  }
  void set_windows(int K, int W, const int* start, int n, int max_batch) {
    if (n == 0) { win_on_ = false; return; }
    const std::string bad = window_plan_error(K, W, start, n);
    if (!bad.empty()) throw EngineArgError("set_windows: " + bad);
    if (max_batch < 1) throw EngineArgError("set_windows: max_batch must be >= 1");
    const int down = 1 << (cfg_.n_levels - 1);
    if (W % down) throw EngineArgError("set_windows: W must be a multiple of 2^(levels-1) = " + std::to_string(down) + " (only the windows reach the network)");
    WinPlan p;
    p.K = K; p.W = W; p.n = n; p.max_batch = max_batch; p.start.assign(start, start + n);
    p.C = (n + max_batch - 1) / max_batch; p.Bc = (n + p.C - 1) / p.C;
    if (!p.same(win_)) { p.id = ++win_serial_; win_ = std::move(p); win_dirty_ = true; }
    win_on_ = true;
  }
  bool windowed() const { return win_on_; }
  // the two kernels on their own (sgmse_window_gather / sgmse_window_blend): the plan, checked by the caller, goes up through
  // upload_windows, whose table begins with the n starts (the kernels read nothing behind them)
  void op_window_gather(const float2* src, float2* windows, int F, int K, int W, const int* start, int n) {
    SG_REQUIRE(F <= 65535, "window_gather: more than 65535 rows");
    WinArgs a{src, windows, upload_windows(start, start, n), F, K, W, n};
    DRT_LAUNCH(window_gather_kernel, dim3((W + 255) / 256, F, n), dim3(256), stream_, a);
    check_launch();
  }
  void op_window_blend(const float2* windows, float2* dst, int F, int K, int W, const int* start, int n) {
    SG_REQUIRE(F <= 65535, "window_blend: more than 65535 rows");
    WinArgs a{windows, dst, upload_windows(start, start, n), F, K, W, n};
    DRT_LAUNCH(window_blend_kernel, dim3((K + 255) / 256, F), dim3(256), stream_, a);
    check_launch();
  }
  int last_nfe() const { return nfe_; }
  int graph_captures() const { return graph_captures_; }     // how many times a step was captured + instantiated (tests, bench)
  int graph_updates() const { return graph_updates_; }       // ... captured and applied to the existing executable in place
  int split_mode() const { return split_mode_; }
  bool winograd() const { return split_mode_ == 2 && wino_; }
  size_t arena_bytes() const { return arena_buf_.capacity(); }

  // ---- single ops (op-level C ABI + tests) ------------------------------------------------------------------
  // per-utterance max |x| of one or two NCHW tensors -> [B] (+ [B]) floats, for the op-level entry points
  DevBuf input_bounds(const float* x1, int C1, const float* x2, int C2, int B, int HW) {
    const size_t per = (size_t)B * kAmaxSpread;
    DevBuf buf = fresh(2 * per * 4);
    float* out = buf.as<float>();
    SG_CHECK(drt::memset_dev(out, 0, 2 * per * 4, stream_));
    for (int b = 0; b < B; ++b) {
      const size_t n1 = (size_t)C1 * HW;
      DRT_LAUNCH(absmax_kernel, dim3((unsigned)std::min<size_t>((n1 + 255) / 256, 1024)), dim3(256), stream_, x1 + b * n1, n1,
                 out + (size_t)b * kAmaxSpread);
      if (x2) {
        const size_t n2 = (size_t)C2 * HW;
        DRT_LAUNCH(absmax_kernel, dim3((unsigned)std::min<size_t>((n2 + 255) / 256, 1024)), dim3(256), stream_, x2 + b * n2, n2,
                   out + per + (size_t)b * kAmaxSpread);
      }
    }
    return buf;
  }

  // the bound gn_finalize_kernel leaves for an fp16x2 3x3 consumer, for a producer given as explicit coefficients (or none)
  DevBuf producer_bound(const float* in_scale, const float* in_shift, int C, const float* amax1, const float* amax2, int B) {
    DevBuf buf = fresh((size_t)B * kAmaxSpread * 4);
    float* out = buf.as<float>();
    DRT_LAUNCH(xform_bound_kernel, dim3(B), dim3(64), stream_, in_scale, in_shift, C, amax1, amax2, out);
    return buf;
  }

  // ---- stand-alone convolution launches (op_conv2d, bench_conv): what Engine::conv() takes from the layer and from the forward,
  // made on the spot from OIHW weights and the input tensors
  struct ConvPack { enum Kind { Mfma, Thin, Split, Wino } kind; int smode = 0; WinoForm form = WinoForm::F23; int co_t = 0; };
  // the launch arguments and the scratch behind their pointers.  Declare it in front of the launch: its scope then ends behind the
  // stream synchronisation that follows the launch.  (When an exception unwinds it earlier the buffers are freed with work still
  // queued; that is sound, freeing device memory waits for the device.  The same holds for every scoped DevBuf of this file.)
  struct StandaloneConv { ConvArgs a{}; DevBuf packed, bounds, xbound; };
  // a0: sources, shape and fused producer.  Packs the weights for the family; for the fp16x2 families (dynamic input scale) also
  // computes the range bounds as the producers of the forward would have left them.
  StandaloneConv standalone_conv(const ConvArgs& a0, const ConvPack& f, const float* w_oihw, int ks) {
    StandaloneConv s;
    ConvArgs& a = s.a = a0;
    const int Cin = a.C1 + a.C2;
    switch (f.kind) {
      case ConvPack::Mfma: s.packed = pack_mfma(oihw_sources(w_oihw, ks, Cin, a.Cout), f.co_t); break;
      case ConvPack::Thin: s.packed = pack_thin(w_oihw, Cin, a.Cout); break;
      case ConvPack::Split: s.packed = pack_split(w_oihw, ks, Cin, a.Cout, f.smode, &a.co_scale); break;
      case ConvPack::Wino: s.packed = pack_wino(f.form, w_oihw, Cin, a.Cout, &a.co_scale); break;      // (all Winograd forms are fp16x2)
    }
    a.w = s.packed.as<float>();
    if (f.kind == ConvPack::Wino || (f.kind == ConvPack::Split && f.smode == 2)) {
      s.bounds = input_bounds(a.src1, a.C1, a.src2, a.C2, a.B, a.H * a.W);
      const float* am1 = s.bounds.as<float>();
      const float* am2 = a.src2 ? am1 + (size_t)a.B * kAmaxSpread : nullptr;
      if (ks == 1 && a.in_scale == nullptr) bind_bounds(a, 1, nullptr, am1, am2);      // raw input, as the network's shortcuts run it
      else {      // a fused producer: the kernel scales by the bound of the producer's output (1x1: in the place of the raw range)
        s.xbound = producer_bound(a.in_scale, a.in_shift, Cin, am1, am2, a.B);
        bind_bounds(a, ks, s.xbound.as<float>(), s.xbound.as<float>(), nullptr);
      }
    }
    return s;
  }
  // where an fp16x2 launch reads its input range: a 3x3 kernel from the bound of its (fused producer's) input, a 1x1 kernel from the
  // range bounds of its sources
  static void bind_bounds(ConvArgs& ca, int ks, const float* xbound, const float* amax1, const float* amax2) {
    if (ks == 3) ca.xbound = xbound;
    else { ca.amax1 = amax1; ca.amax2 = amax2; }
  }

  // the `force_direct` argument of sgmse_op_conv2d (include/sgmse_hip.h); sgmse_amd/ops.py maps its force_split names to these values
  enum ForceConv { FC_AUTO = 0, FC_DIRECT = 1, FC_SPLIT_B3 = 2, FC_SPLIT_H2 = 3, FC_WINO = 4, FC_WINO_4ROW = 5, FC_THIN = 6, FC_WINO2D = 7,
                   FC_WINO43 = 8, FC_WINO43_4ROW = 9 };
  void op_conv2d(const float* x, const float* w_oihw, const float* bias, const float* res, float* out, int B, int Cin,
                 int Cout, int H, int W, int ks, float out_scale, int force_direct, const float* in_scale,
                 const float* in_shift, int in_act, const float* x2, int C2) {
    ConvArgs a{};
    a.src1 = x; a.src2 = x2; a.C1 = Cin - C2; a.C2 = C2; a.bias = bias; a.res = res; a.out_scale = out_scale; a.out = out;
    a.Cout = Cout; a.B = B; a.H = H; a.W = W; a.in_scale = in_scale; a.in_shift = in_shift; a.in_act = in_act;
    ConvPlan pl = choose_conv_plan(ks, Cin, Cout, H, W);
    const bool wino = force_direct == FC_WINO || force_direct == FC_WINO_4ROW || force_direct == FC_WINO2D || force_direct == FC_WINO43 || force_direct == FC_WINO43_4ROW;
    StandaloneConv s;      // (of whichever launch follows; released at the end of the function, behind the synchronisations)
    if (force_direct == FC_THIN) {                         // exact-fp32 VALU kernel of the C -> 4 pyramid convolutions
      SG_REQUIRE(conv_thin_eligible(ks, a.C1, C2, Cout), "op_conv2d: shape is not eligible for the thin-output kernel");
      s = standalone_conv(a, ConvPack{ConvPack::Thin}, w_oihw, ks);
      launch_conv_thin(s.a, stream_);
      SG_CHECK(drt::stream_sync(stream_));
    } else if (wino || force_direct == FC_SPLIT_B3 || force_direct == FC_SPLIT_H2) {      // the Winograd x fp16x2 forms and the split kernels
      const WinoForm form = force_direct == FC_WINO2D ? WinoForm::F2x2 : force_direct >= FC_WINO43 ? WinoForm::F43 : WinoForm::F23;
      const int smode = wino ? 2 : force_direct - 1;       // (all Winograd forms are fp16x2)
      if (!wino) SG_REQUIRE(conv_split_eligible(ks, a.C1, C2, Cout) || conv_thin_split_eligible(ks, a.C1, C2, Cout), "op_conv2d: shape is not eligible for the split kernels");
      else if (form == WinoForm::F43) SG_REQUIRE(ks == 3 && conv_wino43_eligible(a.C1, C2, Cout, W) && conv_wino43_aligned(a), "op_conv2d: shape is not eligible for the Winograd F(4,3) kernel");
      else SG_REQUIRE(ks == 3 && conv_wino_eligible(a.C1, C2, Cout, W), form == WinoForm::F2x2 ? "op_conv2d: shape is not eligible for the 2-D Winograd kernel" : "op_conv2d: shape is not eligible for the Winograd kernel");
      s = standalone_conv(a, wino ? ConvPack{ConvPack::Wino, smode, form} : ConvPack{ConvPack::Split, smode}, w_oihw, ks);
      if (wino) launch_conv_wino(form, s.a, stream_, force_direct == FC_WINO_4ROW || force_direct == FC_WINO43_4ROW);
      else launch_conv_split(s.a, ks, smode, stream_);
      SG_CHECK(drt::stream_sync(stream_));
    } else if (pl.mfma && !force_direct && (C2 == 0 || a.C1 % ((ks == 3) ? 8 : 32) == 0)) {
      s = standalone_conv(a, ConvPack{ConvPack::Mfma, 0, WinoForm::F23, pl.co_t}, w_oihw, ks);
      launch_conv_mfma(s.a, ks, pl, stream_);
      SG_CHECK(drt::stream_sync(stream_));
    } else {
      a.w = w_oihw;
      launch_conv_direct(a, ks, stream_);
    }
    check_launch();
  }

  void op_groupnorm(const float* x, const float* gamma, const float* beta, float* out, int B, int C, int H, int W, int act,
                    const float* x2, int C2) {
    const int HW = H * W, C1 = C - C2;
    const DevBuf stats_buf = fresh((size_t)B * C * 2 * 4), sc_buf = fresh((size_t)B * C * 4), sh_buf = fresh((size_t)B * C * 4);
    float *stats = stats_buf.as<float>(), *sc = sc_buf.as<float>(), *sh = sh_buf.as<float>();
    float* stats2 = stats + (size_t)B * C1 * 2;
    DRT_LAUNCH(gn_chan_stats_kernel, dim3(B * C1), dim3(256), stream_, x, (const float*)nullptr, C1, 0, HW, stats, Rag{nullptr, nullptr, nullptr}, 0);
    if (C2) DRT_LAUNCH(gn_chan_stats_kernel, dim3(B * C2), dim3(256), stream_, x2, (const float*)nullptr, C2, 0, HW, stats2, Rag{nullptr, nullptr, nullptr}, 0);
    const int G = std::min(C / 4, 32);
    const GnFin f{stats, stats2, nullptr, nullptr, gamma, beta, sc, sh, nullptr, Rag{nullptr, nullptr, nullptr}, C1, 1, 1, C2, 1, 1, G, HW, 0, 1e-6f};
    DRT_LAUNCH(gn_finalize_kernel, dim3(G, B), dim3(256), stream_, f);
    DRT_LAUNCH(gn_apply_kernel, dim3((HW + 1023) / 1024, B * C), dim3(256), stream_, x, x2, C1, C2, HW, (const float*)sc,
               (const float*)sh, act, out);
    SG_CHECK(drt::stream_sync(stream_));
    check_launch();
  }

  void op_fir(const float* x, float* out, int BC, int H, int W, int up, const float* in_scale, const float* in_shift, int in_act,
              float* out_raw) {
    FirArgs fa{x, out, in_scale, in_shift, in_act, BC, H, W, out_raw, 1, Rag{nullptr, nullptr, nullptr}};
    launch_fir(fa, up);
    check_launch();
  }

  // dtype: 0 float, 1 double, 2 half (the element types of the reference op, op/upfirdn2d_kernel.cu:311)
  void op_upfirdn2d(int dtype, const void* x, const void* kern, void* out, int BC, int H, int W, int kh, int kw, int up_x, int up_y,
                    int down_x, int down_y, int px0, int px1, int py0, int py1) {
    UpfirdnArgs a{x, kern, out, BC, H, W, kh, kw, up_x, up_y, down_x, down_y, px0, px1, py0, py1, 0, 0};
    a.Ho = (H * up_y + py0 + py1 - kh) / down_y + 1;
    a.Wo = (W * up_x + px0 + px1 - kw) / down_x + 1;
    SG_REQUIRE(a.Ho > 0 && a.Wo > 0, "upfirdn2d: empty output");
    const dim3 grid((a.Ho * a.Wo + 255) / 256, BC);
    if (dtype == 0) DRT_LAUNCH(upfirdn2d_generic_kernel<UpfirdnF32>, grid, dim3(256), stream_, a);
    else if (dtype == 1) DRT_LAUNCH(upfirdn2d_generic_kernel<UpfirdnF64>, grid, dim3(256), stream_, a);
    else DRT_LAUNCH(upfirdn2d_generic_kernel<UpfirdnF16>, grid, dim3(256), stream_, a);
    check_launch();
  }

  void op_attention(const float* qkv, float* out, int B, int C, int S) {
    AttnArgs a{qkv, out, B, C, S, 1.0f / sqrtf((float)C), Rag{nullptr, nullptr, nullptr}, 0};
    SG_REQUIRE(launch_attn_core(a, stream_), "attention: C must be one of " + attn_widths_text());
    check_launch();
  }

  void op_stft(const float* sig, const float* window, float2* spec, int B, int L, int n_fft, int hop) {
    SG_REQUIRE(n_fft <= kMaxNfft && n_fft >= 2 && hop >= 1 && L > n_fft / 2, "stft: unsupported geometry");
    const float2* tw = twiddle(n_fft);
    StftArgs a{sig, window, tw, spec, L, n_fft, hop, n_fft / 2 + 1, (L + 2 * (n_fft / 2) - n_fft) / hop + 1};
    DRT_LAUNCH(stft_kernel, dim3(a.K, B), dim3(256), stream_, a);
    check_launch();
  }

  void op_istft(const float2* spec, const float* window, float* out, int B, int K, int n_fft, int hop, int length) {
    SG_REQUIRE(n_fft <= kMaxNfft && n_fft >= 2 && hop >= 1, "istft: unsupported geometry");
    SG_REQUIRE(K >= 1 && length >= 1 && length + n_fft / 2 <= n_fft + hop * (K - 1), "istft: length exceeds the overlap-add span");
    const float2* tw = twiddle(n_fft);
    IstftArgs a{spec, window, tw, out, n_fft, hop, n_fft / 2 + 1, K, length};
    DRT_LAUNCH(istft_kernel, dim3((length + 255) / 256, B), dim3(256), stream_, a);
    check_launch();
  }

  void op_spec_xform(const float2* in, float2* out, size_t n, int type, float factor, float exponent, int inverse) {
    SpecXformArgs a{in, out, n, type, factor, exponent, inverse};
    DRT_LAUNCH(spec_xform_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), stream_, a);
    check_launch();
  }

  // Windows of a long spectrogram (kernels_stft.h: spec_split_kernel / spec_merge_kernel).  The plan -- checked by the caller
  // (capi.h: sg_check_windows) -- goes to the device as start | frames | col0 through the staging buffer.
  const int* upload_windows(const int* start, const int* frames, int n) {
    const size_t nb = (size_t)3 * n * sizeof(int);
    grow(win_tab_, nb);
    int* h = reinterpret_cast<int*>(stage_.acquire(nb));
    int col = 0;
    for (int j = 0; j < n; ++j) { h[j] = start[j]; h[n + j] = frames[j]; h[2 * n + j] = col; col += frames[j]; }
    SG_CHECK(drt::memcpy_h2d(win_tab_, h, nb, stream_));
    stage_.commit(stream_);
    return win_tab_.get();
  }

  void op_spec_split(const float2* spec, float2* windows, int F, int K, const int* start, const int* frames, int n, int type, float factor,
                     float exponent) {
    SG_REQUIRE(n <= 65535 && F <= 65535, "spec_split: more than 65535 windows or rows");
    SpecWinArgs a{spec, windows, upload_windows(start, frames, n), F, K, n, type, factor, exponent};
    const int tmax = *std::max_element(frames, frames + n);
    DRT_LAUNCH(spec_split_kernel, dim3((tmax + 255) / 256, F, n), dim3(256), stream_, a);
    check_launch();
  }

  void op_spec_merge(const float2* windows, float2* spec, int F, int K, const int* start, const int* frames, int n, int type, float factor,
                     float exponent) {
    SG_REQUIRE(F <= 65535, "spec_merge: more than 65535 rows");
    SpecWinArgs a{windows, spec, upload_windows(start, frames, n), F, K, n, type, factor, exponent};
    DRT_LAUNCH(spec_merge_kernel, dim3((K + 255) / 256, F), dim3(256), stream_, a);
    check_launch();
  }

  void sync() { SG_CHECK(drt::stream_sync(stream_)); }

  // Kernel micro-benchmark of one MFMA convolution shape on random operands: `iters` back-to-back launches between two
  // events on this stream.  variant = SGMSE_CONV_VARIANT encoding (-1: process default).  Returns ms per launch.
  float bench_conv(int ks, int B, int Cin, int Cout, int H, int W, int variant, int iters, int fused) {
    ConvPlan pl = choose_conv_plan(ks, Cin, Cout, H, W);
    SG_REQUIRE(pl.mfma, "bench_conv: shape is not MFMA-eligible");
    if (variant >= 0 && (variant & 512)) { pl.rows = 4; variant &= ~512; }   // measurement knob: 128 co x 128 px tile
    int ablate = 0, abl_split = 0;
    bool split_rows4 = false, wino43 = false;
    if (variant >= 0) {
      split_rows4 = (variant >> 23) & 1;         // measurement knob: 4-row workgroup shape of the split 3x3 kernel
      wino43 = (variant >> 22) & 1;              // with bit 10: the F(4,3) form of the Winograd kernel (kernels_conv_wino43.h)
      abl_split = (variant >> 12) & 1023;        // measurement knob: compile-time variant of the split 3x3 kernel, bits 12..21
      if (!(variant & (64 | 128))) { ablate = abl_split & 15; abl_split = 0; }   // fp32 kernels: run-time ablation bits 12..15
      variant &= 4095;
    }
    const bool wino = variant >= 0 && (variant & 1024);          // measurement: the Winograd F(2,3) x fp16x2 kernel (bit 23: its 4-row shape)
    const bool wino2d = variant >= 0 && (variant & 2048) && !wino;   // ... the 2-D F(2x2,3x3) x fp16x2 kernel (ablation bits 12..: 8 / 16)
    const int smode = variant < 0 ? 0 : ((variant & 128) ? 2 : ((variant & 64) ? 1 : 0));
    const bool b3 = smode != 0 && !wino && !wino2d;
    SG_REQUIRE(!(wino || wino2d) || (ks == 3 && conv_wino_eligible(Cin, 0, Cout, W)), "bench_conv: shape is not eligible for the Winograd kernel");
    SG_REQUIRE(!b3 || conv_split_eligible(ks, Cin, 0, Cout), "bench_conv: shape is not eligible for the split kernels");
    wino43 = wino43 && wino;
    SG_REQUIRE(!wino43 || conv_wino43_eligible(Cin, 0, Cout, W), "bench_conv: shape is not eligible for the Winograd F(4,3) kernel");
    const WinoForm wform = wino2d ? WinoForm::F2x2 : wino43 ? WinoForm::F43 : WinoForm::F23;
    const size_t nx = (size_t)B * Cin * H * W, no = (size_t)B * Cout * H * W, nw = (size_t)Cout * Cin * ks * ks;
    const DevBuf x_buf = fresh(nx * 4), o_buf = fresh(no * 4), r_buf = fresh(no * 4), w_buf = fresh(nw * 4), sc_buf = fresh((size_t)B * Cin * 8);
    float *x = x_buf.as<float>(), *o = o_buf.as<float>(), *r = r_buf.as<float>(), *w = w_buf.as<float>(), *sc = sc_buf.as<float>();
    auto fill = [&](float* d, size_t n, uint32_t seed) {
      DRT_LAUNCH(fill_random_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), stream_, d, n, seed);
    };
    fill(x, nx, 1); fill(r, no, 2); fill(w, nw, 3); fill(sc, (size_t)B * Cin * 2, 4);
    ConvArgs a0{};
    a0.src1 = x; a0.C1 = Cin; a0.out = o; a0.Cout = Cout; a0.B = B; a0.H = H; a0.W = W; a0.out_scale = 1.f;
    a0.ablate = ablate;
    if (fused) { a0.in_scale = sc; a0.in_shift = sc + (size_t)B * Cin; a0.in_act = 1; a0.res = r; a0.bias = w; a0.out_scale = 0.70710678f; }
    if (b3 && smode == 2 && ks == 1) { a0.in_scale = nullptr; a0.in_shift = nullptr; a0.in_act = 0; }     // raw input, as in the network's shortcut layers
    EventTimer timer;
    StandaloneConv s = standalone_conv(a0, b3 ? ConvPack{ConvPack::Split, smode} : (wino || wino2d) ? ConvPack{ConvPack::Wino, 2, wform}
                                                                               : ConvPack{ConvPack::Mfma, 0, WinoForm::F23, pl.co_t}, w, ks);
    ConvArgs& a = s.a;
    DevBuf trace_buf;
    unsigned long long* trace_dev = nullptr;
    const size_t n_wg = (size_t)B * ((H + 7) / 8) * ((W + 31) / 32) * ((Cout + 127) / 128);
    if (abl_split & 64) {
      trace_buf = fresh(n_wg * 256);      // (16 words per workgroup; the Winograd kernel's trace: 32)
      trace_dev = trace_buf.as<unsigned long long>();
      SG_CHECK(drt::memset_dev(trace_dev, 0, n_wg * 256, stream_));
      a.trace = trace_dev;
    }
    auto go = [&]() {
      if (wino || wino2d) launch_conv_wino(wform, a, stream_, split_rows4, (abl_split & 64) != 0, abl_split & 63);
      else if (b3) launch_conv_split(a, ks, smode, stream_, split_rows4, abl_split);
      else launch_conv_mfma(a, ks, pl, stream_, variant);
    };
    for (int i = 0; i < 2; ++i) go();
    timer.start(stream_);
    for (int i = 0; i < iters; ++i) go();
    const float ms = timer.stop_ms(stream_) / (float)iters;
    check_launch();
    if (trace_dev) {                    // phase time stamps of the LAST launch -> $SGMSE_TRACE_OUT (binary: 16 x u64 per workgroup)
      const size_t words = wino ? 32 : 16;
      std::vector<unsigned long long> h(n_wg * words);
      SG_CHECK(drt::memcpy_d2h(h.data(), trace_dev, n_wg * words * 8, stream_));
      SG_CHECK(drt::stream_sync(stream_));
      if (const char* path = getenv("SGMSE_TRACE_OUT")) { if (FILE* f = fopen(path, "wb")) { fwrite(h.data(), 8, h.size(), f); fclose(f); } }
    }
    return ms;
  }

  // Measurement only: one launch of a known-size stream (calib_stream_kernel) for the counter calibration of tools/gpu_visit.sh
  // STEPS=pmcbench.  mode 0 = read, 1 = write; bytes_per_lane 8 or 16.  Returns ms of the launch.
  float calib_stream(int mode, int bytes_per_lane, size_t total_bytes) {
    SG_REQUIRE((bytes_per_lane == 8 || bytes_per_lane == 16) && (mode == 0 || mode == 1) && total_bytes >= 4096, "calib_stream: bad arguments");
    const DevBuf scratch = fresh(total_bytes + 256);
    float* buf = scratch.as<float>();
    SG_CHECK(drt::memset_dev(buf, 0, total_bytes + 256, stream_));
    const size_t nvec = total_bytes / (size_t)bytes_per_lane;
    EventTimer timer;
    timer.start(stream_);
    const dim3 g(256 * 16), b(256);
    float* sink = buf + total_bytes / 4;
    if (bytes_per_lane == 8) { if (mode) DRT_LAUNCH((calib_stream_kernel<2, 1>), g, b, stream_, buf, nvec, sink); else DRT_LAUNCH((calib_stream_kernel<2, 0>), g, b, stream_, buf, nvec, sink); }
    else { if (mode) DRT_LAUNCH((calib_stream_kernel<4, 1>), g, b, stream_, buf, nvec, sink); else DRT_LAUNCH((calib_stream_kernel<4, 0>), g, b, stream_, buf, nvec, sink); }
    const float ms = timer.stop_ms(stream_);
    check_launch();
    return ms;
  }

  // per-kernel-class timing of one forward (eager, events on this stream); fills ms per class
  enum { TC_CONV3_BIG = 0, TC_CONV3, TC_CONV1, TC_DIRECT, TC_GN, TC_FIR, TC_ATTN, TC_MISC, TC_COUNT };
  // work[] = algorithmic FLOPs for the conv/attention classes, algorithmic bytes (each operand read once, each result
  // written once) for the HBM-bound classes (groupnorm statistics, FIR, misc)
  void profile_forward(const float2* xy, const float* t_dev, float2* out, int B, int F, int T, float* ms_out, double* work_out,
                       int* launches_out) {
    prof_ = true;
    for (int i = 0; i < TC_COUNT; ++i) { prof_ms_[i] = 0.f; prof_flops_[i] = 0.0; prof_n_[i] = 0; }
    prof_used_ = 0;
    forward_xy(xy, t_dev, out, B, F, T);
    prof_ = false;
    // the event pairs are read after the whole forward has been queued: launches then follow each other as in the replayed graph
    // (with a wait after every launch the device idled between them and each interval carried ~40 us of dispatch: the class times
    // were 4-5 % above the kernel durations rocprofv3 reports for the captured step)
    SG_CHECK(drt::stream_sync(stream_));
    for (size_t i = 0; i < prof_used_; ++i) {
      ProfRec& r = prof_recs_[i];
      if (r.cls < 0) continue;                      // (a tock() without its tick())
      const float ms = drt::event_elapsed_ms(*r.a.get(), *r.b.get());
      prof_ms_[r.cls] += ms;
      prof_flops_[r.cls] += r.work;
      prof_n_[r.cls] += r.launches;
      if (prof_dump_ && r.note[0]) fprintf(stderr, "[sgmse-prof] %s %.4f ms %.1f Gwork/s\n", r.note, ms, r.work / ms * 1e-6);
    }
    for (int i = 0; i < TC_COUNT; ++i) { ms_out[i] = prof_ms_[i]; work_out[i] = prof_flops_[i]; launches_out[i] = prof_n_[i]; }
  }

 private:
  // ---- memory helpers ------------------------------------------------------------------------------------------
  // Every device buffer is a holder (dev_memory.h): a member for what persists (grow / renew), a local for scratch (fresh), an
  // element of wset_ for what belongs to the current weight set (keep).
  // SGMSE_POISON=1 (tests): every allocation, and the activation arena before every forward, is filled with 0xFF bytes (a NaN
  // in every float), so that a kernel reading memory nobody wrote shows up as a NaN in the result instead of depending on
  // what the allocation happened to hold
  bool grow(DevBuf& b, size_t bytes) { return b.ensure(bytes, stream_, poison_); }
  void renew(DevBuf& b, size_t bytes) { b.renew(bytes, stream_, poison_); }
  DevBuf fresh(size_t bytes) { DevBuf b; grow(b, bytes); return b; }
  // the current weight set: released together, behind a stream synchronisation, when new weights are loaded (EMA swap, reload)
  template <class T = float> T* keep(DevBuf b) { wset_.push_back(std::move(b)); return wset_.back().as<T>(); }
  void release_weights() {
    if (wset_.empty()) return;
    drt::stream_sync(stream_);
    wset_.clear();
  }
  void check_launch() { SG_CHECK(drt::last_error()); }
  void require_ready() { SG_REQUIRE(weights_ready_, "weights not loaded (call sgmse_load_weights first)"); }
  // A captured step that no longer matches (new shape, new ragged composition, new weights) is not destroyed but kept as the
  // target of an in-place update by the next capture (capture_step): same launch sequence, other arguments.
  void invalidate_graph() { if (graph_valid_) { graph_valid_ = false; graph_stale_ = true; } }
  void drop_graph() { if (graph_valid_ || graph_stale_) { drt::graph_destroy(&graph_); graph_valid_ = graph_stale_ = false; } }
  template <class Body>
  void capture_step(Body&& body) {
    SG_CHECK(drt::stream_sync(stream_));
    SG_CHECK(drt::graph_begin_capture(stream_));
    capturing_ = true;
    try { body(); } catch (...) {
      // leave the stream usable: end the capture, throw its graph away, and forget the executable a stale update would have reused
      capturing_ = false;
      drt::graph_abort_capture(stream_);
      drop_graph();
      throw;
    }
    capturing_ = false;
    if (graph_stale_) {
      const int r = drt::graph_end_capture_update(stream_, &graph_);
      if (r > 0) { drt::graph_destroy(&graph_); graph_stale_ = false; graph_valid_ = false; SG_CHECK(r); }     // (nothing left to leak or to reuse)
      if (r == 0) ++graph_updates_; else ++graph_captures_;
    } else {
      const int r = drt::graph_end_capture(stream_, &graph_);
      if (r != 0) { drt::graph_destroy(&graph_); graph_valid_ = false; SG_CHECK(r); }
      ++graph_captures_;
    }
    graph_stale_ = false;
    graph_valid_ = true;
  }
  bool graph_stale_ = false, capturing_ = false; int graph_updates_ = 0;

  const float2* twiddle(int n_fft) {
    auto it = twiddles_.find(n_fft);
    if (it != twiddles_.end()) return it->second.get();
    std::vector<float2> h(n_fft);
    for (int m = 0; m < n_fft; ++m) {
      const double ang = 2.0 * 3.14159265358979323846 * (double)m / (double)n_fft;
      h[m] = make_float2((float)cos(ang), (float)sin(ang));
    }
    DevArray<float2> d;
    grow(d, sizeof(float2) * n_fft);
    SG_CHECK(drt::memcpy_h2d(d, h.data(), sizeof(float2) * n_fft, stream_));
    SG_CHECK(drt::stream_sync(stream_));
    return twiddles_.emplace(n_fft, std::move(d)).first->second.get();
  }

  const float* Wp(const std::string& name) const {
    auto it = W_.find(name);
    if (it == W_.end()) throw EngineError("internal: unknown parameter " + name);
    return it->second;
  }

  ConvW make_conv(const std::string& wname, const std::string& bname, int ks, int cin, int cout) {
    return make_conv(Wp(wname), bname.empty() ? nullptr : Wp(bname), ks, cin, cout);
  }
  ConvW make_conv(const float* oihw, const float* bias, int ks, int cin, int cout) {
    ConvW c; c.ks = ks; c.cin = cin; c.cout = cout;
    c.oihw = oihw; c.bias = bias;
    ConvPlan pl = choose_conv_plan(ks, cin, cout, 8, 32);
    if (pl.mfma) {
      c.co_t = pl.co_t;
      const PackArgs pa = oihw_sources(c.oihw, ks, cin, cout);
      c.packed = keep(pack_mfma(pa, pl.co_t));
      if (pl.co_t > 32) c.packed32 = keep(pack_mfma(pa, 32));
    }
    // fp16x2: the input scale is a per-utterance power of two derived at run time -- 3x3 layers from the bound of their GroupNorm
    // producer's output (gn_finalize_kernel), 1x1 layers (raw residual stream) from the producers' range bounds -- the stored
    // factor only undoes the weights'
    if (split_mode_ && (conv_split_eligible(ks, cin, 0, cout) || conv_thin_split_eligible(ks, cin, 0, cout))) {
      c.split_mode = split_mode_;
      c.packed_split = keep(pack_split(c.oihw, ks, cin, cout, c.split_mode, &c.split_scale));
    }
    if (conv_thin_eligible(ks, cin, 0, cout)) c.packed_thin = keep(pack_thin(c.oihw, cin, cout));
    // the wide levels run these layers on a Winograd x fp16x2 kernel (conv_route(): use_wino): F(4,3) along the frame axis, or F(2,3) under SGMSE_WINO43=0
    // (one form per engine, decided here; the channel conditions of the two forms are the same, the width condition is a property of the level: conv_route())
    if (split_mode_ == 2 && wino_ && ks == 3 && conv_wino_eligible(cin, 0, cout, 2)) {
      c.wino_form = (wino43_ && conv_wino43_eligible(cin, 0, cout, 4)) ? WinoForm::F43 : WinoForm::F23;
      c.packed_wino = keep(pack_wino(c.wino_form, c.oihw, cin, cout, &c.wino_scale));
    }
    return c;
  }

  // weights in the fp32 MFMA kernels' layout (pack_weights_kernel) for co_t-channel output tiles; pa names the sources
  static PackArgs oihw_sources(const float* oihw, int ks, int cin, int cout) {
    PackArgs pa{}; pa.src[0] = oihw; pa.nsrc = 1; pa.cout_per_src = cout; pa.io = 0; pa.cin = cin; pa.taps = ks * ks; pa.cout = cout;
    return pa;
  }
  // (the pack_* functions return a fresh buffer: the caller keeps it in the weight set, or holds it as scratch)
  DevBuf pack_mfma(PackArgs pa, int co_t) {
    pa.co_t = co_t; pa.total = packed_weight_elems(pa.taps == 9 ? 3 : 1, pa.cin, pa.cout, co_t);
    DevBuf buf = fresh(pa.total * 4);
    pa.dst = buf.as<float>();
    DRT_LAUNCH(pack_weights_kernel, dim3((unsigned)((pa.total + 255) / 256)), dim3(256), stream_, pa);
    return buf;
  }

  // weights in the fragment order of conv3x3_split_kernel (mode 1: bf16x3, 2: fp16x2 with the layer's power-of-two scale)
  DevBuf pack_split(const float* oihw, int ks, int cin, int cout, int mode, const float** scale_out) {
    const int taps = ks * ks;
    const size_t frags = mode == 2 ? packed_split_frags<SplitH2>(cin, cout, taps) : packed_split_frags<SplitB3>(cin, cout, taps);
    const int cout_pad = (cout + 127) / 128 * 128;
    const size_t bytes = frags * 16 + (size_t)cout_pad * 8;             // [fragments][per-channel inverse scales][scales (packing scratch)]
    DevBuf buf = fresh(bytes);
    uint32_t* pk = buf.as<uint32_t>();
    PackSplitArgs pa{oihw, pk, cin, cout, frags, nullptr, taps};
    const dim3 grid((unsigned)((frags + 255) / 256));
    if (mode == 2) {
      float* inv = reinterpret_cast<float*>(pk) + frags * 4;
      float* sc = inv + cout_pad;
      DRT_LAUNCH(split_co_scale_kernel, dim3((unsigned)((cout_pad + 255) / 256)), dim3(256), stream_, oihw, cin * taps, cout, cout_pad, inv, sc);
      pa.co_scale = sc;
      DRT_LAUNCH(pack_weights_split_kernel<SplitH2>, grid, dim3(256), stream_, pa);
      *scale_out = inv;
    } else {
      DRT_LAUNCH(pack_weights_split_kernel<SplitB3>, grid, dim3(256), stream_, pa);
      *scale_out = nullptr;
    }
    return buf;
  }

  // weights of the C -> 4 layers as [ci][tap][4 co] (conv3x3_thin_kernel)
  DevBuf pack_thin(const float* oihw, int cin, int cout) {
    const size_t ne = packed_thin_elems(cin);
    DevBuf buf = fresh(ne * 4);
    float* pk = buf.as<float>();
    DRT_LAUNCH(pack_weights_thin_kernel, dim3((unsigned)((ne + 255) / 256)), dim3(256), stream_, oihw, pk, cin, cout);
    return buf;
  }
  // weights in the fragment order of the Winograd kernel of `form`: transformed in fp64, scaled per output channel
  DevBuf pack_wino(WinoForm form, const float* oihw, int cin, int cout, const float** scale_out) {
    const bool f43 = form == WinoForm::F43, f2d = form == WinoForm::F2x2;
    const size_t frags = f43 ? packed_wino43_frags(cin, cout) : f2d ? packed_wino2d_frags(cin, cout) : packed_wino_frags(cin, cout);
    const int cout_pad = (cout + 127) / 128 * 128;
    const size_t bytes = (f43 ? packed_wino43_bytes(cin, cout) : f2d ? packed_wino2d_bytes(cin, cout) : packed_wino_bytes(cin, cout)) +
                         (size_t)cout_pad * 4;                          // [fragments][inverse scales][scales (packing scratch)]
    DevBuf buf = fresh(bytes);
    uint32_t* pk = buf.as<uint32_t>();
    float* inv = reinterpret_cast<float*>(pk) + frags * 4;
    float* sc = inv + cout_pad;
    const PackWinoArgs pa{oihw, pk, cin, cout, frags};
    const dim3 gs((unsigned)((cout_pad + 255) / 256)), gp((unsigned)((frags + 255) / 256));
    if (f43) {              // (one wave per output channel)
      DRT_LAUNCH(wino43_co_scale_kernel, dim3((unsigned)cout_pad), dim3(64), stream_, oihw, cin, cout, cout_pad, inv, sc);
      DRT_LAUNCH(pack_weights_wino43_kernel, gp, dim3(256), stream_, pa, (const float*)sc);
    } else if (f2d) {
      DRT_LAUNCH(wino2d_co_scale_kernel, gs, dim3(256), stream_, oihw, cin, cout, cout_pad, inv, sc);
      DRT_LAUNCH(pack_weights_wino2d_kernel, gp, dim3(256), stream_, pa, (const float*)sc);
    } else {
      DRT_LAUNCH(wino_co_scale_kernel, gs, dim3(256), stream_, oihw, cin, cout, cout_pad, inv, sc);
      DRT_LAUNCH(pack_weights_wino_kernel, gp, dim3(256), stream_, pa, (const float*)sc);
    }
    *scale_out = inv;
    return buf;
  }

  // NIN weights W[cin][cout] (layers.py:549); nsrc of them concatenated along cout (fused q|k|v projection)
  ConvW make_nin(const std::string& pre, const int* which, int nsrc, int C) {
    ConvW c; c.ks = 1; c.cin = C; c.cout = nsrc * C;
    float* tr = keep(fresh((size_t)nsrc * C * C * 4));
    float* bb = keep(fresh((size_t)nsrc * C * 4));
    for (int s = 0; s < nsrc; ++s) {
      const std::string n = pre + "NIN_" + std::to_string(which[s]);
      DRT_LAUNCH(transpose_io_kernel, dim3((C * C + 255) / 256), dim3(256), stream_, Wp(n + ".W"), tr + (size_t)s * C * C, C, C);
      SG_CHECK(drt::memcpy_d2d(bb + (size_t)s * C, Wp(n + ".b"), (size_t)C * 4, stream_));
    }
    c.oihw = tr; c.bias = bb;
    ConvPlan pl = choose_conv_plan(1, C, c.cout, 8, 32);
    if (pl.mfma) {
      c.co_t = pl.co_t;
      PackArgs pa{}; pa.nsrc = nsrc; pa.cout_per_src = C; pa.io = 1; pa.cin = C; pa.taps = 1; pa.cout = c.cout;
      for (int s = 0; s < nsrc; ++s) pa.src[s] = Wp(pre + "NIN_" + std::to_string(which[s]) + ".W");
      c.packed = keep(pack_mfma(pa, pl.co_t));
      // (round 5) the 32-channel-tile layout too, as make_conv does: the attention projections sit at the 16 x 32 and 4 x 8 levels, where
      // conv() runs the fp32 layers on 32-channel tiles with chunked accumulation and, at small batches, split-K -- without this layout
      // q|k|v and the output projection stayed on 128-channel tiles: 24 / 8 workgroups running 16 serial K-stages at batch 1
      // (31 / 30 us per launch against 18 us for the 1x1 shortcut of the same size, profiles/r05_prof_dump_b1.txt)
      // (round 6: the compile-time switch of round 5's A/B is gone -- one build variant, the tested one.  Attention outputs changed in
      //  their last bits with that round: fixtures of these levels recorded before it are not bit-comparable.)
      if (pl.co_t > 32) c.packed32 = keep(pack_mfma(pa, 32));
    }
    if (split_mode_ && conv_split_eligible(1, C, 0, c.cout)) {
      c.split_mode = 1;
      c.packed_split = keep(pack_split(c.oihw, 1, C, c.cout, 1, &c.split_scale));
    }
    return c;
  }

  void finalize_weights() {
    res_.clear(); attn_.clear(); conv_.clear(); gn_.clear();
    std::vector<DenseDesc> descs;
    int off = 0;
    for (const Mod& m : layout_) {
      const std::string p = "all_modules." + std::to_string(m.idx) + ".";
      if (m.kind == Mod::RES) {
        ResW r{};
        r.g0w = Wp(p + "GroupNorm_0.weight"); r.g0b = Wp(p + "GroupNorm_0.bias");
        r.g1w = Wp(p + "GroupNorm_1.weight"); r.g1b = Wp(p + "GroupNorm_1.bias");
        r.c0 = make_conv(p + "Conv_0.weight", p + "Conv_0.bias", 3, m.cin, m.cout);
        r.c1 = make_conv(p + "Conv_1.weight", p + "Conv_1.bias", 3, m.cout, m.cout);
        r.has_c2 = (m.cin != m.cout) || m.up || m.down;
        if (r.has_c2) r.c2 = make_conv(p + "Conv_2.weight", p + "Conv_2.bias", 1, m.cin, m.cout);
        r.temb_off = off;
        descs.push_back(DenseDesc{Wp(p + "Dense_0.weight"), Wp(p + "Dense_0.bias"), r.c0.bias, m.cout, off});
        off += m.cout;
        res_[m.idx] = r;
      } else if (m.kind == Mod::ATTN) {
        AttnW a{};
        a.gw = Wp(p + "GroupNorm_0.weight"); a.gb = Wp(p + "GroupNorm_0.bias");
        const int qkv[3] = {0, 1, 2}, pr[1] = {3};
        a.qkv = make_nin(p, qkv, 3, m.cin);
        a.proj = make_nin(p, pr, 1, m.cin);
        attn_[m.idx] = a;
      } else if (m.kind == Mod::CONV3) {
        conv_[m.idx] = make_conv(p + "weight", p + "bias", 3, m.cin, m.cout);
        if (m.cin == 4 && entry_mfma_) {
          // Entry convolution (4 -> nf on the full-resolution image, ncsnpp.py:286): as a direct VALU kernel it was bound by
          // its scalar weight loads (1.6 ms at batch 32 for a 0.36 ms output write, plus a 0.4 ms statistics pass).  With the
          // input channels zero-padded to one 8-channel K-stage it runs on the fp32 MFMA kernel, GroupNorm partials fused
          // (1.07 ms; 16 channels on the bf16x3 split kernel measured the same at batch 32 and twice the time at batch 1)
          constexpr int cp = 8;
          float* w8 = keep(fresh((size_t)m.cout * cp * 9 * 4));
          DRT_LAUNCH(pad_cin_kernel, dim3((unsigned)(((size_t)m.cout * cp * 9 + 255) / 256)), dim3(256), stream_, Wp(p + "weight"), w8, m.cout, 4, cp, 9);
          entry8_ = make_conv(w8, Wp(p + "bias"), 3, cp, m.cout);
          entry8_idx_ = m.idx;
        }
      } else if (m.kind == Mod::COMBINE) {
        conv_[m.idx] = make_conv(p + "Conv_0.weight", p + "Conv_0.bias", 1, m.cin, m.cout);
      } else if (m.kind == Mod::GN) {
        gn_[m.idx] = {Wp(p + "weight"), Wp(p + "bias")};
      }
    }
    tot_temb_ = off;
    n_dense_ = (int)descs.size();
    dense_descs_ = keep<DenseDesc>(fresh(sizeof(DenseDesc) * descs.size()));
    SG_CHECK(drt::memcpy_h2d(dense_descs_, descs.data(), sizeof(DenseDesc) * descs.size(), stream_));
    SG_CHECK(drt::stream_sync(stream_));
    check_launch();
    weights_ready_ = true;
    shape_B_ = 0;
    temb_rows_ = 0;      // the time-embedding tables are sized by nf / the Dense layout of THIS net
  }

  // ---- shape-dependent buffers --------------------------------------------------------------------------------
  void ensure_shape(int B, int F, int T, int nrows) {
    SG_REQUIRE(B >= 1 && F >= 1 && T >= 1, "bad shape");
    const int down = 1 << (cfg_.n_levels - 1);
    SG_REQUIRE(F % down == 0 && T % down == 0, "F and T must be multiples of 2^(levels-1) (pad_spec pads T to a multiple of 64)");
    if (B != shape_B_ || F != shape_F_ || T != shape_T_ || (ragged() && !rag_built_)) {
      invalidate_graph();
      cur_F_ = F;
      if (ragged()) build_rag_tables(B, F, T);
      // size the arena by a dry run
      arena_.measure_mode();
      dry_ = true;
      {
        FwdCtl ctl{nullptr, 0, 0, nullptr, nullptr, 0, 0, 1.f};
        run_forward(nullptr, 0, nullptr, 0, nullptr, B, F, T, ctl);
      }
      dry_ = false;
      grow(arena_buf_, arena_.high_water() + (1 << 20));
      arena_.configure(arena_buf_.as<char>(), arena_buf_.capacity());
      const size_t n = (size_t)B * F * T;      // (a ragged batch needs at most this)
      for (DevArray<float2>* q : {&sx_, &sxm_, &sscore_, &sy_}) grow(*q, n * 8);
      // range-bound slots: one per convolution output of the forward just dry-run
      amax_slots_ = amax_next_;
      grow(amax_pool_, (size_t)amax_next_ * B * kAmaxSpread * 4);
      grow(step_ctr_, 256);
      grow(lang_scal_, std::max<size_t>(256, (size_t)B * 2 * 4));      // {step, sqrt(2 step)}: one pair, or one per utterance
      renew(lang_partial_, (size_t)B * LANG_NBLK * 2 * 4);
      shape_B_ = B; shape_F_ = F; shape_T_ = T;
    }
    if (nrows > temb_rows_) {      // the six time-embedding tables: sized by the rows and by this net's Dense layout, re-allocated together
      invalidate_graph();
      temb_rows_ = 0;
      const size_t rows = std::max(nrows, 64);
      renew(temb_act_, rows * 4 * cfg_.nf * 4);
      renew(bias_table_, rows * std::max(tot_temb_, 1) * 4);
      renew(bias_cur_, (size_t)std::max(tot_temb_, 1) * 4);
      renew(step_table_, rows * SC_STRIDE * 4);
      renew(tsteps_, rows * 4);
      renew(coef_table_, rows * 16);
      temb_rows_ = (int)rows;
    }
  }

  // ---- windowed score (set_windows) ------------------------------------------------------------------------------
  struct WinPlan {
    int K = 0, W = 0, n = 0, max_batch = 0, C = 0, Bc = 0, id = 0; std::vector<int> start;
    bool same(const WinPlan& o) const { return K == o.K && W == o.W && n == o.n && max_batch == o.max_batch && start == o.start; }
  };
  WinPlan win_; bool win_on_ = false, win_dirty_ = false; int win_serial_ = 0;
  DevArray<int> win_plan_tab_;               // start[C * Bc]: the plan's starts, the last one repeated in the filler slots
  DevArray<float2> win_x_, win_y_, win_score_;   // [Bc][F][W] gathered state of one chunk; [C * Bc][F][W] y and scores of all slots
  int win_key() const { return win_on_ ? win_.id : 0; }
  // A sampler call under the plan: what it refuses, the network's shape (Bc, F, W), state arrays of F * K elements, window buffers, the
  // plan on the device.  A buffer that moved invalidates the captured step.
  void win_begin(const std::string& who, int B, int F, int T, int nrows) {
    const auto refuse = [&](const std::string& why) {
      frames_next_.clear(); streams_next_.clear();      // (what was pending belonged to this call)
      throw EngineArgError(who + ": " + why);
    };
    if (ragged()) refuse("a window plan (sgmse_set_windows) and a ragged batch (sgmse_set_frames) exclude each other");
    if (!frames_next_.empty()) refuse("a window plan (sgmse_set_windows) draws the recording's own noise field: a noise geometry (sgmse_set_noise_frames) does not apply");
    if (B != 1) refuse("a window plan (sgmse_set_windows) takes one recording: B must be 1, got " + std::to_string(B));
    if (T != win_.K) refuse("T = " + std::to_string(T) + " is not the window plan's K = " + std::to_string(win_.K));
    const int down = 1 << (cfg_.n_levels - 1);
    if (win_.W % down) refuse("the window plan's W must be a multiple of 2^(levels-1) = " + std::to_string(down));
    SG_REQUIRE(F <= 65535, "window plan: more than 65535 rows");
    ensure_shape(win_.Bc, F, win_.W, nrows);
    const size_t state = (size_t)F * win_.K * 8, slot = (size_t)F * win_.W * 8, slots = (size_t)win_.C * win_.Bc;
    bool moved = false;
    for (DevArray<float2>* q : {&sx_, &sxm_, &sscore_, &sy_}) moved |= grow(*q, state);
    moved |= grow(win_x_, slot * win_.Bc);
    moved |= grow(win_y_, slot * slots);
    moved |= grow(win_score_, slot * slots);
    moved |= grow(win_plan_tab_, slots * sizeof(int));
    if (moved) invalidate_graph();
    if (win_dirty_ || moved) {
      int* h = reinterpret_cast<int*>(stage_.acquire(slots * sizeof(int)));
      for (size_t j = 0; j < slots; ++j) h[j] = win_.start[std::min<size_t>(j, win_.n - 1)];
      SG_CHECK(drt::memcpy_h2d(win_plan_tab_, h, slots * sizeof(int), stream_));
      stage_.commit(stream_);
      win_dirty_ = false;
    }
  }
  void win_gather(const float2* src, float2* dst, int F, int first, int slots) {
    WinArgs a{src, dst, win_plan_tab_.get() + first, F, win_.K, win_.W, slots};
    DRT_LAUNCH(window_gather_kernel, dim3((win_.W + 255) / 256, F, slots), dim3(256), stream_, a);
  }
  void win_gather_y(int F) { win_gather(sy_, win_y_, F, 0, win_.C * win_.Bc); }      // once per sampler call
  // One score evaluation of the samplers' step: sscore_ = network(sx_, sy_) of the batch, or, under a window plan, of the recording
  // through its windows.
  void eval_score(int B, int F, int T, const FwdCtl& ctl) {
    if (!win_on_) {
      const long long FT = ragged() ? 1 : (long long)F * T;          // batch stride of x / y (ragged: multiplier of the utterance's offset)
      arena_.reset();
      run_forward(sx_, FT, sy_, FT, sscore_, B, F, T, ctl);
      return;
    }
    const long long FW = (long long)F * win_.W;
    for (int c = 0; c < win_.C; ++c) {
      const size_t off = (size_t)c * win_.Bc * FW;
      win_gather(sx_, win_x_, F, c * win_.Bc, win_.Bc);
      arena_.reset();
      run_forward(win_x_, FW, win_y_ + off, FW, win_score_ + off, win_.Bc, F, win_.W, ctl);      // (the score wrapper reads the gathered x)
    }
    WinArgs a{win_score_, sscore_, win_plan_tab_, F, win_.K, win_.W, win_.n};
    DRT_LAUNCH(window_blend_kernel, dim3((win_.K + 255) / 256, F), dim3(256), stream_, a);
  }

  void compute_temb(const float* t_dev, int rows) {
    TembArgs ta{t_dev, rows, Wp("all_modules.0.W"), Wp("all_modules.1.weight"), Wp("all_modules.1.bias"),
                Wp("all_modules.2.weight"), Wp("all_modules.2.bias"), cfg_.nf, temb_act_};
    SG_REQUIRE(cfg_.nf <= 256, "nf > 256 not supported by temb kernel");
    DRT_LAUNCH(temb_mlp_kernel, dim3(rows), dim3(256), stream_, ta);
    DRT_LAUNCH(temb_dense_kernel, dim3(n_dense_, rows), dim3(256), stream_, (const DenseDesc*)dense_descs_,
               (const float*)temb_act_, 4 * cfg_.nf, bias_table_.get(), tot_temb_);
    check_launch();
  }

  // ---- op wrappers used by the forward ------------------------------------------------------------------------
  // fused producer of a consumer's input.  `bound`: per-utterance upper bound of |producer output| (gn_coeffs), from which the
  // fp16x2 3x3 kernel derives its input scale.  A tensor that IS the FIR-resampled output of a producer applied upstream
  // (scale == nullptr) inherits that producer's bound: the [1,3,3,1] resamplers are convex combinations.
  struct Xform { const float* scale = nullptr; const float* shift = nullptr; int act = 0; const float* bound = nullptr; };

  void tick(int cls, double work, int launches = 1) {
    if (debug_sync_ && !dry_ && !capturing_) {      // SGMSE_DEBUG_SYNC=1: wait for every launch and name it (a device fault then names its kernel)
      const int e = drt::stream_sync(stream_);
      fprintf(stderr, "[sgmse-dbg] %s -> %s\n", prof_note_[0] ? prof_note_ : "(launch)", e ? drt::error_string(e) : "ok");
      fflush(stderr);
      if (!prof_) prof_note_[0] = 0;
    }
    if (!prof_ || prof_used_ == 0) return;
    ProfRec& r = prof_recs_[prof_used_ - 1];
    drt::event_record(r.b.get(), stream_);
    r.cls = cls; r.work = work; r.launches = launches;
    snprintf(r.note, sizeof r.note, "%s", prof_note_);
    prof_note_[0] = 0;
  }
  bool noting() const { return (prof_ && prof_dump_) || debug_sync_; }
  // one event pair per launch of a profiled forward (created on first use, reused by later profiles, destroyed with the engine)
  struct ProfRec { Event a, b; int cls = -1; double work = 0.0; int launches = 0; char note[160] = {0}; };
  void tock() {
    if (lds_poison_ && !dry_ && !capturing_ && !drt::is_emulator()) {
      const int idx = lds_poison_count_++;
      if (lds_poison_at_ < 0 || idx == lds_poison_at_ || (lds_poison_upto_ && idx <= lds_poison_at_)) {
        grow(lds_sink_, 256);
        DRT_LAUNCH(lds_poison_kernel, dim3(768), dim3(256), stream_, lds_sink_.get(), (unsigned)idx);
      }
    }
    if (!prof_) return;
    if (prof_used_ == prof_recs_.size()) {
      prof_recs_.emplace_back();
      prof_recs_.back().a.create(); prof_recs_.back().b.create();
    }
    ProfRec& r = prof_recs_[prof_used_++];
    r.cls = -1; r.note[0] = 0;
    drt::event_record(r.a.get(), stream_);
  }

  Tensor new_tensor(int C, int H, int W) { Tensor t; t.C = C; t.H = H; t.W = W; t.p = arena_.alloc((size_t)C * pix_total(H, W)); return t; }

  // ---- ragged batches (set_frames): utterances of different frame counts in one launch ------------------------------------
  // Every activation tensor holds utterance b's planes with its own row stride, packed one utterance after the other; the
  // per-level tables below give each kernel an utterance's width and first pixel (Rag, kernels_conv.h).  Which kernel FAMILY a
  // layer runs on is decided from the level alone (dec_W: the width a 512-frame utterance has there), never from the actual
  // widths: an utterance then goes through the same kernels, with the same arithmetic, alone, in a uniform batch or in a
  // ragged one.
  static constexpr int kNominalFrames = 512;
  bool ragged() const { return !rag_T_.empty(); }
  int level_of(int H) const { int l = 0; while ((cur_F_ >> l) > H && l < 30) ++l; return l; }
  int dec_W(int H) const { return std::max(1, kNominalFrames >> level_of(H)); }
  size_t pix_total(int H, int W) const { return ragged() ? rag_.at(level_of(H)).pix : (size_t)B_ * H * W; }
  Rag rag_of(int H) const {
    if (!ragged()) return Rag{nullptr, nullptr, nullptr};
    const RagLevel& r = rag_.at(level_of(H));
    return Rag{r.w, r.off, r.soff};
  }
  const long long* rag_off0() const { return ragged() ? rag_[0].off.get() : nullptr; }      // first elements of the utterances in the packed tensors
  bool rag_all_mult(int H, int m) const {          // a ragged batch: is every utterance's width at this level a multiple of m?  (uniform batches: yes, the caller checks W)
    const int l = level_of(H);
    for (int t : rag_T_) if ((t >> l) % m) return false;
    return true;
  }
  void set_frames(const int* frames, int n) {          // n == 0: uniform batches again
    std::vector<int> v(frames, frames + n);
    if (v != rag_T_) { rag_T_ = v; rag_built_ = false; shape_B_ = 0; invalidate_graph(); }
  }
  void build_rag_tables(int B, int F, int T) {
    const int L = cfg_.n_levels, down = 1 << (L - 1);
    SG_REQUIRE((int)rag_T_.size() == B, "ragged batch: sgmse_set_frames gave a different number of utterances");
    int tmax = 0;
    for (int t : rag_T_) { SG_REQUIRE(t >= down && t % down == 0, "ragged batch: frame counts must be multiples of 2^(levels-1)"); tmax = std::max(tmax, t); }
    SG_REQUIRE(tmax == T, "ragged batch: T must be the largest frame count");
    rag_.clear();
    for (int l = 0; l < L; ++l) {
      const int H = F >> l;
      std::vector<int> w(B), cols(B + 1, 0);
      std::vector<long long> off(B + 1, 0), soff(B + 1, 0);
      for (int b = 0; b < B; ++b) {
        w[b] = rag_T_[b] >> l;
        off[b + 1] = off[b] + (long long)H * w[b];
        soff[b + 1] = soff[b] + (long long)H * ((w[b] + 31) / 32);
        cols[b + 1] = cols[b] + (w[b] + 31) / 32;             // tile columns that exist (ConvArgs::rag_cols)
      }
      RagLevel r;
      r.pix = (size_t)off[B]; r.ncols = cols[B];
      grow(r.w, (size_t)B * 4); grow(r.off, (size_t)(B + 1) * 8); grow(r.soff, (size_t)(B + 1) * 8); grow(r.cols, (size_t)(B + 1) * 4);
      SG_CHECK(drt::memcpy_h2d(r.w, w.data(), (size_t)B * 4, stream_));
      SG_CHECK(drt::memcpy_h2d(r.off, off.data(), (size_t)(B + 1) * 8, stream_));
      SG_CHECK(drt::memcpy_h2d(r.soff, soff.data(), (size_t)(B + 1) * 8, stream_));
      SG_CHECK(drt::memcpy_h2d(r.cols, cols.data(), (size_t)(B + 1) * 4, stream_));
      SG_CHECK(drt::stream_sync(stream_));
      rag_.push_back(std::move(r));
    }
    rag_built_ = true;
  }
  std::vector<int> rag_T_;
  // one U-Net level's tables: per utterance its width, first pixel, first statistics sub-tile and first tile column (B + 1 entries:
  // prefix sums); pixels and tile columns of the whole batch
  struct RagLevel { DevArray<int> w; DevArray<long long> off, soff; DevArray<int> cols; size_t pix = 0; int ncols = 0; };
  std::vector<RagLevel> rag_;
  bool rag_built_ = false;
  int cur_F_ = 0;
  void drop(Tensor& t) { arena_.release(t.p); t.p = nullptr; if (t.st) { arena_.release(t.st); t.st = nullptr; } }

  // GroupNorm coefficients of the virtual concat [a | b].  Per-channel partial sums come from the producing convolution's
  // epilogue when it emitted them (Tensor::st), otherwise from one streaming pass over the tensor.
  // *bound (optional): per-utterance upper bound of |GroupNorm(+SiLU) output| for an fp16x2 consumer (gn_finalize_kernel)
  void gn_coeffs(const Tensor& a, const Tensor* b, const float* gamma, const float* beta, float** sc, float** sh,
                 const float** bound = nullptr) {
    const int C = a.C + (b ? b->C : 0), HW = a.H * a.W;
    float* bslot = bound ? next_amax() : nullptr;
    if (bound) *bound = bslot;
    const float* st[2] = {a.st, b ? b->st : nullptr};
    int nsub[2] = {a.nsub, b ? b->nsub : 0};
    int srows[2] = {a.srows, b ? b->srows : 1};
    float* tmp[2] = {nullptr, nullptr};
    const Tensor* src[2] = {&a, b};
    for (int k = 0; k < 2; ++k) {
      if (!src[k] || st[k]) continue;
      tmp[k] = arena_.alloc((size_t)B_ * src[k]->C * 2);
      st[k] = tmp[k]; nsub[k] = 1; srows[k] = 1;
      if (!dry_) {
        tock();
        DRT_LAUNCH(gn_chan_stats_kernel, dim3(B_ * src[k]->C), dim3(256), stream_, (const float*)src[k]->p, (const float*)nullptr,
                   src[k]->C, 0, HW, tmp[k], rag_of(a.H), a.H);
        if (noting()) snprintf(prof_note_, sizeof prof_note_, "gn_chan_stats C=%d @%dx%dx%d", src[k]->C, B_, a.H, a.W);
        tick(TC_GN, 4.0 * B_ * (double)src[k]->C * HW, 1);
      }
    }
    *sc = arena_.alloc((size_t)B_ * C);
    *sh = arena_.alloc((size_t)B_ * C);
    if (!dry_) {
      tock();
      const int G = std::min(C / 4, 32);
      const GnFin f{st[0], st[1], a.amax, b ? b->amax : nullptr, gamma, beta, *sc, *sh, bslot, rag_of(a.H),
                    a.C, nsub[0], srows[0], b ? b->C : 0, nsub[1], srows[1], G, HW, a.H, 1e-6f};
      DRT_LAUNCH(gn_finalize_kernel, dim3(G, B_), dim3(256), stream_, f);
      if (noting()) snprintf(prof_note_, sizeof prof_note_, "gn_finalize C=%d nsub=%d @%dx%dx%d", C, nsub[0], B_, a.H, a.W);
      tick(TC_GN, 8.0 * B_ * ((double)a.C * nsub[0] + (b ? (double)b->C * nsub[1] : 0.0)), 1);
    }
    for (int k = 0; k < 2; ++k) if (tmp[k]) arena_.release(tmp[k]);
  }

  // residual shortcut folded into a 3x3 split launch (ConvArgs::sc_*): the 1x1 layer and its (raw) input
  struct Shortcut { const ConvW* w; const Tensor* a; const Tensor* b; };
  // may this 1x1 shortcut be folded at all: split-packed in fp16x2, with known input ranges
  bool shortcut_foldable(const ConvW& c2, const Tensor& a, const Tensor* b) const {
    return fold_shortcut_ && c2.packed_split && c2.split_mode == 2 && c2.ks == 1 && conv_split_eligible(1, a.C, b ? b->C : 0, c2.cout) &&
           a.amax && (!b || b->amax);
  }

  // the route of one convolution (conv_route.h) from the layer, the level of its input and what the call brings
  ConvRoute route_of(const ConvW& w, int C1, int C2, int H, int W, const ConvCall& call) const {
    const ConvLayer layer{w.ks, C1, C2, w.cout, w.co_t, w.packed != nullptr, w.packed32 != nullptr, w.packed_thin != nullptr,
                          w.packed_split != nullptr, w.packed_wino != nullptr, w.split_mode, w.wino_form};
    const ConvKnobs knobs{tile_min_blocks_, split_min_tiles_, wino_min_tiles_, wino_, fuse_gn_stats_, chunk_max_tiles_, coarse_splitk_div_,
                          coarse_chunked_, coarse_split_};
    return conv_route(layer, ConvLevel{H, W, dec_W(H), level_of(H)}, call, B_, knobs);
  }

  Tensor conv(const ConvW& w, const Tensor& a, const Tensor* b, const Xform& xf, const float* bias, const float* bias2,
              const float* res, float out_scale, const FwdCtl& ctl, bool emit_stats = false, const Shortcut* sc = nullptr) {
    const int C2 = b ? b->C : 0, Cin = a.C + C2;
    SG_REQUIRE(Cin == w.cin, "conv: channel mismatch");
    Tensor o = new_tensor(w.cout, a.H, a.W);
    const ConvRoute rt = route_of(w, a.C, C2, a.H, a.W, ConvCall{xf.bound != nullptr, a.amax && (!b || b->amax), xf.scale != nullptr, emit_stats,
                                                                 bias2 != nullptr, sc != nullptr});
    const ConvFamily fam = rt.family;
    // what the route's kernels need of the actual widths and of the call: checks on the route (the family is decided by the level alone)
    SG_REQUIRE(fam != ConvFamily::Wino23 || (a.W % 2 == 0 && rag_all_mult(a.H, 2)), "conv: odd width on a Winograd level");
    SG_REQUIRE(fam != ConvFamily::Wino43 || (a.W % 4 == 0 && rag_all_mult(a.H, 4)), "conv: width not a multiple of 4 on a Winograd F(4,3) level");
    SG_REQUIRE(!sc || (rt.accepts_shortcut && xf.act && !res), "conv: shortcut fold on an ineligible launch");
    // ---- allocate: split-K partial sums, GroupNorm statistics, the range-bound slot
    float* partial = rt.ksplit > 1 ? arena_.alloc((size_t)rt.ksplit * w.cout * pix_total(a.H, a.W)) : nullptr;
    if (emit_stats && fuse_gn_stats_ && fam != ConvFamily::Direct) {
      o.srows = rt.srows;
      SG_REQUIRE(o.srows == 1 || !ragged() || a.H % 4 == 0, "ragged batch: 4-row statistics sub-tiles need H % 4 == 0");
      o.nsub = conv_plan_nsub(a.H, a.W, o.srows);
      o.st = arena_.alloc((size_t)B_ * w.cout * o.nsub * 2);
    } else if (emit_stats && fuse_gn_stats_) {
      // direct kernel: one statistics pass right behind it, kept with the tensor -- these outputs (entry conv, Combine)
      // are normalised twice, by the next block and again as skip connections on the way up
      o.nsub = 1;
      o.st = arena_.alloc((size_t)B_ * w.cout * 2);
    }
    o.amax = next_amax();
    if (dry_) { if (partial) arena_.release(partial); return o; }
    ConvArgs ca{};
    ca.xcd_map = conv_xcd_map_ ? 1 : 0;
    ca.stats_out = o.st; ca.stats_nsub = o.nsub; ca.stats_rows = o.srows;
    ca.amax_out = o.amax;
    ca.src1 = a.p; ca.src2 = b ? b->p : nullptr; ca.C1 = a.C; ca.C2 = C2;
    ca.bias = bias; ca.bias2 = bias2; ca.bias2_bstride = ctl.bias_bstride; ca.bias2_sstride = ctl.bias_sstride;
    ca.step_ptr = bias2 ? ctl.bias_step : nullptr;
    ca.in_scale = xf.scale; ca.in_shift = xf.shift; ca.in_act = xf.act;
    ca.res = res; ca.out_scale = out_scale; ca.out = o.p; ca.Cout = w.cout; ca.B = B_; ca.H = a.H; ca.W = a.W;
    ca.kchunk_stages = rt.kchunk; ca.partial = partial;
    if (ragged()) {
      const Rag rg = rag_of(a.H);
      ca.rag_w = rg.w; ca.rag_off = rg.off; ca.rag_soff = rg.soff; ca.rag_slab = (long long)w.cout * (long long)pix_total(a.H, a.W);
      ca.rag_vec_ok = rag_all_mult(a.H, 4) ? 1 : 0;
      if (rag_prefix_) { const RagLevel& r = rag_.at(level_of(a.H)); ca.rag_cols = r.cols; ca.rag_ncols = r.ncols; }
    }
    double fl = 2.0 * B_ * (double)w.cout * Cin * w.ks * w.ks * a.H * a.W;
    if (sc) {
      const int Cs = sc->a->C + (sc->b ? sc->b->C : 0);
      SG_REQUIRE(Cs == sc->w->cin && sc->w->cout == w.cout && sc->a->H == a.H && sc->a->W == a.W, "conv: shortcut shape mismatch");
      ca.sc_src1 = sc->a->p; ca.sc_src2 = sc->b ? sc->b->p : nullptr; ca.sc_C1 = sc->a->C; ca.sc_C2 = sc->b ? sc->b->C : 0;
      ca.sc_w = sc->w->packed_split; ca.sc_scale = sc->w->split_scale; ca.sc_bias = sc->w->bias;
      ca.sc_amax1 = sc->a->amax; ca.sc_amax2 = sc->b ? sc->b->amax : nullptr;
      fl += 2.0 * B_ * (double)w.cout * Cs * a.H * a.W;
    }
    tock();
    const char* gn = xf.scale ? " +gn" : "";
    const char* rs = res ? " +res" : "";
    const char* ex = ca.rag_cols ? " existing-tiles" : "";
    auto note_split = [&](const char* name) {        // the split and Winograd families
      if (!noting()) return;
      char scn[24] = "";
      if (sc) snprintf(scn, sizeof scn, " +shortcut(%d)", ca.sc_C1 + ca.sc_C2);      // (input channels of the folded 1x1)
      snprintf(prof_note_, sizeof prof_note_, "conv3x3-%s %d->%d @%dx%dx%d%s%s%s%s", name, Cin, w.cout, B_, a.H, a.W, rs, gn, scn, ex);
    };
    int cls = w.ks == 3 ? (w.cout >= 128 ? TC_CONV3_BIG : TC_CONV3) : TC_CONV1;      // (the split and Winograd families)
    switch (fam) {
      case ConvFamily::Thin:
        ca.w = w.packed_thin; ca.stats_out = nullptr;
        launch_conv_thin(ca, stream_);
        if (noting()) snprintf(prof_note_, sizeof prof_note_, "conv3x3-thin %d->%d @%dx%dx%d%s%s", Cin, w.cout, B_, a.H, a.W, rs, gn);
        cls = TC_CONV3;
        break;
      case ConvFamily::Wino43:
        SG_REQUIRE(conv_wino43_aligned(ca), "conv: unaligned source on a Winograd F(4,3) level");
        [[fallthrough]];
      case ConvFamily::Wino23:
        ca.w = w.packed_wino; ca.co_scale = w.wino_scale;
        bind_bounds(ca, w.ks, xf.bound, a.amax, b ? b->amax : nullptr);
        launch_conv_wino(w.wino_form, ca, stream_, rt.rows4);
        note_split(fam == ConvFamily::Wino43 ? "wino43" : "wino");
        break;
      case ConvFamily::Split:
      case ConvFamily::SplitCoarse:
        ca.w = w.packed_split; ca.co_scale = w.split_scale;      // (null for bf16x3: no scale)
        if (w.split_mode == 2) bind_bounds(ca, w.ks, xf.bound, a.amax, b ? b->amax : nullptr);
        launch_conv_split(ca, w.ks, w.split_mode, stream_, rt.rows4, 0, rt.ksplit);
        note_split("split");
        break;
      case ConvFamily::Mfma:
        ca.w = (rt.co_t == w.co_t) ? w.packed : w.packed32;
        launch_conv_mfma(ca, w.ks, ConvPlan{rt.co_t, rt.rows, true}, stream_, -1, rt.ksplit);
        if (noting())
          snprintf(prof_note_, sizeof prof_note_, "conv%dx%d %d->%d @%dx%dx%d tile %dco x %drows%s%s%s%s", w.ks, w.ks, Cin, w.cout, B_, a.H, a.W,
                   rt.co_t, rt.rows, rs, gn, rt.ksplit > 1 ? " split-K" : "", ex);
        // class "wide" = the dominant kernel family only: the split kernels, or (SGMSE_CONV_SPLIT=0) the fp32 128 x 256 tile
        cls = w.ks == 3 ? ((split_mode_ == 0 && rt.co_t == 128 && rt.rows == 8) ? TC_CONV3_BIG : TC_CONV3) : TC_CONV1;
        break;
      case ConvFamily::Direct:
        ca.w = w.oihw; ca.stats_out = nullptr;
        launch_conv_direct(ca, w.ks, stream_);
        if (noting()) snprintf(prof_note_, sizeof prof_note_, "conv-direct%dx%d %d->%d @%dx%dx%d", w.ks, w.ks, Cin, w.cout, B_, a.H, a.W);
        cls = TC_DIRECT;
        break;
    }
    tick(cls, fl);
    if (partial) arena_.release(partial);
    if (fam == ConvFamily::Direct && o.st) {
      tock();
      DRT_LAUNCH(gn_chan_stats_kernel, dim3(B_ * w.cout), dim3(256), stream_, (const float*)o.p, (const float*)nullptr, w.cout, 0,
                 a.H * a.W, o.st, rag_of(a.H), a.H);
      if (noting()) snprintf(prof_note_, sizeof prof_note_, "gn_chan_stats(direct) C=%d @%dx%dx%d", w.cout, B_, a.H, a.W);
      tick(TC_GN, 4.0 * B_ * (double)w.cout * a.H * a.W, 1);
    }
    return o;
  }

  void launch_fir(const FirArgs& fa, bool up, bool by_level = false) {
    const int H = fa.H, W = fa.W, BC = fa.BC;
    // tiled or per-pixel kernel: by the LEVEL (dec_W) inside the network, so that an utterance's FIR never depends on its length
    const bool tiled = by_level ? (W % 4 == 0 && dec_W(H) >= 64 && rag_all_mult(H, 4)) : fir_use_tiled(W);
    if (tiled && !fir_scalar_) {
      if (up) DRT_LAUNCH(fir_up2_tiled_kernel, dim3(((W + 63) / 64) * ((H + 7) / 8), BC), dim3(256), stream_, fa);
      else DRT_LAUNCH(fir_down2_tiled_kernel, dim3(((W / 2 + 63) / 64) * ((H / 2 + 7) / 8), BC), dim3(256), stream_, fa);
    } else {
      if (up) DRT_LAUNCH(fir_up2_kernel, dim3((H * W + 255) / 256, BC), dim3(256), stream_, fa);
      else DRT_LAUNCH(fir_down2_kernel, dim3(((H / 2) * (W / 2) + 255) / 256, BC), dim3(256), stream_, fa);
    }
  }

  // FIR x2 / /2 of `a` through the fused producer `xf`; with `raw` also FIR(a) itself from the same pass
  Tensor fir(const Tensor& a, bool up, const Xform& xf, Tensor* raw = nullptr) {
    Tensor o = up ? new_tensor(a.C, a.H * 2, a.W * 2) : new_tensor(a.C, a.H / 2, a.W / 2);
    if (raw) {
      *raw = up ? new_tensor(a.C, a.H * 2, a.W * 2) : new_tensor(a.C, a.H / 2, a.W / 2);
      raw->amax = a.amax;      // the [1,3,3,1] resamplers are convex combinations (per output phase): max|FIR(x)| <= max|x|
    }
    if (dry_) return o;
    FirArgs fa{a.p, o.p, xf.scale, xf.shift, xf.act, B_ * a.C, a.H, a.W, raw ? raw->p : nullptr, a.C, rag_of(a.H)};
    tock();
    launch_fir(fa, up, true);
    if (noting()) snprintf(prof_note_, sizeof prof_note_, "fir-%s C=%d @%dx%dx%d%s", up ? "up" : "down", a.C, B_, a.H, a.W, raw ? " +raw" : "");
    tick(TC_FIR, 4.0 * B_ * (double)a.C * (a.H * a.W + (raw ? 2.0 : 1.0) * o.H * o.W));
    return o;
  }

  // ResnetBlockBigGANpp.forward (layerspp.py:242-274).  Inputs stay owned by the caller.
  Tensor res_block(const Mod& m, Tensor& a, Tensor* b, const FwdCtl& ctl) {
    const ResW& r = res_.at(m.idx);
    float *sc0, *sh0, *sc1, *sh1;
    const float *bd0, *bd1;
    gn_coeffs(a, b, r.g0w, r.g0b, &sc0, &sh0, &bd0);
    Xform x0{sc0, sh0, 1, bd0};
    const float* temb = ctl.bias_table ? ctl.bias_table + r.temb_off : nullptr;
    Tensor h, xs;       // xs: resampled shortcut input (only for up/down)
    bool have_xs = false;
    // The block's 1x1 shortcut Conv_2 (layerspp.py:266-269), where it is its own launch (not folded into Conv_1's launch: the levels
    // below the split kernels' threshold, and any layer the fold's conditions exclude): it needs the block input only and its result only
    // at the end of the block, so at small batches it runs on the side stream beside GroupNorm - Conv_0 - GroupNorm (round 6).
    Tensor sh_t; bool sc_side = false;
    // Does Conv_1's launch take the shortcut?  Asked of Conv_1's own route (it reads the Conv_0 output, the shortcut input's shape, behind
    // GroupNorm_1 + SiLU with a known bound), once per block: the early launch below and the Conv_1 call cannot disagree.
    bool fold = false;
    auto shortcut_early = [&](const Tensor& sa, const Tensor* sb) {
      if (!r.has_c2) return;
      fold = route_of(r.c1, r.c0.cout, 0, sa.H, sa.W, ConvCall{true, true, true, true, false, true}).accepts_shortcut &&
             shortcut_foldable(r.c2, sa, sb) && !((nofold_levels_ >> level_of(sa.H)) & 1);
      if (fold || !side_enabled()) return;
      side_begin();
      sh_t = conv(r.c2, sa, sb, Xform{}, r.c2.bias, nullptr, nullptr, 1.f, ctl);
      side_end();
      sc_side = true;
    };
    if (m.up || m.down) {
      SG_REQUIRE(b == nullptr, "resample block with concat input");
      Tensor hr = fir(a, m.up, x0, &xs);
      have_xs = true;
      shortcut_early(xs, nullptr);
      h = conv(r.c0, hr, nullptr, Xform{nullptr, nullptr, 0, bd0}, nullptr, temb, nullptr, 1.f, ctl, true);
      drop(hr);
    } else {
      shortcut_early(a, b);
      h = conv(r.c0, a, b, x0, nullptr, temb, nullptr, 1.f, ctl, true);
    }
    arena_.release(sc0); arena_.release(sh0);
    gn_coeffs(h, nullptr, r.g1w, r.g1b, &sc1, &sh1, &bd1);
    Xform x1{sc1, sh1, 1, bd1};
    Tensor out;
    const float inv_sqrt2 = 0.70710678118654752440f;
    if (r.has_c2) {
      const Tensor& sa = have_xs ? xs : a;
      const Tensor* sb = have_xs ? nullptr : b;
      if (fold) {
        // (Conv_1(h) + Conv_2(x)) / sqrt 2 as one accumulation: the shortcut's K-stages run inside the 3x3 launch
        const Shortcut scin{&r.c2, &sa, sb};
        out = conv(r.c1, h, nullptr, x1, r.c1.bias, nullptr, nullptr, inv_sqrt2, ctl, true, &scin);
      } else {
        if (sc_side) side_join();                    // (also joins a pyramid branch still pending from the level above)
        else sh_t = conv(r.c2, sa, sb, Xform{}, r.c2.bias, nullptr, nullptr, 1.f, ctl);
        out = conv(r.c1, h, nullptr, x1, r.c1.bias, nullptr, sh_t.p, inv_sqrt2, ctl, true);
        drop(sh_t);
      }
    } else {
      SG_REQUIRE(b == nullptr, "identity shortcut with concat input");
      out = conv(r.c1, h, nullptr, x1, r.c1.bias, nullptr, a.p, inv_sqrt2, ctl, true);
    }
    if (have_xs) drop(xs);
    drop(h);
    arena_.release(sc1); arena_.release(sh1);
    return out;
  }

  // AttnBlockpp.forward (layerspp.py:75-91)
  Tensor attn_block(const Mod& m, Tensor& x, const FwdCtl& ctl) {
    const AttnW& w = attn_.at(m.idx);
    float *sc, *sh;
    gn_coeffs(x, nullptr, w.gw, w.gb, &sc, &sh);
    Tensor qkv = conv(w.qkv, x, nullptr, Xform{sc, sh, 0}, w.qkv.bias, nullptr, nullptr, 1.f, ctl);
    arena_.release(sc); arena_.release(sh);
    Tensor o = new_tensor(x.C, x.H, x.W);
    if (!dry_) {
      AttnArgs aa{qkv.p, o.p, B_, x.C, x.H * x.W, 1.0f / sqrtf((float)x.C), rag_of(x.H), x.H};
      tock();
      SG_REQUIRE(launch_attn_core(aa, stream_), "attention: unsupported channel count");
      if (noting()) snprintf(prof_note_, sizeof prof_note_, "attention C=%d S=%d B=%d", x.C, x.H * x.W, B_);
      tick(TC_ATTN, 4.0 * B_ * (double)x.C * (x.H * x.W) * (double)(x.H * x.W));
    }
    drop(qkv);
    Tensor out = conv(w.proj, o, nullptr, Xform{}, w.proj.bias, nullptr, x.p, 0.70710678118654752440f, ctl, true);
    drop(o);
    return out;
  }

  // ---- side stream (round 6) ---------------------------------------------------------------------------------------------------------
  // Launches that the main chain needs only later -- the output-pyramid branch of a level (run_forward), the 1x1 shortcut of a residual
  // block that is not folded into the block's second 3x3 launch (res_block) -- go to the engine's SECOND STREAM at small batches, where
  // they are latency, not throughput:
  //   side_begin() .. side_end(): the launches in between run on the side stream, ordered behind everything the main stream holds at
  //     side_begin() (an event recorded there); sections may follow each other before a join (the side stream keeps their order);
  //   side_join(): the main stream waits for everything the side stream holds.
  // From the first side_begin() to the join every arena release is DEFERRED (Arena::defer_begin): memory freed on one stream's behalf is
  // not handed to the other stream's later launches while its last user may still run -- in the dry run too, so that the planned arena
  // is the one the real run uses.  Same kernels, same arguments, same bits (test_sampler_graph_equals_eager, the batch-independence and
  // device-memory tests, tools/probes/side_stream_bits_probe.py).  Off above side_max_batch_ utterances (no deferral either: the arena of
  // the large batches is unchanged) and for instrumented evaluations (one stream: profile_forward times launches that follow each other).
  bool side_enabled() const { return side_stream_on_ && B_ <= side_max_batch_; }
  bool side_active() const { return side_enabled() && !prof_ && !dry_ && !drt::is_emulator(); }
  drt::event_t* side_event() {
    if (side_ev_next_ == side_ev_.size()) side_ev_.emplace_back(Event::Order);
    return side_ev_[side_ev_next_++].get();
  }
  void side_begin() {
    SG_REQUIRE(!side_open_, "side stream: nested section");
    side_open_ = true;
    if (!side_enabled()) return;
    if (!side_pending_) arena_.defer_begin();
    if (!side_active()) return;
    if (!side_stream_ready_) { SG_CHECK(drt::stream_create(&side_stream_)); side_stream_ready_ = true; }
    drt::event_t* e = side_event();
    SG_CHECK(drt::event_record(e, stream_));
    SG_CHECK(drt::stream_wait_event(side_stream_, e));
    std::swap(stream_, side_stream_);
    side_swapped_ = true;
  }
  void side_end() {
    SG_REQUIRE(side_open_, "side stream: end without begin");
    side_open_ = false;
    if (!side_enabled()) return;
    side_pending_ = true;
    if (!side_swapped_) return;
    drt::event_t* e = side_event();
    SG_CHECK(drt::event_record(e, stream_));         // (stream_ is the side stream here)
    std::swap(stream_, side_stream_);
    side_swapped_ = false;
    side_join_ev_ = e;                               // (the side stream is in order: its latest event covers the earlier sections)
  }
  void side_join() {
    if (!side_pending_) return;
    side_pending_ = false;
    if (side_join_ev_) { SG_CHECK(drt::stream_wait_event(stream_, side_join_ev_)); side_join_ev_ = nullptr; }
    arena_.defer_end();
  }
  drt::stream_t side_stream_{}; bool side_stream_ready_ = false, side_open_ = false, side_pending_ = false, side_swapped_ = false;
  std::deque<Event> side_ev_; size_t side_ev_next_ = 0; drt::event_t* side_join_ev_ = nullptr;
  bool side_stream_on_ = true; int side_max_batch_ = 8;

  // NCSNpp.forward (ncsnpp.py:256-419) / NCSNpp_48k.forward
  void run_forward(const float2* x, long long xbs, const float2* y, long long ybs, float2* out, int B, int F, int T,
                   const FwdCtl& ctl_in) {
    side_ev_next_ = 0; side_open_ = side_pending_ = false; side_join_ev_ = nullptr;
    try { run_forward_main(x, xbs, y, ybs, out, B, F, T, ctl_in); }
    catch (...) {                 // never leave the engine on its side stream, nor the arena deferring its releases
      if (side_swapped_) { std::swap(stream_, side_stream_); side_swapped_ = false; }
      side_open_ = side_pending_ = false; side_join_ev_ = nullptr;
      arena_.reset();             // (also takes back whatever the failed forward still held)
      throw;
    }
  }
  void run_forward_main(const float2* x, long long xbs, const float2* y, long long ybs, float2* out, int B, int F, int T,
                        const FwdCtl& ctl_in) {
    FwdCtl ctl = ctl_in;
    ctl.bias_step = ctl.step_ptr;
    if (!dry_ && ctl.step_ptr && ctl.bias_table && ctl.bias_bstride == 0 && tot_temb_ > 0) {
      // sampler loop: this step's bias row into a fixed buffer (bias_select_kernel), the convolutions read it without indirection
      DRT_LAUNCH(bias_select_kernel, dim3((tot_temb_ + 255) / 256), dim3(256), stream_, ctl.bias_table, ctl.bias_sstride, ctl.step_ptr,
                 bias_cur_.get(), tot_temb_);
      ctl.bias_table = bias_cur_; ctl.bias_sstride = 0; ctl.bias_step = nullptr;
    }
    B_ = B;
    cur_F_ = F;
    amax_next_ = 0;
    lds_poison_count_ = 0;
    if (!dry_ && poison_ && arena_buf_.capacity()) SG_CHECK(drt::memset_dev(arena_buf_.as<char>(), 0xFF, arena_buf_.capacity(), stream_));
    if (!dry_ && amax_pool_) {
      const int n = amax_slots_ * B * kAmaxSpread;
      DRT_LAUNCH(zero_floats_kernel, dim3((n + 255) / 256), dim3(256), stream_, amax_pool_.get(), n);
    }
    const NetCfg& c = cfg_;
    const int L = c.n_levels;
    size_t mi = 3;
    auto next = [&]() -> const Mod& { SG_REQUIRE(mi < layout_.size(), "layout exhausted"); return layout_[mi++]; };
    const int FT = F * T;
    std::vector<Tensor> hs;
    Tensor xr = new_tensor(4, F, T);
    const bool entry8 = entry_mfma_ && entry8_.packed && layout_[mi].idx == entry8_idx_;
    Tensor xr8{};
    if (entry8) xr8 = new_tensor(entry8_.cin, F, T);   // the same four planes + planes of zeros: one K-stage of the MFMA kernel
    if (!dry_) { tock(); const WrapCoef wc{ctl.coef, ctl.coef_bstride, ctl.coef_sstride, ctl.step_ptr, ctl.sign};
      DRT_LAUNCH(entry_kernel, dim3((FT + 255) / 256, B), dim3(256), stream_, x, xbs, y, ybs, xr.p, entry8 ? xr8.p : (float*)nullptr,
                 entry8 ? entry8_.cin : 0, FT, wc, rag_of(F), F, ctl.y_plane);
      tick(TC_MISC, (32.0 + (entry8 ? 4.0 * entry8_.cin : 0.0)) * B * FT); }
    {
      const Mod& m = next();
      const ConvW& w = entry8 ? entry8_ : conv_.at(m.idx);
      hs.push_back(conv(w, entry8 ? xr8 : xr, nullptr, Xform{}, w.bias, nullptr, nullptr, 1.f, ctl, true));
      if (entry8) drop(xr8);
    }
    Tensor pyr_in = xr;   // input pyramid (ncsnpp.py:293-296); released at the end / when replaced
    bool pyr_in_is_xr = true;
    for (int l = 0; l < L; ++l) {
      for (int rb = 0; rb < c.num_res_blocks; ++rb) {
        const Mod& m = next();
        Tensor h = res_block(m, hs.back(), nullptr, ctl);
        // the reference's forward places attention by the ACTUAL height (ncsnpp.py:308) while its module list was built from the
        // configured image_size (ncsnpp.py:189-193): an input of another height runs off the list there (TypeError); say why
        SG_REQUIRE(cfg_has_attn(c, h.H) == cfg_has_attn(c, c.image_size >> l),
                   "input height does not match the image_size the network was built for (attention placement, ncsnpp.py:308)");
        if (cfg_has_attn(c, h.H)) {
          const Mod& ma = next();
          Tensor h2 = attn_block(ma, h, ctl);
          drop(h);
          h = h2;
        }
        hs.push_back(h);
      }
      if (l != L - 1) {
        const Mod& m = next();
        Tensor h = res_block(m, hs.back(), nullptr, ctl);
        if (c.progressive_input == 1) {
          const Mod& mc = next();
          Tensor np = fir(pyr_in, false, Xform{});
          if (!pyr_in_is_xr) drop(pyr_in);
          pyr_in = np; pyr_in_is_xr = false;
          const ConvW& w = conv_.at(mc.idx);
          Tensor h2 = conv(w, pyr_in, nullptr, Xform{}, w.bias, nullptr, h.p, 1.f, ctl, true);
          drop(h);
          h = h2;
        }
        hs.push_back(h);
      }
    }
    if (!pyr_in_is_xr) drop(pyr_in);
    drop(xr);

    Tensor h = hs.back();   // not popped: still referenced by the skip stack (ncsnpp.py:337)
    {
      const Mod& m1 = next(); Tensor a = res_block(m1, h, nullptr, ctl);
      const Mod& m2 = next(); Tensor b2 = attn_block(m2, a, ctl); drop(a);
      const Mod& m3 = next(); h = res_block(m3, b2, nullptr, ctl); drop(b2);
    }
    Tensor pyramid; bool have_pyr = false;
    for (int l = L - 1; l >= 0; --l) {
      for (int rb = 0; rb < c.num_res_blocks + 1; ++rb) {
        const Mod& m = next();
        Tensor skip = hs.back(); hs.pop_back();
        Tensor o = res_block(m, h, &skip, ctl);
        drop(h); drop(skip);
        h = o;
      }
      SG_REQUIRE(cfg_has_attn(c, h.H) == cfg_has_attn(c, c.image_size >> l),
                 "input height does not match the image_size the network was built for (attention placement, ncsnpp.py:354)");
      if (cfg_has_attn(c, h.H)) {
        const Mod& ma = next();
        Tensor h2 = attn_block(ma, h, ctl);
        drop(h); h = h2;
      }
      if (c.progressive == 1) {
        // The output-pyramid branch of the level (GroupNorm finalize, C -> 4 convolution, 4-channel FIR; ncsnpp.py:358-379) reads h and the
        // previous level's pyramid only and rejoins the main chain at the network's exit: it runs on the engine's SIDE STREAM beside the
        // level's up-sampling block (round 6; small batches, where these launches are latency, not throughput).  Same kernels, same
        // arguments, same bits; the join sits in front of drop(h).
        const Mod& mg = next(); const Mod& mc = next();
        side_begin();
        float *sc, *sh;
        const float* bd;
        gn_coeffs(h, nullptr, gn_.at(mg.idx).first, gn_.at(mg.idx).second, &sc, &sh, &bd);
        const ConvW& w = conv_.at(mc.idx);
        Tensor up; bool have_up = false;
        if (have_pyr) { up = fir(pyramid, true, Xform{}); have_up = true; drop(pyramid); }
        pyramid = conv(w, h, nullptr, Xform{sc, sh, 1, bd}, w.bias, nullptr, have_up ? up.p : nullptr, 1.f, ctl);
        have_pyr = true;
        if (have_up) drop(up);
        arena_.release(sc); arena_.release(sh);
        side_end();
      }
      if (l != 0) {
        const Mod& m = next();
        Tensor o = res_block(m, h, nullptr, ctl);
        side_join();
        drop(h); h = o;
      }
    }
    side_join();
    SG_REQUIRE(hs.empty(), "skip stack not empty");
    Tensor h4;
    if (c.progressive == 1) { h4 = pyramid; drop(h); }
    else {
      const Mod& mg = next(); const Mod& mc = next();
      float *sc, *sh;
      const float* bd;
      gn_coeffs(h, nullptr, gn_.at(mg.idx).first, gn_.at(mg.idx).second, &sc, &sh, &bd);
      const ConvW& w = conv_.at(mc.idx);
      h4 = conv(w, h, nullptr, Xform{sc, sh, 1, bd}, w.bias, nullptr, nullptr, 1.f, ctl);
      arena_.release(sc); arena_.release(sh);
      drop(h);
    }
    SG_REQUIRE(mi == layout_.size(), "forward did not consume every module");
    if (!dry_) {
      ExitArgs ea{h4.p, Wp("output_layer.weight"), Wp("output_layer.bias"), ctl.tvals, ctl.t_bstride, ctl.t_sstride, ctl.step_ptr,
                  c.variant == 1 ? 1 : 0, c.scale_by_sigma,
                  WrapCoef{ctl.coef, ctl.coef_bstride, ctl.coef_sstride, ctl.step_ptr, ctl.sign}, x, xbs, out, FT, rag_of(F), F};
      tock();
      DRT_LAUNCH(exit_kernel, dim3((FT + 255) / 256, B), dim3(256), stream_, ea);
      tick(TC_MISC, 24.0 * B * FT);
      check_launch();
    }
    drop(h4);
  }

  // ONE page-locked staging buffer is the host side of every table upload (upload_tables, the rounds of ode_run), so the copies are
  // asynchronous and a sampler call never synchronises the host with the stream (no hidden host syncs): the caller may
  // already enqueue the next batch's front end while this one samples.  acquire(n) returns n bytes of it once the event recorded
  // behind the previous use's copies has passed (for a new call it has, long before: the copies are the first thing a call
  // enqueues); commit(stream) records that event behind the copies just enqueued on `stream`.
  struct HostStage {
    PinnedArray<char> buf_; Event ev_; bool pending_ = false;
    char* acquire(size_t n) {
      if (pending_) { SG_CHECK(drt::event_sync(ev_.get())); pending_ = false; }
      buf_.ensure(std::max(n, size_t(1) << 16));
      return buf_;
    }
    void commit(drt::stream_t stream) {
      ev_.create();
      SG_CHECK(drt::event_record(ev_.get(), stream));
      pending_ = true;
    }
  } stage_;
  // Per-call sampler constants -> device (through stage_): the step table, the time steps, the score-wrapper rows (may be empty) and
  // the noise table -- seed word + one noise-stream id per utterance (SamplerArgs::seed; ids given by set_noise_streams are consumed
  // by the next sampler call of the same batch size, otherwise utterance b gets stream b), then the noise geometry of the call
  // (take_noise_frames) in the layout SamplerArgs::seed describes.
  const unsigned long long* upload_tables(const std::vector<float>& tab, const std::vector<float>& tv, const std::vector<float>& cf,
                                          unsigned long long seed, int B) {
    SG_REQUIRE(B + 1 <= kMaxStreams, "batch too large for the noise-stream table");
    grow(seed_dev_, (size_t)kMaxStreams * (8 + 12) + 8);      // seed + ids, the geometry flag, three ints per utterance
    const size_t nb_geom = geom_call_.empty() ? 0 : ((size_t)3 * B * 4 + 7) / 8 * 8;
    const size_t nb_seed = ((size_t)B + 2) * 8 + nb_geom, nb_tab = tab.size() * 4, nb_tv = tv.size() * 4, nb_cf = cf.size() * 4;
    char* q = stage_.acquire(nb_seed + nb_tab + nb_tv + nb_cf);
    unsigned long long* hs = reinterpret_cast<unsigned long long*>(q);
    hs[0] = seed;
    const bool given = (int)streams_next_.size() == B;
    for (int b = 0; b < B; ++b) hs[1 + b] = given ? streams_next_[b] : (unsigned long long)b;
    streams_next_.clear();
    hs[1 + B] = nb_geom ? 1ull : 0ull;                        // the noise geometry of this call (take_noise_frames), if any
    if (nb_geom) { hs[1 + B + nb_geom / 8] = 0; memcpy(hs + 2 + B, geom_call_.data(), (size_t)3 * B * 4); }
    geom_call_.clear();
    q += nb_seed;
    memcpy(q, tab.data(), nb_tab); memcpy(q + nb_tab, tv.data(), nb_tv);
    if (nb_cf) memcpy(q + nb_tab + nb_tv, cf.data(), nb_cf);
    SG_CHECK(drt::memcpy_h2d(seed_dev_, hs, nb_seed, stream_));
    SG_CHECK(drt::memcpy_h2d(step_table_, q, nb_tab, stream_));
    SG_CHECK(drt::memcpy_h2d(tsteps_, q + nb_tab, nb_tv, stream_));
    if (nb_cf) SG_CHECK(drt::memcpy_h2d(coef_table_, q + nb_tab + nb_tv, nb_cf, stream_));
    stage_.commit(stream_);
    return seed_dev_.get();
  }
  static constexpr int kMaxStreams = 4096;
  std::vector<unsigned long long> streams_next_;
  std::vector<int> frames_next_;      // pending noise geometry (set_noise_frames): [first_frame x n][total_frames x n]
  std::vector<int> geom_call_;        // ... of the running sampler call, checked: (first_frame, total_frames, T_b) per utterance; empty: default
  DevArray<unsigned long long> seed_dev_;
  DevArray<int> win_tab_;             // window plan of the last spec_split / spec_merge
  int graph_captures_ = 0;

  int device_;
  drt::stream_t stream_;
  NetCfg cfg_;
  std::vector<Mod> layout_;
  std::map<std::string, const float*> W_;
  std::map<int, ResW> res_;
  std::map<int, AttnW> attn_;
  std::map<int, ConvW> conv_;
  std::map<int, std::pair<const float*, const float*>> gn_;
  DenseDesc* dense_descs_ = nullptr; int n_dense_ = 0; int tot_temb_ = 0;
  bool weights_ready_ = false;
  std::vector<DevBuf> wset_;
  std::map<int, DevArray<float2>> twiddles_;

  Arena arena_; DevBuf arena_buf_;
  bool dry_ = false;
  // Runtime switches, re-read from the environment at every configure / weight load (so one process can compare settings).
  // User-facing: SGMSE_CONV_SPLIT, SGMSE_WINO, SGMSE_WINO43, SGMSE_CONV_XCD_MAP, SGMSE_RAGGED_PREFIX, SGMSE_DEBUG_SYNC,
  // SGMSE_PROFILE_DUMP.  Test hooks (what the bitwise / parity tests toggle to reach a code path; not for users):
  // SGMSE_TILE_MIN_BLOCKS, SGMSE_SPLIT_MIN_TILES, SGMSE_WINO_MIN_TILES, SGMSE_FUSE_GN_STATS, SGMSE_POISON, SGMSE_CONV_VARIANT.
  // Everything else that used to be a switch is a constant now: the losing side of each was measured and removed (round 4).
  void read_knobs() {
    auto flag = [](const char* name, bool dflt) { const char* e = getenv(name); return e ? e[0] == '1' : dflt; };
    const char* e = getenv("SGMSE_CONV_SPLIT");          // 0: fp32 MFMA only, 1: bf16x3, 2: fp16x2 (+ Winograd, see SGMSE_WINO) on the wide levels
    split_mode_ = e ? atoi(e) : SGMSE_CONV_SPLIT_DEFAULT;
    SG_REQUIRE(split_mode_ >= 0 && split_mode_ <= 2, "SGMSE_CONV_SPLIT must be 0, 1 or 2");
    wino_ = flag("SGMSE_WINO", true);                    // a Winograd x fp16x2 kernel on the wide levels (0: the direct fp16x2 split kernel there too)
    wino43_ = flag("SGMSE_WINO43", true);                // ... in its F(4,3) form (kernels_conv_wino43.h); 0: the F(2,3) form (kernels_conv_wino.h)
    // ragged convolution launches over the tiles that exist (ConvArgs::rag_cols) and the XCD-aware tile order of the convolution
    // kernels (ConvArgs::xcd_map): both bit-identical, both measured in round 4 (profiles/r04_knobs_ab.txt: ragged batches 1.15 -> 1.04x
    // per frame; +3.5-4 % at T = 512 and T = 448) and on since
    rag_prefix_ = flag("SGMSE_RAGGED_PREFIX", true);
    conv_xcd_map_ = flag("SGMSE_CONV_XCD_MAP", true);
    debug_sync_ = flag("SGMSE_DEBUG_SYNC", false);       // synchronise after every launch of the forward and print its label (stderr)
    prof_dump_ = flag("SGMSE_PROFILE_DUMP", false);      // per-launch lines from profile_forward
    // ---- test hooks
    e = getenv("SGMSE_TILE_MIN_BLOCKS");
    tile_min_blocks_ = e ? atol(e) : 512L;               // workgroups below which a launch takes the smaller tile shape (profiles/r01_tile_sweep.txt)
    e = getenv("SGMSE_SPLIT_MIN_TILES");
    split_min_tiles_ = e ? atol(e) : 8L;                 // per-image 8x32 tiles from which a layer uses a split kernel (profiles/r01_b3_threshold.txt)
    e = getenv("SGMSE_WINO_MIN_TILES");
    wino_min_tiles_ = e ? atol(e) : 32L;                 // ... and the Winograd kernel (32: the 64 x 128 level and up)
    fuse_gn_stats_ = flag("SGMSE_FUSE_GN_STATS", true);  // GroupNorm partial sums in the conv epilogue (0: stand-alone statistics passes)
    lds_poison_ = flag("SGMSE_POISON_LDS", false);       // test hook: NaN patterns in every CU's LDS in front of every launch (lds_poison_kernel)
    e = getenv("SGMSE_POISON_LDS_AT");
    lds_poison_at_ = e ? atoi(e) : -1;                   // ... in front of launch number n only (bisection); SGMSE_POISON_LDS_UPTO=1: launches 0..n
    lds_poison_upto_ = flag("SGMSE_POISON_LDS_UPTO", false);
    side_stream_on_ = flag("SGMSE_SIDE_STREAM", true);   // output-pyramid branches on the second stream (run_forward) ...
    e = getenv("SGMSE_SIDE_MAX_BATCH");
    side_max_batch_ = e ? atoi(e) : 8;                   // ... for batches up to this size (batch 1: -1.4 %, batch 4 / 8: -0.8 %; nothing at 32: profiles/r06_side_stream.txt)
    e = getenv("SGMSE_NOFOLD_LEVELS");
    nofold_levels_ = e ? atoi(e) : 0;                    // measurement (round 6): bit l = the 1x1 shortcuts of U-Net level l as their own launch
    poison_ = flag("SGMSE_POISON", false);               // NaN patterns in every allocation and in the arena before every forward
  }
  // per-forward range-bound slots ([B][kAmaxSpread] floats each), handed out in program order; counted by the dry run
  DevArray<float> amax_pool_; int amax_slots_ = 0, amax_next_ = 0;
  float* next_amax() {
    const int i = amax_next_++;
    // dry run: a fake address (never dereferenced), non-null so that the kernel-family decisions that ask "is the bound known?"
    // come out as in the real run and the arena is sized for the launches that will really happen
    if (dry_) return reinterpret_cast<float*>(uintptr_t(1) << 43) + (size_t)i * kAmaxSpread;
    SG_REQUIRE(amax_pool_ && i < amax_slots_, "range-bound pool smaller than the forward needs");
    return amax_pool_ + (size_t)i * B_ * kAmaxSpread;
  }
  long tile_min_blocks_ = 512, split_min_tiles_ = 8;
  // (settled in rounds 2-3, switches removed in round 4: chunked accumulation of the coarse fp32 layers, shortcuts folded into the 3x3
  //  launches, chunked 4-row fp16x2 kernel on the 16 x 32 / 32 x 64 levels, entry convolution on the MFMA kernel)
  static constexpr bool coarse_chunked_ = true, fold_shortcut_ = true, coarse_split_ = true, entry_mfma_ = true;
  ConvW entry8_{}; int entry8_idx_ = -1;
  bool poison_ = false, debug_sync_ = false, conv_xcd_map_ = true, rag_prefix_ = true, wino_ = true, wino43_ = true;
  long wino_min_tiles_ = 32;
  int nofold_levels_ = 0;
  bool lds_poison_ = false, lds_poison_upto_ = false; int lds_poison_at_ = -1, lds_poison_count_ = 0; DevArray<unsigned> lds_sink_;
  static constexpr long coarse_splitk_div_ = 4, chunk_max_tiles_ = 8;      // (profiles/r02_chunk_splitk.txt)
  int split_mode_ = SGMSE_CONV_SPLIT_DEFAULT;
  bool prof_dump_ = false;
  char prof_note_[160] = {0};
  static constexpr bool fir_scalar_ = false;      // (per-pixel FIR kernels everywhere: a round-1 measurement switch)
  bool fuse_gn_stats_ = true;
  int B_ = 0, shape_B_ = 0, shape_F_ = 0, shape_T_ = 0;
  DevArray<float2> sx_, sxm_, sscore_, sy_;
  DevArray<int> step_ctr_;
  DevArray<float> lang_partial_, lang_scal_;
  DevArray<float> bias_cur_, temb_act_, bias_table_, step_table_, tsteps_, coef_table_; int temb_rows_ = 0;
  drt::graph_t graph_{}; bool graph_valid_ = false; GraphKey graph_key_{};
  int nfe_ = 0;
  // adaptive ODE sampler (ode_run): slopes K_0..K_6, stage input; scalar table, reduction buffers and the pinned results for the
  // largest number of groups so far; last run's controllers (one per group) and round statistics
  DevArray<float2> ode_k_[7], ode_xs_;
  static constexpr int kOdeEachMaxB = 1024;
  DevArray<double> ode_table_, ode_partial_, ode_result_; PinnedArray<double> ode_host_;
  std::vector<OdeControl> ode_ctl_; int ode_rounds_ = 0, ode_wasted_ = 0;
  bool prof_ = false; std::vector<ProfRec> prof_recs_; size_t prof_used_ = 0; float prof_ms_[TC_COUNT]; double prof_flops_[TC_COUNT]; int prof_n_[TC_COUNT];
};

}  // namespace sgmse
