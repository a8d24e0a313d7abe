// Stand-alone lifetime check of sgmse::Engine's memory management on the CPU emulator runtime (TEST INFRASTRUCTURE ONLY).
//
// Built with -fsanitize=address (make -C sgmse_amd/csrc lifetime) and run in its own process (tests/test_engine_lifetime.py): walks
// every path of the engine that allocates, grows, re-allocates or releases a buffer -- shape growth, ragged tables built twice, a
// weight reload, the fixed-step and adaptive samplers, the op-level entry points with their scoped scratch (one of them throwing),
// the measurement entry points -- and destroys the engine.  Pass: exit status 0 and no sanitizer report (invalid access, or leak
// at exit).
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "engine.h"

namespace {

// "device" memory of the emulator: plain host memory, 256-byte aligned as the runtime's own allocations
struct Mem {
  float* p;
  explicit Mem(size_t nfloats, float scale = 1.f, unsigned seed = 1) {
    p = static_cast<float*>(aligned_alloc(256, (nfloats * 4 + 255) / 256 * 256));
    unsigned h = seed * 2654435761u + 12345u;
    for (size_t i = 0; i < nfloats; ++i) { h = h * 1664525u + 1013904223u; p[i] = scale * ((float)(h >> 8) * (2.0f / 16777216.0f) - 1.0f); }
  }
  ~Mem() { free(p); }
  Mem(const Mem&) = delete;
  Mem& operator=(const Mem&) = delete;
  const float2* c() const { return reinterpret_cast<const float2*>(p); }
  float2* c() { return reinterpret_cast<float2*>(p); }
};

void load(sgmse::Engine& e, unsigned seed) {
  const auto manifest = sgmse::param_manifest(e.config());
  std::vector<std::vector<float>> vals;
  std::vector<const char*> names;
  std::vector<const void*> ptrs;
  std::vector<long long> numels;
  unsigned h = seed;
  for (const auto& kv : manifest) {
    std::vector<float> v(kv.second);
    const bool gain = kv.first.find("GroupNorm") != std::string::npos && kv.first.find("weight") != std::string::npos;
    for (float& x : v) { h = h * 1664525u + 1013904223u; x = (gain ? 1.f : 0.f) + 0.05f * ((float)(h >> 8) * (2.0f / 16777216.0f) - 1.0f); }
    vals.push_back(std::move(v));
  }
  for (size_t i = 0; i < manifest.size(); ++i) {
    names.push_back(manifest[i].first.c_str()); ptrs.push_back(vals[i].data()); numels.push_back((long long)manifest[i].second);
  }
  e.load_weights(names.data(), ptrs.data(), numels.data(), (int)names.size(), /*on_device=*/0);
}

#define STEP(what) do { fprintf(stderr, "[lifetime] %s\n", what); fflush(stderr); } while (0)

}  // namespace

int main() {
  using sgmse::Engine;
  constexpr int F = 64, T = 64;
  {
    Engine e(0, nullptr);
    sgmse::NetCfg cfg;
    cfg.nf = 32; cfg.n_levels = 4; cfg.num_res_blocks = 1; cfg.image_size = 64; cfg.n_attn = 1;
    const int cm[8] = {1, 1, 2, 2, 0, 0, 0, 0}, ar[8] = {16, 0, 0, 0, 0, 0, 0, 0};
    for (int i = 0; i < 8; ++i) { cfg.ch_mult[i] = cm[i]; cfg.attn_res[i] = ar[i]; }
    e.set_config(cfg);
    STEP("load weights");
    load(e, 1);

    Mem xy((size_t)2 * 2 * F * 2 * T * 2, 0.5f, 2), out((size_t)2 * F * 2 * T * 2), tt(2, 0.f);
    tt.p[0] = 0.6f; tt.p[1] = 0.3f;
    STEP("forward B = 1, B = 2");
    e.forward_xy(xy.c(), tt.p, out.c(), 1, F, T);
    e.forward_xy(xy.c(), tt.p, out.c(), 2, F, T);
    STEP("ragged {64, 128}, {128, 64}, uniform again");
    const int fa[2] = {64, 128}, fb[2] = {128, 64};
    e.set_ragged_frames(fa, 2);
    e.forward_xy(xy.c(), tt.p, out.c(), 2, F, 128);
    e.set_ragged_frames(fb, 2);
    e.forward_xy(xy.c(), tt.p, out.c(), 2, F, 128);
    e.set_ragged_frames(nullptr, 0);
    STEP("load weights again");
    load(e, 7);

    {
      STEP("PC sampler, N = 2; fixed-step probability-flow sampler, N = 2");
      const float t[2] = {1.0f, 0.5f}, dt[2] = {0.5f, 0.5f}, G[2] = {0.4f, 0.2f}, G2[2] = {0.16f, 0.04f}, eps[2] = {1e-3f, 1e-3f}, an[2] = {0.04f, 0.04f};
      sgmse_sampler_cfg sc{};
      sc.N = 2; sc.corrector = 1; sc.corrector_steps = 1; sc.predictor = 1; sc.denoise = 1; sc.theta = 1.5f; sc.std1 = 0.5f;
      sc.t = t; sc.dt = dt; sc.G = G; sc.G2 = G2; sc.ald_eps = eps; sc.ald_noise = an; sc.snr = 0.5f;
      e.pc_sample(xy.c(), out.c(), 1, F, T, sc, nullptr, 11ull);
      sc.corrector = 0; sc.corrector_steps = 0; sc.probability_flow = 1;
      e.pc_sample(xy.c(), out.c(), 1, F, T, sc, nullptr, 12ull);
    }
    {
      STEP("adaptive sampler: one group at B = 1, per utterance at B = 2");
      sgmse_ode_cfg oc{};
      oc.theta = 1.5f; oc.sigma_min = 0.05f; oc.sigma_max = 0.5f; oc.std1 = 0.5f; oc.t_end = 1.0; oc.eps = 0.5;
      oc.rtol = 1e6; oc.atol = 1e6;                // every attempted step is accepted ...
      oc.first_step = 0.5; oc.max_step = 0.0;      // ... and the first one spans the interval: f0 and one round
      oc.max_nfe = 100;
      e.ode_run(xy.c(), out.c(), 1, F, T, oc, nullptr, nullptr, 21ull, false);
      e.ode_run(xy.c(), out.c(), 2, F, T, oc, nullptr, nullptr, 22ull, true);
    }
    {
      STEP("op_stft at two n_fft");
      Mem sig(4096), win(512), spec((size_t)2 * 257 * 64);
      e.op_stft(sig.p, win.p, spec.c(), 1, 4096, 510, 128);
      e.op_stft(sig.p, win.p, spec.c(), 1, 4096, 256, 64);
    }
    {
      STEP("op_groupnorm");
      Mem x((size_t)32 * 8 * 32), g(32), b(32), o((size_t)32 * 8 * 32);
      e.op_groupnorm(x.p, g.p, b.p, o.p, 1, 32, 8, 32, 1, nullptr, 0);
    }
    {
      STEP("op_conv2d, every ForceConv value");
      constexpr int H = 8, W = 32;
      Mem x((size_t)64 * H * W, 1.f, 3), w((size_t)128 * 16 * 9, 0.1f, 4), wt((size_t)4 * 64 * 9, 0.1f, 5), w1((size_t)128 * 16, 0.1f, 6);
      Mem sc(16, 1.f, 7), sh(16, 1.f, 8), o((size_t)128 * H * W);
      for (int fc : {Engine::FC_AUTO, Engine::FC_DIRECT, Engine::FC_SPLIT_B3, Engine::FC_SPLIT_H2, Engine::FC_WINO, Engine::FC_WINO_4ROW,
                     Engine::FC_WINO2D, Engine::FC_WINO43, Engine::FC_WINO43_4ROW})
        e.op_conv2d(x.p, w.p, nullptr, nullptr, o.p, 1, 16, 128, H, W, 3, 1.f, fc, sc.p, sh.p, 1, nullptr, 0);
      e.op_conv2d(x.p, wt.p, nullptr, nullptr, o.p, 1, 64, 4, H, W, 3, 1.f, Engine::FC_THIN, nullptr, nullptr, 0, nullptr, 0);
      e.op_conv2d(x.p, w1.p, nullptr, nullptr, o.p, 1, 16, 128, H, W, 1, 1.f, Engine::FC_SPLIT_H2, nullptr, nullptr, 0, nullptr, 0);      // raw 1x1
      e.op_conv2d(x.p, w1.p, nullptr, nullptr, o.p, 1, 16, 128, H, W, 1, 1.f, Engine::FC_SPLIT_H2, sc.p, sh.p, 1, nullptr, 0);            // 1x1 behind a producer
      STEP("op_conv2d on an ineligible shape");
      bool threw = false;
      try { e.op_conv2d(x.p, w.p, nullptr, nullptr, o.p, 1, 16, 128, H, 30, 3, 1.f, Engine::FC_WINO43, sc.p, sh.p, 1, nullptr, 0); }
      catch (const sgmse::EngineError& err) { threw = true; fprintf(stderr, "[lifetime]   (expected) %s\n", err.what()); }
      if (!threw) { fprintf(stderr, "[lifetime] op_conv2d accepted an ineligible shape\n"); return 1; }
    }
    STEP("bench_conv: fp32, split, Winograd; calib_stream");
    e.bench_conv(3, 1, 16, 128, 8, 32, 0, 1, 1);
    e.bench_conv(3, 1, 16, 128, 8, 32, 128, 1, 1);
    e.bench_conv(3, 1, 16, 128, 8, 32, 128 | 1024, 1, 0);
    e.calib_stream(0, 8, 4096);
    e.calib_stream(1, 16, 4096);
    e.sync();
    STEP("destroy the engine");
  }
  fprintf(stderr, "[lifetime] done\n");
  return 0;
}
