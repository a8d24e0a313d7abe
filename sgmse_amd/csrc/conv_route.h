// Which kernel family a convolution runs on, and in which shape: decided HERE, once, before anything is allocated or launched.
// Host-only and pure (no HIP, no engine state): Engine::conv() launches what conv_route() returns, Engine::res_block() asks the same
// function whether Conv_1's launch takes the block's 1x1 shortcut.  The kernels are in kernels_conv*.h, their launchers in conv_launch.h.
#pragma once
#include <algorithm>

namespace sgmse {

// ---- shape conditions of the kernel families ---------------------------------------------------------------------------------------
// split-operand convolutions (kernels_conv_split.h)
inline bool conv_split_eligible(int ks, int C1, int C2, int Cout) {
  return (ks == 3 || ks == 1) && Cout % 128 == 0 && (C1 + C2) % 16 == 0 && (C2 == 0 || C1 % 16 == 0) && (C1 + C2) <= 512;
}
// thin 3x3 layers (the C->4 pyramid convolutions): one zero-padded 32-channel fragment, the waves split the pixels
inline bool conv_thin_split_eligible(int ks, int C1, int C2, int Cout) {
  return ks == 3 && Cout <= 32 && (C1 + C2) >= 64 && (C1 + C2) % 16 == 0 && (C2 == 0 || C1 % 16 == 0) && (C1 + C2) <= 512;
}
// rows per GroupNorm-statistics sub-tile the split kernels emit for this layer (ConvArgs::stats_rows): 4, except the thin shape
// (two rows per wave; its layers emit no statistics in the network)
inline int conv_split_stats_rows(int ks, int Cout) { return (ks == 3 && Cout <= 32) ? 1 : 4; }
// Winograd F(2,3) x fp16x2 (kernels_conv_wino.h; also the channel conditions of the 2-D form, kernels_conv_wino2d.h): aligned column pairs
inline bool conv_wino_eligible(int C1, int C2, int Cout, int W) {
  return Cout % 128 == 0 && (C1 + C2) % 16 == 0 && (C2 == 0 || C1 % 16 == 0) && (C1 + C2) <= 512 && W % 2 == 0;
}
// Winograd F(4,3) x fp16x2 (kernels_conv_wino43.h): aligned column quads
inline bool conv_wino43_eligible(int C1, int C2, int Cout, int W) {
  return Cout % 128 == 0 && (C1 + C2) % 16 == 0 && (C2 == 0 || C1 % 16 == 0) && (C1 + C2) <= 512 && W % 4 == 0;
}
// exact-fp32 VALU kernel of the C -> 4 pyramid convolutions (kernels_conv_thin.h; kConvThinKC = its channels per stage)
constexpr int kConvThinKC = 4;
inline bool conv_thin_eligible(int ks, int C1, int C2, int Cout) {
  return ks == 3 && Cout <= 4 && (C1 + C2) % kConvThinKC == 0 && (C2 == 0 || C1 % kConvThinKC == 0) && (C1 + C2) <= 512;
}

// The Winograd x fp16x2 forms.  An engine packs ONE of F23 / F43 for its wide 3x3 layers (Engine::make_conv); F2x2 is reachable through
// the op-level entry points only.
enum class WinoForm { F23, F43, F2x2 };

enum class ConvFamily { Direct, Mfma, Split, SplitCoarse, Wino23, Wino43, Thin };

struct ConvLayer {          // the layer: shape, the packings that exist, the engine's split mode and Winograd form
  int ks, C1, C2, cout, co_t;
  bool packed, packed32, packed_thin, packed_split, packed_wino;
  int split_mode;           // 1 bf16x3, 2 fp16x2 (0: no split layout)
  WinoForm wino_form;
};
struct ConvLevel { int H, W, dec_W, level; };     // W: the actual (widest) width; dec_W / level: the U-Net level (Engine::dec_W, level_of)
struct ConvCall {           // what this call brings
  bool bound_known;         // Xform::bound: the bound of the GroupNorm producer's output
  bool amax_known;          // range bounds of the raw inputs
  bool scale_present;       // Xform::scale: a fused producer
  bool emit_stats, bias2;
  bool fold_requested;      // a residual shortcut to fold into this launch
};
struct ConvKnobs {          // Engine::read_knobs and the engine's settled constants
  long tile_min_blocks, split_min_tiles, wino_min_tiles;
  bool wino, fuse_gn_stats;
  long chunk_max_tiles, coarse_splitk_div;
  bool coarse_chunked, coarse_split;
};

struct ConvRoute {
  ConvFamily family = ConvFamily::Direct;
  int co_t = 0, rows = 8;   // Mfma: the tile
  bool rows4 = false;       // split and Winograd families: the 4-row workgroup shape
  int kchunk = 0;           // K-stages per accumulation chunk (0: unchunked)
  int ksplit = 1;           // > 1: the chunks spread over gridDim.z (split-K; needs a partial-sum buffer)
  int srows = 1;            // image rows per GroupNorm-statistics sub-tile of the output (Tensor::srows)
  bool accepts_shortcut = false;   // fold_requested, and this launch takes the folded 1x1
};

inline ConvRoute conv_route(const ConvLayer& w, const ConvLevel& lv, const ConvCall& c, int B, const ConvKnobs& k) {
  ConvRoute r;
  const int Cin = w.C1 + w.C2, H = lv.H, W = lv.W;
  const int kc = (w.ks == 3) ? 8 : 32;
  const bool use_mfma = w.packed && (w.C2 == 0 || w.C1 % kc == 0);
  // tile choice: the most efficient tile (widest channel block, 8 rows) that still gives the chip enough workgroups
  // (tile_min_blocks, 2 per CU), falling back towards 32 channels x 4 rows for the coarse U-Net levels and for small
  // batches.  All tile shapes accumulate every output in the same order and emit the same per-row GroupNorm partials
  // (kernels_conv.h), so the choice -- and with it the batch size -- never changes a result bit.
  r.co_t = w.co_t; r.rows = H >= 8 ? 8 : 4;
  if (use_mfma) {
    const int cand_co[2] = {w.co_t, w.packed32 ? 32 : w.co_t};
    long best = -1;
    bool done = false;
    for (int ci = 0; ci < 2 && !done; ++ci)
      for (int rows = (H >= 8 ? 8 : 4); rows >= 4 && !done; rows -= 4) {
        if (ci == 1 && cand_co[1] == cand_co[0]) break;
        const long nblk = (long)B * ((H + rows - 1) / rows) * ((W + 31) / 32) * ((w.cout + cand_co[ci] - 1) / cand_co[ci]);
        if (nblk > best) { best = nblk; r.co_t = cand_co[ci]; r.rows = rows; }
        if (nblk >= k.tile_min_blocks) done = true;
      }
  }
  // fp32-accurate bf16x3 kernel for the wide levels.  Decided per layer and per LEVEL (never by the batch size or the utterance length), because
  // its results differ from the fp32-MFMA kernels in the last bits and an utterance must not depend on its batch.
  const int Wd = lv.dec_W;            // family decisions by the level, not by the utterance length (see Engine::dec_W)
  const long tiles8 = (long)((H + 7) / 8) * ((Wd + 31) / 32);
  // Levels with at most chunk_max_tiles tiles per nominal image (32 x 64 and below): the fp16x2 split kernel in its 4-row shape with
  // CHUNKED accumulation, so that a small batch can spread the chunks over workgroups (split-K, bit-identical) instead of running 16-32
  // serial stages on 8-32 workgroups; full 3x3 blocks behind a GroupNorm producer only (not the launches with a folded
  // shortcut).  Decided per layer and level, never by the batch or the utterance length: chunking fixes the summation order.
  // The 8 x 16 and 4 x 8 levels joined in round 4: their tiles are half / three quarters empty, yet at batch 32 the layers take 0.057 /
  // 0.038 ms against 0.115 / 0.065 ms on the fp32 kernels (+1.7 % utterances/s); a single utterance pays 9 us per layer for the
  // four times wider output tile of a workgroup (434 -> 452 ms per utterance at batch 1; profiles/r04_coarse_levels.txt).
  const bool coarse_split = k.coarse_split && use_mfma && w.packed_split && w.split_mode == 2 && w.ks == 3 && w.cout > 32 && !c.fold_requested &&
                            conv_split_eligible(3, w.C1, w.C2, w.cout) && tiles8 <= k.chunk_max_tiles && c.bound_known;
  const bool use_split = coarse_split || (use_mfma && w.packed_split &&
                      (conv_split_eligible(w.ks, w.C1, w.C2, w.cout) || conv_thin_split_eligible(w.ks, w.C1, w.C2, w.cout)) &&
                      tiles8 >= k.split_min_tiles &&
                      // fp16x2: 3x3 layers scale by the bound of their GroupNorm producer's output, 1x1 layers read the
                      // raw residual stream and scale by the producers' range bounds; either must be known
                      (w.split_mode != 2 || (w.ks == 3 ? c.bound_known : (!c.scale_present && c.amax_known))));
  // The wide levels (>= wino_min_tiles tiles per nominal image: 64 x 128 and up) run the full 3x3 blocks on a Winograd x
  // fp16x2 kernel: F(4,3) along the frame axis (kernels_conv_wino43.h: half of the matrix work of the direct split kernel, which is bound by the
  // energy of its MFMAs) or, under SGMSE_WINO43=0, F(2,3) (kernels_conv_wino.h: 2/3).  One form per engine: only its weights are packed.
  // Decided per layer and level like every kernel family; its 4-row shape (launches that cannot fill the chip) gives the same bits.
  // (F(2,3) stages aligned column pairs: frame counts are multiples of 64, so every utterance's width is even down to level 5)
  // The F(4,3) form stages aligned column QUADS: frame counts are multiples of 64, so every utterance's width is a multiple of 4 down to
  // level 4 -- where SGMSE_WINO_MIN_TILES lets Winograd reach level 5, an engine that holds the F(4,3) packing runs that level on the
  // direct split kernel (the level condition below), so conv()'s width requirement cannot fail for a width the F(2,3) form would have taken.
  const bool f43 = w.wino_form == WinoForm::F43;
  const bool use_wino = use_split && !coarse_split && k.wino && w.packed_wino && w.ks == 3 && w.split_mode == 2 && c.bound_known &&
                        conv_wino_eligible(w.C1, w.C2, w.cout, 2) && lv.level <= (f43 ? 4 : 5) && tiles8 >= k.wino_min_tiles;
  if (coarse_split) {
    const int nstages = Cin / 16;
    r.kchunk = std::max(2, (nstages + 7) / 8);
    const int nchunks = (nstages + r.kchunk - 1) / r.kchunk;
    const long nblk = (long)B * ((H + 3) / 4) * ((W + 31) / 32) * (w.cout / 128);
    if (nchunks > 1 && nblk * k.coarse_splitk_div <= k.tile_min_blocks) r.ksplit = nchunks;
  }
  // Coarse levels (at most 512 pixels per nominal image) on the fp32 kernels: 32-channel tiles with CHUNKED accumulation (decided per
  // layer and image, never by the batch: it fixes the summation order), and -- when even those tiles leave most CUs idle
  // (small batches) -- the chunks spread over workgroups (split-K, bit-identical): a K loop of 32-64 serial stages was the
  // latency of these launches (60-120 us each at batch 1, profiles/r02_prof_dump_b1_per_launch.txt)
  if (use_mfma && !use_split && k.coarse_chunked && (long)H * Wd <= 512 && (w.co_t == 32 || w.packed32)) {
    r.co_t = 32;
    const long nblk8 = (long)B * ((H + 7) / 8) * ((W + 31) / 32) * ((w.cout + 31) / 32);
    r.rows = (H >= 8 && nblk8 >= k.tile_min_blocks) ? 8 : 4;
    const int nstages = Cin / kc;
    r.kchunk = std::max(w.ks == 3 ? 4 : 2, (nstages + 7) / 8);
    const int nchunks = (nstages + r.kchunk - 1) / r.kchunk;
    const long nblk = (long)B * ((H + r.rows - 1) / r.rows) * ((W + 31) / 32) * ((w.cout + 31) / 32);
    if (nchunks > 1 && nblk * 2 <= k.tile_min_blocks) r.ksplit = nchunks;
  }
  // the split kernels emit one partial pair per 4 image rows, the fp32 kernels one per row (ConvArgs::stats_rows): a property
  // of the kernel family, which is a property of the layer and level
  if (c.emit_stats && k.fuse_gn_stats && use_split) r.srows = conv_split_stats_rows(w.ks, w.cout);
  // 4-row workgroups when 8-row ones would leave CUs idle (bit-identical results, so this may follow the batch size)
  // (Winograd: one 512-thread workgroup per CU, the 8-row shape from two rounds of the chip)
  const long nblk8 = (long)B * ((H + 7) / 8) * ((W + 31) / 32) * ((w.cout + 127) / 128);
  r.rows4 = use_split && (coarse_split || nblk8 < k.tile_min_blocks);
  // the C -> 4 convolutions of the output pyramid: exact-fp32 VALU kernel (kernels_conv_thin.h) -- on the matrix pipe
  // seven eighths of their work was padding (decided by the layer's shape and U-Net level alone: never by batch or utterance length)
  // (the two finest levels: below them a launch at batch 1 has few 16 x 64 tiles and their 32-64 serial stages are slower than the MFMA path's split-K)
  // (conv3x3_thin_kernel has no time-embedding row, accumulator scale or folded shortcut: a layer that carries one stays on the MFMA shapes)
  const bool use_thin = w.packed_thin && conv_thin_eligible(w.ks, w.C1, w.C2, w.cout) && !c.emit_stats && lv.level <= 1 && !c.bias2 && !c.fold_requested;
  r.family = use_thin ? ConvFamily::Thin
           : use_wino ? (f43 ? ConvFamily::Wino43 : ConvFamily::Wino23)
           : coarse_split ? ConvFamily::SplitCoarse
           : use_split ? ConvFamily::Split
           : use_mfma ? ConvFamily::Mfma : ConvFamily::Direct;
  // A folded residual shortcut (Conv_1(h) + Conv_2(x) as one accumulation): the fp16x2 full-block 3x3 kernels behind a fused producer,
  // direct split or Winograd F(2,3).  F(4,3) has no folded shortcut: res_block() keeps the 1x1 its own launch on its levels.
  r.accepts_shortcut = c.fold_requested && (r.family == ConvFamily::Split || r.family == ConvFamily::Wino23) && w.ks == 3 &&
                       w.split_mode == 2 && w.cout > 32 && c.scale_present;
  return r;
}

}  // namespace sgmse
