/* sgmse_hip.h — C ABI of libsgmse_hip.so, the MI355X (gfx950) implementation of the reverse-SDE enhancement
 * sampler of sp-uhh/sgmse.
 *
 * The reference has no C ABI of its own; its native boundary is one pybind11 function
 * (sgmse/backbones/ncsnpp_utils/op/upfirdn2d.cpp:12-23) and everything else on the hot path is torch calls from
 * Python.  Each entry point below names the reference interface it replaces (paths relative to the upstream tree).
 *
 * Conventions
 *   - all pointers are caller-owned DEVICE pointers unless the parameter comment says "host";
 *   - complex tensors are interleaved (re, im) fp32 pairs == torch.complex64 storage;
 *   - tensors are dense and contiguous in the index order written in the comment;
 *   - work is enqueued on the context's stream (the caller's current HIP stream); only the functions marked
 *     "synchronises" wait for it;
 *   - return 0 on success, a negative sgmse_status otherwise; sgmse_last_error(ctx) gives the message.  The Python
 *     host layer re-raises SGMSE_EINVAL as ValueError and the rest as RuntimeError (reference: TORCH_CHECK ->
 *     RuntimeError, upfirdn2d.cpp:8-16; registry ValueError, util/registry.py:30).
 *   - a context is not re-entrant; use one per (device, stream).
 */
#ifndef SGMSE_HIP_H
#define SGMSE_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sgmse_ctx sgmse_ctx;

typedef enum { SGMSE_OK = 0, SGMSE_EINVAL = -1, SGMSE_ERUNTIME = -2, SGMSE_ENOTREADY = -3 } sgmse_status;

/* Constructor arguments of NCSNpp that change the graph (sgmse/backbones/ncsnpp.py:50-72,
 * ncsnpp_48k.py:50-72).  Fixed by this implementation, as in every shipped checkpoint: resblock_type='biggan',
 * fir=True, fir_kernel=[1,3,3,1], skip_rescale=True, resamp_with_conv=True (unused with biggan blocks),
 * combine_method='sum', embedding_type='fourier', conditional=True, centered=True, nonlinearity='swish',
 * init_scale=0, dropout=0. */
typedef struct {
  int variant;            /* 0: "ncsnpp" (ncsnpp.py) and, with scale_by_sigma = 0, "ncsnpp_v2" (ncsnpp_v2.py: same network, no /t);
                             1: "ncsnpp_48k" (ncsnpp_48k.py: output_layer before /t) */
  int nf;                 /* base width (128) */
  int n_levels;           /* len(ch_mult) (7) */
  int ch_mult[8];         /* (1,1,2,2,2,2,2) */
  int num_res_blocks;     /* 2 */
  int n_attn;             /* len(attn_resolutions) */
  int attn_res[8];        /* (16,) ; () for ncsnpp_48k */
  int image_size;         /* 256 */
  int progressive;        /* 0 'none', 1 'output_skip' */
  int progressive_input;  /* 0 'none', 1 'input_skip' */
  int scale_by_sigma;     /* 1 */
} sgmse_net_cfg;

/* One call of get_pc_sampler(...)() (sgmse/sampling/__init__.py:26-70).  The per-step scalars are HOST arrays of
 * length N computed by the caller with the reference's own fp32 expressions (sgmse/sdes.py:188-219,
 * sampling/__init__.py:56-62, correctors.py:77-79): t = linspace(T, eps, N); dt[i] = t[i]-t[i+1], dt[N-1] = t[N-1];
 * ald_eps = 2 (snr std(t))^2; ald_noise = sqrt(2 ald_eps); G = g(t) sqrt(dt); G2 = G^2. */
typedef struct {
  int N;
  int corrector;          /* 0 'none' (correctors.py:85-94), 1 'ald' (correctors.py:60-81), 2 'langevin' (correctors.py:37-56:
                             step size from batch-mean norms of score and noise; refused by a ragged context), 3 'langevin' with the
                             step size PER UTTERANCE, 2 (snr ||z_b|| / ||score_b||)^2: utterance b gets what value 2 gives it in a
                             batch of its own (the reference's one-file-at-a-time loop), uniform and ragged batches */
  int corrector_steps;
  int predictor;          /* 0 'none', 1 'reverse_diffusion' (predictors.py:56-65) */
  int probability_flow;   /* 1: fixed-step PF-ODE Euler step (sdes.py:130-135 with probability_flow=True), no noise */
  int denoise;            /* 1: return x_mean of the last step (sampling/__init__.py:66) */
  float theta;            /* OUVESDE.theta */
  float std1;             /* OUVESDE._std(T=1) for prior_sampling (sdes.py:224-229) */
  const float* t; const float* dt; const float* ald_eps; const float* ald_noise; const float* G; const float* G2;
  /* ScoreModel.forward as an affine wrapper of the backbone output F (model.py:284-310): the network sees in_scale*x_t and
   * in_scale*y, score = score_alpha*x_t + score_beta*F.  Host arrays [N], all three or all NULL.  NULL = old-code branch
   * (model.py:307-310): in_scale 1, alpha 0, beta -1.  ncsnpp_v2 models: in_scale = c_in(t); 'score_matching': alpha =
   * c_skip(t), beta = c_out(t)*s(t); 'denoiser': alpha = -1/std(t)^2, beta = s(t)/std(t)^2; s = network_scaling. */
  const float* in_scale; const float* score_alpha; const float* score_beta;
  float snr;              /* 'langevin' only: r in step = 2 (r * mean||z|| / mean||score||)^2; corrector 3: the utterance's own norms
                             ('ald' has it folded into ald_eps) */
  int use_graph;          /* 1: capture one predictor-corrector step as a hipGraph and replay it N times */
} sgmse_sampler_cfg;

/* -- context ------------------------------------------------------------------------------------------------ */
int sgmse_ctx_create(int device, void* hip_stream, sgmse_ctx** out);
void sgmse_ctx_destroy(sgmse_ctx* ctx);
int sgmse_set_stream(sgmse_ctx* ctx, void* hip_stream);
int sgmse_sync(sgmse_ctx* ctx);                      /* synchronises */
const char* sgmse_last_error(sgmse_ctx* ctx);
const char* sgmse_backend(void);                     /* "hip-gfx950" for the product library */

/* -- model: replaces BackboneRegistry.get_by_name(name)(**kwargs) + load_state_dict (model.py:60-61,100-106) -- */
/* Accepts nf in {32, 64, ..., 256}, 1-8 levels with nf * ch_mult[l] <= 256, num_res_blocks >= 1, up to 8 attention resolutions, both
 * pyramids on or off, both variants.  Every attention block (the bottleneck's and those of attn_res) must stand at 32, 64, 128, 192 or
 * 256 channels: anything else is SGMSE_EINVAL here, with the level's resolution and channel count in sgmse_last_error. */
int sgmse_configure(sgmse_ctx* ctx, const sgmse_net_cfg* cfg);
/* names = the reference state_dict keys of the backbone ("output_layer.weight", "all_modules.3.weight", ...;
 * ncsnpp.py:105,253), fp32, shapes as in the reference; every key of the configured network must be present.
 * ptrs are host pointers (on_device = 0; synchronises) or device pointers (on_device = 1, e.g. the buffer an RCCL
 * broadcast just filled). */
int sgmse_load_weights(sgmse_ctx* ctx, const char* const* names, const void* const* ptrs, const long long* numels,
                       int n, int on_device);
int sgmse_param_count(sgmse_ctx* ctx, long long* out);

/* -- NCSNpp.forward(x, time_cond) (ncsnpp.py:256-419; ncsnpp_48k.py:260-424) ---------------------------------
 * xy: complex64 [B][2][F][T] (channel 0 = x_t, 1 = y); t: fp32 [B]; out: complex64 [B][1][F][T]. */
int sgmse_ncsnpp_forward(sgmse_ctx* ctx, const void* xy, const float* t, void* out, int B, int F, int T);

/* -- get_pc_sampler(...)() (sampling/__init__.py:52-68) with score_fn = ScoreModel.forward (model.py:307-310) --
 * Y, out: complex64 [B][1][F][T].  noise: complex64 [1 + N*draws_per_step][B][1][F][T] standard-normal draws in the
 * reference's call order (prior, then per step: corrector draws, predictor draw), or NULL for the in-kernel Philox
 * stream seeded by `seed`.  A ragged context (sgmse_set_frames) takes PACKED Y / out and noise [1 + N*draws_per_step][sum_b F*T_b].
 * *nfe receives N*(corrector_steps+1). */
int sgmse_pc_sample(sgmse_ctx* ctx, const void* Y, void* out, int B, int F, int T, const sgmse_sampler_cfg* cfg,
                    const void* noise, unsigned long long seed, int* nfe);

/* -- get_sb_sampler(sde, model, y, ...)() (sampling/__init__.py:145-249), Schroedinger-bridge 'ode' and 'sde' samplers:
 *    x_0 = y; for i in 0..N-1:  x <- w_prev[i] x + w_est[i] model(x, y, t[i]) + w_y[i] y + w_z[i] z_i.  Host arrays [N] computed
 *    by the caller from SBVESDE._sigmas_alphas (sdes.py:276-288) with the reference's expressions (t = linspace(T, eps, N+1)[1:]);
 *    'ode': w_z = 0; 'sde' (stochastic = 1): w_y = 0, one draw per step, noise complex64 [N][B][1][F][T] or NULL (Philox).
 *    model = ScoreModel.forward with loss_type 'data_prediction': in_scale / score_alpha / score_beta as in sgmse_sampler_cfg.
 *    Honours sgmse_set_frames: a ragged context takes T = max_b T_b, PACKED Y / out and noise [N][sum_b F*T_b]; every step is
 *    element-wise apart from the network, so an utterance's result is bit-identical to its single-utterance call. */
int sgmse_sb_sample(sgmse_ctx* ctx, const void* Y, void* out, int B, int F, int T, int N, const float* t, const float* w_prev,
                    const float* w_est, const float* w_y, const float* w_z, const float* in_scale, const float* score_alpha,
                    const float* score_beta, int stochastic, const void* noise, unsigned long long seed, int use_graph, int* nfe);

/* -- get_ode_sampler(sde, score_fn, y, denoise=False, rtol, atol, method="RK45")() (sampling/__init__.py:96-143) with the solver in
 *    the library: Dormand-Prince 5(4) with the step control of scipy's RK45 (initial step, error norm over the WHOLE flattened batch,
 *    accept / reject factors, minimum step 10 ulp(t), last step clipped to eps) over the OUVE probability-flow drift
 *    theta (y - x) - g(t)^2 score / 2, from t_end (sde.T) down to eps.  State, stage slopes and error estimate stay on the device;
 *    one scalar per attempted step (the error norm) reaches the host, where the step control runs in double.
 *    Y, out: complex64 [B][1][F][T].  Prior: x0 (complex64 like Y: the start state itself), else y + std1 * z with z = noise
 *    (complex64 like Y, replayed) or the Philox stream of `seed` and the noise-stream ids.  *nfe receives the evaluation count,
 *    counted as scipy's nfev (1 + 1 for the automatic first step + 6 per attempted step).
 *    Errors (SGMSE_ERUNTIME, message in the last-error string): more than max_nfe evaluations needed; step size below 10 ulp(t) (a
 *    non-finite error norm counts as a rejected step and ends there); a ragged context (the error norm couples the utterances).
 *    coef_fn (may be NULL = old-code score wrapper, score = -F): the score wrapper of ncsnpp_v2 models at times only the solver
 *    knows; called on the host once per attempted step with that attempt's n stage times (fp32, as the network sees them), fills
 *    in_scale (gamma), score_alpha, score_beta [n] as in the sampler configuration above. */
typedef void (*sgmse_ode_coef_fn)(void* user, int n, const float* t, float* gamma, float* alpha, float* beta);
typedef struct sgmse_ode_cfg {
  float theta, sigma_min, sigma_max;   /* OUVESDE */
  float std1;                          /* OUVESDE._std(T) for the prior draw (unused with x0) */
  double t_end, eps;                   /* integrate from t_end = sde.T to eps */
  double rtol, atol;
  double first_step, max_step;         /* 0: scipy's select_initial_step / no limit */
  int max_nfe;                         /* cap on evaluations */
  sgmse_ode_coef_fn coef_fn; void* coef_user;
} sgmse_ode_cfg;
int sgmse_ode_sample(sgmse_ctx* ctx, const void* Y, void* out, int B, int F, int T, const sgmse_ode_cfg* cfg, const void* noise,
                     const void* x0, unsigned long long seed, int* nfe);
/* the last sgmse_ode_sample run of this context: accepted and rejected step counts and the first min(cap, accepted) accepted time
 * points (the last one is eps exactly after a completed run).  Any of the pointers may be NULL.  The two samplers keep one set of
 * statistics: after a sgmse_ode_sample_each run this reports that run's utterance 0. */
int sgmse_ode_stats(sgmse_ctx* ctx, int* accepted, int* rejected, double* t_accepted, int cap);
/* -- the same solver with PER-UTTERANCE step control: every utterance of the batch is integrated as if it were alone -- its own
 *    initial step, stage times, error norm (over its own F*T_b elements), accept / reject decisions, step count and end of
 *    integration -- while every network evaluation is still one launch sequence over the whole batch.  Utterance b's result is
 *    bit-identical to what sgmse_ode_sample gives for that utterance alone (B = 1, same prior: x0 / noise / seed and noise-stream id,
 *    same cfg), in any batch and any slot, and so are its evaluation count, step counts and accepted times: what the reference's
 *    one-file-at-a-time enhancement.py loop computes, batched.
 *    Honours sgmse_set_frames: a ragged context takes T = max_b T_b and PACKED Y / out / x0 / noise (utterance after utterance, [F][T_b]
 *    each), as sgmse_pc_sample does; otherwise complex64 [B][1][F][T].
 *    A "round" is one attempted step of every unfinished utterance: six batch evaluations, one table up, B error sums back.  A finished
 *    utterance is frozen (its slot is still evaluated by the network; nothing of it is written) until the last one has finished.
 *    cfg: as for sgmse_ode_sample; max_nfe caps EVERY utterance's own count; coef_fn is called once per round (and once per the one
 *    or two evaluations of the start) with n = stages * B times in STAGE-MAJOR order, t[stage * B + b] (stages = 6 in a round, 1 at the start), and fills its
 *    three arrays in the same order.
 *    *nfe_max receives max_b of utterance b's evaluation count (scipy's nfev) = the number of batch evaluations run.
 *    Errors (SGMSE_ERUNTIME; the message names the utterance and its time; the context stays usable): an utterance needs more than
 *    max_nfe evaluations, or its step size falls below 10 ulp(t) (a non-finite error norm counts as a rejected step). */
int sgmse_ode_sample_each(sgmse_ctx* ctx, const void* Y, void* out, int B, int F, int T, const sgmse_ode_cfg* cfg, const void* noise,
                          const void* x0, unsigned long long seed, int* nfe_max);
/* utterance b of the last sgmse_ode_sample_each run of this context: its evaluation count, accepted and rejected step counts and the
 * first min(cap, accepted) accepted time points; and of the run as a whole: *rounds, and *wasted = the utterance-evaluations spent on
 * slots of utterances that had already finished (6 per finished utterance and round; B * *nfe_max is the total).  Any pointer may be NULL.
 * After a sgmse_ode_sample run the one "utterance", b = 0, is that run's whole batch. */
int sgmse_ode_stats_each(sgmse_ctx* ctx, int b, int* nfe, int* accepted, int* rejected, double* t_accepted, int cap, int* rounds,
                         int* wasted);

/* -- SpecsDataModule.stft / istft / spec_fwd / spec_back (data_module.py:162-188,212-218) ---------------------
 * sig fp32 [B][L] -> spec complex64 [B][n_fft/2+1][L/hop+1] (center=True, reflect pad, window fp32 [n_fft]). */
int sgmse_stft(sgmse_ctx* ctx, const float* sig, const float* window, void* spec, int B, int L, int n_fft, int hop);
int sgmse_istft(sgmse_ctx* ctx, const void* spec, const float* window, float* out, int B, int K, int n_fft, int hop,
                int length);
/* transform_type: 0 'exponent', 1 'log', 2 'none'; n = number of complex elements; in may equal out */
int sgmse_spec_fwd(sgmse_ctx* ctx, const void* in, void* out, long long n, int transform_type, float factor, float exponent);
int sgmse_spec_back(sgmse_ctx* ctx, const void* in, void* out, long long n, int transform_type, float factor, float exponent);

/* -- windows of a long spectrogram (not in the reference, which enhances a recording as one spectrogram) ----------------------
 * A plan is n windows, window j = frames [start[j], start[j] + frames[j]) of a spectrogram of K frames; start and frames are HOST
 * arrays of length n.  Both calls return SGMSE_EINVAL (message in sgmse_last_error) unless the starts are strictly increasing, every
 * window lies inside [0, K), the windows cover [0, K) without a gap and no frame lies under three windows (nor may a window end
 * inside its predecessor: a frame's one or two windows are then always neighbours).
 * `windows` is PACKED: window after window, complex64 [F][frames[j]] each -- what a ragged context (sgmse_set_frames with these
 * frame counts) takes for Y and returns for out.  transform_type / factor / exponent: as for sgmse_spec_fwd.
 * split: windows[j][f][t] = spec_fwd(spec[f][start[j] + t]) for the untransformed spec complex64 [F][K]: a gather, bit-identical to
 *    slicing sgmse_spec_fwd's output. */
int sgmse_spec_split(sgmse_ctx* ctx, const void* spec, void* windows, int F, int K, const int* start, const int* frames, int n,
                     int transform_type, float factor, float exponent);
/* merge: spec[f][k] (complex64 [F][K], back-transformed) from the transformed-domain windows.  A frame under one window:
 *    spec_back of its element, bit-identical to sgmse_spec_back.  A frame under windows j and j + 1, whose overlap
 *    [start[j+1], start[j] + frames[j]) has O_j frames: with a = spec_back(window j's element), b = spec_back(window j+1's) and
 *    w = ((float)(k - start[j+1]) + 0.5f) / (float)O_j, each real component is fmaf(w, b - a, a): a linear cross-fade of the two
 *    back-transformed signals, w running from 0.5 / O_j to 1 - 0.5 / O_j.  One thread per output element, no atomics. */
int sgmse_spec_merge(sgmse_ctx* ctx, const void* windows, void* spec, int F, int K, const int* start, const int* frames, int n,
                     int transform_type, float factor, float exponent);

/* -- one reverse process over a long recording, only the network windowed (not in the reference) ------------------------------
 * A UNIFORM plan is n windows of exactly W frames, window j = frames [start[j], start[j] + W) of a recording of K frames; start is a
 * HOST array of length n.  All three calls return SGMSE_EINVAL (message in sgmse_last_error) unless start[0] = 0, the starts strictly
 * increase, every window lies inside [0, K), the windows cover [0, K) without a gap and no frame lies under four windows (a frame
 * may lie under three).  The window layout is complex64 [n][F][W], frames fastest.
 * gather: windows[j][f][t] = src[f][start[j] + t] for src complex64 [F][K]: a plain copy, no spectrogram transform. */
int sgmse_window_gather(sgmse_ctx* ctx, const void* src, void* windows, int F, int K, int W, const int* start, int n);
/* blend: dst[f][k] (complex64 [F][K]) from the windows over frame k.  Window j has the local frame t = k - start[j] and the weight
 *    w_j = min(1, up, down): up = ((float)t + 0.5f) / (float)L_j for j > 0, L_j = start[j-1] + W - start[j] (its overlap with its
 *    predecessor); down = ((float)(W - t) - 0.5f) / (float)L_{j+1} for j < n - 1.  With a the value of the first window over k and
 *    S the sum of the weights (ascending j), each real component is out = a, then out = fmaf(w_j / S, v_j - a, out) for every later
 *    window over k.  So a frame under one window is that window's element bit for bit, windows that agree give their common value
 *    bit for bit, and two neighbours whose overlap has the length of both their other overlaps get sgmse_spec_merge's cross-fade
 *    (without its spec_back).  IEEE division and fma, one thread per output element, no atomics. */
int sgmse_window_blend(sgmse_ctx* ctx, const void* windows, void* dst, int F, int K, int W, const int* start, int n);
/* The plan for ALL FOLLOWING sgmse_pc_sample / sgmse_sb_sample calls, until the next call (n = 0 withdraws it).  Those calls then take
 * ONE recording, B = 1 and T = K (K need not be a multiple of 2^(levels-1); W must be), and run ONE reverse process on it: state,
 * noise and every sampler update are the recording's, [F][K] -- the in-kernel noise is the recording's own field, index f * K + t,
 * and replayed noise is [ndraws][F][K] --; only the network is windowed.  Each score evaluation gathers the current state's windows,
 * runs the network on them in C = ceil(n / max_batch) chunks of Bc = ceil(n / C) windows (y's windows are gathered once per call)
 * and blends the windows' scores (sgmse_window_blend) into the recording's score.  The up to C - 1 empty slots of the last chunk
 * evaluate its last window again; their scores are not blended.  So the network runs at one shape, the whole step is one captured
 * graph (a second recording of the same K and plan does not capture again), and -- a window's score depending on its own frames
 * only -- the result does not depend on max_batch.  Memory: 4 * 8 F K bytes of state, (2 C Bc + Bc) * 8 F W bytes of window buffers
 * (C Bc < n + C) and the activation arena of Bc windows.
 * The sampler call returns SGMSE_EINVAL with a plan in force if B != 1 or T != K, in a ragged context (sgmse_set_frames) and with a
 * pending noise geometry (sgmse_set_noise_frames); sgmse_set_windows itself for a bad plan, max_batch < 1 and W not a multiple of
 * 2^(levels-1).  sgmse_ode_sample / sgmse_ode_sample_each with a plan in force: SGMSE_EINVAL, "not supported" (the adaptive
 * solver's error norm and step control are not built for it).  Unmeasured: quality -- no trained checkpoint exists here. */
int sgmse_set_windows(sgmse_ctx* ctx, int K, int W, const int* start, int n, int max_batch);

/* -- upfirdn2d(input, kernel, up_x, up_y, down_x, down_y, pad_x0, pad_x1, pad_y0, pad_y1)
 *    (op/upfirdn2d.cpp:12-23, op/upfirdn2d_kernel.cu:209-369).  input fp32 [BC][H][W], kernel fp32 [kh][kw],
 *    out fp32 [BC][(H*up_y+pad_y0+pad_y1-kh)/down_y+1][(W*up_x+pad_x0+pad_x1-kw)/down_x+1]. */
int sgmse_upfirdn2d(sgmse_ctx* ctx, const float* input, const float* kernel, float* out, int BC, int H, int W, int kh,
                    int kw, int up_x, int up_y, int down_x, int down_y, int pad_x0, int pad_x1, int pad_y0, int pad_y1);
/*    The same op over the other element types the reference dispatches (AT_DISPATCH_FLOATING_TYPES_AND_HALF,
 *    op/upfirdn2d_kernel.cu:311): dtype 0 = float (as above), 1 = double, 2 = half (IEEE binary16 bits; fp32 accumulation, one
 *    rounding on the way out).  input, kernel and out share the element type. */
int sgmse_upfirdn2d_dtype(sgmse_ctx* ctx, int dtype, const void* input, const void* kernel, void* out, int BC, int H, int W,
                          int kh, int kw, int up_x, int up_y, int down_x, int down_y, int pad_x0, int pad_x1, int pad_y0,
                          int pad_y1);

/* -- single layers, exported for per-op parity tests (all NCHW fp32) --------------------------------------------
 * conv2d: F.conv2d(cat[x, x2], w, bias, padding=ks/2) (layers.py:100-124), optionally with a fused per-(b,c)
 * affine(+SiLU) on the input, a fused residual and output scale: out = (conv + bias + res) * out_scale.
 * x holds Cin-C2 channels, x2 (may be NULL) the remaining C2.  force_direct = 1 selects the VALU kernel,
 * 2 / 3 the bf16x3 / fp16x2 split MFMA kernels (3x3, Cout % 128 == 0, channel counts % 16 == 0; error otherwise). */
int sgmse_op_conv2d(sgmse_ctx* ctx, const float* x, const float* w_oihw, const float* bias, const float* res, float* out,
                    int B, int Cin, int Cout, int H, int W, int ks, float out_scale, int force_direct,
                    const float* in_scale, const float* in_shift, int in_act, const float* x2, int C2);
/* act(GroupNorm(min(C/4,32), C, eps=1e-6)(cat[x, x2])) (layerspp.py:219,243); act: 0 none, 1 SiLU.  synchronises */
int sgmse_op_groupnorm(sgmse_ctx* ctx, const float* x, const float* gamma, const float* beta, float* out, int B, int C,
                       int H, int W, int act, const float* x2, int C2);
/* upsample_2d / downsample_2d with k=(1,3,3,1), factor 2 (up_or_down_sampling.py:195-257); x fp32 [BC][H][W].
 * Optional fused producer as inside the network: out = FIR(act(x * in_scale[bc] + in_shift[bc])) (in_scale NULL: none;
 * in_act 1: SiLU), and with out_raw != NULL also out_raw = FIR(x) from the same pass (layerspp.py:243-262). */
int sgmse_op_fir(sgmse_ctx* ctx, const float* x, float* out, int BC, int H, int W, int up, const float* in_scale,
                 const float* in_shift, int in_act, float* out_raw);
/* attention core of AttnBlockpp (layerspp.py:82-88): qkv fp32 [B][3C][S] -> out fp32 [B][C][S] */
int sgmse_op_attention(sgmse_ctx* ctx, const float* qkv, float* out, int B, int C, int S);

/* which kernel family the wide 3x3 layers use in this context: 0 fp32 MFMA, 1 bf16x3 split, 2 fp16x2 split
 * (SGMSE_CONV_SPLIT, read at configure time; kernels_conv_split.h) */
int sgmse_conv_split_mode(sgmse_ctx* ctx, int* out);
/* 1 when the levels of >= 32 tiles per image run their full 3x3 layers on the Winograd F(2,3) x fp16x2 kernel (split mode 2 and
 * SGMSE_WINO != 0; kernels_conv_wino.h), else 0.  Like the split mode it replaces nothing in the reference (F.conv2d picks its own
 * algorithm, layers.py:118-124); bench.py names the dominant kernel by it. */
int sgmse_conv_winograd(sgmse_ctx* ctx, int* out);

/* -- measurement: one eager forward with HIP events (on the context's stream) around every kernel launch, summed per
 *    kernel class.  ms, work and launches are host arrays of SGMSE_NCLASS entries:
 *      0 conv3x3 MFMA, 128-channel x 256-pixel tile (the dominant kernel)   1 conv3x3 MFMA, other tiles
 *      2 conv1x1 MFMA   3 direct (VALU) conv   4 groupnorm statistics   5 FIR resampling   6 attention core   7 entry/exit
 *    work = algorithmic FLOPs (classes 0-3, 6) or algorithmic bytes (classes 4, 5, 7).  synchronises */
#define SGMSE_NCLASS 8
int sgmse_profile_forward(sgmse_ctx* ctx, const void* xy, const float* t, void* out, int B, int F, int T, float* ms,
                          double* work, int* launches);
/* micro-benchmark of one MFMA convolution shape on random operands: ms per launch over `iters` back-to-back launches
 * (HIP events on the context's stream).  variant: kernel-variant id (see kernels_conv.h), -1 = default.
 * fused = 1 adds the GroupNorm-affine+SiLU producer and the bias/residual/scale epilogue.  synchronises */
int sgmse_bench_conv(sgmse_ctx* ctx, int ks, int B, int Cin, int Cout, int H, int W, int variant, int iters, int fused,
                     float* ms);
/* measurement only: ONE launch of a coalesced stream of exactly total_bytes (mode 0: read, 1: write; bytes_per_lane 8 or 16) on the
 * context's stream, so that the FETCH_SIZE / WRITE_SIZE counters of a rocprofv3 --pmc pass can be calibrated against a known byte
 * count in the pass that reads them (tools/gpu_visit.sh STEPS=pmcbench; nothing in the reference corresponds).  synchronises */
int sgmse_calib_stream(sgmse_ctx* ctx, int mode, int bytes_per_lane, long long total_bytes, float* ms);
int sgmse_arena_bytes(sgmse_ctx* ctx, long long* out);
/* Noise-stream ids (host array, one per utterance) for the NEXT sgmse_pc_sample / sgmse_sb_sample call of batch size n with
 * in-kernel (Philox) noise: an utterance's draws depend on (seed, stream id, element index inside the utterance, draw index)
 * only, so with ids that name the utterance its noise does not depend on batch composition or slot.  Default (no call, or a
 * different batch size): utterance b uses stream b.  Replaces nothing in the reference (torch.randn_like draws depend on the
 * global generator state, sdes.py:229, correctors.py:74, predictors.py:62). */
int sgmse_set_noise_streams(sgmse_ctx* ctx, const unsigned long long* ids, int n);
/* Noise geometry (host arrays, one entry per utterance) for the NEXT sgmse_pc_sample / sgmse_sb_sample / sgmse_ode_sample /
 * sgmse_ode_sample_each call of batch size n with in-kernel (Philox) noise, consumed like the stream ids: utterance b is the frames
 * first_frame[b] .. first_frame[b] + T_b - 1 of a recording of total_frames[b] frames, and its element (f, t) draws at the counter
 * index f * total_frames[b] + first_frame[b] + t instead of f * T_b + t (stream id and draw index unchanged).  Windows cut from one
 * recording and given ONE stream id therefore draw one noise field: a frame under two windows sees the same draws in both.
 * Default (no call, n = 0, or a different batch size): (0, T_b), today's index; an explicit (0, T_b) gives the same bits.  The
 * geometry is device data like the seed: a captured step serves every geometry of its shape.  The sampler call returns
 * SGMSE_EINVAL (the message names the utterance) if first_frame[b] < 0 or first_frame[b] + T_b > total_frames[b], and if it is
 * given replayed noise (noise != NULL) together with a pending geometry.  Nothing in the reference corresponds. */
int sgmse_set_noise_frames(sgmse_ctx* ctx, const int* first_frame, const int* total_frames, int n);
/* Ragged batches: frames[b] = number of spectrogram frames T_b of utterance b (host array; each a multiple of 2^(levels-1), i.e.
 * of 64 -- what pad_spec produces) for ALL FOLLOWING sgmse_ncsnpp_forward / sgmse_pc_sample / sgmse_sb_sample / sgmse_ode_sample_each calls of batch size n, until the next
 * call (n = 0: uniform batches again).  Those calls then take T = max_b T_b and PACKED tensors: utterance after utterance, each
 * with its own row stride -- xy: [2][F][T_b] per utterance, y / the results: [F][T_b] per utterance (sum_b F*T_b complex elements).
 * An utterance's result is bit-identical to the one its own single-utterance call gives (every kernel addresses an utterance's
 * block exactly as in that call; which kernel family a layer uses depends on the U-Net level only, never on T), so a corpus of
 * mixed lengths runs in full batches.  Supported: the predictor-corrector sampler with correctors 'none', 'ald' and 'langevin'
 * per utterance (corrector = 3), the Schroedinger-bridge sampler and the adaptive solver with per-utterance step control; noise
 * in-kernel (noise == NULL: utterance b draws from its stream id and the element index inside the utterance) or replayed, then
 * PACKED like the results: [ndraws][sum_b F*T_b], draw-major, the utterances of a draw in batch order.  Not supported, because they
 * couple the utterances of a batch: 'langevin' with the batch-mean step size (corrector = 2, correctors.py:50-52) and
 * sgmse_ode_sample (one error norm over the batch).
 * Replaces the one-file-at-a-time loop of enhancement.py:57-103. */
int sgmse_set_frames(sgmse_ctx* ctx, const int* frames, int n);
/* how many times this context captured + instantiated a sampler step as a hipGraph (a run over many batches of one shape and
 * sampler configuration captures once: the Philox seed is device data, not a graph parameter) */
int sgmse_graph_captures(sgmse_ctx* ctx, int* out);
/* how many times a captured step was brought up to date IN PLACE (hipGraphExecUpdate: same launch sequence, other arguments --
 * a new ragged batch composition, a new batch size of the same kernel sequence) instead of being instantiated anew */
int sgmse_graph_updates(sgmse_ctx* ctx, int* out);

#ifdef __cplusplus
}
#endif
#endif /* SGMSE_HIP_H */
