"""ctypes binding of libsgmse_hip.so (C ABI: include/sgmse_hip.h).

The product path has exactly one implementation: the HIP library built for gfx950 by ``__graft_entry__.build()`` /
``make -C sgmse_amd/csrc``.  If it is missing, or no GPU is visible, every entry point fails loudly -- there is no
PyTorch or CPU fallback.  (The test-suite can point ``load_library`` at the CPU workgroup *emulator* build of the
same kernel sources, ``tests/emu/libsgmse_emu.so``, to check kernel logic in a GPU-less container; that library
reports a different ``backend`` string and is never loaded implicitly.)
"""
from __future__ import annotations

import contextlib
import ctypes as C
import os
import threading
from typing import Dict, Optional, Sequence

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_LIB = os.path.join(_HERE, "libsgmse_hip.so")

SGMSE_NCLASS = 8
CLASS_NAMES = ("conv3x3_wide", "conv3x3_other", "conv1x1", "conv_direct", "groupnorm_stats", "fir",
               "attention", "entry_exit")
CLASS_WORK_UNIT = ("flop", "flop", "flop", "flop", "byte", "byte", "flop", "byte")


class NetCfgC(C.Structure):
    _fields_ = [("variant", C.c_int), ("nf", C.c_int), ("n_levels", C.c_int), ("ch_mult", C.c_int * 8),
                ("num_res_blocks", C.c_int), ("n_attn", C.c_int), ("attn_res", C.c_int * 8), ("image_size", C.c_int),
                ("progressive", C.c_int), ("progressive_input", C.c_int), ("scale_by_sigma", C.c_int)]


class SamplerCfgC(C.Structure):
    _fields_ = [("N", C.c_int), ("corrector", C.c_int), ("corrector_steps", C.c_int), ("predictor", C.c_int),
                ("probability_flow", C.c_int), ("denoise", C.c_int), ("theta", C.c_float), ("std1", C.c_float),
                ("t", C.POINTER(C.c_float)), ("dt", C.POINTER(C.c_float)), ("ald_eps", C.POINTER(C.c_float)),
                ("ald_noise", C.POINTER(C.c_float)), ("G", C.POINTER(C.c_float)), ("G2", C.POINTER(C.c_float)),
                ("in_scale", C.POINTER(C.c_float)), ("score_alpha", C.POINTER(C.c_float)), ("score_beta", C.POINTER(C.c_float)),
                ("snr", C.c_float), ("use_graph", C.c_int)]


ODE_COEF_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float))


class OdeCfgC(C.Structure):
    _fields_ = [("theta", C.c_float), ("sigma_min", C.c_float), ("sigma_max", C.c_float), ("std1", C.c_float),
                ("t_end", C.c_double), ("eps", C.c_double), ("rtol", C.c_double), ("atol", C.c_double),
                ("first_step", C.c_double), ("max_step", C.c_double), ("max_nfe", C.c_int), ("coef_fn", ODE_COEF_FN),
                ("coef_user", C.c_void_p)]


_P = C.c_void_p
_I = C.c_int
_F = C.c_float
_LL = C.c_longlong
_SIGS = {
    "sgmse_ctx_create": (_I, [_I, _P, C.POINTER(_P)]),
    "sgmse_ctx_destroy": (None, [_P]),
    "sgmse_set_stream": (_I, [_P, _P]),
    "sgmse_sync": (_I, [_P]),
    "sgmse_last_error": (C.c_char_p, [_P]),
    "sgmse_backend": (C.c_char_p, []),
    "sgmse_configure": (_I, [_P, C.POINTER(NetCfgC)]),
    "sgmse_load_weights": (_I, [_P, C.POINTER(C.c_char_p), C.POINTER(_P), C.POINTER(_LL), _I, _I]),
    "sgmse_param_count": (_I, [_P, C.POINTER(_LL)]),
    "sgmse_ncsnpp_forward": (_I, [_P, _P, _P, _P, _I, _I, _I]),
    "sgmse_pc_sample": (_I, [_P, _P, _P, _I, _I, _I, C.POINTER(SamplerCfgC), _P, C.c_ulonglong, C.POINTER(_I)]),
    "sgmse_sb_sample": (_I, [_P, _P, _P, _I, _I, _I, _I] + [C.POINTER(_F)] * 8 + [_I, _P, C.c_ulonglong, _I, C.POINTER(_I)]),
    "sgmse_ode_sample": (_I, [_P, _P, _P, _I, _I, _I, C.POINTER(OdeCfgC), _P, _P, C.c_ulonglong, C.POINTER(_I)]),
    "sgmse_ode_stats": (_I, [_P, C.POINTER(_I), C.POINTER(_I), C.POINTER(C.c_double), _I]),
    "sgmse_ode_sample_each": (_I, [_P, _P, _P, _I, _I, _I, C.POINTER(OdeCfgC), _P, _P, C.c_ulonglong, C.POINTER(_I)]),
    "sgmse_ode_stats_each": (_I, [_P, _I, C.POINTER(_I), C.POINTER(_I), C.POINTER(_I), C.POINTER(C.c_double), _I, C.POINTER(_I), C.POINTER(_I)]),
    "sgmse_stft": (_I, [_P, _P, _P, _P, _I, _I, _I, _I]),
    "sgmse_istft": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I]),
    "sgmse_spec_fwd": (_I, [_P, _P, _P, _LL, _I, _F, _F]),
    "sgmse_spec_back": (_I, [_P, _P, _P, _LL, _I, _F, _F]),
    "sgmse_spec_split": (_I, [_P, _P, _P, _I, _I, C.POINTER(_I), C.POINTER(_I), _I, _I, _F, _F]),
    "sgmse_spec_merge": (_I, [_P, _P, _P, _I, _I, C.POINTER(_I), C.POINTER(_I), _I, _I, _F, _F]),
    "sgmse_upfirdn2d": (_I, [_P, _P, _P, _P] + [_I] * 13),
    "sgmse_upfirdn2d_dtype": (_I, [_P, _I, _P, _P, _P] + [_I] * 13),
    "sgmse_op_conv2d": (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _F, _I, _P, _P, _I, _P, _I]),
    "sgmse_op_groupnorm": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P, _I]),
    "sgmse_conv_split_mode": (_I, [_P, _P]),
    "sgmse_conv_winograd": (_I, [_P, _P]),
    "sgmse_op_fir": (_I, [_P, _P, _P, _I, _I, _I, _I, _P, _P, _I, _P]),
    "sgmse_op_attention": (_I, [_P, _P, _P, _I, _I, _I]),
    "sgmse_profile_forward": (_I, [_P, _P, _P, _P, _I, _I, _I, C.POINTER(_F), C.POINTER(C.c_double), C.POINTER(_I)]),
    "sgmse_bench_conv": (_I, [_P, _I, _I, _I, _I, _I, _I, _I, _I, _I, C.POINTER(_F)]),
    "sgmse_calib_stream": (_I, [_P, _I, _I, C.c_longlong, C.POINTER(_F)]),
    "sgmse_arena_bytes": (_I, [_P, C.POINTER(_LL)]),
    "sgmse_graph_captures": (_I, [_P, C.POINTER(_I)]),
    "sgmse_graph_updates": (_I, [_P, C.POINTER(_I)]),
    "sgmse_set_noise_streams": (_I, [_P, C.POINTER(C.c_ulonglong), _I]),
    "sgmse_set_noise_frames": (_I, [_P, C.POINTER(_I), C.POINTER(_I), _I]),
    "sgmse_set_frames": (_I, [_P, C.POINTER(_I), _I]),
    "sgmse_set_windows": (_I, [_P, _I, _I, C.POINTER(_I), _I, _I]),
    "sgmse_window_gather": (_I, [_P, _P, _P, _I, _I, _I, C.POINTER(_I), _I]),
    "sgmse_window_blend": (_I, [_P, _P, _P, _I, _I, _I, C.POINTER(_I), _I]),
}
EXPORTED_SYMBOLS = tuple(_SIGS)

_lock = threading.Lock()
_lib: Optional[C.CDLL] = None
_lib_path: Optional[str] = None


class SgmseLibraryError(RuntimeError):
    pass


def load_library(path: Optional[str] = None) -> C.CDLL:
    """Load (once) and return the shared library.  ``path`` defaults to the in-tree HIP build."""
    global _lib, _lib_path
    with _lock:
        want = os.path.abspath(path or DEFAULT_LIB)
        if _lib is not None:
            if path is None or want == _lib_path:
                return _lib
            raise SgmseLibraryError(f"a different sgmse library is already loaded: {_lib_path}")
        if not os.path.exists(want):
            raise SgmseLibraryError(
                f"{want} not found: build the HIP extension first (python -c 'import __graft_entry__ as g; g.build()' "
                f"or make -C sgmse_amd/csrc).  sgmse_amd has no CPU/PyTorch fallback.")
        lib = C.CDLL(want)
        for name, (res, args) in _SIGS.items():
            fn = getattr(lib, name)      # AttributeError if a declared symbol is not exported
            fn.restype = res
            fn.argtypes = args
        _lib, _lib_path = lib, want
        return lib


def backend() -> str:
    return load_library().sgmse_backend().decode()


def is_emulator() -> bool:
    return backend().startswith("cpu-emulator")


def ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def check_tensor(t: torch.Tensor, name: str, dtype: torch.dtype, device: torch.device) -> torch.Tensor:
    if t.dtype != dtype:
        raise ValueError(f"{name}: expected dtype {dtype}, got {t.dtype}")
    if t.device != device:
        raise ValueError(f"{name}: expected device {device}, got {t.device}")
    return t if t.is_contiguous() else t.contiguous()


def _ragged_geometry(items, planes: int, what: str):
    """Frame counts and the common F of a ragged batch: every element [planes,F,T_b] (or [F,T_b] when planes == 1).  The packed
    buffer and the engine's own size arithmetic (sum F*T_b) must agree, so mismatching shapes are refused here."""
    if len(items) == 0:
        raise ValueError(f"ragged batch: empty list of {what}")
    F_ = int(items[0].shape[-2]) if items[0].dim() >= 2 else -1
    frames = []
    for i, v in enumerate(items):
        ok = v.dim() in ((2, 3) if planes == 1 else (3,)) and int(v.shape[-2]) == F_ and v.numel() == planes * F_ * int(v.shape[-1])
        if not ok:
            raise ValueError(f"ragged batch: {what}[{i}] has shape {tuple(v.shape)}; every utterance must be "
                             f"[{planes},{F_},T_b]" + (" or [F,T_b]" if planes == 1 else ""))
        frames.append(int(v.shape[-1]))
    return frames, F_


def _unpack_ragged(out: torch.Tensor, frames, F_: int):
    """The packed result of a ragged call as one [1,F,T_b] tensor per utterance."""
    outs, o = [], 0
    for T_b in frames:
        outs.append(out[o:o + F_ * T_b].reshape(1, F_, T_b))
        o += F_ * T_b
    return outs


def _host_rows(affine, N: int):
    """The score wrapper's (in_scale, score_alpha, score_beta) as fp32 host arrays of length N each; three None without a wrapper."""
    if affine is None:
        return [None, None, None]
    return [torch.as_tensor(v, dtype=torch.float32).detach().to("cpu").expand(N).contiguous() for v in affine]


class Context:
    """One sgmse_ctx: a device, a stream, the weights and the activation arena."""

    def __init__(self, device: "torch.device | str | int | None" = None):
        lib = load_library()
        self.lib = lib
        emu = is_emulator()
        if device is None:
            device = "cpu" if emu else "cuda"
        device = torch.device(device)
        if emu:
            if device.type != "cpu":
                raise SgmseLibraryError("the emulator build only works on CPU tensors")
            self.device = device
            dev_index, stream = 0, None
        else:
            if device.type != "cuda":
                raise SgmseLibraryError("sgmse_amd runs on an AMD GPU only (device must be 'cuda'); there is no CPU path")
            if not torch.cuda.is_available():
                raise SgmseLibraryError("no GPU visible to PyTorch-ROCm; sgmse_amd has no CPU fallback")
            dev_index = device.index if device.index is not None else torch.cuda.current_device()
            self.device = torch.device("cuda", dev_index)
            stream = torch.cuda.current_stream(self.device).cuda_stream
        h = _P()
        rc = lib.sgmse_ctx_create(dev_index, stream, C.byref(h))
        if rc != 0 or not h:
            raise SgmseLibraryError(f"sgmse_ctx_create failed ({rc})")
        self.h = h
        self._keep: Dict[str, object] = {}
        self._frames: list = []          # frame table in force in the library (set_frames); [] = uniform batches
        self._noise_frames_pending = False      # a noise geometry handed to the library that no sampler call has consumed yet
        self._windows = None             # window plan in force in the library (set_windows); None = none

    def __del__(self):
        try:
            if getattr(self, "h", None):
                self.lib.sgmse_ctx_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def check(self, rc: int):
        if rc == 0:
            return
        msg = self.lib.sgmse_last_error(self.h).decode(errors="replace")
        if rc == -1:
            raise ValueError(msg)
        raise RuntimeError(f"sgmse_hip error {rc}: {msg}")

    def _get_int(self, fn, ctype=_I) -> int:
        """``fn(ctx, &out)`` of the C ABI: the integer it writes."""
        out = ctype(0)
        self.check(fn(self.h, C.byref(out)))
        return out.value

    def _pack_ragged(self, items, planes: int, what: str):
        """A ragged batch (list of [planes,F,T_b] tensors, see set_frames) as the library takes it: (utterance after utterance in one
        flat complex64 tensor, the frame counts, F)."""
        frames, F_ = _ragged_geometry(items, planes, what)
        return torch.cat([check_tensor(v, what, torch.complex64, self.device).reshape(-1) for v in items]), frames, F_

    def _pack_ragged_noise(self, noise, frames, F_: int, need: int):
        """Replayed noise of a ragged batch (a list of [ndraws,1,F,T_b] tensors, one per utterance, ndraws >= ``need``) as the library
        takes it: flat [ndraws][sum_b F*T_b], draw-major, the utterances of a draw packed in batch order."""
        if not isinstance(noise, (list, tuple)) or len(noise) != len(frames):
            raise ValueError(f"the replayed noise of a ragged batch is a list of {len(frames)} tensors [ndraws,1,F,T_b], one per utterance")
        nd = int(noise[0].shape[0]) if noise[0].dim() == 4 else -1
        for i, (v, T_b) in enumerate(zip(noise, frames)):
            if v.dim() != 4 or tuple(v.shape) != (nd, 1, F_, T_b) or nd < need:
                raise ValueError(f"ragged batch: noise[{i}] must be [ndraws >= {need},1,{F_},{T_b}] complex64 with one ndraws for all "
                                 f"utterances, got {tuple(v.shape)}")
        return torch.cat([check_tensor(v, "noise", torch.complex64, self.device).reshape(nd, -1) for v in noise], dim=1).contiguous()

    def _take_streams(self, streams, B: int) -> None:
        """``streams`` of a sampler call (None: the default ids): checked against the batch and handed to the library."""
        if streams is not None:
            if len(streams) != B:
                raise ValueError(f"streams must name the {B} utterances of the batch, got {len(streams)}")
            self.set_noise_streams(streams)

    def _take_noise_frames(self, noise_frames, B: int, noise) -> None:
        """``noise_frames`` of a sampler call (None: the default geometry): checked against the batch and handed to the library, which
        checks it against the utterances' frame counts in the call itself.  None withdraws a table an earlier, refused call left."""
        if noise_frames is None:
            if self._noise_frames_pending:
                self.set_noise_frames([])
            return
        if len(noise_frames) != B:
            raise ValueError(f"noise_frames must give (first_frame, total_frames) for the {B} utterances of the batch, got {len(noise_frames)}")
        if noise is not None:
            raise ValueError("noise_frames applies to in-kernel noise (seed / streams), not to replayed noise")
        self.set_noise_frames(noise_frames)

    def _with_capturable_stream(self, run, use_graph) -> None:
        """``run()`` on the current stream, or, when it is to capture a graph there and cannot, on a side stream ordered with it."""
        cur = torch.cuda.current_stream(self.device) if self.device.type == "cuda" else None
        if cur is not None and use_graph and cur.cuda_stream == 0:
            # stream capture is not allowed on the legacy default stream: run the sampler on a side stream
            side = self._keep.get("side_stream")
            if side is None:
                side = self._keep["side_stream"] = torch.cuda.Stream(self.device)
            side.wait_stream(cur)
            with torch.cuda.stream(side):
                run()
            cur.wait_stream(side)
        else:
            run()

    def use_current_stream(self):
        if self.device.type == "cuda":
            self.check(self.lib.sgmse_set_stream(self.h, torch.cuda.current_stream(self.device).cuda_stream))

    def sync(self):
        self.check(self.lib.sgmse_sync(self.h))

    # -- model ------------------------------------------------------------------------------------------------
    def configure(self, *, variant: str, nf: int, ch_mult: Sequence[int], num_res_blocks: int,
                  attn_resolutions: Sequence[int], image_size: int, progressive: str, progressive_input: str,
                  scale_by_sigma: bool = True):
        c = NetCfgC()
        variants = {"ncsnpp": 0, "ncsnpp_48k": 1}
        if variant not in variants:
            raise ValueError(f"unsupported backbone variant {variant!r}")
        prog = {"none": 0, "output_skip": 1}
        pin = {"none": 0, "input_skip": 1}
        if progressive not in prog:
            raise ValueError(f"progressive={progressive!r} is not supported by the HIP backbone (none|output_skip)")
        if progressive_input not in pin:
            raise ValueError(f"progressive_input={progressive_input!r} is not supported by the HIP backbone (none|input_skip)")
        if len(ch_mult) > 8 or len(attn_resolutions) > 8:
            raise ValueError("at most 8 levels / attention resolutions")
        c.variant = variants[variant]; c.nf = nf; c.n_levels = len(ch_mult)
        for i, v in enumerate(ch_mult):
            c.ch_mult[i] = int(v)
        c.num_res_blocks = num_res_blocks; c.n_attn = len(attn_resolutions)
        for i, v in enumerate(attn_resolutions):
            c.attn_res[i] = int(v)
        c.image_size = image_size; c.progressive = prog[progressive]; c.progressive_input = pin[progressive_input]
        c.scale_by_sigma = int(bool(scale_by_sigma))
        self.check(self.lib.sgmse_configure(self.h, C.byref(c)))

    def load_weights(self, state: Dict[str, torch.Tensor]):
        """state: reference state_dict of the backbone (fp32).  Host tensors are copied synchronously; device
        tensors (e.g. after an RCCL broadcast) are copied device-to-device."""
        names = list(state.keys())
        on_dev = all(v.device.type == "cuda" for v in state.values())
        tens = []
        for k in names:
            v = state[k].detach()
            if v.dtype != torch.float32:
                v = v.float()
            if not on_dev and v.device.type != "cpu":
                v = v.cpu()
            tens.append(v.contiguous())
        n = len(names)
        c_names = (C.c_char_p * n)(*[s.encode() for s in names])
        c_ptrs = (_P * n)(*[t.data_ptr() for t in tens])
        c_num = (_LL * n)(*[t.numel() for t in tens])
        self.use_current_stream()
        self.check(self.lib.sgmse_load_weights(self.h, c_names, c_ptrs, c_num, n, int(on_dev)))
        if on_dev:
            self.sync()

    def param_count(self) -> int:
        return self._get_int(self.lib.sgmse_param_count, _LL)

    def forward(self, xy: torch.Tensor, t: torch.Tensor) -> torch.Tensor:
        """NCSNpp.forward: xy complex64 [B,2,F,T], t float32 [B] -> complex64 [B,1,F,T]."""
        if xy.dim() != 4 or xy.shape[1] != 2:
            raise ValueError(f"expected x of shape [B,2,F,T], got {tuple(xy.shape)}")
        xy = check_tensor(xy, "x", torch.complex64, self.device)
        t = check_tensor(t.reshape(-1), "time_cond", torch.float32, self.device)
        B, _, F_, T = xy.shape
        if t.numel() != B:
            raise ValueError("time_cond must have one entry per batch element")
        out = torch.empty((B, 1, F_, T), dtype=torch.complex64, device=self.device)
        self.set_frames([])
        self.use_current_stream()
        self.check(self.lib.sgmse_ncsnpp_forward(self.h, xy.data_ptr(), t.data_ptr(), out.data_ptr(), B, F_, T))
        return out

    def pc_sample(self, Y: torch.Tensor, table: Dict[str, torch.Tensor], *, theta: float, std1: float,
                  corrector: str, corrector_steps: int, predictor: str, probability_flow: bool, denoise: bool,
                  noise: Optional[torch.Tensor], seed: int, use_graph: bool = True, affine=None, snr: float = 0.0, streams=None,
                  corrector_scope: str = "batch", noise_frames=None, windows=None, window_batch=None):
        """``affine``: optional (in_scale, score_alpha, score_beta) fp32 tensors of length N: the score wrapper of
        ScoreModel.forward's new-code branch (ncsnpp_v2); None = old-code branch (score = -F).  ``corrector_scope``: 'batch' --
        the 'langevin' corrector takes its step size from the batch-mean norms (the reference) -- or 'utterance': from each
        utterance's own norms, what that utterance gets in a batch of its own (uniform and ragged batches).  ``noise`` of a ragged
        batch: a list of [ndraws,1,F,T_b] tensors, one per utterance.  ``noise_frames``: see set_noise_frames.  ``windows`` = (W, starts),
        ``window_batch``: the call runs under that window plan (set_windows: one recording [1,1,F,K], K = starts[-1] + W, one reverse
        process, the network on up to ``window_batch`` windows at a time); the plan is withdrawn when the call returns."""
        if corrector_scope not in ("batch", "utterance"):
            raise ValueError(f"corrector_scope must be 'batch' or 'utterance', got {corrector_scope!r}")
        frames = None
        if isinstance(Y, (list, tuple)):       # ragged batch: utterances [F,T_b] (or [1,F,T_b]) of different lengths, see set_frames
            B = len(Y)
            Y, frames, F_ = self._pack_ragged(Y, 1, "y")
            T = max(frames)
        else:
            Y = check_tensor(Y, "y", torch.complex64, self.device)
            if Y.dim() != 4 or Y.shape[1] != 1:
                raise ValueError(f"expected y of shape [B,1,F,T], got {tuple(Y.shape)}")
            B, _, F_, T = Y.shape
        N = int(table["t"].numel())
        cfg = SamplerCfgC()
        cfg.N = N
        cfg.corrector = {"none": 0, "ald": 1, "langevin": 2}[corrector]
        if corrector == "langevin" and corrector_scope == "utterance":
            cfg.corrector = 3
        cfg.snr = float(snr)
        cfg.corrector_steps = int(corrector_steps)
        cfg.predictor = {"none": 0, "reverse_diffusion": 1}[predictor]
        cfg.probability_flow = int(bool(probability_flow)); cfg.denoise = int(bool(denoise))
        cfg.theta = float(theta); cfg.std1 = float(std1); cfg.use_graph = int(bool(use_graph))
        keep = {}
        for k in ("t", "dt", "ald_eps", "ald_noise", "G", "G2"):
            v = table[k].detach().to("cpu", torch.float32).contiguous()
            keep[k] = v
            setattr(cfg, k, C.cast(v.data_ptr(), C.POINTER(C.c_float)))
        if affine is not None:
            for k, v in zip(("in_scale", "score_alpha", "score_beta"), _host_rows(affine, N)):
                keep[k] = v
                setattr(cfg, k, C.cast(v.data_ptr(), C.POINTER(C.c_float)))
        if noise is not None:
            ncorr = cfg.corrector_steps if cfg.corrector else 0
            need = 1 + N * (ncorr + (1 if (cfg.predictor == 1 and not probability_flow) else 0))
        if noise is not None and frames is not None:
            noise = self._pack_ragged_noise(noise, frames, F_, need)
        elif noise is not None:
            noise = check_tensor(noise, "noise", torch.complex64, self.device)
            if noise.shape[0] < need or tuple(noise.shape[1:]) != tuple(Y.shape):
                raise ValueError(f"noise must be [{need},{B},1,{F_},{T}] complex64, got {tuple(noise.shape)}")
        out = torch.empty_like(Y)
        nfe = _I(0)
        self._take_streams(streams, B)
        self._take_noise_frames(noise_frames, B, noise)

        def run():
            self.use_current_stream()
            # the frame table stays in force between calls: consecutive ragged batches of one composition re-use the arena plan
            # and the captured graph; a uniform call switches it off
            self.set_frames(frames if frames is not None else [])
            with self._windows_for_call(windows, window_batch):
                self.check(self.lib.sgmse_pc_sample(self.h, Y.data_ptr(), out.data_ptr(), B, F_, T, C.byref(cfg), ptr(noise),
                                                    C.c_ulonglong(seed & (2 ** 64 - 1)), C.byref(nfe)))
            self._noise_frames_pending = False

        self._with_capturable_stream(run, use_graph)
        self._keep["sampler"] = (noise, keep)   # the captured graph refers to the replayed-noise buffer
        return (out if frames is None else _unpack_ragged(out, frames, F_)), nfe.value

    def sb_sample(self, Y: torch.Tensor, table: Dict[str, torch.Tensor], *, stochastic: bool, noise: Optional[torch.Tensor],
                  seed: int, affine=None, use_graph: bool = True, streams=None, noise_frames=None, windows=None, window_batch=None):
        """Schroedinger-bridge sampler; table: fp32 tensors t, w_prev, w_est, w_y, w_z of length N.  ``Y``: [B,1,F,T], or a ragged list
        of [F,T_b] / [1,F,T_b] spectrograms (``set_frames``; the samples come back as a list of [1,F,T_b], ``noise`` is then a list of
        [ndraws,1,F,T_b] tensors).  ``noise_frames``: see set_noise_frames.  ``windows``, ``window_batch``: see pc_sample."""
        frames = None
        if isinstance(Y, (list, tuple)):
            B = len(Y)
            Y, frames, F_ = self._pack_ragged(Y, 1, "y")
            T = max(frames)
        else:
            Y = check_tensor(Y, "y", torch.complex64, self.device)
            if Y.dim() != 4 or Y.shape[1] != 1:
                raise ValueError(f"expected y of shape [B,1,F,T], got {tuple(Y.shape)}")
            B, _, F_, T = Y.shape
        N = int(table["t"].numel())
        fp = lambda v: C.cast(v.data_ptr(), C.POINTER(_F))
        keep = [table[k].detach().to("cpu", torch.float32).contiguous() for k in ("t", "w_prev", "w_est", "w_y", "w_z")]
        aff = _host_rows(affine, N)
        if noise is not None and frames is not None:
            noise = self._pack_ragged_noise(noise, frames, F_, N)
        elif noise is not None:
            noise = check_tensor(noise, "noise", torch.complex64, self.device)
            if noise.shape[0] < N or tuple(noise.shape[1:]) != tuple(Y.shape):
                raise ValueError(f"noise must be [{N},{B},1,{F_},{T}] complex64, got {tuple(noise.shape)}")
        out = torch.empty_like(Y)
        nfe = _I(0)
        self._take_streams(streams, B)
        self._take_noise_frames(noise_frames, B, noise)

        def run():
            self.use_current_stream()
            self.set_frames(frames if frames is not None else [])
            with self._windows_for_call(windows, window_batch):
                self.check(self.lib.sgmse_sb_sample(self.h, Y.data_ptr(), out.data_ptr(), B, F_, T, N, *[fp(v) for v in keep],
                                                    *[None if v is None else fp(v) for v in aff], int(bool(stochastic)), ptr(noise),
                                                    C.c_ulonglong(seed & (2 ** 64 - 1)), int(bool(use_graph)), C.byref(nfe)))
            self._noise_frames_pending = False

        self._with_capturable_stream(run, use_graph)
        self._keep["sb"] = (noise, keep, aff)
        return (out if frames is None else _unpack_ragged(out, frames, F_)), nfe.value

    def ode_sample(self, Y: torch.Tensor, *, theta: float, sigma_min: float, sigma_max: float, std1: float, t_end: float, eps: float,
                   rtol: float, atol: float, first_step: float = 0.0, max_step: float = 0.0, noise: Optional[torch.Tensor] = None,
                   x0: Optional[torch.Tensor] = None, seed: int = 0, streams=None, affine_fn=None, max_nfe: int = 100000,
                   step_control: str = "batch", noise_frames=None):
        """Adaptive probability-flow sampler inside the library (sgmse_ode_sample): Dormand-Prince 5(4) with scipy's RK45 step
        control, state and stage slopes on the device.  ``x0``: the start state itself; else the prior y + std1 z with ``noise``
        ([B,1,F,T], or the samplers' [ndraws,B,1,F,T] layout whose first entry is the prior draw) or the Philox stream of
        (``seed``, ``streams``; ``noise_frames``: see set_noise_frames).  ``affine_fn``: ``ScoreModel.score_affine`` of an ncsnpp_v2
        model (None: old-code wrapper), called
        with each attempted step's stage times.  Returns (sample, nfe); ``ode_stats`` describes the run.  Raises RuntimeError when
        the solver needs more than ``max_nfe`` evaluations or its step size underflows.

        ``step_control="utterance"`` (sgmse_ode_sample_each): every utterance is integrated as if it were alone -- its result, bit for
        bit, and its counts are those of its own single-utterance call -- while each network evaluation still covers the whole batch.
        ``Y`` (and ``x0``) may then be a ragged list of [F,T_b] / [1,F,T_b] spectrograms (``set_frames``; the samples come back as a
        list of [1,F,T_b]); ``max_nfe`` caps every utterance's own count, ``affine_fn`` sees a round's 6 B stage times stage-major,
        the returned nfe is the largest utterance's, and ``ode_stats_each`` describes the run."""
        if step_control not in ("batch", "utterance"):
            raise ValueError(f"step_control must be 'batch' or 'utterance', got {step_control!r}")
        values = dict(theta=theta, sigma_min=sigma_min, sigma_max=sigma_max, std1=std1, t_end=t_end, eps=eps, rtol=rtol, atol=atol,
                      first_step=first_step, max_step=max_step, max_nfe=max_nfe)
        if step_control == "utterance":
            return self._ode_sample_each(Y, values, noise, x0, seed, streams, affine_fn, noise_frames)
        if isinstance(Y, (list, tuple)):
            raise TypeError("the adaptive ODE sampler integrates one rectangular batch (its error norm couples the utterances): "
                            "pass a tensor, not a ragged list")
        Y, noise, x0 = self._ode_rect_inputs(Y, noise, x0)
        # as in forward / pc_sample / sb_sample: a frame table left in force by an earlier ragged call is no request of this caller's
        # (a ragged batch is a list, refused above); a uniform call switches it off
        return self._ode_call(self.lib.sgmse_ode_sample, Y, Y.shape[0], Y.shape[2], Y.shape[3], [], 1, values, noise, x0, seed, streams, affine_fn,
                              noise_frames)

    def _ode_rect_inputs(self, Y, noise, x0):
        """y [B,1,F,T] and the replayed noise or the start state of a rectangular batch, checked: (y, noise, x0)."""
        Y = check_tensor(Y, "y", torch.complex64, self.device)
        if Y.dim() != 4 or Y.shape[1] != 1:
            raise ValueError(f"expected y of shape [B,1,F,T], got {tuple(Y.shape)}")
        B, _, F_, T = Y.shape
        if noise is not None and x0 is not None:
            raise ValueError("give replayed noise or a start state, not both")
        if noise is not None:
            noise = check_tensor(noise, "noise", torch.complex64, self.device)
            if noise.dim() == Y.dim() + 1:
                noise = noise[0].contiguous()
            if tuple(noise.shape) != tuple(Y.shape):
                raise ValueError(f"noise must be [{B},1,{F_},{T}] complex64 (or [ndraws,{B},1,{F_},{T}]), got {tuple(noise.shape)}")
        if x0 is not None:
            x0 = check_tensor(x0, "z", torch.complex64, self.device)
            if tuple(x0.shape) != tuple(Y.shape):
                raise ValueError(f"the start state must have y's shape {tuple(Y.shape)}, got {tuple(x0.shape)}")
        return Y, noise, x0

    def _ode_call(self, fn, Y, B, F_, T, frames, groups, values, noise, x0, seed, streams, affine_fn, noise_frames=None):
        """One sgmse_ode_sample / sgmse_ode_sample_each call over checked inputs (``frames``: the ragged batch's frame table, [] for
        a rectangular one; ``groups``: controllers of the run, what ode_stats_each will list): (out, nfe).  An exception of the host
        callback is raised again here; a failed run raises RuntimeError."""
        cfg, failure, cb = self._ode_cfg(values, affine_fn)
        self._take_streams(streams, B)
        self._take_noise_frames(noise_frames, B, noise)
        out = torch.empty_like(Y)
        nfe = _I(0)
        self.use_current_stream()
        self.set_frames(frames)
        rc = fn(self.h, Y.data_ptr(), out.data_ptr(), B, F_, T, C.byref(cfg), ptr(noise), ptr(x0), C.c_ulonglong(seed & (2 ** 64 - 1)), C.byref(nfe))
        if failure:
            raise failure[0]
        self.check(rc)
        self._noise_frames_pending = False
        self._ode_each_B = groups
        return out, nfe.value

    @staticmethod
    def _ode_cfg(v, affine_fn):
        """sgmse_ode_cfg of one call: (cfg, failure list of the host callback, the callback object to keep alive)."""
        cfg = OdeCfgC()
        cfg.theta, cfg.sigma_min, cfg.sigma_max, cfg.std1 = float(v["theta"]), float(v["sigma_min"]), float(v["sigma_max"]), float(v["std1"])
        cfg.t_end, cfg.eps, cfg.rtol, cfg.atol = float(v["t_end"]), float(v["eps"]), float(v["rtol"]), float(v["atol"])
        cfg.first_step, cfg.max_step, cfg.max_nfe = float(v["first_step"]), float(v["max_step"]), int(v["max_nfe"])
        failure, cb = [], None
        if affine_fn is not None:
            def _coef(user, n, t, gamma, alpha, beta):      # host callback: exceptions must not cross the C frames
                try:
                    rows = affine_fn(torch.tensor([t[i] for i in range(n)], dtype=torch.float32))
                    for dst, v in zip((gamma, alpha, beta), rows):
                        v = torch.as_tensor(v, dtype=torch.float32).reshape(-1).expand(n)
                        for i in range(n):
                            dst[i] = float(v[i])
                except Exception as e:      # noqa: BLE001
                    failure.append(e)
                    for i in range(n):
                        gamma[i] = alpha[i] = beta[i] = float("nan")
            cb = ODE_COEF_FN(_coef)
            cfg.coef_fn = cb
        return cfg, failure, cb

    def _ode_sample_each(self, Y, values, noise, x0, seed, streams, affine_fn, noise_frames=None):
        """``ode_sample(step_control="utterance")``: sgmse_ode_sample_each over a tensor [B,1,F,T] or a ragged list."""
        if not isinstance(Y, (list, tuple)):
            Y, noise, x0 = self._ode_rect_inputs(Y, noise, x0)
            B, _, F_, T = Y.shape
            return self._ode_call(self.lib.sgmse_ode_sample_each, Y, B, F_, T, [], B, values, noise, x0, seed, streams, affine_fn,
                                  noise_frames)
        if noise is not None:
            raise ValueError("ragged batches take the prior from seed / streams or a start state z, not from replayed noise")
        B = len(Y)
        Y, frames, F_ = self._pack_ragged(Y, 1, "y")
        if x0 is not None:
            if not isinstance(x0, (list, tuple)) or len(x0) != B or _ragged_geometry(x0, 1, "z") != (frames, F_):
                raise ValueError("the start state of a ragged batch is a list with the shapes of y's utterances")
            x0 = self._pack_ragged(x0, 1, "z")[0]
        out, nfe = self._ode_call(self.lib.sgmse_ode_sample_each, Y, B, F_, max(frames), frames, B, values, None, x0, seed, streams, affine_fn,
                                  noise_frames)
        return _unpack_ragged(out, frames, F_), nfe

    def ode_stats_each(self):
        """The last ``ode_sample(step_control="utterance")`` run: dict(utterances=[dict(nfe=..., accepted=..., rejected=...,
        t=[accepted time points]) per utterance], rounds=attempted-step rounds, wasted=utterance-evaluations spent on slots of
        utterances that had already finished)."""
        utts, rounds, wasted = [], _I(0), _I(0)
        for b in range(getattr(self, "_ode_each_B", 0)):
            nfe, acc, rej = _I(0), _I(0), _I(0)
            self.check(self.lib.sgmse_ode_stats_each(self.h, b, C.byref(nfe), C.byref(acc), C.byref(rej), None, 0, None, None))
            ts = (C.c_double * max(acc.value, 1))()
            self.check(self.lib.sgmse_ode_stats_each(self.h, b, None, None, None, ts, acc.value, C.byref(rounds), C.byref(wasted)))
            utts.append(dict(nfe=nfe.value, accepted=acc.value, rejected=rej.value, t=[ts[i] for i in range(acc.value)]))
        return dict(utterances=utts, rounds=rounds.value, wasted=wasted.value)

    def ode_stats(self):
        """The last ``ode_sample`` run: dict(accepted=..., rejected=..., t=[accepted time points]) (of utterance 0 after a
        ``step_control="utterance"`` run)."""
        acc, rej = _I(0), _I(0)
        self.check(self.lib.sgmse_ode_stats(self.h, C.byref(acc), C.byref(rej), None, 0))
        ts = (C.c_double * max(acc.value, 1))()
        self.check(self.lib.sgmse_ode_stats(self.h, C.byref(acc), C.byref(rej), ts, acc.value))
        return dict(accepted=acc.value, rejected=rej.value, t=[ts[i] for i in range(acc.value)])

    def profile_forward(self, xy, t: torch.Tensor):
        """Per-kernel-class HIP-event timing of ONE network evaluation (eager).  xy: complex64 [B,2,F,T], or a list of [2,F,T_b]
        (a ragged batch, as forward_ragged takes it)."""
        t = check_tensor(t, "t", torch.float32, self.device)
        frames = []
        if isinstance(xy, (list, tuple)):
            B = len(xy)
            xy, frames, F_ = self._pack_ragged(xy, 2, "x")
            T = max(frames)
            out = torch.empty(F_ * sum(frames), dtype=torch.complex64, device=self.device)
        else:
            xy = check_tensor(xy, "x", torch.complex64, self.device)
            B, _, F_, T = xy.shape
            out = torch.empty((B, 1, F_, T), dtype=torch.complex64, device=self.device)
        ms = (_F * SGMSE_NCLASS)()
        fl = (C.c_double * SGMSE_NCLASS)()
        nl = (_I * SGMSE_NCLASS)()
        self.use_current_stream()
        self.set_frames(frames)
        self.check(self.lib.sgmse_profile_forward(self.h, xy.data_ptr(), t.data_ptr(), out.data_ptr(), B, F_, T, ms, fl, nl))
        return {n: {"ms": ms[i], "work": fl[i], "unit": CLASS_WORK_UNIT[i], "launches": nl[i]}
                for i, n in enumerate(CLASS_NAMES)}, out

    def bench_conv(self, ks, B, Cin, Cout, H, W, variant=-1, iters=10, fused=False) -> float:
        ms = _F(0)
        self.use_current_stream()
        self.check(self.lib.sgmse_bench_conv(self.h, ks, B, Cin, Cout, H, W, variant, iters, int(fused), C.byref(ms)))
        return ms.value

    def calib_stream(self, mode: int, bytes_per_lane: int, total_bytes: int) -> float:
        """Measurement only: one launch of a known-size coalesced read (mode 0) / write (mode 1) stream; ms of the launch."""
        ms = _F(0)
        self.use_current_stream()
        self.check(self.lib.sgmse_calib_stream(self.h, int(mode), int(bytes_per_lane), int(total_bytes), C.byref(ms)))
        return ms.value

    def conv_winograd(self) -> bool:
        """True when the wide levels' 3x3 layers run on the Winograd F(2,3) x fp16x2 kernel (kernels_conv_wino.h)."""
        return bool(self._get_int(self.lib.sgmse_conv_winograd))

    def conv_split_mode(self) -> int:
        """0: fp32 MFMA, 1: bf16x3 split, 2: fp16x2 split on the wide 3x3 layers (kernels_conv_split.h)."""
        return self._get_int(self.lib.sgmse_conv_split_mode)

    def set_noise_streams(self, ids) -> None:
        """Noise-stream ids (one per utterance) for the next sampler call with in-kernel noise: see sgmse_set_noise_streams."""
        ids = [int(v) & (2 ** 64 - 1) for v in (ids.tolist() if hasattr(ids, "tolist") else ids)]
        arr = (C.c_ulonglong * len(ids))(*ids)
        self.check(self.lib.sgmse_set_noise_streams(self.h, arr, len(ids)))

    def set_noise_frames(self, noise_frames) -> None:
        """Noise geometry, one (first_frame, total_frames) per utterance, for the next sampler call of that batch size with in-kernel
        noise (sgmse_set_noise_frames): utterance b is the frames first_frame .. first_frame + T_b - 1 of a recording of total_frames
        frames and draws the noise that recording's frames draw, so windows of one recording that share a stream id share the draws
        of the frames they share.  [] withdraws a pending table.  The sampler call raises ValueError for a window that does not lie
        inside its recording."""
        pairs = [(int(a), int(b)) for a, b in noise_frames]
        n = len(pairs)
        first, total = (_I * max(n, 1))(*[p[0] for p in pairs]), (_I * max(n, 1))(*[p[1] for p in pairs])
        self.check(self.lib.sgmse_set_noise_frames(self.h, first if n else None, total if n else None, n))
        self._noise_frames_pending = n > 0

    def set_frames(self, frames) -> None:
        """Ragged batches (sgmse_set_frames): frame count of every utterance of the following calls; [] = uniform batches again."""
        frames = [int(v) for v in frames]
        if frames == self._frames:            # unchanged: the library keeps its tables, arena plan and captured graph
            return
        arr = (_I * max(len(frames), 1))(*frames)
        self.check(self.lib.sgmse_set_frames(self.h, arr if frames else None, len(frames)))
        self._frames = frames

    def set_windows(self, windows, window_batch=None) -> None:
        """Window plan of the following pc_sample / sb_sample calls (sgmse_set_windows): ``windows`` = (W, starts), n windows of W
        frames over a recording of K = starts[-1] + W frames, the network on chunks of up to ``window_batch`` (default: all n)
        windows; None withdraws it.  Those calls then take ONE recording [1,1,F,K] and run one reverse process on it, only the
        network windowed.  ValueError for a plan the library refuses.  (pc_sample / sb_sample set and withdraw their own
        ``windows=`` argument; ode_sample refuses to run while a plan is in force.)"""
        if windows is None:
            if self._windows is not None:
                self.check(self.lib.sgmse_set_windows(self.h, 0, 0, None, 0, 0))
                self._windows = None
            return
        W, starts = windows
        W, starts = int(W), [int(v) for v in starts]
        if not starts:
            raise ValueError("a window plan needs at least one start")
        mb = len(starts) if window_batch is None else int(window_batch)
        key = (W, tuple(starts), mb)
        if key == self._windows:
            return
        self._windows = None
        self.check(self.lib.sgmse_set_windows(self.h, starts[-1] + W, W, (_I * len(starts))(*starts), len(starts), mb))
        self._windows = key

    @contextlib.contextmanager
    def _windows_for_call(self, windows, window_batch):
        """The plan of one sampler call: set (None: whatever a set_windows call left is withdrawn) and withdrawn afterwards.  The
        library keeps the last plan's captured step: the same plan in the next call does not capture again."""
        self.set_windows(windows, window_batch)
        try:
            yield
        finally:
            self.set_windows(None)

    def _uniform_window_op(self, fn, src, dst, F_: int, K: int, W: int, starts) -> None:
        starts = [int(v) for v in starts]
        if not starts:
            raise ValueError("a window plan needs at least one start")
        self.use_current_stream()
        self.check(fn(self.h, src.data_ptr(), dst.data_ptr(), F_, K, int(W), (_I * len(starts))(*starts), len(starts)))

    def window_gather(self, src: torch.Tensor, W: int, starts) -> torch.Tensor:
        """sgmse_window_gather: src complex64 [F,K] -> windows complex64 [n,F,W], windows[j] = src[:, starts[j] : starts[j] + W]."""
        src = check_tensor(src, "src", torch.complex64, self.device)
        if src.dim() != 2:
            raise ValueError(f"expected src of shape [F,K], got {tuple(src.shape)}")
        F_, K = src.shape
        out = torch.empty((len(starts), F_, int(W)), dtype=torch.complex64, device=self.device)
        self._uniform_window_op(self.lib.sgmse_window_gather, src, out, F_, K, W, starts)
        return out

    def window_blend(self, windows: torch.Tensor, K: int, starts) -> torch.Tensor:
        """sgmse_window_blend: windows complex64 [n,F,W] -> complex64 [F,K], the windows over a frame blended by their weights."""
        windows = check_tensor(windows, "windows", torch.complex64, self.device)
        if windows.dim() != 3 or windows.shape[0] != len(starts):
            raise ValueError(f"expected windows of shape [{len(starts)},F,W], got {tuple(windows.shape)}")
        _, F_, W = windows.shape
        out = torch.empty((F_, int(K)), dtype=torch.complex64, device=self.device)
        self._uniform_window_op(self.lib.sgmse_window_blend, windows, out, F_, int(K), W, starts)
        return out

    def _window_call(self, fn, src, dst, F_: int, K: int, starts, frames, transform_type: int, factor: float, exponent: float) -> None:
        starts, frames = [int(v) for v in starts], [int(v) for v in frames]
        if len(starts) != len(frames) or not starts:
            raise ValueError(f"a window plan is two lists of one length >= 1, got {len(starts)} starts and {len(frames)} frame counts")
        n = len(starts)
        self.use_current_stream()
        self.check(fn(self.h, src.data_ptr(), dst.data_ptr(), F_, K, (_I * n)(*starts), (_I * n)(*frames), n, int(transform_type),
                      float(factor), float(exponent)))

    def spec_split(self, spec: torch.Tensor, starts, frames, transform_type: int, factor: float, exponent: float) -> torch.Tensor:
        """sgmse_spec_split: spec complex64 [F,K] (untransformed) -> the packed windows (flat complex64, window after window, [F,T_i]
        each, spec_fwd applied).  ValueError for a plan the library refuses."""
        spec = check_tensor(spec, "spec", torch.complex64, self.device)
        if spec.dim() != 2:
            raise ValueError(f"expected spec of shape [F,K], got {tuple(spec.shape)}")
        F_, K = spec.shape
        out = torch.empty(F_ * sum(max(int(v), 0) for v in frames), dtype=torch.complex64, device=self.device)
        self._window_call(self.lib.sgmse_spec_split, spec, out, F_, K, starts, frames, transform_type, factor, exponent)
        return out

    def spec_merge(self, windows: torch.Tensor, F_: int, K: int, starts, frames, transform_type: int, factor: float, exponent: float) -> torch.Tensor:
        """sgmse_spec_merge: the packed windows (transformed domain) -> complex64 [F,K], back-transformed, overlaps cross-faded."""
        windows = check_tensor(windows, "windows", torch.complex64, self.device)
        if windows.numel() != F_ * sum(int(v) for v in frames):
            raise ValueError(f"the packed windows must hold F * sum(frames) = {F_ * sum(int(v) for v in frames)} elements, got {windows.numel()}")
        out = torch.empty((F_, K), dtype=torch.complex64, device=self.device)
        self._window_call(self.lib.sgmse_spec_merge, windows, out, F_, K, starts, frames, transform_type, factor, exponent)
        return out

    def forward_ragged(self, xys, t: torch.Tensor):
        """NCSNpp.forward on utterances of different lengths in ONE batch: xys = list of complex64 [2,F,T_b]; returns the list of
        complex64 [1,F,T_b], each bit-identical to ``forward(xy[None], t[b:b+1])[0]``."""
        packed, frames, F_ = self._pack_ragged(xys, 2, "x")
        t = check_tensor(t.reshape(-1), "time_cond", torch.float32, self.device)
        if t.numel() != len(xys):
            raise ValueError("time_cond must have one entry per utterance")
        out = torch.empty(F_ * sum(frames), dtype=torch.complex64, device=self.device)
        self.set_frames(frames)
        self.use_current_stream()
        self.check(self.lib.sgmse_ncsnpp_forward(self.h, packed.data_ptr(), t.data_ptr(), out.data_ptr(), len(xys), F_, max(frames)))
        return _unpack_ragged(out, frames, F_)

    def graph_captures(self) -> int:
        """Number of hipGraph captures (+ instantiations) of a sampler step this context has done."""
        return self._get_int(self.lib.sgmse_graph_captures)

    def graph_updates(self) -> int:
        """Number of times a captured step was updated in place (hipGraphExecUpdate) instead of being instantiated anew."""
        return self._get_int(self.lib.sgmse_graph_updates)

    def arena_bytes(self) -> int:
        return self._get_int(self.lib.sgmse_arena_bytes, _LL)
