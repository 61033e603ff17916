"""ctypes binding of libwm.so (include/wm.h).  PyTorch is used only to own device memory and
the HIP stream; every call below crosses the C-ABI with plain pointers and sizes.

There is NO fallback: if the HIP library is missing or there is no GPU, construction raises.
"""
from __future__ import annotations

import ctypes as C
import itertools
import os
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from .config import MedusaConfig, GenParams, HEADS_BLOCK

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libwm.so")      # the product library; tests/microbench scripts may point WM_LIB at a debug build
LIB_PATH_F16 = os.path.join(_HERE, "libwm_f16.so")  # the same sources built for the fp16 single-plane decode contract (wm_config.act_fp16)
WM_ABI_VERSION = 9


class WmConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "abi_version", "d_model", "enc_layers", "dec_layers", "n_heads", "ffn_dim", "vocab", "n_mels",
        "n_ctx", "n_tgt", "medusa_heads", "heads_type", "max_batch", "dec_weight_fp8")] + [("medusa_choices", C.c_int32 * 16), ("enc_fp8", C.c_int32),
                                                                                          ("act_fp16", C.c_int32), ("cross_kv_fp8", C.c_int32), ("sibling_rows", C.c_int32)]


class WmWeights(C.Structure):
    _fields_ = [("blob", C.c_void_p), ("blob_bytes", C.c_uint64), ("offsets", C.POINTER(C.c_uint64)),
                ("n_offsets", C.c_int32)]


class WmGenParams(C.Structure):
    _fields_ = [("prompt", C.POINTER(C.c_int32)), ("prompt_len", C.c_int32),
                ("eos_token_id", C.c_int32), ("pad_token_id", C.c_int32),
                ("suppress", C.POINTER(C.c_int32)), ("n_suppress", C.c_int32),
                ("begin_suppress", C.POINTER(C.c_int32)), ("n_begin_suppress", C.c_int32),
                ("max_length", C.c_int32), ("hard_max_length", C.c_int32),
                ("exp_decay_start", C.c_int32), ("exp_decay_factor", C.c_float),
                ("posterior_threshold", C.c_float), ("posterior_alpha", C.c_float),
                ("temperature", C.c_float), ("accept_mode", C.c_int32), ("vanilla", C.c_int32), ("begin_index", C.c_int32),
                ("force_accept", C.c_int32)]


class WmTimestampParams(C.Structure):
    _fields_ = [("timestamp_begin", C.c_int32), ("no_timestamps_token_id", C.c_int32), ("max_initial_timestamp_index", C.c_int32),
                ("begin_index", C.c_int32)]


class WmRepeatParams(C.Structure):
    _fields_ = [("repetition_penalty", C.c_float), ("no_repeat_ngram_size", C.c_int32)]


class WmSampleParams(C.Structure):
    _fields_ = [("temperature", C.c_float), ("seed", C.c_uint64), ("stream_keys", C.POINTER(C.c_uint64)), ("n_keys", C.c_int32)]


class WmSampleFilter(C.Structure):
    _fields_ = [("top_k", C.c_int32), ("top_p", C.c_float), ("min_p", C.c_float)]


class WmBeamParams(C.Structure):
    _fields_ = [("num_beams", C.c_int32), ("length_penalty", C.c_float), ("early_stopping", C.c_int32)]


EARLY_STOPPING_MODES = {False: 0, True: 1, "never": 2}      # wm_beam_params.early_stopping (HF generation_config.early_stopping)


class WmSeqBiasParams(C.Structure):
    _fields_ = [("tokens", C.POINTER(C.c_int32)), ("lens", C.POINTER(C.c_int32)), ("bias", C.POINTER(C.c_float)), ("n", C.c_int32)]


SEQ_BIAS_MAX, SEQ_BIAS_MAX_LEN = 1024, 16                  # WM_SEQ_BIAS_MAX / WM_SEQ_BIAS_MAX_LEN (include/wm.h)


def seq_bias_groups(entries):
    """The grouped table wm_set_sequence_bias builds from ``entries`` [(ids, bias), ..] (include/wm.h): one group per target token — the last id —
    in the order of first appearance, its one-token entry first, then the caller's order.  Returns [(target, [(ids, bias), ..]), ..]: the host-side
    restatement of the lowering, for tests and tools."""
    groups, where = [], {}
    for ids, b in entries:
        ids = tuple(int(t) for t in ids)
        g = where.setdefault(ids[-1], len(groups))
        if g == len(groups):
            groups.append((ids[-1], []))
        if len(ids) == 1:
            groups[g][1].insert(0, (ids, float(b)))
        else:
            groups[g][1].append((ids, float(b)))
    return groups


class WmConstraintParams(C.Structure):
    _fields_ = [("tokens", C.POINTER(C.c_int32)), ("lens", C.POINTER(C.c_int32)), ("n", C.c_int32)]


CONSTRAINT_MAX, CONSTRAINT_MAX_LEN = 16384, 32             # WM_CONSTRAINT_MAX / WM_CONSTRAINT_MAX_LEN (include/wm.h)


class WmAlignParams(C.Structure):
    _fields_ = [("heads", C.POINTER(C.c_int32)), ("n_heads", C.c_int32), ("median_filter_width", C.c_int32), ("time_precision", C.c_float)]


class WmScoreParams(C.Structure):
    _fields_ = [("no_speech_token_id", C.c_int32), ("sot_index", C.c_int32)]


class WmStats(C.Structure):
    _fields_ = [("iterations", C.c_int64), ("iterations_launched", C.c_int64), ("tokens_emitted", C.c_int64),
                ("accept_hist", C.c_int64 * 16),
                ("ms_logmel", C.c_float), ("ms_encode", C.c_float), ("ms_decode", C.c_float),
                ("graph_replays", C.c_int32), ("schedule_steps", C.c_int32), ("sibling_hits", C.c_int32)]


EXPORTS = ["wm_create", "wm_destroy", "wm_last_error", "wm_abi_version", "wm_build_act_fp16", "wm_resample_len", "wm_resample", "wm_logmel", "wm_encode", "wm_set_encoder_output",
           "wm_decode_begin", "wm_decode_run", "wm_get_tokens", "wm_get_stats", "wm_sync",
           "wm_get_encoder_output", "wm_forward_logits", "wm_get_cross_kv", "wm_profile_kernel",
           "wm_decode_begin_ts", "wm_select_rows",
           "wm_token_timestamps", "wm_get_align_probs", "wm_get_align_matrix", "wm_dtw",
           "wm_score_tokens", "wm_score_rows", "wm_set_repeat_rules", "wm_score_tokens_topk", "wm_topk_rows",
           "wm_logmel_long", "wm_gather_windows", "wm_set_sampling", "wm_sample_rows", "wm_set_sampling_filter", "wm_filter_rows",
           "wm_set_beam", "wm_get_beam_result", "wm_beam_rows", "wm_beam_reorder_kv",
           "wm_set_sequence_bias", "wm_seq_bias_rows", "wm_set_constraint", "wm_constraint_rows",
           "wm_set_stream_prompts", "wm_detect_language", "wm_lang_pick_rows", "wm_merge_windows",
           "wm_set_word_table", "wm_word_spans", "wm_vad_windows", "wm_stream_agree"]

LANG_MAX = 256                                             # WM_LANG_MAX (include/wm.h)
MERGE_LEN_MAX, MERGE_WINDOWS_MAX = 512, 4096               # WM_MERGE_LEN_MAX, WM_MERGE_WINDOWS_MAX
WORDS_SPACES, WORDS_UNICODE = 0, 1                         # WM_WORDS_SPACES, WM_WORDS_UNICODE
WORDS_ROWS_MAX, WORDS_IDS_MAX = 65536, 4 << 20             # WM_WORDS_ROWS_MAX, WM_WORDS_IDS_MAX
WORDS_TILE = 1024                                          # WW_TILE (csrc/wm_words.h): tokens of a row staged per round of k_word_spans
VAD_HOP, VAD_TILE = 160, 1024                              # VAD_HOP (csrc/wm_vad.h), VAD_TILE (csrc/wm_vad.hip): samples per frame, frame positions per block
VAD_CLIPS_MAX, VAD_FRAMES_MAX, VAD_TOTAL_FRAMES_MAX, VAD_WINDOWS_MAX = 4096, 1 << 24, 1 << 25, 65536      # WM_VAD_*_MAX
STREAM_TAIL, STREAM_SESSIONS_MAX, STREAM_WORDS_MAX, STREAM_IDS_MAX = 5, 4096, 1 << 20, 4 << 20         # WM_STREAM_*
STREAM_LATE_CS, STREAM_NEAR_CS = 10, 100                   # WM_STREAM_LATE_CS, WM_STREAM_NEAR_CS


class WmStreamList(C.Structure):
    """wm_stream_list (include/wm.h)."""
    _fields_ = [("words", C.POINTER(C.c_int32)), ("tok", C.POINTER(C.c_int32)), ("ids", C.POINTER(C.c_int32))]


class WmStreamParams(C.Structure):
    """wm_stream_params (include/wm.h), in the header's order."""
    _fields_ = [("late_cs", C.c_int32), ("near_cs", C.c_int32), ("max_ngram", C.c_int32)]


class WmVadParams(C.Structure):
    """wm_vad_params (include/wm.h), in the header's order."""
    _fields_ = [("k_on", C.c_float), ("k_off", C.c_float), ("abs_on", C.c_float), ("abs_off", C.c_float),
                ("q_permille", C.c_int32), ("min_silence", C.c_int32), ("min_speech", C.c_int32), ("pad", C.c_int32), ("F", C.c_int32)]

_lib = {}


def default_sibling_rows() -> int:
    """Sibling rows a context is created with when the caller does not choose: WM_SIBLINGS (default 5; the engine caps it at 15 - K).  They only
    act in single-stream decodes over a candidate chain (include/wm.h: wm_config.sibling_rows); emitted ids are the reference's with or without."""
    return int(os.environ.get("WM_SIBLINGS", "5"))


def default_act_fp16() -> bool:
    """The decode numerics contract a model gets when the caller does not choose (``act_fp16=None``): WM_ACT=f16|hilo.  Default f16 (round 6:
    token ids identical to the hi / lo contract and to the fp32-pinned tables in every compared run, one stream +7 %, 32 streams +16 %;
    DESIGN.md §2) — WM_ACT=hilo keeps rounds 1-5's bf16 hi / lo operand pairs."""
    return os.environ.get("WM_ACT", "f16").lower() in ("f16", "fp16")


def load_library(path: Optional[str] = None, act_fp16: bool = False) -> C.CDLL:
    """dlopen libwm.so (bf16 hi / lo decode contract) or libwm_f16.so (fp16 single-plane contract) and declare the prototypes.
    Raises if the library has not been built."""
    global _lib
    if path is None and act_fp16 in _lib:
        return _lib[act_fp16]
    p = path or os.environ.get("WM_LIB_F16" if act_fp16 else "WM_LIB") or (LIB_PATH_F16 if act_fp16 else LIB_PATH)
    if not os.path.exists(p):
        raise RuntimeError(f"{p} not found: build the HIP engine first (python whisper-medusa_amd/build.py). "
                           "There is no CPU fallback.")
    lib = C.CDLL(p)
    vp, i32, f32p, i32p = C.c_void_p, C.c_int32, C.POINTER(C.c_float), C.POINTER(C.c_int32)
    lib.wm_create.argtypes = [C.POINTER(WmConfig), C.POINTER(WmWeights), i32, vp, C.POINTER(vp)]
    lib.wm_destroy.argtypes = [vp]; lib.wm_destroy.restype = None
    lib.wm_last_error.argtypes = [vp]; lib.wm_last_error.restype = C.c_char_p
    lib.wm_abi_version.argtypes = []
    lib.wm_build_act_fp16.argtypes = []
    lib.wm_resample_len.argtypes = [C.c_int64, i32, i32]; lib.wm_resample_len.restype = C.c_int64
    lib.wm_resample.argtypes = [vp, vp, i32, i32, i32, i32, i32, vp]
    lib.wm_logmel.argtypes = [vp, vp, i32, i32, vp]
    lib.wm_logmel_long.argtypes = [vp, vp, i32, i32, vp]
    lib.wm_gather_windows.argtypes = [vp, vp, i32, i32, i32p, i32p, i32p, i32, vp]
    lib.wm_encode.argtypes = [vp, vp, i32]
    lib.wm_set_encoder_output.argtypes = [vp, vp, i32]
    lib.wm_decode_begin.argtypes = [vp, C.POINTER(WmGenParams), i32]
    lib.wm_decode_begin_ts.argtypes = [vp, C.POINTER(WmGenParams), C.POINTER(WmTimestampParams), i32]
    lib.wm_select_rows.argtypes = [vp, C.POINTER(WmGenParams), C.POINTER(WmTimestampParams), i32, f32p, i32p, i32, i32p, i32p,
                                   i32p, f32p, f32p, i32p]
    lib.wm_set_repeat_rules.argtypes = [vp, C.POINTER(WmRepeatParams)]
    lib.wm_set_sampling.argtypes = [vp, C.POINTER(WmSampleParams)]
    lib.wm_sample_rows.argtypes = [vp, C.POINTER(WmGenParams), C.POINTER(WmTimestampParams), C.POINTER(WmSampleParams), i32, f32p, i32p, i32, i32p,
                                   C.POINTER(C.c_uint64), i32p, f32p, i32p]
    lib.wm_set_sampling_filter.argtypes = [vp, C.POINTER(WmSampleFilter)]
    lib.wm_filter_rows.argtypes = [vp, C.POINTER(WmGenParams), C.POINTER(WmTimestampParams), C.POINTER(WmSampleParams), C.POINTER(WmSampleFilter), i32,
                                   f32p, i32p, i32, i32p, C.POINTER(C.c_uint64), f32p, i32p, i32p, i32p, f32p]
    lib.wm_set_beam.argtypes = [vp, C.POINTER(WmBeamParams)]
    lib.wm_get_beam_result.argtypes = [vp, i32, i32, i32p, i32, i32p, f32p]
    lib.wm_beam_rows.argtypes = [vp, C.POINTER(WmGenParams), C.POINTER(WmTimestampParams), C.POINTER(WmBeamParams), i32, i32, f32p, i32p, i32, i32, f32p,
                                 f32p, i32p, i32p, i32p, i32p, i32p, i32p, f32p, i32p, i32p, i32p, f32p]
    lib.wm_beam_reorder_kv.argtypes = [vp, i32, i32p, i32]
    lib.wm_set_sequence_bias.argtypes = [vp, C.POINTER(WmSeqBiasParams)]
    lib.wm_seq_bias_rows.argtypes = [vp, C.POINTER(WmSeqBiasParams), i32, f32p, i32p, i32, i32p, f32p]
    lib.wm_set_constraint.argtypes = [vp, C.POINTER(WmConstraintParams)]
    lib.wm_constraint_rows.argtypes = [vp, C.POINTER(WmConstraintParams), i32, i32, i32, f32p, i32p, i32, i32p, f32p, i32p]
    lib.wm_set_stream_prompts.argtypes = [vp, i32p, i32, i32]
    lib.wm_detect_language.argtypes = [vp, i32, i32p, i32, i32, i32p, f32p]
    lib.wm_lang_pick_rows.argtypes = [vp, i32, f32p, i32p, i32, i32p]
    lib.wm_merge_windows.argtypes = [vp, i32, i32p, i32p, i32, i32p, f32p, i32p, f32p]
    lib.wm_set_word_table.argtypes = [vp, C.POINTER(C.c_uint8), i32p, i32]
    lib.wm_word_spans.argtypes = [vp, i32, i32p, i32p, i32p, f32p, f32p, i32p, i32p, f32p, f32p, f32p]
    lib.wm_vad_windows.argtypes = [vp, i32, vp, C.c_int64, C.POINTER(C.c_int64), C.POINTER(WmVadParams), i32p, i32p, i32, i32p, i32p, i32,
                                   f32p, f32p, f32p, f32p, f32p]
    lib.wm_stream_agree.argtypes = [vp, i32, C.POINTER(WmStreamList), C.POINTER(WmStreamList), C.POINTER(WmStreamList), i32p, i32p,
                                    C.POINTER(WmStreamParams), i32p, i32p, i32p, f32p]
    lib.wm_decode_run.argtypes = [vp, i32, i32p]
    lib.wm_get_tokens.argtypes = [vp, i32, i32p, i32, i32p]
    lib.wm_get_stats.argtypes = [vp, C.POINTER(WmStats)]
    lib.wm_sync.argtypes = [vp]
    lib.wm_get_encoder_output.argtypes = [vp, i32, f32p]
    lib.wm_forward_logits.argtypes = [vp, i32, i32p, i32, i32, i32, f32p]
    lib.wm_get_cross_kv.argtypes = [vp, i32, i32, i32, f32p, f32p]
    lib.wm_profile_kernel.argtypes = [vp, i32, i32, i32, f32p, C.POINTER(C.c_double)]
    lib.wm_token_timestamps.argtypes = [vp, C.POINTER(WmAlignParams), i32, i32p, i32, i32p, i32p, i32p, f32p, f32p]
    lib.wm_get_align_probs.argtypes = [vp, i32, i32, f32p]
    lib.wm_get_align_matrix.argtypes = [vp, i32, f32p]
    lib.wm_dtw.argtypes = [vp, f32p, i32, i32, i32p, i32p, i32p, i32p]
    lib.wm_score_tokens.argtypes = [vp, C.POINTER(WmGenParams), C.POINTER(WmTimestampParams), C.POINTER(WmScoreParams), i32, i32p, i32, i32p, i32p,
                                    f32p, f32p, f32p]
    lib.wm_score_rows.argtypes = [vp, C.POINTER(WmGenParams), C.POINTER(WmTimestampParams), i32, f32p, i32p, i32, i32p, i32p, f32p]
    lib.wm_score_tokens_topk.argtypes = [vp, C.POINTER(WmGenParams), C.POINTER(WmTimestampParams), C.POINTER(WmScoreParams), i32, i32p, i32, i32p, i32p,
                                         i32, f32p, f32p, i32p, f32p, i32p, f32p]
    lib.wm_topk_rows.argtypes = [vp, C.POINTER(WmGenParams), C.POINTER(WmTimestampParams), i32, f32p, i32p, i32, i32p, i32p, i32, i32p, f32p, i32p]
    for name in EXPORTS:
        if name not in ("wm_destroy", "wm_last_error", "wm_resample_len"):      # wm_resample_len returns int64 (set above)
            getattr(lib, name).restype = i32
    if lib.wm_abi_version() != WM_ABI_VERSION and not (os.environ.get("WM_LIB") and os.environ.get("WM_ABI_ANY")):
        raise RuntimeError("libwm.so ABI version mismatch")        # WM_ABI_ANY: A/B runs against an older debug build (tests/microbench)
    if bool(lib.wm_build_act_fp16()) != bool(act_fp16) and path is None:
        raise RuntimeError(f"{p} is built for the other decode contract (wm_build_act_fp16)")
    if path is None:
        _lib[act_fp16] = lib
    return lib


def _i32arr(v: Sequence[int]):
    a = (C.c_int32 * max(len(v), 1))(*[int(x) for x in v])
    return a


def _ip(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def _fp(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _u64p(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_uint64))


def _keys64(keys: Sequence[int]) -> np.ndarray:
    return np.ascontiguousarray([int(k) & (2 ** 64 - 1) for k in keys], dtype=np.uint64)


class Engine:
    """One context = one GPU.  ``blob`` is the packed parameter tensor (uint8, on that GPU)."""

    def __init__(self, cfg: MedusaConfig, blob: torch.Tensor, offsets: np.ndarray, max_batch: int = 1,
                 device: Optional[torch.device] = None, dec_weight_fp8: bool = False, enc_fp8: bool = False, act_fp16: bool = False,
                 cross_kv_fp8: bool = False, sibling_rows: Optional[int] = None):
        if not torch.cuda.is_available():
            raise RuntimeError("no HIP device visible: the Whisper-Medusa engine has no CPU path")
        self.act_fp16 = bool(act_fp16)
        self.lib = load_library(act_fp16=self.act_fp16)
        # wm_config.sibling_rows (include/wm.h): head 1's next-best tokens in the spare rows of a single-stream verify pass; WM_SIBLINGS=0 turns them off
        self.sibling_rows = default_sibling_rows() if sibling_rows is None else int(sibling_rows)
        self.cfg = cfg
        self.device = torch.device(device if device is not None else blob.device)
        if self.device.type != "cuda" or blob.device != self.device:
            raise RuntimeError("parameter blob must live on the engine's GPU")
        self.blob = blob                      # keep alive: the engine borrows it
        self.max_batch = int(max_batch)
        self._offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        c = WmConfig(WM_ABI_VERSION, cfg.d_model, cfg.encoder_layers, cfg.decoder_layers, cfg.n_heads,
                     cfg.decoder_ffn_dim, cfg.vocab_size, cfg.num_mel_bins, cfg.max_source_positions,
                     cfg.max_target_positions, cfg.medusa_num_heads,
                     1 if cfg.medusa_heads_type == HEADS_BLOCK else 0, self.max_batch, 1 if dec_weight_fp8 else 0,
                     (C.c_int32 * 16)(*[int(x) for x in cfg.medusa_choices]), 1 if enc_fp8 else 0, 1 if self.act_fp16 else 0, 1 if cross_kv_fp8 else 0, self.sibling_rows)
        w = WmWeights(C.c_void_p(blob.data_ptr()), blob.numel(),
                      self._offsets.ctypes.data_as(C.POINTER(C.c_uint64)), len(self._offsets))
        # every context owns a private non-blocking HIP stream (NULL -> wm_create makes one): several contexts built under
        # one torch.cuda.stream(s) block must not capture graphs on / launch into the same stream from different host threads
        h = C.c_void_p()
        rc = self.lib.wm_create(C.byref(c), C.byref(w), self.device.index or 0, C.c_void_p(None), C.byref(h))
        if rc != 0:
            raise RuntimeError(f"wm_create failed ({rc}): {self.lib.wm_last_error(None).decode()}")
        self.h = h
        self._B = None
        self._enc_stamp = None
        self._kv_stamp = object()

    def close(self):
        if getattr(self, "h", None):
            self.lib.wm_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int, what: str):
        if rc != 0:
            msg = self.lib.wm_last_error(self.h).decode()
            if rc == -1:
                raise ValueError(f"{what}: {msg}")
            raise RuntimeError(f"{what} failed ({rc}): {msg}")

    def _inputs_ready(self):
        """The context runs on its own HIP stream: tensors PyTorch is still producing on its stream must be complete
        before the engine reads them (pageable H2D copies return before the DMA lands, kernels are asynchronous)."""
        torch.cuda.current_stream(self.device).synchronize()

    # ---- audio front door -----------------------------------------------------------------
    def resample(self, wav: torch.Tensor, sr_in: int, sr_out: int = 16000) -> torch.Tensor:
        """wav [B, channels, n] (or [B, n]) float32 on the GPU -> mono [B, ceil(n * sr_out / sr_in)] at ``sr_out``:
        channel mean + torchaudio-default windowed-sinc resampling (README.md:120-125 of the reference)."""
        wav = wav.to(self.device, torch.float32)
        if wav.dim() == 2:
            wav = wav[:, None, :]
        wav = wav.contiguous()
        B, ch, n = wav.shape
        n_out = int(self.lib.wm_resample_len(n, int(sr_in), int(sr_out)))
        if n_out < 1:
            raise ValueError("resample: empty input or bad sampling rates")
        out = torch.empty(B, n_out, dtype=torch.float32, device=wav.device)
        self._inputs_ready()
        self._check(self.lib.wm_resample(self.h, C.c_void_p(wav.data_ptr()), B, ch, n, int(sr_in), int(sr_out),
                                         C.c_void_p(out.data_ptr())), "wm_resample")
        return out

    # ---- F0 -------------------------------------------------------------------------------
    def logmel(self, wav: torch.Tensor) -> torch.Tensor:
        """wav [B, 160*2*n_ctx] float32 on the GPU -> features [B, n_mels, 2*n_ctx]."""
        wav = wav.to(self.device, torch.float32).contiguous()
        B, n = wav.shape
        feats = torch.empty(B, self.cfg.num_mel_bins, self.cfg.n_mel_frames, dtype=torch.float32, device=wav.device)
        self._inputs_ready()
        self._check(self.lib.wm_logmel(self.h, C.c_void_p(wav.data_ptr()), B, n, C.c_void_p(feats.data_ptr())), "wm_logmel")
        return feats

    def logmel_long(self, wav: torch.Tensor) -> torch.Tensor:
        """wav [B, n] float32 on the GPU, n any positive multiple of 160 -> features [B, n_mels, n / 160] of the whole recordings
        (``WhisperFeatureExtractor(truncation=False)``: the clamp at each recording's own maximum)."""
        wav = wav.to(self.device, torch.float32).contiguous()
        B, n = wav.shape
        feats = torch.empty(B, self.cfg.num_mel_bins, n // 160, dtype=torch.float32, device=wav.device)
        self._inputs_ready()
        self._check(self.lib.wm_logmel_long(self.h, C.c_void_p(wav.data_ptr()), B, n, C.c_void_p(feats.data_ptr())), "wm_logmel_long")
        return feats

    def gather_windows(self, feats: torch.Tensor, clip: Sequence[int], seek: Sequence[int], n_valid: Sequence[int],
                       out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The windows of one long-form round in one launch (HF ``_get_input_segment``): feats [n_clips, n_mels, frames] on the GPU ->
        [len(clip), n_mels, 2*n_ctx] with ``out[w, :, f] = feats[clip[w], :, seek[w] + f]`` for ``f < n_valid[w]`` and 0 behind."""
        feats = feats.to(self.device, torch.float32).contiguous()
        n_clips, n_mels, frames = feats.shape
        Bw = len(clip)
        if n_mels != self.cfg.num_mel_bins or len(seek) != Bw or len(n_valid) != Bw:
            raise ValueError("gather_windows: feats must be [n_clips, n_mels, frames] with one clip, seek and n_valid per window")
        if out is None:
            out = torch.empty(Bw, n_mels, self.cfg.n_mel_frames, dtype=torch.float32, device=self.device)
        c, s, v = (np.ascontiguousarray(a, dtype=np.int32) for a in (clip, seek, n_valid))
        i32p = C.POINTER(C.c_int32)
        self._inputs_ready()
        self._check(self.lib.wm_gather_windows(self.h, C.c_void_p(feats.data_ptr()), n_clips, frames, c.ctypes.data_as(i32p), s.ctypes.data_as(i32p),
                                               v.ctypes.data_as(i32p), Bw, C.c_void_p(out.data_ptr())), "wm_gather_windows")
        return out

    # ---- F1/F2 ------------------------------------------------------------------------------
    def encode(self, feats: torch.Tensor) -> None:
        feats = feats.to(self.device, torch.float32).contiguous()
        B = feats.shape[0]
        if tuple(feats.shape[1:]) != (self.cfg.num_mel_bins, self.cfg.n_mel_frames):
            raise ValueError(f"Whisper expects the mel input features to be of length {self.cfg.n_mel_frames}, "
                             f"but found {feats.shape[-1]}")
        self._inputs_ready()
        self._check(self.lib.wm_encode(self.h, C.c_void_p(feats.data_ptr()), B), "wm_encode")
        self._B = B
        self._enc_stamp = object()            # identity of the resident encoder pass (api.forward: encoder_outputs / past_key_values handles)

    def set_encoder_output(self, hidden: torch.Tensor) -> None:
        """hidden [B, n_ctx, d_model] (the encoder's last hidden state, e.g. ``encoder_outputs[0]`` of a previous forward) replaces
        the encoder pass: stored bf16, cross K/V projected from it (reference forward(encoder_outputs=...), model.py:1232)."""
        hidden = hidden.to(self.device, torch.float32).contiguous()
        if hidden.dim() != 3 or tuple(hidden.shape[1:]) != (self.cfg.max_source_positions, self.cfg.d_model):
            raise ValueError(f"encoder_outputs[0] must be [B, {self.cfg.max_source_positions}, {self.cfg.d_model}], got {tuple(hidden.shape)}")
        self._inputs_ready()
        self._check(self.lib.wm_set_encoder_output(self.h, C.c_void_p(hidden.data_ptr()), hidden.shape[0]), "wm_set_encoder_output")
        self._B = hidden.shape[0]
        self._enc_stamp = object()

    # ---- F3..F14 ------------------------------------------------------------------------------
    @staticmethod
    def _gen_struct(gp: GenParams):
        prompt, sup, bsup = _i32arr(gp.prompt), _i32arr(gp.suppress_tokens), _i32arr(gp.begin_suppress_tokens)
        g = WmGenParams(prompt, len(gp.prompt), gp.eos_token_id, gp.pad_token_id, sup, len(gp.suppress_tokens),
                        bsup, len(gp.begin_suppress_tokens), gp.max_length, gp.hard_max_length,
                        int(gp.exp_decay[0]) if gp.exp_decay is not None else -1,      # the eval CLI parses the start as float
                        float(gp.exp_decay[1]) if gp.exp_decay is not None else 1.0,
                        gp.posterior_threshold, gp.posterior_alpha, gp.temperature if gp.temperature else 0.0,
                        gp.accept_mode, 1 if gp.vanilla else 0, int(gp.begin_index), int(getattr(gp, "force_accept", -1)))
        return g, (prompt, sup, bsup)          # (the arrays the struct points into: keep them alive with it)

    @staticmethod
    def _ts_struct(gp: GenParams) -> WmTimestampParams:
        mit = gp.max_initial_timestamp_index
        return WmTimestampParams(int(gp.no_timestamps_token_id) + 1, int(gp.no_timestamps_token_id), -1 if mit is None else int(mit),
                                 int(gp.begin_index))

    def _set_repeat_rules(self, gp: GenParams) -> None:
        """The context's repetition rules follow ``gp`` before every call that reads them (wm_set_repeat_rules is sticky): neutral fields
        clear them, so a pooled context never inherits the rules of an earlier call."""
        pen, g = float(getattr(gp, "repetition_penalty", 1.0)), int(getattr(gp, "no_repeat_ngram_size", 0))
        if pen == 1.0 and g == 0:
            self._check(self.lib.wm_set_repeat_rules(self.h, None), "wm_set_repeat_rules")
        else:
            rp = WmRepeatParams(pen, g)
            self._check(self.lib.wm_set_repeat_rules(self.h, C.byref(rp)), "wm_set_repeat_rules")

    def set_sampling(self, temperature: Optional[float], seed: int = 0, stream_keys: Optional[Sequence[int]] = None, n_keys: Optional[int] = None) -> None:
        """wm_set_sampling: seeded sampling for the following plain decodes (``gp.vanilla``), sticky until cleared (``temperature=None``).
        ``stream_keys``: one 64-bit key per stream (None: 0 .. n_keys - 1); their number must equal the decode's B."""
        if temperature is None:
            self._check(self.lib.wm_set_sampling(self.h, None), "wm_set_sampling")
            return
        if stream_keys is None:
            sp = WmSampleParams(float(temperature), int(seed) & (2 ** 64 - 1), None, int(n_keys or 0))
        else:
            keys = _keys64(stream_keys)
            sp = WmSampleParams(float(temperature), int(seed) & (2 ** 64 - 1), _u64p(keys), len(keys))
        self._check(self.lib.wm_set_sampling(self.h, C.byref(sp)), "wm_set_sampling")

    def _set_sampling(self, gp: GenParams, B: int) -> None:
        """The context's sampling request follows ``gp`` before every decode (wm_set_sampling is sticky), like the repetition rules."""
        T = float(getattr(gp, "sampling_temperature", 0.0) or 0.0)
        if T == 0.0:
            self.set_sampling(None)
        else:
            self.set_sampling(T, int(gp.sampling_seed), gp.sampling_keys, B)
        # (the filter follows gp too; set while T == 0 it stays set, and the decode refuses it by name: it is never ignored)
        flt = (int(getattr(gp, "sampling_top_k", 0) or 0), float(getattr(gp, "sampling_top_p", 1.0)), float(getattr(gp, "sampling_min_p", 0.0) or 0.0))
        if flt != getattr(self, "_filter_set", (0, 1.0, 0.0)):       # (a context starts with the filter off: the default path makes no call)
            self.set_sampling_filter(*flt)

    def set_sampling_filter(self, top_k: Optional[int] = 0, top_p: float = 1.0, min_p: float = 0.0) -> None:
        """wm_set_sampling_filter: top-k / top-p / min-p for the following sampled decodes, sticky until cleared (``top_k=None``,
        or all three off: 0, 1.0, 0.0).  Read only while sampling is on; a decode that does not sample refuses a set filter."""
        if top_k is None or (int(top_k) == 0 and float(top_p) == 1.0 and float(min_p) == 0.0):
            self._check(self.lib.wm_set_sampling_filter(self.h, None), "wm_set_sampling_filter")
            self._filter_set = (0, 1.0, 0.0)
            return
        f = WmSampleFilter(int(top_k), float(top_p), float(min_p))
        self._check(self.lib.wm_set_sampling_filter(self.h, C.byref(f)), "wm_set_sampling_filter")
        self._filter_set = (int(top_k), float(top_p), float(min_p))

    @staticmethod
    def _beam_struct(num_beams: int, length_penalty: float = 1.0, early_stopping=False) -> WmBeamParams:
        if isinstance(early_stopping, str):
            es = early_stopping
        else:
            es = bool(early_stopping)
        if es not in EARLY_STOPPING_MODES:
            raise ValueError(f"`early_stopping` must be a boolean or 'never', but is {early_stopping!r}")
        return WmBeamParams(int(num_beams), float(length_penalty), EARLY_STOPPING_MODES[es])

    def set_beam(self, num_beams: Optional[int], length_penalty: float = 1.0, early_stopping=False) -> None:
        """wm_set_beam: beam search for the following plain decodes (``gp.vanilla``), sticky until cleared (``num_beams`` None or 1).  The
        decode's B is then the number of clips; it runs B * num_beams streams (<= max_batch)."""
        if num_beams is None or int(num_beams) == 1:
            self._check(self.lib.wm_set_beam(self.h, None), "wm_set_beam")
            return
        bp = self._beam_struct(num_beams, length_penalty, early_stopping)
        self._check(self.lib.wm_set_beam(self.h, C.byref(bp)), "wm_set_beam")

    def _set_beam(self, gp: GenParams) -> None:
        """The context's beam request follows ``gp`` before every decode (wm_set_beam is sticky), like the sampling request."""
        self.set_beam(int(getattr(gp, "num_beams", 1) or 1), float(getattr(gp, "length_penalty", 1.0)), getattr(gp, "early_stopping", False))

    @staticmethod
    def _seq_bias_struct(entries):
        """[(ids, bias), ..] -> (wm_seq_bias_params, the arrays it points into).  The checks are the library's (wm_set_sequence_bias)."""
        ent = [(tuple(int(t) for t in ids), float(b)) for ids, b in entries]
        tok = np.ascontiguousarray([t for ids, _ in ent for t in ids] or [0], dtype=np.int32)
        lens = np.ascontiguousarray([len(ids) for ids, _ in ent] or [0], dtype=np.int32)
        bias = np.ascontiguousarray([b for _, b in ent] or [0.0], dtype=np.float32)
        i32p = C.POINTER(C.c_int32)
        sb = WmSeqBiasParams(tok.ctypes.data_as(i32p), lens.ctypes.data_as(i32p), bias.ctypes.data_as(C.POINTER(C.c_float)), len(ent))
        return sb, (tok, lens, bias)

    def set_sequence_bias(self, entries) -> None:
        """wm_set_sequence_bias: HF's SequenceBiasLogitsProcessor / NoBadWordsLogitsProcessor for the following plain decodes (``gp.vanilla``),
        sticky until cleared (``entries`` None).  ``entries``: [(ids, bias), ..] in the caller's order, a bias finite or -inf."""
        if entries is None:
            self._check(self.lib.wm_set_sequence_bias(self.h, None), "wm_set_sequence_bias")
            return
        sb, _keep = self._seq_bias_struct(entries)
        self._check(self.lib.wm_set_sequence_bias(self.h, C.byref(sb)), "wm_set_sequence_bias")

    def _set_sequence_bias(self, gp: GenParams) -> None:
        """The context's sequence bias follows ``gp`` before every decode (wm_set_sequence_bias is sticky), like the repetition rules."""
        self.set_sequence_bias(getattr(gp, "sequence_bias", None) or None)

    @staticmethod
    def _constraint_struct(seqs):
        """[ids, ..] -> (wm_constraint_params, the arrays it points into).  The checks are the library's (wm_set_constraint)."""
        seqs = [tuple(int(t) for t in ids) for ids in seqs]
        tok = np.ascontiguousarray([t for ids in seqs for t in ids] or [0], dtype=np.int32)
        lens = np.ascontiguousarray([len(ids) for ids in seqs] or [0], dtype=np.int32)
        i32p = C.POINTER(C.c_int32)
        return WmConstraintParams(tok.ctypes.data_as(i32p), lens.ctypes.data_as(i32p), len(seqs)), (tok, lens)

    def set_constraint(self, seqs) -> None:
        """wm_set_constraint: the closed set of token sequences the following plain decodes (``gp.vanilla``) are held to — HF's
        PrefixConstrainedLogitsProcessor over a fixed list —, sticky until cleared (``seqs`` None).  Every sequence is closed by eos implicitly."""
        if seqs is None:
            self._check(self.lib.wm_set_constraint(self.h, None), "wm_set_constraint")
            self._constraint_set = False
            return
        c, _keep = self._constraint_struct(seqs)
        self._constraint_set = True             # (a refused table leaves the earlier one in place: the next decode without one clears it)
        self._check(self.lib.wm_set_constraint(self.h, C.byref(c)), "wm_set_constraint")

    def _set_constraint(self, gp: GenParams) -> None:
        """The context's constraint follows ``gp`` before every decode (wm_set_constraint is sticky), like the sequence bias.  A context that never
        had a table makes no call (like the sampling filter)."""
        seqs = getattr(gp, "allowed_sequences", None) or None
        if seqs is not None or getattr(self, "_constraint_set", False):
            self.set_constraint(seqs)

    def constraint_rows(self, seqs, eos: int, prompt_len: int, logits: np.ndarray, prefixes: Sequence[Sequence[int]]):
        """Constraint parity tap (wm_constraint_rows): rows ``logits [R, V]``, row r under ``prefixes[r]`` (its first ``prompt_len`` ids the decoder
        prompt), through k_constraint alone.  Returns (the masked rows, numpy float32 [R, V]; the number of allowed ids of every row, int32 [R])."""
        x, R, pre, lens, Tmax = self._tap_rows("constraint_rows", logits, prefixes)
        out, n_allowed = np.zeros_like(x), np.zeros(R, dtype=np.int32)
        c, _keep = self._constraint_struct(seqs)
        self._kv_stamp = object()
        self._check(self.lib.wm_constraint_rows(self.h, C.byref(c), int(eos), int(prompt_len), R, _fp(x), _ip(pre), Tmax, _ip(lens), _fp(out), _ip(n_allowed)),
                    "wm_constraint_rows")
        return out, n_allowed

    def set_stream_prompts(self, prompts: Optional[Sequence[Sequence[int]]]) -> None:
        """wm_set_stream_prompts: one decoder prompt per clip for the following decodes, all of one length, sticky until cleared
        (``prompts`` None).  The shape is checked against the decode by wm_decode_begin*."""
        if prompts is None:
            self._check(self.lib.wm_set_stream_prompts(self.h, None, 0, 0), "wm_set_stream_prompts")
            return
        rows = [[int(t) for t in r] for r in prompts]
        if not rows or len({len(r) for r in rows}) != 1:
            raise ValueError("set_stream_prompts: one prompt per clip, all of one length (ragged prompts are not supported)")
        a = np.ascontiguousarray(rows, dtype=np.int32)
        self._check(self.lib.wm_set_stream_prompts(self.h, a.ctypes.data_as(C.POINTER(C.c_int32)), a.shape[0], a.shape[1]), "wm_set_stream_prompts")

    def _set_stream_prompts(self, gp: GenParams) -> None:
        """The context's per-stream prompts follow ``gp`` before every decode (wm_set_stream_prompts is sticky): a missing field clears them, so a
        pooled context never inherits the table of an earlier call."""
        self.set_stream_prompts(getattr(gp, "prompts", None) or None)

    def detect_language(self, lang_ids: Sequence[int], start_token: int) -> List[int]:
        """wm_detect_language: the language token of every clip of the resident encoder pass — one base pass over ``start_token``, then the pick
        among ``lang_ids`` on the device (the largest value, among equal values the smallest id).  B ints come back, never a logits row.
        Overwrites the decode state; ``last_detect_ms`` holds the hipEvent time."""
        if self._B is None:
            raise RuntimeError("detect_language: encode first")
        ids = np.ascontiguousarray([int(t) for t in lang_ids], dtype=np.int32)
        out = np.zeros(self._B, dtype=np.int32)
        ms = C.c_float(0)
        i32p = C.POINTER(C.c_int32)
        self._kv_stamp = object()
        self._check(self.lib.wm_detect_language(self.h, self._B, ids.ctypes.data_as(i32p), len(ids), int(start_token), out.ctypes.data_as(i32p),
                                                C.byref(ms)), "wm_detect_language")
        self.last_detect_ms = ms.value
        return [int(t) for t in out]

    def lang_pick_rows(self, logits: np.ndarray, lang_ids: Sequence[int]) -> np.ndarray:
        """Language-pick parity tap (wm_lang_pick_rows): rows ``logits [R, V]`` through k_lang_pick alone.  Returns numpy int32 [R]: the id of
        ``lang_ids`` with the largest value in the row, among equal values the smallest id."""
        x, R, _, _, _ = self._tap_rows("lang_pick_rows", logits)
        ids = np.ascontiguousarray([int(t) for t in lang_ids], dtype=np.int32)
        out = np.zeros(R, dtype=np.int32)
        self._kv_stamp = object()
        self._check(self.lib.wm_lang_pick_rows(self.h, R, _fp(x), _ip(ids), len(ids), _ip(out)), "wm_lang_pick_rows")
        return out

    def merge_windows(self, windows_per_clip, times_per_clip=None) -> List[List[Tuple[int, int]]]:
        """wm_merge_windows: the slices that stitch the overlapping windows of every clip — transformers' ``_find_longest_common_sequence`` as one
        kernel launch for all boundaries of all clips.  ``windows_per_clip[c][j]``: the text ids of clip c's window j (no prompt, EOS or padding; an
        empty window is skipped by the chain); ``times_per_clip``: one absolute time per id in the same shape (float32), a match then also needs
        the times in order.  Returns per clip ``[(a, b), ..]``: window j contributes ``ids[a:b]``.  Touches nothing of the decode state;
        ``last_merge_ms`` holds the hipEvent time of upload + kernel + download."""
        wins = [list(w) for clip in windows_per_clip for w in clip]
        first = np.zeros(len(windows_per_clip) + 1, dtype=np.int32)
        first[1:] = np.cumsum([len(clip) for clip in windows_per_clip])
        W = len(wins)
        Tmax = max([len(w) for w in wins] + [1])
        tok = np.zeros((max(W, 1), Tmax), dtype=np.int32)
        lens = np.zeros(max(W, 1), dtype=np.int32)
        for w, ids in enumerate(wins):
            tok[w, : len(ids)] = np.asarray(ids, dtype=np.int64)
            lens[w] = len(ids)
        tm = None
        if times_per_clip is not None:
            tms = [w for clip in times_per_clip for w in clip]
            if [len(clip) for clip in times_per_clip] != [len(clip) for clip in windows_per_clip] or [len(w) for w in tms] != [len(w) for w in wins]:
                raise ValueError("merge_windows: times_per_clip must have the shape of windows_per_clip")
            tm = np.zeros((max(W, 1), Tmax), dtype=np.float32)
            for w, t in enumerate(tms):
                tm[w, : len(t)] = np.asarray(t, dtype=np.float32)
        keep = np.zeros((max(W, 1), 2), dtype=np.int32)
        ms = C.c_float(0)
        self._check(self.lib.wm_merge_windows(self.h, len(windows_per_clip), _ip(first), _ip(tok), Tmax, _ip(lens), None if tm is None else _fp(tm),
                                              _ip(keep), C.byref(ms)), "wm_merge_windows")
        self.last_merge_ms = ms.value
        return [[(int(keep[w, 0]), int(keep[w, 1])) for w in range(first[c], first[c + 1])] for c in range(len(windows_per_clip))]

    def set_word_table(self, blob: np.ndarray, offsets: np.ndarray) -> None:
        """wm_set_word_table: the bytes of every text id (``blob`` uint8, ``offsets`` int32 [n_tokens + 1]; whisper_medusa/words.py WordTable builds
        them).  Uploaded once; a later call replaces the table."""
        blob = np.ascontiguousarray(blob, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.int32)
        self._check(self.lib.wm_set_word_table(self.h, blob.ctypes.data_as(C.POINTER(C.c_uint8)), _ip(offsets), len(offsets) - 1), "wm_set_word_table")

    def word_spans(self, rows, modes, times=None, logprobs=None):
        """wm_word_spans: the words of every row of text ids — transformers' ``_combine_tokens_into_words`` as one kernel launch for all rows of the
        call.  ``rows[r]``: text ids (below the table's n_tokens; may be empty, any length); ``modes[r]``: WORDS_SPACES or WORDS_UNICODE;
        ``times[r]``: float32 [len, 2] (start, end) per id; ``logprobs[r]``: float32 [len].  Returns per row ``(word_first, word_times, word_logprobs)``:
        int32 [n_words + 1] ascending starts ending in the row's length, float32 [n_words, 2] or None, float32 [n_words] or None.  Touches nothing
        of the decode state; ``last_words_ms`` holds the hipEvent time of upload + kernel + download."""
        R = len(rows)
        if len(modes) != R or (times is not None and len(times) != R) or (logprobs is not None and len(logprobs) != R):
            raise ValueError("word_spans: modes, times and logprobs must have one entry per row")
        if R == 0:
            self.last_words_ms = 0.0
            return []
        first = np.zeros(R + 1, dtype=np.int32)
        first[1:] = np.cumsum([len(r) for r in rows])
        N = int(first[R])
        ids = np.zeros(max(N, 1), dtype=np.int32)
        if N:
            ids[:N] = np.concatenate([np.asarray(r, dtype=np.int64).reshape(-1) for r in rows])
        md = np.ascontiguousarray([int(m) for m in modes], dtype=np.int32)
        tm = lp = wt = wl = None
        if times is not None:
            tm = np.zeros((max(N, 1), 2), dtype=np.float32)
            for r, t in enumerate(times):
                t = np.asarray(t, dtype=np.float32).reshape(-1, 2)
                if len(t) != len(rows[r]):
                    raise ValueError("word_spans: times must have the shape of rows")
                tm[first[r]: first[r + 1]] = t
            wt = np.zeros_like(tm)
        if logprobs is not None:
            lp = np.zeros(max(N, 1), dtype=np.float32)
            for r, t in enumerate(logprobs):
                t = np.asarray(t, dtype=np.float32).reshape(-1)
                if len(t) != len(rows[r]):
                    raise ValueError("word_spans: logprobs must have the shape of rows")
                lp[first[r]: first[r + 1]] = t
            wl = np.zeros_like(lp)
        nw = np.zeros(R, dtype=np.int32)
        wf = np.zeros(N + R, dtype=np.int32)
        ms = C.c_float(0)
        self._check(self.lib.wm_word_spans(self.h, R, _ip(first), _ip(ids), _ip(md), None if tm is None else _fp(tm), None if lp is None else _fp(lp),
                                           _ip(nw), _ip(wf), None if wt is None else _fp(wt), None if wl is None else _fp(wl), C.byref(ms)), "wm_word_spans")
        self.last_words_ms = ms.value
        out = []
        for r in range(R):
            b, n = int(first[r]), int(nw[r])
            out.append((wf[b + r: b + r + n + 1].copy(), None if wt is None else wt[b: b + n].copy(), None if wl is None else wl[b: b + n].copy()))
        return out

    @staticmethod
    def _stream_list(name: str, sessions):
        """One word list of a stream_agree call as (words, tok, ids) int32 arrays: ``sessions[s]`` is a list of words, a word a list of ids."""
        words = np.zeros(len(sessions) + 1, dtype=np.int32)
        words[1:] = np.cumsum([len(w) for w in sessions])
        flat = [w for ws in sessions for w in ws]           # one pass over the words, one over the ids: no array per word
        lens = list(map(len, flat))
        if 0 in lens:
            raise ValueError(f"stream_agree: {name}: every word needs at least one id")
        tok = np.zeros(len(lens) + 1, dtype=np.int32)
        tok[1:] = np.cumsum(lens)
        n = int(tok[-1])
        ids = np.zeros(max(n, 1), dtype=np.int32)
        if n:
            ids[:n] = np.fromiter(itertools.chain.from_iterable(flat), dtype=np.int64, count=n)
        return words, tok, ids

    def stream_agree(self, new, prev, tail, times, last_cs, late_cs: int = STREAM_LATE_CS, near_cs: int = STREAM_NEAR_CS, max_ngram: int = STREAM_TAIL):
        """wm_stream_agree: the LocalAgreement-2 decision for all live sessions of a tick as one kernel launch (include/wm.h states the contract).
        ``new[s]`` / ``prev[s]`` / ``tail[s]``: the session's hypothesis of this tick, the uncommitted rest of the last one and its last (at most
        STREAM_TAIL) committed words — lists of words, a word a list of text ids; ``times[s]``: int [n, 2] (start, end) of the words of ``new[s]``
        in centiseconds on the recording's clock; ``last_cs[s]``: the end of the last committed word.  Returns ``(skip, commit, ender)``, int32
        [S] each: the session commits ``new[s][skip: skip + commit]``.  Needs the table of ``set_word_table``; touches nothing of the decode
        state; ``last_stream_ms`` holds the hipEvent time of upload + kernel + download."""
        S = len(new)
        if len(prev) != S or len(tail) != S or len(times) != S or len(last_cs) != S:
            raise ValueError("stream_agree: new, prev, tail, times and last_cs must have one entry per session")
        if S == 0:
            self.last_stream_ms = 0.0
            z = np.zeros(0, dtype=np.int32)
            return z, z.copy(), z.copy()
        if any(len(t) > STREAM_TAIL for t in tail):
            raise ValueError(f"stream_agree: tail holds at most STREAM_TAIL = {STREAM_TAIL} words per session")
        arrs = [self._stream_list(nm, l) for nm, l in (("new", new), ("prev", prev), ("tail", tail))]
        if any(len(t) != len(w) for t, w in zip(times, new)):
            raise ValueError("stream_agree: times must have one (start, end) per word of new")
        n_new = int(arrs[0][0][-1])
        tm = np.zeros((max(n_new, 1), 2), dtype=np.int32)
        if n_new:
            tm[:n_new] = np.fromiter(itertools.chain.from_iterable(itertools.chain.from_iterable(times)), dtype=np.int64, count=2 * n_new).reshape(-1, 2)
        last = np.ascontiguousarray([int(x) for x in last_cs], dtype=np.int32)
        lists = [WmStreamList(_ip(w), _ip(t), _ip(i)) for w, t, i in arrs]
        params = WmStreamParams(int(late_cs), int(near_cs), int(max_ngram))
        skip, commit, ender = (np.zeros(S, dtype=np.int32) for _ in range(3))
        ms = C.c_float(0)
        self._check(self.lib.wm_stream_agree(self.h, S, C.byref(lists[0]), C.byref(lists[1]), C.byref(lists[2]), _ip(tm), _ip(last), C.byref(params),
                                             _ip(skip), _ip(commit), _ip(ender), C.byref(ms)), "wm_stream_agree")
        self.last_stream_ms = ms.value
        return skip, commit, ender

    def vad_windows(self, samples_dev: torch.Tensor, n_samples: Sequence[int], params, taps: bool = False):
        """wm_vad_windows: the speech regions of every recording and the windows of at most ``F`` frames that hold them, cut only at pauses (or, in
        speech without pauses, at the quietest frame) — one call, a fixed number of kernel launches, for all recordings.  ``samples_dev``: float32
        [C, n_max] on the GPU, 16 kHz mono; ``n_samples[c]``: the recording's own length, what lies behind it is not read; ``params``: a
        ``WmVadParams`` or a dict of its fields (include/wm.h states the contract).  Returns ``(regions, windows)``, per recording a list of
        ``(start, stop)`` in 10 ms frames; with ``taps=True`` also ``dict(E=[float32 [T_c]..], R=, thr_on=, thr_off=float32 [C])``.  More than
        VAD_WINDOWS_MAX windows: ``ValueError``, split the call.  Touches nothing of the decode state; ``last_vad_ms`` holds the hipEvent time."""
        if not isinstance(params, WmVadParams):
            params = WmVadParams(**dict(params))
        x = samples_dev.to(self.device, torch.float32).contiguous()
        if x.dim() != 2:
            raise ValueError("vad_windows: samples_dev must be [C, n_max]")
        Cn, n_max = x.shape
        ns = np.ascontiguousarray([int(n) for n in n_samples], dtype=np.int64)
        if len(ns) != Cn:
            raise ValueError("vad_windows: n_samples must have one entry per recording")
        T = (np.clip(ns, 0, None) + VAD_HOP - 1) // VAD_HOP
        # the header's bounds: regions are at least min_speech long and min_silence apart, a cut piece is at least F / 2 frames
        ms_, sp_, F_ = max(int(params.min_silence), 1), max(int(params.min_speech), 1), max(int(params.F), 2)
        cap_r = int(np.sum((T + ms_) // (sp_ + ms_) + 1))
        cap_w = cap_r + int(np.sum(T // (F_ // 2)))
        nr, nw = np.zeros(Cn, dtype=np.int32), np.zeros(Cn, dtype=np.int32)
        reg, win = np.zeros((max(cap_r, 1), 2), dtype=np.int32), np.zeros((max(cap_w, 1), 2), dtype=np.int32)
        E = R = on = off = None
        if taps:
            E = np.zeros(max(int(T.sum()), 1), dtype=np.float32)
            R, on, off = (np.zeros(Cn, dtype=np.float32) for _ in range(3))
        ms = C.c_float(0)
        self._inputs_ready()
        self._check(self.lib.wm_vad_windows(self.h, Cn, C.c_void_p(x.data_ptr()), n_max, ns.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(params),
                                            _ip(nr), _ip(reg), cap_r, _ip(nw), _ip(win), cap_w,
                                            None if E is None else _fp(E), None if R is None else _fp(R), None if on is None else _fp(on),
                                            None if off is None else _fp(off), C.byref(ms)), "wm_vad_windows")
        self.last_vad_ms = ms.value
        r0, w0 = np.concatenate([[0], np.cumsum(nr)]), np.concatenate([[0], np.cumsum(nw)])
        regions = [[(int(a), int(b)) for a, b in reg[r0[c]: r0[c + 1]]] for c in range(Cn)]
        windows = [[(int(a), int(b)) for a, b in win[w0[c]: w0[c + 1]]] for c in range(Cn)]
        if not taps:
            return regions, windows
        t0 = np.concatenate([[0], np.cumsum(T)])
        return regions, windows, dict(E=[E[t0[c]: t0[c + 1]].copy() for c in range(Cn)], R=R, thr_on=on, thr_off=off)

    def seq_bias_rows(self, entries, logits: np.ndarray, prefixes: Sequence[Sequence[int]]) -> np.ndarray:
        """Sequence-bias parity tap (wm_seq_bias_rows): rows ``logits [R, V]``, row r under ``prefixes[r]``, through k_seq_bias alone.  Returns the
        edited rows, numpy float32 [R, V]."""
        x, R, pre, lens, Tmax = self._tap_rows("seq_bias_rows", logits, prefixes)
        out = np.zeros_like(x)
        sb, _keep = self._seq_bias_struct(entries)
        self._kv_stamp = object()
        self._check(self.lib.wm_seq_bias_rows(self.h, C.byref(sb), R, _fp(x), _ip(pre), Tmax, _ip(lens), _fp(out)), "wm_seq_bias_rows")
        return out

    def beam_result(self, clip: int, rank: int):
        """wm_get_beam_result: (ids, score) of the finished hypothesis ``rank`` (0 = best) of ``clip`` of the last beam decode."""
        cap = self.cfg.max_target_positions + 16
        buf = (C.c_int32 * cap)()
        n, sc = C.c_int32(0), C.c_float(0)
        self._check(self.lib.wm_get_beam_result(self.h, int(clip), int(rank), buf, cap, C.byref(n), C.byref(sc)), "wm_get_beam_result")
        return list(buf[: min(n.value, cap)]), float(sc.value)

    def beam_reorder_kv(self, beam_idx: Sequence[int], length: int) -> None:
        """wm_beam_reorder_kv: stream s takes over the self K/V rows [0, length) of stream ``beam_idx[s]`` (the reorder of a beam step alone)."""
        idx = np.ascontiguousarray(beam_idx, dtype=np.int32)
        self._kv_stamp = object()
        self._check(self.lib.wm_beam_reorder_kv(self.h, len(idx), idx.ctypes.data_as(C.POINTER(C.c_int32)), int(length)), "wm_beam_reorder_kv")

    def beam_rows(self, gp: GenParams, logits: np.ndarray, prefixes: Sequence[Sequence[int]], num_beams: int, length_penalty: float = 1.0,
                  early_stopping=False, init_scores=None) -> dict:
        """Beam-search parity tap (wm_beam_rows): ``logits [S, G, n, V]`` through the select, bookkeeping and ids-reorder kernels, stream
        g * n + j starting from ``prefixes[g * n + j]`` (one common length) with running score ``init_scores[g * n + j]`` (None: HF's first step).
        Returns numpy arrays cand_val / cand_beam / cand_tok [S, G, 2n], beam_idx [S, G * n], steps [G], fin_ids [G, n, Tmax], fin_len /
        fin_score / fin_set [G, n], run_ids [G * n, Tmax], run_len / run_score [G * n]."""
        x = np.ascontiguousarray(logits, dtype=np.float32)
        S, G, n, V = x.shape
        if V != self.cfg.vocab_size or n != int(num_beams) or len(prefixes) != G * n or len({len(p) for p in prefixes}) != 1:
            raise ValueError("beam_rows: logits must be [S, G, num_beams, vocab] with one prefix per stream, all of one length")
        plen = len(prefixes[0])
        Tmax = plen + S
        pre = np.zeros((G * n, Tmax), dtype=np.int32)
        for s, p in enumerate(prefixes):
            pre[s, :plen] = p
        init = None if init_scores is None else np.ascontiguousarray(init_scores, dtype=np.float32).reshape(G * n)
        o = dict(cand_val=np.zeros((S, G, 2 * n), np.float32), cand_beam=np.zeros((S, G, 2 * n), np.int32), cand_tok=np.zeros((S, G, 2 * n), np.int32),
                 beam_idx=np.zeros((S, G * n), np.int32), steps=np.zeros(G, np.int32), fin_ids=np.zeros((G, n, Tmax), np.int32),
                 fin_len=np.zeros((G, n), np.int32), fin_score=np.zeros((G, n), np.float32), fin_set=np.zeros((G, n), np.int32),
                 run_ids=np.zeros((G * n, Tmax), np.int32), run_len=np.zeros(G * n, np.int32), run_score=np.zeros(G * n, np.float32))
        g, ts, _keep = self._proc_args(gp)
        bp = self._beam_struct(num_beams, length_penalty, early_stopping)
        self._kv_stamp = object()
        self._check(self.lib.wm_beam_rows(self.h, g, ts, C.byref(bp), G, S, _fp(x), _ip(pre), Tmax, plen,
                                          None if init is None else _fp(init), _fp(o["cand_val"]), _ip(o["cand_beam"]), _ip(o["cand_tok"]),
                                          _ip(o["beam_idx"]), _ip(o["steps"]), _ip(o["fin_ids"]), _ip(o["fin_len"]), _fp(o["fin_score"]), _ip(o["fin_set"]),
                                          _ip(o["run_ids"]), _ip(o["run_len"]), _fp(o["run_score"])), "wm_beam_rows")
        return o

    def decode(self, gp: GenParams, B: int, max_iters: int = 1 << 30, on_iteration=None) -> List[List[int]]:
        """``gp.num_beams > 1`` (with ``gp.vanilla``): beam search over B clips (B * num_beams streams); the ids returned are every clip's best
        finished hypothesis, the others are read with ``beam_result``."""
        g, _keep = self._gen_struct(gp)
        self._set_repeat_rules(gp)
        self._set_sampling(gp, B)
        self._set_beam(gp)
        self._set_sequence_bias(gp)
        self._set_constraint(gp)
        self._set_stream_prompts(gp)
        self._kv_stamp = object()             # the decode loop rewrites the self-attention cache: forward()'s cache handles go stale
        if gp.timestamps:                     # WhisperTimeStampLogitsProcessor in the loop (include/wm.h wm_decode_begin_ts)
            ts = self._ts_struct(gp)
            self._check(self.lib.wm_decode_begin_ts(self.h, C.byref(g), C.byref(ts), B), "wm_decode_begin_ts")
        else:
            self._check(self.lib.wm_decode_begin(self.h, C.byref(g), B), "wm_decode_begin")
        left = C.c_int32(0)
        if on_iteration is None:
            self._check(self.lib.wm_decode_run(self.h, max_iters, C.byref(left)), "wm_decode_run")
            return [self.tokens(b) for b in range(B)]
        # streaming: one iteration per call, the tokens each stream gained are handed over as they appear
        seen = [len(gp.prompt)] * B
        it = 0
        while it < max_iters:
            self._check(self.lib.wm_decode_run(self.h, 1, C.byref(left)), "wm_decode_run")
            it += 1
            cur = [self.tokens(b) for b in range(B)]
            stop = on_iteration([cur[b][seen[b]:] for b in range(B)])
            seen = [len(c) for c in cur]
            if left.value == 0 or stop is True:                   # the callback may end the run (host-side stopping criteria)
                break
        return [self.tokens(b) for b in range(B)]

    @staticmethod
    def _pack_ids(lists: Sequence[Sequence[int]], n_prompt=None):
        """Ragged id lists -> (int32 [B, Tmax] zero-padded, int32 [B] lengths, Tmax >= 1, int32 [B] ``n_prompt`` broadcast from an int or
        one per list; None when not given)."""
        B = len(lists)
        Tmax = max(max(len(s) for s in lists), 1)
        tok = np.zeros((B, Tmax), dtype=np.int32)
        for b, s in enumerate(lists):
            tok[b, : len(s)] = s
        lens = np.array([len(s) for s in lists], dtype=np.int32)
        npr = None if n_prompt is None else np.ascontiguousarray(np.broadcast_to(np.asarray(n_prompt, dtype=np.int32), (B,)))
        return tok, lens, Tmax, npr

    def _tap_rows(self, name: str, logits: np.ndarray, prefixes: Optional[Sequence[Sequence[int]]] = None, **per_row):
        """The prelude of a row tap: ``logits [R, vocab]`` -> (contiguous float32 rows, R, the packed prefixes, their lengths, Tmax; ``_pack_ids``).
        ``per_row``: what else comes one per row, under its word in the error text (``stream_key=keys``).  Without prefixes: None, None, 0."""
        x = np.ascontiguousarray(logits, dtype=np.float32)
        items = per_row if prefixes is None else dict(prefix=prefixes, **per_row)
        if x.ndim != 2 or x.shape[1] != self.cfg.vocab_size or any(len(v) != x.shape[0] for v in items.values()):
            words = " and ".join("one " + w.replace("_", " ") for w in items)
            raise ValueError(f"{name}: logits must be [R, vocab]" + (f" with {words} per row" if items else ""))
        pre, lens, Tmax = (None, None, 0) if prefixes is None else self._pack_ids(prefixes)[:3]
        return x, x.shape[0], pre, lens, Tmax

    def _proc_args(self, gp: GenParams, ts: Optional[bool] = None):
        """The logits processors of a tap / scoring call: sets the context's repetition rules from ``gp``, then -> (byref wm_gen_params, byref
        wm_timestamp_params or None, what the two point into: keep it alive over the call).  ``ts``: pass the timestamp struct; None = ``gp.timestamps``
        (the one exception is select_rows)."""
        g, keep = self._gen_struct(gp)
        self._set_repeat_rules(gp)
        t = self._ts_struct(gp) if (gp.timestamps if ts is None else ts) else None
        return C.byref(g), None if t is None else C.byref(t), (g, t, keep)

    def select_rows(self, gp: GenParams, logits: np.ndarray, prefixes: Sequence[Sequence[int]], probe_tokens: Sequence[int]) -> dict:
        """Timestamp parity tap (wm_select_rows): rows ``logits [R, V]`` as verify rows with the given prefixes, through the decode loop's
        state fold and select kernels.  Returns numpy arrays argmax, p_probe, entropy, ts_forced (the log-softmax decision masked all text)."""
        x, R, pre, lens, Tmax = self._tap_rows("select_rows", logits, prefixes, probe_token=probe_tokens)
        probe = np.ascontiguousarray(probe_tokens, dtype=np.int32)
        am = np.zeros(R, np.int32); pp = np.zeros(R, np.float32); H = np.zeros(R, np.float32); fo = np.zeros(R, np.int32)
        # (the repetition rules alone: no timestamp argument; otherwise the timestamp rules as ever)
        g, ts, _keep = self._proc_args(gp, ts=gp.timestamps or not gp.repeat_rules)
        self._kv_stamp = object()
        self._check(self.lib.wm_select_rows(self.h, g, ts, R, _fp(x), _ip(pre), Tmax, _ip(lens), _ip(probe), _ip(am), _fp(pp), _fp(H), _ip(fo)),
                    "wm_select_rows")
        return dict(argmax=am, p_probe=pp, entropy=H, ts_forced=fo)

    def sample_rows(self, gp: GenParams, logits: np.ndarray, prefixes: Sequence[Sequence[int]], keys: Sequence[int], temperature: float,
                    seed: int) -> dict:
        """Sampling parity tap (wm_sample_rows): rows ``logits [R, V]``, row r under its own prefix at position ``len(prefixes[r])`` with stream
        key ``keys[r]``, through k_sample1 / k_sample_fin.  Returns numpy arrays token, value (the winner's v / T + g), ts_forced."""
        x, R, pre, lens, Tmax = self._tap_rows("sample_rows", logits, prefixes, stream_key=keys)
        k64 = _keys64(keys)
        tok = np.zeros(R, np.int32); val = np.zeros(R, np.float32); fo = np.zeros(R, np.int32)
        g, ts, _keep = self._proc_args(gp)
        sp = WmSampleParams(float(temperature), int(seed) & (2 ** 64 - 1), None, 0)
        self._kv_stamp = object()
        self._check(self.lib.wm_sample_rows(self.h, g, ts, C.byref(sp), R, _fp(x), _ip(pre), Tmax, _ip(lens), _u64p(k64), _ip(tok), _fp(val), _ip(fo)),
                    "wm_sample_rows")
        return dict(token=tok, value=val, ts_forced=fo)

    def filter_rows(self, gp: GenParams, logits: np.ndarray, prefixes: Sequence[Sequence[int]], keys: Sequence[int], temperature: float,
                    seed: int, top_k: int = 0, top_p: float = 1.0, min_p: float = 0.0) -> dict:
        """Filter parity tap (wm_filter_rows): ``sample_rows`` with the top-k / top-p / min-p filter, through k_sample1 / k_filter_prep /
        k_filter_row.  Returns numpy arrays thr (the row's threshold; -inf: nothing cut), kept (ids at or above it), ts_forced, token, value."""
        x, R, pre, lens, Tmax = self._tap_rows("filter_rows", logits, prefixes, stream_key=keys)
        k64 = _keys64(keys)
        tok = np.zeros(R, np.int32); val = np.zeros(R, np.float32); fo = np.zeros(R, np.int32)
        thr = np.zeros(R, np.float32); kept = np.zeros(R, np.int32)
        g, ts, _keep = self._proc_args(gp)
        sp = WmSampleParams(float(temperature), int(seed) & (2 ** 64 - 1), None, 0)
        f = WmSampleFilter(int(top_k), float(top_p), float(min_p))
        self._kv_stamp = object()
        self._check(self.lib.wm_filter_rows(self.h, g, ts, C.byref(sp), C.byref(f), R, _fp(x), _ip(pre), Tmax, _ip(lens), _u64p(k64), _fp(thr), _ip(kept),
                                            _ip(fo), _ip(tok), _fp(val)), "wm_filter_rows")
        return dict(thr=thr, kept=kept, ts_forced=fo, token=tok, value=val)

    # ---- token-level timestamps (include/wm.h wm_token_timestamps) ---------------------------------
    def token_timestamps(self, seqs: Sequence[Sequence[int]], n_prompt, alignment_heads: Sequence[Sequence[int]], median_filter_width: int = 7,
                         time_precision: float = 0.02, num_frames=None):
        """Teacher-forced replay of ``seqs`` (one id list per stream of the resident encoder pass: prompt + generated, the stream's own end)
        that taps the alignment heads, then normalisation, median filter and DTW on the GPU (HF _extract_token_timestamps).  ``n_prompt``:
        int or one per stream; ``num_frames``: None, int or one per stream (mel frames of the clip: the attention is cropped to half of it).
        Returns (numpy float32 [B, max len] seconds, ms).  Overwrites the decode state."""
        B = len(seqs)
        heads = np.ascontiguousarray(alignment_heads, dtype=np.int32).reshape(-1, 2)
        tok, lens, Tmax, npr = self._pack_ids(seqs, n_prompt)
        nf = None if num_frames is None else np.ascontiguousarray(np.broadcast_to(np.asarray(num_frames, dtype=np.int32), (B,)))
        out = np.zeros((B, Tmax), dtype=np.float32)
        ms = C.c_float(0)
        ap = WmAlignParams(heads.ctypes.data_as(C.POINTER(C.c_int32)), heads.shape[0], int(median_filter_width), float(time_precision))
        i32p, f32p = C.POINTER(C.c_int32), C.POINTER(C.c_float)
        self._kv_stamp = object()
        self._align_shape = (lens - npr - 1, None if nf is None else nf // 2)
        self._check(self.lib.wm_token_timestamps(self.h, C.byref(ap), B, tok.ctypes.data_as(i32p), Tmax, lens.ctypes.data_as(i32p),
                                                 npr.ctypes.data_as(i32p), None if nf is None else nf.ctypes.data_as(i32p),
                                                 out.ctypes.data_as(f32p), C.byref(ms)), "wm_token_timestamps")
        return out, ms.value

    def _align_nf(self, stream: int):
        N, F = self._align_shape
        S = self.cfg.max_source_positions
        return int(N[stream]), S if F is None else min(int(F[stream]), S)

    def align_probs(self, stream: int, a: int) -> np.ndarray:
        """Parity tap: softmax weights [N, n_ctx] of alignment head ``a`` of the last token_timestamps call."""
        N, _ = self._align_nf(stream)
        out = np.zeros((max(N, 0), self.cfg.max_source_positions), dtype=np.float32)
        self._check(self.lib.wm_get_align_probs(self.h, stream, a, out.ctypes.data_as(C.POINTER(C.c_float))), "wm_get_align_probs")
        return out

    def align_matrix(self, stream: int) -> np.ndarray:
        """Parity tap: the matrix [N, F] the DTW of the last token_timestamps call ran on."""
        N, F = self._align_nf(stream)
        out = np.zeros((max(N, 0), F), dtype=np.float32)
        self._check(self.lib.wm_get_align_matrix(self.h, stream, out.ctypes.data_as(C.POINTER(C.c_float))), "wm_get_align_matrix")
        return out

    def dtw(self, matrix: np.ndarray):
        """Parity tap: HF _dynamic_time_warping(-matrix) by the engine's kernel -> (text_indices, time_indices, first_frame)."""
        m = np.ascontiguousarray(matrix, dtype=np.float32)
        N, F = m.shape
        first = np.zeros(N, np.int32); pt = np.zeros(N + F, np.int32); pm = np.zeros(N + F, np.int32)
        n = C.c_int32(0)
        i32p = C.POINTER(C.c_int32)
        self._check(self.lib.wm_dtw(self.h, m.ctypes.data_as(C.POINTER(C.c_float)), N, F, first.ctypes.data_as(i32p), pt.ctypes.data_as(i32p),
                                    pm.ctypes.data_as(i32p), C.byref(n)), "wm_dtw")
        return pt[: n.value].copy(), pm[: n.value].copy(), first

    # ---- token log-probabilities (include/wm.h wm_score_tokens) -----------------------------------
    def score_tokens(self, seqs: Sequence[Sequence[int]], n_prompt, gp: GenParams, no_speech_token_id: Optional[int] = None, sot_index: int = 0):
        """Teacher-forced replay of ``seqs`` (one id list per stream of the resident encoder pass: prompt + generated, the stream's own end)
        through all decoder layers and the base head, then HF's per-step scores on the GPU: ``log_softmax(processors(z_t), cur_len = t)[s[t]]``
        for every generated position, the timestamp rules included when ``gp.timestamps``.  ``n_prompt``: int or one per stream.
        Returns (numpy float32 [B, max len] log-probabilities — 0 inside the prompt and after a stream's end —, numpy float32 [B]
        no-speech probabilities or None, ms).  Overwrites the decode state."""
        B = len(seqs)
        tok, lens, Tmax, npr = self._pack_ids(seqs, n_prompt)
        out = np.zeros((B, Tmax), dtype=np.float32)
        want_ns = no_speech_token_id is not None and int(no_speech_token_id) >= 0
        nsp = np.zeros(B, dtype=np.float32)
        ms = C.c_float(0)
        g, ts, _keep = self._proc_args(gp)
        sp = WmScoreParams(int(no_speech_token_id) if want_ns else -1, int(sot_index))
        self._kv_stamp = object()
        self._check(self.lib.wm_score_tokens(self.h, g, ts, C.byref(sp), B, _ip(tok), Tmax, _ip(lens), _ip(npr), _fp(out),
                                             _fp(nsp) if want_ns else None, C.byref(ms)), "wm_score_tokens")
        return out, (nsp if want_ns else None), ms.value

    def score_rows(self, gp: GenParams, logits: np.ndarray, prefixes: Sequence[Sequence[int]], targets: Sequence[int]) -> np.ndarray:
        """Scoring parity tap (wm_score_rows): rows ``logits [R, V]``, each under its own prefix and length, through the scoring kernels only.
        Returns numpy float32 [R]: log_softmax(processed row)[target], -inf for a masked target."""
        x, R, pre, lens, Tmax = self._tap_rows("score_rows", logits, prefixes, target=targets)
        tgt = np.ascontiguousarray(targets, dtype=np.int32)
        out = np.zeros(R, np.float32)
        g, ts, _keep = self._proc_args(gp)
        self._kv_stamp = object()
        self._check(self.lib.wm_score_rows(self.h, g, ts, R, _fp(x), _ip(pre), Tmax, _ip(lens), _ip(tgt), _fp(out)), "wm_score_rows")
        return out

    # ---- token alternatives (include/wm.h wm_score_tokens_topk) -------------------------
    def score_tokens_topk(self, seqs: Sequence[Sequence[int]], n_prompt, gp: GenParams, top_k: int, no_speech_token_id: Optional[int] = None,
                          sot_index: int = 0):
        """``score_tokens`` plus the ``top_k`` (1..8) best tokens of every scored row — value descending, then id ascending — and the rank of the
        emitted id in that order (0: masked).  Returns (log-probabilities, no-speech probabilities or None — both as ``score_tokens`` —,
        numpy int32 [B, max len, top_k] ids, float32 [B, max len, top_k] log-probabilities, int32 [B, max len] ranks, ms); -1 / -inf / 0 inside
        the prompt and after a stream's end.  Overwrites the decode state."""
        B = len(seqs)
        tok, lens, Tmax, npr = self._pack_ids(seqs, n_prompt)
        k = int(top_k)
        out = np.zeros((B, Tmax), dtype=np.float32)
        tid = np.full((B, Tmax, max(k, 1)), -1, dtype=np.int32)
        tlp = np.full((B, Tmax, max(k, 1)), -np.inf, dtype=np.float32)
        rk = np.zeros((B, Tmax), dtype=np.int32)
        want_ns = no_speech_token_id is not None and int(no_speech_token_id) >= 0
        nsp = np.zeros(B, dtype=np.float32)
        ms = C.c_float(0)
        g, ts, _keep = self._proc_args(gp)
        sp = WmScoreParams(int(no_speech_token_id) if want_ns else -1, int(sot_index))
        self._kv_stamp = object()
        self._check(self.lib.wm_score_tokens_topk(self.h, g, ts, C.byref(sp), B, _ip(tok), Tmax, _ip(lens), _ip(npr), k, _fp(out),
                                                  _fp(nsp) if want_ns else None, _ip(tid), _fp(tlp), _ip(rk), C.byref(ms)), "wm_score_tokens_topk")
        return out, (nsp if want_ns else None), tid, tlp, rk, ms.value

    def topk_rows(self, gp: GenParams, logits: np.ndarray, prefixes: Sequence[Sequence[int]], targets: Sequence[int], top_k: int):
        """Alternatives parity tap (wm_topk_rows): the rows of ``score_rows`` through the scoring and the top-k kernels.  Returns numpy
        (int32 [R, top_k] ids, float32 [R, top_k] log-probabilities, int32 [R] ranks)."""
        x, R, pre, lens, Tmax = self._tap_rows("topk_rows", logits, prefixes, target=targets)
        tgt = np.ascontiguousarray(targets, dtype=np.int32)
        k = int(top_k)
        tid = np.full((R, max(k, 1)), -1, dtype=np.int32)
        tlp = np.full((R, max(k, 1)), -np.inf, dtype=np.float32)
        rk = np.zeros(R, dtype=np.int32)
        g, ts, _keep = self._proc_args(gp)
        self._kv_stamp = object()
        self._check(self.lib.wm_topk_rows(self.h, g, ts, R, _fp(x), _ip(pre), Tmax, _ip(lens), _ip(tgt), k, _ip(tid), _fp(tlp), _ip(rk)), "wm_topk_rows")
        return tid, tlp, rk

    def tokens(self, stream: int) -> List[int]:
        cap = self.cfg.max_target_positions + 16
        buf = (C.c_int32 * cap)()
        n = C.c_int32(0)
        self._check(self.lib.wm_get_tokens(self.h, stream, buf, cap, C.byref(n)), "wm_get_tokens")
        return list(buf[: min(n.value, cap)])

    def stats(self) -> dict:
        s = WmStats()
        self._check(self.lib.wm_get_stats(self.h, C.byref(s)), "wm_get_stats")
        return dict(iterations=s.iterations, iterations_launched=s.iterations_launched, tokens_emitted=s.tokens_emitted,
                    accept_hist=list(s.accept_hist)[: self.cfg.medusa_num_heads + 1],
                    ms_logmel=s.ms_logmel, ms_encode=s.ms_encode, ms_decode=s.ms_decode,
                    graph_replays=s.graph_replays, schedule_steps=s.schedule_steps, sibling_hits=s.sibling_hits)

    def sync(self):
        self._check(self.lib.wm_sync(self.h), "wm_sync")

    # ---- taps -------------------------------------------------------------------------------
    def encoder_output(self, B: int) -> torch.Tensor:
        out = np.empty((B, self.cfg.max_source_positions, self.cfg.d_model), dtype=np.float32)
        self._check(self.lib.wm_get_encoder_output(self.h, B, out.ctypes.data_as(C.POINTER(C.c_float))), "wm_get_encoder_output")
        return torch.from_numpy(out)

    def encoder_output_cached(self, B: int) -> torch.Tensor:
        """The resident encoder pass's hidden state, fetched from the device once per encoder pass (api.forward's tuple return hands it
        out on every call of a per-token loop: one D2H copy of [B, n_ctx, d] per pass, not per token)."""
        c = getattr(self, "_enc_host", None)
        if c is None or c[0] is not self._enc_stamp or c[1] != B:
            self._enc_host = (self._enc_stamp, B, self.encoder_output(B))
        return self._enc_host[2]

    def cross_kv(self, kv_layer: int, stream: int, head: int):
        S = self.cfg.max_source_positions
        k = np.empty((S, 64), dtype=np.float32); v = np.empty((S, 64), dtype=np.float32)
        self._check(self.lib.wm_get_cross_kv(self.h, kv_layer, stream, head, k.ctypes.data_as(C.POINTER(C.c_float)),
                                             v.ctypes.data_as(C.POINTER(C.c_float))), "wm_get_cross_kv")
        return torch.from_numpy(k), torch.from_numpy(v)

    def forward_logits(self, tokens: Sequence[Sequence[int]], pos0: int, disable_medusa: bool) -> torch.Tensor:
        B, T = len(tokens), len(tokens[0])
        flat = _i32arr([t for row in tokens for t in row])
        n_out = 1 if disable_medusa else self.cfg.medusa_num_heads + 1
        out = np.empty((n_out, B, T, self.cfg.vocab_size), dtype=np.float32)
        # the pass overwrites cache rows pos0 .. pos0 + T: every EngineKVCache handle issued so far goes stale (api.forward hands the
        # caller a fresh one carrying the new stamp) — a later pass at a smaller position can no longer be followed by an old handle
        self._kv_stamp = object()
        self._check(self.lib.wm_forward_logits(self.h, B, flat, T, pos0, 1 if disable_medusa else 0,
                                               out.ctypes.data_as(C.POINTER(C.c_float))), "wm_forward_logits")
        return torch.from_numpy(out)

    def profile_layer_gemms(self, rows: int, reps: int = 50, kernel: int = 0):
        """hipEvent-timed decode GEMMs of decoder layer 0 at `rows` token rows: kernel 0 = all six of a layer, 1..6 = one of them
        (LN1+QKV, out-proj, LN2+cross-q, cross-out, LN3+FC1, FC2), 7 = vocabulary projection.  Returns (ms per repetition, weight bytes)."""
        ms, nbytes = C.c_float(0), C.c_double(0)
        self._check(self.lib.wm_profile_kernel(self.h, kernel, rows, reps, C.byref(ms), C.byref(nbytes)), "wm_profile_kernel")
        return ms.value, nbytes.value
