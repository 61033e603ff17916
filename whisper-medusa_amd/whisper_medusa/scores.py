"""Host side of the token log-probabilities (engine: csrc/wm_score.hip): the per-clip figures HF's Whisper front end derives
from the scores of a decode, and the gating rule built on them.  Pure Python; importable without a GPU.

    avg_logprob        WhisperGenerationMixin._retrieve_avg_logprobs: the sum of the generated tokens' log-probabilities — the one EOS
                       included — divided by their number
    compression_ratio  WhisperGenerationMixin._retrieve_compression_ratio: bytes of the generated ids over their zlib-compressed bytes
    should_skip        openai-whisper's no-speech rule (transcribe.py: no_speech_prob > no_speech_threshold, unless the average
                       log-probability clears logprob_threshold) — HF's `_need_fallback` wherever HF's is defined (it needs a
                       logprob_threshold)
    needs_fallback     HF `_need_fallback`: the compression ratio above its threshold or the average log-probability below its own; a skipped
                       clip needs none
"""
from __future__ import annotations

import math
import zlib
from typing import Optional, Sequence

import numpy as np


TOPK_MAX = 8            # include/wm.h WM_TOPK_MAX: alternatives per scored row (generate(top_logprobs=k))
TOPK_FIELDS = ("top_token_ids", "top_token_logprobs", "token_ranks")


def topk_fills(n: int, k: int):
    """The alternative fields of ``n`` positions nothing was scored at: ids -1 [n, k], log-probabilities -inf [n, k], ranks 0 [n]."""
    return np.full((n, k), -1, dtype=np.int64), np.full((n, k), -np.inf, dtype=np.float32), np.zeros(n, dtype=np.int64)


def avg_logprob(token_logprobs: Sequence[float], n_prompt: int, length: int) -> float:
    """Mean of ``token_logprobs[n_prompt:length]`` (``length`` = the stream's own end, EOS included); 0.0 for an empty range.  The sum runs
    in the order and the precision HF's Python ``sum`` over float32 tensors takes, so the figure is HF's bit for bit."""
    n = int(length) - int(n_prompt)
    if n <= 0:
        return 0.0
    total = np.float32(0.0)
    with np.errstate(invalid="ignore", over="ignore"):
        for v in token_logprobs[int(n_prompt): int(length)]:
            total = np.float32(total + np.float32(v))
        return float(np.float32(total / np.float32(n)))


def compression_ratio(tokens: Sequence[int], vocab_size: int) -> float:
    """len(raw bytes) / len(zlib bytes) of the ids, every id as ``int(log2(vocab_size) / 8) + 1`` little-endian bytes.  An empty list has no
    ratio: 0.0 (never above a threshold)."""
    toks = [int(t) for t in tokens]
    if not toks:
        return 0.0
    length = int(math.log2(vocab_size) / 8) + 1
    raw = b"".join(t.to_bytes(length, "little") for t in toks)
    return len(raw) / len(zlib.compress(raw))


def should_skip(no_speech_prob: Optional[float], avg_lp: float, no_speech_threshold: Optional[float],
                logprob_threshold: Optional[float]) -> bool:
    if no_speech_threshold is None or no_speech_prob is None:
        return False
    if not (float(no_speech_prob) > float(no_speech_threshold)):
        return False
    return logprob_threshold is None or float(avg_lp) < float(logprob_threshold)


def needs_fallback(avg_lp: float, ratio: float, logprob_threshold: Optional[float], compression_ratio_threshold: Optional[float],
                   skipped: bool = False) -> bool:
    if skipped:
        return False
    need = False
    if compression_ratio_threshold is not None and float(ratio) > float(compression_ratio_threshold):
        need = True
    if logprob_threshold is not None and float(avg_lp) < float(logprob_threshold):
        need = True
    return need


def gate(no_speech_prob: Optional[float], avg_lp: float, ratio: float, no_speech_threshold: Optional[float] = None,
         logprob_threshold: Optional[float] = None, compression_ratio_threshold: Optional[float] = None):
    """(needs_fallback, should_skip) of one clip, as HF's `_need_fallback` returns them."""
    skip = should_skip(no_speech_prob, avg_lp, no_speech_threshold, logprob_threshold)
    return needs_fallback(avg_lp, ratio, logprob_threshold, compression_ratio_threshold, skip), skip
