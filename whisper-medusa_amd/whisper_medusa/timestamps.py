"""Segments of a timestamped Whisper decode (``generate(return_timestamps=True, return_segments=True)``).

The splitting rule is HF's ``WhisperGenerationMixin._retrieve_segment`` (transformers models/whisper/generation_whisper.py),
restated over plain token ids: no device work, no model.  Timestamp token ``t >= timestamp_begin`` means
``(t - timestamp_begin) * time_precision`` seconds from the start of its 30 s window.
"""
from __future__ import annotations

from typing import List, Optional, Sequence

import torch


def generated_ids(row: Sequence[int], prompt_len: int, eos_token_id: int) -> List[int]:
    """The generated ids of one output row: after the prompt, up to (not including) the first EOS."""
    out = []
    for t in list(row)[prompt_len:]:
        t = int(t)
        if t == eos_token_id:
            break
        out.append(t)
    return out


def retrieve_segments(seq: Sequence[int], timestamp_begin: int, time_precision: float = 0.02, time_offset: float = 0.0,
                      window_frames: int = 3000, time_precision_features: float = 0.01, result=None) -> List[dict]:
    """Segments of one window's generated ids ``seq`` (no prompt, no EOS):

    - a segment ends at every pair of consecutive timestamp tokens;
    - a single timestamp at the very end closes the last segment at it (HF: no speech after it);
    - otherwise the tokens after the last pair form an unfinished segment, which is dropped (HF seeks to the last timestamp);
    - with no pair at all, the whole window is one segment ending at its last timestamp (if that is not <|0.00|>), else at the
      window length ``window_frames * time_precision_features``.

    Each segment: ``start`` / ``end`` (float64 tensors, seconds, offset by ``time_offset``), ``tokens`` (LongTensor) and ``result``."""
    seq = [int(t) for t in seq]
    tb = int(timestamp_begin)
    is_ts = [t >= tb for t in seq]
    single_ending = is_ts[-2:] == [False, True]
    pairs = [i + 1 for i in range(len(seq) - 1) if is_ts[i] and is_ts[i + 1]]
    off = torch.tensor(float(time_offset), dtype=torch.float64)

    def seg(start, end, toks):
        return {"start": start, "end": end, "tokens": torch.tensor(toks, dtype=torch.long), "result": result}

    if pairs:
        slices = list(pairs)
        if single_ending:
            slices.append(len(seq))
        else:
            slices[-1] += 1             # the last pair's second timestamp belongs to the last segment
        segments, last = [], 0
        for i, cur in enumerate(slices):
            is_last = i == len(slices) - 1
            toks = seq[last:cur]
            start_pos = toks[0] - tb
            end_pos = toks[-1 if (not is_last or single_ending) else -2] - tb
            segments.append(seg(off + torch.tensor(start_pos, dtype=torch.float64) * time_precision,
                                off + torch.tensor(end_pos, dtype=torch.float64) * time_precision, toks))
            last = cur
        return segments
    stamps = [t for t in seq if t >= tb]
    last_pos = torch.tensor(int(window_frames * time_precision_features / time_precision), dtype=torch.float64)
    if stamps and stamps[-1] != tb:
        last_pos = torch.tensor(stamps[-1] - tb, dtype=torch.float64)
    return [seg(off, off + last_pos * time_precision, seq)]


def row_segments(row: Sequence[int], prompt_len: int, eos_token_id: int, timestamp_begin: int, window_frames: int,
                 time_precision: float = 0.02, time_precision_features: float = 0.01, time_offset: float = 0.0,
                 result: Optional[torch.Tensor] = None) -> List[dict]:
    """``retrieve_segments`` of one padded output row (prompt + generated ids + EOS / padding)."""
    return retrieve_segments(generated_ids(row, prompt_len, eos_token_id), timestamp_begin, time_precision, time_offset,
                             window_frames, time_precision_features, result)
