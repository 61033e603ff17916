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
    - otherwise the tokens after the last pair form an unfinished segment, which is dropped (HF seeks to the last timestamp:
      ``retrieve_segments_and_offset`` returns that seek);
    - with no pair at all, the whole window is one segment ending at its last timestamp (if that is not <|0.00|>), else at the
      window length ``window_frames * time_precision_features``.

    Each segment: ``start`` / ``end`` (float64 tensors, seconds, offset by ``time_offset``), ``tokens`` (LongTensor) and ``result``."""
    return retrieve_segments_and_offset(seq, timestamp_begin, time_precision, time_offset, window_frames, time_precision_features,
                                        result=result)[0]


def retrieve_segments_and_offset(seq: Sequence[int], timestamp_begin: int, time_precision: float = 0.02, time_offset=0.0,
                                 seek_num_frames: int = 3000, time_precision_features: float = 0.01, input_stride: int = 2,
                                 result=None):
    """``retrieve_segments`` of a window that holds ``seek_num_frames`` frames of audio, plus HF's ``segment_offset``: the mel frames the
    sequential long-form loop advances its seek by (``WhisperGenerationMixin._retrieve_segment``).

    - at least one pair of consecutive timestamps and no single timestamp at the end: the unfinished tail is dropped and the next window
      starts at the last pair, ``segment_offset = last_timestamp_pos * input_stride``;
    - otherwise (no pair, or a single timestamp at the end: no speech after it) the whole window is consumed, ``seek_num_frames``.

    ``time_offset``: seconds, a float or a float64 tensor (HF: ``seek * time_precision / input_stride``)."""
    seq = [int(t) for t in seq]
    tb = int(timestamp_begin)
    is_ts = [t >= tb for t in seq]
    single_ending = is_ts[-2:] == [False, True]
    pairs = [i + 1 for i in range(len(seq) - 1) if is_ts[i] and is_ts[i + 1]]
    off = time_offset.to(torch.float64) if isinstance(time_offset, torch.Tensor) else torch.tensor(float(time_offset), dtype=torch.float64)

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
        if single_ending:
            return segments, int(seek_num_frames)
        return segments, (seq[last - 2] - tb) * int(input_stride)
    stamps = [t for t in seq if t >= tb]
    last_pos = torch.tensor(int(seek_num_frames * time_precision_features / time_precision), dtype=torch.float64)
    if stamps and stamps[-1] != tb:
        last_pos = torch.tensor(stamps[-1] - tb, dtype=torch.float64)
    return [seg(off, off + last_pos * time_precision, seq)], int(seek_num_frames)


def row_segments(row: Sequence[int], prompt_len: int, eos_token_id: int, timestamp_begin: int, window_frames: int,
                 time_precision: float = 0.02, time_precision_features: float = 0.01, time_offset: float = 0.0,
                 result: Optional[torch.Tensor] = None) -> List[dict]:
    """``retrieve_segments`` of one padded output row (prompt + generated ids + EOS / padding)."""
    return retrieve_segments(generated_ids(row, prompt_len, eos_token_id), timestamp_begin, time_precision, time_offset,
                             window_frames, time_precision_features, result)


def sequential_seek_loop(max_frames: Sequence[int], window_frames: int, decode_round, timestamp_begin: int, time_precision: float = 0.02,
                         time_precision_features: float = 0.01, input_stride: int = 2) -> List[List[dict]]:
    """Whisper's sequential long-form loop over a batch of recordings (openai/whisper ``transcribe``; HF ``WhisperGenerationMixin.generate``
    on more than one window of features), with HF's quantities under HF's names.

    ``seek[b] = 0``; while any ``seek[b] < max_frames[b]``: the active clips form one round.  Per active clip ``seek_num_frames =
    min(window_frames, max_frames - seek)`` and ``time_offset = seek * time_precision / input_stride``; ``decode_round(clips, seeks,
    seek_num_frames)`` (three equally long int lists) gathers, encodes and decodes the windows and returns, per window, a dict with ``ids``
    (the generated ids: no prompt, no EOS), ``skipped`` (the no-speech gate's verdict) and ``result``.  A skipped window gives no segments
    and advances by ``seek_num_frames`` (HF's ``should_skip``); any other advances by ``retrieve_segments_and_offset``'s segment_offset.

    Returns, per clip, its window records in order: the round's dict plus ``seek``, ``seek_num_frames``, ``time_offset`` (float64 tensor),
    ``segments`` and ``segment_offset``."""
    B, F = len(max_frames), int(window_frames)
    max_frames = [int(v) for v in max_frames]
    seek = [0] * B
    windows: List[List[dict]] = [[] for _ in range(B)]
    while any(seek[b] < max_frames[b] for b in range(B)):
        clips = [b for b in range(B) if seek[b] < max_frames[b]]
        snf = [min(F, max_frames[b] - seek[b]) for b in clips]
        got = decode_round(clips, [seek[b] for b in clips], snf)
        if len(got) != len(clips):
            raise RuntimeError("sequential long-form: the round returned another number of windows than it was given")
        for b, n, w in zip(clips, snf, got):
            rec = dict(w, seek=seek[b], seek_num_frames=n,
                       time_offset=torch.tensor(seek[b], dtype=torch.float64) * time_precision / input_stride)
            if rec.get("skipped"):
                rec["ids"], rec["segments"], rec["segment_offset"] = [], [], n
            else:
                rec["segments"], rec["segment_offset"] = retrieve_segments_and_offset(
                    rec["ids"], timestamp_begin, time_precision, rec["time_offset"], n, time_precision_features, input_stride,
                    result=rec.get("result"))
            # HF's rules cannot yield 0 (the last pair cannot sit at <|0.00|> behind text): raise rather than decode the same window for ever
            if rec["segment_offset"] <= 0:
                raise RuntimeError(f"sequential long-form: clip {b} would not advance at frame {seek[b]} (segment_offset "
                                   f"{rec['segment_offset']}, ids {rec['ids']})")
            seek[b] += rec["segment_offset"]
            windows[b].append(rec)
    return windows


def assemble_sequence(prompt: Sequence[int], windows: Sequence[dict], eos_token_id: int) -> List[int]:
    """One clip's ``sequences`` row of the sequential loop: the prompt once, the tokens of every kept segment of every window in order
    (timestamp tokens stay relative to their window, as in HF), then one EOS."""
    ids = [int(t) for t in prompt]
    for w in windows:
        for sg in w["segments"]:
            ids += [int(t) for t in sg["tokens"].tolist()]
    return ids + [int(eos_token_id)]
