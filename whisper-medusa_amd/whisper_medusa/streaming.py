"""Live transcription: streaming sessions under the LocalAgreement-2 policy of Macháček et al., "Turning Whisper into Real-Time
Transcription System" (2023).  A recording grows chunk by chunk; on every tick the rolling buffers of ALL sessions that are due are transcribed
again as one ``generate(return_word_timestamps=True)`` batch, and one ``engine.stream_agree`` call (csrc/wm_stream.hip: one kernel launch)
decides for all of them which words two consecutive hypotheses agree on.  Those are committed; committed audio is cut from the front of the buffer.

The layer touches the engine only through ``model.extract_features``, ``model.generate``, ``model.engine.stream_agree``, ``model.config`` and
``model.device``.  All times are whole centiseconds on the recording's clock; a buffer always starts on a centisecond (160 samples)."""
import time
from typing import List, Optional, Sequence

import numpy as np
import torch

HOP = 160                                                   # samples per centisecond at 16 kHz: the log-mel's hop
TAIL = 5                                                    # WM_STREAM_TAIL (include/wm.h)
REFUSED_FLAGS = ("sequential_longform", "chunk_longform", "vad_longform")


class _Word:
    __slots__ = ("text", "ids", "start", "end", "prob")

    def __init__(self, text, ids, start, end, prob=None):
        self.text, self.ids, self.start, self.end, self.prob = text, ids, start, end, prob

    def public(self) -> dict:
        w = {"text": self.text, "timestamp": (self.start / 100.0, self.end / 100.0), "ids": list(self.ids)}
        if self.prob is not None:
            w["probability"] = self.prob
        return w


class _Session:
    __slots__ = ("length", "offset_cs", "committed", "pending", "last_cs", "sentence_cs", "lost_cs", "since")

    def __init__(self):
        self.length = 0                 # samples in the buffer
        self.offset_cs = 0              # the recording clock of the buffer's first sample
        self.committed: List[_Word] = []
        self.pending: List[_Word] = []
        self.last_cs = 0                # end of the last committed word
        self.sentence_cs = 0            # end of the last committed word that ends a sentence
        self.lost_cs = 0                # uncommitted audio cut by the overflow rule
        self.since = 0                  # samples received since the last decode


def check_generate_kwargs(kw: dict) -> None:
    """What a streaming session cannot pass to generate(): each refusal names its keyword."""
    if kw.get("streamer") is not None:
        raise NotImplementedError("stream_sessions: streamer= is not supported (a session returns its words from feed())")
    if kw.get("num_beams") not in (None, 1):
        raise NotImplementedError("stream_sessions: num_beams > 1 is not supported (one hypothesis per session and tick)")
    if kw.get("num_return_sequences") not in (None, 1):
        raise NotImplementedError("stream_sessions: num_return_sequences > 1 is not supported (one hypothesis per session and tick)")
    if kw.get("return_timestamps"):
        raise NotImplementedError("stream_sessions: return_timestamps is not supported (the buffer is one window; words carry their times)")
    for flag in REFUSED_FLAGS:
        if kw.get(flag):
            raise NotImplementedError(f"stream_sessions: {flag} is not supported (the buffer of a session is one short-form window)")


class StreamSessions:
    """``n`` live sessions over one model (``model.stream_sessions`` builds it).  ``feed(chunks)`` appends audio, decodes the sessions that are
    due as one batch and returns what every session committed; ``finish`` / ``reset`` / ``transcript`` as their names say; ``last_stats`` holds
    ``n_due``, ``batches``, ``ms_generate`` (host clock around extract_features + generate), ``ms_agree`` (the kernel call's event time) and
    ``ms_feed`` (host clock around the whole call)."""

    def __init__(self, model, n: int, *, max_batch: Optional[int] = None, tokenizer=None, word_table=None, min_chunk_s: float = 1.0,
                 trim_s: Optional[float] = None, hard_trim_s: Optional[float] = None, late_s: float = 0.1, near_s: float = 1.0, **generate_kwargs):
        if int(n) < 1:
            raise ValueError("stream_sessions: n must be at least 1")
        check_generate_kwargs(generate_kwargs)
        if tokenizer is None and word_table is None:
            raise ValueError("return_word_timestamps=True needs the bytes of the vocabulary: pass tokenizer= (or word_table=)")
        self.model, self.n = model, int(n)
        self.window = HOP * int(model.config.n_mel_frames)              # samples: 30 s on real checkpoints
        self.max_batch = max(int(max_batch if max_batch is not None else n), 1)
        self.min_chunk = int(round(float(min_chunk_s) * 16000))
        w_cs = self.window // HOP
        self.trim_cs = w_cs // 2 if trim_s is None else int(round(float(trim_s) * 100))
        self.hard_trim_cs = 5 * w_cs // 6 if hard_trim_s is None else int(round(float(hard_trim_s) * 100))
        self.late_cs, self.near_cs = int(round(float(late_s) * 100)), int(round(float(near_s) * 100))
        self.kw = dict(generate_kwargs)
        self.kw["return_word_timestamps"] = True
        if word_table is not None:
            self.kw["word_table"] = word_table
        if tokenizer is not None:
            self.kw["tokenizer"] = tokenizer
        self.buf = torch.zeros(self.n, self.window, dtype=torch.float32, device=model.device)
        self.s = [_Session() for _ in range(self.n)]
        self.last_stats = dict(n_due=0, batches=0, ms_generate=0.0, ms_agree=0.0, ms_feed=0.0)

    # ---- the buffer ---------------------------------------------------------------------------------------------------------------------------
    def _cut(self, i: int, c: int) -> None:
        """Drop the audio of session i in front of centisecond ``c`` (offset_cs < c <= the buffer's end): shift the row, zero what the shift frees."""
        s = self.s[i]
        shift = (c - s.offset_cs) * HOP
        keep = s.length - shift
        row = self.buf[i]
        if keep > 0:
            row[:keep] = row[shift: s.length].clone()
        row[max(keep, 0): s.length] = 0.0                   # exact zeros: the log-mel sees zero padding
        s.length, s.offset_cs = max(keep, 0), c

    def _append(self, i: int, x: torch.Tensor) -> None:
        s = self.s[i]
        excess = s.length + x.numel() - self.window
        if excess > 0:                                      # the front goes first; committed audio (up to last_cs, as far as the buffer holds it) with it
            c = max(min(s.last_cs, s.offset_cs + s.length // HOP), s.offset_cs + -(-excess // HOP))
            s.lost_cs += max(0, c - max(s.last_cs, s.offset_cs))
            over = (c - s.offset_cs) * HOP - s.length       # > 0: the cut lies inside the chunk (a chunk of nearly a whole window)
            self._cut(i, c)
            if over > 0:
                x = x[over:]
        self.buf[i, s.length: s.length + x.numel()] = x.to(self.buf.device)
        s.length += x.numel()

    def _chunk(self, c) -> Optional[torch.Tensor]:
        if c is None:
            return None
        x = c.detach() if isinstance(c, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(c, dtype=np.float32)))
        if x.dim() != 1:
            raise ValueError(f"feed: a chunk is 1-D mono audio, got {x.dim()} dimensions (feed every session its own chunk)")
        if x.numel() > self.window:
            raise ValueError(f"feed: a chunk of {x.numel()} samples is longer than the window of {self.window}: feed it in pieces")
        return x.to(torch.float32) if x.numel() else None

    # ---- a tick -------------------------------------------------------------------------------------------------------------------------------
    def feed(self, chunks: Sequence, sampling_rate: int = 16000) -> List[dict]:
        """``chunks[i]``: 1-D float32 16 kHz audio for session i, or None / empty.  Returns one dict per session: ``committed`` (the words
        committed by this call), ``pending``, ``offset_s``, ``buffer_s``, ``decoded``, ``lost_s``."""
        t0 = time.perf_counter()
        if int(sampling_rate) != 16000:
            raise ValueError(f"feed: sampling_rate={sampling_rate}: a session takes 16 kHz audio (resample the stream in front of it)")
        if len(chunks) != self.n:
            raise ValueError(f"feed: {len(chunks)} chunks for {self.n} sessions (None for a session without new audio)")
        xs = [self._chunk(c) for c in chunks]               # every chunk is checked before any session changes
        for i, x in enumerate(xs):
            if x is not None:
                self._append(i, x)
                self.s[i].since += x.numel()
        due = [i for i in range(self.n) if self.s[i].length > 0 and self.s[i].since >= self.min_chunk and self.s[i].since > 0]
        new_words = {i: [] for i in due}
        ms_gen, batches = 0.0, 0
        for g in range(0, len(due), self.max_batch):
            grp = due[g: g + self.max_batch]
            t1 = time.perf_counter()
            feats = self.model.extract_features(self.buf[grp] if len(grp) < self.n else self.buf)
            out = self.model.generate(feats, **self.kw)
            ms_gen += (time.perf_counter() - t1) * 1e3
            batches += 1
            rows = out["sequences"].tolist()
            for b, i in enumerate(grp):
                off = self.s[i].offset_cs
                for w in out["words"][b]:
                    a, z = w["tokens"]
                    new_words[i].append(_Word(w["text"], [int(t) for t in rows[b][a:z]], int(round(w["timestamp"][0] * 100)) + off,
                                              int(round(w["timestamp"][1] * 100)) + off, w.get("probability")))
        ms_agree = 0.0
        done = {i: [] for i in range(self.n)}
        if due:
            tails = [[w for w in self.s[i].committed[-TAIL:] if w.end > self.s[i].offset_cs] for i in due]
            skip, commit, ender = self.model.engine.stream_agree(
                [[w.ids for w in new_words[i]] for i in due], [[w.ids for w in self.s[i].pending] for i in due], [[w.ids for w in t] for t in tails],
                [[(w.start, w.end) for w in new_words[i]] for i in due], [self.s[i].last_cs for i in due],
                late_cs=self.late_cs, near_cs=self.near_cs, max_ngram=TAIL)
            ms_agree = float(getattr(self.model.engine, "last_stream_ms", 0.0))
            for k, i in enumerate(due):
                s, nw = self.s[i], new_words[i]
                k0, m, e = int(skip[k]), int(commit[k]), int(ender[k])
                done[i] = nw[k0: k0 + m]
                s.committed += done[i]
                s.pending = nw[k0 + m:]
                if m:
                    s.last_cs = done[i][-1].end
                if e >= 0:
                    s.sentence_cs = nw[e].end
                s.since = 0
                self._trim(i)
        self.last_stats = dict(n_due=len(due), batches=batches, ms_generate=ms_gen, ms_agree=ms_agree, ms_feed=0.0)
        isdue = set(due)
        res = [self._result(i, done[i], i in isdue) for i in range(self.n)]
        self.last_stats["ms_feed"] = (time.perf_counter() - t0) * 1e3
        return res

    def _trim(self, i: int) -> None:
        s = self.s[i]
        d = s.length // HOP
        if d <= self.trim_cs:
            return
        if s.sentence_cs > s.offset_cs:
            c = s.sentence_cs
        elif d > self.hard_trim_cs and s.last_cs > s.offset_cs:
            c = s.last_cs
        else:
            return
        self._cut(i, min(c, s.offset_cs + d))               # (a word may end in the zero padding behind the audio: the cut stays inside the audio)

    def _result(self, i: int, committed: List[_Word], decoded: bool) -> dict:
        s = self.s[i]
        return dict(committed=[w.public() for w in committed], pending=[w.public() for w in s.pending], offset_s=s.offset_cs / 100.0,
                    buffer_s=s.length / 16000.0, decoded=bool(decoded), lost_s=s.lost_cs / 100.0)

    # ---- the other doors ----------------------------------------------------------------------------------------------------------------------
    def _which(self, which) -> List[int]:
        idx = list(range(self.n)) if which is None else ([int(which)] if isinstance(which, (int, np.integer)) else [int(i) for i in which])
        for i in idx:
            if not 0 <= i < self.n:
                raise IndexError(f"session {i} of {self.n}")
        return idx

    def finish(self, which=None) -> List[List[dict]]:
        """Commit the pending words of those sessions (default: all) as they stand, without a decode; returns them per session, in the order
        of ``which``, and resets those sessions (read ``transcript(i)`` first if the whole text is wanted)."""
        out = []
        for i in self._which(which):
            s = self.s[i]
            out.append([w.public() for w in s.pending])
            s.committed += s.pending
            s.pending = []
        self.reset(which)
        return out

    def reset(self, which=None) -> None:
        """Drop everything of those sessions (default: all): audio, words, clock."""
        for i in self._which(which):
            self.buf[i].zero_()
            self.s[i] = _Session()

    def transcript(self, i: int) -> str:
        """The committed text of session i so far."""
        return "".join(w.text for w in self.s[self._which(i)[0]].committed).strip()

    def committed_words(self, i: int) -> List[dict]:
        """All committed words of session i so far."""
        return [w.public() for w in self.s[self._which(i)[0]].committed]
