"""``vad_options`` of ``generate_from_wav(vad_longform=True)`` / ``detect_speech``, lowered to the parameters of the engine's wm_vad_windows
(include/wm.h).  The detector is an energy detector with a stated contract, not a trained VAD model, and the defaults below are
untuned: the project has no real checkpoint and no real speech to tune them on."""
import math

import numpy as np

FRAME_MS = 10                                   # a frame is the log-mel's hop: 160 samples at 16 kHz
DEFAULTS = dict(onset_db=-30.0, offset_db=-35.0, loud_percentile=95.0, min_level_dbfs=-60.0, min_silence_ms=500, min_speech_ms=250,
                speech_pad_ms=200, max_window_s=None)


def _number(name, v):
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(float(v)):
        raise ValueError(f"vad_options: `{name}` has to be a finite number, but is {v!r}")
    return float(v)


def _frames(name, v, least):
    v = _number(name, v)
    if v != round(v) or int(round(v)) % FRAME_MS != 0:
        raise ValueError(f"vad_options: `{name}` has to be a whole multiple of {FRAME_MS} ms, but is {v!r}")
    f = int(round(v)) // FRAME_MS
    if f < least:
        raise ValueError(f"vad_options: `{name}` has to be at least {least * FRAME_MS} ms, but is {v!r}")
    return f


def lower_options(vad_options, window_frames: int) -> dict:
    """The wm_vad_params fields of ``vad_options`` (None: the defaults) for a model whose window is ``window_frames`` frames.  dB values are
    relative powers: ``k = float32(10 ** (dB / 10))``; ``abs_on = float32(160 * 10 ** (min_level_dbfs / 10))`` is the energy of a frame of 160
    samples at that level, ``abs_off = abs_on * k_off / k_on`` in float32.  Every bad value or unknown key is a ValueError."""
    opts = dict(DEFAULTS)
    if vad_options is not None:
        if not isinstance(vad_options, dict):
            raise ValueError(f"vad_options has to be a dict, but is {type(vad_options).__name__}")
        unknown = sorted(set(vad_options) - set(DEFAULTS))
        if unknown:
            raise ValueError(f"vad_options: unknown key(s) {unknown}; known: {sorted(DEFAULTS)}")
        opts.update(vad_options)
    on_db, off_db = _number("onset_db", opts["onset_db"]), _number("offset_db", opts["offset_db"])
    if off_db > on_db:
        raise ValueError(f"vad_options: `offset_db` ({off_db}) must not lie above `onset_db` ({on_db})")
    with np.errstate(over="ignore"):                # (a value that leaves the float32 range is an error below, not a warning)
        k_on, k_off = np.float32(10.0 ** (on_db / 10.0)), np.float32(10.0 ** (off_db / 10.0))
    if not (0.0 < k_off <= k_on and np.isfinite(k_on)):
        raise ValueError(f"vad_options: `onset_db` / `offset_db` ({on_db}, {off_db}) leave the float32 range")
    pct = _number("loud_percentile", opts["loud_percentile"])
    if not 0.0 <= pct <= 100.0:
        raise ValueError(f"vad_options: `loud_percentile` has to be in [0, 100], but is {pct}")
    with np.errstate(over="ignore"):
        abs_on = np.float32(160.0 * 10.0 ** (_number("min_level_dbfs", opts["min_level_dbfs"]) / 10.0))
    if not np.isfinite(abs_on):
        raise ValueError(f"vad_options: `min_level_dbfs` ({opts['min_level_dbfs']}) leaves the float32 range")
    abs_off = np.float32(np.float32(abs_on * k_off) / k_on)
    F = int(window_frames)
    if opts["max_window_s"] is not None:
        w = _number("max_window_s", opts["max_window_s"]) * 100.0
        if abs(w - round(w)) > 1e-6 or not 2 <= int(round(w)) <= window_frames:
            raise ValueError(f"vad_options: `max_window_s` has to be a whole number of 10 ms frames between 0.02 s and the model's window of "
                             f"{window_frames * 0.01:g} s, but is {opts['max_window_s']!r}")
        F = int(round(w))
    return dict(k_on=float(k_on), k_off=float(k_off), abs_on=float(abs_on), abs_off=float(min(abs_off, abs_on)),
                q_permille=int(round(pct * 10.0)), min_silence=_frames("min_silence_ms", opts["min_silence_ms"], 1),
                min_speech=_frames("min_speech_ms", opts["min_speech_ms"], 1), pad=_frames("speech_pad_ms", opts["speech_pad_ms"], 0), F=F)
