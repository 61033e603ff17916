"""Helpers of the sequential long-form tests (tests/test_longform_seek_cpu.py, tests/test_gpu_longform_seek.py; no test in here).

The reference loop: per window torch slicing plus zero pad on the ORACLE's whole-recording log-mel (HF `_get_input_segment`), the oracle's
encoder, `Ref.decode` of tests/test_gpu_timestamps.py (the oracle's chain loop with transformers' WhisperTimeStampLogitsProcessor on every
row) and transformers' own `WhisperGenerationMixin._retrieve_segment` for the segments and the seek.  Nothing of the package under test is
in it but the generation parameters `generate()` itself builds.

SEED / CLIPS: the checkpoint seed and the recordings of the end-to-end runs, chosen on the CPU with this reference alone (the search is
`python tests/longform_seek.py --search 24 12`); tests/test_longform_seek_cpu.py asserts the three conditions they were chosen under."""
import sys

import numpy as np
import torch
import torch.nn.functional as F

from helpers import synth
from oracle.whisper_medusa_oracle import log_mel
from test_gpu_timestamps import micro_ts, state_dict, Ref, TIE, TIE_P, TS_SCALE
from scores_ref import no_speech_prob
from whisper_medusa import WhisperMedusaModel

HEADS = "base_head"
MAX_NEW = 12
WINDOW = 192 * 160                                  # samples of one window of the micro shape (192 frames)
MARGIN = 10.0                                       # every decision margin >= MARGIN x the tie tolerances (the rule of tests/long_history.py)
# lengths in samples: about 2.3, 1.0 and 3.6 windows, none a multiple of 160 (the last partial hop is dropped: frames = len // 160)
LENGTHS = (70_700, 30_500, 110_650)
# checkpoint seed; per recording (clip index of synth.synth_clip, gains of its half windows: `recording`): see the module docstring
SEED = 24
CLIPS = ((660, (0.0, 1.0, 0.1, 1.0, 1.0)), (543, (1.0, 1.0)), (797, (0.0, 0.003, 1.0, 0.0, 0.003, 0.1, 1.0, 1.0)))


def checkpoint(seed=SEED):
    cfg = micro_ts(HEADS)
    return cfg, state_dict(cfg, seed, TS_SCALE)


def gen_params(cfg, sd, max_new=MAX_NEW):
    """What generate(return_timestamps=True, max_new_tokens=max_new) decodes every window under (no device needed)."""
    return WhisperMedusaModel(cfg, sd)._gen_params(None, None, None, max_new, None, None, False, None, None, None, None, None, timestamps=True)


def recording(clip, n, gains=(1.0,)):
    """synth.synth_clip(clip) of n samples, every half window of it scaled by the next of `gains` (cyclic): loud, quiet and silent stretches
    give the windows of one recording different features — the per-recording clamp flattens the quiet ones — and with them different ids."""
    w = synth.synth_clip(clip, n_samples=n).copy()
    h = WINDOW // 2
    for j in range(0, n, h):
        w[j: j + h] *= np.float32(gains[(j // h) % len(gains)])
    return w


def padded_len(lengths):
    return max(160, -(-max(lengths) // 160) * 160)


def oracle_features(cfg, wavs):
    """extract_features(truncation=False) by the oracle: zero pad as audio to the longest (a multiple of 160), log-mel of the whole."""
    n = padded_len([len(w) for w in wavs])
    return torch.stack([torch.from_numpy(log_mel(w, cfg.num_mel_bins, n)) for w in wavs]), [len(w) // 160 for w in wavs]


def hf_retrieve(gen, P, tb, seek, seek_num_frames, time_precision=0.02, time_precision_features=0.01, input_stride=2):
    """transformers' `_retrieve_segment` on one window's generated ids -> (segments, segment_offset); time_offset as HF's loop computes it."""
    from transformers.models.whisper.generation_whisper import WhisperGenerationMixin
    off = torch.tensor([seek], dtype=torch.float64) * time_precision / input_stride
    segs, so = WhisperGenerationMixin._retrieve_segment(
        seek_sequence=torch.tensor(gen, dtype=torch.long), seek_outputs=[None], time_offset=off, timestamp_begin=tb,
        seek_num_frames=[seek_num_frames], time_precision=time_precision, time_precision_features=time_precision_features,
        input_stride=input_stride, prev_idx=0, idx=0, return_token_timestamps=False, decoder_input_ids=torch.zeros(1, P, dtype=torch.long))
    return segs, int(so)


def generated(ids, P, eos):
    g = ids[P:]
    return g[: g.index(eos)] if eos in g else g


@torch.no_grad()
def reference_recording(ref, cfg, gp, feats, max_frames, no_speech_threshold=None, stop_below=None):
    """The sequential loop over ONE recording's oracle features [n_mels, frames].  Returns the window records: seek, seek_num_frames, ids
    (generated, no EOS), segments, segment_offset, no_speech_prob, skipped, and the smallest (logit, relative p_c) margins Ref recorded.
    `stop_below` = (logit, rel): give up (None) at the first window with a smaller margin (the search)."""
    Fw, P, tb = cfg.n_mel_frames, len(gp.prompt), cfg.timestamp_begin
    seek, out = 0, []
    while seek < max_frames:
        snf = min(Fw, max_frames - seek)
        win = F.pad(feats[:, seek: seek + snf], (0, Fw - snf))
        enc = ref.orc.encode(win)
        ids, marg, _ = ref.decode(enc, gp)
        m = (min(x[0] for x in marg), min(x[1] for x in marg))
        if stop_below is not None and (m[0] < stop_below[0] or m[1] < stop_below[1]):
            return None
        z0 = ref.orc.decoder_pass(ref.orc.new_state(enc), [gp.prompt[0]], 0, True)[0][0]
        ns = no_speech_prob(z0, cfg.no_speech_token_id)
        rec = dict(seek=seek, seek_num_frames=snf, no_speech_prob=ns, margins=m, raw=generated(ids, P, gp.eos_token_id))
        if no_speech_threshold is not None and ns > no_speech_threshold:
            rec.update(ids=[], segments=[], segment_offset=snf, skipped=True)
        else:
            segs, so = hf_retrieve(rec["raw"], P, tb, seek, snf)
            rec.update(ids=rec["raw"], segments=segs, segment_offset=so, skipped=False)
        assert rec["segment_offset"] > 0
        seek += rec["segment_offset"]
        out.append(rec)
    return out


def reference_run(seed=SEED, clips=CLIPS, lengths=LENGTHS, no_speech_threshold=None):
    """The whole batch -> (cfg, sd, gp, wavs, per recording its window records)."""
    cfg, sd = checkpoint(seed)
    gp = gen_params(cfg, sd)
    ref = Ref(cfg, sd)
    wavs = [recording(c, n, g) for (c, g), n in zip(clips, lengths)]
    feats, frames = oracle_features(cfg, wavs)
    return cfg, sd, gp, wavs, [reference_recording(ref, cfg, gp, feats[b], frames[b], no_speech_threshold) for b in range(len(wavs))]


def sequence_of(gp, windows):
    """prompt once, the tokens of every kept segment in order, one EOS."""
    ids = list(gp.prompt)
    for w in windows:
        for sg in w["segments"]:
            ids += sg["tokens"].tolist()
    return ids + [gp.eos_token_id]


def conditions(cfg, windows_per_recording):
    """The three conditions the recordings were chosen under -> dict of figures."""
    Fw = cfg.n_mel_frames
    ws = [w for rec in windows_per_recording for w in rec]
    inside = sum(1 for w in ws if not w["skipped"] and w["segment_offset"] < w["seek_num_frames"])
    full = sum(1 for w in ws if w["segment_offset"] == w["seek_num_frames"] == Fw)
    # an unfinished tail dropped (ids behind the last kept segment) that the next window of the same recording decodes again
    tails = 0
    for rec in windows_per_recording:
        for w, nxt in zip(rec, rec[1:]):
            kept = sum(int(sg["tokens"].numel()) for sg in w["segments"])
            if not w["skipped"] and kept < len(w["ids"]) and nxt["seek"] == w["seek"] + w["segment_offset"] and len(nxt["ids"]) > 0:
                tails += 1
    return dict(min_logit=min(w["margins"][0] for w in ws), min_rel=min(w["margins"][1] for w in ws), inside=inside, full=full, tails=tails,
                windows=[len(r) for r in windows_per_recording])


NS_LOG_GAP = 2 * 0.12      # twice the bound tests/test_gpu_scores.py holds |log no_speech_prob - log reference| to


def skip_threshold(windows_per_recording):
    """A no_speech_threshold that skips exactly one window: the geometric mean of the two largest no-speech probabilities of the reference.
    Returns (threshold, largest, second largest)."""
    ps = sorted((w["no_speech_prob"] for rec in windows_per_recording for w in rec), reverse=True)
    return float(np.sqrt(ps[0] * ps[1])), ps[0], ps[1]


if __name__ == "__main__" and "--search" in sys.argv:
    # `--search SEED [MAX_NEW]`: random clips and half-window gains per recording length; prints every recording all of whose windows clear
    # MARGIN x the tie tolerances under checkpoint SEED, with its seeks and no-speech probabilities.  CLIPS were picked from this output:
    # one recording with both seek branches and a re-decoded tail, one whose only window has a no-speech probability NS_LOG_GAP above the rest.
    import random
    a = sys.argv[sys.argv.index("--search") + 1:]
    seed, max_new = int(a[0]) if a else SEED, int(a[1]) if len(a) > 1 else MAX_NEW
    cfg, sd = checkpoint(seed)
    gp, ref = gen_params(cfg, sd, max_new), Ref(cfg, sd)
    n_pad, rng = padded_len(LENGTHS), random.Random(seed * 100 + max_new)
    for trial in range(40):
        for role, n in enumerate(LENGTHS):
            clip = rng.randrange(1000)
            gains = tuple(rng.choice((1.0, 0.1, 0.003, 0.0)) for _ in range(-(-n // (WINDOW // 2))))
            if not any(gains):
                continue
            f = torch.from_numpy(log_mel(recording(clip, n, gains), cfg.num_mel_bins, n_pad))
            rec = reference_recording(ref, cfg, gp, f, n // 160, stop_below=(MARGIN * TIE, MARGIN * TIE_P))
            if rec is not None:
                print(seed, max_new, role, clip, gains, conditions(cfg, [rec]), [(x["seek"], x["segment_offset"]) for x in rec],
                      [round(x["no_speech_prob"], 7) for x in rec], flush=True)
