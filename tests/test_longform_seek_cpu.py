"""Sequential long-form decoding (generate(sequential_longform=True)) without a GPU: the segment / seek rule against transformers'
own `WhisperGenerationMixin._retrieve_segment`, the public surface and its refusals, the oracle's whole-recording log-mel against
`WhisperFeatureExtractor(truncation=False)`, the loop against a scripted engine, and the conditions the recordings of the GPU test
(tests/longform_seek.py) were chosen under."""
import math
import os
import re

import numpy as np
import pytest
import torch

import longform_seek as LS
from helpers import ROOT, synth
from oracle.whisper_medusa_oracle import log_mel
from whisper_medusa import WhisperMedusaModel, MedusaConfig
from whisper_medusa import engine as wm_engine
from whisper_medusa.timestamps import retrieve_segments, retrieve_segments_and_offset, sequential_seek_loop, assemble_sequence

CFG = LS.micro_ts()
TB, FW = CFG.timestamp_begin, CFG.n_mel_frames          # 934, 192


def ts(i):
    return TB + i


# ---- the rule, against HF ------------------------------------------------------------------------------------------------------------------
ROWS = {
    "pairs, unfinished tail": ([ts(0), 10, 11, ts(40), ts(40), 12, 13, ts(61), ts(61), 14, 15], FW),
    "pairs, tail ends in a timestamp run": ([ts(0), 10, ts(30), ts(31), 12, ts(50), ts(50)], FW),
    "pairs, single-timestamp ending": ([ts(2), 10, ts(40), ts(40), 12, 13, ts(70)], FW),
    "no pair, last timestamp": ([ts(0), 10, 11, ts(33)], FW),
    "no pair, last timestamp, text behind it": ([ts(0), 10, ts(33), 11], FW),
    "no pair, only <|0.00|>": ([ts(0), 10, 11, 12], FW),
    "no timestamp at all": ([10, 11, 12], FW),
    "nothing generated": ([], FW),
    "last window, no pair": ([ts(0), 10, 11], 57),
    "last window, odd frame count, no timestamp": ([10, 11], 169),
    "last window, pairs": ([ts(0), 10, ts(20), ts(20), 11], 57),
    "last window, single ending": ([ts(0), 10, ts(20), ts(20), 11, ts(25)], 57),
}


@pytest.mark.parametrize("name", list(ROWS))
@pytest.mark.parametrize("seek", [0, 148, 1234567])
def test_segments_and_offset_are_hfs(name, seek):
    seq, snf = ROWS[name]
    want, want_off = LS.hf_retrieve(seq, 1, TB, seek, snf)
    off = torch.tensor(seek, dtype=torch.float64) * 0.02 / 2
    got, got_off = retrieve_segments_and_offset(seq, TB, 0.02, off, snf, 0.01, 2)
    assert got_off == want_off and isinstance(got_off, int)
    assert len(got) == len(want)
    for g, w in zip(got, want):
        for k in ("start", "end"):
            assert g[k].dtype == torch.float64 and float(g[k]) == float(w[k]), (name, k, g[k], w[k])
        assert g["tokens"].tolist() == w["tokens"].tolist()


def test_offset_branches():
    off = lambda name: retrieve_segments_and_offset(ROWS[name][0], TB, seek_num_frames=ROWS[name][1])[1]      # noqa: E731
    assert off("pairs, unfinished tail") == 61 * 2
    assert off("pairs, single-timestamp ending") == FW
    assert off("no pair, last timestamp") == FW and off("no timestamp at all") == FW
    assert off("last window, no pair") == 57 and off("last window, pairs") == 40 and off("last window, single ending") == 57
    # the no-pair segment's default end is the window's own audio, not the full window
    sg = retrieve_segments_and_offset([10, 11], TB, seek_num_frames=57)[0][0]
    assert float(sg["end"]) == int(57 * 0.01 / 0.02) * 0.02


def test_existing_return_value_is_unchanged():
    seq = ROWS["pairs, unfinished tail"][0]
    a = retrieve_segments(seq, TB, 0.02, 1.5, FW)
    b = retrieve_segments_and_offset(seq, TB, 0.02, 1.5, FW)[0]
    assert isinstance(a, list) and len(a) == len(b) == 2
    assert all(torch.equal(x["start"], y["start"]) and torch.equal(x["end"], y["end"]) and torch.equal(x["tokens"], y["tokens"]) for x, y in zip(a, b))
    assert float(retrieve_segments([10, 11], TB, window_frames=FW)[0]["end"]) == 96 * 0.02


# ---- the surface ---------------------------------------------------------------------------------------------------------------------------
def test_entries_are_declared_and_exported(built_lib):
    hdr = open(os.path.join(ROOT, "include", "wm.h")).read()
    assert re.search(r"#define WM_ABI_VERSION 9\b", hdr) and wm_engine.WM_ABI_VERSION == 9
    for name in ("wm_logmel_long", "wm_gather_windows"):
        assert re.search(r"\bint " + name + r"\s*\(", hdr), name
        assert name in wm_engine.EXPORTS
    for f16 in (False, True):
        lib = wm_engine.load_library(act_fp16=f16)
        assert lib.wm_abi_version() == 9 and lib.wm_logmel_long and lib.wm_gather_windows


def _cpu_model(cfg=None, seed=3):
    cfg = cfg or CFG
    return WhisperMedusaModel(cfg, synth.synth_state_dict(cfg, seed=seed), max_batch=4)


REFUSALS = [
    (dict(condition_on_prev_tokens=True), "condition_on_prev_tokens"),
    (dict(temperature=(0.0, 0.2, 0.4)), "temperature"),
    (dict(return_token_timestamps=True), "return_token_timestamps"),
    (dict(return_timestamps=False), "return_timestamps"),
    (dict(return_timestamps=None), "return_timestamps"),
    (dict(logits_processor=[object()]), "logits_processor"),
    (dict(stopping_criteria=[object()]), "stopping_criteria"),
    (dict(streamer=object()), "streamer"),
    (dict(prompt_ids=torch.tensor([5, 6])), "prompt_condition_type"),
]


@pytest.mark.parametrize("kw,word", REFUSALS, ids=[w + str(i) for i, (_, w) in enumerate(REFUSALS)])
def test_refusals_name_what_they_refuse(kw, word):
    m = _cpu_model()
    x = torch.zeros(1, CFG.num_mel_bins, 3 * FW)
    args = dict(dict(sequential_longform=True, return_timestamps=True), **kw)
    with pytest.raises(NotImplementedError, match=word) as e:
        m.generate(x, **args)
    assert "sequential_longform" in str(e.value)


def test_refusals_of_the_checkpoint():
    x = torch.zeros(1, 80, 400)
    plain = MedusaConfig.micro(K=4)                          # no timestamp block
    assert not plain.supports_timestamps
    with pytest.raises(NotImplementedError, match="timestamp block"):
        _cpu_model(plain).generate(x, sequential_longform=True, return_timestamps=True)
    import dataclasses
    tree = dataclasses.replace(CFG, medusa_choices=[1, 2, 1, 1, 1])
    assert tree.is_tree
    with pytest.raises(NotImplementedError, match="candidate tree"):
        _cpu_model(tree).generate(x, sequential_longform=True, return_timestamps=True)


def test_old_paths_keep_their_refusals():
    m = _cpu_model()
    x = torch.zeros(1, CFG.num_mel_bins, 3 * FW)
    with pytest.raises(NotImplementedError, match="Longform generation is not supported yet"):
        m.generate(x, return_timestamps=True)
    with pytest.raises(RuntimeError, match="not on a HIP device"):      # chunk_longform still goes its own way (to the engine)
        m.generate(x, chunk_longform=True, return_timestamps=True)


# ---- the oracle's whole-recording log-mel is HF's ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [160 * 7, 30720 + 160 * 7, 3 * 30720 + 160])
def test_oracle_log_mel_of_a_whole_recording_is_hfs(n):
    from transformers import WhisperFeatureExtractor
    fe = WhisperFeatureExtractor()
    wav = LS.recording(3, n, (1.0, 0.003, 0.1))
    ref = fe(wav, sampling_rate=16000, truncation=False, padding="longest", return_tensors="np").input_features[0]
    got = log_mel(wav, 80, n)
    assert got.shape == ref.shape == (80, n // 160)
    np.testing.assert_allclose(got, ref, atol=5e-5)          # the figure of tests/test_oracle_golden.py's 30 s check


# ---- the loop against a scripted engine ----------------------------------------------------------------------------------------------------
class ScriptedEngine:
    """Engine stand-in: `gather_windows` notes which (clip, seek, n_valid) the loop asks for, `decode` answers each with its scripted ids
    (a window the script does not know is an error: the seeks are asserted by construction), `score_tokens` with its scripted no-speech
    probability."""

    def __init__(self, cfg, script, no_speech=None):
        self.cfg, self.script, self.no_speech = cfg, script, no_speech or {}
        self.rounds, self._B, self._cur = [], None, None

    def gather_windows(self, feats, clip, seek, n_valid, out=None):
        self._cur = list(zip(clip, seek, n_valid))
        self.rounds.append(self._cur)
        win = torch.zeros(len(clip), feats.shape[1], self.cfg.n_mel_frames)
        for w, (c, s, n) in enumerate(self._cur):
            assert 0 <= s and s + n <= feats.shape[-1] and 0 < n <= self.cfg.n_mel_frames
            win[w, :, :n] = feats[c, :, s: s + n]
        return win

    def encode(self, feats):
        assert feats.shape[0] == len(self._cur)
        self._B = feats.shape[0]

    def decode(self, gp, B):
        assert gp.timestamps and B == len(self._cur)
        return [list(gp.prompt) + list(self.script[(c, s)]) + [gp.eos_token_id] for c, s, _ in self._cur]

    def stats(self):
        return dict(iterations=0)

    def score_tokens(self, seqs, n_prompt, gp, ns_id, sot_index):
        T = max(len(s) for s in seqs)
        nsp = np.array([self.no_speech.get((c, s), 0.0) for c, s, _ in self._cur], dtype=np.float32)
        return np.full((len(seqs), T), -0.5, dtype=np.float32), nsp, 0.0


FRAMES = (441, 192, 77)                                     # 2.3, 1.0 and 0.4 windows
SCRIPT = {
    (0, 0): [ts(0), 10, 11, ts(40), ts(40), 12, 13],        # a pair, then an unfinished tail: seek to 80, the tail is decoded again
    (0, 80): [ts(0), 12, 13, ts(50)],                       # single closing timestamp: the whole window
    (0, 272): [20, 21],                                     # last window (169 frames), no timestamp
    (1, 0): [ts(0), 30, ts(96), ts(96)],                    # the pair sits at the window's end
    (2, 0): [ts(0), 31, ts(10), ts(10), 32],                # 77 frames: seek to 20
    (2, 20): [ts(0), 33, ts(20)],                           # 57 frames, single ending
}
SEEKS = {0: [(0, 192, 80), (80, 192, 192), (272, 169, 169)], 1: [(0, 192, 192)], 2: [(0, 77, 20), (20, 57, 57)]}


def _scripted_model(no_speech=None):
    m = _cpu_model()
    m._engine = ScriptedEngine(CFG, SCRIPT, no_speech)
    return m


def _features():
    return torch.arange(3 * CFG.num_mel_bins * 441, dtype=torch.float32).reshape(3, CFG.num_mel_bins, 441)


def test_loop_on_a_scripted_engine():
    m = _scripted_model()
    out = m.generate(_features(), sequential_longform=True, return_timestamps=True, return_segments=True, num_frames=torch.tensor(FRAMES))
    P, eos = [CFG.decoder_start_token_id], CFG.eos_token_id
    assert m.last_stats["longform_windows"] == [3, 1, 2]
    # rounds: all three clips, then clips 0 and 2, then clip 0 alone, each at HF's seek with HF's seek_num_frames
    assert m._engine.rounds == [[(0, 0, 192), (1, 0, 192), (2, 0, 77)], [(0, 80, 192), (2, 20, 57)], [(0, 272, 169)]]
    want_ids, want_segs = [], []
    for b in range(3):
        ids, segs = list(P), []
        for seek, snf, off in SEEKS[b]:
            s_, o_ = LS.hf_retrieve(SCRIPT[(b, seek)], 1, TB, seek, snf)
            assert o_ == off
            segs += s_
            for sg in s_:
                ids += sg["tokens"].tolist()
        want_ids.append(ids + [eos])
        want_segs.append(segs)
    T = max(len(s) for s in want_ids)
    assert out["sequences"].shape == (3, T)
    for b in range(3):
        assert out["sequences"][b].tolist() == want_ids[b] + [CFG.pad_token_id] * (T - len(want_ids[b]))
        assert len(out["segments"][b]) == len(want_segs[b])
        for g, w in zip(out["segments"][b], want_segs[b]):
            assert g["start"].dtype == torch.float64 and float(g["start"]) == float(w["start"]) and float(g["end"]) == float(w["end"])
            assert g["tokens"].tolist() == w["tokens"].tolist()
    # clip 0 in numbers: the dropped tail [12, 13] comes back with the second window; times are absolute
    assert want_ids[0] == P + [ts(0), 10, 11, ts(40), ts(40)] + [ts(0), 12, 13, ts(50)] + [20, 21] + [eos]
    s0 = out["segments"][0]
    assert [(float(g["start"]), float(g["end"])) for g in s0] == [(0.0, 40 * 0.02), (0.8, 0.8 + 50 * 0.02), (2.72, 2.72 + 84 * 0.02)]
    # attention_mask gives the same lengths, HF's way; the default length is the whole tensor
    mask = torch.zeros(3, 441, dtype=torch.long)
    for b, n in enumerate(FRAMES):
        mask[b, :n] = 1
    m2 = _scripted_model()
    again = m2.generate(_features(), sequential_longform=True, return_timestamps=True, attention_mask=mask)
    assert torch.equal(again, out["sequences"]) and m2._engine.rounds == m._engine.rounds
    m3 = _scripted_model()
    m3._engine.script = {(0, 0): [ts(0), 9, ts(96), ts(96)], (0, 192): [9]}
    m3.generate(_features()[:1, :, :200], sequential_longform=True, return_timestamps=True)
    assert m3._engine.rounds == [[(0, 0, 192)], [(0, 192, 8)]] and m3.last_stats["longform_windows"] == [2]


def test_loop_skips_a_window_the_gate_rejects():
    m = _scripted_model(no_speech={(0, 80): 0.9, (2, 0): 0.4})
    out = m.generate(_features(), sequential_longform=True, return_timestamps=True, return_segments=True, num_frames=list(FRAMES),
                     no_speech_threshold=0.5)
    assert m.last_stats["longform_windows"] == [3, 1, 2]
    # the skipped window advances by its seek_num_frames and gives neither ids nor segments
    assert [r for rnd in m._engine.rounds for r in rnd if r[0] == 0] == [(0, 0, 192), (0, 80, 192), (0, 272, 169)]
    assert out["skipped"][0].tolist() == [False, True, False] and out["skipped"][2].tolist() == [False, False]
    assert out["no_speech_prob"][0].tolist() == pytest.approx([0.0, 0.9, 0.0])
    P, eos = [CFG.decoder_start_token_id], CFG.eos_token_id
    assert out["sequences"][0].tolist()[: 1 + 5 + 2 + 1] == P + [ts(0), 10, 11, ts(40), ts(40)] + [20, 21] + [eos]
    assert [(float(g["start"]), float(g["end"])) for g in out["segments"][0]] == [(0.0, 0.8), (2.72, 2.72 + 84 * 0.02)]
    assert int(out["lengths"][0]) == 9 and float(out["token_logprobs"][0, 1]) == -0.5


def test_loop_refuses_to_stand_still():
    def stuck(clips, seeks, snf):
        return [dict(ids=[ts(0), ts(0), 10], skipped=False, result=None) for _ in clips]      # a pair at <|0.00|>: HF's rules cannot emit it
    with pytest.raises(RuntimeError, match="would not advance"):
        sequential_seek_loop([300], FW, stuck, TB)
    assert sequential_seek_loop([0, 0], FW, stuck, TB) == [[], []]
    assert assemble_sequence([1, 2], [], 9) == [1, 2, 9]


# ---- the recordings of the GPU test ----------------------------------------------------------------------------------------------------------
def test_recordings_meet_the_conditions_they_were_chosen_under():
    """Figures of the reference alone (oracle sim="bf16" on its own log-mel and encoder output; seed 24, max_new_tokens 12): 8 windows
    ([3, 1, 4]); smallest logit margin 5.46e-3 (>= 10 x 5e-4), smallest relative p_c margin 5.3e-2 (>= 10 x 2e-3); one seek strictly inside
    a window (192 -> 340 of the third recording, whose dropped tail the window at 340 decodes again), four full-window advances; the two
    largest no-speech probabilities 1.20e-4 (the second recording's only window) and 8.75e-5: log ratio 0.32 >= 0.24."""
    cfg, sd, gp, wavs, recs = LS.reference_run()
    c = LS.conditions(cfg, recs)
    print("reference:", c)
    assert c["min_logit"] >= LS.MARGIN * LS.TIE and c["min_rel"] >= LS.MARGIN * LS.TIE_P
    assert c["inside"] >= 1 and c["full"] >= 1 and c["tails"] >= 1
    assert [round(len(w) / LS.WINDOW, 1) for w in wavs] == [2.3, 1.0, 3.6]
    thr, p0, p1 = LS.skip_threshold(recs)
    print("no-speech:", thr, p0, p1, math.log(p0 / p1))
    assert math.log(p0 / p1) >= LS.NS_LOG_GAP
    # the skipped window is one whose advance was the whole window already: the other windows stay the ones the margins were checked on
    hit = [(b, w) for b, rec in enumerate(recs) for w in rec if w["no_speech_prob"] > thr]
    assert len(hit) == 1 and hit[0][1]["segment_offset"] == hit[0][1]["seek_num_frames"]
