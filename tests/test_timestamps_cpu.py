"""Host side of return_timestamps: the segment builder against HF's own _retrieve_segment, the checkpoint rule, the prompt, the ctypes
mirror of wm_timestamp_params and the generation_config field.  No GPU."""
import json
import os
import re

import pytest
import torch

from helpers import MedusaConfig, synth
from whisper_medusa import engine as _engine
from whisper_medusa.timestamps import retrieve_segments, row_segments, generated_ids

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TB = 50364          # large-v2 <|0.00|>


def hf_segments(seq, tb=TB, offset=0.0, frames=3000, prec=0.02):
    from transformers.models.whisper.generation_whisper import WhisperGenerationMixin
    s = torch.tensor(seq, dtype=torch.long)
    segs, _ = WhisperGenerationMixin._retrieve_segment(
        seek_sequence=s, seek_outputs=[None], time_offset=torch.tensor([offset], dtype=torch.float64), timestamp_begin=tb,
        seek_num_frames=torch.tensor([frames]), time_precision=prec, time_precision_features=0.01, input_stride=2, prev_idx=0, idx=0,
        return_token_timestamps=False, decoder_input_ids=torch.zeros(1, 3, dtype=torch.long))
    return segs


def T(x):           # timestamp token of x seconds
    return TB + int(round(x / 0.02))


CASES = {
    "pairs": [T(0), 10, 11, T(1.2), T(1.2), 12, T(2.5), T(2.5), 13, T(3.0)],
    "pairs_unfinished_tail": [T(0), 10, T(1.0), T(1.0), 11, 12],
    "single_ending": [T(0), 10, T(1.0), T(1.0), 11, T(2.0)],
    "lone_timestamp": [T(0.4), 10, 11, 12],
    "lone_zero_timestamp": [T(0), 10, 11],
    "none": [10, 11, 12],
    "only_pair": [T(0), T(0.2)],
    "trailing_pair": [T(0), 10, T(1.0), T(1.0)],
}


@pytest.mark.parametrize("name", list(CASES))
def test_segments_equal_hf(name):
    seq = CASES[name]
    for off in (0.0, 30.0):
        want = hf_segments(seq, offset=off)
        got = retrieve_segments(seq, TB, time_offset=off)
        assert len(got) == len(want), (name, got, want)
        for g, w in zip(got, want):
            assert g["start"].dtype == torch.float64 and g["end"].dtype == torch.float64
            assert torch.allclose(g["start"], torch.as_tensor(w["start"], dtype=torch.float64)), (name, g, w)
            assert torch.allclose(g["end"], torch.as_tensor(w["end"], dtype=torch.float64)), (name, g, w)
            assert g["tokens"].tolist() == w["tokens"].tolist()


def test_row_segments_cut_at_first_eos_and_offset():
    eos = 50257
    row = [50258, 50259, 50359] + CASES["pairs"] + [eos, eos, eos]
    assert generated_ids(row, 3, eos) == CASES["pairs"]
    segs = row_segments(row, 3, eos, TB, 3000, time_offset=30.0)
    assert float(segs[0]["start"]) == pytest.approx(30.0) and float(segs[-1]["end"]) == pytest.approx(33.0)


def test_supports_timestamps_rule():
    assert MedusaConfig.large_v2().supports_timestamps
    assert MedusaConfig.tiny_en().supports_timestamps
    assert not MedusaConfig.micro().supports_timestamps


def test_prompt_drops_notimestamps():
    for cfg in (MedusaConfig.large_v2(), MedusaConfig.tiny_en()):
        on, off = synth.default_prompt(cfg, timestamps=True), synth.default_prompt(cfg)
        assert off[-1] == cfg.no_timestamps_token_id and on == off[:-1] and cfg.no_timestamps_token_id not in on
    assert synth.default_prompt(MedusaConfig.tiny_en(), timestamps=True) == [50257]
    assert synth.default_prompt(MedusaConfig.large_v2(), timestamps=True) == [50258, 50259, 50359]


def test_return_timestamps_still_raises_without_timestamp_block():
    from whisper_medusa import WhisperMedusaModel
    cfg = MedusaConfig.micro()
    m = WhisperMedusaModel(cfg, {})
    with pytest.raises(NotImplementedError, match="return_timestamps"):
        m.generate(torch.zeros(1, 80, cfg.n_mel_frames), return_timestamps=True)


def test_ctypes_mirror_follows_header():
    src = open(os.path.join(ROOT, "include", "wm.h")).read()
    body = re.search(r"typedef struct wm_timestamp_params \{(.*?)\} wm_timestamp_params;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"int32_t\s+(\w+)\s*;", body)
    assert [f for f, _ in _engine.WmTimestampParams._fields_] == fields
    assert all(t is __import__("ctypes").c_int32 for _, t in _engine.WmTimestampParams._fields_)
    for name in ("wm_decode_begin_ts", "wm_select_rows"):
        assert name in _engine.EXPORTS and re.search(rf"\bint {name}\(", src)


def test_max_initial_timestamp_index_roundtrip(tmp_path):
    cfg = MedusaConfig.tiny_en()
    cfg.save_pretrained(str(tmp_path))
    assert MedusaConfig.from_pretrained(str(tmp_path)).max_initial_timestamp_index is None
    with open(tmp_path / "generation_config.json", "w") as f:
        json.dump({"max_initial_timestamp_index": 50, "no_timestamps_token_id": cfg.no_timestamps_token_id}, f)
    assert MedusaConfig.from_pretrained(str(tmp_path)).max_initial_timestamp_index == 50


def test_gen_params_carry_timestamps():
    from whisper_medusa import WhisperMedusaModel
    cfg = MedusaConfig.tiny_en()
    cfg.max_initial_timestamp_index = 50
    m = WhisperMedusaModel(cfg, {})
    gp = m._gen_params(None, None, None, 10, None, None, False, None, None, None, None, None, timestamps=True)
    assert gp.timestamps and gp.prompt == [cfg.decoder_start_token_id] and gp.begin_index == 1
    assert gp.no_timestamps_token_id == cfg.no_timestamps_token_id and gp.max_initial_timestamp_index == 50
    ts = _engine.Engine._ts_struct(gp)
    assert (ts.timestamp_begin, ts.no_timestamps_token_id, ts.max_initial_timestamp_index, ts.begin_index) == (50363, 50362, 50, 1)
    gp0 = m._gen_params(None, None, None, 10, None, None, False, None, None, None, None, None)
    assert not gp0.timestamps and gp0.prompt[-1] == cfg.no_timestamps_token_id
