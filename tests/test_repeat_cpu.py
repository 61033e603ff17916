"""Host side of repetition_penalty / no_repeat_ngram_size (include/wm.h wm_set_repeat_rules): the C-ABI surface, the ctypes
mirror, GenParams, generate()'s argument plumbing and refusals, and the reference helper against a hand-worked case.  No GPU."""
import ctypes
import os
import re
import warnings

import pytest
import torch

from helpers import MedusaConfig, GenParams, synth
from whisper_medusa import WhisperMedusaModel, engine as _engine
import repeat_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_abi_surface():
    hdr = open(os.path.join(ROOT, "include", "wm.h")).read()
    assert "#define WM_ABI_VERSION 9" in hdr and _engine.WM_ABI_VERSION == 9
    assert re.search(r"\bint wm_set_repeat_rules\(wm_ctx\*", hdr)
    body = re.search(r"typedef struct wm_repeat_params \{(.*?)\} wm_repeat_params;", hdr, re.S).group(1)
    fields = re.findall(r"(float|int32_t)\s+(\w+)\s*;", body)
    assert [n for _, n in fields] == [n for n, _ in _engine.WmRepeatParams._fields_]
    assert [t for _, t in _engine.WmRepeatParams._fields_] == [ctypes.c_float, ctypes.c_int32]
    assert "RepetitionPenaltyLogitsProcessor" in hdr and "NoRepeatNGramLogitsProcessor" in hdr        # cites the HF classes it stands in for
    assert "wm_set_repeat_rules" in _engine.EXPORTS
    for path in (_engine.LIB_PATH, _engine.LIB_PATH_F16):
        assert os.path.exists(path), f"{path}: build the engine first"
        lib = ctypes.CDLL(path)
        assert lib.wm_abi_version() == 9 and hasattr(lib, "wm_set_repeat_rules")


def test_gen_params_defaults_are_neutral():
    gp = GenParams(prompt=[1], eos_token_id=2, pad_token_id=2)
    assert gp.repetition_penalty == 1.0 and gp.no_repeat_ngram_size == 0 and not gp.repeat_rules
    assert GenParams(prompt=[1], eos_token_id=2, pad_token_id=2, no_repeat_ngram_size=2).repeat_rules
    assert GenParams(prompt=[1], eos_token_id=2, pad_token_id=2, repetition_penalty=0.8).repeat_rules


class _Lib:
    def __init__(self):
        self.calls = []

    def wm_set_repeat_rules(self, h, rp):
        self.calls.append(None if rp is None else (round(rp._obj.repetition_penalty, 6), rp._obj.no_repeat_ngram_size))
        return 0


def test_engine_sets_and_clears_the_rules():
    e = _engine.Engine.__new__(_engine.Engine)
    e.lib, e.h = _Lib(), None
    e._set_repeat_rules(GenParams(prompt=[1], eos_token_id=2, pad_token_id=2, repetition_penalty=1.3, no_repeat_ngram_size=3))
    e._set_repeat_rules(GenParams(prompt=[1], eos_token_id=2, pad_token_id=2))
    assert e.lib.calls == [(1.3, 3), None]          # neutral fields clear what an earlier call left on the context


class _Eng:
    def __init__(self):
        self.seen, self._B = [], None
        self._enc_stamp, self._kv_stamp = object(), object()

    def encode(self, feats):
        self._B = feats.shape[0]

    def decode(self, gp, B, **kw):
        self.seen.append(gp)
        return [list(gp.prompt) + [7, gp.eos_token_id] for _ in range(B)]

    def stats(self):
        return {}


def test_generate_plumbing():
    from transformers import GenerationConfig
    cfg = MedusaConfig.micro(K=4)
    m = WhisperMedusaModel(cfg, {})
    m._engine = eng = _Eng()
    m._max_batch = 2
    x = torch.zeros(1, cfg.num_mel_bins, cfg.n_mel_frames)
    m.generate(x, language="en")
    assert not eng.seen[-1].repeat_rules
    m.generate(x, language="en", repetition_penalty=1.3, no_repeat_ngram_size=3)
    assert (eng.seen[-1].repetition_penalty, eng.seen[-1].no_repeat_ngram_size) == (1.3, 3)
    # both fields are read from a passed config, without the "does not honour" warning; an explicit argument wins
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        m.generate(x, language="en", generation_config=GenerationConfig(max_new_tokens=3, repetition_penalty=1.2, no_repeat_ngram_size=2))
    assert (eng.seen[-1].repetition_penalty, eng.seen[-1].no_repeat_ngram_size) == (1.2, 2)
    m.generate(x, language="en", generation_config=GenerationConfig(max_new_tokens=3, no_repeat_ngram_size=2), no_repeat_ngram_size=4)
    assert eng.seen[-1].no_repeat_ngram_size == 4
    # two windows of a long clip: every window's call carries the rules
    n0 = len(eng.seen)
    m.generate(torch.zeros(1, cfg.num_mel_bins, 2 * cfg.n_mel_frames), language="en", chunk_longform=True, no_repeat_ngram_size=2)
    assert len(eng.seen) > n0 and all(g.no_repeat_ngram_size == 2 for g in eng.seen[n0:])
    for bad in (dict(repetition_penalty=0.0), dict(repetition_penalty=-2.0), dict(no_repeat_ngram_size=-1)):
        with pytest.raises(ValueError):
            m.generate(x, language="en", **bad)


def test_generate_refusals():
    class Odd:
        def __call__(self, ids, scores):
            return scores
    m = WhisperMedusaModel(MedusaConfig.micro(K=4), {})
    x = torch.zeros(1, 80, 192)
    with pytest.raises(NotImplementedError, match="host processor path"):
        m.generate(x, no_repeat_ngram_size=2, logits_processor=[Odd()])
    tree = WhisperMedusaModel(MedusaConfig.micro(K=4, medusa_choices=[1, 2, 2, 1, 1]), {})
    with pytest.raises(NotImplementedError, match="candidate tree"):
        tree.generate(x, repetition_penalty=1.3)
    # neutral values are no request
    with pytest.raises(RuntimeError, match="HIP device"):
        tree.generate(x, language="en", repetition_penalty=1.0, no_repeat_ngram_size=0)


def test_reference_helper_on_a_hand_worked_row():
    """tests/repeat_ref.py calls HF's processors as the contract orders them: penalty on the raw logit, then the n-gram ban."""
    gp = GenParams(prompt=[1], eos_token_id=9, pad_token_id=9, repetition_penalty=2.0, no_repeat_ngram_size=2)
    z = torch.tensor([4.0, -4.0, 2.0, -2.0, 1.0, 0.5, 0.0, 0.0, 0.0, 0.0])
    out = R.hf_row(z, [0, 1, 2, 0], gp)                 # the bigram (0, 1) occurred: 1 is banned; 0, 1, 2 are penalised
    assert out.tolist()[:5] == [2.0, -float("inf"), 1.0, -2.0, 1.0]
    assert R.repeated_ngrams([1, 2, 3, 1, 2], 2) == 1 and R.repeated_ngrams([1, 2, 3], 2) == 0
