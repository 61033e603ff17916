"""Sequence bias, bad words and hotwords on the plain decode path, without a GPU (include/wm.h wm_set_sequence_bias): the C-ABI
surface, the lowering, the contract's numpy restatement against transformers' SequenceBiasLogitsProcessor, the hotword expansion, generate()'s
validation and refusals, and — from tests/seq_bias_ref.py alone — the conditions under which the decode cases of tests/test_gpu_seq_bias.py
were chosen."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import seq_bias_ref as B
import sample_ref as S
from helpers import ROOT, MedusaConfig
from whisper_medusa import WhisperMedusaModel, engine, api

NEG = float("-inf")


# ---- surface ---------------------------------------------------------------------------------------------------------------------------------
def test_header_struct_and_exports(built_lib):
    hdr = open(os.path.join(ROOT, "include", "wm.h")).read()
    assert re.search(r"int wm_set_sequence_bias\(wm_ctx\* ctx, const wm_seq_bias_params\* sb", hdr)
    assert re.search(r"int wm_seq_bias_rows\(wm_ctx\* ctx, const wm_seq_bias_params\* sb, int R,", hdr)
    assert "#define WM_SEQ_BIAS_MAX 1024" in hdr and "#define WM_SEQ_BIAS_MAX_LEN 16" in hdr and "#define WM_ABI_VERSION 9" in hdr
    assert "SequenceBiasLogitsProcessor" in hdr and "NoBadWordsLogitsProcessor" in hdr
    body = re.search(r"typedef struct wm_seq_bias_params \{(.*?)\} wm_seq_bias_params;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [re.sub(r"[\*\s]", "", d.strip().split()[-1]) for d in body.split(";") if d.strip()]
    assert names == [f[0] for f in engine.WmSeqBiasParams._fields_] == ["tokens", "lens", "bias", "n"]
    assert (engine.SEQ_BIAS_MAX, engine.SEQ_BIAS_MAX_LEN) == (1024, 16) == (B.MAX_ENTRIES, B.MAX_LEN)
    assert "wm_set_sequence_bias" in engine.EXPORTS and "wm_seq_bias_rows" in engine.EXPORTS
    for path in (built_lib, engine.LIB_PATH_F16):
        lib = ctypes.CDLL(path)
        assert hasattr(lib, "wm_set_sequence_bias") and hasattr(lib, "wm_seq_bias_rows") and lib.wm_abi_version() == 9
    assert engine.WM_ABI_VERSION == 9


# ---- lowering --------------------------------------------------------------------------------------------------------------------------------
def test_grouped_table_of_a_crafted_set():
    V = 516
    ents = [((7, 30), 1.0), ((8, 7, 30), 2.0),             # two on one target ...
            ((8, 7, 31), 2.0), ((7, 31), 1.0),             # ... and in the other order
            ((5, 40), 0.5), ((40,), -1.0), ((6, 5, 40), NEG),      # a one-token entry given between longer ones
            ((0,), 3.0), ((9, V - 1), -2.0), ((V - 1,), 0.25), ((9, 0), 1.0)]
    want = [(30, [((7, 30), 1.0), ((8, 7, 30), 2.0)]),
            (31, [((8, 7, 31), 2.0), ((7, 31), 1.0)]),
            (40, [((40,), -1.0), ((5, 40), 0.5), ((6, 5, 40), NEG)]),
            (0, [((0,), 3.0), ((9, 0), 1.0)]),
            (V - 1, [((V - 1,), 0.25), ((9, V - 1), -2.0)])]
    assert engine.seq_bias_groups(ents) == want == B.groups_of(ents)
    # the struct the library is handed: ids back to back, in the caller's order
    sb, (tok, lens, bias) = engine.Engine._seq_bias_struct(ents)
    assert sb.n == len(ents) and lens.tolist() == [len(i) for i, _ in ents] and tok.tolist() == [t for i, _ in ents for t in i]
    assert bias.tolist()[:2] == [1.0, 2.0] and bias[6] == -np.inf


# ---- the contract's restatement against HF -------------------------------------------------------------------------------------------------------
def test_contract_equals_hf_on_random_rows():
    rng = np.random.default_rng(3)
    V = 97
    for trial in range(20):
        # entries over a small alphabet so that prefixes match often; biases whose sums round differently in different orders
        ents, seen = [], set()
        while len(ents) < 12:
            m = int(rng.integers(1, 5))
            ids = tuple(int(t) for t in rng.integers(0, 6, size=m - 1)) + (int(rng.integers(0, 8)),)
            if ids in seen:
                continue
            seen.add(ids)
            ents.append((ids, [1.0e-3, 1.0, -1.0, 0.3, NEG, 2.5e-4][int(rng.integers(0, 6))]))
        rows = (rng.standard_normal((10, V)) * 3.0).astype(np.float32)
        pre = [[int(t) for t in rng.integers(0, 6, size=int(rng.integers(1, 7)))] for _ in range(10)]
        assert np.array_equal(B.contract_rows(rows, pre, ents), B.hf_rows(rows, pre, ents)), trial


def test_contract_length_edges_and_order():
    V = 64
    x = np.linspace(-2.0, 2.0, V, dtype=np.float32)[None]
    ents = [((1, 2, 3, 9), 1.0)]
    for pre, hit in (([1, 2, 3], False),            # m = len + 1: the leading ids are the whole context — ignored
                     ([0, 1, 2, 3], True),          # m = len: applied
                     ([2, 3], False), ([5, 0, 1, 2, 3], True), ([1, 2, 4], False)):
        got, want = B.contract_rows(x, [pre], ents), B.hf_rows(x, [pre], ents)
        assert np.array_equal(got, want) and (got[0, 9] != x[0, 9]) == hit, pre
    # the order of the caller is the order of the sum
    a = [((4, 9), 1.0e-3), ((3, 4, 9), 1.0), ((2, 3, 4, 9), -1.0)]
    x = x.copy(); x[0, 9] = 0.0                      # (so that the sum itself is what comes back)
    pre = [2, 3, 4]                                  # m = 4 = len + 1 is ignored; pad it
    pre = [0] + pre
    r1, r2 = B.contract_rows(x, [pre], a), B.contract_rows(x, [pre], a[::-1])
    assert np.array_equal(r1, B.hf_rows(x, [pre], a)) and np.array_equal(r2, B.hf_rows(x, [pre], a[::-1]))
    assert r1[0, 9] != r2[0, 9]                      # (1e-3 + 1) - 1 != (-1 + 1) + 1e-3 in fp32


@pytest.mark.parametrize("V", B.TAP_V)
def test_tap_cases_restatement_equals_hf(V):
    ents = B.tap_entries(V)
    assert len({i for i, _ in ents}) == len(ents) and {len(i) for i, _ in ents} >= {1, 2, 15, 16}
    R = 33
    rows, pre = B.tap_rows(V, R), B.tap_prefixes(V, R)
    want = B.hf_rows(rows, pre, ents)
    assert np.array_equal(B.contract_rows(rows, pre, ents), want)
    multi = B.tap_entries(V, singles=False)
    want_m = B.hf_rows(rows, pre, multi)
    assert np.array_equal(B.contract_rows(rows, pre, multi), want_m)
    changed = (want_m != rows).any(axis=1)
    assert changed.any() and not changed.all()       # rows with a match and rows that come back unchanged
    big = B.big_table(V)
    assert len(big) == 1024 and len(B.groups_of(big)) > 256
    assert np.array_equal(B.contract_rows(rows[:4], pre[:4], big), B.hf_rows(rows[:4], pre[:4], big))


# ---- hotwords --------------------------------------------------------------------------------------------------------------------------------
def test_hotword_entries_on_a_fake_tokenizer():
    tok = B.FakeTokenizer({"Kadcyla": [11, 12, 13], " Kadcyla": [20, 12, 13], "Ng": [30], " Ng": [31, 30], "ab": [11, 12], " ab": [40]})
    got = api.hotword_entries(["Kadcyla", "Ng", "ab"], 2.5, tok)
    assert got == [((11,), 2.5), ((11, 12), 2.5), ((11, 12, 13), 2.5), ((20,), 2.5), ((20, 12), 2.5), ((20, 12, 13), 2.5),
                   ((30,), 2.5), ((31,), 2.5), ((31, 30), 2.5), ((40,), 2.5)]          # ("ab" adds nothing new but its " ab" spelling)
    for bad in ([], "word", [""], [3]):
        with pytest.raises(ValueError, match="hotwords"):
            api.hotword_entries(bad, 1.0, tok)
    with pytest.raises(ValueError, match="hotword_boost"):
        api.hotword_entries(["Ng"], float("inf"), tok)
    with pytest.raises(ValueError, match="tokenizer"):
        api.hotword_entries(["Ng"], 1.0, None)


# ---- generate(): validation and refusals -------------------------------------------------------------------------------------------------------
class _Eng:
    def __init__(self):
        self.seen, self._B, self.max_batch = [], None, 4

    def encode(self, feats):
        self._B = feats.shape[0]

    def decode(self, gp, B, **kw):
        self.seen.append(gp)
        return [list(gp.prompt) + [7, gp.eos_token_id] for _ in range(B)]

    def beam_result(self, clip, rank):
        return list(self.seen[-1].prompt) + [7, self.seen[-1].eos_token_id], -1.0 - rank

    def stats(self):
        return {}


def _model(cfg=None):
    cfg = cfg or MedusaConfig.micro(K=4)
    m = WhisperMedusaModel(cfg, {})
    m._max_batch = 4
    m._engine = _Eng()
    return cfg, m, torch.zeros(1, cfg.num_mel_bins, cfg.n_mel_frames)


def test_generate_lowers_the_three_arguments():
    cfg, m, feats = _model()
    eos = cfg.eos_token_id
    m.generate(feats, vanilla=True, sequence_bias={(5, 6): 1.5, (9,): -2.0})
    assert m._engine.seen[-1].sequence_bias == [((5, 6), 1.5), ((9,), -2.0)] and m._engine.seen[-1].vanilla
    # the list form: a repeated sequence keeps the last value (HF's dict conversion)
    m.generate(feats, vanilla=True, sequence_bias=[[[5, 6], 1.5], [[9], -2.0], [[5, 6], 0.5]])
    assert m._engine.seen[-1].sequence_bias == [((5, 6), 0.5), ((9,), -2.0)]
    # bad words: -inf entries, [eos] filtered out; a sequence given both ways keeps -inf
    m.generate(feats, vanilla=True, bad_words_ids=[[4, 5], [eos], [8]], sequence_bias={(8,): 3.0, (1, 2): 1.0})
    assert m._engine.seen[-1].sequence_bias == [((8,), NEG), ((1, 2), 1.0), ((4, 5), NEG)]
    # hotwords through a tokenizer argument, with num_beams as well
    tok = B.FakeTokenizer({"Ng": [30], " Ng": [31, 30]})
    m.generate(feats, vanilla=True, hotwords=["Ng"], hotword_boost=1.25, tokenizer=tok, num_beams=2)
    gp = m._engine.seen[-1]
    assert gp.sequence_bias == [((30,), 1.25), ((31,), 1.25), ((31, 30), 1.25)] and gp.num_beams == 2
    # the plain path through sampling_seed with a scalar temperature needs no vanilla=True
    m.generate(feats, sequence_bias={(5,): 1.0}, temperature=0.5, sampling_seed=3)
    assert m._engine.seen[-1].sequence_bias == [((5,), 1.0)] and m._engine.seen[-1].vanilla and m._engine.seen[-1].sampling_temperature == 0.5
    # without the new arguments: today's call, no table on the parameters
    m.generate(feats, vanilla=True)
    assert m._engine.seen[-1].sequence_bias is None
    m.generate(feats)
    assert m._engine.seen[-1].sequence_bias is None and not m._engine.seen[-1].vanilla


def test_generate_without_vanilla_raises_instead_of_ignoring():
    cfg, m, feats = _model()
    for kw in (dict(sequence_bias={(5,): 1.0}), dict(bad_words_ids=[[5]]), dict(hotwords=["Ng"], tokenizer=B.FakeTokenizer({"Ng": [3], " Ng": [4]}))):
        with pytest.raises(NotImplementedError, match=r"vanilla=True") as e:
            m.generate(feats, **kw)
        assert list(kw)[0] in str(e.value)
    assert not m._engine.seen


def test_generate_refuses_by_name():
    import dataclasses
    cfg, m, feats = _model()
    sb = dict(vanilla=True, sequence_bias={(5,): 1.0})

    class Other:                                    # a processor / criterion the engine cannot lower: the host path
        def __call__(self, ids, scores):
            return scores

    cases = [dict(logits_processor=[Other()]), dict(stopping_criteria=[Other()]), dict(streamer=object()), dict(chunk_longform=True),
             dict(sequential_longform=True, return_timestamps=True), dict(return_token_logprobs=True), dict(top_logprobs=2),
             dict(no_speech_threshold=0.6), dict(logprob_threshold=-1.0), dict(compression_ratio_threshold=2.4),
             dict(temperature=(0.0, 0.4), sampling_seed=1), dict(return_token_timestamps=True)]
    for extra in cases:
        with pytest.raises(NotImplementedError, match="sequence_bias"):
            m.generate(feats, **dict(sb, **extra))
    with pytest.raises(NotImplementedError, match="bad_words_ids"):
        m.generate(feats, vanilla=True, bad_words_ids=[[5]], return_token_logprobs=True)
    m.set_micro_batches(2)
    with pytest.raises(NotImplementedError, match="sequence_bias.*micro-batch pool"):
        m.generate(feats, **sb)
    m._micro_batches = None
    tree = dataclasses.replace(cfg, medusa_choices=[1, 2, 1, 1, 1])
    _, mt, _ = _model(tree)
    with pytest.raises(NotImplementedError, match="sequence_bias.*candidate tree"):
        mt.generate(feats, **sb)
    assert not m._engine.seen and not mt._engine.seen
    # too many / too long: the engine's limits, as ValueError
    with pytest.raises(ValueError, match="WM_SEQ_BIAS_MAX"):
        m.generate(feats, vanilla=True, sequence_bias={(t,): 1.0 for t in range(1025)})
    with pytest.raises(ValueError, match="WM_SEQ_BIAS_MAX_LEN"):
        m.generate(feats, vanilla=True, sequence_bias={tuple(range(1, 18)): 1.0})
    m.generate(feats, vanilla=True, sequence_bias={tuple(range(1, 17)): 1.0})           # 16 tokens: fine


def test_generate_validation_is_hfs():
    cfg, m, feats = _model()
    V, eos = cfg.vocab_size, cfg.eos_token_id
    for bad, word in (({}, "non-empty"), ([], "non-empty"), ({5: 1.0}, "tuples as keys"), ({(5, -1): 1.0}, "positive integers"),
                      ({(): 1.0}, "positive integers"), ({(5,): 1}, "floats as values"), ([[[5], 1]], "positive integers and float"),
                      ({(V,): 1.0}, "tokens were being biased"), ({(3, V + 7): -1.0}, "tokens were being biased")):
        with pytest.raises(ValueError, match=word):
            m.generate(feats, vanilla=True, sequence_bias=bad)
        # HF raises the same way
        from transformers.generation.logits_process import SequenceBiasLogitsProcessor
        with pytest.raises(ValueError, match=word):
            SequenceBiasLogitsProcessor(bad)(torch.zeros(1, 2, dtype=torch.long), torch.zeros(1, V))
    for bad, word in (([], "non-empty list"), ([5], "list of lists"), ([[5, -2]], "positive integers"), ([[V]], "tokens were being biased")):
        with pytest.raises(ValueError, match=word):
            m.generate(feats, vanilla=True, bad_words_ids=bad)
    with pytest.raises(ValueError, match="eos"):
        m.generate(feats, vanilla=True, bad_words_ids=[[5, eos]])
    with pytest.raises(ValueError, match="finite or -inf"):
        m.generate(feats, vanilla=True, sequence_bias={(5,): float("inf")})
    with pytest.raises(ValueError, match="hotwords"):
        m.generate(feats, vanilla=True, hotword_boost=2.0)
    # [eos] alone is filtered out (NoBadWordsLogitsProcessor): what is left decides
    m.generate(feats, vanilla=True, bad_words_ids=[[eos], [9]])
    assert m._engine.seen[-1].sequence_bias == [((9,), NEG)]
    # a passed generation_config's bad_words_ids is still only warned about: explicit arguments alone are honoured
    from transformers import GenerationConfig
    with pytest.warns(UserWarning, match="bad_words_ids"):
        m.generate(feats, generation_config=GenerationConfig(max_new_tokens=3, bad_words_ids=[[5]]))
    assert m._engine.seen[-1].sequence_bias is None


# ---- the decode cases of tests/test_gpu_seq_bias.py, from the reference alone ----------------------------------------------------------------------
@pytest.fixture(scope="module")
def dec_ref():
    cfg, sd = B.dec_checkpoint()
    ref = B.BiasRef(cfg, sd)
    encs = {c: S.oracle_encode(ref.orc, cfg, c) for c in set(B.DEC_CLIPS)}
    return cfg, ref, encs


@pytest.mark.parametrize("name", sorted(B.DEC_PICKS))
def test_greedy_cases_differ_everywhere_and_are_decisive(dec_ref, name):
    cfg, ref, encs = dec_ref
    gp = B.dec_gp(cfg, "plain" if name == "plain2" else name)
    ents = B.DEC_ENTRIES[name]
    assert [len(i) for i, _ in ents] == [3, 1, 2] and ents[0][1] > 0 and ents[1][1] == ents[2][1] == NEG
    B.dec_guards(ref, gp, encs, ents)                # every clip (so every stream) differs; every decision clears 10 x TIE
    assert all(B.entries_that_act(ref, gp, encs, ents))
    if name == "plain2":
        assert ents != B.DEC_ENTRIES["plain"]


def test_sampled_case_is_decisive(dec_ref):
    cfg, ref, encs = dec_ref
    gp = B.dec_gp(cfg, "plain")
    ents = B.SAMPLE_ENTRIES
    assert [len(i) for i, _ in ents] == [3, 1] and ents[0][1] > 0 and ents[1][1] == NEG      # a boost and a ban
    B.sample_guards(ref, gp, encs, ents, B.SAMPLE_CASE["T"], B.SAMPLE_CASE["seed"])


@pytest.mark.parametrize("name", sorted(B.BEAM_CASES))
def test_beam_cases_have_no_indecisive_step(name):
    cfg, sd, gp, case, runs, ents = B.beam_reference(name, None, B.BEAM_ENTRIES[name])
    assert case[2] == (4 if name == "n4" else 2) and case[5] == (name == "n2_ts")
    assert sorted(len(i) for i, _ in ents) == [2, 3] and {b for _, b in ents} == {1.5, NEG}
    B.beam_guards(runs)
