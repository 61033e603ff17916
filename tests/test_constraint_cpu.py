"""Constrained decoding on the plain decode path, without a GPU (include/wm.h wm_set_constraint): the C-ABI surface, the
reference's A(g) against a brute-force scan and against transformers' PrefixConstrainedLogitsProcessor, the two argument lowerings, generate()'s
validation and refusals, and — from tests/constraint_ref.py alone — the conditions under which the decode cases of tests/test_gpu_constraint.py
were chosen."""
import ctypes
import dataclasses
import os
import re

import numpy as np
import pytest
import torch

import constraint_ref as C
import seq_bias_ref as B
import sample_ref as S
from helpers import ROOT, MedusaConfig
from whisper_medusa import WhisperMedusaModel, engine, api


# ---- surface ---------------------------------------------------------------------------------------------------------------------------------
def test_header_struct_and_exports(built_lib):
    hdr = open(os.path.join(ROOT, "include", "wm.h")).read()
    assert re.search(r"int wm_set_constraint\(wm_ctx\* ctx, const wm_constraint_params\* c", hdr)
    assert re.search(r"int wm_constraint_rows\(wm_ctx\* ctx, const wm_constraint_params\* c, int eos, int prompt_len, int R,", hdr)
    assert re.search(r"#define WM_CONSTRAINT_MAX\s+16384\b", hdr) and re.search(r"#define WM_CONSTRAINT_MAX_LEN\s+32\b", hdr)
    assert "#define WM_ABI_VERSION 9" in hdr and "PrefixConstrainedLogitsProcessor" in hdr
    body = re.search(r"typedef struct wm_constraint_params \{(.*?)\} wm_constraint_params;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [re.sub(r"[\*\s]", "", d.strip().split()[-1]) for d in body.split(";") if d.strip()]
    assert names == [f[0] for f in engine.WmConstraintParams._fields_] == ["tokens", "lens", "n"]
    assert (engine.CONSTRAINT_MAX, engine.CONSTRAINT_MAX_LEN) == (16384, 32) == (C.MAX_SEQS, C.MAX_LEN)
    assert "wm_set_constraint" in engine.EXPORTS and "wm_constraint_rows" in engine.EXPORTS
    for path in (built_lib, engine.LIB_PATH_F16):
        lib = ctypes.CDLL(path)
        assert hasattr(lib, "wm_set_constraint") and hasattr(lib, "wm_constraint_rows") and lib.wm_abi_version() == 9
    assert engine.WM_ABI_VERSION == 9
    # the struct the library is handed: ids back to back, in the caller's order
    c, (tok, lens) = engine.Engine._constraint_struct([(5, 6), (9,), (1, 2, 3)])
    assert c.n == 3 and lens.tolist() == [2, 1, 3] and tok.tolist() == [5, 6, 9, 1, 2, 3]


# ---- A(g) ------------------------------------------------------------------------------------------------------------------------------------
def test_allowed_equals_a_brute_force_scan():
    rng = np.random.default_rng(5)
    eos, total = 99, 0
    for trial in range(20):
        seqs = list({tuple(int(t) for t in rng.integers(0, 7, size=int(rng.integers(1, 6)))) for _ in range(int(rng.integers(1, 40)))})
        probes = [[]] + [list(s[:k]) for s in seqs for k in range(1, len(s) + 1)] + [list(s) + [3] for s in seqs] + [list(s) + [eos] for s in seqs]
        probes += [[int(t) for t in rng.integers(0, 7, size=int(rng.integers(1, 8)))] for _ in range(30)]
        for g in probes:
            a = C.allowed(seqs, eos, g)
            assert a == C.allowed_scan(seqs, eos, g) and a, (trial, g)
            total += a == {eos} and not any(list(s[: len(g)]) == g for s in seqs)
    assert total > 100                               # the total-function case: the prefix has left the trie
    # a sequence that is a prefix of another gives both; a whole sequence gives eos alone
    assert C.allowed([(1, 2), (1, 2, 3)], eos, [1, 2]) == {eos, 3} and C.allowed([(1, 2), (1, 2, 3)], eos, [1, 2, 3]) == {eos}
    assert C.allowed([(1, 2), (4,)], eos, []) == {1, 4}


@pytest.mark.parametrize("V", C.TAP_V)
def test_hf_rows_on_the_tap_inputs(V):
    eos, table = C.tap_eos(V), C.tap_table(V)
    assert len(set(table)) == len(table) and max(map(len, table)) == C.MAX_LEN and all(eos not in s for s in table)
    assert {0, V - 1, C.slice_span(V) - 1, C.slice_span(V)} <= {t for s in table for t in s}
    for P in C.TAP_P:
        R = 33
        rows, pre = C.tap_rows(V, R), C.tap_prefixes(V, R, P)
        want, n = C.contract_rows(rows, pre, table, eos, P)
        assert np.array_equal(C.hf_rows(rows, pre, table, eos, P), want)
        sizes = {tuple(p[P:]): int(k) for p, k in zip(pre, n)}
        assert sizes[()] == len({s[0] for s in table}) and sizes[(10, 11)] == 2 and sizes[(10, 11, 12)] == 1 and sizes[(10,)] == 2
        assert sizes[(6,)] == sizes[(20, 22)] == sizes[tuple(C.LONG[:-1]) + (7,)] == sizes[tuple(C.LONG) + (1, 2, 3)] == 1
        assert sizes[tuple(C.LONG[:-1])] == 2 and sizes[tuple(C.LONG)] == 1
        assert max(len(p) - P for p in pre) > C.MAX_LEN + 1 and min(len(p) - P for p in pre) == 0
        assert np.isinf(want[0, 5]) and (np.isfinite(want).sum(axis=1) <= n).all()
    big = C.big_table(V)
    assert len(big) == C.MAX_SEQS == len(set(big))
    rows, pre = C.tap_rows(V, 6), C.big_prefixes(big, 6, 4)
    want, n = C.contract_rows(rows, pre, big, eos, 4)
    assert np.array_equal(C.hf_rows(rows, pre, big, eos, 4), want) and n[0] == 5 and 1 in n.tolist()


# ---- the two lowerings -----------------------------------------------------------------------------------------------------------------------
def test_allowed_sequence_and_phrase_entries():
    V, eos = 516, 500
    assert api.allowed_sequence_entries([[5, 6], (9,), [5, 6], [np.int64(7), 8]], eos, V) == [(5, 6), (9,), (7, 8)]
    for bad, word in (([], "non-empty list"), ("ab", "non-empty list"), (None, "non-empty list"), ([5], "non-empty list of non-negative"),
                      ([[]], "non-empty list of non-negative"), ([[5, -1]], "non-negative"), ([[5.0]], "non-negative"), ([[True]], "non-negative"),
                      ([[V]], "vocabulary size"), ([[5, eos]], "eos_token_id"), ([[eos]], "eos_token_id")):
        with pytest.raises(ValueError, match=word):
            api.allowed_sequence_entries(bad, eos, V)
    tok = B.FakeTokenizer({"yes": [11], " yes": [20, 11], "no way": [30, 31], " no way": [32, 31], "ja": [11], " ja": [40], "": [], " ": [], "x": [], " x": [41]})
    assert api.allowed_phrase_entries(["yes", "no way", "ja"], tok) == [(11,), (20, 11), (30, 31), (32, 31), (40,)]
    for bad in ([], "yes", [""], [3]):
        with pytest.raises(ValueError, match="allowed_phrases"):
            api.allowed_phrase_entries(bad, tok)
    with pytest.raises(ValueError, match="tokenizer"):
        api.allowed_phrase_entries(["yes"], None)
    with pytest.raises(ValueError, match="encodes to no token"):
        api.allowed_phrase_entries(["x"], tok)


# ---- generate(): lowering, validation and refusals ---------------------------------------------------------------------------------------------
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


def test_generate_lowers_the_two_arguments():
    cfg, m, feats = _model()
    m.generate(feats, vanilla=True, allowed_sequences=[[25, 26], [29], [25, 26]])
    assert m._engine.seen[-1].allowed_sequences == [(25, 26), (29,)] and m._engine.seen[-1].vanilla
    tok = B.FakeTokenizer({"Ng": [30], " Ng": [31, 30]})
    m.generate(feats, vanilla=True, allowed_phrases=["Ng"], tokenizer=tok)
    assert m._engine.seen[-1].allowed_sequences == [(30,), (31, 30)]
    # both: merged in that order; with beams, the bias, the repetition rules and one language per clip
    m.generate(torch.cat([feats, feats]), vanilla=True, allowed_sequences=[[31, 30], [29]], allowed_phrases=["Ng"], tokenizer=tok, num_beams=2,
               num_return_sequences=2, sequence_bias={(29,): 1.5}, repetition_penalty=1.2, language=["en", "de"] if cfg.is_multilingual else None)
    gp = m._engine.seen[-1]
    assert gp.allowed_sequences == [(31, 30), (29,), (30,)] and gp.num_beams == 2 and gp.sequence_bias == [((29,), 1.5)] and gp.repetition_penalty == 1.2
    # the plain path through sampling_seed with a scalar temperature needs no vanilla=True; the filters ride along
    m.generate(feats, allowed_sequences=[[25]], temperature=0.5, sampling_seed=3, sampling_top_k=2)
    gp = m._engine.seen[-1]
    assert gp.allowed_sequences == [(25,)] and gp.vanilla and gp.sampling_temperature == 0.5 and gp.sampling_top_k == 2
    m.generate(feats, vanilla=True, allowed_sequences=[[25]], prompt_ids=torch.tensor([cfg.prev_sot_token_id, 40, 41]))
    assert m._engine.seen[-1].allowed_sequences == [(25,)] and len(m._engine.seen[-1].prompt) > 3
    # without the new arguments: today's call, no table on the parameters
    m.generate(feats, vanilla=True)
    assert m._engine.seen[-1].allowed_sequences is None
    m.generate(feats)
    assert m._engine.seen[-1].allowed_sequences is None and not m._engine.seen[-1].vanilla


def test_generate_without_vanilla_raises_instead_of_ignoring():
    cfg, m, feats = _model()
    for kw in (dict(allowed_sequences=[[25]]), dict(allowed_phrases=["Ng"], tokenizer=B.FakeTokenizer({"Ng": [23], " Ng": [24]}))):
        with pytest.raises(NotImplementedError, match=r"vanilla=True") as e:
            m.generate(feats, **kw)
        assert list(kw)[0] in str(e.value)
    assert not m._engine.seen


def test_generate_refuses_by_name():
    cfg, m, feats = _model()
    al = dict(vanilla=True, allowed_sequences=[[25, 26]])

    class Other:                                    # a processor / criterion the engine cannot lower: the host path
        def __call__(self, ids, scores):
            return scores

    cases = [dict(logits_processor=[Other()]), dict(stopping_criteria=[Other()]), dict(streamer=object()), dict(chunk_longform=True),
             dict(return_token_logprobs=True), dict(top_logprobs=2), dict(no_speech_threshold=0.6), dict(logprob_threshold=-1.0),
             dict(compression_ratio_threshold=2.4), dict(temperature=(0.0, 0.4), sampling_seed=1), dict(return_token_timestamps=True)]
    for extra in cases:
        with pytest.raises(NotImplementedError, match="allowed_sequences"):
            m.generate(feats, **dict(al, **extra))
    with pytest.raises(NotImplementedError, match="allowed_phrases"):
        m.generate(feats, vanilla=True, allowed_phrases=["Ng"], tokenizer=B.FakeTokenizer({"Ng": [23], " Ng": [24]}), return_token_logprobs=True)
    m.set_micro_batches(2)
    with pytest.raises(NotImplementedError, match="allowed_sequences.*micro-batch pool"):
        m.generate(feats, **al)
    m._micro_batches = None
    tree = dataclasses.replace(cfg, medusa_choices=[1, 2, 1, 1, 1])
    _, mt, _ = _model(tree)
    with pytest.raises(NotImplementedError, match="allowed_sequences.*candidate tree"):
        mt.generate(feats, **al)
    # timestamps, on a checkpoint whose vocabulary has them
    tcfg, mts, tfeats = _model(S._sr.micro_ts("base_head"))
    for extra in (dict(return_timestamps=True), dict(return_timestamps=True, sequential_longform=True)):
        with pytest.raises(NotImplementedError, match="allowed_sequences"):
            mts.generate(tfeats, **dict(al, **extra))
    with pytest.raises(NotImplementedError, match="allowed_sequences"):
        m.generate(feats, prefix_allowed_tokens_fn=lambda b, s: [1])       # HF's hook stays refused; the message names what replaces it
    assert not m._engine.seen and not mt._engine.seen and not mts._engine.seen
    # too many / too long: the engine's limits, as ValueError
    with pytest.raises(ValueError, match="WM_CONSTRAINT_MAX_LEN"):
        m.generate(feats, vanilla=True, allowed_sequences=[list(range(20, 53))])
    m.generate(feats, vanilla=True, allowed_sequences=[list(range(20, 52))])               # 32 tokens: fine
    V = cfg.vocab_size
    many = [[a, b] for a in range(20, 150) for b in range(20, 150)][: C.MAX_SEQS + 1]
    if all(t < V and t != cfg.eos_token_id for q in many for t in q):
        with pytest.raises(ValueError, match=r"WM_CONSTRAINT_MAX\)"):
            m.generate(feats, vanilla=True, allowed_sequences=many)


def test_generate_validation():
    cfg, m, feats = _model()
    V, eos = cfg.vocab_size, cfg.eos_token_id
    for bad, word in (([], "non-empty list"), ([5], "non-negative"), ([[5, -2]], "non-negative"), ([[V]], "vocabulary size"), ([[21, eos]], "eos_token_id")):
        with pytest.raises(ValueError, match=word):
            m.generate(feats, vanilla=True, allowed_sequences=bad)
    with pytest.raises(ValueError, match="suppress_tokens"):
        m.generate(feats, vanilla=True, allowed_sequences=[[21, 22]], suppress_tokens=[22])
    with pytest.raises(ValueError, match="begin_suppress_tokens"):
        m.generate(feats, vanilla=True, allowed_sequences=[[21, 22]], begin_suppress_tokens=[21])
    m.generate(feats, vanilla=True, allowed_sequences=[[21, 22]], begin_suppress_tokens=[22], suppress_tokens=[23])     # (22 is no first id)
    with pytest.raises(ValueError, match="exponential decay"):
        m.generate(feats, vanilla=True, allowed_sequences=[[21, 22]], exponential_decay_length_penalty=(4, 1.1))
    from transformers import GenerationConfig
    with pytest.raises(ValueError, match="exponential decay"):     # a generation config that turns the decay on
        m.generate(feats, vanilla=True, allowed_sequences=[[21, 22]], generation_config=GenerationConfig(exponential_decay_length_penalty=(4, 1.1)))


# ---- the decode cases of tests/test_gpu_constraint.py, from the reference alone --------------------------------------------------------------------
@pytest.fixture(scope="module")
def dec_ref():
    cfg, sd = C.dec_checkpoint()
    ref = C.ConsRef(cfg, sd)
    encs = {c: S.oracle_encode(ref.orc, cfg, c) for c in set(C.DEC_CLIPS)}
    return cfg, ref, encs


def test_decode_table_shape():
    t = C.DEC_TABLE
    assert len(t) == len(set(t)) >= 48 and {len(s) for s in t} == {1, 2, 3, 4, 5, 6}
    assert any(a != b and b[: len(a)] == a for a in t for b in t)       # a sequence that is a strict prefix of another
    cfg, _ = C.dec_checkpoint()
    gp = C.dec_gp(cfg)
    used = {x for s in t for x in s}
    assert not used & (set(gp.suppress_tokens) | set(gp.begin_suppress_tokens) | {gp.eos_token_id}) and gp.exp_decay is None


@pytest.mark.parametrize("name", sorted(C.DEC_CASES))
def test_greedy_cases_differ_at_the_root_and_later_and_are_decisive(dec_ref, name):
    cfg, ref, encs = dec_ref
    gp = C.dec_gp(cfg, C.DEC_CASES[name][0])
    ents = C.case_entries(name)
    runs = C.dec_guards(ref, gp, encs, C.DEC_TABLE, ents)
    if ents:                                         # the boost and the penalty act: another member of the table than without them
        base = C.dec_guards(ref, C.dec_gp(cfg), encs, C.DEC_TABLE, None)
        assert gp.repetition_penalty != 1.0 and all(runs[c][0] != base[c][0] for c in runs)
        assert tuple(runs[0][0][len(gp.prompt):-1]) == C.DEC_TABLE[C.DEC_CASES[name][1]]


def test_sampled_case_is_decisive(dec_ref):
    cfg, ref, encs = dec_ref
    k = C.SAMPLE_CASE
    C.sample_guards(ref, C.dec_gp(cfg), encs, C.DEC_TABLE, k["T"], k["seed"], (k["top_k"], 1.0, 0.0))


@pytest.mark.parametrize("name", sorted(C.BEAM_CASES))
def test_beam_cases_keep_2n_finite_candidates_and_are_decisive(name):
    cfg, sd, gp, case, runs, seqs = C.beam_reference(name)
    n = case[2]
    assert n == (4 if name == "n4" else 2) and case[7] == n and len(seqs) == 2 * n * (4 ** C.BEAM_DEPTH - 1) // 3 == len(set(seqs))
    used = {x for s in seqs for x in s}
    assert not used & (set(gp.suppress_tokens) | set(gp.begin_suppress_tokens) | {gp.eos_token_id}) and gp.exp_decay is None
    C.beam_guards(runs, gp, n)
    # the processor built with num_beams = n reads n rows per clip: one row alone would come back all -inf
    proc = C.hf_processor(seqs, gp.eos_token_id, len(gp.prompt), n)
    one = proc(torch.tensor([list(gp.prompt)]), torch.zeros(1, cfg.vocab_size))
    assert torch.isinf(one).all()


def test_under_populated_beam_case_shape():
    assert len(C.FEW_TABLE) == 3 < C.FEW_CASE[2] == 4 == C.FEW_CASE[7]
