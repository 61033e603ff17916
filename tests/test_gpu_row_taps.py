"""The staging of the parity taps on the GPU (csrc/wm_internal.h: wm_tap_stage / wm_tap_groups).  sample_rows, filter_rows,
score_rows, topk_rows and seq_bias_rows promise that a row's result does not depend on where the row stands in the call; the sampling, scoring and
sequence-bias suites hold that for equal-length prefixes inside one call.  Here the promise is fixed at the group boundaries with ragged prefixes:
max_batch = 1 makes the logits scratch 16 rows, so the taps work in groups of 15 (WM_TAP_ROWS) or 16 (score / top-k) and R = 15, 16, 17, 33 put a
boundary at, before and behind both.  The batched call must equal, bit for bit, the R single-row calls and the reverse of the reversed call.
(select_rows takes cur_len from row 0 of the call and lang_pick_rows has this test in tests/test_gpu_language_list.py: neither is here.)"""
import dataclasses

import numpy as np
import pytest

from helpers import MedusaConfig, GenParams, synth, ACCEPT_GREEDY
from whisper_medusa import WhisperMedusaModel

pytestmark = pytest.mark.gpu

V, RMAX = 516, 33
RS = [1, 15, 16, 17, 33]
TAPS = ["sample_rows", "filter_rows", "score_rows", "topk_rows"]
_SINGLE = {}            # (tap, setting) -> the RMAX single-row results, computed once


def _cfg():
    """micro(vocab=516) with the vocabulary ending in a max_source_positions + 1 timestamp block (the remap of tests/scores_ref.py micro_ts)"""
    c = MedusaConfig.micro(vocab=V)
    tb = V - (c.max_source_positions + 1)
    return dataclasses.replace(c, eos_token_id=tb - 4, pad_token_id=tb - 4, decoder_start_token_id=tb - 3, prev_sot_token_id=tb - 2,
                               no_timestamps_token_id=tb - 1, begin_suppress_tokens=[7, tb - 4], max_initial_timestamp_index=5)


def _gp(cfg, setting):
    """plain, or the timestamp rules with both repetition rules: every processor that reads a row's own prefix"""
    ts = setting == "ts_rep"
    rep = dict(repetition_penalty=1.3, no_repeat_ngram_size=2) if ts else {}
    return GenParams(prompt=synth.default_prompt(cfg, timestamps=ts), eos_token_id=cfg.eos_token_id, pad_token_id=cfg.pad_token_id,
                     suppress_tokens=[3, 40], begin_suppress_tokens=[cfg.timestamp_begin + 2, 7], max_length=cfg.max_target_positions,
                     hard_max_length=cfg.max_length, exp_decay=(2, 1.0625), accept_mode=ACCEPT_GREEDY, temperature=0.0, vanilla=True, timestamps=ts,
                     no_timestamps_token_id=cfg.no_timestamps_token_id if ts else -1,
                     max_initial_timestamp_index=cfg.max_initial_timestamp_index if ts else None, **rep)


def _inputs(gp):
    """seeded rows; prefixes of prompt + 0 .. 6 ids, no two neighbours of one length; distinct keys and targets"""
    rng = np.random.default_rng(1234)
    rows = (3.0 * rng.standard_normal((RMAX, V))).astype(np.float32)
    extra = [(0, 3, 1, 6, 2, 5, 4)[r % 7] for r in range(RMAX)]
    pre = [list(gp.prompt) + rng.integers(0, V, size=extra[r]).tolist() for r in range(RMAX)]
    assert all(len(pre[r]) != len(pre[r + 1]) for r in range(RMAX - 1)) and {len(p) - len(gp.prompt) for p in pre} == set(range(7))
    keys = [1000003 * r + 17 for r in range(RMAX)]
    targets = [(37 * r + 5) % V for r in range(RMAX)]
    assert len(set(keys)) == RMAX and len(set(targets)) == RMAX
    return rows, pre, keys, targets


def _entries(pre):
    """one-token entries, and entries whose leading ids end some of the prefixes (so the bias differs from row to row)"""
    ents = [((9,), 1.5), ((40,), float("-inf")), ((V - 1,), -2.25)]
    for r in (3, 5, 10, 12, 20, 31):
        tail = pre[r][-min(len(pre[r]), 3):]
        ents.append((tuple(tail) + (100 + r,), 0.5 + r))
    return ents


@pytest.fixture(scope="module")
def rig(gpu):
    cfg = _cfg()
    m = WhisperMedusaModel(cfg, synth.synth_state_dict(cfg, seed=3), device=gpu, max_batch=1)
    yield cfg, m.engine
    m.engine.close()


def _call(eng, cfg, tap, setting, idx):
    """the tap over rows `idx` of the inputs, as a list of arrays"""
    gp = _gp(cfg, "plain" if tap == "seq_bias_rows" else setting)
    rows, pre, keys, targets = _inputs(gp)
    x, p = rows[idx], [pre[i] for i in idx]
    k, t = [keys[i] for i in idx], [targets[i] for i in idx]
    if tap == "sample_rows":
        o = eng.sample_rows(gp, x, p, k, 0.75, 0x5EED)
        return [o["token"], o["value"], o["ts_forced"]]
    if tap == "filter_rows":
        o = eng.filter_rows(gp, x, p, k, 0.75, 0x5EED, top_k=7, top_p=0.9, min_p=0.01)
        return [o["thr"], o["kept"], o["ts_forced"], o["token"], o["value"]]
    if tap == "score_rows":
        return [eng.score_rows(gp, x, p, t)]
    if tap == "topk_rows":
        return list(eng.topk_rows(gp, x, p, t, 4))
    return [eng.seq_bias_rows(_entries(pre), x, p)]


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()          # bit for bit, NaN and -inf included


def _check(rig, tap, setting, R):
    cfg, eng = rig
    if (tap, setting) not in _SINGLE:
        one = [_call(eng, cfg, tap, setting, [r]) for r in range(RMAX)]
        _SINGLE[(tap, setting)] = [np.concatenate([o[j] for o in one]) for j in range(len(one[0]))]
    idx = list(range(R))
    fwd = _call(eng, cfg, tap, setting, idx)
    rev = _call(eng, cfg, tap, setting, idx[::-1])
    for j, a in enumerate(fwd):
        assert _same(a, _SINGLE[(tap, setting)][j][:R]), (tap, setting, R, j, "batched call != single-row calls")
        assert _same(np.ascontiguousarray(rev[j][::-1]), a), (tap, setting, R, j, "reversed call != batched call")


@pytest.mark.parametrize("R", RS)
@pytest.mark.parametrize("setting", ["plain", "ts_rep"])
@pytest.mark.parametrize("tap", TAPS)
def test_rows_do_not_depend_on_their_group(rig, tap, setting, R):
    _check(rig, tap, setting, R)


@pytest.mark.parametrize("R", RS)
def test_seq_bias_rows_do_not_depend_on_their_group(rig, R):
    _check(rig, "seq_bias_rows", "plain", R)


def test_the_bias_table_reads_the_ragged_prefixes(rig):
    """the one-token entries edit every row, the longer ones only the six rows whose prefix they end: the edit differs from row to row"""
    cfg, eng = rig
    assert eng.max_batch == 1
    rows = _inputs(_gp(cfg, "plain"))[0]
    hit = (_call(eng, cfg, "seq_bias_rows", "plain", list(range(RMAX)))[0] != rows).sum(axis=1)
    assert hit.min() >= 1 and len(set(hit.tolist())) > 1
