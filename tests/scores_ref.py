"""CPU reference of the token log-probabilities (include/wm.h wm_score_tokens), pinned to transformers' own code.

One teacher-forced oracle pass per stream gives the base-head logits of every input position; each generated position's row then goes through
`oracle.process_logits` at the row's OWN length, transformers' WhisperTimeStampLogitsProcessor under the row's own prefix when the timestamp
rules are on (built as tests/test_gpu_timestamps.py::hf_processor builds it), and `torch.log_softmax` in fp64.  Averages and compression ratios
come from WhisperGenerationMixin's static methods, the no-speech probability from the softmax line of WhisperNoSpeechDetection.__call__."""
import copy
import dataclasses

import torch

from helpers import MedusaConfig, GenParams, synth, ACCEPT_TYPICAL  # noqa: F401  (also puts the package on sys.path)
from oracle.whisper_medusa_oracle import process_logits


def micro_ts(heads_type="base_head", K=4):
    """The micro shape of tests/test_gpu_timestamps.py: vocabulary ending in a max_source_positions + 1 timestamp block."""
    c = MedusaConfig.micro(K=K, heads_type=heads_type)
    tb = c.vocab_size - (c.max_source_positions + 1)
    c = dataclasses.replace(c, eos_token_id=tb - 4, pad_token_id=tb - 4, decoder_start_token_id=tb - 3, prev_sot_token_id=tb - 2,
                            no_timestamps_token_id=tb - 1, begin_suppress_tokens=[7, tb - 4], max_initial_timestamp_index=5)
    assert c.supports_timestamps
    return c


TS_SCALE = 3.0


def ts_state_dict(cfg, seed, ts_scale=TS_SCALE):
    """The ts_scale recipe of tests/test_gpu_timestamps.py::state_dict."""
    sd = synth.synth_state_dict(cfg, seed=seed)
    sd["whisper_model.proj_out.weight"][cfg.timestamp_begin:] *= ts_scale
    return sd


def hf_processor(cfg, begin_index):
    from transformers import GenerationConfig
    from transformers.generation.logits_process import WhisperTimeStampLogitsProcessor
    gc = GenerationConfig(no_timestamps_token_id=cfg.no_timestamps_token_id, eos_token_id=cfg.eos_token_id)
    gc.max_initial_timestamp_index = cfg.max_initial_timestamp_index
    return WhisperTimeStampLogitsProcessor(gc, begin_index=begin_index, _detect_timestamp_from_logprob=True)


def masks_only(proc):
    q = copy.copy(proc)
    q._detect_timestamp_from_logprob = False
    return q


def decision_margin(row, tb):
    """|logsumexp(ts) - max(text)| of a row after the per-token masks."""
    lse = torch.logsumexp(row[tb:].double(), 0)
    mt = row[:tb].double().max()
    return float((lse - mt).abs())


def processed_row(z_row, prefix, gp, proc=None):
    """HF's processors on one raw logits row under ``prefix`` (cur_len = len(prefix), the row's own length) -> (fp32 row, decision margin)."""
    x = process_logits(z_row[None].float(), len(prefix), gp)
    margin = float("inf")
    if proc is not None:
        ids = torch.tensor([list(prefix)])
        margin = decision_margin(masks_only(proc)(ids, x.clone())[0], proc.timestamp_begin)
        x = proc(ids, x.clone())
    return x[0], margin


def row_logprob(z_row, prefix, target, gp, proc=None):
    x, margin = processed_row(z_row, prefix, gp, proc)
    return float(torch.log_softmax(x.double(), 0)[target]), margin


def no_speech_prob(z_row, token):
    """WhisperNoSpeechDetection.__call__: `probs = no_speech_scores.float().softmax(dim=-1)`; `probs[:, no_speech_token]`."""
    return float(z_row[None].float().softmax(dim=-1)[:, token][0])


def hf_avg_logprob(score_rows, tokens):
    from transformers.models.whisper.generation_whisper import WhisperGenerationMixin
    return float(WhisperGenerationMixin._retrieve_avg_logprobs(tuple(score_rows), torch.tensor(tokens), 0.0))


def hf_compression_ratio(tokens, vocab_size):
    from transformers.models.whisper.generation_whisper import WhisperGenerationMixin
    return float(WhisperGenerationMixin._retrieve_compression_ratio(torch.tensor(tokens), vocab_size))


def reference_scores(orc, enc, ids, P, gp, cfg, sot_index=0, no_speech_token=None):
    """Scores of the stream ``ids`` (prompt ids[:P], its own end) from ONE teacher-forced oracle pass.  Returns a dict: logprobs [T] (0 before
    P), margins [T] (timestamp-decision margin of every scored row, inf with the rules off), avg_logprob and compression_ratio by
    transformers' static methods, no_speech_prob."""
    ids = [int(t) for t in ids]
    T = len(ids)
    z = orc.decoder_pass(orc.new_state(enc), ids[:-1], 0, True)[0]        # [T - 1, V]: row t - 1 is the logits given ids[:t]
    proc = hf_processor(cfg, gp.begin_index) if gp.timestamps else None
    lp, mg, rows = [0.0] * T, [float("inf")] * T, []
    for t in range(P, T):
        x, mg[t] = processed_row(z[t - 1], ids[:t], gp, proc)
        rows.append(x)
        lp[t] = float(torch.log_softmax(x.double(), 0)[ids[t]])
    out = dict(logprobs=lp, margins=mg,
               avg_logprob=hf_avg_logprob(rows, ids[P:]) if rows else 0.0,
               compression_ratio=hf_compression_ratio(ids[P:], cfg.vocab_size) if T > P else 0.0)
    if no_speech_token is not None:
        out["no_speech_prob"] = no_speech_prob(z[sot_index], no_speech_token)
    return out
