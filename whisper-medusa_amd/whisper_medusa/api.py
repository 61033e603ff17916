"""Drop-in ``WhisperMedusaModel`` backed by the HIP engine.

Mirrors the reference's public API for the inference path (whisper_medusa/models/model.py):
``from_pretrained`` (:265-291), ``generate`` (:1419-1779, same keyword names, same error behaviour for
the unsupported features), ``forward`` (:1223-1347, logits ``[K+1, B, T, V]``), ``to``/``eval``.
The canonical caller is eval_whisper_medusa.py:28-69 / README.md:101-142:

    model = WhisperMedusaModel.from_pretrained(path); model = model.to("cuda")
    ids = model.generate(input_features, language="en")        # LongTensor [1, T]
    text = processor.decode(ids[0], skip_special_tokens=True)

Differences, all supersets: batch > 1 is accepted (semantics = B independent batch-1 runs, SURVEY.md §0
fact 2); ``extract_features(wav)`` computes the log-mel on the GPU (the reference leaves it to
``WhisperProcessor``); ``vanilla=True`` runs plain greedy decoding for the anchor measurement.
"""
from __future__ import annotations

from dataclasses import dataclass, field, replace
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from .config import MedusaConfig, GenParams, ACCEPT_TYPICAL, ACCEPT_GREEDY, language_token
from .engine import Engine, SEQ_BIAS_MAX as _SEQ_BIAS_MAX, SEQ_BIAS_MAX_LEN as _SEQ_BIAS_MAX_LEN
from .engine import CONSTRAINT_MAX as _CONSTRAINT_MAX, CONSTRAINT_MAX_LEN as _CONSTRAINT_MAX_LEN
from . import engine as _engine_mod
from . import weights as _weights
from . import synth as _synth
from . import timestamps as _timestamps
from . import scores as _scores
from . import words as _words
from . import vad as _vad


class EngineKVCache:
    """``past_key_values`` of ``forward(use_cache=True)``: the self-attention K/V rows themselves stay in the engine's contiguous cache
    (DESIGN.md §3); this handle records which engine / encoder pass / batch they belong to and how many positions are filled, which
    is all a following ``forward(past_key_values=...)`` needs to append behind them (HF's Cache.get_seq_length())."""

    def __init__(self, engine_id: int, enc_stamp, kv_stamp, batch: int, seq_length: int):
        self.engine_id, self.enc_stamp, self.kv_stamp, self.batch, self._len = engine_id, enc_stamp, kv_stamp, batch, int(seq_length)

    def get_seq_length(self, layer_idx: int = 0) -> int:
        return self._len

    def __len__(self):
        return self._len


class EngineEncoderOutput:
    """``encoder_outputs`` as ``forward`` hands them back (HF BaseModelOutput shape: ``[0]`` / ``.last_hidden_state``).  The hidden
    state is fetched from the engine only when somebody looks at it; passed back into ``forward(encoder_outputs=...)`` while the
    engine still holds that encoder pass, it is recognised by its stamp and nothing is recomputed."""

    def __init__(self, engine, batch: int, stamp):
        self._engine, self._batch, self._wm_stamp, self._t = engine, batch, stamp, None

    @property
    def last_hidden_state(self) -> torch.Tensor:
        if self._t is None:
            if getattr(self._engine, "_enc_stamp", None) is not self._wm_stamp:
                raise RuntimeError("this encoder pass is no longer resident in the engine")
            self._t = self._engine.encoder_output_cached(self._batch)
        return self._t

    def __getitem__(self, i):
        if i != 0:
            raise IndexError(i)
        return self.last_hidden_state


@dataclass
class MedusaForwardOutput:
    """Seq2SeqLMOutput fields the engine can fill (model.py:1336-1347)."""
    logits: torch.Tensor                 # [K+1 (or 1), B, T, V]  (model.py:1301)
    past_key_values: Optional[EngineKVCache] = None
    encoder_outputs: Optional[EngineEncoderOutput] = None
    loss: Optional[torch.Tensor] = None

    @property
    def encoder_last_hidden_state(self):
        return None if self.encoder_outputs is None else self.encoder_outputs.last_hidden_state


class GenerateEncoderDecoderOutput(dict):
    """What ``generate(return_dict_in_generate=True)`` returns in the reference (model.py:812-823: HF's ModelOutput of the same
    name): fields by attribute, by key and by position.  The engine keeps scores / attentions / hidden states on the device and
    never materialises them, so — as in the reference when ``output_scores`` etc. are not requested — they are ``None``; the KV
    cache is engine state, not a Python object (``past_key_values`` is ``None``)."""
    _fields = ("sequences", "scores", "logits", "encoder_attentions", "encoder_hidden_states", "decoder_attentions",
               "cross_attentions", "decoder_hidden_states", "past_key_values")

    def __init__(self, sequences, **extra):
        super().__init__()                       # like ModelOutput: only the fields that are not None are keys
        self["sequences"] = sequences
        self.update({k: v for k, v in extra.items() if v is not None})

    def __getattr__(self, k):
        if k in self:
            return dict.__getitem__(self, k)
        if k in self._fields:
            return None
        raise AttributeError(k)

    def to_tuple(self):
        return tuple(dict.__getitem__(self, k) for k in self.keys())

    def __getitem__(self, k):
        if isinstance(k, int):
            return self.to_tuple()[k]
        return super().__getitem__(k)


# HF logits processors / stopping criteria that are STATIC functions of (token id, current length) are lowered into wm_gen_params
# (reference: generate() hands `logits_processor` / `stopping_criteria` to HF's _get_logits_processor / _get_stopping_criteria,
# model.py:1106-1124; the engine fuses exactly these into its select kernels).  Matched by class name: no transformers import.
_LOWERABLE_PROCESSORS = ("SuppressTokensLogitsProcessor", "SuppressTokensAtBeginLogitsProcessor", "ExponentialDecayLengthPenalty")
_LOWERABLE_CRITERIA = ("MaxLengthCriteria", "EosTokenCriteria")


def _needs_host_processors(logits_processor) -> bool:
    """Is a logits processor given that the engine cannot lower (lower_processors keeps it for the host loop)?"""
    return any(type(p_).__name__ not in _LOWERABLE_PROCESSORS for p_ in (logits_processor or []))


def _as_int_list(x) -> List[int]:
    if x is None:
        return []
    if hasattr(x, "flatten"):
        return [int(v) for v in x.flatten().tolist()]
    if isinstance(x, (list, tuple, set)):
        return [int(v) for v in x]
    return [int(x)]


def lower_processors(gp: GenParams, logits_processor, stopping_criteria) -> GenParams:
    """Fold caller-supplied HF processors / criteria into the generation parameters.  A custom processor replaces the default of
    its type (HF's merge rule); a logits processor that is not a static mask / penalty is kept for the host (``gp._host_processors``:
    generate() then runs the loop with the logits copied out after every pass — the slow path, the reference's own); a stopping
    criterion that is not a static length / EOS rule is kept for the host (``gp._host_criteria``) and evaluated after every iteration."""
    P = len(gp.prompt)
    for proc in (logits_processor or []):
        name = type(proc).__name__
        if name == "SuppressTokensLogitsProcessor":
            gp.suppress_tokens = _as_int_list(proc.suppress_tokens)
        elif name == "SuppressTokensAtBeginLogitsProcessor":
            # only the token list is the caller's: the reference overwrites begin_index on every processor that has set_begin_index
            # with the number of init tokens (model.py:1537, :1640-1644) — _gen_params has already put that number in gp
            gp.begin_suppress_tokens = _as_int_list(proc.begin_suppress_tokens)
        elif name == "ExponentialDecayLengthPenalty":
            if _as_int_list(proc.eos_token_id) != [gp.eos_token_id]:
                raise NotImplementedError("ExponentialDecayLengthPenalty on a token other than eos_token_id is not supported by the HIP engine")
            start = int(proc.regulation_start) - P                   # regulation_start is absolute in HF, relative to the prompt in wm_gen_params
            if start < 0:
                # HF would already be penalising at the first generated token with exponent P - regulation_start; the engine's
                # field cannot say that (negative = off), and silently dropping the penalty would change the tokens
                raise NotImplementedError(f"ExponentialDecayLengthPenalty.regulation_start ({int(proc.regulation_start)}) lies inside the "
                                          f"decoder prompt ({P} tokens): build it with input_ids_seq_length = the prompt length")
            gp.exp_decay = (start, float(proc.regulation_factor))
        else:
            # any other processor is a Python callable on the logits (the reference hands the list to HF, model.py:1106-1116): it runs on
            # the host between the engine's passes (WhisperMedusaModel._decode_host_processors: the reference's own loop structure,
            # one stream at a time, logits copied out after every pass).  Order as in HF: the defaults above first, custom ones after.
            gp._host_processors = (gp._host_processors or []) + [proc]
    for crit in (stopping_criteria or []):
        name = type(crit).__name__
        if name == "MaxLengthCriteria":
            gp.max_length = min(gp.max_length, int(crit.max_length))
        elif name == "EosTokenCriteria":
            if _as_int_list(crit.eos_token_id) != [gp.eos_token_id]:
                raise NotImplementedError("EosTokenCriteria with other ids than eos_token_id is not supported by the HIP engine")
        else:
            # anything else is evaluated on the host after every iteration (generate(): the per-iteration path the streamer uses),
            # exactly where the reference calls it (model.py:786: once per Medusa iteration, on the ids emitted so far)
            gp._host_criteria = (gp._host_criteria or []) + [crit]
    return gp


# ---- sequence bias, bad words and hotwords (engine: csrc/wm_seq_bias.hip) -----------------------------------------------------
def _is_int(t) -> bool:
    return isinstance(t, (int, np.integer)) and not isinstance(t, bool)


def sequence_bias_entries(sequence_bias, vocab_size: int) -> List[Tuple[Tuple[int, ...], float]]:
    """HF ``generate(sequence_bias=)`` -> [(ids, bias), ..] in the caller's order, under SequenceBiasLogitsProcessor's own validation and
    messages (transformers generation/logits_process.py ``_validate_arguments`` / ``_prepare_bias_variables``).  Both of HF's forms: a dict
    ``{tuple(ids): float}`` or a list of ``[ids, float]``, where a repeated sequence keeps its first place and its last value (HF's dict
    conversion)."""
    sb = sequence_bias
    if (not isinstance(sb, dict) and not isinstance(sb, list)) or len(sb) == 0:
        raise ValueError(f"`sequence_bias` has to be a non-empty dictionary, or non-empty list of lists but is {sb}.")
    if isinstance(sb, dict):
        if any(not isinstance(k, tuple) for k in sb):
            raise ValueError(f"`sequence_bias` has to be a dict with tuples as keys, but is {sb}.")
        if any(len(k) == 0 or any(not _is_int(t) or t < 0 for t in k) for k in sb):
            raise ValueError(f"Each key in `sequence_bias` has to be a non-empty tuple of positive integers, but is {sb}.")
        if any(not isinstance(b, float) for b in sb.values()):
            raise ValueError(f"`sequence_bias` has to be a dict with floats as values, but is {sb}.")
        merged = dict(sb)
    else:
        def ok(e):
            return (isinstance(e, (list, tuple)) and len(e) == 2 and isinstance(e[0], list) and len(e[0]) > 0
                    and all(_is_int(t) and t >= 0 for t in e[0]) and isinstance(e[1], float))
        if any(not ok(e) for e in sb):
            raise ValueError(f"Each element in `sequence_bias` has to be a non-empty list of lists of positive integers and float, but is {sb}.")
        merged = {}
        for ids, b in sb:
            merged[tuple(ids)] = b
    bad = [int(t) for k in merged for t in k if t >= vocab_size]
    if bad:
        raise ValueError(f"The model vocabulary size is {vocab_size}, but the following tokens were being biased: {bad}")
    return [(tuple(int(t) for t in k), float(b)) for k, b in merged.items()]


def bad_words_entries(bad_words_ids, eos_token_id: int, vocab_size: int) -> List[Tuple[Tuple[int, ...], float]]:
    """HF ``generate(bad_words_ids=)`` -> -inf entries, under NoBadWordsLogitsProcessor's validation and messages; ``[eos]`` is filtered out as
    that processor does."""
    bw = bad_words_ids
    if not isinstance(bw, list) or len(bw) == 0:
        raise ValueError(f"`bad_words_ids` has to be a non-empty list, but is {bw}.")
    if any(not isinstance(w, list) for w in bw):
        raise ValueError(f"`bad_words_ids` has to be a list of lists, but is {bw}.")
    if any(any(not _is_int(t) or t < 0 for t in w) for w in bw):
        raise ValueError(f"Each list in `bad_words_ids` has to be a list of positive integers, but is {bw}.")
    kept = [w for w in bw if w != [int(eos_token_id)]]
    if any(len(w) == 0 for w in kept):
        raise ValueError(f"Each key in `sequence_bias` has to be a non-empty tuple of positive integers, but is {bw}.")
    bad = [int(t) for w in kept for t in w if t >= vocab_size]
    if bad:
        raise ValueError(f"The model vocabulary size is {vocab_size}, but the following tokens were being biased: {bad}")
    return list({tuple(int(t) for t in w): float("-inf") for w in kept}.items())


def hotword_entries(hotwords, boost: float, tokenizer) -> List[Tuple[Tuple[int, ...], float]]:
    """The contextual-biasing convenience as a pure function: every word is encoded as ``w`` and as ``" " + w`` (no special tokens) and EVERY
    prefix t0, t0 t1, .. of each encoding becomes an entry with ``boost`` — each token of the phrase is lifted once its predecessors were
    emitted.  Duplicates collapse (first place kept).  ``tokenizer``: anything with ``encode(text, add_special_tokens=False) -> ids``."""
    if isinstance(hotwords, str) or not isinstance(hotwords, (list, tuple)) or len(hotwords) == 0 or any(not isinstance(w, str) or not w for w in hotwords):
        raise ValueError(f"`hotwords` has to be a non-empty list of non-empty strings, but is {hotwords!r}")
    if isinstance(boost, bool) or not isinstance(boost, (int, float, np.floating, np.integer)) or not np.isfinite(float(boost)):
        raise ValueError(f"`hotword_boost` has to be a finite float, but is {boost!r}")
    if tokenizer is None or not hasattr(tokenizer, "encode"):
        raise ValueError("`hotwords` needs a tokenizer (tokenizer=, or a model built with its processor): something with encode(text, add_special_tokens=False)")
    out: Dict[Tuple[int, ...], float] = {}
    for w in hotwords:
        for text in (w, " " + w):
            ids = [int(t) for t in tokenizer.encode(text, add_special_tokens=False)]
            for k in range(1, len(ids) + 1):
                out.setdefault(tuple(ids[:k]), float(boost))
    return list(out.items())


# ---- constrained decoding: a closed set of token sequences (engine: csrc/wm_constraint.hip) ------------------------------------
def allowed_sequence_entries(allowed_sequences, eos_token_id: int, vocab_size: int) -> List[Tuple[int, ...]]:
    """``generate(allowed_sequences=)`` -> [ids, ..] in the caller's order: a non-empty list of non-empty lists of token ids, none of them eos
    (every sequence is closed by eos implicitly).  Duplicates collapse (first place kept)."""
    a = allowed_sequences
    if isinstance(a, (str, bytes)) or not isinstance(a, (list, tuple)) or len(a) == 0:
        raise ValueError(f"`allowed_sequences` has to be a non-empty list of lists of token ids, but is {a!r}")
    if any(isinstance(q, (str, bytes)) or not isinstance(q, (list, tuple)) or len(q) == 0 or any(not _is_int(t) or t < 0 for t in q) for q in a):
        raise ValueError(f"Each element of `allowed_sequences` has to be a non-empty list of non-negative integers, but is {a!r}")
    bad = [int(t) for q in a for t in q if t >= vocab_size]
    if bad:
        raise ValueError(f"The model vocabulary size is {vocab_size}, but `allowed_sequences` holds the token ids {bad}")
    if any(int(t) == int(eos_token_id) for q in a for t in q):
        raise ValueError(f"`allowed_sequences`: eos_token_id ({int(eos_token_id)}) must not stand inside a sequence: every sequence is closed "
                         "by eos implicitly")
    return list(dict.fromkeys(tuple(int(t) for t in q) for q in a))


def allowed_phrase_entries(phrases, tokenizer) -> List[Tuple[int, ...]]:
    """``generate(allowed_phrases=)`` as a pure function: every phrase is encoded as ``p`` and as ``" " + p`` (no special tokens), like
    ``hotword_entries``; each encoding is one allowed sequence.  Duplicates collapse (first place kept); a phrase that encodes to nothing is
    refused.  ``tokenizer``: anything with ``encode(text, add_special_tokens=False) -> ids``."""
    if isinstance(phrases, str) or not isinstance(phrases, (list, tuple)) or len(phrases) == 0 or any(not isinstance(p, str) or not p for p in phrases):
        raise ValueError(f"`allowed_phrases` has to be a non-empty list of non-empty strings, but is {phrases!r}")
    if tokenizer is None or not hasattr(tokenizer, "encode"):
        raise ValueError("`allowed_phrases` needs a tokenizer (tokenizer=, or a model built with its processor): something with "
                         "encode(text, add_special_tokens=False)")
    out: Dict[Tuple[int, ...], None] = {}
    for p in phrases:
        for text in (p, " " + p):
            ids = tuple(int(t) for t in tokenizer.encode(text, add_special_tokens=False))
            if not ids:
                raise ValueError(f"`allowed_phrases`: {text!r} encodes to no token")
            out.setdefault(ids)
    return list(out)


def _resolve_checkpoint(name_or_path, revision=None, cache_dir=None, local_files_only=False) -> str:
    """A checkpoint directory as it is; anything else is taken as a hub repo id and resolved with huggingface_hub.snapshot_download
    (cached snapshot first; config, weights and tokenizer files only)."""
    import os
    path = os.fspath(name_or_path)
    if os.path.isdir(path):
        return path
    try:
        from huggingface_hub import snapshot_download
    except ImportError as e:                                    # pragma: no cover - huggingface_hub ships with transformers
        raise OSError(f"{path!r} is not a checkpoint directory and huggingface_hub is not installed to resolve it as a hub name") from e
    patterns = ["*.json", "*.safetensors", "pytorch_model.bin", "*.txt", "*.model"]
    try:
        try:
            return snapshot_download(path, revision=revision, cache_dir=cache_dir, allow_patterns=patterns, local_files_only=True)
        except Exception:
            if local_files_only:
                raise
            return snapshot_download(path, revision=revision, cache_dir=cache_dir, allow_patterns=patterns)
    except Exception as e:
        raise OSError(f"{path!r} is neither a checkpoint directory nor a hub repository that could be resolved "
                      f"({type(e).__name__}: {e})") from e


# ---- ragged per-stream rows -> tensors, and the slices of a row that belong to its segments ----------------------------------------------------
def _stack_rows(rows, fill, dtype, T: Optional[int] = None) -> torch.Tensor:
    """Ragged rows (lists, arrays or 1-D tensors) -> [len(rows), T or the longest]; behind a row's end ``fill``, or with ``fill=None`` the
    row's own last value.  Built where the rows live (tensor rows: their device; anything else: the CPU)."""
    dev = rows[0].device if isinstance(rows[0], torch.Tensor) else None
    t = torch.full((len(rows), max(len(r) for r in rows) if T is None else T), 0 if fill is None else fill, dtype=dtype, device=dev)
    for i, r in enumerate(rows):
        t[i, : len(r)] = torch.as_tensor(r, dtype=dtype)
        if fill is None and len(r):
            t[i, len(r):] = t[i, len(r) - 1]
    return t


def _ids_tensor(rows, pad: int) -> torch.Tensor:
    """Token id rows -> LongTensor, right-padded with ``pad``."""
    return _stack_rows(rows, pad, torch.long)


def _ts_tensor(rows, T: Optional[int] = None) -> torch.Tensor:
    """Per-stream token timestamps -> float32 [B, T] next to the padded ids: positions after a stream's end repeat its last value."""
    return _stack_rows(rows, None, torch.float32, T)


def _lp_tensor(rows, T: Optional[int] = None) -> torch.Tensor:
    """Per-stream token log-probabilities -> float32 [B, T] next to the padded ids: 0 after a stream's end."""
    return _stack_rows(rows, 0.0, torch.float32, T)


def _segment_slices(segments, prompt_len: int, name: str, row) -> None:
    """Every segment of one output row gets, as ``name``, the slice of ``row`` (values per position of that output row) under its own tokens."""
    o = prompt_len
    for sg in segments:
        n = int(sg["tokens"].numel())
        sg[name] = row[o: o + n]
        o += n


@dataclass
class ResolvedCall:
    """What generate() has made of its arguments, once per public call, for the route that decodes it: the request dicts of
    the features that ride on the short-form decode (None: not asked for) and the resolved scalars."""
    samp: Optional[dict] = None              # seeded sampling / temperature fallback (_sampling_request)
    bias: Optional[list] = None              # sequence bias entries (_bias_request)
    cons: Optional[list] = None              # allowed sequences (_constraint_request)
    beam: Optional[dict] = None              # beam search (_beam_request)
    sc_req: Optional[dict] = None            # scoring pass: token log-probabilities, thresholds, alternatives
    tt_req: Optional[dict] = None            # token timestamps (_token_ts_request)
    rep_pen: float = 1.0
    rep_g: int = 0
    return_timestamps: bool = False
    time_precision: float = 0.02
    task: Optional[str] = None
    prompt_ids: Optional[torch.Tensor] = None
    temperature: Union[None, float, Sequence[float]] = None
    logits_processor: Optional[list] = None
    stopping_criteria: Optional[list] = None
    return_dict_in_generate: Optional[bool] = None
    return_segments: bool = False
    opts: dict = field(default_factory=dict)     # the call's other keywords as given: max_new_tokens, max_length, vanilla, posterior_*, streamer, ..


@dataclass
class ShortResult:
    """What one short-form decode (_generate_short) hands to its route; nothing of it travels through the model's attributes."""
    seqs: List[List[int]]                            # per stream: prompt + generated ids (beams: num_return_sequences rows per clip, clip-major)
    gp: GenParams                                    # the parameters it ran under (``prompt`` / ``prompts``: the decoder prompts)
    stats: dict
    token_timestamps: Optional[torch.Tensor] = None  # [B, T] next to the padded ids
    scores: Optional[dict] = None                    # _score_pack's fields (with the fallback fields, where both were asked for)
    sequences_scores: Optional[torch.Tensor] = None  # beam search
    fallback: Optional[dict] = None                  # fallback_temperature / fallback_attempts
    fallback_beams: Optional[dict] = None            # clip -> hypotheses of its beam-search attempt


class WhisperMedusaModel:
    def __init__(self, config: MedusaConfig, state_dict: Dict[str, torch.Tensor], device: Union[str, torch.device, None] = None,
                 max_batch: int = 1, dec_weight_fp8: bool = False, enc_fp8: bool = False, act_fp16: Optional[bool] = None,
                 cross_kv_fp8: bool = False):
        self.config = config
        self.generation_config = config          # posterior_threshold / alpha / token ids live on the config here
        self._sd = state_dict
        self._max_batch = max_batch
        self._fp8 = bool(dec_weight_fp8)         # decoder-layer matrices stored as fp8 e4m3 + per-row scale (BASELINE configs[4])
        self._enc_fp8 = bool(enc_fp8)            # encoder QKV / FC1 / cross-K/V projection on the fp8 MFMA (BASELINE configs[4])
        # decode numerics contract (include/wm.h wm_config.act_fp16): False = bf16 hi / lo operand pairs (libwm.so), True = one fp16
        # plane (libwm_f16.so, decoder matrices held as fp16); None = the default (engine.default_act_fp16: WM_ACT)
        from .engine import default_act_fp16
        self._act_fp16 = default_act_fp16() if act_fp16 is None else bool(act_fp16)
        self._xkv_fp8 = bool(cross_kv_fp8)       # the decode loop streams an e4m3 copy of the encoder cross-K/V (BASELINE configs[4]; wm_config.cross_kv_fp8)
        self._micro_batches = 1                  # contexts a batch is decoded with; None = automatic (set_micro_batches(None))
        self._pool = None
        self._engine: Optional[Engine] = None
        self._blob = None
        self.device = torch.device("cpu")
        if device is not None:
            self.to(device)

    # ---- construction ---------------------------------------------------------------------
    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path, *args, device=None, max_batch: int = 1, dec_weight_fp8: bool = False,
                        enc_fp8: bool = False, act_fp16: Optional[bool] = None, cross_kv_fp8: bool = False, **kwargs):
        """Load ``config.json`` + ``model.safetensors`` from a checkpoint directory, or from a Hugging Face hub name
        (``aiola/whisper-medusa-linear-libri``, README.md:101-104 of the reference) resolved through ``huggingface_hub`` — its
        local cache first, a download when the machine has network access (reference model.py:265-291)."""
        pretrained_model_name_or_path = _resolve_checkpoint(pretrained_model_name_or_path, kwargs.get("revision"),
                                                            kwargs.get("cache_dir"), kwargs.get("local_files_only", False))
        config = MedusaConfig.from_pretrained(pretrained_model_name_or_path)
        sd = _weights.load_state_dict_from_dir(pretrained_model_name_or_path)
        return cls(config, sd, device=device, max_batch=max_batch, dec_weight_fp8=dec_weight_fp8, enc_fp8=enc_fp8, act_fp16=act_fp16, cross_kv_fp8=cross_kv_fp8)

    def save_pretrained(self, save_directory: str, safe_serialization: bool = True) -> None:
        """``config.json`` + ``model.safetensors`` with the reference's parameter names (what its Trainer writes,
        trainer.py:45-51; the tied ``proj_out.weight`` is dropped like HF does) — re-loadable by ``from_pretrained`` here
        and by the reference.  Needs the state dict (models built with ``from_blob`` only hold the packed blob)."""
        import os
        if not self._sd:
            raise RuntimeError("save_pretrained needs the parameter state dict; this model was built from a packed blob")
        os.makedirs(save_directory, exist_ok=True)
        self.config.save_pretrained(save_directory)
        sd = {k: v.detach().cpu().contiguous().clone() for k, v in self._sd.items() if k != "whisper_model.proj_out.weight"}
        if safe_serialization:
            from safetensors.torch import save_file
            save_file(sd, os.path.join(save_directory, "model.safetensors"), metadata={"format": "pt"})
        else:
            torch.save(sd, os.path.join(save_directory, "pytorch_model.bin"))

    # ---- packed export (checkpoint tooling; the fp8 export format) -----------------------------------------
    PACKED_FORMAT = 1

    def save_packed(self, save_directory: str) -> None:
        """Write the engine-ready parameter blob: ``wm_packed.bin`` (the bytes ``wm_create`` consumes: bf16 MFMA-fragment
        matrices, fp32 vectors and — for models built with ``dec_weight_fp8`` / ``enc_fp8`` — the e4m3 matrices with their
        per-row scales, quantised once, on the CPU) and ``wm_packed.json`` (format + ABI layout version, the fp8 flags, the
        offset table, sha256 of the blob) next to ``config.json``.  ``from_packed`` loads it without touching the fp32 checkpoint."""
        import hashlib, json, os
        from .engine import WM_ABI_VERSION
        if self._blob is None:
            if not self._sd:
                raise RuntimeError("nothing to export: the model holds neither a state dict nor a packed blob")
            self._blob, self._offsets = _weights.build_blob(self.config, self._sd, device="cpu", dec_fp8=self._fp8, enc_fp8=self._enc_fp8, act_fp16=self._act_fp16)
        os.makedirs(save_directory, exist_ok=True)
        self.config.save_pretrained(save_directory)
        raw = self._blob.detach().cpu().contiguous().numpy().tobytes()
        with open(os.path.join(save_directory, "wm_packed.bin"), "wb") as f:
            f.write(raw)
        meta = dict(packed_format=self.PACKED_FORMAT, abi_layout=WM_ABI_VERSION, dec_weight_fp8=self._fp8, enc_fp8=self._enc_fp8, act_fp16=self._act_fp16, cross_kv_fp8=self._xkv_fp8,
                    n_bytes=len(raw), sha256=hashlib.sha256(raw).hexdigest(), offsets=[int(o) for o in self._offsets])
        with open(os.path.join(save_directory, "wm_packed.json"), "w") as f:
            json.dump(meta, f)

    @classmethod
    def from_packed(cls, directory: str, device=None, max_batch: int = 1):
        """Load a ``save_packed`` export.  Refuses a blob written for another parameter-table layout or with a wrong checksum."""
        import hashlib, json, os
        from .engine import WM_ABI_VERSION
        with open(os.path.join(directory, "wm_packed.json")) as f:
            meta = json.load(f)
        if meta.get("packed_format") != cls.PACKED_FORMAT or meta.get("abi_layout") != WM_ABI_VERSION:
            raise ValueError(f"packed export has format {meta.get('packed_format')} / table layout {meta.get('abi_layout')}; this build "
                             f"reads format {cls.PACKED_FORMAT} / layout {WM_ABI_VERSION}: re-export from the checkpoint")
        raw = np.fromfile(os.path.join(directory, "wm_packed.bin"), dtype=np.uint8)
        if raw.size != meta["n_bytes"] or hashlib.sha256(raw.tobytes()).hexdigest() != meta["sha256"]:
            raise ValueError("packed export is truncated or corrupt (size / sha256 mismatch)")
        config = MedusaConfig.from_pretrained(directory)
        if len(meta["offsets"]) != _weights.n_table_entries(config, meta["dec_weight_fp8"], meta["enc_fp8"]):
            raise ValueError("packed export's offset table does not match its config")
        self = cls(config, {}, device=None, max_batch=max_batch, dec_weight_fp8=meta["dec_weight_fp8"], enc_fp8=meta["enc_fp8"],
                   act_fp16=bool(meta.get("act_fp16", False)), cross_kv_fp8=bool(meta.get("cross_kv_fp8", False)))
        self._blob, self._offsets = torch.from_numpy(raw), np.asarray(meta["offsets"], dtype=np.uint64)
        return self.to(device) if device is not None else self

    @classmethod
    def from_blob(cls, config: MedusaConfig, blob: torch.Tensor, offsets: np.ndarray, max_batch: int = 1, dec_weight_fp8: bool = False,
                  enc_fp8: bool = False, act_fp16: bool = False, cross_kv_fp8: bool = False):
        """Build directly from a packed parameter blob already resident on a GPU (the path the
        8-GPU data-parallel launcher uses after the RCCL broadcast, ``dist.py``)."""
        self = cls(config, {}, device=None, max_batch=max_batch, dec_weight_fp8=dec_weight_fp8, enc_fp8=enc_fp8, act_fp16=act_fp16, cross_kv_fp8=cross_kv_fp8)
        self._blob, self._offsets = blob, offsets
        self.device = blob.device
        self._engine = Engine(config, blob, offsets, max_batch=max_batch, device=blob.device, dec_weight_fp8=dec_weight_fp8, enc_fp8=enc_fp8, act_fp16=act_fp16, cross_kv_fp8=cross_kv_fp8)
        return self

    def to(self, device):
        device = torch.device(device)
        if device.type != "cuda":
            if self._engine is None:
                self.device = device
                return self
            raise RuntimeError("the Whisper-Medusa engine runs on a HIP device only")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if self._engine is not None and self.device == device:
            return self
        self._drop_pool()
        if self._engine is not None:
            self._engine.close()                                   # frees its KV caches / scratch before the new context allocates
            self._engine = None
        with torch.cuda.device(device):
            if self._sd:
                self._blob, self._offsets = _weights.build_blob(self.config, self._sd, device=device, dec_fp8=self._fp8, enc_fp8=self._enc_fp8, act_fp16=self._act_fp16)
            elif self._blob is not None:
                self._blob = self._blob.to(device)                 # built with from_blob: move the packed blob itself
            else:
                raise RuntimeError("model has neither a state dict nor a packed blob to place on the device")
            self._engine = Engine(self.config, self._blob, self._offsets, max_batch=self._max_batch, device=device, dec_weight_fp8=self._fp8, enc_fp8=self._enc_fp8, act_fp16=self._act_fp16, cross_kv_fp8=self._xkv_fp8)
        self._drop_pool()
        self.device = device
        return self

    def cuda(self, device=None):
        return self.to("cuda" if device is None else device)

    def eval(self):
        return self

    def set_max_batch(self, max_batch: int):
        if max_batch != self._max_batch:
            self._max_batch = max_batch
            if self._engine is not None:
                self._engine.close()
                self._engine = Engine(self.config, self._blob, self._offsets, max_batch=max_batch, device=self.device, dec_weight_fp8=self._fp8, enc_fp8=self._enc_fp8, act_fp16=self._act_fp16, cross_kv_fp8=self._xkv_fp8)
            self._drop_pool()
        return self

    def set_micro_batches(self, n: Optional[int]):
        """Decode batches as ``n`` concurrent micro-batches (own engine context + HIP stream each, shared weights):
        see ``pool.py``.  n = 1 (default) is the single-context path — the model's own engine then holds the state of the
        last call (encoder output, statistics); ``None`` picks per call (``_micro_batches_for``).  Tokens do not depend on n."""
        if n is not None and n < 1:
            raise ValueError("micro_batches must be >= 1")
        if n != self._micro_batches:
            self._micro_batches = n
            self._drop_pool()
        return self

    def _micro_batches_for(self, B: int) -> int:
        """Contexts a batch of B clips is decoded with.  Automatic policy, measured on MI355X with large-v2 (tests/microbench/
        r02_call25.sh): two or three streams decode faster as single-stream contexts running side by side (2: 2135 vs 1455
        tokens/s, 3: 2335 vs 2187 — the single-stream kernels are the fused 16-row ones and two chains of short launches fill
        each other's gaps), from four streams on one batched context wins (4: 2822 vs 2517 / 2477; 8: 4177 vs 3834 / 2326)."""
        if self._micro_batches is not None:
            return self._micro_batches
        return B if B in (2, 3) else 1

    def _drop_pool(self):
        if self._pool is not None:
            self._pool.close()
            self._pool = None

    def _get_pool(self, n: int):
        """Pool of n contexts.  Under the automatic policy (two or three clips -> as many single-stream contexts) ONE pool serves both
        sizes: it is built with as many contexts as the first batch needs — two clips do not pay for a third context's KV caches and
        scratch — and GROWS to three when a batch of three arrives (the existing contexts, their caches and captured graphs stay)."""
        auto = self._micro_batches is None
        have = getattr(self, "_pool_n", None)
        if self._pool is not None and not auto and have != n:
            self._drop_pool()
        if self._pool is None:
            from .pool import ContextPool
            _ = self.engine                                         # raises when not on a HIP device
            # automatic policy: contexts of ONE stream each (per_ctx = ceil(max_batch / contexts) must not depend on the first batch's size)
            self._pool = ContextPool(self.config, self._blob, self._offsets, n, n if auto else max(self._max_batch, n), self._fp8, self._enc_fp8, self._act_fp16, self._xkv_fp8)
            self._pool_n = n
        elif auto and have < n:
            self._pool.grow(n)
            self._pool_n = n
        return self._pool

    @property
    def engine(self) -> Engine:
        if self._engine is None:
            raise RuntimeError("model is not on a HIP device: call model.to('cuda') first (there is no CPU path)")
        return self._engine

    def get_medusa_choice(self):
        return self.config.medusa_choices

    # ---- F0 ---------------------------------------------------------------------------------
    def extract_features(self, wav: Union[np.ndarray, torch.Tensor, Sequence[np.ndarray]], sampling_rate: int = 16000,
                         truncation: bool = True) -> torch.Tensor:
        """waveform(s) -> log-mel ``input_features`` [B, 80, 3000] on the GPU; pads / trims to 30 s like
        ``WhisperFeatureExtractor`` (eval_whisper_medusa.py:46-50).  Clips in a list are mono [n] or multi-channel
        [channels, n] (a bare 2-D array is a batch of mono clips); anything that is not 16 kHz mono first goes through the audio front door on the GPU
        (channel mean + torchaudio-default resampling, README.md:120-125 of the reference).

        ``truncation=False`` (``WhisperFeatureExtractor(truncation=False, padding="longest")``, the input of sequential long-form
        decoding): the clips are zero-padded as audio to the longest, rounded up to a multiple of 160 samples, and transformed whole in
        one call -> [B, n_mels, frames]; every clip's own frame count (``len // 160``: what HF derives from ``attention_mask``) is left
        in ``self.last_num_frames`` (LongTensor [B])."""
        n = 160 * self.config.n_mel_frames
        if isinstance(wav, (list, tuple)):
            clips = [np.asarray(w, dtype=np.float32) for w in wav]
        else:
            a = wav.detach().cpu().numpy() if isinstance(wav, torch.Tensor) else np.asarray(wav)
            a = a.astype(np.float32)
            clips = [a] if a.ndim == 1 else [r for r in a]          # 2-D array = batch of mono clips; multi-channel clips go in a list
        if len(clips) > self._max_batch:
            self.set_max_batch(len(clips))                          # wm_logmel checks B <= max_batch
        if not truncation:
            mono = self._wav_mono(clips, sampling_rate)
            n = max(160, -(-max(r.numel() for r in mono) // 160) * 160)
            buf = torch.zeros(len(mono), n, dtype=torch.float32, device=self.device)
            for i, r in enumerate(mono):
                buf[i, : r.numel()] = r
            self.last_num_frames = torch.tensor([r.numel() // 160 for r in mono], dtype=torch.long)
            return self.engine.logmel_long(buf)
        buf = torch.zeros(len(clips), n, dtype=torch.float32, device=self.device)
        for i, c in enumerate(clips):
            if c.ndim == 2 or sampling_rate != 16000:
                t = torch.from_numpy(np.atleast_2d(c)[None]).to(self.device)         # [1, channels, n_in]
                r = self.engine.resample(t, sampling_rate, 16000)[0]
            else:
                r = torch.from_numpy(c).to(self.device)
            m = min(r.numel(), n)
            buf[i, :m] = r[:m]
        return self.engine.logmel(buf)

    def features_from_file(self, path: str) -> torch.Tensor:
        """PCM WAV file -> ``input_features`` [1, 80, 3000] (decode, downmix, resample, log-mel)."""
        from .audio import read_wav
        x, sr = read_wav(path)
        return self.extract_features([x], sampling_rate=sr)

    # ---- generate ---------------------------------------------------------------------------
    def _gen_params(self, language, task, exponential_decay_length_penalty, max_new_tokens, max_length,
                    temperature, vanilla, posterior_threshold, posterior_alpha, suppress_tokens,
                    begin_suppress_tokens, prompt_ids, timestamps: bool = False, repetition_penalty=None, no_repeat_ngram_size=None) -> GenParams:
        cfg = self.config
        # G1, model.py:1519-1537; timestamps: without <|notimestamps|> (HF _retrieve_init_tokens with return_timestamps)
        # language=[...] (one entry per clip, already resolved by _language_list): one row of init tokens per clip, as HF's
        # _retrieve_init_tokens builds them — the rows differ at the language slot alone, so they have ONE length
        prompts = None
        if isinstance(language, (list, tuple)):
            prompts = [_synth.default_prompt(cfg, l, task or "transcribe", timestamps=timestamps) for l in language]
            language = language[0]
        prompt = _synth.default_prompt(cfg, language or "en", task or "transcribe", timestamps=timestamps)
        begin_suppress_index = None
        if prompt_ids is not None:
            # short-form conditioning (HF _prepare_decoder_input_ids): decoder_input_ids = cat([prompt_ids, init_tokens]);
            # `prompt_ids` comes from processor.get_prompt_ids() and already starts with <|startofprev|>
            pid = [int(t) for t in (prompt_ids.flatten().tolist() if hasattr(prompt_ids, "flatten") else list(prompt_ids))]
            if len(pid) + len(prompt) + cfg.medusa_num_heads + 2 > cfg.max_target_positions:
                raise ValueError(f"prompt_ids of length {len(pid)} leave no room to generate "                      # model.py:1526-1529
                                 f"(max_target_positions {cfg.max_target_positions})")
            begin_suppress_index = len(prompt)      # reference model.py:1537: begin_index = init_tokens.shape[1] (without prompt_ids)
            prompt = pid + prompt
            prompts = None if prompts is None else [pid + r for r in prompts]      # (the shared previous-text part, then each clip's init tokens)
        if prompts is not None and all(r == prompt for r in prompts):
            prompts = None                      # equal entries: the scalar call's parameters
        P = len(prompt)
        if max_new_tokens is not None:
            mlen = P + int(max_new_tokens)                                                # G2, model.py:1635-1639
        elif max_length is not None:
            mlen = int(max_length)
        else:
            mlen = cfg.max_length
        mlen = min(mlen, cfg.max_target_positions)
        if temperature is not None and float(temperature) > 0.0:
            # reference: do_sample path falls through with `result` unbound (model.py:1128-1156)
            raise NotImplementedError("sampling (temperature > 0) is not supported with medusa; pass sampling_seed= for the engine's seeded "
                                      "sampling on the plain decode path")
        # G4: generate() forces generation_config.temperature = 1.0 when not sampling (model.py:1877-1881),
        # so the typical-acceptance branch of evaluate_posterior runs.  temperature=0.0 selects exact-match.
        mode = ACCEPT_GREEDY if (temperature is not None and float(temperature) == 0.0) else ACCEPT_TYPICAL
        sup = list(cfg.suppress_tokens or []) if suppress_tokens is None else list(suppress_tokens)
        bsup = list(cfg.begin_suppress_tokens or []) if begin_suppress_tokens is None else list(begin_suppress_tokens)
        return GenParams(prompt=prompt, eos_token_id=cfg.eos_token_id, pad_token_id=cfg.pad_token_id,
                         suppress_tokens=sup, begin_suppress_tokens=bsup, max_length=mlen,
                         hard_max_length=cfg.max_length,
                         exp_decay=tuple(exponential_decay_length_penalty) if exponential_decay_length_penalty else None,
                         posterior_threshold=cfg.posterior_threshold if posterior_threshold is None else posterior_threshold,
                         posterior_alpha=cfg.posterior_alpha if posterior_alpha is None else posterior_alpha,
                         accept_mode=mode, temperature=1.0 if mode == ACCEPT_TYPICAL else 0.0, vanilla=bool(vanilla),
                         begin_suppress_index=begin_suppress_index, timestamps=bool(timestamps),
                         no_timestamps_token_id=cfg.no_timestamps_token_id if timestamps else -1,
                         max_initial_timestamp_index=cfg.max_initial_timestamp_index if timestamps else None,
                         repetition_penalty=1.0 if repetition_penalty is None else float(repetition_penalty),
                         no_repeat_ngram_size=0 if no_repeat_ngram_size is None else int(no_repeat_ngram_size), prompts=prompts)

    def _language_list(self, language, batch_size: int) -> List[str]:
        """``language=[...]`` of a generate() call over ``batch_size`` clips -> one language token string ('<|de|>') per clip.  HF's own checks and
        messages (WhisperGenerationMixin._retrieve_init_tokens): a None inside is a TypeError, a length other than the batch a ValueError; every
        entry is resolved as a scalar is (``Unsupported language: ...``)."""
        if any(l is None for l in language):
            raise TypeError("Expected `language` to be `None`, a single string (e.g. `'en'`), or a list of strings with "
                            "length equal to the batch size (e.g. `('en', 'fr')` for a batch size of 2). Got a list "
                            "containing `None`.")
        if len(language) != batch_size:
            raise ValueError("When passing a list of languages, the length of the list must match the batch size. "
                             f"Expected length of {batch_size}, but got {len(language)} languages.")
        out = []
        for l in language:
            if not isinstance(l, str):
                raise ValueError(f"Unsupported language: {l}")
            key = language_token(l)
            if self.config.is_multilingual and key not in self.config.lang_to_id:
                raise ValueError(f"Unsupported language: {l}")
            out.append(key)
        return out

    def _language_candidates(self) -> Tuple[List[str], List[int]]:
        """The language tokens of lang_to_id that lie inside the vocabulary, by id, and their ids: what language detection picks among."""
        cfg = self.config
        toks = [k for k in sorted(cfg.lang_to_id, key=lambda k: cfg.lang_to_id[k]) if 0 <= cfg.lang_to_id[k] < cfg.vocab_size]
        if not toks:
            raise ValueError("language detection: no language token of lang_to_id lies inside the vocabulary")
        return toks, [int(cfg.lang_to_id[t]) for t in toks]

    def _detect_language_on_device(self, feats: torch.Tensor) -> List[str]:
        """``group_by_language=False``: one encoder pass over ``feats`` on the model's own engine, then the engine's own detection
        (wm_detect_language: B ints come back, never a logits row).  The encoder pass stays resident for the decode that follows."""
        B = feats.shape[0]
        if B > self._max_batch:
            self.set_max_batch(B)
        toks, ids = self._language_candidates()
        if len(ids) > _engine_mod.LANG_MAX:
            raise ValueError(f"language detection: more than {_engine_mod.LANG_MAX} language tokens")
        eng = self.engine
        eng.encode(feats)
        name = dict(zip(ids, toks))
        return [name[i] for i in eng.detect_language(ids, self.config.decoder_start_token_id)]

    # ---- seeded sampling and HF's temperature fallback (engine: csrc/wm_sample.hip) -------------------------------------------
    def _sampling_request(self, temperature, kwargs, logits_processor) -> Optional[dict]:
        """The sampling side of a generate() call: None unless ``sampling_seed`` is given AND the call asks for sampling (a positive scalar
        temperature, ``do_sample=True``, or a tuple / list temperature: HF's fallback schedule) — then {seed, ids, seeks, temps, fallback},
        after refusing, each by name, what sampling does not run with."""
        req = self._sampling_request_unfiltered(temperature, kwargs, logits_processor)
        flt = self._sampling_filter(kwargs)
        if req is None:
            if flt != (0, 1.0, 0.0):
                given = [k for k in ("sampling_top_k", "sampling_top_p", "sampling_min_p") if kwargs.get(k) is not None]
                raise ValueError(f"{', '.join(given)} given on a call that does not sample: the filters belong to the engine's seeded sampling "
                                 "(sampling_seed= with a temperature > 0, do_sample=True or a temperature tuple)")
            return None
        req["filter"] = flt
        return req

    @staticmethod
    def _sampling_filter(kwargs) -> tuple:
        """(top_k, top_p, min_p) of ``sampling_top_k= / sampling_top_p= / sampling_min_p=`` (off: 0, 1.0, 0.0), refused in HF's words."""
        k, p, m = kwargs.get("sampling_top_k"), kwargs.get("sampling_top_p"), kwargs.get("sampling_min_p")
        if k is not None and (isinstance(k, bool) or not isinstance(k, (int, np.integer)) or int(k) < 0):
            raise ValueError(f"`sampling_top_k` has to be a non-negative integer (0: off), but is {k!r}")
        if p is not None and (isinstance(p, bool) or not isinstance(p, (int, float, np.floating)) or not 0.0 < float(p) <= 1.0):
            raise ValueError(f"`sampling_top_p` has to be a float > 0 and <= 1 (1: off), but is {p!r}")
        if m is not None and (isinstance(m, bool) or not isinstance(m, (int, float, np.floating)) or not 0.0 <= float(m) <= 1.0):
            raise ValueError(f"`sampling_min_p` has to be a float in the [0, 1] interval (0: off), but is {m!r}")
        return (0 if k is None else int(k), 1.0 if p is None else float(p), 0.0 if m is None else float(m))

    def _sampling_request_unfiltered(self, temperature, kwargs, logits_processor) -> Optional[dict]:
        seed = kwargs.get("sampling_seed")
        if seed is None:
            return None
        ladder = isinstance(temperature, (tuple, list))
        if ladder:
            temps = [float(t) for t in temperature]
        elif temperature is not None and float(temperature) > 0.0:
            temps = [float(temperature)]
        elif kwargs.get("do_sample"):
            temps = [1.0]
        else:
            return None
        if not temps or any(not np.isfinite(t) or t < 0.0 for t in temps):
            raise ValueError(f"`temperature` has to hold finite values >= 0, but is {temperature!r}")
        if kwargs.get("top_k") is not None or kwargs.get("top_p") is not None:
            raise NotImplementedError("top_k / top_p are not supported with sampling_seed: the engine samples softmax(logits / T) over the whole "
                                      "vocabulary (openai-whisper's Categorical; HF's default top_k=50 warper is not applied) unless its own filters "
                                      "are asked for: sampling_top_k= / sampling_top_p= / sampling_min_p= (DESIGN.md §2k), e.g. sampling_top_k=50")
        if self.config.is_tree:
            raise NotImplementedError("sampling (sampling_seed) is not supported with a candidate tree (medusa_choices with top-k > 1)")
        if _needs_host_processors(logits_processor):
            raise NotImplementedError("sampling (sampling_seed) is not supported on the host processor path (logits_processor=)")
        if kwargs.get("streamer") is not None:
            raise NotImplementedError("streamer= is not supported with sampling (sampling_seed): a fallback attempt would take streamed tokens back")
        if kwargs.get("chunk_longform"):
            raise NotImplementedError("chunk_longform is not supported with sampling (sampling_seed); use sequential_longform")
        ids = kwargs.get("sampling_stream_ids")
        return dict(seed=int(seed), ids=None if ids is None else [int(v) for v in ids], seeks=None, temps=temps, fallback=ladder)

    @staticmethod
    def sampling_stream_key(stream_id: int, seek_frames: int, attempt: int) -> int:
        """The 64-bit stream key of one decode attempt: key_lo = the stream id, key_hi = 16 * the window's seek (mel frames) + the attempt index."""
        return (int(stream_id) & 0xFFFFFFFF) | (((16 * int(seek_frames) + int(attempt)) & 0xFFFFFFFF) << 32)

    @staticmethod
    def _sampled_gp(gp: GenParams, T: float, seed: int, keys: List[int], flt: tuple = (0, 1.0, 0.0)) -> GenParams:
        """``gp`` for one sampled attempt: the engine's plain decode path with the (filtered) draw in place of the arg-max."""
        return replace(gp, vanilla=True, accept_mode=ACCEPT_GREEDY, temperature=0.0, sampling_temperature=float(T),
                       sampling_seed=int(seed), sampling_keys=list(keys), num_beams=1,     # (HF: a sampled retry runs with one beam)
                       sampling_top_k=int(flt[0]), sampling_top_p=float(flt[1]), sampling_min_p=float(flt[2]))

    # ---- beam search on the plain decode path (engine: csrc/wm_beam.hip) ------------------------------------------------------
    BEAM_MAX = 8

    def _beam_request(self, kwargs, temperature, logits_processor, stopping_criteria, side: bool) -> Optional[dict]:
        """The beam side of a generate() call: None for ``num_beams`` 1 / None; without ``vanilla=True`` the reference's exception (model.py:1153-1156);
        else {n, length_penalty, early_stopping, num_return_sequences} after refusing, each by name, what beam search does not run with."""
        nb = kwargs.get("num_beams", 1)
        if nb in (None, 1):
            return None
        if not kwargs.get("vanilla"):
            raise Exception("Beam search is not supported with medusa for now (vanilla=True selects the engine's beam search on the plain "
                            "decode path)")                                                 # model.py:1153-1156
        if isinstance(nb, bool) or not isinstance(nb, (int, np.integer)) or int(nb) < 1:
            raise ValueError(f"`num_beams` has to be an integer strictly greater than 0, but is {nb!r}")        # HF's own check
        n = int(nb)
        if n > self.BEAM_MAX:
            raise NotImplementedError(f"num_beams > {self.BEAM_MAX} is not supported by the engine's beam search (num_beams={n})")
        if kwargs.get("do_sample") or (not isinstance(temperature, (tuple, list)) and temperature is not None and float(temperature) > 0.0):
            raise NotImplementedError("do_sample with beams (beam-search multinomial sampling) is not supported; a tuple `temperature` with "
                                      "sampling_seed= runs the beam search at temperature 0 and the sampled retries with one beam")
        if self.config.is_tree:
            raise NotImplementedError("beam search is not supported with a candidate tree (medusa_choices with top-k > 1)")
        if logits_processor or stopping_criteria:
            raise NotImplementedError("beam search is not supported on the host processor path (logits_processor= / stopping_criteria=)")
        if kwargs.get("streamer") is not None:
            raise NotImplementedError("streamer= is not supported with beam search: a beam's tokens are not final until the search ends")
        if kwargs.get("chunk_longform") or kwargs.get("sequential_longform"):
            raise NotImplementedError("chunk_longform / sequential_longform are not supported with beam search (short-form only)")
        if self._micro_batches not in (None, 1):
            raise NotImplementedError("the micro-batch pool (set_micro_batches) is not supported with beam search: the beams of a clip share one context")
        lp = kwargs.get("length_penalty")
        lp = 1.0 if lp is None else float(lp)
        if not np.isfinite(lp):
            raise ValueError(f"`length_penalty` has to be a finite float, but is {lp}")
        es = kwargs.get("early_stopping")
        es = False if es is None else es
        if not (isinstance(es, bool) or es == "never"):
            raise ValueError(f"`early_stopping` must be a boolean or 'never', but is {es!r}")                  # HF's own check
        r = kwargs.get("num_return_sequences")
        r = 1 if r is None else int(r)
        if not 1 <= r <= n:
            raise ValueError(f"`num_return_sequences` ({r}) has to be in 1..`num_beams` ({n})")                 # HF's own check
        if r > 1 and side:
            raise NotImplementedError("num_return_sequences > 1 is not supported together with the requests that replay the final ids "
                                      "(token log-probabilities, thresholds, top_logprobs, return_token_timestamps): they score one row per clip")
        if n > self._max_batch:
            raise ValueError(f"num_beams={n} needs {n} streams per clip and the context holds max_batch={self._max_batch}: call set_max_batch({n}) "
                             "or more first")
        return dict(n=n, length_penalty=lp, early_stopping=es, num_return_sequences=r)

    # ---- sequence bias, bad words, hotwords on the plain decode path (engine: csrc/wm_seq_bias.hip) ----------------------------------
    def _bias_request(self, kwargs, samp, temperature, logits_processor, stopping_criteria, side: dict):
        """The bias side of a generate() call: None unless ``sequence_bias=``, ``bad_words_ids=`` or ``hotwords=`` is given; else the entries
        [(ids, bias), ..] — HF's two processors merged into one table, a sequence given both ways keeps -inf — after HF's own validation and after
        refusing, each by the argument's name, what the bias does not run with.  ``side``: name -> value of the requests that replay the final ids."""
        given = [n for n in ("sequence_bias", "bad_words_ids", "hotwords") if kwargs.get(n) is not None]
        if not given:
            if kwargs.get("hotword_boost") is not None:
                raise ValueError("`hotword_boost` needs `hotwords`")
            return None
        names = " / ".join(given)
        cfg = self.config
        merged: Dict[Tuple[int, ...], float] = {}
        if kwargs.get("sequence_bias") is not None:
            merged.update(sequence_bias_entries(kwargs["sequence_bias"], cfg.vocab_size))
        if kwargs.get("hotwords") is not None:
            tok = kwargs.get("tokenizer")
            if tok is None:
                proc = getattr(self, "processor", None)
                tok = getattr(proc, "tokenizer", None) or getattr(self, "tokenizer", None)
            boost = kwargs.get("hotword_boost")
            for ids, b in hotword_entries(kwargs["hotwords"], 2.0 if boost is None else boost, tok):
                if any(t < 0 or t >= cfg.vocab_size for t in ids):
                    raise ValueError(f"The model vocabulary size is {cfg.vocab_size}, but the following tokens were being biased: {list(ids)}")
                merged.setdefault(ids, b)            # (an explicit sequence_bias entry on the same sequence wins over the convenience)
        if kwargs.get("bad_words_ids") is not None:
            for ids, b in bad_words_entries(kwargs["bad_words_ids"], cfg.eos_token_id, cfg.vocab_size):
                merged[ids] = b                      # -inf wins
        entries = list(merged.items())
        plain = bool(kwargs.get("vanilla")) or (samp is not None and not samp["fallback"] and samp["temps"][0] > 0.0)
        if isinstance(temperature, (tuple, list)):
            raise NotImplementedError(f"{names} is not supported with a tuple `temperature` (the fallback schedule scores its attempts in a replay "
                                      "that does not know the bias)")
        if not plain:
            raise NotImplementedError(f"{names} runs on the plain decode path only: pass vanilla=True (the Medusa loop's select, candidate and "
                                      "accept kernels do not know the bias)")
        if cfg.is_tree:
            raise NotImplementedError(f"{names} is not supported with a candidate tree (medusa_choices with top-k > 1)")
        if _needs_host_processors(logits_processor) or \
                (stopping_criteria and any(type(c_).__name__ not in _LOWERABLE_CRITERIA for c_ in stopping_criteria)):
            raise NotImplementedError(f"{names} is not supported on the host processor path (logits_processor= / stopping_criteria=); pass HF's "
                                      "SequenceBiasLogitsProcessor there instead")
        if kwargs.get("streamer") is not None:
            raise NotImplementedError(f"{names} is not supported with streamer=")
        if kwargs.get("chunk_longform"):
            raise NotImplementedError(f"{names} is not supported with chunk_longform (short-form only)")
        if kwargs.get("sequential_longform"):
            raise NotImplementedError(f"{names} is not supported with sequential_longform (short-form only)")
        if self._micro_batches not in (None, 1):
            raise NotImplementedError(f"{names} is not supported with the micro-batch pool (set_micro_batches)")
        for n, v in side.items():
            if v is not None and v is not False:
                raise NotImplementedError(f"{names} is not supported together with {n}: it replays the final ids through kernels that do not "
                                          "know the bias")
        if len(entries) > _SEQ_BIAS_MAX:
            raise ValueError(f"{names}: {len(entries)} entries, the engine holds at most {_SEQ_BIAS_MAX} (WM_SEQ_BIAS_MAX)")
        long = [ids for ids, _ in entries if len(ids) > _SEQ_BIAS_MAX_LEN]
        if long:
            raise ValueError(f"{names}: a sequence of {len(long[0])} tokens, the engine holds at most {_SEQ_BIAS_MAX_LEN} per entry (WM_SEQ_BIAS_MAX_LEN)")
        bad = [ids for ids, b in entries if b == float("-inf") and len(ids) > 1 and ids[-1] == cfg.eos_token_id]
        if bad:
            raise ValueError(f"{names}: a banned sequence of more than one token ends in eos_token_id ({list(bad[0])}): under the exponential "
                             "decay HF's processors turn its -inf into NaN")
        if any(not np.isfinite(b) and b != float("-inf") for _, b in entries):
            raise ValueError(f"{names}: a bias has to be finite or -inf")
        return entries

    # ---- constrained decoding on the plain decode path (engine: csrc/wm_constraint.hip) -----------------------------------------------
    def _constraint_request(self, kwargs, samp, temperature, logits_processor, stopping_criteria, return_timestamps, side: dict):
        """The constraint side of a generate() call: None unless ``allowed_sequences=`` or ``allowed_phrases=`` is given; else the sequences —
        both merged in that order, duplicates collapsed — after their validation and after refusing, each by the argument's name, what the
        constraint does not run with.  ``side``: name -> value of the requests that replay the final ids."""
        given = [n for n in ("allowed_sequences", "allowed_phrases") if kwargs.get(n) is not None]
        if not given:
            return None
        names = " / ".join(given)
        cfg = self.config
        merged: Dict[Tuple[int, ...], None] = {}
        if kwargs.get("allowed_sequences") is not None:
            merged.update(dict.fromkeys(allowed_sequence_entries(kwargs["allowed_sequences"], cfg.eos_token_id, cfg.vocab_size)))
        if kwargs.get("allowed_phrases") is not None:
            tok = kwargs.get("tokenizer")
            if tok is None:
                proc = getattr(self, "processor", None)
                tok = getattr(proc, "tokenizer", None) or getattr(self, "tokenizer", None)
            phr = [list(q) for q in allowed_phrase_entries(kwargs["allowed_phrases"], tok)]
            merged.update(dict.fromkeys(allowed_sequence_entries(phr, cfg.eos_token_id, cfg.vocab_size)))
        seqs = list(merged)
        plain = bool(kwargs.get("vanilla")) or (samp is not None and not samp["fallback"] and samp["temps"][0] > 0.0)
        if isinstance(temperature, (tuple, list)):
            raise NotImplementedError(f"{names} is not supported with a tuple `temperature` (the fallback schedule scores its attempts in a replay "
                                      "that does not know the mask)")
        if not plain:
            raise NotImplementedError(f"{names} runs on the plain decode path only: pass vanilla=True (the Medusa loop's select, candidate and "
                                      "accept kernels do not know the mask)")
        if cfg.is_tree:
            raise NotImplementedError(f"{names} is not supported with a candidate tree (medusa_choices with top-k > 1)")
        if return_timestamps:
            raise NotImplementedError(f"{names} is not supported with return_timestamps=True (a timestamp is never in the allowed set: the "
                                      "timestamp rules would force a row of -inf)")
        if _needs_host_processors(logits_processor) or \
                (stopping_criteria and any(type(c_).__name__ not in _LOWERABLE_CRITERIA for c_ in stopping_criteria)):
            raise NotImplementedError(f"{names} is not supported on the host processor path (logits_processor= / stopping_criteria=); pass HF's "
                                      "PrefixConstrainedLogitsProcessor there instead")
        if kwargs.get("streamer") is not None:
            raise NotImplementedError(f"{names} is not supported with streamer=")
        if kwargs.get("chunk_longform"):
            raise NotImplementedError(f"{names} is not supported with chunk_longform (short-form only)")
        if kwargs.get("sequential_longform"):
            raise NotImplementedError(f"{names} is not supported with sequential_longform (short-form only)")
        if self._micro_batches not in (None, 1):
            raise NotImplementedError(f"{names} is not supported with the micro-batch pool (set_micro_batches)")
        for n, v in side.items():
            if v is not None and v is not False:
                raise NotImplementedError(f"{names} is not supported together with {n}: it replays the final ids through kernels that do not "
                                          "know the mask")
        if len(seqs) > _CONSTRAINT_MAX:
            raise ValueError(f"{names}: {len(seqs)} sequences, the engine holds at most {_CONSTRAINT_MAX} (WM_CONSTRAINT_MAX)")
        long = [q for q in seqs if len(q) > _CONSTRAINT_MAX_LEN]
        if long:
            raise ValueError(f"{names}: a sequence of {len(long[0])} tokens, the engine holds at most {_CONSTRAINT_MAX_LEN} per sequence "
                             "(WM_CONSTRAINT_MAX_LEN)")
        return seqs

    @staticmethod
    def _check_constraint_params(gp: GenParams) -> None:
        """What the constraint cannot run with once the decode's parameters are known (the engine refuses the same at wm_decode_begin)."""
        if gp.exp_decay is not None:
            raise ValueError("allowed_sequences / allowed_phrases cannot run with the exponential decay length penalty "
                             "(exponential_decay_length_penalty): on a masked eos HF's x + |x| p is NaN")
        used = {t for q in gp.allowed_sequences for t in q}
        sup = sorted(used & set(gp.suppress_tokens or []))
        if sup:
            raise ValueError(f"allowed_sequences / allowed_phrases: the token ids {sup} of the allowed sequences are in suppress_tokens")
        first = sorted({q[0] for q in gp.allowed_sequences} & set(gp.begin_suppress_tokens or []))
        if first:
            raise ValueError(f"allowed_sequences / allowed_phrases: the token ids {first} start an allowed sequence and are in begin_suppress_tokens")

    def _beam_decode(self, eng, feats, gp: GenParams, encoded: bool):
        """Beam search over the clips ``feats`` in groups of max_batch // num_beams, each group encoded and decoded in turn (B clips need
        B * num_beams streams).  Returns (every clip's best finished hypothesis, all of them — [(ids, score)] * num_beams per clip, best first —,
        the summed statistics).  Ends with ALL clips resident (one more encoder pass when there was more than one group), so that the
        requests that replay the final ids find the state an ordinary decode leaves."""
        B, n = feats.shape[0], int(gp.num_beams)
        per = max(eng.max_batch // n, 1)
        hyps, stats = [], None
        for lo in range(0, B, per):
            hi = min(B, lo + per)
            if not (encoded and lo == 0 and hi == B):
                eng.encode(feats if (lo == 0 and hi == B) else feats[lo:hi])
            eng.decode(gp.for_streams(range(lo, hi)), hi - lo)      # (per-stream prompts follow their clips into the group)
            hyps += [[eng.beam_result(c, k) for k in range(n)] for c in range(hi - lo)]
            st = eng.stats()
            if stats is None:
                stats = st
            else:
                for k in ("ms_decode", "ms_encode", "iterations", "iterations_launched", "tokens_emitted", "graph_replays"):
                    stats[k] += st[k]
        if per < B:
            eng.encode(feats)
        stats["beam_groups"] = -(-B // per)
        return [h[0][0] for h in hyps], hyps, stats

    def _decode_with_fallback(self, eng, feats, gp: GenParams, samp: dict, sc_req: Optional[dict], encoded: bool):
        """HF ``generate_with_fallback``: attempt i decodes the streams still flagged at temps[i] — 0: the configured path, > 0: the sampled plain
        decode —, scores them (the existing scoring pass, at temperature 1 on the processed rows, as HF's _retrieve_avg_logprobs undoes the
        temperature) and gates them.  A stream is final when it needs no fallback, was skipped by the no-speech gate, or the temperatures are
        exhausted (the last attempt is kept).  Flagged streams are re-encoded as a sub-batch.  Without thresholds nothing is ever flagged.
        Returns (seqs, infos or None, kept temperature, attempts per stream, ms of the scoring passes, the hypotheses of every clip whose
        temperature-0 attempt was a beam search, the summed statistics)."""
        B = feats.shape[0]
        ids = samp["ids"] if samp["ids"] is not None else list(range(B))
        seeks = samp["seeks"] if samp["seeks"] is not None else [0] * B
        if len(ids) != B or len(seeks) != B:
            raise ValueError(f"sampling_stream_ids needs one id per stream ({B}), got {len(ids)}")
        seqs, infos, kept, att = [None] * B, [None] * B, [0.0] * B, [0] * B
        todo, stats, ms_sc, n_dec = list(range(B)), None, 0.0, 0
        beams: Dict[int, list] = {}             # clip -> the hypotheses of its beam-search attempt (the temperature-0 attempt of a beam call)
        for i, T in enumerate(samp["temps"]):
            if len(todo) != B or not (encoded or i > 0):
                eng.encode(feats if len(todo) == B else feats[todo])        # (a rare path: one encoder pass over the flagged streams)
            gp_i = gp if T == 0.0 else self._sampled_gp(gp, T, samp["seed"], [self.sampling_stream_key(ids[b], seeks[b], i) for b in todo],
                                                             samp.get("filter", (0, 1.0, 0.0)))
            gp_i = gp_i.for_streams(todo)       # (per-stream prompts follow their streams into the sub-batch)
            if gp_i.num_beams > 1:      # HF generate_with_fallback: num_beams stays exactly when the attempt does not sample
                out, hyps, _ = self._beam_decode(eng, feats if len(todo) == B else feats[todo], gp_i, True)
                beams.update(zip(todo, hyps))
            else:
                out = eng.decode(gp_i, len(todo))
            n_dec += 1
            st = eng.stats()
            if stats is None:
                stats = st
            else:
                stats["ms_decode"] += st["ms_decode"]; stats["ms_encode"] += st["ms_encode"]
            inf = None
            if sc_req is not None:
                out, inf, ms = self._score_run(eng, out, gp_i, sc_req)
                ms_sc += ms
            for j, b in enumerate(todo):
                seqs[b], kept[b], att[b] = out[j], float(T), i + 1
                infos[b] = None if inf is None else inf[j]
            todo = [b for j, b in enumerate(todo) if inf is not None and inf[j]["needs_fallback"] and not inf[j]["skipped"]]
            if not todo:
                break
        stats["fallback_decodes"] = n_dec - 1
        return seqs, (infos if sc_req is not None else None), kept, att, ms_sc, beams, stats

    @torch.no_grad()
    def generate(self, input_features: Optional[torch.Tensor] = None, generation_config=None, logits_processor=None,
                 stopping_criteria=None, prefix_allowed_tokens_fn=None, synced_gpus: bool = False,
                 return_timestamps: Optional[bool] = None, task: Optional[str] = None, language: Optional[Union[str, Sequence[str]]] = None,
                 is_multilingual: Optional[bool] = None, prompt_ids: Optional[torch.Tensor] = None,
                 prompt_condition_type: Optional[str] = None, condition_on_prev_tokens: Optional[bool] = None,
                 temperature: Optional[Union[float, Tuple[float, ...]]] = None,
                 compression_ratio_threshold: Optional[float] = None, logprob_threshold: Optional[float] = None,
                 no_speech_threshold: Optional[float] = None, num_segment_frames: Optional[int] = None,
                 attention_mask: Optional[torch.Tensor] = None, time_precision: float = 0.02,
                 time_precision_features: float = 0.01, return_token_timestamps: Optional[bool] = None,
                 return_segments: bool = False, return_dict_in_generate: Optional[bool] = None,
                 force_unique_generate_call: Optional[bool] = None, return_token_logprobs: Optional[bool] = None,
                 top_logprobs: Optional[int] = None, **kwargs):
        """Same signature as the reference (model.py:1419-1449).  Returns ``LongTensor [B, T]`` holding the
        prompt + generated ids, right-padded with ``pad_token_id`` (model.py:1747-1762).

        ``return_token_logprobs=True`` returns a GenerateEncoderDecoderOutput with ``token_logprobs [B, T]``, ``avg_logprob``,
        ``compression_ratio`` and ``no_speech_prob``; ``no_speech_threshold`` / ``logprob_threshold`` / ``compression_ratio_threshold`` run the
        same scoring pass and gate on it (``skipped``, ``needs_fallback`` in the dict outputs and in ``self.last_scores``).

        ``top_logprobs=k`` (1..8) implies that pass and the dict output and adds the k best tokens of every scored row:
        ``top_token_ids [B, T, k]``, ``top_token_logprobs [B, T, k]`` (value descending, then id ascending) and ``token_ranks [B, T]``, the
        rank of the emitted id in its row (0: masked); -1 / -inf / 0 where nothing is scored.

        ``sequential_longform=True`` with ``return_timestamps=True``: ``input_features [B, n_mels, T]`` of any length — per-clip
        lengths from ``attention_mask [B, T]`` or ``num_frames=`` — are transcribed by Whisper's sequential long-form loop.

        ``chunk_longform=True, stride_length_s=s | (left, right)`` (the HF ASR pipeline's keyword): the windows of a long clip
        overlap by the strides and their token lists are stitched on the device by HF's ``_find_longest_common_sequence``; ``window_keep
        [B, n, 2]`` in the dict forms says which slice of every window's text was kept.  ``None``: the windows are cut at multiples of 30 s.

        ``return_word_timestamps=True, tokenizer=tok | word_table=WordTable`` (the HF ASR pipeline's ``return_timestamps="word"``):
        implies ``return_token_timestamps=True`` and adds ``words`` to the dict output — per clip a list of ``{"text", "timestamp": (start, end),
        "tokens": (first, stop)[, "probability"]}`` — grouped from the ids and the token timestamps by ONE HIP kernel launch per call, on every
        route on which token timestamps work; with ``return_segments=True`` every segment carries its own ``words``.

        ``language=[...]`` (HF ``language: str | list[str]``): one language per clip, decoded as ONE batch — one encoder pass, one
        decode, row b carrying clip b's language token.  ``language=None, group_by_language=False``: the languages are detected on the device
        (``Engine.detect_language``) and the batch is decoded from the same encoder pass, whatever the mix; the default ``True`` detects on the
        host and decodes every language group as a batch of its own."""
        if generation_config is not None:
            # HF semantics (model.py:936-943 -> GenerationMixin._prepare_generation_config): a copy of the passed config, updated by every
            # explicit argument of this call — an explicit argument wins, the config fills what the call leaves open.  Only the fields this
            # path reads are consulted; sampling has no Medusa path in the reference either (model.py:1128-1156).
            gc = generation_config

            def pick(name, cur):
                return cur if cur is not None else getattr(gc, name, None)
            return_timestamps = pick("return_timestamps", return_timestamps)
            task, language = pick("task", task), pick("language", language)
            no_speech_threshold = pick("no_speech_threshold", no_speech_threshold)
            logprob_threshold = pick("logprob_threshold", logprob_threshold)
            compression_ratio_threshold = pick("compression_ratio_threshold", compression_ratio_threshold)
            return_token_timestamps = pick("return_token_timestamps", return_token_timestamps)
            return_dict_in_generate = pick("return_dict_in_generate", return_dict_in_generate)
            for name in ("max_new_tokens", "max_length", "num_beams", "suppress_tokens", "begin_suppress_tokens",
                         "exponential_decay_length_penalty", "posterior_threshold", "posterior_alpha",
                         "repetition_penalty", "no_repeat_ngram_size", "num_return_sequences", "early_stopping"):
                if kwargs.get(name) is None and getattr(gc, name, None) is not None:
                    kwargs[name] = getattr(gc, name)
            if kwargs.get("do_sample") is None and getattr(gc, "do_sample", False):
                kwargs["do_sample"] = True
            # fields HF's _prepare_generation_config would apply and this path does not read: say so instead of ignoring them silently
            # (a value equal to the model's own generation config, or to HF's default, is not a request)
            own = getattr(self, "generation_config", None)
            ignored = []
            beam_call = bool(kwargs.get("vanilla")) and kwargs.get("num_beams") not in (None, 1)
            if beam_call and kwargs.get("length_penalty") is None and getattr(gc, "length_penalty", None) is not None:
                kwargs["length_penalty"] = gc.length_penalty        # (read by the engine's beam search, DESIGN.md §2i: not ignored there)
            for name, dflt in (("temperature", 1.0), ("eos_token_id", None), ("pad_token_id", None), ("forced_decoder_ids", None),
                               ("top_k", 50), ("top_p", 1.0),
                               ("length_penalty", 1.0), ("bad_words_ids", None), ("min_length", 0), ("min_new_tokens", None)):
                v = getattr(gc, name, None)
                if v is None or v == dflt or (own is not None and v == getattr(own, name, None)) or (beam_call and name == "length_penalty"):
                    continue
                ignored.append(name)
            if ignored:
                import warnings
                warnings.warn("generate(generation_config=...): the Medusa path does not honour " + ", ".join(ignored) +
                              " from a passed config (see INTEGRATION.md, 'generation_config fields'); pass processors / criteria explicitly",
                              UserWarning, stacklevel=2)
        # return_word_timestamps: the words of every clip with a start and an end, grouped on the device from the ids and the token
        # timestamps of whatever route decodes the call; it implies return_token_timestamps, whose refusals all stand
        words_req = self._words_request(kwargs, return_token_timestamps, return_token_logprobs)
        out = self._generate_routes(input_features, generation_config, logits_processor, stopping_criteria, prefix_allowed_tokens_fn,
                                    return_timestamps, task, language, prompt_ids, prompt_condition_type, condition_on_prev_tokens,
                                    temperature, compression_ratio_threshold, logprob_threshold, no_speech_threshold, attention_mask,
                                    time_precision, time_precision_features, True if words_req is not None else return_token_timestamps,
                                    return_segments, return_dict_in_generate, return_token_logprobs, top_logprobs, kwargs)
        return out if words_req is None else self._attach_words(out, words_req, language)

    def _generate_routes(self, input_features, generation_config, logits_processor, stopping_criteria, prefix_allowed_tokens_fn,
                         return_timestamps, task, language, prompt_ids, prompt_condition_type, condition_on_prev_tokens,
                         temperature, compression_ratio_threshold, logprob_threshold, no_speech_threshold, attention_mask,
                         time_precision, time_precision_features, return_token_timestamps, return_segments,
                         return_dict_in_generate, return_token_logprobs, top_logprobs, kwargs):
        """generate() behind its generation_config merge: the checks of every feature, the resolved call and the route that decodes it."""
        # vad_longform: speech windows cut at pauses; its refusals come first, each under its own message
        plan = self._check_vad(kwargs, top_logprobs)
        # stride_length_s: overlapping windows for chunk_longform, merged on the device; checked before every route's own refusals
        stride = None
        if kwargs.get("stride_length_s") is not None:
            if not kwargs.get("chunk_longform") or kwargs.get("sequential_longform"):
                raise ValueError("stride_length_s is only valid together with chunk_longform=True (overlapping windows of the chunked long-form "
                                 "route; sequential_longform seeks by timestamps and has no strides)")
            stride = self._stride_frames(kwargs["stride_length_s"])
            if return_timestamps:
                raise NotImplementedError("return_timestamps=True is not supported with stride_length_s: resolving strides by timestamp tokens is "
                                          "another algorithm than the token merge (use return_token_timestamps, or chunk_longform without strides)")
        # Seeded sampling / temperature fallback: opt-in through `sampling_seed=` — the random stream is the engine's own
        # counter-based one, not torch's generator; without it every refusal below stands as it always has
        samp = self._sampling_request(temperature, kwargs, logits_processor)
        if samp is None and kwargs.get("do_sample"):
            raise NotImplementedError("sampling (do_sample=True) is not supported with medusa; pass sampling_seed= for the engine's seeded "
                                      "sampling on the plain decode path")      # model.py:1128-1156: no Medusa branch
        # HF SequenceBiasLogitsProcessor / NoBadWordsLogitsProcessor (the reference's generate() builds neither): one in-place edit of the logits
        # row on the engine's plain decode path, before every other processor
        bias = self._bias_request(kwargs, samp, temperature, logits_processor, stopping_criteria,
                                  dict(return_token_logprobs=return_token_logprobs, top_logprobs=top_logprobs, no_speech_threshold=no_speech_threshold,
                                       logprob_threshold=logprob_threshold, compression_ratio_threshold=compression_ratio_threshold,
                                       return_token_timestamps=return_token_timestamps))
        if top_logprobs is not None:
            if isinstance(top_logprobs, bool) or not isinstance(top_logprobs, (int, np.integer)) or not 1 <= int(top_logprobs) <= _scores.TOPK_MAX:
                raise ValueError(f"`top_logprobs` has to be an integer in 1..{_scores.TOPK_MAX}, but is {top_logprobs!r}")
            if kwargs.get("sequential_longform") or kwargs.get("chunk_longform"):
                raise NotImplementedError("top_logprobs is not supported with chunk_longform / sequential_longform (short-form only)")
            top_logprobs = int(top_logprobs)
        if kwargs.get("sequential_longform"):
            self._check_sequential(return_timestamps, condition_on_prev_tokens, None if samp is not None else temperature,
                                   return_token_timestamps, logits_processor, stopping_criteria, kwargs.get("streamer"), prompt_ids,
                                   prompt_condition_type)
        # HF RepetitionPenaltyLogitsProcessor / NoRepeatNGramLogitsProcessor (GenerationMixin._get_logits_processor builds them from these two
        # fields; the reference's generate() drops both): inside the engine's select kernels, every row under its own prefix
        rep_pen, rep_g = kwargs.get("repetition_penalty"), kwargs.get("no_repeat_ngram_size")
        rep_pen = 1.0 if rep_pen is None else float(rep_pen)
        rep_g = 0 if rep_g is None else int(rep_g)
        if not (rep_pen > 0.0 and np.isfinite(rep_pen)):
            raise ValueError(f"`repetition_penalty` has to be a strictly positive float, but is {rep_pen}")        # HF's own check
        if rep_g < 0:
            raise ValueError(f"`no_repeat_ngram_size` has to be a positive integer or 0, but is {rep_g}")
        if rep_pen != 1.0 or rep_g != 0:
            if self.config.is_tree:
                raise NotImplementedError("repetition_penalty / no_repeat_ngram_size are not supported with a candidate tree "
                                          "(medusa_choices with top-k > 1)")
            if _needs_host_processors(logits_processor):
                raise NotImplementedError("repetition_penalty / no_repeat_ngram_size are not supported on the host processor path "
                                          "(logits_processor=); pass the HF processor objects there instead")
        if return_timestamps:
            # model.py:1171-1175 raises for every checkpoint; the engine runs HF's WhisperTimeStampLogitsProcessor in its decode loop
            #  where the vocabulary carries Whisper's timestamp block
            if not self.config.supports_timestamps:
                raise NotImplementedError("return_timestamps is not supported with medusa for this checkpoint: its vocabulary has no "
                                          "timestamp block (vocab_size - no_timestamps_token_id - 1 != max_source_positions + 1)")
            if self.config.is_tree:
                raise NotImplementedError("return_timestamps is not supported with a candidate tree (medusa_choices with top-k > 1)")
            if logits_processor or stopping_criteria:
                raise NotImplementedError("return_timestamps is not supported together with logits_processor= / stopping_criteria= "
                                          "(the host processor path)")
            return_timestamps = True
        # model.py:1201-1205 raises for no_speech_threshold and ignores the other two; the engine scores the final ids in a teacher-forced
        # replay whenever one of these arguments is given — none of them: no new launch
        sc_req = None
        if return_token_logprobs or top_logprobs is not None or no_speech_threshold is not None or logprob_threshold is not None \
                or compression_ratio_threshold is not None:
            if no_speech_threshold is not None and self.config.no_speech_token_id is None:
                raise NotImplementedError("no_speech_threshold needs a <|nospeech|> token (no_timestamps_token_id - 1) inside the vocabulary")
            if no_speech_threshold is not None and self._engine is None:
                # the reference's refusal (model.py:1201-1205) stays where nothing can score the clip: the detection is the engine's scoring pass
                raise NotImplementedError("no_speech_detection is not supported with medusa without the HIP engine's scoring pass: "
                                          "call model.to('cuda') first (no_speech_threshold)")
            if _needs_host_processors(logits_processor):
                raise NotImplementedError(("top_logprobs / " if top_logprobs is not None else "") +
                                          "token log-probabilities / quality gating are not supported on the host processor path (logits_processor=)")
            sc_req = dict(want=bool(return_token_logprobs) or top_logprobs is not None, no_speech_threshold=no_speech_threshold,
                          logprob_threshold=logprob_threshold, compression_ratio_threshold=compression_ratio_threshold, top_k=top_logprobs)
        # model.py:1153-1156 raises for num_beams > 1; with vanilla=True the engine runs HF's _beam_search on its plain decode path
        beam = self._beam_request(kwargs, temperature, logits_processor, stopping_criteria,
                                  side=sc_req is not None or bool(return_token_timestamps))
        if prefix_allowed_tokens_fn:
            raise NotImplementedError("prefix_allowed_tokens_fn is not supported by the HIP engine (a Python callback cannot run in its decode "
                                      "loop); for a fixed list of token sequences pass allowed_sequences= / allowed_phrases= with vanilla=True")
        # HF PrefixConstrainedLogitsProcessor over a fixed list of sequences: one in-place mask of the logits row on the engine's plain decode
        # path, right behind the sequence bias
        cons = self._constraint_request(kwargs, samp, temperature, logits_processor, stopping_criteria, return_timestamps,
                                        dict(return_token_logprobs=return_token_logprobs, top_logprobs=top_logprobs,
                                             no_speech_threshold=no_speech_threshold, logprob_threshold=logprob_threshold,
                                             compression_ratio_threshold=compression_ratio_threshold,
                                             return_token_timestamps=return_token_timestamps))
        tt_req = None
        if return_token_timestamps:
            # HF WhisperGenerationMixin.generate -> _extract_token_timestamps (the reference raises); the engine replays the final ids and
            # aligns them on the GPU
            tt_req = self._token_ts_request(kwargs.get("alignment_heads"), generation_config, kwargs.get("num_frames"), logits_processor,
                                            time_precision)
        if input_features is None:
            raise ValueError("input_features is required")
        if input_features.dim() != 3:
            raise ValueError("input_features must be [B, n_mels, frames]")
        # language=[...]: one language per clip (HF `language: str | list[str]`, _retrieve_init_tokens).  The entries become language
        # token strings; the long-form loops below take them as one language per recording, the short-form path as per-stream prompts of one length
        # (generate_from_wav with stride_length_s hands in the windows of all recordings, cut in the sample domain, and how many each one owns)
        counts = kwargs.get("_window_counts") if stride is not None else None
        if isinstance(language, (list, tuple)):
            language = self._language_list(language, len(plan["windows"]) if plan is not None else
                                           input_features.shape[0] if counts is None else len(counts))
            if not self.config.is_multilingual:
                language = None                         # ignored, as a scalar is (the prompt has no language slot)
        call = ResolvedCall(samp=samp, bias=bias, cons=cons, beam=beam, sc_req=sc_req, tt_req=tt_req, rep_pen=rep_pen, rep_g=rep_g,
                            return_timestamps=bool(return_timestamps), time_precision=time_precision, task=task, prompt_ids=prompt_ids,
                            temperature=temperature, logits_processor=logits_processor, stopping_criteria=stopping_criteria,
                            return_dict_in_generate=return_dict_in_generate, return_segments=return_segments, opts=kwargs)
        # the route: every one of them decodes its <= 30 s windows through _generate_short
        detect = bool(language is None and self.config.is_multilingual and kwargs.get("detect_language", True))
        if kwargs.get("sequential_longform"):
            return self._generate_sequential(input_features, attention_mask, call, language, detect, time_precision_features)
        if plan is not None:
            return self._generate_vad(input_features, plan, call, language, detect)
        if counts is not None:
            return self._generate_strided(input_features, [int(c) for c in counts], stride, call, language, detect)
        if input_features.shape[-1] > self.config.n_mel_frames:
            if not kwargs.get("chunk_longform"):
                raise NotImplementedError("Longform generation is not supported yet")              # model.py:1213-1214
            if stride is not None:
                win, counts = self._strided_feature_windows(input_features, stride)
                return self._generate_strided(win, counts, stride, call, language, detect)
            return self._generate_longform(input_features, call, language, detect)
        if detect and input_features.shape[0] >= 1 and kwargs.get("group_by_language", True) is False:
            # group_by_language=False: encode, detect on the device, then decode from the encoder pass that is resident — one
            # encode, one decode, whatever the mix of languages
            language = self._detect_language_on_device(input_features.to(self.device, torch.float32).contiguous())
            self.detected_languages = list(language)
            self._clip_languages = list(language)
            res = self._generate_short(input_features, call, language=language, encoded=True)
        elif detect and input_features.shape[0] >= 1:
            return self._generate_detecting_language(input_features, call)
        else:
            res = self._generate_short(input_features, call, language=language)
        out = self._outputs(res.seqs, res.gp, return_dict_in_generate, return_segments, res.token_timestamps, res.scores)
        if isinstance(out, dict):
            if res.fallback is not None and res.scores is None:
                out.update(res.fallback)
            if res.sequences_scores is not None:
                out["sequences_scores"] = res.sequences_scores
        return self._publish(res, out)

    # ---- word timestamps (HF pipeline return_timestamps="word"; engine: csrc/wm_words.hip) ------------------------------------
    def _words_request(self, kwargs, return_token_timestamps, return_token_logprobs) -> Optional[dict]:
        """``return_word_timestamps=True[, tokenizer=, word_table=]`` of a generate() call; takes its own two keywords out of ``kwargs``."""
        want, table = kwargs.pop("return_word_timestamps", None), kwargs.pop("word_table", None)
        if not want:
            return None
        if return_token_timestamps is not None and not return_token_timestamps:
            raise ValueError("return_word_timestamps=True is built on the token timestamps: return_token_timestamps=False contradicts it")
        tok = kwargs.get("tokenizer")
        if table is None and tok is None:
            raise ValueError("return_word_timestamps=True needs the bytes of the vocabulary: pass tokenizer= (or word_table=)")
        if table is None:
            cache = self.__dict__.setdefault("_word_tables", {})
            if id(tok) not in cache:
                cache[id(tok)] = (tok, _words.WordTable.from_tokenizer(tok, self.config.eos_token_id))     # (the tokenizer stays alive with its key)
            table = cache[id(tok)][1]
        self._clip_languages = None
        return dict(table=table, logprobs=bool(return_token_logprobs))

    def _attach_words(self, out, req: dict, language):
        """``out["words"]`` (and ``segments[b][k]["words"]``) of a finished call: ONE ``engine.word_spans`` call over the text rows of all clips."""
        cfg, eng, table = self.config, self.engine, req["table"]
        if getattr(eng, "_word_table", None) is not table:
            eng.set_word_table(table.blob, table.offsets)
            eng._word_table = table
        seqs = out["sequences"].cpu().tolist()
        langs = self._clip_languages
        if langs is None:
            langs = list(language) if isinstance(language, (list, tuple)) else [language] * len(seqs)
        per = len(seqs) // max(len(langs), 1)                  # (beam search with num_return_sequences: rows per clip, clip-major)
        modes = [_words.language_mode(langs[b // max(per, 1)] if cfg.is_multilingual else None) for b in range(len(seqs))]
        lp = out["token_logprobs"].float().cpu().numpy() if req["logprobs"] and "token_logprobs" in out else None
        P = len(self._last_prompt)
        words = _words.collate(eng, table, seqs, out["token_timestamps"].float().cpu().numpy(), P, cfg.eos_token_id, modes, lp)
        out["words"] = words
        if "segments" in out and out["segments"] is not None:
            for b, segs in enumerate(out["segments"]):
                o = P
                for sg in segs:
                    n = int(sg["tokens"].numel())
                    sg["words"] = [w for w in words[b] if o <= w["tokens"][0] < o + n]
                    o += n
        self.last_stats["ms_words"] = float(getattr(eng, "last_words_ms", 0.0))
        return out

    def _publish(self, res: "ShortResult", out):
        """The attributes a public call leaves behind, from the (last) short-form result of its route; hands ``out`` through."""
        self._last_prompt = list(res.gp.prompt)         # (per-stream prompts, gp.prompts, have this one's length: the representative row)
        self.last_stats = res.stats
        if res.fallback is not None:
            self.last_fallback, self._fallback_beams = res.fallback, res.fallback_beams
        if res.sequences_scores is not None:
            self.last_sequences_scores = res.sequences_scores
        return out

    def _generate_short(self, input_features, call: "ResolvedCall", *, language, encoded: bool = False, stream_ids=None, seeks=None,
                        num_frames=None) -> "ShortResult":
        """Decode one batch of <= 30 s windows under the resolved call: what all four routes of generate() come down to.  ``language``: a
        language token string / None, or one per clip (per-stream prompts).  ``encoded``: the caller has just encoded exactly this batch on the
        model's own engine (language detection) — the decode starts from that pass while it is still resident.  ``stream_ids`` / ``seeks``: the
        seeded sampling's stream keys follow their clips (global ids, the window's seek); ``num_frames``: likewise for the token timestamps.
        Checks that depend on the batch live here; the call's arguments were checked once, in generate()."""
        opts, samp, beam, bias, sc_req, tt_req = call.opts, call.samp, call.beam, call.bias, call.sc_req, call.tt_req
        if tt_req is not None and num_frames is not None:
            tt_req = dict(tt_req, num_frames=num_frames)
        if samp is not None and (stream_ids is not None or seeks is not None):
            samp = dict(samp, ids=stream_ids, seeks=seeks)
        lang_list, streamer = isinstance(language, (list, tuple)), opts.get("streamer")
        B = input_features.shape[0]
        if lang_list and streamer is not None:
            raise NotImplementedError("language=[...] / group_by_language=False (one language per clip) is not supported with streamer= "
                                      "(the streaming path is built around a single prompt)")
        if B > self._max_batch:
            self.set_max_batch(B)
        if beam is not None and beam["n"] > self._max_batch:        # (a wrapper may have resized the context since the request was read)
            raise ValueError(f"num_beams={beam['n']} exceeds max_batch={self._max_batch}: call set_max_batch first")
        temperature = call.temperature
        gp = self._gen_params(language, call.task, opts.get("exponential_decay_length_penalty"),
                              opts.get("max_new_tokens"), opts.get("max_length"),
                              # (sampling: attempt 0 of a fallback schedule at temperature 0 is today's call with that tuple — exact-match
                              # acceptance —, every sampled attempt derives its own parameters from these: _sampled_gp)
                              (0.0 if samp["temps"][0] == 0.0 else None) if samp is not None else
                              temperature if not isinstance(temperature, (tuple, list)) else temperature[0],
                              opts.get("vanilla", False), opts.get("posterior_threshold"),
                              opts.get("posterior_alpha"), opts.get("suppress_tokens"),
                              opts.get("begin_suppress_tokens"), call.prompt_ids, timestamps=call.return_timestamps,
                              repetition_penalty=call.rep_pen, no_repeat_ngram_size=call.rep_g)
        gp._time_precision = float(call.time_precision)
        if beam is not None:
            gp.num_beams, gp.length_penalty, gp.early_stopping = beam["n"], beam["length_penalty"], beam["early_stopping"]
        if bias is not None:
            gp.sequence_bias = bias
        if call.logits_processor or call.stopping_criteria:
            gp = lower_processors(gp, call.logits_processor, call.stopping_criteria)
        if call.cons is not None:
            gp.allowed_sequences = call.cons
            self._check_constraint_params(gp)
        host_crit = gp._host_criteria
        on_host = bool(host_crit or gp._host_processors)
        if lang_list and on_host:
            raise NotImplementedError("language=[...] / group_by_language=False (one language per clip) is not supported on the host processor path "
                                      "(logits_processor= / stopping_criteria= that the engine cannot lower: it is built around a single prompt)")
        feats = input_features.to(self.device, torch.float32).contiguous()
        n_ctx = self._micro_batches_for(B) if (streamer is None and not on_host) else 1
        # language detection has just encoded exactly this batch on the model's own engine (one language group, same order): its encoder
        # output and cross-K/V are still resident — decoding there saves the pool's second encoder pass over the same clips (the automatic
        # policy's gain at 2-3 clips is smaller than an encoder pass), and the decode below starts from it instead of encoding again
        resident = encoded and getattr(self._engine, "_B", None) == B
        if self._micro_batches is None and resident:
            n_ctx = 1
        if samp is not None:
            if on_host:
                raise NotImplementedError("sampling (sampling_seed) is not supported on the host processor path (logits_processor= / "
                                          "stopping_criteria= that the engine cannot lower)")
            n_ctx = 1           # the model's own engine: the micro-batch pool is not taught sampling
        if beam is not None or bias is not None or call.cons is not None:
            n_ctx = 1           # ... nor beams (the beams of a clip share one context), nor the sequence bias, nor the constraint
        if n_ctx > 1 and B >= 2:
            pool = self._get_pool(n_ctx)
            extra = {}
            if tt_req is not None:
                extra["token_ts"] = lambda e, sq, lo: self._token_ts_run(e, sq, gp.for_streams(range(lo, lo + len(sq))), tt_req, lo)   # noqa: E731
            if sc_req is not None:
                extra["score"] = lambda e, sq, lo: self._score_run(e, sq, gp.for_streams(range(lo, lo + len(sq))), sc_req)    # noqa: E731
            seqs = pool.run(feats, gp, **extra)      # F1..F14 per micro-batch, concurrently
            tt = _ts_tensor(pool.last_token_timestamps).to(self.device) if tt_req is not None else None
            sc = self._score_pack(pool.last_scores, seqs, gp, sc_req) if sc_req is not None else None
            return ShortResult(seqs, gp, pool.last_stats, tt, sc)
        eng = self.engine
        if streamer is not None and B != 1:
            raise ValueError("streamer only supports batch size 1")        # HF streamers are batch-1
        if gp._host_processors:
            if gp.repeat_rules:
                raise NotImplementedError("repetition_penalty / no_repeat_ngram_size are not supported on the host processor path "
                                          "(logits_processor=); pass the HF processor objects there instead")
            if tt_req is not None:
                raise NotImplementedError("return_token_timestamps is not supported on the host processor path (logits_processor=)")
            if sc_req is not None:
                raise NotImplementedError(("top_logprobs / " if sc_req.get("top_k") else "") +
                                          "token log-probabilities / quality gating are not supported on the host processor path (logits_processor=)")
            seqs, stats = self._decode_host_processors(feats, gp, streamer, host_crit)
            return ShortResult(seqs, gp, stats)
        # (beam search over more clips than max_batch // num_beams encodes group by group: _beam_decode)
        if samp is None and not resident and not (beam is not None and B * beam["n"] > eng.max_batch):
            eng.encode(feats)                                               # F1 + F2
        if samp is not None:
            seqs, infos, kept, att, ms, beams, stats = self._decode_with_fallback(eng, feats, gp, samp, sc_req, resident)
            fb = dict(fallback_temperature=torch.tensor(kept, dtype=torch.float32, device=self.device),
                      fallback_attempts=torch.tensor(att, dtype=torch.long, device=self.device))
            sc = None
            if sc_req is not None:
                stats["ms_token_logprobs"] = ms
                sc = dict(self._score_pack(infos, seqs, gp, sc_req), **fb)
            tt = None
            if tt_req is not None:
                if getattr(eng, "_B", None) != B:       # the last attempt left a sub-batch resident
                    eng.encode(feats)
                rows, ms = self._token_ts_run(eng, seqs, gp, tt_req, 0)
                stats["ms_token_timestamps"] = ms
                tt = _ts_tensor(rows).to(self.device)
            ss = None
            if beam is not None:
                # the score of a clip whose kept attempt is the beam search; NaN where a sampled retry was kept
                ss = torch.tensor([beams[b][0][1] if (kept[b] == 0.0 and b in beams) else float("nan") for b in range(B)],
                                  dtype=torch.float32, device=self.device)
            return ShortResult(seqs, gp, stats, tt, sc, ss, fb, beams)
        hyps = None
        if streamer is not None or host_crit:
            # one iteration per engine call: the streamer gets the tokens of every iteration (model.py:1034-1035 prompt, :758-759
            # tokens, :795-796 end); stopping criteria that are not static length / EOS rules are asked after every iteration with
            # the ids emitted so far (model.py:786) — a stream they stop keeps its ids up to that iteration
            cur = [list(gp.prompt) for _ in range(B)]
            stop_len: List[Optional[int]] = [None] * B
            if streamer is not None:
                streamer.put(torch.tensor([gp.prompt], dtype=torch.long))

            K = self.config.medusa_num_heads

            def over(b):
                # stopped by a criterion, or finished by the engine's own rules (EOS emitted / length limits, model.py:774-793).  NOT "the
                # stream emitted nothing": with several streams a step may be a stream's base pass (merged-step schedule), which emits nothing
                if stop_len[b] is not None:
                    return True
                gen = cur[b][len(gp.prompt):]
                return gp.eos_token_id in gen or len(cur[b]) >= gp.max_length or len(cur[b]) + K >= gp.hard_max_length

            def on_it(new):
                for b in range(B):
                    if stop_len[b] is not None or not new[b]:
                        continue
                    cur[b].extend(new[b])
                    if streamer is not None:
                        streamer.put(torch.tensor(new[b], dtype=torch.long))
                    ids_b = torch.tensor([cur[b]], dtype=torch.long)
                    if host_crit and any(bool(torch.as_tensor(c(ids_b, None)).all()) for c in host_crit):
                        stop_len[b] = len(cur[b])
                return bool(host_crit) and all(over(b) for b in range(B))     # True ends the run (every stream stopped or finished)

            seqs = eng.decode(gp, B, on_iteration=on_it)
            seqs = [s_[: stop_len[b]] if stop_len[b] is not None else s_ for b, s_ in enumerate(seqs)]
            if streamer is not None:
                streamer.end()
        elif beam is not None:
            seqs, hyps, stats = self._beam_decode(eng, feats, gp, True)    # (encoded above; more than one group encodes again)
        else:
            seqs = eng.decode(gp, B)                                        # F3..F14
        if hyps is None:
            stats = eng.stats()
        sc = None
        if sc_req is not None:
            # scoring first: a skipped clip's row becomes prompt + EOS before anything else looks at it (two replays when token timestamps
            # are asked for in the same call)
            seqs, infos, ms = self._score_run(eng, seqs, gp, sc_req)
            stats["ms_token_logprobs"] = ms
            sc = self._score_pack(infos, seqs, gp, sc_req)
        tt = None
        if tt_req is not None:
            rows, ms = self._token_ts_run(eng, seqs, gp, tt_req, 0)
            stats["ms_token_timestamps"] = ms
            tt = _ts_tensor(rows).to(self.device)
        ss = None
        if hyps is not None:
            # HF: `sequences` [B * num_return_sequences, T], clip-major and best first, and `sequences_scores` with return_dict_in_generate
            r = beam["num_return_sequences"]
            seqs = [h[k][0] for h in hyps for k in range(r)] if r > 1 else seqs
            ss = torch.tensor([h[k][1] for h in hyps for k in range(r)], dtype=torch.float32, device=self.device)
        return ShortResult(seqs, gp, stats, tt, sc, ss)

    # ---- token log-probabilities, no-speech probability, quality gating (engine: csrc/wm_score.hip) --------------------------
    def _score_run(self, eng, seqs, gp: GenParams, req: dict):
        """Scores of the streams ``seqs`` an engine context has just decoded -> (seqs with every skipped stream replaced by prompt + EOS,
        one info dict per stream, ms)."""
        cfg = self.config
        own = [self._own_end(s, gp) for s in seqs]
        P = len(gp.prompt)
        ns_id = cfg.no_speech_token_id
        # <|startoftranscript|> sits behind the prompt_ids: index len(prompt_ids) (HF's WhisperNoSpeechDetection reads index 0 there)
        sot = P - gp.begin_index if gp.begin_suppress_index is not None else 0
        k = req.get("top_k")
        if k:       # token alternatives: the same launches plus the top-k kernels; never without the argument
            lp, nsp, tid, tlp, rk, ms = eng.score_tokens_topk(own, P, gp, k, ns_id, sot)
        else:
            lp, nsp, ms = eng.score_tokens(own, P, gp, ns_id, sot)
        infos, out = [], []
        for b, s in enumerate(own):
            row = lp[b, : len(s)].copy()
            avg = _scores.avg_logprob(row, P, len(s))
            cr = _scores.compression_ratio(s[P:], cfg.vocab_size)
            ns = None if nsp is None else float(nsp[b])
            fb, skip = _scores.gate(ns, avg, cr, req["no_speech_threshold"], req["logprob_threshold"], req["compression_ratio_threshold"])
            if skip:
                s = list(gp.prompt_of(b)) + [gp.eos_token_id]       # (its own prompt: per-stream prompts)
                row = np.zeros(len(s), dtype=np.float32)
            infos.append(dict(token_logprobs=row, avg_logprob=avg, compression_ratio=cr, no_speech_prob=ns, skipped=skip, needs_fallback=fb))
            if k:
                n = len(s)
                if skip:    # a gated stream is prompt + EOS: nothing of it was scored
                    alt = _scores.topk_fills(n, k)
                else:
                    alt = (np.array(tid[b, :n], dtype=np.int64), np.array(tlp[b, :n], dtype=np.float32), np.array(rk[b, :n], dtype=np.int64))
                infos[-1].update(top_token_ids=alt[0], top_token_logprobs=alt[1], token_ranks=alt[2])
            out.append(s if skip else seqs[b])
        return out, infos, ms

    def _score_pack(self, infos, seqs, gp: GenParams, req: dict) -> dict:
        """Per-stream infos -> the tensors of the dict output, next to _pad's ids (token_logprobs is 0 after a stream's end)."""
        T = max(len(self._own_end(s, gp)) for s in seqs)
        sc = dict(token_logprobs=_lp_tensor([f["token_logprobs"] for f in infos], T).to(self.device),
                  avg_logprob=torch.tensor([f["avg_logprob"] for f in infos], dtype=torch.float32, device=self.device),
                  compression_ratio=torch.tensor([f["compression_ratio"] for f in infos], dtype=torch.float32, device=self.device),
                  # the streams' own ends (EOS included): with pad == eos a padded row alone cannot tell a stream's EOS from its padding
                  lengths=torch.tensor([len(self._own_end(s, gp)) for s in seqs], dtype=torch.long, device=self.device))
        if req.get("top_k"):
            sc.update(self._topk_stack([{k_: torch.from_numpy(np.asarray(f[k_])) for k_ in _scores.TOPK_FIELDS} for f in infos], T))
        if all(f["no_speech_prob"] is not None for f in infos):
            sc["no_speech_prob"] = torch.tensor([f["no_speech_prob"] for f in infos], dtype=torch.float32, device=self.device)
        if req["no_speech_threshold"] is not None:
            sc["skipped"] = torch.tensor([f["skipped"] for f in infos], dtype=torch.bool, device=self.device)
        if req["logprob_threshold"] is not None or req["compression_ratio_threshold"] is not None:
            sc["needs_fallback"] = torch.tensor([f["needs_fallback"] for f in infos], dtype=torch.bool, device=self.device)
        sc["_want"] = req["want"]
        return sc

    def _topk_stack(self, rows, T: int) -> dict:
        """Per-stream alternative fields (``top_token_ids [n, k]``, ``top_token_logprobs [n, k]``, ``token_ranks [n]``) -> tensors over T positions,
        -1 / -inf / 0 behind every stream's end."""
        k = int(rows[0]["top_token_ids"].shape[-1])
        ids, lps, rks = _scores.topk_fills(T, k)
        out = dict(top_token_ids=torch.from_numpy(ids).repeat(len(rows), 1, 1), top_token_logprobs=torch.from_numpy(lps).repeat(len(rows), 1, 1),
                   token_ranks=torch.from_numpy(rks).repeat(len(rows), 1))
        for i, f in enumerate(rows):
            for name in _scores.TOPK_FIELDS:
                v = f[name].cpu()
                out[name][i, : v.shape[0]] = v.to(out[name].dtype)
        return {name: v.to(self.device) for name, v in out.items()}

    # ---- token-level timestamps (HF _extract_token_timestamps; engine: csrc/wm_align.hip) ----------------------------------------------
    def _token_ts_request(self, alignment_heads, generation_config, num_frames, logits_processor, time_precision) -> dict:
        heads = alignment_heads
        if heads is None and generation_config is not None:
            heads = getattr(generation_config, "alignment_heads", None)
        if heads is None:
            heads = self.config.alignment_heads
        if heads is None:
            # HF raises ValueError here; the class is the one this path has always raised for token timestamps
            raise NotImplementedError("token timestamps need alignment heads and this checkpoint has no `alignment_heads` in its generation "
                                      "config: pass generate(alignment_heads=[[layer, head], ..])")
        heads = self.config.check_alignment_heads(heads)
        if logits_processor:
            raise NotImplementedError("return_token_timestamps is not supported together with logits_processor= (the host processor path)")
        if num_frames is not None and not isinstance(num_frames, int):
            num_frames = [int(v) for v in (num_frames.tolist() if hasattr(num_frames, "tolist") else num_frames)]
        return dict(heads=heads, width=int(self.config.median_filter_width), num_frames=num_frames, time_precision=float(time_precision))

    @staticmethod
    def _own_end(s: List[int], gp: GenParams) -> List[int]:
        """The stream's ids up to and including its first generated EOS (what _pad keeps)."""
        P = len(gp.prompt)
        return s[: s.index(gp.eos_token_id, P) + 1] if gp.eos_token_id in s[P:] else s

    def _token_ts_run(self, eng, seqs, gp: GenParams, req: dict, lo: int):
        """Token timestamps of the streams ``seqs`` an engine context has just decoded (streams lo .. of the batch) -> (rows, ms)."""
        own = [self._own_end(s, gp) for s in seqs]
        nf = req["num_frames"]
        if isinstance(nf, list):
            nf = nf[lo: lo + len(own)]
        out, ms = eng.token_timestamps(own, len(gp.prompt), req["heads"], req["width"], req["time_precision"], nf)
        return [out[b, : len(s)].copy() for b, s in enumerate(own)], ms

    # ---- arbitrary logits processors: the reference's loop with the passes on the engine --------------------------------------------
    @staticmethod
    def _static_processors(scores: torch.Tensor, cur_len: int, gp: GenParams) -> torch.Tensor:
        """The processors the engine fuses into its select kernels, in torch, for the host path: HF's ExponentialDecayLengthPenalty,
        SuppressTokensAtBeginLogitsProcessor, SuppressTokensLogitsProcessor on rows ``scores [R, V]``; every row sees the same
        ``cur_len = input_ids.shape[-1]`` (model.py:653-665, :689-694)."""
        s_ = scores.clone()
        if gp.exp_decay is not None:
            start = int(gp.exp_decay[0]) + len(gp.prompt)
            if cur_len > start:
                e = gp.eos_token_id
                s_[:, e] = s_[:, e] + s_[:, e].abs() * (pow(float(gp.exp_decay[1]), cur_len - start) - 1.0)
        if gp.begin_suppress_tokens and cur_len == gp.begin_index:
            s_[:, list(gp.begin_suppress_tokens)] = -float("inf")
        if gp.suppress_tokens:
            s_[:, list(gp.suppress_tokens)] = -float("inf")
        return s_

    @staticmethod
    def _accept_length(v: torch.Tensor, cand: torch.Tensor, gp: GenParams) -> int:
        """evaluate_posterior for one candidate chain (medusa_utils.py:526-588): exact match at temperature 0 (:547-560), typical
        acceptance otherwise (:562-577: p_c > min(threshold, alpha exp(-H)), H = -sum p log(p + 1e-5)); the number of leading accepts."""
        if gp.accept_mode == ACCEPT_GREEDY or not gp.temperature:
            ok = cand[1:] == torch.argmax(v[:-1], dim=-1)
        else:
            p = torch.softmax(v[:-1] / gp.temperature, dim=-1)
            p_c = torch.gather(p, -1, cand[1:].unsqueeze(-1)).squeeze(-1)
            H = -torch.sum(p * torch.log(p + 1e-5), dim=-1)
            ok = p_c > torch.minimum(torch.full_like(H, gp.posterior_threshold), torch.exp(-H) * gp.posterior_alpha)
        return int(torch.cumprod(ok.int(), dim=0).sum().item())

    def _decode_host_processors(self, feats: torch.Tensor, gp: GenParams, streamer=None, host_crit=None) -> Tuple[List[List[int]], dict]:
        """generate() with logits processors that are arbitrary Python callables (the reference hands ANY list to HF's machinery,
        model.py:1106-1116, and calls it on the base / Medusa logits and on the verify logits, :653-665, :689-694).  The engine's fused
        loop never lets logits leave the device, so this path runs the reference's loop structure (model.py:634-793) on the host, one
        stream at a time (the reference asserts batch 1), with every decoder pass on the engine (`wm_forward_logits`: K/V rows appended
        to the contiguous cache at the pass's position; rejected rows are overwritten by the next pass) and everything that touches
        logits — the static processors, the caller's processors, arg-max candidates, the posterior — in torch.  Same tokens as the fused
        loop wherever the caller's processors are pure functions of (ids, logits); orders of magnitude slower: it exists for API
        completeness, not for throughput.  Candidate chains only."""
        cfg, eng = self.config, self.engine
        if cfg.is_tree:
            raise NotImplementedError("custom logits processors with a candidate tree (medusa_choices with top-k > 1) are not supported")
        if gp.vanilla:
            raise NotImplementedError("custom logits processors with vanilla=True are not supported")
        procs = list(gp._host_processors)
        K, P, eos = cfg.medusa_num_heads, len(gp.prompt), gp.eos_token_id

        def run(ids_t: torch.Tensor, scores: torch.Tensor) -> torch.Tensor:
            out = self._static_processors(scores, ids_t.shape[-1], gp)
            for pr in procs:
                out = pr(ids_t, out)
            return out

        def engine_pass(tokens: List[int], pos0: int, disable_medusa: bool) -> torch.Tensor:       # [n_out, T, V]
            if len(tokens) <= 16:
                return eng.forward_logits([tokens], pos0, disable_medusa)[:, 0]
            return torch.cat([eng.forward_logits([tokens[c: c + 16]], pos0 + c, disable_medusa)[:, 0] for c in range(0, len(tokens), 16)], dim=1)

        seqs: List[List[int]] = []
        n_iter = n_tok = 0
        hist = [0] * (K + 1)
        for b in range(feats.shape[0]):
            eng.encode(feats[b: b + 1].contiguous())
            ids, kv = list(gp.prompt), 0
            if streamer is not None:
                streamer.put(torch.tensor([gp.prompt], dtype=torch.long))
            while True:
                L = len(ids)
                ids_t = torch.tensor([ids], dtype=torch.long)
                z = engine_pass(ids[kv:L], kv, False)[:, -1]                     # base + Medusa logits of the last position  [K+1, V]
                # two calls like the reference (model.py:653-655 base rows, :656-665 Medusa rows): a processor that indexes rows by batch
                # (HF RepetitionPenalty / NoRepeatNGram gather on row 0 of input_ids) then touches the base row in one call and the first
                # Medusa head's row in the other, as there.  (Only the LAST position is processed: on the first iteration the reference hands
                # over all P prompt positions x heads and consumes the last, medusa_utils.py:446-449.)
                zp = torch.cat([run(ids_t, z[:1]), run(ids_t, z[1:])], dim=0) if z.shape[0] > 1 else run(ids_t, z)
                cand = torch.argmax(zp, dim=-1)                                   # generate_candidates, top-1 chain (medusa_utils.py:446-458)
                v = run(ids_t, engine_pass(cand.tolist(), L, True)[0])            # verify pass (medusa_utils.py:494-521), same input_ids
                a = self._accept_length(v, cand, gp)
                if a == 0:
                    emit = [int(cand[0]), int(torch.argmax(v[0]))]               # model.py:710-713, medusa_utils.py:636-641
                    kv = L + 1
                else:
                    emit = [int(t) for t in cand[: a + 1]]
                    kv = L + a
                ids += emit
                hist[a] += 1; n_iter += 1; n_tok += len(emit)
                if streamer is not None:
                    streamer.put(torch.tensor(emit, dtype=torch.long))
                stop = bool(host_crit) and any(bool(torch.as_tensor(c(torch.tensor([ids], dtype=torch.long), None)).all()) for c in host_crit)
                if stop or eos in emit or len(ids) >= gp.max_length or len(ids) + K >= gp.hard_max_length:     # model.py:774-793
                    break
            if eos in ids[P:]:                                                    # post-EOS overwrite, model.py:798-810
                j = ids.index(eos, P)
                ids = ids[: j + 1] + [eos] * (len(ids) - j - 1)
            seqs.append(ids)
            if streamer is not None:
                streamer.end()
        return seqs, dict(iterations=n_iter, iterations_launched=n_iter, tokens_emitted=n_tok, accept_hist=hist, host_processors=len(procs))

    def _outputs(self, seqs, gp, return_dict_in_generate, return_segments, token_timestamps=None, scores=None):
        """Default: the padded LongTensor.  ``return_dict_in_generate`` / ``return_segments``: the reference's dict form
        ``{"sequences": ..., ["segments": ...]}`` (model.py:1747-1779; one segment per clip, short-form only)."""
        return self._wrap_outputs(self._pad(seqs, gp), [len(gp.prompt)] * len(seqs), gp.pad_token_id, gp.eos_token_id,
                                  return_dict_in_generate, return_segments, timestamps=gp.timestamps,
                                  time_precision=gp._time_precision, token_timestamps=token_timestamps, scores=scores)

    def _wrap_outputs(self, t, prompt_lens, pad, eos, return_dict_in_generate, return_segments, timestamps=False, time_precision=0.02,
                      token_timestamps=None, scores=None):
        """``return_dict_in_generate``: a GenerateEncoderDecoderOutput (model.py:812-823, :1715-1742); ``return_segments`` alone:
        the dict {"sequences", "segments"} of model.py:1764-1779 (one segment per clip, short-form only)."""
        if scores is not None:
            # the scoring pass ran: its fields go into every dict form of the output and stay in self.last_scores; return_token_logprobs forces
            # the dict form (as HF does for return_token_timestamps), thresholds alone keep the shape the caller asked for
            want = scores.get("_want", False)
            fields = {k: v for k, v in scores.items() if not k.startswith("_")}
            self.last_scores = fields
            out = self._wrap_outputs(t, prompt_lens, pad, eos, return_dict_in_generate or (want and not return_segments) or token_timestamps is not None,
                                     return_segments, timestamps, time_precision, token_timestamps)
            if not isinstance(out, dict):
                return out
            if "segments" not in out and return_segments:
                out["segments"] = self._wrap_outputs(t, prompt_lens, pad, eos, False, True, timestamps, time_precision)["segments"]
            if "segments" in out:
                for name in ("token_logprobs",) + _scores.TOPK_FIELDS:
                    if name in fields:
                        for i, P in enumerate(prompt_lens):
                            _segment_slices(out["segments"][i], P, name, fields[name][i])
            out.update(fields)
            return out
        if token_timestamps is not None:
            # HF forces return_dict_in_generate with return_token_timestamps: sequences + token_timestamps [B, T]; with return_segments every
            # segment also carries the slice of its own tokens (HF's long-form output shape)
            out = GenerateEncoderDecoderOutput(t, token_timestamps=token_timestamps)
            if return_segments:
                segs = self._wrap_outputs(t, prompt_lens, pad, eos, False, True, timestamps, time_precision)["segments"]
                for i, P in enumerate(prompt_lens):
                    _segment_slices(segs[i], P, "token_timestamps", token_timestamps[i])
                out["segments"] = segs
            return out
        if not return_dict_in_generate and not return_segments:
            return t
        segs = None
        if return_segments and not return_dict_in_generate and timestamps:
            # real segments: HF's _retrieve_segment over each row's generated ids (whisper_medusa/timestamps.py)
            rows = t.cpu()
            segs = [_timestamps.row_segments(rows[i].tolist(), P, eos, self.config.timestamp_begin, self.config.n_mel_frames,
                                             time_precision, result=t[i]) for i, P in enumerate(prompt_lens)]
        elif return_segments and not return_dict_in_generate:
            segs = [[{"start": torch.tensor(0.0), "end": torch.tensor(30.0 * self.config.max_source_positions / 1500.0),
                      "tokens": t[i, P:][t[i, P:] != pad] if pad != eos else t[i, P:],
                      "result": t[i]}] for i, P in enumerate(prompt_lens)]
        if return_dict_in_generate:
            # the reference returns the plain ModelOutput here (model.py:1715-1745 returns before the segments dict is built):
            # no extra key, so to_tuple() / integer indexing keep HF's positions
            return GenerateEncoderDecoderOutput(t)
        return {"sequences": t, "segments": segs}

    def _pad(self, seqs: List[List[int]], gp: GenParams) -> torch.Tensor:
        """G3: strip trailing pad/eos beyond the first EOS, right-pad to a tensor (model.py:1929-1973,1747-1762)."""
        return _ids_tensor([self._own_end(s, gp) for s in seqs], gp.pad_token_id).to(self.device)

    # ---- beyond the reference's generate(): language detection, long-form chunking, data-parallel sharding -------------
    @torch.no_grad()
    def detect_language(self, input_features: torch.Tensor) -> List[str]:
        """Language token of every clip: argmax over the language ids of the base logits after <|startoftranscript|>
        (HF WhisperGenerationMixin.detect_language, which the reference reaches through _retrieve_init_tokens when
        `language` is None, model.py:1519-1537; with the Medusa model the first of the stacked heads is the base head)."""
        cfg = self.config
        if not cfg.is_multilingual:
            raise ValueError("language detection needs a multilingual checkpoint")
        feats = input_features.to(self.device, torch.float32).contiguous()
        B = feats.shape[0]
        if B > self._max_batch:
            self.set_max_batch(B)
        self.engine.encode(feats)
        z = self.engine.forward_logits([[cfg.decoder_start_token_id]] * B, 0, True)[0, :, 0]      # [B, V]
        toks = [k for k in sorted(cfg.lang_to_id, key=lambda k: cfg.lang_to_id[k]) if 0 <= cfg.lang_to_id[k] < cfg.vocab_size]
        if not toks:
            raise ValueError("language detection: no language token of lang_to_id lies inside the vocabulary")
        ids = torch.tensor([cfg.lang_to_id[t] for t in toks])
        best = z[:, ids].argmax(-1)
        return [toks[int(i)] for i in best]

    def _generate_detecting_language(self, input_features, call: "ResolvedCall"):
        langs = self.detect_language(input_features)
        groups: Dict[str, List[int]] = {}
        for i, l in enumerate(langs):
            groups.setdefault(l, []).append(i)
        req, sreq, samp = call.tt_req, call.sc_req, call.samp
        nret = call.beam["num_return_sequences"] if call.beam is not None else 1
        rows: List[Optional[list]] = [None] * len(langs)
        plens = [0] * len(langs)
        tts: List[Optional[torch.Tensor]] = [None] * len(langs)
        scs: List[Optional[dict]] = [None] * len(langs)
        ms_tt = ms_sc = 0.0
        bscores: Dict[int, torch.Tensor] = {}
        nf = req["num_frames"] if req is not None else None
        for l, idx in groups.items():
            # one group = every clip in its original order: the engine still holds the encoder pass detect_language() ran.  Per-stream
            # num_frames and the seeded sampling's stream ids follow their clips into the group
            res = self._generate_short(input_features[idx], call, language=l, encoded=len(groups) == 1,
                                       stream_ids=None if samp is None else [i if samp["ids"] is None else samp["ids"][i] for i in idx],
                                       num_frames=[nf[i] for i in idx] if isinstance(nf, list) else None)
            ms_tt += res.stats.get("ms_token_timestamps", 0.0)
            ms_sc += res.stats.get("ms_token_logprobs", 0.0)
            own = [self._own_end(s, res.gp) for s in res.seqs]
            for j, i in enumerate(idx):
                rows[i] = own[j * nret: (j + 1) * nret]     # (beam search with num_return_sequences: nret rows per clip)
                plens[i] = len(res.gp.prompt)
                if call.beam is not None:
                    bscores[i] = res.sequences_scores[j * nret: (j + 1) * nret]
                if req is not None:
                    tts[i] = res.token_timestamps[j]
                if sreq is not None:
                    scs[i] = {k: v[j] for k, v in res.scores.items() if not k.startswith("_")}
        t = _ids_tensor([r_ for r in rows for r_ in r], self.config.pad_token_id).to(self.device)      # clip-major
        plens = [p_ for p_ in plens for _ in range(nret)]
        T = t.shape[1]
        self.detected_languages = langs
        self._clip_languages = list(langs)
        tt = None
        if req is not None:
            tt = _ts_tensor(tts, T)
            res.stats["ms_token_timestamps"] = ms_tt
        sc = None
        if sreq is not None:
            # per-clip fields of the groups back in the clips' order; token_logprobs rows are 0 after a stream's end
            sc = {"_want": sreq["want"]}
            for k in scs[0]:
                if k == "token_logprobs":
                    sc[k] = _lp_tensor([f[k] for f in scs], T)
                elif k in _scores.TOPK_FIELDS:      # [T_group(, k)] per clip: -1 / -inf / 0 behind the group's own length
                    if k == _scores.TOPK_FIELDS[0]:
                        sc.update(self._topk_stack(scs, T))
                else:
                    sc[k] = torch.stack([f[k] for f in scs])
            res.stats["ms_token_logprobs"] = ms_sc
        out = self._wrap_outputs(t, plens, self.config.pad_token_id, self.config.eos_token_id, call.return_dict_in_generate, call.return_segments,
                                 timestamps=call.return_timestamps, time_precision=call.time_precision, token_timestamps=tt, scores=sc)
        if bscores:
            res.sequences_scores = torch.cat([bscores[i] for i in range(len(langs))])
            if isinstance(out, dict):
                out["sequences_scores"] = res.sequences_scores
        return self._publish(res, out)

    def _generate_longform(self, input_features, call: "ResolvedCall", language, detect: bool):
        """`chunk_longform=True`: clips longer than 30 s (the reference raises, model.py:1213-1214) are cut into 30 s windows,
        the windows of all clips are decoded as ONE batch of independent streams (that is what the engine's batch is), and
        each clip's windows are concatenated: prompt once, then the generated ids of every window without its EOS / padding.
        No conditioning on the previous window (unsupported with Medusa in the reference as well).  `return_timestamps=True`: every
        window keeps its timestamp tokens (relative to the window); `return_segments=True` then gives each window's segments offset by
        the window's start, j * n_mel_frames * 10 ms (the windows stay fixed: HF's sequential seek to the last timestamp is not done).
        With the scoring arguments every window is scored and gated on its own: a skipped window (no_speech_threshold) contributes no ids, no
        segments and no token timestamps to its clip and leaves the offsets of the following windows where they are."""
        cfg = self.config
        rdg, sreq, req = call.return_dict_in_generate, call.sc_req, call.tt_req
        rseg, tprec, rts = call.return_segments, call.time_precision, call.return_timestamps
        F = cfg.n_mel_frames
        B, _, T = input_features.shape
        n = -(-T // F)
        x = torch.zeros(B, cfg.num_mel_bins, n * F, dtype=torch.float32, device=self.device)
        x[..., :T] = input_features.to(self.device, torch.float32)
        # zero-padded log-mel frames are not silence (silence maps to a constant negative level): pad in the feature domain
        # with the clip's own minimum, which is what the log-mel of digital silence clamps to
        if n * F > T:
            x[..., T:] = input_features.to(self.device, torch.float32).amin(dim=(1, 2), keepdim=True)
        win = x.view(B, cfg.num_mel_bins, n, F).permute(0, 2, 1, 3).reshape(B * n, cfg.num_mel_bins, F).contiguous()
        # the language is detected ONCE per clip, on its first window, and every window of the clip is decoded in that language
        # (clips of different languages are decoded as separate groups, each with its own prompt); language=[...]: one language per
        # recording (generate() has checked and resolved them)
        if detect:
            langs = self.detect_language(win[::n])
        else:
            langs = list(language) if isinstance(language, (list, tuple)) else [language] * B
        self._clip_languages = list(langs)
        rows, prompts = [None] * (B * n), [None] * B
        if req is not None and req["num_frames"] is not None:
            raise NotImplementedError("num_frames= is not supported together with chunk_longform=True (the windows are fixed)")
        wtt = [None] * (B * n)
        wsc: List[Optional[dict]] = [None] * (B * n)
        ms_tt = ms_sc = 0.0
        for l in sorted(set(langs), key=lambda v: (v is None, v or "")):
            clips = [b for b in range(B) if langs[b] == l]
            widx = [b * n + j for b in clips for j in range(n)]
            res = self._generate_short(win[widx], call, language=l)
            o = self._pad(res.seqs, res.gp)
            ms_tt += res.stats.get("ms_token_timestamps", 0.0)
            ms_sc += res.stats.get("ms_token_logprobs", 0.0)
            for q, wi in enumerate(widx):
                rows[wi] = o[q]
                if req is not None:
                    wtt[wi] = res.token_timestamps[q].cpu()
                if sreq is not None:
                    wsc[wi] = {k: v[q].cpu() for k, v in res.scores.items() if not k.startswith("_")}
            for b in clips:
                prompts[b] = list(res.gp.prompt)
        eos, pad = cfg.eos_token_id, cfg.pad_token_id
        seqs, all_tt, all_lp = [], [], []
        segs = [[] for _ in range(B)]
        for b in range(B):
            ids = list(prompts[b])
            P = len(ids)
            tts = [0.0] * P
            lps, last_eos_lp = [0.0] * P, 0.0
            for j in range(n):
                wi = b * n + j
                if sreq is not None and "skipped" in wsc[wi] and bool(wsc[wi]["skipped"]):
                    continue
                start = torch.tensor(j * F * 0.01, dtype=torch.float32)       # the window's start (float32 sum, as the tensors hold it)
                if rts and rseg:
                    ws = _timestamps.row_segments(rows[wi].tolist(), P, eos, cfg.timestamp_begin, F, tprec, time_offset=j * F * 0.01, result=rows[wi])
                    if req is not None:     # each segment's slice of its own window's values (times offset like its start / end)
                        _segment_slices(ws, P, "token_timestamps", wtt[wi] + start)
                    if sreq is not None:
                        _segment_slices(ws, P, "token_logprobs", wsc[wi]["token_logprobs"])
                    segs[b] += ws
                for q, t in enumerate(rows[wi][P:].tolist()):
                    if t == eos or t == pad:
                        if sreq is not None:      # the clip's one EOS takes the score of the last kept window's
                            last_eos_lp = float(wsc[wi]["token_logprobs"][P + q])
                        break
                    ids.append(t)
                    if sreq is not None:
                        lps.append(float(wsc[wi]["token_logprobs"][P + q]))
                    if req is not None:       # the window's own value, offset by the window's start
                        tts.append(float(wtt[wi][P + q] + start))
            seqs.append(ids + [eos])
            all_tt.append(tts + [tts[-1]])
            all_lp.append(lps + [last_eos_lp])
        t = _ids_tensor(seqs, pad).to(self.device)
        fields = None
        if sreq is not None:
            # per clip: the kept tokens' scores, their average and the compression ratio of the assembled ids; per window [B, n]: the gate's inputs and verdicts
            fields = self._clip_score_fields(all_lp, seqs, prompts)
            for k in ("no_speech_prob", "skipped", "needs_fallback"):
                if k in wsc[0]:
                    fields[k] = torch.stack([wsc[i][k] for i in range(B * n)]).view(B, n).to(self.device)
            fields["window_avg_logprob"] = torch.stack([wsc[i]["avg_logprob"] for i in range(B * n)]).view(B, n).to(self.device)
            self.last_scores = fields
            res.stats["ms_token_logprobs"] = ms_sc
        if req is not None:
            res.stats["ms_token_timestamps"] = ms_tt
        self._publish(res, None)
        if req is not None:
            out = GenerateEncoderDecoderOutput(t, token_timestamps=_ts_tensor(all_tt).to(self.device))
            if rts and rseg:
                out["segments"] = segs
            if fields is not None:
                out.update(fields)
            return out
        if fields is not None and (sreq["want"] or rdg):
            out = GenerateEncoderDecoderOutput(t, **fields)
            if rts and rseg:
                out["segments"] = segs
            return out
        if rts and rseg:
            return dict({"sequences": t, "segments": segs}, **(fields or {}))
        return t

    # ---- chunk long-form with overlapping windows: HF's strided chunks, merged on the device --------------------------
    def _stride_frames(self, stride_length_s) -> Tuple[int, int]:
        """``stride_length_s`` (HF pipeline: a float for both sides, or a pair (left, right)) as whole 10 ms frames."""
        F = self.config.n_mel_frames
        sides = tuple(stride_length_s) if isinstance(stride_length_s, (list, tuple)) else (stride_length_s, stride_length_s)
        if len(sides) != 2 or any(isinstance(s, bool) or not isinstance(s, (int, float, np.integer, np.floating)) for s in sides):
            raise ValueError(f"`stride_length_s` has to be a float or a pair (left, right) of floats, but is {stride_length_s!r}")
        frames = []
        for s in sides:
            f = float(s) * 100.0
            if not np.isfinite(f) or f < 0 or abs(f - round(f)) > 1e-6:
                raise ValueError(f"`stride_length_s`: each side has to be a whole number of 10 ms frames (>= 0), but is {s!r}")
            frames.append(int(round(f)))
        if frames[0] + frames[1] <= 0:
            raise ValueError("`stride_length_s`: left + right has to be positive (without an overlap call chunk_longform=True alone)")
        if frames[0] + frames[1] >= F:
            raise ValueError(f"`stride_length_s`: left + right = {frames[0] + frames[1]} frames has to be less than the window of {F} frames")
        return frames[0], frames[1]

    @staticmethod
    def _window_plan(T: int, F: int, left: int, right: int) -> List[int]:
        """The start frame of every window over T frames (HF ``chunk_iter``): window j starts at j * (F - left - right), the last one is the
        first that reaches T."""
        step = F - left - right
        starts = [0]
        while starts[-1] + F < T:
            starts.append(starts[-1] + step)
        return starts

    def _strided_feature_windows(self, input_features, stride: Tuple[int, int]):
        """``input_features [B, n_mels, T > F]`` cut at the plan's seeks; frames behind T hold the clip's own minimum (the padding rule of
        _generate_longform).  All clips share T, so all own the same number of windows."""
        F = self.config.n_mel_frames
        B, M, T = input_features.shape
        starts = self._window_plan(T, F, *stride)
        x = input_features.to(self.device, torch.float32)
        xp = x.amin(dim=(1, 2), keepdim=True).expand(B, M, starts[-1] + F).clone()
        xp[..., :T] = x
        win = torch.stack([xp[..., s: s + F] for s in starts], dim=1).reshape(B * len(starts), M, F).contiguous()
        return win, [len(starts)] * B

    def _strided_wav_windows(self, wav, sampling_rate: int, stride: Tuple[int, int]):
        """Every recording cut in the sample domain under its own length (ragged window counts); each window zero-padded to the model's window and
        transformed on its own by wm_logmel, in groups of at most max_batch: HF's per-chunk features, the per-chunk ``max - 8`` clamp included."""
        F = self.config.n_mel_frames
        step = (F - stride[0] - stride[1]) * 160
        mono = self._wav_mono(wav, sampling_rate)
        counts, cuts = [], []
        for b, r in enumerate(mono):
            starts = self._window_plan(-(-r.numel() // 160), F, *stride)
            counts.append(len(starts))
            cuts += [(b, j * step) for j in range(len(starts))]
        feats = []
        for g in range(0, len(cuts), self._max_batch):
            grp = cuts[g: g + self._max_batch]
            buf = torch.zeros(len(grp), F * 160, dtype=torch.float32, device=self.device)
            for q, (b, s) in enumerate(grp):
                m = min(mono[b].numel() - s, F * 160)
                if m > 0:
                    buf[q, :m] = mono[b][s: s + m]
            feats.append(self.engine.logmel(buf))
        return torch.cat(feats), counts

    def _generate_strided(self, win, counts: List[int], stride: Tuple[int, int], call: "ResolvedCall", language, detect: bool):
        """`chunk_longform=True, stride_length_s=..`: the overlapping windows ``win [sum(counts), n_mels, F]`` of all clips (clip b owns
        ``counts[b]`` consecutive rows, window j starting at j * step frames) are decoded like _generate_longform's — language once per clip on its
        first window, one batch per language group — stripped to their text ids and stitched by ONE ``engine.merge_windows`` call (HF's
        _find_longest_common_sequence for every boundary of every clip).  Every per-token field follows the kept slices; a window
        the gate skipped enters the merge as an empty window."""
        cfg = self.config
        rdg, sreq, req = call.return_dict_in_generate, call.sc_req, call.tt_req
        F, B = cfg.n_mel_frames, len(counts)
        step = F - stride[0] - stride[1]
        if req is not None and req["num_frames"] is not None:
            raise NotImplementedError("num_frames= is not supported together with chunk_longform=True (the windows are fixed)")
        first = [0]
        for c in counts:
            first.append(first[-1] + c)
        W, n = first[-1], max(counts)
        if win.shape[0] != W or min(counts) < 1:
            raise ValueError(f"strided long-form: {win.shape[0]} windows for the counts {counts}")
        win = win.to(self.device, torch.float32)
        if detect:
            langs = self.detect_language(win[first[:-1]])
        else:
            langs = list(language) if isinstance(language, (list, tuple)) else [language] * B
        self._clip_languages = list(langs)
        rows, prompts = [None] * W, [None] * B
        wtt = [None] * W
        wsc: List[Optional[dict]] = [None] * W
        ms_tt = ms_sc = 0.0
        for l in sorted(set(langs), key=lambda v: (v is None, v or "")):
            clips = [b for b in range(B) if langs[b] == l]
            widx = [w for b in clips for w in range(first[b], first[b + 1])]
            res = self._generate_short(win[widx], call, language=l)
            ms_tt += res.stats.get("ms_token_timestamps", 0.0)
            ms_sc += res.stats.get("ms_token_logprobs", 0.0)
            for q, wi in enumerate(widx):
                rows[wi] = self._own_end(res.seqs[q], res.gp)      # (up to its own EOS, if it emitted one)
                if req is not None:
                    wtt[wi] = res.token_timestamps[q].cpu()
                if sreq is not None:
                    wsc[wi] = {k: v[q].cpu() for k, v in res.scores.items() if not k.startswith("_")}
            for b in clips:
                prompts[b] = list(res.gp.prompt)
        eos, pad = cfg.eos_token_id, cfg.pad_token_id
        # every window's text ids (no prompt, EOS, padding) and, with token timestamps, their absolute times as float32
        text: List[List[int]] = [[] for _ in range(W)]
        times: List[List[float]] = [[] for _ in range(W)]
        for b in range(B):
            P = len(prompts[b])
            for j in range(counts[b]):
                wi = first[b] + j
                if sreq is not None and "skipped" in wsc[wi] and bool(wsc[wi]["skipped"]):
                    continue
                gen = rows[wi][P:]
                m = next((q for q, t in enumerate(gen) if t == eos or t == pad), len(gen))
                text[wi] = gen[:m]
                if req is not None:     # the window's own values, offset by the window's start (float32 sum, as the tensors hold it)
                    times[wi] = (wtt[wi][P: P + m] + torch.tensor(j * step * 0.01, dtype=torch.float32)).tolist()
        eng = self.engine
        keeps = eng.merge_windows([text[first[b]: first[b + 1]] for b in range(B)],
                                  [times[first[b]: first[b + 1]] for b in range(B)] if req is not None else None)
        seqs, all_tt, all_lp = [], [], []
        for b in range(B):
            ids = list(prompts[b])
            P = len(ids)
            tts = [0.0] * P
            lps, last_eos_lp = [0.0] * P, 0.0
            for j in range(counts[b]):
                wi = first[b] + j
                if sreq is not None and "skipped" in wsc[wi] and bool(wsc[wi]["skipped"]):
                    continue
                lo, hi = keeps[b][j]
                ids += text[wi][lo:hi]
                if sreq is not None:
                    lp = wsc[wi]["token_logprobs"]
                    lps += [float(v) for v in lp[P + lo: P + hi]]
                    if P + len(text[wi]) < len(rows[wi]):      # the clip's one EOS takes the score of the last kept window's
                        last_eos_lp = float(lp[P + len(text[wi])])
                if req is not None:
                    tts += times[wi][lo:hi]
            seqs.append(ids + [eos])
            all_tt.append(tts + [tts[-1]])
            all_lp.append(lps + [last_eos_lp])
        t = _ids_tensor(seqs, pad).to(self.device)
        window_keep = torch.full((B, n, 2), -1, dtype=torch.long)
        for b in range(B):
            window_keep[b, : counts[b]] = torch.tensor(keeps[b], dtype=torch.long).view(-1, 2)
        window_keep = window_keep.to(self.device)
        self.last_window_keep = window_keep

        def per_window(k, fill):
            # window-level fields stay [B, n]: NaN / False behind a clip's last window
            out = torch.full((B, n), fill, dtype=wsc[0][k].dtype)
            for b in range(B):
                out[b, : counts[b]] = torch.stack([wsc[w][k] for w in range(first[b], first[b + 1])])
            return out.to(self.device)

        fields = None
        if sreq is not None:
            fields = self._clip_score_fields(all_lp, seqs, prompts)
            for k in ("no_speech_prob", "skipped", "needs_fallback"):
                if k in wsc[0]:
                    fields[k] = per_window(k, False if wsc[0][k].dtype == torch.bool else float("nan"))
            fields["window_avg_logprob"] = per_window("avg_logprob", float("nan"))
            self.last_scores = fields
            res.stats["ms_token_logprobs"] = ms_sc
        if req is not None:
            res.stats["ms_token_timestamps"] = ms_tt
        res.stats["ms_merge"] = float(getattr(eng, "last_merge_ms", 0.0))
        res.stats["longform_windows"] = list(counts)
        self._publish(res, None)
        if req is not None:
            return GenerateEncoderDecoderOutput(t, token_timestamps=_ts_tensor(all_tt).to(self.device), window_keep=window_keep, **(fields or {}))
        if rdg or (fields is not None and sreq["want"]):
            return GenerateEncoderDecoderOutput(t, window_keep=window_keep, **(fields or {}))
        return t

    # ---- VAD long-form: speech windows cut at pauses on the device, silence never decoded ----------------------------------
    def _check_vad(self, kwargs, top_logprobs=None) -> Optional[dict]:
        """What ``vad_longform=True`` refuses, each under its own name; returns the plan generate_from_wav handed in (None: not a VAD call)."""
        if not kwargs.get("vad_longform"):
            if kwargs.get("vad_options") is not None:
                raise ValueError("vad_options is only valid together with vad_longform=True")
            return None
        for other in ("chunk_longform", "sequential_longform"):
            if kwargs.get(other):
                raise ValueError(f"vad_longform and {other} are alternatives: pass one of them")
        if kwargs.get("stride_length_s") is not None:
            raise ValueError("vad_longform and stride_length_s are alternatives: VAD windows are cut at pauses and do not overlap")
        if kwargs.get("num_beams") not in (None, 1):
            raise NotImplementedError("beam search (num_beams) is not supported with vad_longform (short-form only)")
        if kwargs.get("sampling_seed") is not None or kwargs.get("do_sample"):
            raise NotImplementedError("sampling (sampling_seed / do_sample) is not supported with vad_longform; use sequential_longform")
        if top_logprobs is not None:
            raise NotImplementedError("top_logprobs is not supported with vad_longform (short-form only)")
        for names in (("sequence_bias", "bad_words_ids", "hotwords"), ("allowed_sequences", "allowed_phrases")):
            given = [k for k in names if kwargs.get(k) is not None]
            if given:
                raise NotImplementedError(f"{' / '.join(given)} is not supported with vad_longform (short-form only)")
        if kwargs.get("num_frames") is not None:
            raise NotImplementedError("num_frames= is not supported together with vad_longform=True (the detector fixes the windows)")
        if kwargs.get("streamer") is not None:
            raise NotImplementedError("streamer= is not supported with vad_longform (the windows of a recording are decoded as one batch)")
        plan = kwargs.get("_vad_plan")
        if plan is None:
            raise ValueError("vad_longform needs the waveform: call generate_from_wav(wav, vad_longform=True), not generate(input_features=...)")
        return plan

    def _wav_mono(self, wav, sampling_rate: int) -> List[torch.Tensor]:
        """The audio front door of extract_features: every recording as 16 kHz mono float32 [n] on the GPU (downmix and resampling there).  Clips in
        a list are mono [n] or multi-channel [channels, n]; a bare 2-D array is a batch of mono clips."""
        if isinstance(wav, (list, tuple)):
            clips = [np.asarray(w, dtype=np.float32) for w in wav]
        else:
            a = wav.detach().cpu().numpy() if isinstance(wav, torch.Tensor) else np.asarray(wav)
            a = a.astype(np.float32)
            clips = [a] if a.ndim == 1 else [r for r in a]
        mono = []
        for c in clips:
            if c.ndim == 2 or sampling_rate != 16000:
                t = torch.from_numpy(np.atleast_2d(c)[None]).to(self.device)     # [1, channels, n_in]
                mono.append(self.engine.resample(t, sampling_rate, 16000)[0])
            else:
                mono.append(torch.from_numpy(c).to(self.device))
        return mono

    def _vad_detect(self, mono: List[torch.Tensor], vad_options) -> dict:
        """ONE ``engine.vad_windows`` call for all recordings: the plan ``dict(regions, windows, params, ms_vad)`` in 10 ms frames."""
        params = _vad.lower_options(vad_options, self.config.n_mel_frames)
        if any(r.numel() < 1 for r in mono):
            raise ValueError("vad_longform / detect_speech: a recording without samples")
        buf = torch.zeros(len(mono), max(r.numel() for r in mono), dtype=torch.float32, device=self.device)
        for i, r in enumerate(mono):
            buf[i, : r.numel()] = r
        eng = self.engine
        regions, windows = eng.vad_windows(buf, [r.numel() for r in mono], params)
        return dict(regions=regions, windows=windows, params=params, ms_vad=float(getattr(eng, "last_vad_ms", 0.0)))

    def detect_speech(self, wav, sampling_rate: int = 16000, **vad_options) -> List[dict]:
        """Where the speech of every recording lies and how ``generate_from_wav(vad_longform=True)`` would cut it: per recording
        ``dict(regions=[(start, end)..], windows=[(start, end)..])`` in seconds (frames * 0.01).  An energy detector with hysteresis relative to
        the recording's own loud level (include/wm.h wm_vad_windows), not a trained VAD model; ``vad_options``: onset_db,
        offset_db, loud_percentile, min_level_dbfs, min_silence_ms, min_speech_ms, speech_pad_ms, max_window_s — the defaults are untuned."""
        plan = self._vad_detect(self._wav_mono(wav, sampling_rate), vad_options or None)
        sec = lambda pairs: [(a * 0.01, b * 0.01) for a, b in pairs]          # noqa: E731
        return [dict(regions=sec(r), windows=sec(w)) for r, w in zip(plan["regions"], plan["windows"])]

    def _vad_wav_windows(self, wav, sampling_rate: int, vad_options):
        """Detect, then cut every window in the sample domain as [160 u, min(160 v, n)), zero-padded to the model's window and transformed on its
        own by wm_logmel in groups of at most max_batch (the recipe of _strided_wav_windows).  A recording without a window contributes its first
        window's worth of audio as one row, so that its language and prompt are defined; ``plan["first"]`` says which rows a recording owns."""
        F = self.config.n_mel_frames
        mono = self._wav_mono(wav, sampling_rate)
        plan = self._vad_detect(mono, vad_options)
        cuts, first = [], [0]
        for b, ws in enumerate(plan["windows"]):
            cuts += [(b, 160 * u, min(160 * v, mono[b].numel())) for u, v in ws] or [(b, 0, min(160 * F, mono[b].numel()))]
            first.append(len(cuts))
        feats = []
        for g in range(0, len(cuts), self._max_batch):
            grp = cuts[g: g + self._max_batch]
            buf = torch.zeros(len(grp), F * 160, dtype=torch.float32, device=self.device)
            for q, (b, lo, hi) in enumerate(grp):
                buf[q, : hi - lo] = mono[b][lo:hi]
            feats.append(self.engine.logmel(buf))
        plan["first"] = first
        return torch.cat(feats), plan

    def _generate_vad(self, win, plan: dict, call: "ResolvedCall", language, detect: bool):
        """`generate_from_wav(vad_longform=True)`: the rows ``win`` are the speech windows of all recordings (recording b owns the rows
        ``plan["first"][b] .. plan["first"][b + 1]``; one placeholder row where it has no window), decoded like _generate_longform's — language
        once per recording on its first row, one batch per language group — and assembled per recording: the prompt once, every window's ids
        without EOS or padding, one EOS.  Window j of a recording starts at u_j * 0.01 s on the recording's clock: that start is added to the
        window's segments and token timestamps.  A recording without speech returns prompt + EOS.  No conditioning across windows; times a
        window emits beyond its own audio, in the zero padding, are not clamped."""
        cfg = self.config
        rdg, sreq, req = call.return_dict_in_generate, call.sc_req, call.tt_req
        rseg, tprec, rts = call.return_segments, call.time_precision, call.return_timestamps
        F, wins, first = cfg.n_mel_frames, plan["windows"], plan["first"]
        B = len(wins)
        counts = [len(w) for w in wins]
        n = max(counts + [0])
        if win.shape[0] != first[-1]:
            raise ValueError(f"vad_longform: {win.shape[0]} rows for the plan's {first[-1]}")
        win = win.to(self.device, torch.float32)
        if detect:
            langs = self.detect_language(win[first[:-1]])
        else:
            langs = list(language) if isinstance(language, (list, tuple)) else [language] * B
        self._clip_languages = list(langs)
        W = first[-1]
        rows, prompts = [None] * W, [None] * B
        wtt = [None] * W
        wsc: List[Optional[dict]] = [None] * W
        ms_tt = ms_sc = 0.0
        for l in sorted(set(langs), key=lambda v: (v is None, v or "")):
            clips = [b for b in range(B) if langs[b] == l]
            # the windows of the group; a group of silent recordings alone decodes one placeholder row for its prompt
            widx = [first[b] + j for b in clips for j in range(counts[b])] or [first[clips[0]]]
            res = self._generate_short(win[widx], call, language=l)
            o = self._pad(res.seqs, res.gp)
            ms_tt += res.stats.get("ms_token_timestamps", 0.0)
            ms_sc += res.stats.get("ms_token_logprobs", 0.0)
            for q, wi in enumerate(widx):
                rows[wi] = o[q]
                if req is not None:
                    wtt[wi] = res.token_timestamps[q].cpu()
                if sreq is not None:
                    wsc[wi] = {k: v[q].cpu() for k, v in res.scores.items() if not k.startswith("_")}
            for b in clips:
                prompts[b] = list(res.gp.prompt)
        eos, pad = cfg.eos_token_id, cfg.pad_token_id
        seqs, all_tt, all_lp = [], [], []
        segs = [[] for _ in range(B)]
        for b in range(B):
            ids = list(prompts[b])
            P = len(ids)
            tts = [0.0] * P
            lps, last_eos_lp = [0.0] * P, 0.0
            for j in range(counts[b]):
                wi = first[b] + j
                if sreq is not None and "skipped" in wsc[wi] and bool(wsc[wi]["skipped"]):
                    continue
                t0 = wins[b][j][0] * 0.01                                  # the window's start on the recording's clock
                start = torch.tensor(t0, dtype=torch.float32)              # (float32 sum, as the tensors hold it)
                if rts and rseg:
                    ws = _timestamps.row_segments(rows[wi].tolist(), P, eos, cfg.timestamp_begin, F, tprec, time_offset=t0, result=rows[wi])
                    if req is not None:
                        _segment_slices(ws, P, "token_timestamps", wtt[wi] + start)
                    if sreq is not None:
                        _segment_slices(ws, P, "token_logprobs", wsc[wi]["token_logprobs"])
                    segs[b] += ws
                for q, t in enumerate(rows[wi][P:].tolist()):
                    if t == eos or t == pad:
                        if sreq is not None:      # the recording's one EOS takes the score of the last kept window's
                            last_eos_lp = float(wsc[wi]["token_logprobs"][P + q])
                        break
                    ids.append(t)
                    if sreq is not None:
                        lps.append(float(wsc[wi]["token_logprobs"][P + q]))
                    if req is not None:
                        tts.append(float(wtt[wi][P + q] + start))
            seqs.append(ids + [eos])
            all_tt.append(tts + [tts[-1]])
            all_lp.append(lps + [last_eos_lp])
        t = _ids_tensor(seqs, pad).to(self.device)
        vad_windows = torch.full((B, n, 2), -1, dtype=torch.long)
        for b in range(B):
            if counts[b]:
                vad_windows[b, : counts[b]] = torch.tensor(wins[b], dtype=torch.long).view(-1, 2)
        vad_windows = vad_windows.to(self.device)
        speech_regions = [[(a * 0.01, e * 0.01) for a, e in r] for r in plan["regions"]]
        self.last_vad_windows, self.last_speech_regions = vad_windows, speech_regions
        tmpl = next((w for w in wsc if w is not None), None)

        def per_window(k, fill):
            # window-level fields stay [B, n]: NaN / False behind a recording's last window
            out = torch.full((B, n), fill, dtype=tmpl[k].dtype)
            for b in range(B):
                if counts[b]:
                    out[b, : counts[b]] = torch.stack([wsc[w][k] for w in range(first[b], first[b] + counts[b])])
            return out.to(self.device)

        fields = None
        if sreq is not None:
            fields = self._clip_score_fields(all_lp, seqs, prompts)
            for k in ("no_speech_prob", "skipped", "needs_fallback"):
                if k in tmpl:
                    fields[k] = per_window(k, False if tmpl[k].dtype == torch.bool else float("nan"))
            fields["window_avg_logprob"] = per_window("avg_logprob", float("nan"))
            self.last_scores = fields
            res.stats["ms_token_logprobs"] = ms_sc
        if req is not None:
            res.stats["ms_token_timestamps"] = ms_tt
        res.stats["ms_vad"] = plan["ms_vad"]
        res.stats["longform_windows"] = list(counts)
        self._publish(res, None)
        extra = dict(vad_windows=vad_windows, speech_regions=speech_regions, **(fields or {}))
        if req is not None:
            out = GenerateEncoderDecoderOutput(t, token_timestamps=_ts_tensor(all_tt).to(self.device), **extra)
            if rts and rseg:
                out["segments"] = segs
            return out
        if rdg or (fields is not None and sreq["want"]):
            out = GenerateEncoderDecoderOutput(t, **extra)
            if rts and rseg:
                out["segments"] = segs
            return out
        if rts and rseg:
            return dict({"sequences": t, "segments": segs}, **extra)
        return t

    # ---- sequential long-form: HF's seek loop around the short-form path ---------------------------------------------
    def _check_sequential(self, return_timestamps, condition_on_prev_tokens, temperature, return_token_timestamps, logits_processor,
                          stopping_criteria, streamer, prompt_ids, prompt_condition_type):
        """What `sequential_longform=True` refuses, each under its own name."""
        if condition_on_prev_tokens:
            raise NotImplementedError("condition_on_prev_tokens=True is not supported with sequential_longform: every window of a clip is "
                                      "decoded under the same prompt (conditioning needs one prompt per stream)")
        if isinstance(temperature, (tuple, list)):
            raise NotImplementedError("a tuple `temperature` (temperature fallback) is not supported with sequential_longform without "
                                      "sampling_seed= (the engine's seeded sampling, DESIGN.md §2h)")
        if return_token_timestamps:
            raise NotImplementedError("return_token_timestamps is not supported together with sequential_longform")
        if not self.config.supports_timestamps:
            raise NotImplementedError("sequential_longform needs timestamp tokens and this checkpoint's vocabulary has no timestamp block "
                                      "(vocab_size - no_timestamps_token_id - 1 != max_source_positions + 1)")
        if not return_timestamps:
            # HF: "to generate transcriptions longer than 30 s you have to pass return_timestamps=True": the seek is read off the timestamps
            raise NotImplementedError("sequential_longform needs return_timestamps=True: the loop seeks to the last predicted timestamp")
        if self.config.is_tree:
            raise NotImplementedError("sequential_longform is not supported with a candidate tree (medusa_choices with top-k > 1)")
        if logits_processor or stopping_criteria:
            raise NotImplementedError("sequential_longform is not supported together with logits_processor= / stopping_criteria= "
                                      "(the host processor path)")
        if streamer is not None:
            raise NotImplementedError("streamer= is not supported with sequential_longform (windows of several clips decode as one batch)")
        if prompt_ids is not None and prompt_condition_type != "all-segments":
            raise NotImplementedError("prompt_ids with sequential_longform needs prompt_condition_type='all-segments': every window of a "
                                      "clip is decoded under the same prompt (HF's default, 'first-segment', needs one prompt per stream)")

    def _generate_sequential(self, input_features, attention_mask, call: "ResolvedCall", language, detect: bool, tprec_f: float):
        """`sequential_longform=True`: Whisper's own long-form algorithm (openai/whisper ``transcribe``; HF ``WhisperGenerationMixin.generate``
        on more than one window of features), batched over recordings.  Every clip keeps a seek into its features; per round the windows of
        all unfinished clips are cut out at their seeks in one launch (``wm_gather_windows``: slice, then zero pad, HF ``_get_input_segment``)
        and decoded as one batch through the short-form driver — timestamps on, the same prompt for every window of a clip, the scoring
        request when thresholds are given —; each clip then seeks to its window's last timestamp pair (the unfinished tail is decoded
        again, whole, by the next window) or, with no pair / a single closing timestamp / a window the no-speech gate skipped, by the whole
        window (``timestamps.sequential_seek_loop``).  The language is detected once per clip, on its first window; clips of different
        languages run as separate groups per round.  No conditioning on the previous window; the temperature fallback needs sampling_seed=."""
        cfg = self.config
        rdg, sreq, rseg, tprec = call.return_dict_in_generate, call.sc_req, call.return_segments, call.time_precision
        num_frames = call.opts.get("num_frames")
        F, eos, pad = cfg.n_mel_frames, cfg.eos_token_id, cfg.pad_token_id
        B, _, T = input_features.shape
        # per-clip lengths: HF's way (max_frames = attention_mask.sum(-1)), or num_frames=, else the whole tensor
        if attention_mask is not None:
            max_frames = [int(v) for v in torch.as_tensor(attention_mask).sum(-1).flatten().tolist()]
        elif num_frames is not None:
            nf = num_frames.tolist() if hasattr(num_frames, "tolist") else num_frames
            max_frames = [int(nf)] * B if isinstance(nf, (int, float)) else [int(v) for v in nf]
        else:
            max_frames = [T] * B
        if len(max_frames) != B or any(v < 0 or v > T for v in max_frames):
            raise ValueError(f"sequential_longform: one length in [0, {T}] per clip is needed (attention_mask [B, T] or num_frames [B])")
        if B > self._max_batch:
            self.set_max_batch(B)
        feats = input_features.to(self.device, torch.float32).contiguous()
        # language=[...]: one language per recording (generate() has checked and resolved them)
        langs: List[Optional[str]] = list(language) if isinstance(language, (list, tuple)) else [None if detect else language] * B
        prompts: List[Optional[List[int]]] = [None] * B
        # seeded sampling / temperature fallback: a window's stream key comes from its clip's id and its seek, not from the round
        sampling = call.opts.get("sampling_seed") is not None
        sids = call.opts.get("sampling_stream_ids")
        if sids is not None and len(sids) != B:
            raise ValueError(f"sampling_stream_ids needs one id per clip ({B}), got {len(sids)}")
        done: List[ShortResult] = []            # the short-form results, in order

        def decode_round(clips, seeks, snf):
            win = self.engine.gather_windows(feats, clips, seeks, snf)
            new = [q for q, b in enumerate(clips) if detect and langs[b] is None]
            if new:     # (every clip's first window)
                for q, l in zip(new, self.detect_language(win[new])):
                    langs[clips[q]] = l
            out: List[Optional[dict]] = [None] * len(clips)
            groups = sorted({langs[b] for b in clips}, key=lambda v: (v is None, v or ""))
            for l in groups:
                widx = [q for q, b in enumerate(clips) if langs[b] == l]
                res = self._generate_short(win[widx], call, language=l, encoded=len(groups) == 1 and len(new) == len(clips),
                                           stream_ids=[clips[q] if sids is None else int(sids[clips[q]]) for q in widx] if sampling else None,
                                           seeks=[int(seeks[q]) for q in widx] if sampling else None)
                done.append(res)
                o = self._pad(res.seqs, res.gp)
                P = len(res.gp.prompt)
                rows = o.cpu()
                if sreq is not None:
                    sc = {k: v.cpu() for k, v in res.scores.items() if not k.startswith("_")}
                for j, q in enumerate(widx):
                    prompts[clips[q]] = list(res.gp.prompt)
                    rec = dict(ids=_timestamps.generated_ids(rows[j].tolist(), P, eos), skipped=False, result=o[j])
                    if sreq is not None:
                        rec["scores"] = {k: v[j] for k, v in sc.items()}
                        rec["skipped"] = bool(rec["scores"]["skipped"]) if "skipped" in rec["scores"] else False
                    out[q] = rec
            return out

        windows = _timestamps.sequential_seek_loop(max_frames, F, decode_round, cfg.timestamp_begin, tprec, tprec_f,
                                                   F // cfg.max_source_positions)
        for b in range(B):
            if prompts[b] is None:      # a clip without a single frame: nothing was decoded, its row is the default prompt + EOS
                prompts[b] = list(self._gen_params(langs[b], call.task, None, None, None, None, False, None, None, None, None,
                                                   call.prompt_ids, timestamps=True).prompt)
        seqs = [_timestamps.assemble_sequence(prompts[b], windows[b], eos) for b in range(B)]
        segs = [[sg for w in windows[b] for sg in w["segments"]] for b in range(B)]
        t = _ids_tensor(seqs, pad).to(self.device)
        if detect:
            self.detected_languages = list(langs)
        stats = dict(done[-1].stats) if done else {}
        stats["longform_windows"] = [len(w) for w in windows]
        if sampling:
            stats["fallback_decodes"] = sum(r.stats.get("fallback_decodes", 0) for r in done)
        fields = None
        if sreq is not None:
            # per clip: the kept tokens' scores (a window's kept segments are a prefix of its ids), their average and the compression ratio of the
            # assembled ids; per window, ragged (clips take different numbers of windows): the gate's inputs and verdicts
            all_lp = []
            for b in range(B):
                P = len(prompts[b])
                r, last_eos = [0.0] * P, 0.0
                for w in windows[b]:
                    if w["skipped"]:
                        continue
                    n = sum(int(sg["tokens"].numel()) for sg in w["segments"])
                    wl = w["scores"]["token_logprobs"]
                    r += [float(v) for v in wl[P: P + n]]
                    k = P + len(w["ids"])                       # the window's own EOS, where it emitted one
                    last_eos = float(wl[k]) if k < int(w["scores"]["lengths"]) else 0.0
                    if rseg:
                        _segment_slices(w["segments"], P, "token_logprobs", wl)
                all_lp.append(r + [last_eos])
            fields = self._clip_score_fields(all_lp, seqs, prompts)
            any_w = next((w for ws in windows for w in ws), None)
            for k in ("no_speech_prob", "skipped", "needs_fallback"):
                if any_w is not None and k in any_w["scores"]:
                    fields[k] = [torch.stack([w["scores"][k] for w in ws]) if ws else torch.zeros(0) for ws in windows]
            fields["window_avg_logprob"] = [torch.stack([w["scores"]["avg_logprob"] for w in ws]) if ws else torch.zeros(0) for ws in windows]
            fields["window_seek"] = [torch.tensor([w["seek"] for w in ws], dtype=torch.long) for ws in windows]
            if any_w is not None and "fallback_temperature" in any_w["scores"]:
                fields["window_temperature"] = [torch.stack([w["scores"]["fallback_temperature"] for w in ws]) if ws else torch.zeros(0) for ws in windows]
                fields["window_attempts"] = [torch.stack([w["scores"]["fallback_attempts"] for w in ws]) if ws else torch.zeros(0, dtype=torch.long)
                                             for ws in windows]
            self.last_scores = fields
            stats["ms_token_logprobs"] = sum(r.stats.get("ms_token_logprobs", 0.0) for r in done)
        if done:
            self._publish(done[-1], None)
        self.last_stats = stats
        if fields is not None and (sreq["want"] or rdg):
            out = GenerateEncoderDecoderOutput(t, **fields)
            if rseg or rdg:
                out["segments"] = segs
            return out
        if rdg:     # (HF: return_dict_in_generate with return_timestamps sets return_segments)
            return GenerateEncoderDecoderOutput(t, segments=segs)
        if rseg:
            return dict({"sequences": t, "segments": segs}, **(fields or {}))
        return t

    def _clip_score_fields(self, all_lp, seqs, prompts) -> dict:
        """The per-clip score fields of a long-form result: the kept tokens' log-probabilities ``all_lp`` next to the assembled ids ``seqs``,
        their average, the compression ratio of the ids behind each clip's prompt, and the rows' lengths."""
        dev, n = self.device, range(len(seqs))
        Pb = [len(p_) for p_ in prompts]
        return dict(token_logprobs=_lp_tensor(all_lp, max(len(s_) for s_ in seqs)).to(dev),
                    avg_logprob=torch.tensor([_scores.avg_logprob(all_lp[i], Pb[i], len(seqs[i])) for i in n], dtype=torch.float32, device=dev),
                    compression_ratio=torch.tensor([_scores.compression_ratio(seqs[i][Pb[i]:], self.config.vocab_size) for i in n],
                                                   dtype=torch.float32, device=dev),
                    lengths=torch.tensor([len(s_) for s_ in seqs], dtype=torch.long, device=dev))

    @torch.no_grad()
    def generate_sharded(self, input_features: torch.Tensor, **kw) -> torch.Tensor:
        """Data-parallel generate() over the ranks of an initialised torch.distributed group (one process per GPU, SURVEY.md
        §8e): stream s is decoded on rank s mod world (dist.shard_streams), every rank receives all sequences
        (dist.gather_token_lists: ragged int lists, no device collective on the data path).  Every rank passes the SAME
        `input_features` (or at least its own shard's rows at the right indices)."""
        import torch.distributed as td
        from . import dist as _dist
        B = input_features.shape[0]
        if not (td.is_available() and td.is_initialized()) or td.get_world_size() == 1:
            return self.generate(input_features, **kw)
        rank, world = td.get_rank(), td.get_world_size()
        mine = _dist.shard_streams(B, rank, world)
        if isinstance(kw.get("language"), (list, tuple)):
            # language=[...]: checked against the WHOLE batch, then split with the clips
            kw = dict(kw, language=[self._language_list(kw["language"], B)[s_] for s_ in mine])
        local, local_sc = [], []
        gc = kw.get("generation_config")        # (the thresholds may come through a passed generation_config, as in generate())
        scoring = any(kw.get(k) is not None or getattr(gc, k, None) is not None
                      for k in ("no_speech_threshold", "logprob_threshold", "compression_ratio_threshold")) \
            or bool(kw.get("return_token_logprobs")) or kw.get("top_logprobs") is not None
        if mine and kw.get("sampling_seed") is not None:
            # seeded sampling: a stream keeps the key of its GLOBAL index (or of its caller-given id) on whichever rank it lands
            gids = kw.get("sampling_stream_ids")
            kw = dict(kw, sampling_stream_ids=[s_ if gids is None else int(gids[s_]) for s_ in mine])
        if mine:
            out = self.generate(input_features[mine], **kw)
            rows = out["sequences"] if isinstance(out, dict) else out
            nret = rows.shape[0] // len(mine)       # beam search with num_return_sequences: nret rows per clip, clip-major
            local = [(s_ * nret + k, rows[j * nret + k].tolist()) for j, s_ in enumerate(mine) for k in range(nret)]
            if scoring:     # every rank's per-stream score fields travel like its ids (ragged Python lists)
                local_sc = [(s_, {k: v[j].tolist() for k, v in self.last_scores.items()}) for j, s_ in enumerate(mine)]
        seqs = _dist.gather_token_lists(local)
        t = _ids_tensor(seqs, self.config.pad_token_id).to(self.device)
        T = t.shape[1]
        if not scoring:
            return t
        infos = _dist.gather_token_lists(local_sc)
        fields = {}
        for k in infos[0]:
            if k == "token_logprobs":
                fields[k] = _lp_tensor([f[k] for f in infos], T).to(self.device)
            elif k in _scores.TOPK_FIELDS:
                if k == _scores.TOPK_FIELDS[0]:
                    fields.update(self._topk_stack([{n_: torch.tensor(f[n_]) for n_ in _scores.TOPK_FIELDS} for f in infos], T))
            else:
                fields[k] = torch.tensor([f[k] for f in infos], device=self.device)
        self.last_scores = fields
        if kw.get("return_token_logprobs") or kw.get("top_logprobs") is not None or kw.get("return_dict_in_generate") or getattr(gc, "return_dict_in_generate", None):
            return GenerateEncoderDecoderOutput(t, **fields)
        return t

    def generate_from_wav(self, wav, **kw) -> torch.Tensor:
        """log-mel on the GPU, then ``generate`` — the whole hot path of SURVEY.md §8a in one call.  ``sequential_longform=True``: the
        log-mel of the whole recordings (``extract_features(truncation=False)``) and every clip's own length, then the sequential loop.
        ``vad_longform=True[, vad_options={..}]``: the speech of every recording is found on the device, cut only at pauses
        and packed into windows of at most the model's window, all windows of all recordings are decoded as batches, and the times go back
        on the recording's clock; ``vad_windows`` / ``speech_regions`` in the dict forms, ``last_stats["ms_vad"]``."""
        if kw.get("vad_longform") or kw.get("vad_options") is not None:
            # speech windows cut at pauses: detect on the device, cut in the sample domain, one log-mel per window
            self._check_vad(dict(kw, _vad_plan={}), kw.get("top_logprobs"))
            win, plan = self._vad_wav_windows(wav, kw.pop("sampling_rate", 16000), kw.pop("vad_options", None))
            return self.generate(win, _vad_plan=plan, **kw)
        if kw.get("sequential_longform"):
            feats = self.extract_features(wav, kw.pop("sampling_rate", 16000), truncation=False)
            kw.setdefault("num_frames", self.last_num_frames)
            return self.generate(feats, **kw)
        if kw.get("stride_length_s") is not None and kw.get("chunk_longform"):
            # overlapping windows: cut in the sample domain, every recording under its own length, one log-mel per window
            win, counts = self._strided_wav_windows(wav, kw.pop("sampling_rate", 16000), self._stride_frames(kw["stride_length_s"]))
            return self.generate(win, _window_counts=counts, **kw)
        return self.generate(self.extract_features(wav), **kw)

    def stream_sessions(self, n: int, *, tokenizer=None, word_table=None, min_chunk_s: float = 1.0, trim_s: Optional[float] = None,
                        hard_trim_s: Optional[float] = None, late_s: float = 0.1, near_s: float = 1.0, **generate_kwargs):
        """``n`` live transcription sessions (whisper_medusa/streaming.py): ``sessions.feed([chunk or None, ...])`` appends 16 kHz
        audio to every session's rolling buffer, transcribes the sessions that received ``min_chunk_s`` of audio since their last decode as ONE
        ``generate(return_word_timestamps=True)`` batch, and commits the words on which two consecutive hypotheses agree (LocalAgreement-2,
        one HIP launch per tick for all sessions), with times on the recording's clock.  ``generate_kwargs`` go to every generate() call."""
        from .streaming import StreamSessions
        return StreamSessions(self, n, max_batch=self._max_batch, tokenizer=tokenizer, word_table=word_table, min_chunk_s=min_chunk_s, trim_s=trim_s,
                              hard_trim_s=hard_trim_s, late_s=late_s, near_s=near_s, **generate_kwargs)

    # ---- forward ----------------------------------------------------------------------------
    @torch.no_grad()
    def forward(self, input_features: Optional[torch.Tensor] = None, attention_mask=None,
                decoder_input_ids: Optional[torch.Tensor] = None, decoder_attention_mask=None, head_mask=None,
                decoder_head_mask=None, cross_attn_head_mask=None, encoder_outputs=None, past_key_values=None,
                decoder_inputs_embeds=None, decoder_position_ids=None, labels=None, use_cache: Optional[bool] = None,
                output_attentions: Optional[bool] = None, output_hidden_states: Optional[bool] = None,
                return_dict: Optional[bool] = None, disable_medusa: Optional[bool] = False, **kwargs):
        """One decoder pass over ``decoder_input_ids`` [B, T] — the reference's ``forward`` (model.py:1223-1347), same keywords:

        * ``input_features``: the encoder runs first; ``encoder_outputs`` (a tuple / ModelOutput whose first element is the last
          hidden state [B, n_ctx, d], or that tensor) replaces the encoder pass (model.py:1232 -> HF WhisperModel.forward) — the
          object a previous ``forward`` returned is recognised and costs nothing; neither: the last encoded batch is reused;
        * ``past_key_values`` / ``use_cache``: the KV cache lives in the engine (contiguous rows per layer / stream / head); the
          returned ``past_key_values`` is an ``EngineKVCache`` handle saying how many positions are cached, and a following call that
          passes it back appends its tokens behind them (``get_seq_length()`` like HF's cache classes).  ``decoder_position_ids``
          override the start position as in the reference;
        * ``return_dict=False`` gives the reference's tuple ``(logits, past_key_values, encoder_last_hidden_state)`` (``use_cache=None``
          counts as True, HF's ``config.use_cache`` default); the hidden state is copied from the device once per encoder pass;
        * masks, ``decoder_inputs_embeds``, attentions / hidden states and ``labels`` (training) are not part of the engine: they raise.

        ``logits`` are ``[K+1 (1 with disable_medusa), B, T, V]``.  The engine evaluates 16 positions per pass: longer inputs go
        through in 16-token chunks, each appending its K/V rows behind the previous chunk's."""
        if decoder_input_ids is None:
            raise ValueError("decoder_input_ids is required")
        if labels is not None or kwargs.get("labels") is not None:
            raise NotImplementedError("training (labels / loss) is out of scope for the inference engine")
        if decoder_attention_mask is not None:
            # a mask that masks nothing is what HF's own generate() passes along; anything else would need per-position masking in the
            # engine's causal attention (not built: the reference's loop never produces one)
            if not bool(torch.as_tensor(decoder_attention_mask).bool().all()):
                raise NotImplementedError("forward(decoder_attention_mask=...) with masked positions is not supported by the HIP engine")
            decoder_attention_mask = None
        for name, v in (("decoder_attention_mask", decoder_attention_mask), ("head_mask", head_mask), ("decoder_head_mask", decoder_head_mask),
                        ("cross_attn_head_mask", cross_attn_head_mask), ("decoder_inputs_embeds", decoder_inputs_embeds)):
            if v is not None:
                raise NotImplementedError(f"forward({name}=...) is not supported by the HIP engine")
        if output_attentions or output_hidden_states:
            raise NotImplementedError("attention weights / hidden states are not materialised by the HIP engine")
        B = int(decoder_input_ids.shape[0])
        if B > self._max_batch and (input_features is not None or encoder_outputs is not None):
            self.set_max_batch(B)                                           # a new encoder pass for more streams than the context holds
        eng = self.engine
        # ---- encoder side
        enc_ref = None
        if encoder_outputs is not None:
            stamp = getattr(encoder_outputs, "_wm_stamp", None)
            if stamp is not None and stamp is getattr(eng, "_enc_stamp", None):
                enc_ref = encoder_outputs                                   # our own handle, still resident: nothing to do
            else:
                first = encoder_outputs if isinstance(encoder_outputs, torch.Tensor) else (
                    encoder_outputs.last_hidden_state if hasattr(encoder_outputs, "last_hidden_state") else encoder_outputs[0])
                eng.set_encoder_output(first)
        elif input_features is not None:
            eng.encode(input_features.to(self.device, torch.float32).contiguous())
        elif getattr(eng, "_enc_stamp", None) is None:
            raise ValueError("forward() needs input_features or encoder_outputs (nothing has been encoded on this model yet)")
        # ---- start position
        pos0 = 0
        if past_key_values is not None:
            if not isinstance(past_key_values, EngineKVCache):
                raise NotImplementedError("past_key_values must be the EngineKVCache a previous forward(use_cache=True) returned: "
                                          "the KV cache is engine state (contiguous HBM rows), not a tuple of tensors")
            if past_key_values.engine_id != id(eng) or past_key_values.enc_stamp is not eng._enc_stamp or past_key_values.batch != B \
                    or past_key_values.kv_stamp is not eng._kv_stamp:
                raise ValueError("past_key_values belongs to another engine, encoder pass or batch size, or a generate() call has "
                                 "reused the cache since")
            pos0 = past_key_values.get_seq_length()
        if decoder_position_ids is not None:
            pos0 = int(torch.as_tensor(decoder_position_ids).flatten()[0])
        toks = decoder_input_ids.tolist()
        T = len(toks[0])
        if pos0 + T > self.config.max_target_positions:
            raise ValueError(f"decoder_input_ids of length {T} at position {pos0} exceed max_target_positions "
                             f"{self.config.max_target_positions}")
        dm = bool(disable_medusa)
        if T <= 16:
            logits = eng.forward_logits(toks, pos0, dm)
        else:
            logits = torch.cat([eng.forward_logits([row[c: c + 16] for row in toks], pos0 + c, dm) for c in range(0, T, 16)], dim=2)
        # use_cache=None means config.use_cache = True, as in HF (the reference's tuple is (logits, past_key_values, encoder state))
        want_cache = (use_cache is None) or bool(use_cache) or past_key_values is not None
        # the handle carries the stamp the pass just set (engine.forward_logits): older handles — positions now overwritten — are refused
        pkv = EngineKVCache(id(eng), eng._enc_stamp, eng._kv_stamp, B, pos0 + T) if want_cache else None
        if enc_ref is None:
            enc_ref = EngineEncoderOutput(eng, B, eng._enc_stamp)
        if return_dict is False:
            return (logits, pkv, enc_ref.last_hidden_state) if pkv is not None else (logits, enc_ref.last_hidden_state)
        return MedusaForwardOutput(logits=logits, past_key_values=pkv, encoder_outputs=enc_ref)

    __call__ = forward


def get_model(path, device=None):
    """reference model.py:2079-2097."""
    return WhisperMedusaModel.from_pretrained(path, device=device)
