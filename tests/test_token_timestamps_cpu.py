"""Token-level timestamps, host side: the reference helper of the GPU tests (tests/token_ts_ref.py) is pinned to transformers' own
_extract_token_timestamps / _dynamic_time_warping, and the config / API plumbing of generate(return_token_timestamps=True)."""
import ctypes as C
import json
import os
import re
import types

import numpy as np
import pytest
import torch

import token_ts_ref as ref
from helpers import MedusaConfig, synth, ROOT


def hf():
    from transformers.models.whisper import generation_whisper as g
    return g


class _Out(dict):
    __getattr__ = dict.__getitem__


def hf_timestamps(weights, heads_layers, n_layers, P, width, num_frames=None):
    """transformers' _extract_token_timestamps on weights [B, A, P + N, S]: head a is put at (layer a % n_layers, head a)."""
    g = hf()
    B, A, R, S = weights.shape
    layers = [torch.zeros(B, A, R, S) for _ in range(n_layers)]
    for a, l in enumerate(heads_layers):
        layers[l][:, a] = weights[:, a]
    out = _Out(cross_attentions=(tuple(layers),), sequences=torch.zeros(B, R + 1, dtype=torch.long))
    me = types.SimpleNamespace(config=types.SimpleNamespace(decoder_layers=n_layers, median_filter_width=width))
    heads = [[l, a] for a, l in enumerate(heads_layers)]
    return g.WhisperGenerationMixin._extract_token_timestamps(me, out, heads, time_precision=0.02, num_frames=num_frames, num_input_ids=P)


def random_softmax(gen, B, A, R, S, sharp=3.0):
    return torch.softmax(sharp * torch.randn(B, A, R, S, generator=gen), dim=-1)


def planted(gen, B, A, R, S, P):
    """A monotone alignment: row r attends around frame (r - P) * S / (R - P), plus noise."""
    x = 0.5 * torch.randn(B, A, R, S, generator=gen)
    f = torch.arange(S)[None, :]
    c = ((torch.arange(R) - P).clamp(min=0).float() * S / max(R - P, 1))[:, None]
    x = x + 6.0 * torch.exp(-0.5 * ((f - c) / 2.0) ** 2)
    return torch.softmax(x, dim=-1)


@pytest.mark.parametrize("N", [0, 1, 2, 17, 447])
@pytest.mark.parametrize("kind", ["random", "planted"])
def test_reference_helper_equals_transformers(N, kind):
    gen = torch.Generator().manual_seed(100 + N)
    P, A, L, width = 3, 4, 3, 7
    S = 60 if N == 447 else 96
    B = 1 if N == 447 else 2
    R = P + N
    w = (random_softmax if kind == "random" else lambda *a: planted(*a, P))(gen, B, A, R, S)
    lay = [a % L for a in range(A)]
    cases = [None, 2 * 40] if N != 447 else [None]
    if B == 2 and N >= 2:
        cases.append([2 * 50, 2 * 30])                 # per-stream num_frames: HF's sequential branch
    for nf in cases:
        want = hf_timestamps(w, lay, L, P, width, np.array(nf) if isinstance(nf, list) else nf)
        assert want.shape == (B, R + 1) and want.dtype == torch.float32
        for b in range(B):
            nfb = nf[b] if isinstance(nf, list) else nf
            got = ref.token_timestamps(w[b, :, P:], P, width, nfb)
            assert torch.equal(got, want[b]), (N, kind, nf, b, got, want[b])


def test_dtw_restatement_equals_transformers_on_ties():
    g = hf()
    gen = torch.Generator().manual_seed(5)
    mats = [torch.zeros(6, 9), torch.randint(0, 4, (12, 20), generator=gen).float(), torch.randn(9, 5, generator=gen), torch.eye(7)]
    for m in mats:
        a, b = ref.dtw(-m.double().numpy()), g._dynamic_time_warping(-m.double().numpy())
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_median_filter_equals_transformers():
    g = hf()
    x = torch.randn(3, 5, 40)
    for w in (1, 3, 7, 15):
        assert torch.equal(ref.median_filter(x, w), g._median_filter(x[None], w)[0])
    assert torch.equal(ref.median_filter(x[..., :3], 7), x[..., :3])          # F <= width // 2: returned as it is


# ---- config / API plumbing ------------------------------------------------------------------------------------------------------------
def test_alignment_heads_round_trip(tmp_path):
    cfg = MedusaConfig.micro(K=4)
    assert cfg.alignment_heads is None and cfg.median_filter_width == 7
    heads = synth.synth_alignment_heads(cfg, 2)
    assert len(heads) == 2 and len({tuple(h) for h in heads}) == 2 and all(l >= cfg.decoder_layers // 2 for l, _ in heads)
    assert heads == synth.synth_alignment_heads(cfg, 2)
    import dataclasses
    c2 = dataclasses.replace(cfg, alignment_heads=heads, median_filter_width=5)
    c2.save_pretrained(str(tmp_path))
    back = MedusaConfig.from_pretrained(str(tmp_path))
    assert back.alignment_heads == heads and back.median_filter_width == 5
    # a generation_config.json wins over config.json, as for the other generation fields
    with open(os.path.join(str(tmp_path), "generation_config.json"), "w") as f:
        json.dump({"alignment_heads": [[1, 0]], "median_filter_width": 3}, f)
    back = MedusaConfig.from_pretrained(str(tmp_path))
    assert back.alignment_heads == [[1, 0]] and back.median_filter_width == 3


def test_alignment_heads_validated():
    import dataclasses
    cfg = MedusaConfig.micro(K=4)
    for bad in ([[cfg.decoder_layers, 0]], [[0, cfg.decoder_attention_heads]], [[-1, 0]], [], [[0]]):
        with pytest.raises(ValueError):
            dataclasses.replace(cfg, alignment_heads=bad)
    with pytest.raises(ValueError):
        dataclasses.replace(cfg, median_filter_width=4)


def test_generate_without_alignment_heads_raises_before_the_device():
    from whisper_medusa import WhisperMedusaModel
    cfg = MedusaConfig.micro(K=4)
    m = WhisperMedusaModel.__new__(WhisperMedusaModel)         # no engine, no device: the check comes first
    m.config = cfg
    with pytest.raises(NotImplementedError, match="alignment_heads"):
        m.generate(torch.zeros(1, cfg.num_mel_bins, cfg.n_mel_frames), return_token_timestamps=True)
    with pytest.raises(ValueError):
        m.generate(torch.zeros(1, cfg.num_mel_bins, cfg.n_mel_frames), return_token_timestamps=True,
                                                alignment_heads=[[99, 0]])
    with pytest.raises(NotImplementedError, match="logits_processor"):
        m.generate(torch.zeros(1, cfg.num_mel_bins, cfg.n_mel_frames), return_token_timestamps=True,
                                                alignment_heads=[[1, 0]], logits_processor=[lambda i, s: s])


def test_align_params_mirror_matches_the_header():
    """wm_align_params field for field against include/wm.h (names, order, C types), as tests/test_host.py does for the other structs."""
    from whisper_medusa import engine
    txt = open(os.path.join(ROOT, "include", "wm.h")).read()
    body = re.search(r"typedef struct wm_align_params \{(.*?)\} wm_align_params;", txt, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        m = re.match(r"(const int32_t\*|int32_t|float)\s+(\w+)$", decl)
        assert m, decl
        fields.append((m.group(2), m.group(1)))
    ctype = {"const int32_t*": C.POINTER(C.c_int32), "int32_t": C.c_int32, "float": C.c_float}
    assert [(n, ctype[t]) for n, t in fields] == list(engine.WmAlignParams._fields_)
    for name in ("wm_token_timestamps", "wm_get_align_probs", "wm_get_align_matrix", "wm_dtw"):
        assert name in engine.EXPORTS
