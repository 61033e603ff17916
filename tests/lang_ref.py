"""References and cases of the per-clip language tests (include/wm.h wm_set_stream_prompts / wm_detect_language / wm_lang_pick_rows, DESIGN.md
§2l): HF's detection rule in torch (every id that is no language token masked to -inf, then argmax — WhisperGenerationMixin.detect_language), the
pick rule the engine's kernel is specified by, restated, HF's _retrieve_init_tokens row construction, restated, the tap cases, and the checkpoint
and clips of the decode tests.  tests/test_language_list_cpu.py holds — from these references alone — that the two pick rules agree on the tap
cases; the clips were chosen on the CPU with the oracle alone (`python tests/lang_ref.py --search`)."""
import numpy as np
import torch

from helpers import MedusaConfig, synth, clip_for  # noqa: F401
import scores_ref as _sr

NEG_INF = float("-inf")


# ---- the pick --------------------------------------------------------------------------------------------------------------------------------
def hf_pick(rows, lang_ids):
    """HF detect_language on rows [R, V]: `non_lang_mask[lang_ids] = False; logits[:, non_lang_mask] = -inf; argmax(-1)`, on the CPU."""
    z = torch.as_tensor(np.asarray(rows, dtype=np.float32)).clone()
    mask = torch.ones(z.shape[-1], dtype=torch.bool)
    mask[torch.as_tensor(list(lang_ids), dtype=torch.long)] = False
    z[:, mask] = -np.inf
    return z.argmax(-1).numpy().astype(np.int32)


def pick_restated(rows, lang_ids):
    """The contract of k_lang_pick: among the candidates the largest value, among equal values the smallest token id (whatever their order)."""
    out = []
    for row in np.asarray(rows, dtype=np.float32):
        best = None
        for t in lang_ids:
            v = float(row[t])
            if best is None or v > best[0] or (v == best[0] and t < best[1]):
                best = (v, int(t))
        out.append(best[1])
    return np.asarray(out, dtype=np.int32)


# ---- HF _retrieve_init_tokens, restated ------------------------------------------------------------------------------------------------------
def init_token_rows(cfg, languages, task="transcribe", timestamps=False, prompt_ids=None):
    """One row of decoder input ids per clip as HF builds them for `language=[...]`: init_tokens = [<|startoftranscript|>], one copy per language
    with that language's id appended, then the task id, then <|notimestamps|> unless return_timestamps; `prompt_ids` (the previous-text part, shared)
    in front of every row (_prepare_decoder_input_ids).  `languages`: token strings ('<|de|>')."""
    rows = []
    for l in languages:
        r = [cfg.decoder_start_token_id, cfg.lang_to_id[l], cfg.task_to_id[task]]
        if not timestamps:
            r.append(cfg.no_timestamps_token_id)
        rows.append([int(t) for t in (prompt_ids or [])] + r)
    return rows


# ---- tap cases (test 1 of tests/test_gpu_language_list.py) -----------------------------------------------------------------------------------
TAP_V = (516, 51865)
TAP_N = (1, 3, 64, 65, 100, 256)        # lane and wave edges of a 256-thread block
TAP_R = (1, 15, 16, 33)                 # one row, a full row group of the tap, one more, three groups


def tap_lang_ids(V, n):
    """n distinct candidate ids in an UNSORTED order; for Whisper's vocabulary in its language block near the top (50259 ...)."""
    base = 50259 if V >= 51865 else 200
    assert base + 300 <= V
    ids = [base + i for i in range(n)]
    rng = np.random.default_rng(1000 + n)
    rng.shuffle(ids)
    return [int(t) for t in ids]


def tap_rows(V, R, lang_ids):
    """R rows [R, V] of fp32 noise, each with a far larger value on an id that is no candidate, and by row index r % 6:
    0 the maximum at the first candidate of the list, 1 at the last, 2 an exact tie between two candidates of one wave (different lanes),
    3 an exact tie between candidates of different waves (n > 64; else of different lanes), 4 a third of the candidates at -inf (the rest
    noise), 5 a tie of three with one of them the smallest id of all, half of the others at -inf."""
    n = len(lang_ids)
    rng = np.random.default_rng(7 * V + 31 * R + n)
    x = rng.standard_normal((R, V)).astype(np.float32)
    other = [t for t in (0, 1, V - 1, lang_ids[0] - 1 if lang_ids[0] > 0 else V - 2) if t not in set(lang_ids)]
    for r in range(R):
        for t in other:
            x[r, t] = 1.0e4 + r                                 # not a language token: must be ignored
        kind, top = r % 6, np.float32(9.0 + 0.125 * r)
        if kind == 0:
            x[r, lang_ids[0]] = top
        elif kind == 1:
            x[r, lang_ids[-1]] = top
        elif kind == 2:
            i, j = (r * 5) % min(n, 64), (r * 5 + 37) % min(n, 64)
            x[r, lang_ids[i]] = x[r, lang_ids[j]] = top
        elif kind == 3:
            i = (r * 3) % min(n, 64)
            j = i + 64 * (1 + r % 3) if i + 64 * (1 + r % 3) < n else (i + 1) % n
            x[r, lang_ids[i]] = x[r, lang_ids[j]] = top
        elif kind == 4:
            for k in range(0, n if n > 1 else 0, 3):
                x[r, lang_ids[k]] = NEG_INF
        else:
            for k in range(1, n, 2):
                x[r, lang_ids[k]] = NEG_INF
            lo = min(lang_ids)
            for t in {lo, lang_ids[0], lang_ids[-1]}:
                x[r, t] = top
    return x


# ---- the checkpoint and clips of the decode tests --------------------------------------------------------------------------------------------
# A synthetic checkpoint prefers ONE of any three ids behind <|startoftranscript|> by far more than its clips differ (with the language ids 20 / 21 / 22
# of tests/test_gpu_features.py every clip of every seed 43 .. 79 detects the same language, 1.5 - 2.0 above the runner-up).  So the language IDS
# were chosen on the CPU, with the oracle alone (`python tests/lang_ref.py --search`): on the checkpoint MIX_SEED, among the ids 40 .. 899 whose value
# in that row varies most between clips 0 .. 7, the triple under which most clips clear 30 x MARGIN and all three languages win somewhere; then four
# clips that cover the three winners.  Written down: the tests run on these whatever a host's oracle arithmetic does to the search
LANGS = {"<|en|>": 60, "<|de|>": 63, "<|fr|>": 748}
TASKS = {"transcribe": 30, "translate": 31}
MARGIN = 1e-3                   # every clip's best language at least this far above its runner-up (what the existing detection test allows for)
MIX_SEED = 43
MIX_CLIPS = (0, 5, 1, 3)        # the search's margins: en 0.035, de 0.122, fr 0.099, fr 0.134
MIX_LIST = ("<|de|>", "<|en|>", "<|de|>", "<|fr|>")      # the explicit list of the tests: language=[a, b, a, c], not what the clips detect


def mix_cfg():
    """tests/scores_ref.py micro_ts (a vocabulary that ends in Whisper's timestamp block) made multilingual as in
    tests/test_gpu_features.py::test_language_detection_groups_clips."""
    cfg = _sr.micro_ts("base_head", K=4)
    cfg.is_multilingual = True
    cfg.lang_to_id = dict(LANGS)
    cfg.task_to_id = dict(TASKS)
    return cfg


def mix_checkpoint(seed=None):
    cfg = mix_cfg()
    return cfg, _sr.ts_state_dict(cfg, MIX_SEED if seed is None else seed)


def lang_values(orc, cfg, enc):
    """The base logits of the language tokens behind <|startoftranscript|> on the encoder output `enc` [S, d]: {token string: value}."""
    z = orc.decoder_pass(orc.new_state(enc), [cfg.decoder_start_token_id], 0, disable_medusa=True)[0, 0]
    return {k: float(z[v]) for k, v in cfg.lang_to_id.items()}


def mix_guard(orc, cfg, encs):
    """What the decode tests ask of their clips, on the reference alone: every clip's best language at least MARGIN above its runner-up, and at
    least two different languages among the clips.  `encs`: one encoder output per clip.  Returns the clips' languages (token strings)."""
    langs = []
    for b, enc in enumerate(encs):
        vals = sorted(lang_values(orc, cfg, enc).items(), key=lambda kv: -kv[1])
        assert vals[0][1] - vals[1][1] >= MARGIN, ("a clip's best language is under MARGIN above its runner-up", b, vals)
        want = orc.detect_language(enc, list(cfg.lang_to_id.values()))
        assert cfg.lang_to_id[vals[0][0]] == want
        langs.append(vals[0][0])
    assert len(set(langs)) >= 2, ("the clips are all of one language", langs)
    return langs


def oracle_encs(orc, cfg, clips):
    import sample_ref as _S
    return [_S.oracle_encode(orc, cfg, c) for c in clips]


if __name__ == "__main__":
    import sys
    if "--search" in sys.argv:
        import itertools
        from oracle.whisper_medusa_oracle import Oracle
        cfg, sd = mix_checkpoint()
        orc = Oracle(cfg, sd, sim="bf16")
        Z = []
        for c in range(8):
            enc = oracle_encs(orc, cfg, [c])[0]
            Z.append(orc.decoder_pass(orc.new_state(enc), [cfg.decoder_start_token_id], 0, disable_medusa=True)[0, 0].numpy().copy())
        Z = np.stack(Z)
        top = sorted([int(i) for i in np.argsort(-Z.std(0)) if 40 <= i < 900][:120])         # the 120 ids that vary most between the clips
        best = None
        for tri in itertools.combinations(top, 3):
            sub = Z[:, list(tri)]
            srt = np.sort(sub, 1)
            margin, win = srt[:, 2] - srt[:, 1], sub.argmax(1)
            good = [c for c in range(len(Z)) if margin[c] >= 30 * MARGIN]
            if len(good) >= 4 and len({int(win[c]) for c in good}) == 3:
                key = (len(good), float(min(margin[c] for c in good)))
                if best is None or key > best[0]:
                    best = (key, tri, [(c, int(win[c]), round(float(margin[c]), 4)) for c in range(len(Z))])
        print("ids (en, de, fr) =", best[1], " per clip (clip, winner, margin):", best[2])
