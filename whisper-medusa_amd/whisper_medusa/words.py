"""Word timestamps: the vocabulary as bytes for the engine's word grouping (``Engine.set_word_table`` / ``Engine.word_spans``,
csrc/wm_words.hip), and what generate(return_word_timestamps=True) builds around one ``word_spans`` call — the rows of text ids of every clip,
their (start, end) pairs, and the words as the Hugging Face ASR pipeline's ``return_timestamps="word"`` shapes them."""
import math
from typing import List, Optional, Sequence

import numpy as np

SPACES, UNICODE = 0, 1                                      # WM_WORDS_SPACES, WM_WORDS_UNICODE (include/wm.h)
# the languages transformers' _combine_tokens_into_words splits on characters instead of spaces, by name and by Whisper's code
UNICODE_LANGUAGES = {"chinese": "zh", "japanese": "ja", "thai": "th", "lao": "lo", "myanmar": "my", "cantonese": "yue"}


def bytes_to_unicode() -> dict:
    """GPT-2's byte -> printable code point map (what a byte-level BPE vocabulary is written in)."""
    bs = list(range(ord("!"), ord("~") + 1)) + list(range(ord("¡"), ord("¬") + 1)) + list(range(ord("®"), ord("ÿ") + 1))
    cs, n = bs[:], 0
    for b in range(256):
        if b not in bs:
            bs.append(b)
            cs.append(256 + n)
            n += 1
    return {b: chr(c) for b, c in zip(bs, cs)}


_UNICODE_TO_BYTE = {c: b for b, c in bytes_to_unicode().items()}


def language_mode(language: Optional[str]) -> int:
    """SPACES or UNICODE for a clip's language as generate() knows it: a name, a code or a ``<|xx|>`` token; None (English-only checkpoints):
    SPACES."""
    if not language:
        return SPACES
    l = str(language).strip().lower()
    if l.startswith("<|") and l.endswith("|>"):
        l = l[2:-2]
    return UNICODE if l in UNICODE_LANGUAGES or l in UNICODE_LANGUAGES.values() else SPACES


class WordTable:
    """The bytes of every text id: one uint8 blob and int32 offsets [n_text + 1]."""

    def __init__(self, token_bytes: Sequence[bytes]):
        token_bytes = [bytes(b) for b in token_bytes]
        if not token_bytes or any(len(b) == 0 for b in token_bytes):
            raise ValueError("WordTable: every text id needs at least one byte")
        self.token_bytes = token_bytes
        self.offsets = np.zeros(len(token_bytes) + 1, dtype=np.int32)
        self.offsets[1:] = np.cumsum([len(b) for b in token_bytes])
        self.blob = np.frombuffer(b"".join(token_bytes), dtype=np.uint8).copy()

    @property
    def n_text(self) -> int:
        return len(self.token_bytes)

    @classmethod
    def from_tokenizer(cls, tok, n_text: Optional[int] = None) -> "WordTable":
        """From a byte-level BPE tokenizer: ``convert_ids_to_tokens`` of every id below ``n_text`` (default ``tok.eos_token_id``) through the
        inverse of the byte-to-unicode map."""
        n_text = int(tok.eos_token_id if n_text is None else n_text)
        out = []
        for t, s in enumerate(tok.convert_ids_to_tokens(list(range(n_text)))):
            try:
                out.append(bytes(_UNICODE_TO_BYTE[c] for c in s))
            except (KeyError, TypeError):
                raise ValueError(f"WordTable.from_tokenizer: id {t} ({s!r}) is no byte-level BPE entry") from None
        return cls(out)

    def text(self, ids: Sequence[int]) -> str:
        return b"".join(self.token_bytes[int(t)] for t in ids).decode("utf-8", "replace")


def text_rows(row: Sequence[int], prompt_len: int, eos_token_id: int) -> List[tuple]:
    """The maximal runs of text ids (< eos_token_id) in the generated part of one ``sequences`` row, up to its first EOS: [(first, stop)]
    positions in the row.  With timestamp tokens that is one run per segment; without, one per clip."""
    runs, p, n = [], prompt_len, len(row)
    while p < n and row[p] != eos_token_id:
        if row[p] < eos_token_id:
            q = p
            while q < n and row[q] < eos_token_id:
                q += 1
            runs.append((p, q))
            p = q
        else:
            p += 1
    return runs


def collate(engine, table: WordTable, sequences, token_timestamps, prompt_len: int, eos_token_id: int, modes: Sequence[int],
            token_logprobs=None) -> List[List[dict]]:
    """Per clip the words of its ``sequences`` row (lists of ints) under ``token_timestamps`` (float32 [B, T]): ONE ``engine.word_spans`` call
    over the text rows of all clips.  The token at position p gets (token_timestamps[p - 1], token_timestamps[p]), the pipeline's pairing.  A word:
    ``{"text", "timestamp": (start, end), "tokens": (first, stop)[, "probability"]}`` — text decoded with errors="replace", times rounded to 2
    decimals, positions in the ``sequences`` row, probability = exp(mean log-probability of the word's tokens)."""
    tt = np.asarray(token_timestamps, dtype=np.float32)
    lp = None if token_logprobs is None else np.asarray(token_logprobs, dtype=np.float32)
    rows, md, tms, lps, where = [], [], [], [], []
    for b, row in enumerate(sequences):
        for a, z in text_rows(row, prompt_len, eos_token_id):
            rows.append(row[a:z])
            md.append(int(modes[b]))
            tms.append(np.stack([tt[b, a - 1: z - 1], tt[b, a: z]], axis=1))
            if lp is not None:
                lps.append(lp[b, a: z])
            where.append((b, a))
    words: List[List[dict]] = [[] for _ in sequences]
    spans = engine.word_spans(rows, md, tms, lps if lp is not None else None) if rows else []
    for (b, a), ids, (wf, wt, wl) in zip(where, rows, spans):
        for w in range(len(wf) - 1):
            f, s = int(wf[w]), int(wf[w + 1])
            word = {"text": table.text(ids[f:s]), "timestamp": (round(float(wt[w, 0]), 2), round(float(wt[w, 1]), 2)), "tokens": (a + f, a + s)}
            if wl is not None:
                word["probability"] = math.exp(float(wl[w]))
            words[b].append(word)
    return words
