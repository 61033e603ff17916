"""Reference code of the token-timestamp tests (no test in here).

(i)  A plain torch / numpy restatement of steps 2-6 of HF WhisperGenerationMixin._extract_token_timestamps for ONE stream: z-score over the
     rows, median filter, mean over the heads, dynamic time warping, jump times.  tests/test_token_timestamps_cpu.py pins it to
     transformers' own code.
(ii) RecordingOracle: oracle.Oracle whose `_attend` keeps the softmax weights of the cross-attention calls of a teacher-forced
     decoder_pass (the oracle file itself is not edited)."""
import numpy as np
import torch

from oracle.whisper_medusa_oracle import Oracle


# ---- (i) steps 2-6 -----------------------------------------------------------------------------------------------------------------
def median_filter(x: torch.Tensor, width: int) -> torch.Tensor:
    """HF _median_filter along the last dimension of [A, N, F]: reflect padding, sorted window's middle; skipped when F <= width // 2."""
    pad = width // 2
    if x.shape[-1] <= pad:
        return x
    xp = torch.nn.functional.pad(x[None], (pad, pad, 0, 0), mode="reflect")[0]
    return xp.unfold(-1, width, 1).sort()[0][..., pad]


def align_matrix(weights: torch.Tensor, width: int = 7, dtype=torch.float32) -> torch.Tensor:
    """Steps 2-4: weights [A, N, F] (already cropped to F frames) -> matrix [N, F], evaluated in `dtype`."""
    w = weights.to(dtype)
    std = torch.std(w, dim=-2, keepdim=True, unbiased=False)
    mean = torch.mean(w, dim=-2, keepdim=True)
    w = (w - mean) / std
    w = median_filter(w, width)
    return w.mean(dim=0)


def dtw(cost: np.ndarray):
    """Step 5, HF _dynamic_time_warping restated: `cost` is float64 [N, F] (the NEGATED matrix); the table is float32, every sum is
    formed in float64 and rounded to float32 on the store; strict `<` tie rules; back-trace from (N, F)."""
    N, F = cost.shape
    c = np.full((N + 1, F + 1), np.inf, dtype=np.float32)
    tr = -np.ones((N + 1, F + 1), dtype=np.int8)
    c[0, 0] = 0
    for j in range(1, F + 1):
        for i in range(1, N + 1):
            c0, c1, c2 = c[i - 1, j - 1], c[i - 1, j], c[i, j - 1]
            if c0 < c1 and c0 < c2:
                cc, t = c0, 0
            elif c1 < c0 and c1 < c2:
                cc, t = c1, 1
            else:
                cc, t = c2, 2
            c[i, j] = cost[i - 1, j - 1] + cc
            tr[i, j] = t
    tr[0, :] = 2
    tr[:, 0] = 1
    i, j = N, F
    text, time = [], []
    while i > 0 or j > 0:
        text.append(i - 1)
        time.append(j - 1)
        t = tr[i, j]
        if t == 0:
            i -= 1
            j -= 1
        elif t == 1:
            i -= 1
        else:
            j -= 1
    return np.array(text)[::-1], np.array(time)[::-1]


def jump_times(text_indices: np.ndarray, time_indices: np.ndarray, time_precision: float = 0.02) -> np.ndarray:
    jumps = np.pad(np.diff(text_indices), (1, 0), constant_values=1).astype(bool)
    return time_indices[jumps] * time_precision


def timestamps_from_matrix(matrix: torch.Tensor, n_prompt: int, total_len: int = None, time_precision: float = 0.02, dtw_fn=None) -> torch.Tensor:
    """Steps 5-6 on matrix [N, F] -> float32 [n_prompt + N + 1] (padded to total_len with the last value).  dtw_fn: the DTW to use
    (default: the restatement above; the tests also pass transformers' own)."""
    f = dtw if dtw_fn is None else dtw_fn
    text, time = f(-matrix.detach().cpu().double().numpy())
    jt = jump_times(text, time, time_precision)
    out = torch.cat([torch.zeros(n_prompt), torch.tensor(jt), torch.tensor([jt[-1]])]).to(torch.float32)
    if total_len is not None and total_len > out.numel():
        out = torch.cat([out, out[-1:].expand(total_len - out.numel())])
    return out


def token_timestamps(weights: torch.Tensor, n_prompt: int, width: int = 7, num_frames=None, time_precision: float = 0.02, dtw_fn=None) -> torch.Tensor:
    """Steps 2-6 for one stream.  weights [A, N, n_ctx]: softmax rows of input positions n_prompt .. T-2 (N = G - 1).  N == 0: zeros of
    length n_prompt + 1.  N == 1 is HF's 0 / 0 case: the matrix is NaN, every comparison of the DTW fails, the path walks left along the one row
    and the only jump sits at frame 0 — zeros, returned here without the arithmetic."""
    A, N, S = weights.shape
    if N <= 1:
        return torch.zeros(n_prompt + N + 1, dtype=torch.float32)
    F = S if num_frames is None else min(int(num_frames) // 2, S)
    return timestamps_from_matrix(align_matrix(weights[..., :F], width), n_prompt, None, time_precision, dtw_fn)


# ---- (ii) recording oracle ---------------------------------------------------------------------------------------------------------
class RecordingOracle(Oracle):
    """Keeps the softmax weights of every cross-attention call (`mask is None`, keys == n_ctx) in self.cross: one [H, T, n_ctx] per
    decoder layer and pass, in call order."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.cross = []
        self.recording = False

    def _attend(self, q, k, v, mask=None, round_p=False, dec=False):
        if self.recording and mask is None and dec and k.shape[1] == self.cfg.max_source_positions:
            self.cross.append(torch.softmax(q @ k.transpose(1, 2), dim=-1))
        return super()._attend(q, k, v, mask=mask, round_p=round_p, dec=dec)

    @torch.no_grad()
    def alignment_weights(self, enc: torch.Tensor, ids, n_prompt: int, heads) -> torch.Tensor:
        """Teacher-forced pass over ids[:-1] -> weights [A, N, n_ctx] of the alignment heads, rows n_prompt .. T-2."""
        st = self.new_state(enc)
        self.cross, self.recording = [], True
        try:
            self.decoder_pass(st, list(ids[:-1]), 0, True)
        finally:
            self.recording = False
        per_layer = self.cross[: self.cfg.decoder_layers]           # (a Medusa-Block extra layer comes after them and is never an alignment layer)
        return torch.stack([per_layer[l][h, n_prompt:] for l, h in heads])
