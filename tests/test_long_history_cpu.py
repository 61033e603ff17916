"""The proof that tests/test_gpu_long_history.py can fail, on the oracle alone (no GPU).

At n_tgt = 448 a self-attention that loses its second 32-key step, reads a stale register set in its place, or loses one key must leave the
decoder-logits contract (max |d| <= 6e-2, mean |d| <= 4e-3) by a wide margin, while the contract oracle itself stays inside it against the fp32
oracle; and the decode runs to the length limit sit on no decision whose margin is near the tie tolerances."""
import pytest
import torch

import long_history as LH
from long_history import Oracle, MutantOracle, ACCEPT_TYPICAL, ACCEPT_GREEDY

ACTS = ["hilo", "f16"]


@pytest.fixture(scope="module")
def walks():
    """(heads, act) -> the teacher-forced aligned walk of the true contract oracle, its three mutants and the fp32 oracle; computed once."""
    cache = {}

    def get(heads, act):
        if (heads, act) not in cache:
            cfg, sd = LH.checkpoint(heads)
            ids, tiles = LH.walk_ids(), LH.tiles_aligned()
            true = Oracle(cfg, sd, sim="bf16", act=act)
            enc = true.encode(LH.features(cfg, LH.WALK_CLIP))
            z = dict(true=LH.oracle_walk(true, enc, ids, tiles), fp32=LH.oracle_walk(Oracle(cfg, sd, sim="fp32"), enc, ids, tiles))
            for m in LH.MUTANTS:
                z[m] = LH.oracle_walk(MutantOracle(cfg, sd, sim="bf16", act=act, mutant=m), enc, ids, tiles)
            cache[(heads, act)] = (cfg, tiles, z)
        return cache[(heads, act)]
    return get


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("heads", LH.HEADS)
def test_mutants_leave_the_logits_contract_and_the_contract_oracle_does_not(walks, heads, act):
    """Walk of 448 ids in 16-row tiles, checkpoint seed 51 with the self-attention q_proj x 4, clip 2; base head for the mutants (the GPU test
    bounds all K + 1 heads: a subset), all heads for the bf16-vs-fp32 gap.  Measured, max |d| / mean |d| over the whole walk (and, for the
    step-sized mutants, the smallest per-tile maximum over the tiles behind key 160):

      heads / act           bf16 vs fp32 (all heads)   dropped step             stale step               dropped key
      base_head / hilo      1.16e-2 / 9.2e-4           1.13 / 4.26e-2 (0.333)   1.13 / 4.84e-2 (0.341)   0.723 / 1.98e-3
      base_head / f16       1.20e-2 / 9.9e-4           1.12 / 4.25e-2 (0.333)   1.13 / 4.84e-2 (0.340)   0.721 / 2.10e-3
      medusa_block / hilo   2.12e-2 / 1.72e-3          1.14 / 4.25e-2 (0.340)   1.15 / 4.83e-2 (0.337)   0.695 / 1.97e-3
      medusa_block / f16    2.08e-2 / 1.81e-3          1.14 / 4.24e-2 (0.340)   1.14 / 4.83e-2 (0.337)   0.694 / 2.09e-3

    Logit standard deviation 1.55 (Block: 1.53).  Bounds: 6e-2 / 4e-3; 5 x = 0.30 / 2e-2.
    """
    cfg, tiles, z = walks(heads, act)
    assert z["true"].shape == (cfg.medusa_num_heads + 1, LH.N_TGT, cfg.vocab_size) and tiles[-1][0] + tiles[-1][1] == LH.N_TGT
    # (c) the contract oracle against the fp32 oracle: inside the contract, all heads
    mx, mn, _, _ = LH.tile_stats((z["true"] - z["fp32"]).abs(), tiles)
    fig = {"bf16 vs fp32": (mx, mn), "logit std": float(z["true"][0].std())}
    assert mx <= LH.MAX_D and mn <= LH.MEAN_D, (heads, act, mx, mn)
    for m in LH.MUTANTS:
        d = (z[m][0] - z["true"][0]).abs()[None]
        mx, mn, tmx, _ = LH.tile_stats(d, tiles)
        behind = [x for (p, t), x in zip(tiles, tmx) if p >= LH.MUT_HI]
        fig[m] = (mx, mn, min(behind))
        # rows whose history ends before the mutated keys see no fault: the difference comes from the keys >= 128 alone
        assert float(d[:, : LH.MUT_LO].max()) == 0.0
        # (a) the whole-walk maximum leaves the bound by 5 x, reached on tiles whose history passes the mutated keys
        assert max(behind) >= 5 * LH.MAX_D, (heads, act, m, mx)
        if m != "dropped key":
            # (b) the step-sized faults also leave the mean bound by 5 x — and EVERY tile behind them leaves the max bound by 5 x
            assert mn >= 5 * LH.MEAN_D, (heads, act, m, mn)
            assert min(behind) >= 5 * LH.MAX_D, (heads, act, m, min(behind))
    print(f"long history [{heads}, {act}]: " + "; ".join(f"{k}: " + (" / ".join(f"{x:.3g}" for x in v) if isinstance(v, tuple) else f"{v:.3g}")
                                                          for k, v in fig.items()))


def test_ragged_tiles_straddle_every_128_key_boundary():
    tiles = LH.tiles_ragged()
    assert tiles[-1][0] + tiles[-1][1] == LH.N_TGT and sum(t for _, t in tiles) == LH.N_TGT
    assert any(p % 16 for p, _ in tiles)
    for edge in (128, 256, 384):
        assert any(p < edge < p + t for p, t in tiles), edge          # one tile with rows on both sides
    assert {t for _, t in tiles} >= set(LH.RAGGED)


def test_length_penalty_is_finite_to_the_limit():
    """fp32 pow(factor, cur_len - start) at the last position: the golden recipe's 1.3 is inf there, the factor used here is not."""
    n = LH.N_TGT - LH.EXP_DECAY[0] - 2
    assert torch.isfinite(torch.tensor(LH.EXP_DECAY[1], dtype=torch.float32) ** n)
    assert torch.isinf(torch.tensor(1.3, dtype=torch.float32) ** n)


@pytest.mark.parametrize("mode", [ACCEPT_TYPICAL, ACCEPT_GREEDY], ids=["typical", "greedy"])
@pytest.mark.parametrize("heads", LH.HEADS)
def test_decode_runs_to_the_limit_sit_on_no_near_tie(heads, mode):
    """The (checkpoint seed, clip) of test_gpu_long_history.py::test_decode_runs_to_the_length_limit: over the oracle's own run (its own encoder
    output, which the GPU test hands to the engine), in both act contracts, the smallest top-2 logit margin and the smallest |p_c - thr| / thr of
    the decisions that reach the output are >= 10 x the tie tolerances (5e-4, 2e-3) — a run has no excuse to need a followed tie.  Measured
    (f16 / hilo):

      base_head, typical      seed 3069 clip 8    447 ids, 177 iterations   logit margin 6.31e-3 / 6.57e-3   |p_c - thr| / thr 4.34e-2 / 4.23e-2
      base_head, greedy       seed 168 clip 11    444 ids, 220 iterations   logit margin 5.52e-3 / 5.21e-3
      medusa_block, typical   seed 322 clip 7     445 ids, 195 iterations   logit margin 5.24e-3 / 5.24e-3   |p_c - thr| / thr 2.51e-2 / 2.45e-2
      medusa_block, greedy    seed 121 clip 5     444 ids, 221 iterations   logit margin 5.35e-3 / 5.76e-3

    (Exact-match acceptance takes no Medusa candidate on these checkpoints: two ids per iteration.)"""
    seed, clip = LH.DECODE_RUNS[(heads, mode)]
    cfg, sd = LH.checkpoint(heads, seed)
    gp = LH.limit_gen_params(cfg, mode)
    K = cfg.medusa_num_heads
    for act in ACTS:
        orc = Oracle(cfg, sd, sim="bf16", act=act)
        enc = orc.encode(LH.features(cfg, clip))
        ids, m_logit, m_rel, n_it = LH.decode_with_margins(orc, enc, gp)
        print(f"long history decode [{heads}, mode {mode}, {act}]: seed {seed} clip {clip}: {len(ids)} ids in {n_it} iterations, smallest logit margin "
              f"{m_logit:.4g}, smallest |p_c - thr| / thr {m_rel:.4g}")
        assert LH.N_TGT - K - 1 <= len(ids) <= LH.N_TGT
        assert m_logit >= 10 * LH.TOL_LOGIT and m_rel >= 10 * LH.TOL_REL_P, (heads, mode, act, m_logit, m_rel)
        if act == "f16":
            assert ids == orc.decode(enc, gp).ids           # the restated loop is the oracle's
