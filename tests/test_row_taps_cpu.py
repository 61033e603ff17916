"""What the parity taps of whisper_medusa/engine.py hand to the library, without a library: an Engine made by ``Engine.__new__`` with a ``cfg`` and
a recording stand-in for ``lib``.  Every ``wm_*`` attribute of the stand-in copies what its pointer arguments point at, writes a mark through every
output pointer and returns 0.  Per tap the test holds R, Tmax, the lengths, the zero-padded prefix matrix, the per-row extra (probe / target / key
masked to 64 bits), whether the timestamp pointer is null, the struct fields, the output buffers' dtypes and shapes, that the repetition rules were
set first and the cache stamp renewed, and the texts of the shape errors.  No GPU."""
import ctypes as C
import re

import numpy as np
import pytest

from whisper_medusa import MedusaConfig, GenParams
from whisper_medusa import engine as E

V = 516
M64 = 2 ** 64 - 1


def _obj(ref, cls):
    """the struct behind a byref / pointer argument as a dict of its fields (None: a null pointer)"""
    if ref is None:
        return None
    o = ref._obj if hasattr(ref, "_obj") else ref.contents
    assert isinstance(o, cls), type(o)
    return {n: getattr(o, n) for n, _ in o._fields_}


def _rd(p, n, ct):
    assert isinstance(p, C.POINTER(ct)), type(p)
    return np.array(p[:n], dtype=np.dtype(ct))


def _mark(p, n, ct, v):
    assert isinstance(p, C.POINTER(ct)), type(p)
    for i in range(n):
        p[i] = v


def _gen(ref):
    g = _obj(ref, E.WmGenParams)
    g["prompt"] = g["prompt"][: g["prompt_len"]]
    g["suppress"] = g["suppress"][: g["n_suppress"]]
    g["begin_suppress"] = g["begin_suppress"][: g["n_begin_suppress"]]
    return g


class Lib:
    """the recording stand-in: calls = [(name, what the library saw)]"""

    def __init__(self, eng):
        self.eng, self.calls, self.stale = eng, [], object()

    def __getattr__(self, name):
        if not name.startswith("wm_"):
            raise AttributeError(name)
        see = getattr(self, "see_" + name[3:], lambda *a: {})

        def call(h, *a):
            rec = see(*a)
            rec["stamp_renewed"] = self.eng._kv_stamp is not self.stale
            self.calls.append((name, rec))
            return 0
        return call

    @staticmethod
    def see_set_repeat_rules(rp):
        return dict(rp=_obj(rp, E.WmRepeatParams))

    @staticmethod
    def _rows(R, x, pre, Tmax, lens):
        return dict(R=R, Tmax=Tmax, x=_rd(x, R * V, C.c_float).reshape(R, V), pre=_rd(pre, R * Tmax, C.c_int32).reshape(R, Tmax),
                    lens=_rd(lens, R, C.c_int32))

    def see_select_rows(self, g, ts, R, x, pre, Tmax, lens, probe, am, pp, H, fo):
        _mark(am, R, C.c_int32, 11); _mark(pp, R, C.c_float, 12.5); _mark(H, R, C.c_float, 13.5); _mark(fo, R, C.c_int32, 14)
        return dict(self._rows(R, x, pre, Tmax, lens), g=_gen(g), ts=_obj(ts, E.WmTimestampParams), extra=_rd(probe, R, C.c_int32))

    def see_sample_rows(self, g, ts, sp, R, x, pre, Tmax, lens, keys, tok, val, fo):
        _mark(tok, R, C.c_int32, 21); _mark(val, R, C.c_float, 22.5); _mark(fo, R, C.c_int32, 23)
        return dict(self._rows(R, x, pre, Tmax, lens), g=_gen(g), ts=_obj(ts, E.WmTimestampParams), sp=_obj(sp, E.WmSampleParams),
                    extra=_rd(keys, R, C.c_uint64))

    def see_filter_rows(self, g, ts, sp, f, R, x, pre, Tmax, lens, keys, thr, kept, fo, tok, val):
        _mark(thr, R, C.c_float, 31.5); _mark(kept, R, C.c_int32, 32); _mark(fo, R, C.c_int32, 33); _mark(tok, R, C.c_int32, 34)
        _mark(val, R, C.c_float, 35.5)
        return dict(self._rows(R, x, pre, Tmax, lens), g=_gen(g), ts=_obj(ts, E.WmTimestampParams), sp=_obj(sp, E.WmSampleParams),
                    f=_obj(f, E.WmSampleFilter), extra=_rd(keys, R, C.c_uint64))

    def see_score_rows(self, g, ts, R, x, pre, Tmax, lens, tgt, out):
        _mark(out, R, C.c_float, 41.5)
        return dict(self._rows(R, x, pre, Tmax, lens), g=_gen(g), ts=_obj(ts, E.WmTimestampParams), extra=_rd(tgt, R, C.c_int32))

    def see_topk_rows(self, g, ts, R, x, pre, Tmax, lens, tgt, k, tid, tlp, rk):
        _mark(tid, R * k, C.c_int32, 51); _mark(tlp, R * k, C.c_float, 52.5); _mark(rk, R, C.c_int32, 53)
        return dict(self._rows(R, x, pre, Tmax, lens), g=_gen(g), ts=_obj(ts, E.WmTimestampParams), extra=_rd(tgt, R, C.c_int32), k=k)

    def see_seq_bias_rows(self, sb, R, x, pre, Tmax, lens, out):
        _mark(out, R * V, C.c_float, 61.5)
        s = _obj(sb, E.WmSeqBiasParams)
        n = s["n"]
        el = _rd(s["lens"], n, C.c_int32)
        return dict(self._rows(R, x, pre, Tmax, lens), n=n, elens=el, etok=_rd(s["tokens"], int(el.sum()), C.c_int32), ebias=_rd(s["bias"], n, C.c_float))

    @staticmethod
    def see_lang_pick_rows(R, x, ids, n, out):
        _mark(out, R, C.c_int32, 71)
        return dict(R=R, x=_rd(x, R * V, C.c_float).reshape(R, V), ids=_rd(ids, n, C.c_int32), n=n)

    @staticmethod
    def see_beam_rows(g, ts, bp, G, S, x, pre, Tmax, plen, init, cv, cb, ct, bi, steps, fi, fl, fs, fset, ri, rl, rs):
        b = _obj(bp, E.WmBeamParams)
        n = b["num_beams"]
        Bs = G * n
        for p, cnt, t, v in ((cv, S * G * 2 * n, C.c_float, 80.5), (cb, S * G * 2 * n, C.c_int32, 81), (ct, S * G * 2 * n, C.c_int32, 82),
                             (bi, S * Bs, C.c_int32, 83), (steps, G, C.c_int32, 84), (fi, Bs * Tmax, C.c_int32, 85), (fl, Bs, C.c_int32, 86),
                             (fs, Bs, C.c_float, 87.5), (fset, Bs, C.c_int32, 88), (ri, Bs * Tmax, C.c_int32, 89), (rl, Bs, C.c_int32, 90),
                             (rs, Bs, C.c_float, 91.5)):
            _mark(p, cnt, t, v)
        return dict(g=_gen(g), ts=_obj(ts, E.WmTimestampParams), bp=b, G=G, S=S, Tmax=Tmax, plen=plen, x=_rd(x, S * Bs * V, C.c_float).reshape(S, G, n, V),
                    pre=_rd(pre, Bs * Tmax, C.c_int32).reshape(Bs, Tmax), init=None if init is None else _rd(init, Bs, C.c_float))

    @staticmethod
    def _tokens(B, tok, Tmax, lens, npr):
        return dict(B=B, Tmax=Tmax, tok=_rd(tok, B * Tmax, C.c_int32).reshape(B, Tmax), lens=_rd(lens, B, C.c_int32), npr=_rd(npr, B, C.c_int32))

    def see_score_tokens(self, g, ts, sp, B, tok, Tmax, lens, npr, out, nsp, ms):
        _mark(out, B * Tmax, C.c_float, 101.5)
        if nsp is not None:
            _mark(nsp, B, C.c_float, 102.5)
        ms._obj.value = 103.5
        return dict(self._tokens(B, tok, Tmax, lens, npr), g=_gen(g), ts=_obj(ts, E.WmTimestampParams), sp=_obj(sp, E.WmScoreParams), ns_null=nsp is None)

    def see_score_tokens_topk(self, g, ts, sp, B, tok, Tmax, lens, npr, k, out, nsp, tid, tlp, rk, ms):
        _mark(out, B * Tmax, C.c_float, 111.5); _mark(tid, B * Tmax * k, C.c_int32, 112); _mark(tlp, B * Tmax * k, C.c_float, 113.5)
        _mark(rk, B * Tmax, C.c_int32, 114)
        if nsp is not None:
            _mark(nsp, B, C.c_float, 115.5)
        ms._obj.value = 116.5
        return dict(self._tokens(B, tok, Tmax, lens, npr), g=_gen(g), ts=_obj(ts, E.WmTimestampParams), sp=_obj(sp, E.WmScoreParams), ns_null=nsp is None, k=k)


@pytest.fixture()
def rig():
    eng = E.Engine.__new__(E.Engine)
    eng.cfg = MedusaConfig.micro(vocab=V)
    eng.h = C.c_void_p(1)
    eng.lib = Lib(eng)
    eng._kv_stamp = eng.lib.stale
    yield eng, eng.lib
    eng.h = None                    # (nothing to destroy)


def gp_of(kind):
    """plain / ts (timestamp rules) / rep (repetition rules alone) / ts_rep"""
    kw = {}
    if "ts" in kind:
        kw.update(timestamps=True, no_timestamps_token_id=400, max_initial_timestamp_index=5 if kind == "ts" else None)
    if "rep" in kind:
        kw.update(repetition_penalty=1.25, no_repeat_ngram_size=3)
    return GenParams(prompt=[401, 9] if "ts" not in kind else [398], eos_token_id=397, pad_token_id=396, suppress_tokens=[3, 40],
                     begin_suppress_tokens=[7], max_length=50, hard_max_length=60, exp_decay=(2, 1.0625), posterior_threshold=0.25,
                     posterior_alpha=0.5, temperature=0.5, accept_mode=1, vanilla=True, **kw)


KINDS = ["plain", "ts", "rep", "ts_rep"]
PRE = [[5, 6, 7], [1], [2, 3, 4, 5, 6]]
PRE_M = np.array([[5, 6, 7, 0, 0], [1, 0, 0, 0, 0], [2, 3, 4, 5, 6]], dtype=np.int32)
ROWS = np.asfortranarray(np.random.default_rng(5).standard_normal((3, V)))           # float64, not C-contiguous: the tap converts
KEYS = [-1, 2 ** 64 + 5, 7]
KEYS_M = np.array([M64, 5, 7], dtype=np.uint64)


def check_proc(lib, name, gp, ts_expected):
    """the repetition rules were set first, then the one tap call with a renewed stamp; returns what that call saw"""
    assert [c[0] for c in lib.calls] == ["wm_set_repeat_rules", name]
    rp = lib.calls[0][1]["rp"]
    assert rp == (dict(repetition_penalty=1.25, no_repeat_ngram_size=3) if gp.repeat_rules else None)
    rec = lib.calls[1][1]
    assert rec["stamp_renewed"]
    g = rec["g"]
    assert g["prompt"] == list(gp.prompt) and g["prompt_len"] == len(gp.prompt) and (g["eos_token_id"], g["pad_token_id"]) == (397, 396)
    assert g["suppress"] == [3, 40] and g["begin_suppress"] == [7] and (g["max_length"], g["hard_max_length"]) == (50, 60)
    assert (g["exp_decay_start"], g["exp_decay_factor"]) == (2, 1.0625) and (g["posterior_threshold"], g["posterior_alpha"]) == (0.25, 0.5)
    assert (g["temperature"], g["accept_mode"], g["vanilla"], g["begin_index"], g["force_accept"]) == (0.5, 1, 1, len(gp.prompt), -1)
    if ts_expected:
        mit = gp.max_initial_timestamp_index
        assert rec["ts"] == dict(timestamp_begin=int(gp.no_timestamps_token_id) + 1, no_timestamps_token_id=int(gp.no_timestamps_token_id),
                                 max_initial_timestamp_index=-1 if mit is None else mit, begin_index=len(gp.prompt))
    else:
        assert rec["ts"] is None
    return rec


def check_rows(rec):
    assert rec["R"] == 3 and rec["Tmax"] == 5 and rec["lens"].tolist() == [3, 1, 5]
    assert np.array_equal(rec["pre"], PRE_M) and np.array_equal(rec["x"], ROWS.astype(np.float32))


def check_out(a, dtype, shape, mark):
    assert isinstance(a, np.ndarray) and a.dtype == dtype and a.shape == shape and (a == mark).all(), (a.dtype, a.shape)


@pytest.mark.parametrize("kind", KINDS)
def test_select_rows(rig, kind):
    eng, lib = rig
    gp = gp_of(kind)
    out = eng.select_rows(gp, ROWS, PRE, [4, 5, 6])
    rec = check_proc(lib, "wm_select_rows", gp, ts_expected=kind != "rep")       # the one exception: no rules at all -> the timestamp struct all the same
    check_rows(rec)
    assert rec["extra"].tolist() == [4, 5, 6]
    assert list(out) == ["argmax", "p_probe", "entropy", "ts_forced"]
    check_out(out["argmax"], np.int32, (3,), 11); check_out(out["p_probe"], np.float32, (3,), 12.5)
    check_out(out["entropy"], np.float32, (3,), 13.5); check_out(out["ts_forced"], np.int32, (3,), 14)


@pytest.mark.parametrize("kind", KINDS)
def test_sample_rows(rig, kind):
    eng, lib = rig
    gp = gp_of(kind)
    out = eng.sample_rows(gp, ROWS, PRE, KEYS, 0.75, -3)
    rec = check_proc(lib, "wm_sample_rows", gp, ts_expected="ts" in kind)
    check_rows(rec)
    assert np.array_equal(rec["extra"], KEYS_M)
    sp = rec["sp"]
    assert (sp["temperature"], sp["seed"], sp["n_keys"]) == (0.75, 2 ** 64 - 3, 0) and not sp["stream_keys"]
    assert list(out) == ["token", "value", "ts_forced"]
    check_out(out["token"], np.int32, (3,), 21); check_out(out["value"], np.float32, (3,), 22.5); check_out(out["ts_forced"], np.int32, (3,), 23)


@pytest.mark.parametrize("kind", KINDS)
def test_filter_rows(rig, kind):
    eng, lib = rig
    gp = gp_of(kind)
    out = eng.filter_rows(gp, ROWS, PRE, KEYS, 0.75, 2 ** 64 + 9, top_k=4, top_p=0.5, min_p=0.25)
    rec = check_proc(lib, "wm_filter_rows", gp, ts_expected="ts" in kind)
    check_rows(rec)
    assert np.array_equal(rec["extra"], KEYS_M)
    sp = rec["sp"]
    assert (sp["temperature"], sp["seed"], sp["n_keys"]) == (0.75, 9, 0) and not sp["stream_keys"]
    assert rec["f"] == dict(top_k=4, top_p=0.5, min_p=0.25)
    assert list(out) == ["thr", "kept", "ts_forced", "token", "value"]
    check_out(out["thr"], np.float32, (3,), 31.5); check_out(out["kept"], np.int32, (3,), 32); check_out(out["ts_forced"], np.int32, (3,), 33)
    check_out(out["token"], np.int32, (3,), 34); check_out(out["value"], np.float32, (3,), 35.5)


def test_filter_rows_defaults_are_the_filter_off(rig):
    eng, lib = rig
    eng.filter_rows(gp_of("plain"), ROWS, PRE, KEYS, 1.0, 1)
    assert lib.calls[1][1]["f"] == dict(top_k=0, top_p=1.0, min_p=0.0)


@pytest.mark.parametrize("kind", KINDS)
def test_score_rows(rig, kind):
    eng, lib = rig
    gp = gp_of(kind)
    out = eng.score_rows(gp, ROWS, PRE, [4, 5, 6])
    rec = check_proc(lib, "wm_score_rows", gp, ts_expected="ts" in kind)
    check_rows(rec)
    assert rec["extra"].tolist() == [4, 5, 6]
    check_out(out, np.float32, (3,), 41.5)


@pytest.mark.parametrize("kind", KINDS)
def test_topk_rows(rig, kind):
    eng, lib = rig
    gp = gp_of(kind)
    tid, tlp, rk = eng.topk_rows(gp, ROWS, PRE, [4, 5, 6], 4)
    rec = check_proc(lib, "wm_topk_rows", gp, ts_expected="ts" in kind)
    check_rows(rec)
    assert rec["extra"].tolist() == [4, 5, 6] and rec["k"] == 4
    check_out(tid, np.int32, (3, 4), 51); check_out(tlp, np.float32, (3, 4), 52.5); check_out(rk, np.int32, (3,), 53)


def test_topk_rows_keeps_a_refused_k_for_the_library_to_name(rig):
    eng, lib = rig
    tid, tlp, rk = eng.topk_rows(gp_of("plain"), ROWS, PRE, [4, 5, 6], 0)
    assert lib.calls[1][1]["k"] == 0
    assert tid.shape == (3, 1) and (tid == -1).all() and tlp.shape == (3, 1) and np.isneginf(tlp).all()


def test_seq_bias_rows(rig):
    eng, lib = rig
    out = eng.seq_bias_rows([((3, 4), -1.5), ((9,), float("-inf")), ((1, 2, 4), 2.0)], ROWS, PRE)
    assert [c[0] for c in lib.calls] == ["wm_seq_bias_rows"]
    rec = lib.calls[0][1]
    assert rec["stamp_renewed"]
    check_rows(rec)
    assert rec["n"] == 3 and rec["elens"].tolist() == [2, 1, 3] and rec["etok"].tolist() == [3, 4, 9, 1, 2, 4]
    assert rec["ebias"].tolist() == [-1.5, float("-inf"), 2.0]
    check_out(out, np.float32, (3, V), 61.5)


def test_lang_pick_rows(rig):
    eng, lib = rig
    out = eng.lang_pick_rows(ROWS, [9, 3, 400])
    assert [c[0] for c in lib.calls] == ["wm_lang_pick_rows"]
    rec = lib.calls[0][1]
    assert rec["stamp_renewed"] and rec["R"] == 3 and rec["n"] == 3 and rec["ids"].tolist() == [9, 3, 400]
    assert np.array_equal(rec["x"], ROWS.astype(np.float32))
    check_out(out, np.int32, (3,), 71)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("init", [None, [0.0, -1.0, -2.5, 0.5]])
def test_beam_rows(rig, kind, init):
    eng, lib = rig
    gp = gp_of(kind)
    S, G, n = 4, 2, 2
    x = np.random.default_rng(6).standard_normal((S, G, n, V))
    pre = [[398, 5, 6], [398, 7, 8], [398, 9, 10], [398, 11, 12]]
    o = eng.beam_rows(gp, x, pre, n, length_penalty=0.5, early_stopping="never", init_scores=init)
    rec = check_proc(lib, "wm_beam_rows", gp, ts_expected="ts" in kind)
    assert (rec["G"], rec["S"], rec["Tmax"], rec["plen"]) == (G, S, 3 + S, 3)
    assert rec["bp"] == dict(num_beams=2, length_penalty=0.5, early_stopping=2)
    assert np.array_equal(rec["x"], x.astype(np.float32))
    assert np.array_equal(rec["pre"], np.array([p + [0] * S for p in pre], dtype=np.int32))
    assert rec["init"] is None if init is None else rec["init"].tolist() == init
    assert list(o) == ["cand_val", "cand_beam", "cand_tok", "beam_idx", "steps", "fin_ids", "fin_len", "fin_score", "fin_set", "run_ids", "run_len", "run_score"]
    check_out(o["cand_val"], np.float32, (S, G, 2 * n), 80.5); check_out(o["cand_beam"], np.int32, (S, G, 2 * n), 81)
    check_out(o["cand_tok"], np.int32, (S, G, 2 * n), 82); check_out(o["beam_idx"], np.int32, (S, G * n), 83); check_out(o["steps"], np.int32, (G,), 84)
    check_out(o["fin_ids"], np.int32, (G, n, 3 + S), 85); check_out(o["fin_len"], np.int32, (G, n), 86); check_out(o["fin_score"], np.float32, (G, n), 87.5)
    check_out(o["fin_set"], np.int32, (G, n), 88); check_out(o["run_ids"], np.int32, (G * n, 3 + S), 89); check_out(o["run_len"], np.int32, (G * n,), 90)
    check_out(o["run_score"], np.float32, (G * n,), 91.5)


SEQS = [[398, 5, 6, 7], [398, 9], [398, 1, 2]]
SEQS_M = np.array([[398, 5, 6, 7], [398, 9, 0, 0], [398, 1, 2, 0]], dtype=np.int32)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("ns", [None, 395])
def test_score_tokens(rig, kind, ns):
    eng, lib = rig
    gp = gp_of(kind)
    out, nsp, ms = eng.score_tokens(SEQS, 1, gp, no_speech_token_id=ns, sot_index=0)
    rec = check_proc(lib, "wm_score_tokens", gp, ts_expected="ts" in kind)
    assert (rec["B"], rec["Tmax"]) == (3, 4) and rec["lens"].tolist() == [4, 2, 3] and rec["npr"].tolist() == [1, 1, 1] and np.array_equal(rec["tok"], SEQS_M)
    assert rec["sp"] == dict(no_speech_token_id=-1 if ns is None else ns, sot_index=0) and rec["ns_null"] == (ns is None)
    check_out(out, np.float32, (3, 4), 101.5)
    assert nsp is None if ns is None else (nsp.dtype == np.float32 and nsp.tolist() == [102.5] * 3)
    assert ms == 103.5


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("ns", [None, 395])
def test_score_tokens_topk(rig, kind, ns):
    eng, lib = rig
    gp = gp_of(kind)
    out, nsp, tid, tlp, rk, ms = eng.score_tokens_topk(SEQS, [1, 2, 1], gp, 3, no_speech_token_id=ns, sot_index=0)
    rec = check_proc(lib, "wm_score_tokens_topk", gp, ts_expected="ts" in kind)
    assert (rec["B"], rec["Tmax"], rec["k"]) == (3, 4, 3) and rec["lens"].tolist() == [4, 2, 3] and rec["npr"].tolist() == [1, 2, 1]
    assert np.array_equal(rec["tok"], SEQS_M)
    assert rec["sp"] == dict(no_speech_token_id=-1 if ns is None else ns, sot_index=0) and rec["ns_null"] == (ns is None)
    check_out(out, np.float32, (3, 4), 111.5); check_out(tid, np.int32, (3, 4, 3), 112); check_out(tlp, np.float32, (3, 4, 3), 113.5)
    check_out(rk, np.int32, (3, 4), 114)
    assert nsp is None if ns is None else (nsp.dtype == np.float32 and nsp.tolist() == [115.5] * 3)
    assert ms == 116.5


ROW_ERRORS = [
    ("select_rows", lambda e, x, p: e.select_rows(gp_of("ts"), x, p, [1] * 3), "select_rows: logits must be [R, vocab] with one prefix and one probe token per row"),
    ("sample_rows", lambda e, x, p: e.sample_rows(gp_of("ts"), x, p, [1] * 3, 1.0, 0), "sample_rows: logits must be [R, vocab] with one prefix and one stream key per row"),
    ("filter_rows", lambda e, x, p: e.filter_rows(gp_of("ts"), x, p, [1] * 3, 1.0, 0, top_k=2), "filter_rows: logits must be [R, vocab] with one prefix and one stream key per row"),
    ("score_rows", lambda e, x, p: e.score_rows(gp_of("ts"), x, p, [1] * 3), "score_rows: logits must be [R, vocab] with one prefix and one target per row"),
    ("topk_rows", lambda e, x, p: e.topk_rows(gp_of("ts"), x, p, [1] * 3, 2), "topk_rows: logits must be [R, vocab] with one prefix and one target per row"),
    ("seq_bias_rows", lambda e, x, p: e.seq_bias_rows([((3,), 1.0)], x, p), "seq_bias_rows: logits must be [R, vocab] with one prefix per row"),
]


@pytest.mark.parametrize("name,call,text", ROW_ERRORS, ids=[r[0] for r in ROW_ERRORS])
def test_shape_errors_keep_their_texts(rig, name, call, text):
    eng, lib = rig
    x = ROWS.astype(np.float32)
    for bad_x, bad_p in ((x[:, :-1], PRE), (x, PRE[:2]), (x[:2], PRE)):           # wrong vocabulary; a prefix too few; a per-row item too many
        if name == "seq_bias_rows" and bad_x.shape[0] == 2:
            bad_p = PRE                                                         # (its only per-row item is the prefix)
        with pytest.raises(ValueError, match=re.escape(text)):
            call(eng, bad_x, bad_p)
    assert lib.calls == []                                                       # refused before anything reached the library


def test_shape_errors_of_the_two_other_taps(rig):
    eng, lib = rig
    with pytest.raises(ValueError, match=re.escape("lang_pick_rows: logits must be [R, vocab]")):
        eng.lang_pick_rows(ROWS[:, :-1], [3])
    with pytest.raises(ValueError, match=re.escape("lang_pick_rows: logits must be [R, vocab]")):
        eng.lang_pick_rows(ROWS[0], [3])
    text = "beam_rows: logits must be [S, G, num_beams, vocab] with one prefix per stream, all of one length"
    x = np.zeros((2, 1, 2, V), np.float32)
    for bad_x, pre, n in ((x[..., :-1], [[1], [2]], 2), (x, [[1], [2]], 3), (x, [[1]], 2), (x, [[1], [2, 3]], 2)):
        with pytest.raises(ValueError, match=re.escape(text)):
            eng.beam_rows(gp_of("plain"), bad_x, pre, n)
    assert lib.calls == []
