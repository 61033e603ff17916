// wm_stream.h — the arithmetic of the streaming agreement step (include/wm.h wm_stream_agree), shared by k_stream_agree
// (wm_stream.hip) and by a host build of the same functions: plain C++ on integers and bytes, nothing of the engine.  Four parts:
//   ws_key / ws_key_next         a word's key — the bytes of its tokens with the 0x20 at both ends removed — streamed byte by byte through the
//                                vocabulary table: spaces behind the first kept byte are counted, not emitted, until a byte that is none follows
//   ws_equal, ws_ender           two keys byte-equal; a key ending in . ? ! 。 ？ ！
//   ws_late / ws_mismatch / ws_last_ender    steps 1, 3 and 4 of a session as a lane's share: lane `lane` of `lanes` takes every lanes-th word (pair)
//                                and returns its own answer, the block reduces (minimum, minimum, maximum); with lanes = 1 the answer itself
//   ws_overlap                   step 2, at most 15 word compares: one lane's work
#pragma once
#include <stdint.h>
#if defined(__HIPCC__)
#define WS_HD __host__ __device__ __forceinline__
#else
#define WS_HD inline
#endif

#define WS_TAIL 5                         // WM_STREAM_TAIL: committed words a session hands in, the longest overlap tested

struct ws_table { const unsigned char* blob; const int32_t* offsets; };
// the words [w0, w0 + n) of one session in one list: word w is the ids[tok[w] .. tok[w + 1])
struct ws_list { const int32_t* tok; const int32_t* ids; int w0, n; };
struct ws_session {
    ws_list nw, pv, tl;                   // new, prev, tail
    const int32_t* times;                 // (start, end) of every word of the new list, in centiseconds, indexed like nw.tok
    int32_t last_cs;
};
struct ws_params { int32_t late_cs, near_cs, max_ngram; };

// ---- the key of a word, streamed ----
struct ws_key {
    const int32_t* id; const int32_t* id_end;     // the ids not yet opened
    int off, end;                                 // the open token's bytes left in the blob
    int pend;                                     // 0x20 bytes seen behind a kept byte and not emitted yet
    int hold;                                     // the byte that follows them (-1: none)
    int started;
};
WS_HD void ws_key_open(ws_key& k, const ws_list& l, int w)
{
    k.id = l.ids + l.tok[l.w0 + w]; k.id_end = l.ids + l.tok[l.w0 + w + 1];
    k.off = k.end = 0; k.pend = 0; k.hold = -1; k.started = 0;
}
// the next byte of the key, -1 behind its last
WS_HD int ws_key_next(ws_key& k, const ws_table& t)
{
    for (;;) {
        if (k.hold >= 0) {
            if (k.pend > 0) { --k.pend; return 0x20; }
            const int b = k.hold;
            k.hold = -1;
            return b;
        }
        while (k.off == k.end) {
            if (k.id == k.id_end) return -1;              // (spaces still pending are trailing ones: dropped)
            const int id = *k.id++;
            k.off = t.offsets[id]; k.end = t.offsets[id + 1];
        }
        const int b = t.blob[k.off++];
        if (b == 0x20) { if (k.started) ++k.pend; continue; }
        k.started = 1;
        if (k.pend > 0) { k.hold = b; continue; }
        return b;
    }
}
WS_HD bool ws_equal(const ws_table& t, const ws_list& a, int wa, const ws_list& b, int wb)
{
    ws_key ka, kb;
    ws_key_open(ka, a, wa); ws_key_open(kb, b, wb);
    for (;;) {
        const int x = ws_key_next(ka, t), y = ws_key_next(kb, t);
        if (x != y) return false;
        if (x < 0) return true;
    }
}
// the key ends in 2E / 3F / 21, in E3 80 82 (。), EF BC 9F (？) or EF BC 81 (！)
WS_HD bool ws_ender(const ws_table& t, const ws_list& l, int w)
{
    ws_key k;
    ws_key_open(k, l, w);
    int b0 = -1, b1 = -1, b2 = -1;                        // the last three bytes, b2 the last
    for (int b = ws_key_next(k, t); b >= 0; b = ws_key_next(k, t)) { b0 = b1; b1 = b2; b2 = b; }
    if (b2 == 0x2E || b2 == 0x3F || b2 == 0x21) return true;
    if (b0 == 0xE3 && b1 == 0x80 && b2 == 0x82) return true;
    return b0 == 0xEF && b1 == 0xBC && (b2 == 0x9F || b2 == 0x81);
}

// ---- the four steps ----
WS_HD int64_t ws_start(const ws_session& s, int w) { return s.times[2 * (size_t)(s.nw.w0 + w)]; }
// step 1, a lane's share: its smallest w with start[w] > last_cs - late_cs, else n.  The minimum over the lanes is k0
WS_HD int ws_late(const ws_session& s, const ws_params& p, int lane, int lanes)
{
    const int64_t bound = (int64_t)s.last_cs - p.late_cs;
    for (int w = lane; w < s.nw.n; w += lanes)
        if (ws_start(s, w) > bound) return w;
    return s.nw.n;
}
// step 2: the words the new list repeats from the committed tail in front of it (0: none, or the step does not apply)
WS_HD int ws_overlap(const ws_table& t, const ws_session& s, const ws_params& p, int k0)
{
    const int n = s.nw.n, C = s.tl.n;
    if (k0 >= n || C <= 0) return 0;
    int64_t d = ws_start(s, k0) - (int64_t)s.last_cs;
    if (d < 0) d = -d;
    if (d >= p.near_cs) return 0;
    int top = C < n - k0 ? C : n - k0;
    if (p.max_ngram < top) top = p.max_ngram;
    for (int i = 1; i <= top; ++i) {
        bool same = true;
        for (int j = 0; j < i && same; ++j) same = ws_equal(t, s.tl, C - i + j, s.nw, k0 + j);
        if (same) return i;
    }
    return 0;
}
// step 3, a lane's share: its smallest j < min(n - k0, P) with new[k0 + j] != prev[j], else that bound.  The minimum over the lanes is m
WS_HD int ws_mismatch(const ws_table& t, const ws_session& s, int k0, int lane, int lanes)
{
    const int lim = s.nw.n - k0 < s.pv.n ? s.nw.n - k0 : s.pv.n;
    for (int j = lane; j < lim; j += lanes)
        if (!ws_equal(t, s.nw, k0 + j, s.pv, j)) return j;
    return lim > 0 ? lim : 0;
}
// step 4, a lane's share: its largest w in [k0, k0 + m) whose key ends a sentence, else -1.  The maximum over the lanes is ender
WS_HD int ws_last_ender(const ws_table& t, const ws_session& s, int k0, int m, int lane, int lanes)
{
    for (int w = k0 + m - 1 - lane; w >= k0; w -= lanes)
        if (ws_ender(t, s.nw, w)) return w;
    return -1;
}
// one session on one lane: (skip, commit, ender)
WS_HD void ws_agree(const ws_table& t, const ws_session& s, const ws_params& p, int32_t* skip, int32_t* commit, int32_t* ender)
{
    int k0 = ws_late(s, p, 0, 1);
    k0 += ws_overlap(t, s, p, k0);
    const int m = ws_mismatch(t, s, k0, 0, 1);
    *skip = k0; *commit = m; *ender = ws_last_ender(t, s, k0, m, 0, 1);
}
