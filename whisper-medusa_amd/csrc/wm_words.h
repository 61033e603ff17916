// wm_words.h — the arithmetic of word grouping (include/wm.h wm_word_spans), shared by k_word_spans (wm_words.hip) and by a
// host build of the same functions: plain C++ on integers and bytes, nothing of the engine.  Three parts:
//   ww_utf8_step / ww_token_fn   strict UTF-8 as a 9-state automaton; a token's bytes are a map on its states, packed in 9 nibbles
//   ww_strip, ww_occ             "strip(x) is a substring of S" (and, as a bare 64-bit mask, "x is a substring of S"), streamed byte by byte:
//                                shift-and over the positions of S
//   ww_token / ww_finish         one row's tokens in order under a carried ww_state: pieces, words, prepend runs, the append rule -> word starts
#pragma once
#include <stdint.h>
#if defined(__HIPCC__)
#define WW_HD __host__ __device__ __forceinline__
#else
#define WW_HD inline
#endif

#define WW_TILE 1024                      // tokens of a row staged per round of k_word_spans
#define WW_HEAD 8                         // leading bytes of a token kept with its summary

enum { WW_SET_PUNCT = 0, WW_SET_PREP = 1, WW_SET_APP = 2 };

// bit p + 1 of the result: S[p] == b.  S = string.punctuation / HF's prepend_punctuations / append_punctuations as UTF-8
WW_HD uint64_t ww_occ(int set, unsigned b)
{
    const unsigned char PUNCT[32] = {0x21, 0x22, 0x23, 0x24, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2A, 0x2B, 0x2C, 0x2D, 0x2E, 0x2F, 0x3A,
                                     0x3B, 0x3C, 0x3D, 0x3E, 0x3F, 0x40, 0x5B, 0x5C, 0x5D, 0x5E, 0x5F, 0x60, 0x7B, 0x7C, 0x7D, 0x7E};
    const unsigned char PREP[13] = {0x22, 0x27, 0xE2, 0x80, 0x9C, 0xC2, 0xA1, 0xC2, 0xBF, 0x28, 0x5B, 0x7B, 0x2D};
    const unsigned char APP[31] = {0x22, 0x27, 0x2E, 0xE3, 0x80, 0x82, 0x2C, 0xEF, 0xBC, 0x8C, 0x21, 0xEF, 0xBC, 0x81, 0x3F, 0xEF,
                                   0xBC, 0x9F, 0x3A, 0xEF, 0xBC, 0x9A, 0xE2, 0x80, 0x9D, 0x29, 0x5D, 0x7D, 0xE3, 0x80, 0x81};
    uint64_t m = 0;                                          // (three loops of fixed length over constants: no table in memory)
    if (set == WW_SET_PUNCT) {
#pragma unroll
        for (int p = 0; p < 32; ++p) if (PUNCT[p] == b) m |= 1ull << (p + 1);
    } else if (set == WW_SET_PREP) {
#pragma unroll
        for (int p = 0; p < 13; ++p) if (PREP[p] == b) m |= 1ull << (p + 1);
    } else {
#pragma unroll
        for (int p = 0; p < 31; ++p) if (APP[p] == b) m |= 1ull << (p + 1);
    }
    return m;
}
// the empty string ends at every position 0 .. |S|
WW_HD uint64_t ww_all(int set) { return (2ull << (set == WW_SET_PUNCT ? 32 : set == WW_SET_PREP ? 13 : 31)) - 1; }

// ---- strict UTF-8 (what bytes.decode("utf-8") accepts): 0 between characters, 1 rejected for good, 2 / 3 / 7 one / two / three continuation
// bytes owed, 4 / 5 / 6 / 8 behind E0 / ED / F0 / F4, whose next byte has a narrower range
WW_HD unsigned ww_utf8_step(unsigned s, unsigned b)
{
    const bool cont = (b & 0xC0) == 0x80;
    switch (s) {
    case 0:
        if (b < 0x80) return 0;
        if (b >= 0xC2 && b <= 0xDF) return 2;
        if (b == 0xE0) return 4;
        if (b == 0xED) return 5;
        if (b >= 0xE1 && b <= 0xEF) return 3;
        if (b == 0xF0) return 6;
        if (b >= 0xF1 && b <= 0xF3) return 7;
        if (b == 0xF4) return 8;
        return 1;
    case 2: return cont ? 0 : 1;
    case 3: return cont ? 2 : 1;
    case 4: return b >= 0xA0 && b <= 0xBF ? 2 : 1;
    case 5: return b >= 0x80 && b <= 0x9F ? 2 : 1;
    case 6: return b >= 0x90 && b <= 0xBF ? 3 : 1;
    case 7: return cont ? 3 : 1;
    case 8: return b >= 0x80 && b <= 0x8F ? 3 : 1;
    default: return 1;
    }
}
// the token as a map on the states: nibble s = the state its bytes lead to from s
WW_HD uint64_t ww_token_fn(const unsigned char* p, int len)
{
    uint64_t f = 0;
    for (unsigned s = 0; s < 9; ++s) {
        unsigned q = s;
        for (int i = 0; i < len && q != 1; ++i) q = ww_utf8_step(q, p[i]);
        f |= (uint64_t)q << (4 * s);
    }
    return f;
}

// ---- strip(x) in S, streamed.  Python's strip() takes the str.isspace() code points off both ends; on bytes: their encodings, which neither
// overlap each other nor occur inside S.  phase 0: still in the leading whitespace, 1: in the core (D = the positions of S the core may end at),
// 2: whitespace behind the core, 3: no (the core left S, or went on behind whitespace).  w: a whitespace encoding begun and not finished —
// 1 C2, 2 E1, 3 E1 9A, 4 E2, 5 E2 80, 6 E2 81, 7 E3, 8 E3 80; its bytes count as core bytes once it fails
struct ww_strip { uint64_t D; unsigned phase, w; };

WW_HD void ww_strip_copy(ww_strip& d, const ww_strip& s) { d.D = s.D; d.phase = s.phase; d.w = s.w; }
WW_HD void ww_strip_init(ww_strip& m, int set) { m.D = ww_all(set); m.phase = 0; m.w = 0; }
WW_HD void ww_strip_core(ww_strip& m, const uint64_t* occ, unsigned b)
{
    if (m.phase == 0) m.phase = 1;
    if (m.phase == 1) { m.D = (m.D << 1) & occ[b]; if (!m.D) m.phase = 3; }
    else m.phase = 3;
}
WW_HD void ww_strip_space(ww_strip& m) { if (m.phase == 1) m.phase = 2; m.w = 0; }
WW_HD void ww_strip_flush(ww_strip& m, const uint64_t* occ)
{
    const unsigned w = m.w;
    m.w = 0;
    if (!w) return;
    ww_strip_core(m, occ, w == 1 ? 0xC2 : w <= 3 ? 0xE1 : w <= 6 ? 0xE2 : 0xE3);
    if (w == 3) ww_strip_core(m, occ, 0x9A);
    if (w == 5 || w == 8) ww_strip_core(m, occ, 0x80);
    if (w == 6) ww_strip_core(m, occ, 0x81);
}
WW_HD void ww_strip_byte(ww_strip& m, const uint64_t* occ, unsigned b)
{
    if (m.phase == 3) return;
    switch (m.w) {
    case 1: if (b == 0x85 || b == 0xA0) { ww_strip_space(m); return; } break;
    case 2: if (b == 0x9A) { m.w = 3; return; } break;
    case 3: if (b == 0x80) { ww_strip_space(m); return; } break;
    case 4: if (b == 0x80) { m.w = 5; return; } if (b == 0x81) { m.w = 6; return; } break;
    case 5: if ((b >= 0x80 && b <= 0x8A) || b == 0xA8 || b == 0xA9 || b == 0xAF) { ww_strip_space(m); return; } break;
    case 6: if (b == 0x9F) { ww_strip_space(m); return; } break;
    case 7: if (b == 0x80) { m.w = 8; return; } break;
    case 8: if (b == 0x80) { ww_strip_space(m); return; } break;
    default: break;
    }
    ww_strip_flush(m, occ);
    if (m.phase == 3) return;
    if ((b >= 0x09 && b <= 0x0D) || (b >= 0x1C && b <= 0x20)) { ww_strip_space(m); return; }
    if (b == 0xC2) m.w = 1;
    else if (b == 0xE1) m.w = 2;
    else if (b == 0xE2) m.w = 4;
    else if (b == 0xE3) m.w = 7;
    else ww_strip_core(m, occ, b);
}
WW_HD bool ww_strip_result(const ww_strip& src, const uint64_t* occ)
{
    ww_strip m;
    ww_strip_copy(m, src);
    ww_strip_flush(m, occ);
    return m.phase == 0 || (m.phase != 3 && m.D != 0);
}

// ---- one row under carried state ----
struct ww_state {
    unsigned u;                     // UTF-8 state behind the last token
    int ps;                         // first token of the open piece
    int pfirst, plast;              // its first byte (-1: no token yet), the last byte in front of it (-1: none)
    int lastb;                      // last byte of the last token
    ww_strip mp, qn, qc;            // the piece against PUNCT; the piece as a new word / the word with the piece appended against PREP
    uint64_t an, ac;                // the same two against APP, unstripped (0: no)
    int have_word, wstart, wfirst, wlast;       // the open word: first token, first byte, last byte in front of it
    ww_strip wq; uint64_t wa;       // the open word against PREP and APP
    int gopen, gstart, glast, gcount;           // the open prepend run: first token, last byte in front of it, words
    int nw;                         // words written
};

WW_HD void ww_piece_reset(ww_state& s, int start)
{
    s.ps = start; s.pfirst = -1;
    ww_strip_init(s.mp, WW_SET_PUNCT);
    ww_strip_init(s.qn, WW_SET_PREP);
    s.an = ww_all(WW_SET_APP);
    ww_strip_copy(s.qc, s.wq); s.ac = s.wa;
}
WW_HD void ww_init(ww_state& s)
{
    s.u = 0; s.lastb = -1; s.plast = -1;
    s.have_word = 0; s.wstart = 0; s.wfirst = -1; s.wlast = -1;
    ww_strip_init(s.wq, WW_SET_PREP); s.wa = 0;
    s.gopen = 0; s.gstart = 0; s.glast = -1; s.gcount = 0; s.nw = 0;
    ww_piece_reset(s, 0);
}
// the open word is complete.  It joins the open prepend run; the run ends with a word that is no prepend candidate, or with the row's last word
// (HF never tests it).  A run of one word that is a substring of the append set joins the word in front of it unless that ends in a space.
WW_HD void ww_word_done(ww_state& s, const uint64_t* occ_prep, bool last, int32_t* word_first)
{
    const bool P = s.wfirst == 0x20 && ww_strip_result(s.wq, occ_prep);
    if (!s.gopen) { s.gopen = 1; s.gstart = s.wstart; s.glast = s.wlast; s.gcount = 0; }
    ++s.gcount;
    if (P && !last) return;
    const bool app = s.gcount == 1 && s.wa != 0;
    if (!(s.nw > 0 && s.glast != 0x20 && app)) word_first[s.nw++] = s.gstart;
    s.gopen = 0;
}
// the open piece ends in front of token `end`
WW_HD void ww_piece_close(ww_state& s, const uint64_t* occ /* [3][256] */, int unicode, int end, int32_t* word_first)
{
    const bool opens = unicode || s.pfirst == 0x20 || ww_strip_result(s.mp, occ + 256 * WW_SET_PUNCT) || !s.have_word;
    if (opens) {
        if (s.have_word) ww_word_done(s, occ + 256 * WW_SET_PREP, false, word_first);
        s.have_word = 1; s.wstart = s.ps; s.wfirst = s.pfirst; s.wlast = s.plast;
        ww_strip_copy(s.wq, s.qn); s.wa = s.an;
    } else {
        ww_strip_copy(s.wq, s.qc); s.wa = s.ac;
    }
    ww_piece_reset(s, end);
}
// token t of the row: its bytes (the first WW_HEAD in `head`, little-endian; all of them at `bytes`), its UTF-8 map
WW_HD void ww_token(ww_state& s, const uint64_t* occ, int unicode, int t, uint64_t fn, uint64_t head, int len, const unsigned char* bytes,
                    int32_t* word_first)
{
    if (s.pfirst < 0) { s.pfirst = (int)(head & 0xFF); s.plast = s.lastb; }
    for (int i = 0; i < len; ++i) {
        if (s.mp.phase == 3 && s.qn.phase == 3 && s.qc.phase == 3 && !s.an && !s.ac) break;
        const unsigned b = i < WW_HEAD ? (unsigned)(head >> (8 * i)) & 0xFF : bytes[i];
        ww_strip_byte(s.mp, occ + 256 * WW_SET_PUNCT, b);
        ww_strip_byte(s.qn, occ + 256 * WW_SET_PREP, b);
        ww_strip_byte(s.qc, occ + 256 * WW_SET_PREP, b);
        s.an = (s.an << 1) & occ[256 * WW_SET_APP + b];
        s.ac = (s.ac << 1) & occ[256 * WW_SET_APP + b];
    }
    s.lastb = len <= WW_HEAD ? (int)((head >> (8 * (len - 1))) & 0xFF) : bytes[len - 1];
    s.u = (unsigned)(fn >> (4 * s.u)) & 15;
    if (s.u == 0) ww_piece_close(s, occ, unicode, t + 1, word_first);
}
// the row is over at `len` tokens: tokens left over are a last piece of their own.  Returns n_words; word_first[n_words] = len
WW_HD int ww_finish(ww_state& s, const uint64_t* occ, int unicode, int len, int32_t* word_first)
{
    if (s.ps < len) ww_piece_close(s, occ, unicode, len, word_first);
    if (s.have_word) ww_word_done(s, occ + 256 * WW_SET_PREP, true, word_first);
    word_first[s.nw] = len;
    return s.nw;
}
