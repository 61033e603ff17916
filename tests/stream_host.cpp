// Host build of the streaming agreement arithmetic (csrc/wm_stream.h) as a stand-alone program: tests/test_stream_cpu.py compiles it with the host
// compiler (with the address and undefined-behaviour sanitizers) and holds it against tests/stream_ref.py without a GPU.  The kernel runs the same
// functions with 256 lanes per session and block reductions in the place of the loops over lanes here.
//   stream_host IN OUT [LANES]   IN: the int32 words of stream_ref.pack_cases; OUT: one line "skip commit ender" per session.  LANES (default 1): the
//                                shares of steps 1, 3 and 4 are computed for LANES lanes and reduced as the block does
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "wm_stream.h"

struct List { std::vector<int32_t> words, tok, ids; };

int main(int argc, char** argv)
{
    if (argc < 3) return 2;
    const int lanes = argc > 3 ? atoi(argv[3]) : 1;
    FILE* f = fopen(argv[1], "rb");
    if (!f || lanes < 1) return 2;
    std::vector<int32_t> in;
    int32_t v;
    while (fread(&v, 4, 1, f) == 1) in.push_back(v);
    fclose(f);
    size_t p = 0;
    const int nt = in[p++], nb = in[p++];
    std::vector<int32_t> off(in.begin() + p, in.begin() + p + nt + 1);
    p += nt + 1;
    std::vector<unsigned char> blob(nb);
    for (int i = 0; i < nb; ++i) blob[i] = (unsigned char)in[p++];
    const int S = in[p++];
    ws_params prm;
    prm.late_cs = in[p++]; prm.near_cs = in[p++]; prm.max_ngram = in[p++];
    List L[3];
    for (int k = 0; k < 3; ++k) {
        L[k].words.assign(in.begin() + p, in.begin() + p + S + 1); p += S + 1;
        const int n_tok = in[p++];
        L[k].tok.assign(in.begin() + p, in.begin() + p + n_tok); p += n_tok;
        const int n_ids = in[p++];
        L[k].ids.assign(in.begin() + p, in.begin() + p + n_ids); p += n_ids;
    }
    const size_t n_new = (size_t)L[0].words[S];
    std::vector<int32_t> times(in.begin() + p, in.begin() + p + 2 * n_new);
    p += 2 * n_new;
    std::vector<int32_t> last(in.begin() + p, in.begin() + p + S);
    p += S;
    if (p != in.size()) return 3;
    const ws_table tab = {blob.data(), off.data()};
    FILE* o = fopen(argv[2], "w");
    if (!o) return 2;
    for (int s = 0; s < S; ++s) {
        ws_session ss;
        ss.nw = {L[0].tok.data(), L[0].ids.data(), L[0].words[s], L[0].words[s + 1] - L[0].words[s]};
        ss.pv = {L[1].tok.data(), L[1].ids.data(), L[1].words[s], L[1].words[s + 1] - L[1].words[s]};
        ss.tl = {L[2].tok.data(), L[2].ids.data(), L[2].words[s], L[2].words[s + 1] - L[2].words[s]};
        ss.times = times.data(); ss.last_cs = last[s];
        int32_t skip, commit, ender;
        if (lanes == 1) {
            ws_agree(tab, ss, prm, &skip, &commit, &ender);
        } else {
            int k0 = ss.nw.n;
            for (int l = 0; l < lanes; ++l) { const int r = ws_late(ss, prm, l, lanes); if (r < k0) k0 = r; }
            k0 += ws_overlap(tab, ss, prm, k0);
            int m = 1 << 30;
            for (int l = 0; l < lanes; ++l) { const int r = ws_mismatch(tab, ss, k0, l, lanes); if (r < m) m = r; }
            int e = -1;
            for (int l = 0; l < lanes; ++l) { const int r = ws_last_ender(tab, ss, k0, m, l, lanes); if (r > e) e = r; }
            skip = k0; commit = m; ender = e;
        }
        fprintf(o, "%d %d %d\n", skip, commit, ender);
    }
    fclose(o);
    return 0;
}
