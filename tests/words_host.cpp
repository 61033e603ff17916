// Host build of the word-grouping arithmetic (csrc/wm_words.h) as a stand-alone program: tests/test_words_cpu.py compiles it with the host
// compiler and holds it against tests/words_ref.py without a GPU.  The kernel runs the same functions; only the staging into LDS differs.
//   words_host IN OUT    IN: int32 words [n_tokens, n_bytes, offsets n_tokens+1, bytes (one per word), R, first R+1, modes R, ids]; OUT: one line of
//                        word starts per row
#include <cstdio>
#include <vector>
#include "wm_words.h"

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
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
    const int R = in[p++];
    std::vector<int32_t> first(in.begin() + p, in.begin() + p + R + 1);
    p += R + 1;
    std::vector<int32_t> modes(in.begin() + p, in.begin() + p + R);
    p += R;
    std::vector<int32_t> ids(in.begin() + p, in.end());
    std::vector<uint64_t> occ(3 * 256);
    for (int s = 0; s < 3; ++s)
        for (int b = 0; b < 256; ++b) occ[256 * s + b] = ww_occ(s, b);
    FILE* o = fopen(argv[2], "w");
    if (!o) return 2;
    for (int r = 0; r < R; ++r) {
        const int len = first[r + 1] - first[r];
        std::vector<int32_t> wf(len + 1);
        ww_state s;
        ww_init(s);
        for (int t = 0; t < len; ++t) {
            const int id = ids[first[r] + t], l = off[id + 1] - off[id];
            const unsigned char* b = blob.data() + off[id];
            uint64_t head = 0;
            for (int i = 0; i < l && i < WW_HEAD; ++i) head |= (uint64_t)b[i] << (8 * i);
            ww_token(s, occ.data(), modes[r], t, ww_token_fn(b, l), head, l, b, wf.data());
        }
        const int nw = ww_finish(s, occ.data(), modes[r], len, wf.data());
        for (int w = 0; w <= nw; ++w) fprintf(o, "%d ", wf[w]);
        fprintf(o, "\n");
    }
    fclose(o);
    return 0;
}
