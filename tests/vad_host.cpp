// Host build of the speech-window arithmetic (csrc/wm_vad.h) as a stand-alone program: tests/test_vad_cpu.py compiles it with the host compiler
// and holds it against tests/vad_ref.py without a GPU.  The kernels run the same functions for the energy of a frame, the per-region stage and the
// split-and-pack loop; the order statistic, the hysteresis and the run boundaries, which the kernels do as a radix select and as scans, are plain
// loops here.
//   vad_host IN OUT    IN: int32 n_cases, then per case int32 n, float32 k_on k_off abs_on abs_off, int32 q_permille min_silence min_speech pad F,
//                      float32 x[n];  OUT: per case three lines: E as hex bit patterns, the regions, the windows
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>
#include "wm_vad.h"

struct HostArgMin {
    const float* E;
    int operator()(int lo, int hi) const
    {
        int best = lo;
        for (int t = lo; t <= hi; ++t) {
            uint32_t a, b;
            std::memcpy(&a, E + t, 4);
            std::memcpy(&b, E + best, 4);
            if (a < b) best = t;
        }
        return best;
    }
};

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    FILE* o = fopen(argv[2], "w");
    if (!f || !o) return 2;
    int32_t n_cases = 0;
    if (fread(&n_cases, 4, 1, f) != 1) return 2;
    for (int cs = 0; cs < n_cases; ++cs) {
        int32_t n, ip[5];
        float fp[4];
        if (fread(&n, 4, 1, f) != 1 || fread(fp, 4, 4, f) != 4 || fread(ip, 4, 5, f) != 5) return 2;
        std::vector<float> x(n);
        if (fread(x.data(), 4, n, f) != (size_t)n) return 2;
        const int T = (n + VAD_HOP - 1) / VAD_HOP, q = ip[0], min_silence = ip[1], min_speech = ip[2], pad = ip[3], F = ip[4];
        std::vector<float> E(T);
        std::vector<uint32_t> bits(T);
        for (int t = 0; t < T; ++t) {
            E[t] = vad_energy_frame(x.data() + (size_t)t * VAD_HOP, (long long)n - (long long)t * VAD_HOP);
            std::memcpy(&bits[t], &E[t], 4);
        }
        std::vector<uint32_t> sorted(bits);
        std::sort(sorted.begin(), sorted.end());
        float R;
        const uint32_t rb = sorted[(size_t)(((long long)q * (T - 1)) / 1000)];
        std::memcpy(&R, &rb, 4);
        const float a_on = R * fp[0], a_off = R * fp[1];
        const float thr_on = a_on > fp[2] ? a_on : fp[2], thr_off = a_off > fp[3] ? a_off : fp[3];
        std::vector<int> bnd;
        int prev = 0;
        for (int t = 0; t <= T; ++t) {
            int s = 0;
            if (t < T) s = E[t] >= thr_on ? 1 : (E[t] < thr_off ? 0 : prev);
            if (s != prev) bnd.push_back(t);
            prev = s;
        }
        std::vector<int> reg(2 * (T / 2 + 1)), win(2 * (T / 2 + 1 + T / (F / 2)));
        const int nr = vad_regions(bnd.data(), (int)bnd.size(), T, min_silence, min_speech, pad, reg.data(), (int)reg.size() / 2);
        const int nw = vad_split_pack(reg.data(), nr, F, HostArgMin{E.data()}, true, win.data(), (int)win.size() / 2);
        if (nr > (int)reg.size() / 2 || nw > (int)win.size() / 2) return 3;
        for (int t = 0; t < T; ++t) fprintf(o, "%08x ", bits[t]);
        fprintf(o, "\n");
        for (int r = 0; r < nr; ++r) fprintf(o, "%d %d ", reg[2 * r], reg[2 * r + 1]);
        fprintf(o, "\n");
        for (int w = 0; w < nw; ++w) fprintf(o, "%d %d ", win[2 * w], win[2 * w + 1]);
        fprintf(o, "\n");
    }
    fclose(o);
    fclose(f);
    return 0;
}
