// pitch_check.cpp - csrc/pitch_plan.h on the CPU (tests/test_pitch_host.py): the validation, the tables and the walk of a whole clip
// (mix_plan.h's y, pitch_clip_host, the tail) over tables the test writes, for comparison with tests/pitch_oracle.py bit for bit.
// Stand-alone, built with -ffp-contract=off -fsanitize=address,undefined.
//   pitch_check --tables <out>           float twiddles (cos, sin) [384], win [512], env [16][128]
//   pitch_check --taps <p> <q> <out>     float g [q][16]
//   pitch_check --spec <in> <out>        in: int64 N, p, q; float w[N].  out: RirC X [T + 1][256] (input frames by position), RirC Y
//                                        [T_out][256] (output frames by position), float s [128 (T_out - 1)]
//   pitch_check <in> <out>
//   in : int64 n_tables, then per table int64 arena_samples, B, N, K; int16 arena[arena_samples]; nww_mix_item items[B];
//        nww_pitch_item pitch_items[B]; int32 num[K], den[K]
//   out: per table int64 bad_item, char field[16]; int64 bad_pitch_item, char field[16]; int64 bad_ratio; int64 length_ok; and where all
//        of that is clean int16 clips[B][N], float y[B][N] (the clip before the tail)
// The arena is copied into a heap block of exactly its size, so that AddressSanitizer sees its end.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>
#include "pitch_plan.h"

static_assert(sizeof(nww_pitch_item) == 8, "8-byte pitch items");

static bool rd(std::FILE* f, void* p, size_t n) { return n == 0 || std::fread(p, 1, n, f) == n; }
static void put_name(std::FILE* out, int64_t idx, const char* name, size_t width) {
    char buf[32] = {0};
    std::strncpy(buf, name, width - 1);
    std::fwrite(&idx, 8, 1, out);
    std::fwrite(buf, 1, width, out);
}

// mix_plan.h's y of one clip, as rir_clip_host stages it
static void mix_y_host(const int16_t* arena, const nww_mix_item& it, int32_t N, float* w) {
    const int16_t* fg = arena + it.fg_off;
    const int16_t* bg = it.bg_len > 0 ? arena + it.bg_off : nullptr;
    auto bgs = [&](int64_t i) -> int { return bg[(it.bg_start + i) % it.bg_len]; };
    bool real = false;
    float s = 0.0f;
    if (bg) {
        uint64_t Sf = 0, Sb = 0;
        int32_t P = 0;
        for (int32_t j = 0; j < it.fg_len; ++j) {
            const int64_t f = fg[j], b = bgs((int64_t)it.start + j);
            Sf += (uint64_t)(f * f); Sb += (uint64_t)(b * b);
        }
        for (int32_t i = 0; i < N; ++i) { const int32_t a = bgs(i) < 0 ? -bgs(i) : bgs(i); P = a > P ? a : P; }
        real = mix_real_background(it.bg_len, P);
        if (real) s = mix_scale(Sf, Sb, it.fg_len, it.snr_linear);
    }
    const int64_t ws = real ? it.start : 0;
    for (int32_t i = 0; i < N; ++i) {
        const bool in_fg = i >= ws && i < ws + it.fg_len;
        w[i] = mix_y(in_fg ? fg[i - ws] : 0, real ? bgs(i) : 0, in_fg, real, s, it.gain);
    }
}

int main(int argc, char** argv) {
    if (argc == 3 && !std::strcmp(argv[1], "--tables")) {
        const PitchTables tb;
        std::FILE* out = std::fopen(argv[2], "wb");
        if (!out) return 2;
        std::fwrite(tb.T.data(), sizeof(RirC), tb.T.size(), out);
        std::fwrite(tb.win.data(), 4, tb.win.size(), out);
        std::fwrite(tb.env.data(), 4, tb.env.size(), out);
        return std::fclose(out) != 0 ? 4 : 0;
    }
    if (argc == 5 && !std::strcmp(argv[1], "--taps")) {
        const int32_t p = std::atoi(argv[2]), q = std::atoi(argv[3]);
        if (!pitch_ratio_ok(p, q)) return 2;
        std::vector<float> g((size_t)q * PITCH_TAPS);
        pitch_resample_table(p, q, g.data());
        std::FILE* out = std::fopen(argv[4], "wb");
        if (!out) return 2;
        std::fwrite(g.data(), 4, g.size(), out);
        return std::fclose(out) != 0 ? 4 : 0;
    }
    if (argc == 4 && !std::strcmp(argv[1], "--spec")) {
        std::FILE* in = std::fopen(argv[2], "rb");
        std::FILE* out = std::fopen(argv[3], "wb");
        if (!in || !out) return 2;
        int64_t hdr[3];
        if (!rd(in, hdr, sizeof hdr)) return 3;
        const int32_t N = (int32_t)hdr[0], p = (int32_t)hdr[1], q = (int32_t)hdr[2];
        if (!pitch_length_ok(N) || !pitch_ratio_ok(p, q)) return 2;
        std::unique_ptr<float[]> w(new float[(size_t)N]);
        if (!rd(in, w.get(), (size_t)N * 4)) return 3;
        const PitchTables tb;
        const int32_t T = pitch_frames(N), T_out = pitch_out_frames(T, p, q), S = pitch_stretched(T_out);
        std::vector<RirC> X((size_t)(T + 1) * PITCH_H), Y((size_t)T_out * PITCH_H);
        for (int32_t i = 0; i <= T; ++i) pitch_stft_frame_host(w.get(), N, i, tb, X.data() + (size_t)i * PITCH_H);
        std::vector<float> s((size_t)S);
        pitch_stretch_host(w.get(), N, p, q, tb, s.data(), Y.data());
        std::fwrite(X.data(), sizeof(RirC), X.size(), out);
        std::fwrite(Y.data(), sizeof(RirC), Y.size(), out);
        std::fwrite(s.data(), 4, s.size(), out);
        std::fclose(in);
        return std::fclose(out) != 0 ? 4 : 0;
    }
    if (argc != 3) { std::fprintf(stderr, "usage: pitch_check <in> <out> | --tables <out> | --taps <p> <q> <out> | --spec <in> <out>\n"); return 2; }
    std::FILE* in = std::fopen(argv[1], "rb");
    std::FILE* out = std::fopen(argv[2], "wb");
    if (!in || !out) { std::fprintf(stderr, "cannot open files\n"); return 2; }
    const PitchTables tb;
    int64_t n_tables = 0;
    if (!rd(in, &n_tables, 8)) return 3;
    for (int64_t t = 0; t < n_tables; ++t) {
        int64_t hdr[4];
        if (!rd(in, hdr, sizeof hdr)) return 3;
        const int64_t arena_samples = hdr[0], B = hdr[1], N = hdr[2], K = hdr[3];
        std::unique_ptr<int16_t[]> arena(new int16_t[(size_t)arena_samples]);
        std::vector<nww_mix_item> items((size_t)B);
        std::vector<nww_pitch_item> pitems((size_t)B);
        std::vector<int32_t> num((size_t)K), den((size_t)K);
        if (!rd(in, arena.get(), (size_t)arena_samples * 2) || !rd(in, items.data(), (size_t)B * sizeof(nww_mix_item)) ||
            !rd(in, pitems.data(), (size_t)B * sizeof(nww_pitch_item)) || !rd(in, num.data(), (size_t)K * 4) || !rd(in, den.data(), (size_t)K * 4))
            return 3;
        const char* field = "";
        const int64_t bad = mix_first_bad_item(items.data(), B, arena_samples, (int32_t)N, &field);
        put_name(out, bad, field, 16);
        field = "";
        const int64_t bad_p = pitch_first_bad_item(pitems.data(), B, (int32_t)K, &field);
        put_name(out, bad_p, field, 16);
        const int64_t bad_r = K <= PITCH_MAX_RATIOS ? pitch_first_bad_ratio(num.data(), den.data(), (int32_t)K) : K;
        std::fwrite(&bad_r, 8, 1, out);
        const int64_t length_ok = N <= 0x7fffffff && pitch_length_ok((int32_t)N) ? 1 : 0;
        std::fwrite(&length_ok, 8, 1, out);
        if (bad >= 0 || bad_p >= 0 || bad_r >= 0 || !length_ok) continue;
        std::vector<int16_t> clips((size_t)(B * N));
        std::vector<float> ys((size_t)(B * N));
        for (int64_t i = 0; i < B; ++i) {
            const nww_mix_item& it = items[(size_t)i];
            float* w = ys.data() + i * N;
            mix_y_host(arena.get(), it, (int32_t)N, w);
            const int32_t id = pitems[(size_t)i].pitch_id;
            if (id >= 0) pitch_clip_host(w, (int32_t)N, num[(size_t)id], den[(size_t)id], tb);
            uint32_t m = 0;                                            // the peak as the kernels take it: the max of the bit patterns
            if (it.flags & NWW_MIX_PEAK_NORMALISE)
                for (int64_t n = 0; n < N; ++n) {
                    uint32_t a;
                    std::memcpy(&a, &w[n], 4);
                    a &= 0x7fffffffu;
                    m = a > m ? a : m;
                }
            float pk;
            std::memcpy(&pk, &m, 4);
            const float r = mix_ratio(it.level, it.flags, pk);
            for (int64_t n = 0; n < N; ++n) clips[(size_t)(i * N + n)] = mix_out(w[n], r);
        }
        std::fwrite(clips.data(), 2, clips.size(), out);
        std::fwrite(ys.data(), 4, ys.size(), out);
    }
    std::fclose(in);
    if (std::fclose(out) != 0) return 4;
    std::printf("ok %lld tables\n", (long long)n_tables);
    return 0;
}
