// rir_seg_check.cpp - the segmented route of csrc/rir_plan.h on the CPU (tests/test_rir_seg_host.py): the sizes, the validation and the
// walk of a whole clip (rir_seg_prepare_host, rir_seg_clip_host: mix_plan.h's y, the windows of every (segment, partition) pair through
// the packed radix-4 transform, the float32 sum, the peak over the clip, the tail) over tables the test writes, for comparison with
// tests/rir_seg_oracle.py bit for bit.  Stand-alone, built with -ffp-contract=off -fsanitize=address,undefined.
//   rir_seg_check --sizes <in> <out>     in: int64 n, then n x int64 (K, N, L, M); out: n x int64 (rir_parts, rir_segments,
//                                        rir_spectra_floats, rir_fft_size)
//   rir_seg_check <in> <out>
//   in : int64 n_tables, then per table int64 arena_samples, B, N, K; int16 arena[arena_samples]; nww_mix_item items[B];
//        nww_rir_item rir_items[B]; per response int64 L, float h[L]
//   out: per table int64 bad_item, char field[16]; int64 bad_rir_item, char field[16]; int64 bad_response; and where all of that is
//        clean int16 clips[B][N], float w[B][N] (the clip before the tail)
// Arena, responses and spectra are copied into heap blocks of exactly their sizes, so that AddressSanitizer sees their ends.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>
#include "rir_plan.h"

static bool rd(std::FILE* f, void* p, size_t n) { return n == 0 || std::fread(p, 1, n, f) == n; }
static void put_name(std::FILE* out, int64_t idx, const char* name, size_t width) {
    char buf[32] = {0};
    std::strncpy(buf, name, width - 1);
    std::fwrite(&idx, 8, 1, out);
    std::fwrite(buf, 1, width, out);
}

static int sizes(const char* src, const char* dst) {
    std::FILE* in = std::fopen(src, "rb");
    std::FILE* out = std::fopen(dst, "wb");
    if (!in || !out) return 2;
    int64_t n = 0;
    if (!rd(in, &n, 8)) return 3;
    for (int64_t i = 0; i < n; ++i) {
        int64_t a[4];
        if (!rd(in, a, sizeof a)) return 3;
        const int32_t K = (int32_t)a[0], N = (int32_t)a[1], L = (int32_t)a[2], M = (int32_t)a[3];
        const int64_t r[4] = {rir_parts(N, L), rir_segments(N), rir_spectra_floats(K, N, L, M), rir_fft_size(N, L)};
        std::fwrite(r, 8, 4, out);
    }
    std::fclose(in);
    return std::fclose(out) != 0 ? 4 : 0;
}

int main(int argc, char** argv) {
    if (argc == 4 && !std::strcmp(argv[1], "--sizes")) return sizes(argv[2], argv[3]);
    if (argc != 3) { std::fprintf(stderr, "usage: rir_seg_check <in> <out> | --sizes <in> <out>\n"); return 2; }
    std::FILE* in = std::fopen(argv[1], "rb");
    std::FILE* out = std::fopen(argv[2], "wb");
    if (!in || !out) { std::fprintf(stderr, "cannot open files\n"); return 2; }
    std::vector<RirC> T((size_t)rir_twiddle_count(RIR_M_MAX));
    rir_twiddles_host(RIR_M_MAX, T.data());
    int64_t n_tables = 0;
    if (!rd(in, &n_tables, 8)) return 3;
    for (int64_t t = 0; t < n_tables; ++t) {
        int64_t hdr[4];
        if (!rd(in, hdr, sizeof hdr)) return 3;
        const int64_t arena_samples = hdr[0], B = hdr[1], N = hdr[2], K = hdr[3];
        std::unique_ptr<int16_t[]> arena(new int16_t[(size_t)arena_samples]);
        std::vector<nww_mix_item> items((size_t)B);
        std::vector<nww_rir_item> ritems((size_t)B);
        if (!rd(in, arena.get(), (size_t)arena_samples * 2) || !rd(in, items.data(), (size_t)B * sizeof(nww_mix_item)) ||
            !rd(in, ritems.data(), (size_t)B * sizeof(nww_rir_item)))
            return 3;
        std::vector<std::unique_ptr<float[]>> irs;
        std::vector<int32_t> ir_len;
        for (int64_t k = 0; k < K; ++k) {
            int64_t L = 0;
            if (!rd(in, &L, 8)) return 3;
            irs.emplace_back(new float[(size_t)(L > 0 ? L : 0)]);
            if (L > 0 && !rd(in, irs.back().get(), (size_t)L * 4)) return 3;
            ir_len.push_back((int32_t)L);
        }
        const char* field = "";
        const int64_t bad = mix_first_bad_item(items.data(), B, arena_samples, (int32_t)N, &field);
        put_name(out, bad, field, 16);
        field = "";
        const int64_t bad_r = rir_first_bad_item(ritems.data(), B, (int32_t)K, &field);
        put_name(out, bad_r, field, 16);
        const int64_t bad_h = rir_seg_first_bad_response(ir_len.data(), K);
        std::fwrite(&bad_h, 8, 1, out);
        if (bad >= 0 || bad_r >= 0 || bad_h >= 0) continue;
        std::vector<std::unique_ptr<RirC[]>> spec;
        for (int64_t k = 0; k < K; ++k) {
            spec.emplace_back(new RirC[(size_t)rir_parts((int32_t)N, ir_len[(size_t)k]) * (RIR_M_MAX / 2)]);
            rir_seg_prepare_host(irs[(size_t)k].get(), ir_len[(size_t)k], (int32_t)N, T.data(), spec.back().get());
        }
        std::vector<int16_t> clips((size_t)(B * N));
        std::vector<float> ws((size_t)(B * N));
        for (int64_t i = 0; i < B; ++i) {
            const int32_t id = ritems[(size_t)i].ir_id;
            std::unique_ptr<float[]> w(new float[(size_t)N]);
            rir_seg_clip_host(arena.get(), items[(size_t)i], id >= 0 ? spec[(size_t)id].get() : nullptr,
                              id >= 0 ? rir_parts((int32_t)N, ir_len[(size_t)id]) : 0, (int32_t)N, T.data(), w.get(), clips.data() + i * N);
            std::memcpy(ws.data() + i * N, w.get(), (size_t)N * 4);
        }
        std::fwrite(clips.data(), 2, clips.size(), out);
        std::fwrite(ws.data(), 4, ws.size(), out);
    }
    std::fclose(in);
    if (std::fclose(out) != 0) return 4;
    std::printf("ok %lld tables\n", (long long)n_tables);
    return 0;
}
