// rir_check.cpp - csrc/rir_plan.h on the CPU (tests/test_rir_host.py): the validation, the twiddle table and the walk of a whole clip
// (rir_clip_host: mix_plan.h's y, the packed radix-4 transform, the pair stage, the inverse, the tail) over tables the test writes, for
// comparison with tests/rir_oracle.py bit for bit.  Stand-alone, built with -ffp-contract=off -fsanitize=address,undefined.
//   rir_check --twiddles <M> <out>       float (cos, sin) [3M/4]
//   rir_check <in> <out>
//   in : int64 n_tables, then per table int64 arena_samples, B, N, M, K; int16 arena[arena_samples]; nww_mix_item items[B];
//        nww_rir_item rir_items[B]; per response int64 L, float h[L]
//   out: per table int64 bad_item, char field[16]; int64 bad_rir_item, char field[16]; int64 bad_response, char why[32]; int64 size_ok;
//        and where all of that is clean int16 clips[B][N], float w[B][N] (the clip before the tail)
// Arena and responses are copied into heap blocks of exactly their sizes, so that AddressSanitizer sees their ends.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>
#include "rir_plan.h"

static_assert(sizeof(nww_rir_item) == 8 && sizeof(RirC) == 8, "8-byte rir items and complex values");

static bool rd(std::FILE* f, void* p, size_t n) { return n == 0 || std::fread(p, 1, n, f) == n; }
static void put_name(std::FILE* out, int64_t idx, const char* name, size_t width) {
    char buf[32] = {0};
    std::strncpy(buf, name, width - 1);
    std::fwrite(&idx, 8, 1, out);
    std::fwrite(buf, 1, width, out);
}

int main(int argc, char** argv) {
    if (argc == 4 && !std::strcmp(argv[1], "--twiddles")) {
        const int32_t M = std::atoi(argv[2]);
        if (!rir_is_size(M)) return 2;
        std::vector<RirC> T((size_t)rir_twiddle_count(M));
        rir_twiddles_host(M, T.data());
        std::FILE* out = std::fopen(argv[3], "wb");
        if (!out) return 2;
        std::fwrite(T.data(), sizeof(RirC), T.size(), out);
        return std::fclose(out) != 0 ? 4 : 0;
    }
    if (argc != 3) { std::fprintf(stderr, "usage: rir_check <in> <out> | --twiddles <M> <out>\n"); return 2; }
    std::FILE* in = std::fopen(argv[1], "rb");
    std::FILE* out = std::fopen(argv[2], "wb");
    if (!in || !out) { std::fprintf(stderr, "cannot open files\n"); return 2; }
    int64_t n_tables = 0;
    if (!rd(in, &n_tables, 8)) return 3;
    for (int64_t t = 0; t < n_tables; ++t) {
        int64_t hdr[5];
        if (!rd(in, hdr, sizeof hdr)) return 3;
        const int64_t arena_samples = hdr[0], B = hdr[1], N = hdr[2], M = hdr[3], K = hdr[4];
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
        const char* why = "";
        const int64_t bad_h = rir_first_bad_response(ir_len.data(), K, (int32_t)N, (int32_t)M, &why);
        put_name(out, bad_h, why, 32);
        const int64_t size_ok = rir_size_fits((int32_t)M, (int32_t)N) ? 1 : 0;
        std::fwrite(&size_ok, 8, 1, out);
        if (bad >= 0 || bad_r >= 0 || bad_h >= 0 || !size_ok) continue;
        std::vector<RirC> T((size_t)rir_twiddle_count((int32_t)M));
        rir_twiddles_host((int32_t)M, T.data());
        std::vector<std::vector<RirC>> spec((size_t)K);
        for (int64_t k = 0; k < K; ++k) {
            spec[(size_t)k].resize((size_t)M / 2);
            rir_prepare_host(irs[(size_t)k].get(), ir_len[(size_t)k], (int32_t)N, (int32_t)M, T.data(), spec[(size_t)k].data());
        }
        std::vector<int16_t> clips((size_t)(B * N));
        std::vector<float> ws((size_t)(B * N)), w((size_t)M);
        for (int64_t i = 0; i < B; ++i) {
            const int32_t id = ritems[(size_t)i].ir_id;
            rir_clip_host(arena.get(), items[(size_t)i], id >= 0 ? spec[(size_t)id].data() : nullptr, (int32_t)N, (int32_t)M, T.data(), w.data(),
                          clips.data() + i * N);
            std::memcpy(ws.data() + i * N, w.data(), (size_t)N * 4);
        }
        std::fwrite(clips.data(), 2, clips.size(), out);
        std::fwrite(ws.data(), 4, ws.size(), out);
    }
    std::fclose(in);
    if (std::fclose(out) != 0) return 4;
    std::printf("ok %lld tables\n", (long long)n_tables);
    return 0;
}
