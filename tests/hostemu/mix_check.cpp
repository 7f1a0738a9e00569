// mix_check.cpp - csrc/mix_plan.h on the CPU (tests/test_mix_host.py): the item validation and the per-sample arithmetic the kernel of
// mix.hip runs, over tables the test writes, for comparison with tests/mix_oracle.py bit for bit.  Stand-alone, built with
// -ffp-contract=off -fsanitize=address,undefined: an item the validation lets through that reads outside the arena aborts here.
//   mix_check <in> <out>
//   in : int64 n_tables, then per table int64 arena_samples, B, N; int16 arena[arena_samples]; nww_mix_item items[B]
//   out: per table int64 bad (index of the first bad item, -1: none), char field[16]; and for bad == -1 int16 clips[B][N]
// The arena is copied into a heap block of exactly arena_samples samples, so that AddressSanitizer sees its two ends.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>
#include "mix_plan.h"

static_assert(sizeof(nww_mix_item) == 48, "nww_mix_item is 48 bytes without implicit padding");

static bool rd(std::FILE* f, void* p, size_t n) { return n == 0 || std::fread(p, 1, n, f) == n; }

int main(int argc, char** argv) {
    if (argc != 3) { std::fprintf(stderr, "usage: mix_check <in> <out>\n"); return 2; }
    std::FILE* in = std::fopen(argv[1], "rb");
    std::FILE* out = std::fopen(argv[2], "wb");
    if (!in || !out) { std::fprintf(stderr, "cannot open files\n"); return 2; }
    int64_t n_tables = 0;
    if (!rd(in, &n_tables, 8)) return 3;
    for (int64_t t = 0; t < n_tables; ++t) {
        int64_t hdr[3];
        if (!rd(in, hdr, sizeof hdr)) return 3;
        const int64_t arena_samples = hdr[0], B = hdr[1], N = hdr[2];
        std::unique_ptr<int16_t[]> arena(new int16_t[(size_t)arena_samples]);
        std::vector<nww_mix_item> items((size_t)B);
        if (!rd(in, arena.get(), (size_t)arena_samples * 2) || !rd(in, items.data(), (size_t)B * sizeof(nww_mix_item))) return 3;
        const char* field = "";
        const int64_t bad = mix_first_bad_item(items.data(), B, arena_samples, (int32_t)N, &field);
        char name[16] = {0};
        std::strncpy(name, field, sizeof name - 1);
        std::fwrite(&bad, 8, 1, out);
        std::fwrite(name, 1, sizeof name, out);
        if (bad >= 0) continue;
        std::vector<int16_t> clip((size_t)N);
        for (int64_t i = 0; i < B; ++i) {
            mix_clip_host(arena.get(), items[(size_t)i], (int32_t)N, clip.data());
            std::fwrite(clip.data(), 2, (size_t)N, out);
        }
    }
    std::fclose(in);
    if (std::fclose(out) != 0) return 4;
    std::printf("ok %lld tables\n", (long long)n_tables);
    return 0;
}
