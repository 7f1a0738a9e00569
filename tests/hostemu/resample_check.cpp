// resample_check.cpp - csrc/resample_plan.h on the CPU (tests/test_resample_host.py): the validation, the tap tables and the walk of
// whole items, tile by tile as the kernel goes, over tables the test writes, for comparison with tests/resample_oracle.py bit for bit.
// Stand-alone, built with -ffp-contract=off -fsanitize=address,undefined.
//   resample_check --taps <p> <q> <out>   int32 taps, j0, span; float g [q][taps]
//   resample_check <in> <out>
//   in : int64 n_tables, then per table int64 src_values, B, K, src_format, dst_format, dst_values; the source (src_values values of
//        its format); nww_resample_item items[B]; int32 num[K], den[K]
//   out: per table int64 bad_ratio (K beyond the limit: K); int64 formats_ok; int64 bad_item, char field[16]; and where all of that is
//        clean the destination (dst_values values of its format), every byte 0x5a where no item wrote
// Source and destination are heap blocks of exactly their size, so that AddressSanitizer sees their ends.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>
#include "resample_plan.h"

static_assert(sizeof(nww_resample_item) == 32, "32-byte items");
static_assert(sizeof(ResampleRatio) == 32, "32-byte ratios");

static bool rd(std::FILE* f, void* p, size_t n) { return n == 0 || std::fread(p, 1, n, f) == n; }

template <typename S, typename D>
static void walk(const void* src, const std::vector<nww_resample_item>& items, const std::vector<ResampleRatio>& ratios, const std::vector<float>& taps, void* dst) {
    for (const nww_resample_item& it : items) {
        const ResampleRatio* r = it.rate_id < 0 ? nullptr : &ratios[(size_t)it.rate_id];
        resample_item_host(static_cast<const S*>(src) + it.src_off, it.src_frames, it.channels, r, r ? taps.data() + r->off : nullptr,
                           static_cast<D*>(dst) + it.dst_off);
    }
}

int main(int argc, char** argv) {
    if (argc == 5 && !std::strcmp(argv[1], "--taps")) {
        const int32_t p = std::atoi(argv[2]), q = std::atoi(argv[3]);
        if (!resample_ratio_ok(p, q)) return 2;
        const ResampleRatio r = resample_ratio(p, q, 0);
        std::vector<float> g((size_t)q * (size_t)r.taps);
        resample_table(p, q, g.data());
        std::FILE* out = std::fopen(argv[4], "wb");
        if (!out) return 2;
        const int32_t hdr[3] = {r.taps, r.j0, r.span};
        std::fwrite(hdr, 4, 3, out);
        std::fwrite(g.data(), 4, g.size(), out);
        return std::fclose(out) != 0 ? 4 : 0;
    }
    if (argc != 3) { std::fprintf(stderr, "usage: resample_check <in> <out> | --taps <p> <q> <out>\n"); return 2; }
    std::FILE* in = std::fopen(argv[1], "rb");
    std::FILE* out = std::fopen(argv[2], "wb");
    if (!in || !out) { std::fprintf(stderr, "cannot open files\n"); return 2; }
    int64_t n_tables = 0;
    if (!rd(in, &n_tables, 8)) return 3;
    for (int64_t t = 0; t < n_tables; ++t) {
        int64_t hdr[6];
        if (!rd(in, hdr, sizeof hdr)) return 3;
        const int64_t src_values = hdr[0], B = hdr[1], K = hdr[2], sf = hdr[3], df = hdr[4], dst_values = hdr[5];
        const size_t sv = sf == NWW_PCM_F32 ? 4 : 2, dv = df == NWW_PCM_F32 ? 4 : 2;
        std::unique_ptr<unsigned char[]> src(new unsigned char[(size_t)src_values * sv]);
        std::vector<nww_resample_item> items((size_t)B);
        std::vector<int32_t> num((size_t)K), den((size_t)K);
        if (!rd(in, src.get(), (size_t)src_values * sv) || !rd(in, items.data(), (size_t)B * sizeof(nww_resample_item)) ||
            !rd(in, num.data(), (size_t)K * 4) || !rd(in, den.data(), (size_t)K * 4))
            return 3;
        const int64_t bad_r = K <= RESAMPLE_MAX_RATIOS ? resample_first_bad_ratio(num.data(), den.data(), (int32_t)K) : K;
        std::fwrite(&bad_r, 8, 1, out);
        const int64_t formats_ok = resample_format_ok((int32_t)sf) && resample_format_ok((int32_t)df) ? 1 : 0;
        std::fwrite(&formats_ok, 8, 1, out);
        const char* field = "";
        const int64_t bad = bad_r >= 0 ? -1 : resample_first_bad_item(items.data(), B, src_values, dst_values, num.data(), den.data(), (int32_t)K, &field);
        char name[16] = {0};
        std::strncpy(name, field, 15);
        std::fwrite(&bad, 8, 1, out);
        std::fwrite(name, 1, 16, out);
        if (bad_r >= 0 || !formats_ok || bad >= 0) continue;
        std::vector<ResampleRatio> ratios((size_t)K);
        std::vector<float> taps;
        for (int64_t k = 0; k < K; ++k) {
            ratios[(size_t)k] = resample_ratio(num[(size_t)k], den[(size_t)k], (int32_t)taps.size());
            taps.resize(taps.size() + (size_t)den[(size_t)k] * (size_t)ratios[(size_t)k].taps);
            resample_table(num[(size_t)k], den[(size_t)k], taps.data() + ratios[(size_t)k].off);
        }
        std::unique_ptr<unsigned char[]> dst(new unsigned char[(size_t)dst_values * dv]);
        std::memset(dst.get(), 0x5a, (size_t)dst_values * dv);
        if (sf == NWW_PCM_F32 && df == NWW_PCM_F32) walk<float, float>(src.get(), items, ratios, taps, dst.get());
        else if (sf == NWW_PCM_F32) walk<float, int16_t>(src.get(), items, ratios, taps, dst.get());
        else if (df == NWW_PCM_F32) walk<int16_t, float>(src.get(), items, ratios, taps, dst.get());
        else walk<int16_t, int16_t>(src.get(), items, ratios, taps, dst.get());
        std::fwrite(dst.get(), dv, (size_t)dst_values, out);
    }
    std::fclose(in);
    if (std::fclose(out) != 0) return 4;
    std::printf("ok %lld tables\n", (long long)n_tables);
    return 0;
}
