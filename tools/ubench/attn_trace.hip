// Clip timeline of the fused attention module (attn_x3.hip compiled with -DNWW_TRACE): s_memtime of workgroup 0's waves over its second clip -
// rows split | q/k left-overs | v left-overs | per head: q | k | v | scores + softmax + P V + out_proj | ... | stores issued.
// build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -DNWW_TRACE -I nanowakeword_amd/csrc -I include tools/ubench/attn_trace.hip -o tools/ubench/attn_trace
// run:   tools/ubench/attn_trace [B=2048] [T=101]
#include "../../nanowakeword_amd/csrc/attn_x3.hip"
#include <stdio.h>
#include <vector>
int main(int argc, char** argv) {
    const int B = argc > 1 ? atoi(argv[1]) : 2048, T = argc > 2 ? atoi(argv[2]) : 101, D = 144, NH = 4;
    std::vector<float> h((size_t)B * T * D), iw((size_t)3 * D * D), ib(3 * D), ow((size_t)D * D), ob(D);
    uint32_t st = 1;
    auto rnd = [&](float a) { st = st * 1664525u + 1013904223u; return (((st >> 8) & 0xffff) / 65536.0f - 0.5f) * a; };
    for (auto& v : h) v = rnd(4.0f);
    for (auto& v : iw) v = rnd(0.2f);
    for (auto& v : ow) v = rnd(0.2f);
    for (auto& v : ib) v = rnd(0.1f);
    for (auto& v : ob) v = rnd(0.1f);
    float *dh, *dout, *diw, *dib, *dow, *dob, *dbc; void* packed;
    hipMalloc(&dh, h.size() * 4); hipMalloc(&dout, h.size() * 4); hipMalloc(&diw, iw.size() * 4); hipMalloc(&dib, ib.size() * 4);
    hipMalloc(&dow, ow.size() * 4); hipMalloc(&dob, ob.size() * 4); hipMalloc(&dbc, D * 4); hipMalloc(&packed, attn_x3_packed_bytes(D, NH));
    hipMemcpy(dh, h.data(), h.size() * 4, hipMemcpyHostToDevice); hipMemcpy(diw, iw.data(), iw.size() * 4, hipMemcpyHostToDevice);
    hipMemcpy(dib, ib.data(), ib.size() * 4, hipMemcpyHostToDevice); hipMemcpy(dow, ow.data(), ow.size() * 4, hipMemcpyHostToDevice);
    hipMemcpy(dob, ob.data(), ob.size() * 4, hipMemcpyHostToDevice);
    hipStream_t s; hipStreamCreate(&s);
    int dev = 0, cus = 256; hipGetDevice(&dev); hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    const float ws_in = 65536.0f, ws_out = 65536.0f;                       // |w| <= 0.1 -> <= 6554 < 2^15
    launch_attn_x3_pack(diw, dib, dow, dob, packed, dbc, D, NH, ws_in, ws_out, s);
    const float cK = 1.0f / 32.0f, cV = 1.0f / 32.0f;                     // L1 <= 144 x 0.1 x 65536 < 2^20 ... (timing only)
    AttnArgs a{dh, dout, (const unsigned char*)packed, dbc, B, T, 1.0f / ws_in, cK * 0x1p-15f, cV * 0x1p-15f, 1.0f / (ws_out * ws_in * cV * 0x1p-15f), 1.0f / 6.0f};
    for (int i = 0; i < 3; ++i) launch_attn_x3(a, D, NH, cus, s);
    hipStreamSynchronize(s);
    hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
    hipEventRecord(e0, s);
    for (int i = 0; i < 10; ++i) launch_attn_x3(a, D, NH, cus, s);
    hipEventRecord(e1, s); hipEventSynchronize(e1);
    float ms; hipEventElapsedTime(&ms, e0, e1);
    printf("attn_x3 B=%d T=%d: %.4f ms per launch (%s)\n", B, T, ms / 10, hipGetErrorString(hipGetLastError()));
    std::vector<unsigned long long> tr(4 * 32);
    hipMemcpyFromSymbol(tr.data(), HIP_SYMBOL(g_attn_trace), tr.size() * 8);
    printf("clocks of each phase (second clip of workgroup 0): load+split | qk-left | v-left | 4 x (q | k | v | scores..out_proj) | epilogue | total\n");
    for (int wv = 0; wv < 4; ++wv) {
        const unsigned long long* r = &tr[wv * 32];
        printf("  wave %d:", wv);
        for (int k = 1; k <= 19; ++k) printf(" %6llu", r[k] - r[k - 1]);
        printf(" | %6llu | %7llu\n", r[20] - r[19], r[20] - r[0]);
    }
    return 0;
}
