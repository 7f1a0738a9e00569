// plan_host_check.cpp - the planner's value arithmetic (csrc/plan_host.h) held to what its comments promise (tests/test_plan_host.py):
// the power-of-two scales against the binary16 range, the layer bound against sampled and sign-aligned inputs, the range guards on a
// model with uniform channel gains and on one whose gains spread, and the load-time channel balance against a float32 forward of a
// tiny conv + ReLU + Linear net written out here.
#include <cstdio>
#include <cstring>
#include <random>
#include "plan_host.h"

double f16_range_factor() { return 65536.0; }      // the library's default window (NWW_F16_RANGE_LOG2 = 16)

static int g_fail = 0;
#define CHECK(cond, ...)                                                        \
    do {                                                                        \
        if (!(cond)) {                                                          \
            if (++g_fail <= 20) { std::printf("FAIL %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
        }                                                                       \
    } while (0)

static std::mt19937_64 g_rng(20240607);
static double uni(double a, double b) { return a + (b - a) * (double)(g_rng() >> 11) * (1.0 / 9007199254740992.0); }
static std::vector<float> rand_vec(size_t n, double a, double b) { std::vector<float> v(n); for (float& x : v) x = (float)uni(a, b); return v; }
static bool is_pow2(double x) { int e; return x > 0.0 && std::frexp(x, &e) == 0.5; }
static const double TWO40 = 1099511627776.0;

// ---- f16_scale: the largest power of two (up to 2^40) that keeps bound x 1.02 inside the binary16 range
static void check_scale_at(double b) {
    const double s = (double)f16_scale(b);
    CHECK(is_pow2(s) && s <= TWO40, "b=%.17g s=%.17g", b, s);
    CHECK(b * 1.02 * s <= 65504.0, "b=%.17g s=%.17g", b, s);
    CHECK(s == TWO40 || b * 1.02 * (2.0 * s) > 65504.0, "b=%.17g s=%.17g", b, s);
}
static void check_scale() {
    for (int i = 0; i < 4000; ++i) check_scale_at(std::pow(10.0, uni(-20.0, 20.0)));
    for (int e = -66; e <= 66; ++e) check_scale_at(std::ldexp(1.0, e));
    for (int e = -30; e <= 30; ++e) {                          // around 65504 / 1.02 and its power-of-two multiples, a few ulps either side
        double b = std::ldexp(65504.0 / 1.02, e), lo = b, hi = b;
        check_scale_at(b);
        for (int u = 0; u < 4; ++u) { lo = std::nextafter(lo, 0.0); hi = std::nextafter(hi, INFINITY); check_scale_at(lo); check_scale_at(hi); }
    }
    for (double b : {1e30, 1.0000001e30, 1e300, (double)INFINITY, (double)NAN}) CHECK(f16_scale(b) == 0.0f, "b=%g -> %g", b, (double)f16_scale(b));
    for (double b : {1e-30, 1e-31, 1e-300, 0.0, -0.0, -1.0, -1e30, -(double)INFINITY}) CHECK((double)f16_scale(b) == TWO40, "b=%g -> %g", b, (double)f16_scale(b));
}

// ---- f16_wscale: the largest weight x scale lands where 2.04 x it fits and 4.08 x it does not
static void check_wscale() {
    for (int i = 0; i < 500; ++i) {
        std::vector<float> w = rand_vec(8 + (size_t)(g_rng() % 40), -1.0, 1.0);
        const float g = (float)std::pow(10.0, uni(-3.0, 6.0));      // (the largest weight stays above 65504 / 2.04 / 2^40, where the scale's cap sets in)
        double m = 0.0;
        for (float& x : w) { x *= g; m = std::fmax(m, std::fabs((double)x)); }
        const double s = (double)f16_wscale(w);
        CHECK(is_pow2(s), "m=%.9g s=%.9g", m, s);
        CHECK(2.04 * m * s <= 65504.0 && 65504.0 < 4.08 * m * s, "m=%.17g s=%.17g", m, s);
    }
    std::vector<float> w = rand_vec(9, -1.0, 1.0);
    w[4] = INFINITY;
    CHECK(f16_wscale(w) == 0.0f, "an infinite weight -> %g", (double)f16_wscale(w));
    w[4] = -INFINITY;
    CHECK(f16_wscale(w) == 0.0f, "an infinite weight -> %g", (double)f16_wscale(w));
}

// ---- f16_layer_bound: no input inside the input bound gets past it, and the worst channel's sign-aligned input reaches it
static double layer_value(const std::vector<float>& w, int K, int c, const std::vector<double>& x, const std::vector<float>& b, bool has_b,
                          const std::vector<float>& al, const std::vector<float>& be, bool has_bn) {
    double t = 0.0;
    for (int k = 0; k < K; ++k) t += (double)w[(size_t)c * K + k] * x[k];
    if (has_b) t += (double)b[c];
    if (has_bn) t = t * (double)al[c] + (double)be[c];
    return std::fabs(t);
}
static void check_layer_bound() {
    const int Cout = 5, K = 7;
    const double in_bound = 3.5;
    for (int form = 0; form < 5; ++form) {                      // bias x BatchNorm, then both present with b = 0 and be = 0
        const bool has_b = form & 1, has_bn = (form & 2) || form == 4, zero = form == 4;
        const std::vector<float> w = rand_vec((size_t)Cout * K, -1.0, 1.0), al = rand_vec(Cout, -2.0, 2.0);
        std::vector<float> b = rand_vec(Cout, -3.0, 3.0), be = rand_vec(Cout, -3.0, 3.0);
        if (zero) { b.assign(Cout, 0.0f); be.assign(Cout, 0.0f); }
        const double bound = f16_layer_bound(w, Cout, K, b, has_b || zero, al, be, has_bn, in_bound), slack = bound * (1.0 + 1e-12);
        std::vector<double> x(K);
        for (int i = 0; i < 10000; ++i) {
            for (double& v : x) v = uni(-in_bound, in_bound);
            for (int c = 0; c < Cout; ++c) {
                const double y = layer_value(w, K, c, x, b, has_b || zero, al, be, has_bn);
                CHECK(y <= slack, "form %d channel %d: %.17g > %.17g", form, c, y, bound);
            }
        }
        double reached = 0.0;
        for (int c0 = 0; c0 < Cout; ++c0) {
            for (int k = 0; k < K; ++k) x[k] = w[(size_t)c0 * K + k] < 0.0f ? -in_bound : in_bound;
            for (int c = 0; c < Cout; ++c) {
                const double y = layer_value(w, K, c, x, b, has_b || zero, al, be, has_bn);
                CHECK(y <= slack, "form %d sign-aligned to %d, channel %d: %.17g > %.17g", form, c0, c, y, bound);
                if (c == c0) reached = std::fmax(reached, y);
            }
        }
        if (zero || (!has_b && !has_bn)) CHECK(reached >= bound * (1.0 - 1e-12), "form %d: reached %.17g of %.17g", form, reached, bound);
    }
}

// ---- F16Range::ok (the mean over the channels) and f16_rows_ok (what each consumer row sees)
static void check_range_guards() {
    const int C = 8, K = 9, N = 4;                             // a 3x3 conv on the features, 8 channels, read by a [4][8] layer
    const double in_bound = 8192.0, in_typ = 32.0;
    const std::vector<float> none;
    for (int spread = 0; spread < 2; ++spread) {
        std::vector<float> w = rand_vec((size_t)C * K, -1.0, 1.0), cw = rand_vec((size_t)N * C, 0.5, 1.0);
        if (spread) {                                           // channel 0 at 2^24 times the others' gain, its consumer weights at 2^-24
            for (int k = 0; k < K; ++k) w[k] = std::ldexp(w[k], 24);
            for (int n = 0; n < N; ++n) cw[(size_t)n * C] = std::ldexp(cw[(size_t)n * C], -24);
        }
        const F16Rows m1 = f16_rows_moments(C, K, [&](int q, int co) { return w[(size_t)co * K + q]; }, [](int) { return 0; }, std::vector<double>(1, in_typ));
        F16Range r{f16_layer_bound(w, C, K, none, false, none, none, false, in_bound), f16_layer_typ(w, C, K, none, false, in_typ)};
        r.ch = f16_rows_typ(m1, none, false, none, none, false);
        const F16Rows m2 = f16_rows_moments(N, C, [&](int q, int co) { return cw[(size_t)co * C + q]; }, [](int q) { return q; }, r.ch);
        CHECK(r.ok(), "spread %d: bound %g typ %g", spread, r.bound, r.typ);
        CHECK(f16_rows_ok(r.bound, m2) == !spread, "spread %d: bound %g seen %g", spread, r.bound, f16_rows_seen(m2));
    }
    // a row's RMS weight against the tensor's largest weight: 2^17 is the limit, a row of exact zeros is exempt
    const int R = 3, Kw = 8;
    std::vector<float> w = rand_vec((size_t)R * Kw, 0.5, 1.0);
    w[0] = 1.0f;
    auto weights_ok = [&] {
        return f16_rows_weights_ok(f16_rows_moments(R, Kw, [&](int q, int co) { return w[(size_t)co * Kw + q]; }, [](int) { return 0; }, std::vector<double>(1, 1.0)), Kw);
    };
    CHECK(weights_ok(), "rows of like magnitude");
    for (int k = 0; k < Kw; ++k) w[Kw + k] = std::ldexp(1.0f, -16);
    CHECK(weights_ok(), "a row 2^16 under the largest weight");
    for (int k = 0; k < Kw; ++k) w[Kw + k] = std::ldexp(1.0f, -18);
    CHECK(!weights_ok(), "a row 2^18 under the largest weight");
    for (int k = 0; k < Kw; ++k) w[Kw + k] = 0.0f;
    CHECK(weights_ok(), "a row of zeros");
}

// ---- balance_channels on conv3x3(1 -> 8) + ReLU read by a [4][8 * 2] layer: 3 x 4 input planes, two output pixels per channel
struct TinyNet {
    HostTensor w, b, g, beta, mean, var, fc;
    bool bn = false;
    BalanceLayer layer() { BalanceLayer L; L.w = &w; L.b = &b; if (bn) { L.g = &g; L.beta = &beta; L.mean = &mean; L.var = &var; } return L; }
    std::vector<HostTensor*> all() { return {&w, &b, &g, &beta, &mean, &var, &fc}; }
    // float32, one summation order; the BatchNorm folded the way the library folds it (alpha = g / sqrt(var + eps), beta - mean alpha)
    void forward(const float* x, float* out) const {
        float a[16];
        for (int c = 0; c < 8; ++c)
            for (int p = 0; p < 2; ++p) {
                float acc = 0.0f;
                for (int ky = 0; ky < 3; ++ky)
                    for (int kx = 0; kx < 3; ++kx) acc += w.data[c * 9 + ky * 3 + kx] * x[ky * 4 + kx + p];
                acc += b.data[c];
                if (bn) {
                    const float invstd = 1.0f / std::sqrt(var.data[c] + 1e-5f), al = g.data[c] * invstd, be = beta.data[c] - mean.data[c] * al;
                    acc = acc * al + be;
                }
                a[c * 2 + p] = acc > 0.0f ? acc : 0.0f;
            }
        for (int n = 0; n < 4; ++n) {
            float acc = 0.0f;
            for (int q = 0; q < 16; ++q) acc += fc.data[n * 16 + q] * a[q];
            out[n] = acc;
        }
    }
    // the largest per-channel bound, from the tensors as they are (the BatchNorm folded in double from the raw statistics)
    double bound(double in_bound) const {
        double worst = 0.0;
        for (int c = 0; c < 8; ++c) {
            double t = 0.0;
            for (int k = 0; k < 9; ++k) t += std::fabs((double)w.data[c * 9 + k]);
            t = t * in_bound + std::fabs((double)b.data[c]);
            if (bn) {
                const double al = (double)g.data[c] / std::sqrt((double)var.data[c] + 1e-5), be = (double)beta.data[c] - (double)mean.data[c] * al;
                t = t * std::fabs(al) + std::fabs(be);
            }
            worst = std::fmax(worst, t);
        }
        return worst;
    }
};
static TinyNet tiny_net(bool bn) {
    TinyNet t;
    t.bn = bn;
    t.w.shape = {8, 1, 3, 3}; t.w.data = rand_vec(72, -1.0, 1.0);
    t.b.shape = {8}; t.b.data = rand_vec(8, -0.5, 0.5);
    t.g.shape = t.beta.shape = t.mean.shape = t.var.shape = {8};
    t.g.data = rand_vec(8, 0.8, 1.25); t.beta.data = rand_vec(8, -0.5, 0.5); t.mean.data = rand_vec(8, -0.5, 0.5); t.var.data = rand_vec(8, 0.8, 1.25);
    t.fc.shape = {4, 16}; t.fc.data = rand_vec(64, -1.0, 1.0);
    return t;
}
// channel c at 2^e times its gain, the weights that read it at 2^-e: the same function
static void set_gain(TinyNet& t, int c, int e) {
    if (t.bn) { t.g.data[c] = std::ldexp(t.g.data[c], e); t.beta.data[c] = std::ldexp(t.beta.data[c], e); }
    else { for (int k = 0; k < 9; ++k) t.w.data[c * 9 + k] = std::ldexp(t.w.data[c * 9 + k], e); t.b.data[c] = std::ldexp(t.b.data[c], e); }
    for (int n = 0; n < 4; ++n)
        for (int p = 0; p < 2; ++p) t.fc.data[n * 16 + c * 2 + p] = std::ldexp(t.fc.data[n * 16 + c * 2 + p], -e);
}
static void check_balance() {
    const double in_bound = 4.0;
    std::vector<float> xs = rand_vec(100 * 12, -in_bound, in_bound);
    for (int bn = 0; bn < 2; ++bn) {
        // one channel 2^10 above the rest
        TinyNet before = tiny_net(bn != 0);
        set_gain(before, 5, 10);
        TinyNet after = before;
        const double ret = balance_channels(after.layer(), {&after.fc}, in_bound);
        int moved = 0;
        const std::vector<HostTensor*> tb = before.all(), ta = after.all();
        for (size_t i = 0; i < tb.size(); ++i)
            for (size_t j = 0; j < tb[i]->data.size(); ++j) {
                const float x = tb[i]->data[j], y = ta[i]->data[j];
                if (x == 0.0f) { CHECK(y == 0.0f, "bn %d tensor %zu[%zu]: 0 -> %g", bn, i, j, (double)y); continue; }
                CHECK(is_pow2((double)y / (double)x), "bn %d tensor %zu[%zu]: factor %.9g", bn, i, j, (double)y / (double)x);
                moved += y != x;
            }
        CHECK(moved > 0, "bn %d: nothing was balanced", bn);
        float o0[4], o1[4];
        for (int i = 0; i < 100; ++i) {
            before.forward(&xs[(size_t)i * 12], o0); after.forward(&xs[(size_t)i * 12], o1);
            CHECK(std::memcmp(o0, o1, sizeof o0) == 0, "bn %d input %d: %.9g %.9g %.9g %.9g -> %.9g %.9g %.9g %.9g", bn, i, (double)o0[0], (double)o0[1],
                  (double)o0[2], (double)o0[3], (double)o1[0], (double)o1[1], (double)o1[2], (double)o1[3]);
        }
        CHECK(ret == after.bound(in_bound), "bn %d: returned %.17g, the balanced tensors give %.17g", bn, ret, after.bound(in_bound));
        CHECK(after.bound(in_bound) < before.bound(in_bound) * 0.0625, "bn %d: bound %g -> %g", bn, before.bound(in_bound), after.bound(in_bound));
        // gains within 2^3 of each other: nothing is touched
        TinyNet mild = tiny_net(bn != 0);
        for (int c = 0; c < 8; ++c) set_gain(mild, c, c % 4);
        TinyNet kept = mild;
        const double ret2 = balance_channels(kept.layer(), {&kept.fc}, in_bound);
        const std::vector<HostTensor*> tm = mild.all(), tk = kept.all();
        for (size_t i = 0; i < tm.size(); ++i)
            CHECK(std::memcmp(tm[i]->data.data(), tk[i]->data.data(), tm[i]->data.size() * sizeof(float)) == 0, "bn %d tensor %zu changed", bn, i);
        CHECK(ret2 == mild.bound(in_bound), "bn %d: returned %.17g, the tensors give %.17g", bn, ret2, mild.bound(in_bound));
    }
}

int main() {
    check_scale();
    check_wscale();
    check_layer_bound();
    check_range_guards();
    check_balance();
    if (g_fail) { std::printf("%d check(s) failed\n", g_fail); return 1; }
    std::printf("ok\n");
    return 0;
}
