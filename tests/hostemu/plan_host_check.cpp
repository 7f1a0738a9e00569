// plan_host_check.cpp - the planner's value arithmetic (csrc/plan_host.h) held to what its comments promise (tests/test_plan_host.py):
// the power-of-two scales against the binary16 range, the layer bound against sampled and sign-aligned inputs, the range guards on a
// model with uniform channel gains and on one whose gains spread, and the load-time channel balance against a float32 forward of a
// tiny conv + ReLU + Linear net written out here - and, for a channel with two producers, of a tiny two-branch block; the guard of the
// operands that are scaled per pixel row.
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

// ---- balance_channels with TWO producers of one channel (a BcResNet block): h[c] = ReLU(BN1(pw[c] . d)) + BN2(sc[c] . xs), 8 channels on
// 6 inputs each, read by a [4][8] and a [3][8] layer (the next block's pointwise and shortcut)
struct DualNet {
    HostTensor pw, sc, g1, beta1, mean1, var1, g2, beta2, mean2, var2, n1, n2;
    std::vector<BalanceLayer> layers() {
        BalanceLayer a, b;
        a.w = &pw; a.g = &g1; a.beta = &beta1; a.mean = &mean1; a.var = &var1;
        b.w = &sc; b.g = &g2; b.beta = &beta2; b.mean = &mean2; b.var = &var2;
        return {a, b};
    }
    std::vector<HostTensor*> all() { return {&pw, &sc, &g1, &beta1, &mean1, &var1, &g2, &beta2, &mean2, &var2, &n1, &n2}; }
    static float bn(float acc, const HostTensor& g, const HostTensor& beta, const HostTensor& mean, const HostTensor& var, int c) {
        const float invstd = 1.0f / std::sqrt(var.data[c] + 1e-5f), al = g.data[c] * invstd, be = beta.data[c] - mean.data[c] * al;
        return acc * al + be;
    }
    void forward(const float* d, const float* xs, float* out) const {      // float32, one summation order, the library's fold
        float h[8];
        for (int c = 0; c < 8; ++c) {
            float a = 0.0f, r = 0.0f;
            for (int k = 0; k < 6; ++k) { a += pw.data[c * 6 + k] * d[k]; r += sc.data[c * 6 + k] * xs[k]; }
            a = bn(a, g1, beta1, mean1, var1, c); r = bn(r, g2, beta2, mean2, var2, c);
            h[c] = (a > 0.0f ? a : 0.0f) + r;
        }
        for (int n = 0; n < 4; ++n) { float acc = 0.0f; for (int c = 0; c < 8; ++c) acc += n1.data[n * 8 + c] * h[c]; out[n] = acc; }
        for (int n = 0; n < 3; ++n) { float acc = 0.0f; for (int c = 0; c < 8; ++c) acc += n2.data[n * 8 + c] * h[c]; out[4 + n] = acc; }
    }
    double bound(double bd, double bx) const {                            // the largest channel's: the SUM of the two branches' bounds
        double worst = 0.0;
        for (int c = 0; c < 8; ++c) {
            double t1 = 0.0, t2 = 0.0;
            for (int k = 0; k < 6; ++k) { t1 += std::fabs((double)pw.data[c * 6 + k]); t2 += std::fabs((double)sc.data[c * 6 + k]); }
            const double al1 = (double)g1.data[c] / std::sqrt((double)var1.data[c] + 1e-5), be1 = (double)beta1.data[c] - (double)mean1.data[c] * al1;
            const double al2 = (double)g2.data[c] / std::sqrt((double)var2.data[c] + 1e-5), be2 = (double)beta2.data[c] - (double)mean2.data[c] * al2;
            worst = std::fmax(worst, (t1 * bd * std::fabs(al1) + std::fabs(be1)) + (t2 * bx * std::fabs(al2) + std::fabs(be2)));
        }
        return worst;
    }
};
static DualNet dual_net() {
    DualNet t;
    t.pw.shape = t.sc.shape = {8, 6, 1, 1}; t.pw.data = rand_vec(48, -1.0, 1.0); t.sc.data = rand_vec(48, -1.0, 1.0);
    for (HostTensor* v : {&t.g1, &t.beta1, &t.mean1, &t.var1, &t.g2, &t.beta2, &t.mean2, &t.var2}) v->shape = {8};
    t.g1.data = rand_vec(8, 0.8, 1.25); t.beta1.data = rand_vec(8, -0.5, 0.5); t.mean1.data = rand_vec(8, -0.5, 0.5); t.var1.data = rand_vec(8, 0.8, 1.25);
    t.g2.data = rand_vec(8, 0.8, 1.25); t.beta2.data = rand_vec(8, -0.5, 0.5); t.mean2.data = rand_vec(8, -0.5, 0.5); t.var2.data = rand_vec(8, 0.8, 1.25);
    t.n1.shape = {4, 8, 1, 1}; t.n1.data = rand_vec(32, -1.0, 1.0);
    t.n2.shape = {3, 8, 1, 1}; t.n2.data = rand_vec(24, -1.0, 1.0);
    return t;
}
static void set_dual_gain(DualNet& t, int c, int e) {                      // both BatchNorms of channel c x 2^e, both readers' columns x 2^-e
    for (HostTensor* v : {&t.g1, &t.beta1, &t.g2, &t.beta2}) v->data[c] = std::ldexp(v->data[c], e);
    for (int n = 0; n < 4; ++n) t.n1.data[n * 8 + c] = std::ldexp(t.n1.data[n * 8 + c], -e);
    for (int n = 0; n < 3; ++n) t.n2.data[n * 8 + c] = std::ldexp(t.n2.data[n * 8 + c], -e);
}
static void check_balance_two_producers() {
    const double bd = 6.0, bx = 4.0;
    const std::vector<float> ds = rand_vec(100 * 6, -bd, bd), xs = rand_vec(100 * 6, -bx, bx);
    for (int e : {10, -10}) {
        DualNet before = dual_net();
        set_dual_gain(before, 5, e);
        DualNet after = before;
        const double ret = balance_channels(after.layers(), {bd, bx}, {&after.n1, &after.n2});
        int moved = 0;
        const std::vector<HostTensor*> tb = before.all(), ta = after.all();
        for (size_t i = 0; i < tb.size(); ++i)
            for (size_t j = 0; j < tb[i]->data.size(); ++j) {
                const float x = tb[i]->data[j], y = ta[i]->data[j];
                if (x == 0.0f) { CHECK(y == 0.0f, "dual tensor %zu[%zu]: 0 -> %g", i, j, (double)y); continue; }
                CHECK(is_pow2((double)y / (double)x), "dual tensor %zu[%zu]: factor %.9g", i, j, (double)y / (double)x);
                moved += y != x;
            }
        CHECK(moved > 0, "dual 2^%d: nothing was balanced", e);
        // the two BatchNorms of a channel take the SAME power of two, the convolutions and the statistics none
        for (int c = 0; c < 8; ++c) {
            const double f = (double)after.g1.data[c] / (double)before.g1.data[c];
            CHECK(f == (double)after.g2.data[c] / (double)before.g2.data[c] && f == (double)after.beta1.data[c] / (double)before.beta1.data[c] &&
                  f == (double)after.beta2.data[c] / (double)before.beta2.data[c], "dual 2^%d channel %d: unequal factors", e, c);
            CHECK((c == 5) == (f != 1.0), "dual 2^%d channel %d: factor %g", e, c, f);
        }
        CHECK(after.pw.data == before.pw.data && after.sc.data == before.sc.data && after.var1.data == before.var1.data && after.mean2.data == before.mean2.data,
              "dual 2^%d: a convolution or a statistic moved", e);
        float o0[7], o1[7];
        for (int i = 0; i < 100; ++i) {
            before.forward(&ds[(size_t)i * 6], &xs[(size_t)i * 6], o0); after.forward(&ds[(size_t)i * 6], &xs[(size_t)i * 6], o1);
            CHECK(std::memcmp(o0, o1, sizeof o0) == 0, "dual 2^%d input %d: %.9g .. -> %.9g ..", e, i, (double)o0[0], (double)o1[0]);
        }
        CHECK(ret == after.bound(bd, bx), "dual 2^%d: returned %.17g, the balanced tensors give %.17g", e, ret, after.bound(bd, bx));
        if (e > 0) CHECK(after.bound(bd, bx) < before.bound(bd, bx) * 0.0625, "dual: bound %g -> %g", before.bound(bd, bx), after.bound(bd, bx));
    }
    DualNet mild = dual_net();
    for (int c = 0; c < 8; ++c) set_dual_gain(mild, c, c % 4);
    DualNet kept = mild;
    const double ret2 = balance_channels(kept.layers(), {bd, bx}, {&kept.n1, &kept.n2});
    const std::vector<HostTensor*> tm = mild.all(), tk = kept.all();
    for (size_t i = 0; i < tm.size(); ++i)
        CHECK(std::memcmp(tm[i]->data.data(), tk[i]->data.data(), tm[i]->data.size() * sizeof(float)) == 0, "dual mild: tensor %zu changed", i);
    CHECK(ret2 == mild.bound(bd, bx), "dual mild: returned %.17g, the tensors give %.17g", ret2, mild.bound(bd, bx));
}

// ---- f16_pixel_rows_ok: operands scaled per pixel row, weights per tensor - a channel (and the column that compensates it) 2^g off the rest
static void check_pixel_rows() {
    const int N = 6, K = 8;
    auto ok = [&](const std::vector<float>& w, const std::vector<double>& typ) {
        return f16_pixel_rows_ok(f16_rows_moments(N, K, [&](int q, int co) { return w[(size_t)co * K + q]; }, [](int q) { return q; }, typ), typ);
    };
    const std::vector<float> w0 = rand_vec((size_t)N * K, 0.5, 1.0);
    const std::vector<double> t0(K, 3.0);
    CHECK(ok(w0, t0), "uniform channels");
    for (int g : {-24, -20, -8, 8, 20, 24}) {                   // channel 2 x 2^g, its column x 2^-g: passes at 2^8, fails at 2^20 and beyond
        std::vector<float> w = w0;
        std::vector<double> t = t0;
        t[2] = std::ldexp(t[2], g);
        for (int n = 0; n < N; ++n) w[(size_t)n * K + 2] = std::ldexp(w[(size_t)n * K + 2], -g);
        CHECK(ok(w, t) == (std::abs(g) == 8), "channel 2 x 2^%d compensated", g);
    }
    std::vector<double> t = t0;
    t[2] = std::ldexp(t[2], -24);                               // a quiet channel nothing compensates loses bits nobody reads: fine
    CHECK(ok(w0, t), "a quiet channel with ordinary weights");
    std::vector<float> w = w0;
    for (int k = 0; k < K; ++k) w[(size_t)3 * K + k] = 0.0f;    // a row of zeros is exempt
    CHECK(ok(w, t0), "a row of zeros");
    CHECK(!ok(w0, std::vector<double>(K, 0.0)), "no magnitude known");
}

int main() {
    check_balance_two_producers();
    check_pixel_rows();
    check_scale();
    check_wscale();
    check_layer_bound();
    check_range_guards();
    check_balance();
    if (g_fail) { std::printf("%d check(s) failed\n", g_fail); return 1; }
    std::printf("ok\n");
    return 0;
}
