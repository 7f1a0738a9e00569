// plan_host.h - the value arithmetic of the planner: what nww_finalize derives from the weights' VALUES - the two-term binary16 scales,
// the bounds and typical magnitudes of a layer's output, the per-row guards, the load-time channel balance.  Host-only (no HIP header,
// no handle; g++ compiles it for tests/test_plan_host.py); nww_plan.hip and nww_weights.hip decide with it which kernel a step runs.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

struct HostTensor {
    std::vector<int64_t> shape;
    std::vector<float> data;
    bool loaded = false;
    size_t dev_off = 0;     // float offset in the weight arena
};

// ---- two-term binary16 arithmetic (NWW_ARITH_F16X3): plan-time bounds and power-of-two scales
inline double f16_pow2_floor(double x) { int e; (void)std::frexp(x, &e); return std::ldexp(1.0, e - 1); }      // largest power of two <= x
// scale that keeps |v| <= bound inside the binary16 range (65504), with 2 % to spare for the host / device difference of the bound
inline float f16_scale(double bound) {
    if (!(bound < 1e30)) return 0.0f;                             // no usable bound (a NaN among them)
    if (!(bound > 1e-30)) bound = 1e-30;
    double s = f16_pow2_floor(65504.0 / (bound * 1.02));
    if (s > 1099511627776.0) s = 1099511627776.0;                // 2^40
    return (float)s;
}
inline float f16_wscale(const std::vector<float>& w) {            // the largest weight lands in [2^14, 2^15)
    double m = 0;
    for (float x : w) m = std::fmax(m, std::fabs((double)x));
    return f16_scale(m * 2.0);
}
// |act((sum_k w[c][k] x[k] + b[c]) al[c] + be[c])| <= max_c (sum_k |w[c][k]| bound + |b[c]|) |al[c]| + |be[c]| for ReLU / GELU / SiLU
inline double f16_layer_bound(const std::vector<float>& w, int Cout, int K, const std::vector<float>& b, bool has_b,
                              const std::vector<float>& al, const std::vector<float>& be, bool has_bn, double in_bound) {
    double worst = 0;
    for (int c = 0; c < Cout; ++c) {
        double t = 0;
        for (int k = 0; k < K; ++k) t += std::fabs((double)w[(size_t)c * K + k]);
        t = t * in_bound + (has_b ? std::fabs((double)b[c]) : 0.0);
        if (has_bn) t = t * std::fabs((double)al[c]) + std::fabs((double)be[c]);
        worst = std::fmax(worst, t);
    }
    return worst;
}
// scale of the LayerNorm'd rows that the ffn_x3 epilogues sum exactly over time: |LayerNorm| x scale <= 2^36; 0 = no usable bound
inline float f16_mean_scale(double bound) {
    const float s = bound < 1e30 ? (float)f16_pow2_floor(68719476736.0 / std::fmax(bound, 1e-30)) : 0.0f;
    return s > 0.0f && std::isfinite(s) ? s : 0.0f;
}

// A tensor's plan-time range: a BOUND on its magnitude (what the scale is derived from) and a rough TYPICAL magnitude.  Two binary16
// terms hold 22-23 bits of a value down to 2^-17 of the scaled bound; a bound that is more pessimistic than that against the values
// that matter would cost precision silently - so a layer takes the two-term form only when bound <= 2^16 typ (typ-sized values then
// sit at >= 2^-1 after scaling, one bit above where `lo` starts to lose bits), and otherwise stays on
// the three-term bf16 form (which has float32's range and needs no bound).  typ: the head's features ~ 32 (dB values), a layer's
// output ~ sqrt(sum_k w^2) typ_in (uncorrelated terms; |folded-BN alpha| applied) - order-of-magnitude, which is all the guard needs.
// how far above the typical magnitude a worst-case bound may lie: 2^16 leaves typical values 22+ significant bits in two binary16 terms.
// NWW_F16_RANGE_LOG2 (A/B and test knob): a larger exponent lets deeper stages take the two-term kernels at reduced precision of small values
// (defined by whoever includes this: nww_plan.hip from the knob, a check program as it likes)
double f16_range_factor();
struct F16Range {
    double bound = 0.0, typ = 0.0;
    std::vector<double> ch;                               // the typical magnitude per channel (f16_rows_typ); empty: only the mean is known
    bool ok() const { return bound > 0.0 && typ > 0.0 && bound <= typ * f16_range_factor(); }
};
// The mean over the channels (f16_layer_typ) cannot see a model whose channel gains spread: a channel whose gain is G times the others' (and
// whose weights in the next layer are 1 / G) puts G / Cout into the mean and hides the others, which then sit G below the bound.  So a
// plan-time-scaled operand is also held against what each CONSUMER ROW sees of it.  Per row co of the layer that reads the operand:
// sig2 = sum_q w_q^2 typ_q^2 over the contraction (typ_q: the typical magnitude of the input channel of index q) and norm2 = sum_q w_q^2.
// The operand's absolute error (2^-25 / scale on a value far below the bound) reaches row co through the row's 2-norm, so the operand's
// magnitude as co sees it is sqrt(sig2 / norm2); a row with no weight reads nothing and a channel no row reads weighs nothing.  The
// smallest of those is held against the bound: within 2^4 f16_range_factor() (2^20: the quietest row keeps 20 bits, 1e-6; taken against
// the quietest row and not a mean, hence the 2^4).  Used by the raw frontend's planes, add_trunk, add_conv_mfma and fc1's operand.
struct F16Rows { std::vector<double> sig2, norm2; double wmax = 0.0; };
// w_at(q, co): the weight of row co at contraction index q; ch_of(q): the input channel of index q
template <class WAt, class ChOf>
F16Rows f16_rows_moments(int Cout, int K, WAt&& w_at, ChOf&& ch_of, const std::vector<double>& typ_in) {
    F16Rows m;
    m.sig2.assign(Cout, 0.0); m.norm2.assign(Cout, 0.0);
    for (int q = 0; q < K; ++q) {
        const double t = typ_in[ch_of(q)];
        for (int co = 0; co < Cout; ++co) {
            const double w = (double)w_at(q, co), w2 = w * w;
            m.norm2[co] += w2; m.sig2[co] += w2 * t * t;
            m.wmax = std::fmax(m.wmax, std::fabs(w));
        }
    }
    return m;
}
inline double f16_rows_seen(const F16Rows& m) {          // the operand as its quietest consumer row sees it; INFINITY: no row reads it
    double seen = INFINITY;
    for (size_t co = 0; co < m.norm2.size(); ++co) if (m.norm2[co] > 0.0) seen = std::fmin(seen, std::sqrt(m.sig2[co] / m.norm2[co]));
    return seen;
}
inline bool f16_rows_ok(double bound, const F16Rows& m) {
    const double seen = f16_rows_seen(m);
    return seen < INFINITY && bound <= seen * std::ldexp(f16_range_factor(), 4);
}
// The weights' side of the same thing: one power of two per tensor puts its largest weight in [2^14, 2^15), and a weight's `lo` term keeps
// its 11 bits down to 2^-3 - so every row's RMS weight has to lie within 2^17 of the largest weight (a convolution without a BatchNorm whose
// one output channel is G times the others' carries G in its own rows).  Conservative on purpose: one nearly dead row (pruned to 2^-17 of
// the largest weight but not to zero) sends the layer to three terms although its lost bits cannot matter - the result stays right, the
// step is slower; a row of exact zeros is exempt
inline bool f16_rows_weights_ok(const F16Rows& m, int K) {
    for (size_t co = 0; co < m.norm2.size(); ++co)
        if (m.norm2[co] > 0.0 && m.wmax > std::sqrt(m.norm2[co] / K) * 131072.0) return false;
    return true;
}
// the rows' outputs, per channel: typ_co = sqrt(sig2 + b^2), through a folded BatchNorm sqrt(sig2 al^2 + (b al + be)^2)
inline std::vector<double> f16_rows_typ(const F16Rows& m, const std::vector<float>& b, bool has_b, const std::vector<float>& al,
                                        const std::vector<float>& be, bool has_bn) {
    std::vector<double> typ(m.sig2.size(), 0.0);
    for (size_t co = 0; co < typ.size(); ++co) {
        const double bb = has_b ? (double)b[co] : 0.0;
        typ[co] = has_bn ? std::sqrt(m.sig2[co] * (double)al[co] * (double)al[co] + (bb * (double)al[co] + (double)be[co]) * (bb * (double)al[co] + (double)be[co]))
                         : std::sqrt(m.sig2[co] + bb * bb);
    }
    return typ;
}
inline double f16_layer_typ(const std::vector<float>& w, int Cout, int K, const std::vector<float>& al, bool has_bn, double typ_in) {
    double acc = 0;
    for (int c = 0; c < Cout; ++c) {
        double q = 0;
        for (int k = 0; k < K; ++k) q += (double)w[(size_t)c * K + k] * (double)w[(size_t)c * K + k];
        acc += std::sqrt(q) * (has_bn ? std::fabs((double)al[c]) : 1.0);
    }
    return acc / (Cout > 0 ? Cout : 1) * typ_in;
}

// ---- channel gains balanced at load time (two-term arithmetic, ReLU heads with a plan-time-scaled conv trunk: cnn, crnn, e2e_dnn; and
// BcResNet's blocks, whose operands are scaled per pixel row - a spread of channel gains costs the same bits there, see f16_pixel_rows_ok)
// One power of two per TENSOR serves conv1's and conv2's outputs, so a channel whose gain is G times the others' pushes them log2 G bits
// down the operand, and the range guard (F16Range, f16_rows_ok) then has to send the layer that reads it to three terms.  ReLU and the
// pools are positively homogeneous: channel c of a layer x s_c and the next layer's weights on c / s_c, s_c a power of two, is the same
// function with the same float32 bits.  So a channel whose worst-case bound lies 2^4 or more off the layer's median channel (the upper
// median over the channels that count, see below) is given the
// power of two that brings it next to the median - through the BatchNorm's weight and bias where the layer has one (the fold sees them),
// else through the convolution's row and bias - before the BatchNorms are folded and the arena is uploaded.  Ordinary models (channel
// bounds within a few x of each other) are not touched; GELU / SiLU heads cannot be (the guard decides for them).  -> the layer's bound after
// (the per-channel bound folds the BatchNorm in double from the raw statistics - not f16_layer_bound's float32 folded factors: the two differ in the last bits)
struct BalanceLayer { HostTensor *w = nullptr, *b = nullptr, *g = nullptr, *beta = nullptr, *mean = nullptr, *var = nullptr; };
// A channel may have several PRODUCERS that are added behind their BatchNorms (BcResNet: bn1 and shortcut.1 of one block; the activation sits
// on one branch only, so the channel is positively homogeneous in the pair).  Its bound is the sum of the producers' bounds (each on its own
// input bound) and every producer takes the same 2^e.  One producer is the plain form above, to the bit.
inline double balance_channels(const std::vector<BalanceLayer>& Ls, const std::vector<double>& in_bounds, const std::vector<HostTensor*>& consumers) {
    const int Cout = (int)Ls[0].w->shape[0];
    std::vector<double> bound(Cout, 0.0);
    for (size_t l = 0; l < Ls.size(); ++l) {
        const BalanceLayer& L = Ls[l];
        const int K = (int)(L.w->data.size() / Cout);
        for (int c = 0; c < Cout; ++c) {
            double t = 0.0;
            for (int k = 0; k < K; ++k) t += std::fabs((double)L.w->data[(size_t)c * K + k]);
            t = t * in_bounds[l] + (L.b ? std::fabs((double)L.b->data[c]) : 0.0);
            if (L.g) {
                const double al = (double)L.g->data[c] / std::sqrt((double)L.var->data[c] + 1e-5), be = (double)L.beta->data[c] - (double)L.mean->data[c] * al;
                t = t * std::fabs(al) + std::fabs(be);
            }
            bound[c] = l == 0 ? t : bound[c] + t;
        }
    }
    // what a channel is worth to the layer behind it: its bound times the 2-norm of the weights that read it.  A channel worth less than 2^-8
    // of the layer's best (a nearly dead BatchNorm channel, a pruned column) is neither moved nor counted: the median is taken over the rest
    std::vector<double> worth(Cout, 0.0);
    double best = 0.0;
    for (int c = 0; c < Cout; ++c) {
        double q = 0.0;
        for (HostTensor* W : consumers) {
            const size_t N = (size_t)W->shape[0], Kc = W->data.size() / N, per = Kc / Cout;
            for (size_t n = 0; n < N; ++n)
                for (size_t j = 0; j < per; ++j) { const double v = (double)W->data[n * Kc + (size_t)c * per + j]; q += v * v; }
        }
        worth[c] = bound[c] * std::sqrt(q);
        if (std::isfinite(worth[c])) best = std::fmax(best, worth[c]);
    }
    std::vector<double> sorted;
    for (int c = 0; c < Cout; ++c) if (worth[c] > 0.0 && worth[c] >= best * 0.00390625) sorted.push_back(bound[c]);
    std::sort(sorted.begin(), sorted.end());
    const double med = sorted.empty() ? 0.0 : sorted[sorted.size() / 2];
    double worst = 0.0;
    for (int c = 0; c < Cout; ++c) {
        int e = 0;
        if (med > 0.0 && worth[c] > 0.0 && worth[c] >= best * 0.00390625 && std::isfinite(bound[c]) && std::isfinite(med)) {
            const double l = std::log2(bound[c] / med);
            if (std::fabs(l) >= 4.0 && std::fabs(l) <= 40.0) e = -(int)std::lround(l);
        }
        if (e != 0) {
            const float s = std::ldexp(1.0f, e), r = std::ldexp(1.0f, -e);
            for (const BalanceLayer& L : Ls) {
                const int K = (int)(L.w->data.size() / Cout);
                if (L.g) { L.g->data[c] *= s; L.beta->data[c] *= s; }
                else { for (int k = 0; k < K; ++k) L.w->data[(size_t)c * K + k] *= s; if (L.b) L.b->data[c] *= s; }
            }
            for (HostTensor* W : consumers) {                   // [N][Cout * per]: channel c is columns c per .. c per + per - 1
                const size_t N = (size_t)W->shape[0], Kc = W->data.size() / N, per = Kc / Cout;
                for (size_t n = 0; n < N; ++n)
                    for (size_t j = 0; j < per; ++j) W->data[n * Kc + (size_t)c * per + j] *= r;
            }
        }
        worst = std::fmax(worst, std::ldexp(bound[c], e));
    }
    return worst;
}
inline double balance_channels(const BalanceLayer& L, const std::vector<HostTensor*>& consumers, double in_bound) {
    return balance_channels(std::vector<BalanceLayer>{L}, std::vector<double>{in_bound}, consumers);
}

// ---- operands scaled per pixel row in the kernel (dual_x3 / bc_chain under NWW_ARITH_F16X3): the row's largest element lands in
// [2^14, 2^15) and W carries one power of two per tensor, so no tensor bound is needed - but an element 2^g below its row's (its tensor's)
// largest keeps min(22, 38 - g) bits: the absolute error of a scaled value is 2^-25 once its `lo` term is subnormal, 2^-39 of the largest.
// An activation channel's lost bits reach output row co through W's column on it, a weight's through the activations it multiplies, so
// with typ[c] the per-channel typical magnitudes of the operand and (sig2, norm2, wmax) the moments of W on them (f16_rows_moments):
//   activations: 2^-39 max_c typ[c] sqrt(norm2[co]) against the row's output sqrt(sig2[co])   ->  max typ <= window x f16_rows_seen
//   weights:     2^-39 wmax sqrt(sum_c typ[c]^2)   against the same                           ->  wmax |typ| <= window x sqrt(sig2[co])
// window = f16_range_factor() (2^16: 22 bits, as F16Range::ok; no 2^4 on top as in f16_rows_ok - nothing here is a worst-case bound).
// Uniform channels pass with 2^12 to spare; a channel 2^g louder or quieter than its neighbours (compensated in W's column) fails from
// g ~ 16 + log2 sqrt(K) at the latest.  A row or channel of exact zeros is exempt.  What fails stays on the three-term bf16 form
inline bool f16_pixel_rows_ok(const F16Rows& m, const std::vector<double>& typ) {
    double tmax = 0.0, t2 = 0.0;
    for (double t : typ) { tmax = std::fmax(tmax, t); t2 += t * t; }
    if (!(tmax > 0.0) || !std::isfinite(t2)) return false;
    const double window = f16_range_factor(), seen = f16_rows_seen(m);
    if (!(seen < INFINITY) || !(tmax <= seen * window)) return false;
    for (size_t co = 0; co < m.norm2.size(); ++co)
        if (m.norm2[co] > 0.0 && !(m.wmax * std::sqrt(t2) <= std::sqrt(m.sig2[co]) * window)) return false;
    return true;
}
