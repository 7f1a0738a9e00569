// rnn_cell.h - gate functions of the recurrence kernels (rnn_f32.hip, rnn_x3.hip, rnn_stream.hip) and the float32 cell update.
#pragma once
#include <hip/hip_runtime.h>

// Gate functions of the register-resident recurrences on the hardware exp2 and reciprocal (1 ulp each): absolute error
// <= 2e-7 against ~30 (sigmoid: expf + IEEE division) and ~40 (tanhf) instructions each - the gate arithmetic of a step was
// as long as its matrix products.  tanh x = 1 - 2 / (1 + e^2x) saturates correctly through exp2 = 0 / inf.
__device__ __forceinline__ float rnn_sigmoid(float v) { return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-1.4426950408889634f * v)); }
__device__ __forceinline__ float rnn_tanh(float v) { return 1.0f - 2.0f * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(2.8853900817779268f * v)); }

// the two flavours a float32 kernel picks from: the hardware forms above, or the library's (expf + an IEEE division, tanhf)
struct GatesHw {
    static __device__ __forceinline__ float sigmoid(float v) { return rnn_sigmoid(v); }
    static __device__ __forceinline__ float tanh(float v) { return rnn_tanh(v); }
};
struct GatesLib {
    static __device__ __forceinline__ float sigmoid(float v) { return 1.0f / (1.0f + expf(-v)); }
    static __device__ __forceinline__ float tanh(float v) { return tanhf(v); }
};

// Gate q's element r of the MFMA accumulators acc[q] (a cell's row of h W_hh^T), read where the cell uses it
template <class V>
struct AccRow {
    const V* acc; int r;
    __device__ __forceinline__ float operator[](int q) const { return acc[q][r]; }
};
template <class V>
__device__ __forceinline__ AccRow<V> acc_row(const V* acc, int r) { return AccRow<V>{acc, r}; }

// One float32 cell update of a (clip, hidden unit), PyTorch semantics.  Per gate q: x[q ldx] = its element of x W_ih^T + b_ih (registers with
// ldx = 1, or the xg row in memory with ldx = H), hg[q] = of h W_hh^T (acc_row), b[q] = of b_hh.
//   G = 3, nn.GRU (r, z, n):     r, z = sigmoid(x + hg + b); n = tanh(x_n + r (hg_n + b_n)); h' = (1 - z) n + z h
//   G = 4, nn.LSTM (i, f, g, o): i, f, o = sigmoid(x + hg + b), g = tanh(.); c' = f c + i g; h' = o tanh(c')
// `state` is what the cell carries from step to step - h for the GRU, c for the LSTM - and is replaced by its new value; returns h'.
// F: GatesHw / GatesLib.  The compiler contracts these expressions to FMAs as they are parenthesised: the results' last bits depend on
// their shape.
template <int G, class F, class A>
__device__ __forceinline__ float rnn_cell(const float* x, int ldx, const A& hg, const float (&b)[G], float& state) {
    static_assert(G == 3 || G == 4, "GRU or LSTM");
    if constexpr (G == 3) {
        const float rg = F::sigmoid(x[0] + hg[0] + b[0]);
        const float zg = F::sigmoid(x[ldx] + hg[1] + b[1]);
        const float ng = F::tanh(x[2 * ldx] + rg * (hg[2] + b[2]));
        state = (1.0f - zg) * ng + zg * state;
        return state;
    } else {
        const float ig = F::sigmoid(x[0] + hg[0] + b[0]);
        const float fg = F::sigmoid(x[ldx] + hg[1] + b[1]);
        const float gg = F::tanh(x[2 * ldx] + hg[2] + b[2]);
        const float og = F::sigmoid(x[3 * ldx] + hg[3] + b[3]);
        state = fg * state + ig * gg;
        return og * F::tanh(state);
    }
}
