// nww_weights.hip - Model.state_dict() spec per head, and what nww_finalize does to the loaded weights before it plans: BatchNorm
// folding, derived layouts, the device arena and the frontend's tables.
#include "nww_internal.h"

// ------------------------------------------------------------------------------------------ spec
namespace {
using Shape = std::vector<int64_t>;
struct SpecBuilder {
    std::vector<std::string>& keys;
    std::map<std::string, HostTensor>& t;
    void add(const std::string& k, Shape s) { keys.push_back(k); t[k].shape = std::move(s); }
    void lin(const std::string& p, int out, int in) { add(p + ".weight", {out, in}); add(p + ".bias", {out}); }
    void ln(const std::string& p, int d) { add(p + ".weight", {d}); add(p + ".bias", {d}); }
    void bn(const std::string& p, int c) {
        add(p + ".weight", {c}); add(p + ".bias", {c}); add(p + ".running_mean", {c}); add(p + ".running_var", {c});
    }
    void gru(const std::string& p, int in, int H, int layers, int G = 3) {   // G = 3: nn.GRU, 4: nn.LSTM
        for (int l = 0; l < layers; ++l) {
            const int isz = l == 0 ? in : 2 * H;
            for (const char* sfx : {"", "_reverse"}) {
                const std::string s = "_l" + std::to_string(l) + sfx;
                add(p + ".weight_ih" + s, {G * H, isz}); add(p + ".weight_hh" + s, {G * H, H});
                add(p + ".bias_ih" + s, {G * H}); add(p + ".bias_hh" + s, {G * H});
            }
        }
    }
};

void crnn_out(const nww_config& c, int* C, int* H, int* W) {
    int h = c.in_rows, w = c.in_cols;
    for (int i = 0; i < c.n_crnn_channels; ++i) { h /= 2; w /= 2; }
    *C = c.crnn_channels[c.n_crnn_channels - 1]; *H = h; *W = w;
}

// Mirrors nanowakeword_amd/config.py:param_spec == Model.state_dict() of the reference (model.py:67-296).
}  // namespace

void nww_build_spec(nww_handle* h) {
    const nww_config& c = h->cfg;
    SpecBuilder s{h->keys, h->tensors};
    const int T = c.in_rows, F = c.in_cols, L = c.layer_dim, E = c.embedding_dim, nb = c.n_blocks;
    // the raw-PCM heads: RawAudioFrontend's Conv1d (no bias) + BatchNorm1d per stage (channels in layer_dim, depth in n_blocks)
    auto raw_frontend = [&] {
        for (int i = 0, cin = 1; i < nb; ++i) {
            const int co = L << i;
            s.add("model.frontend.conv_blocks." + std::to_string(3 * i) + ".weight", {co, cin, i == 0 ? 41 : 13});
            s.bn("model.frontend.conv_blocks." + std::to_string(3 * i + 1), co);
            cin = co;
        }
    };
    switch (c.head_type) {
        case NWW_HEAD_DNN:
            s.lin("model.layer1", L, T * F); s.ln("model.layernorm1", L);
            for (int i = 0; i < nb; ++i) {
                const std::string p = "model.blocks." + std::to_string(i);
                s.lin(p + ".fcn_layer", L, L); s.ln(p + ".layer_norm", L);
            }
            s.lin("model.last_layer", E, L);
            break;
        case NWW_HEAD_CNN:
            s.add("model.conv1.weight", {16, 1, 3, 3}); s.add("model.conv1.bias", {16});
            s.add("model.conv2.weight", {32, 16, 3, 3}); s.add("model.conv2.bias", {32});
            s.lin("model.fc1", 128, 32 * (T / 4) * (F / 4)); s.lin("model.fc2", E, 128);
            break;
        case NWW_HEAD_CRNN: {
            int cin = 1;
            for (int i = 0; i < c.n_crnn_channels; ++i) {
                const int co = c.crnn_channels[i];
                const std::string p = "model.cnn." + std::to_string(4 * i);
                s.add(p + ".weight", {co, cin, 3, 3}); s.add(p + ".bias", {co});
                s.bn("model.cnn." + std::to_string(4 * i + 1), co);
                cin = co;
            }
            int C, H, W; crnn_out(c, &C, &H, &W);
            s.gru("model.rnn", C * H, L, nb, c.crnn_rnn_lstm ? 4 : 3); s.lin("model.fc", E, 2 * L);
            break;
        }
        case NWW_HEAD_GRU:
            s.gru("model.gru", F, L, nb); s.lin("model.fc", E, 2 * L);
            break;
        case NWW_HEAD_RNN:                        // RNNModel (architectures.py:149-161): nn.LSTM(F, 64, n_blocks), Linear(128, E)
            s.gru("model.layer1", F, 64, nb, 4); s.lin("model.layer2", E, 128);
            break;
        case NWW_HEAD_BCRESNET: {
            s.add("model.init_conv.0.weight", {32, 1, 3, 3}); s.bn("model.init_conv.1", 32);
            const int ch[4] = {32, 64, 128, 256};
            for (int i = 1; i <= 3; ++i) {
                const std::string p = "model.block" + std::to_string(i);
                s.add(p + ".depthwise.weight", {ch[i - 1], 1, 3, 3});
                s.add(p + ".pointwise.weight", {ch[i], ch[i - 1], 1, 1}); s.bn(p + ".bn1", ch[i]);
                s.add(p + ".shortcut.0.weight", {ch[i], ch[i - 1], 1, 1}); s.bn(p + ".shortcut.1", ch[i]);
            }
            s.lin("model.fc", E, 256);
            break;
        }
        case NWW_HEAD_CONFORMER: {
            const int D = c.conformer_d_model;
            s.lin("model.input_proj", D, F);
            for (int i = 0; i < nb; ++i) {
                const std::string p = "model.conformer_blocks." + std::to_string(i);
                for (const char* ff : {".ff1", ".ff2"}) {
                    s.ln(p + ff + ".layer_norm", D); s.lin(p + ff + ".linear1", 4 * D, D); s.lin(p + ff + ".linear2", D, 4 * D);
                }
                s.add(p + ".attention.in_proj_weight", {3 * D, D}); s.add(p + ".attention.in_proj_bias", {3 * D});
                s.lin(p + ".attention.out_proj", D, D);
                s.ln(p + ".conv_module.layer_norm", D);
                s.add(p + ".conv_module.conv1.weight", {2 * D, D, 1}); s.add(p + ".conv_module.conv1.bias", {2 * D});
                s.add(p + ".conv_module.depthwise_conv.weight", {D, 1, 31}); s.add(p + ".conv_module.depthwise_conv.bias", {D});
                s.bn(p + ".conv_module.batch_norm", D);
                s.add(p + ".conv_module.conv2.weight", {D, D, 1}); s.add(p + ".conv_module.conv2.bias", {D});
                s.ln(p + ".layer_norm", D);
            }
            s.lin("model.output_proj", E, D);
            break;
        }
        case NWW_HEAD_TRANSFORMER: {              // TransformerModel (architectures.py:164-206); d_model / n_head in the conformer_* slots
            const int D = c.conformer_d_model;
            s.lin("model.input_proj", D, F);
            s.add("model.pos_encoder.pe", {NWW_PE_MAX_LEN, 1, D});
            for (int i = 0; i < nb; ++i) {
                const std::string p = "model.transformer_encoder.layers." + std::to_string(i);
                s.add(p + ".self_attn.in_proj_weight", {3 * D, D}); s.add(p + ".self_attn.in_proj_bias", {3 * D});
                s.lin(p + ".self_attn.out_proj", D, D);
                s.lin(p + ".linear1", 4 * D, D); s.lin(p + ".linear2", D, 4 * D);
                s.ln(p + ".norm1", D); s.ln(p + ".norm2", D);
            }
            s.lin("model.output_proj", E, D);
            break;
        }
        case NWW_HEAD_E_BRANCHFORMER: {           // EBranchformerModel (architectures.py:546-616); d_model / n_head in the conformer_* slots
            const int D = c.conformer_d_model;
            s.lin("model.input_proj", D, F);
            for (int i = 0; i < nb; ++i) {
                const std::string p = "model.branchformer_blocks." + std::to_string(i);
                s.ln(p + ".attn_branch_norm", D);
                s.add(p + ".attention.in_proj_weight", {3 * D, D}); s.add(p + ".attention.in_proj_bias", {3 * D});
                s.lin(p + ".attention.out_proj", D, D);
                s.ln(p + ".conv_branch.layer_norm", D);
                s.add(p + ".conv_branch.conv1.weight", {2 * D, D, 1}); s.add(p + ".conv_branch.conv1.bias", {2 * D});
                s.add(p + ".conv_branch.depthwise_conv.weight", {D, 1, 31}); s.add(p + ".conv_branch.depthwise_conv.bias", {D});
                s.bn(p + ".conv_branch.batch_norm", D);
                s.add(p + ".conv_branch.conv2.weight", {D, D, 1}); s.add(p + ".conv_branch.conv2.bias", {D});
                s.lin(p + ".merger.gate", D, D);
                s.ln(p + ".final_norm", D);
                s.ln(p + ".ffn.layer_norm", D); s.lin(p + ".ffn.linear1", 4 * D, D); s.lin(p + ".ffn.linear2", D, 4 * D);
            }
            s.lin("model.output_proj", E, D);
            break;
        }
        case NWW_HEAD_TCN: {                      // TCNModel (architectures.py:290-367); tcn_channels in crnn_channels, tcn_kernel_size in layer_dim
            const int k = c.layer_dim;
            int cin = F;
            for (int i = 0; i < c.n_crnn_channels; ++i) {
                const int co = c.crnn_channels[i];
                const std::string p = "model.tcn_blocks." + std::to_string(i);
                s.add(p + ".conv1.weight", {co, cin, k}); s.add(p + ".conv1.bias", {co});
                s.add(p + ".conv2.weight", {co, co, k}); s.add(p + ".conv2.bias", {co});
                if (cin != co) { s.add(p + ".downsample.weight", {co, cin, 1}); s.add(p + ".downsample.bias", {co}); }
                cin = co;
            }
            s.lin("model.fc", E, cin);
            break;
        }
        case NWW_HEAD_E2E_QUARTZNET:              // E2ERawQuartzNet (architectures.py:798-817): the frontend, then the QuartzNet under model.backbone
            raw_frontend();
            [[fallthrough]];
        case NWW_HEAD_QUARTZNET: {                // QuartzNetModel (architectures.py:370-437); the entries as include/nww.h packs them
            const auto blocks = nww_quartznet_blocks(c);
            const std::string qp = nww_quartznet_prefix(c);
            for (size_t i = 0; i < blocks.size(); ++i) {
                const QnBlock& q = blocks[i];
                const std::string p = qp + "quartznet_blocks." + std::to_string(i);
                s.add(p + ".depthwise_conv.weight", {q.cin, 1, q.k}); s.add(p + ".depthwise_conv.bias", {q.cin});
                s.add(p + ".pointwise_conv.weight", {q.cout, q.cin, 1}); s.add(p + ".pointwise_conv.bias", {q.cout});
                s.bn(p + ".batch_norm", q.cout);
                if (q.cin != q.cout) {
                    s.add(p + ".residual_connector.0.weight", {q.cout, q.cin, 1}); s.add(p + ".residual_connector.0.bias", {q.cout});
                    s.bn(p + ".residual_connector.1", q.cout);
                }
            }
            s.lin(qp + "fc", E, blocks.back().cout);
            break;
        }
        case NWW_HEAD_E2E_CNN: {                  // E2ERawCNN (architectures.py:779-795): the frontend, then RawAudioBackbone's Conv2d (no bias) +
            raw_frontend();                       // BatchNorm2d stages and its Linear
            const RawCnnLayer* ly = nww_raw_cnn_layers();
            for (int i = 0; i < 4; ++i) {
                const std::string p = "model.backbone.conv" + std::to_string(i + 1);
                s.add(p + ".0.weight", {ly[i].cout, ly[i].cin, 3, 3}); s.bn(p + ".1", ly[i].cout);
            }
            s.lin("model.backbone.fc", E, 96);
            break;
        }
        case NWW_HEAD_E2E_DNN: {
            int cin = 1;
            const int ch[3] = {16, 32, 64};
            for (int i = 0; i < 3; ++i) {
                const std::string p = "model.conv_block." + std::to_string(4 * i);
                s.add(p + ".weight", {ch[i], cin, 3, 3}); s.add(p + ".bias", {ch[i]});
                s.bn("model.conv_block." + std::to_string(4 * i + 1), ch[i]);
                cin = ch[i];
            }
            s.lin("model.fc1", 128, 256); s.bn("model.bn1", 128); s.lin("model.out", E, 128);
            break;
        }
    }
    s.lin("classifier.0", E / 2, E);
    s.lin("classifier.3", 1, E / 2);
}

// ------------------------------------------------------------------------------------------ weights and frontend tables
// channel gains balanced at load time (balance_channels, plan_host.h), before the BatchNorms are folded: the conv trunks of the ReLU heads, and
// BcResNet's blocks
void balance_channel_gains(nww_handle* h) {
    const nww_config& c = h->cfg;
    if (!(h->f16 && h->conv_products == 6)) return;
    if (c.head_type != NWW_HEAD_BCRESNET && c.activation != ACT_RELU) return;
    auto T = [&](const std::string& k) -> HostTensor* { auto it = h->tensors.find(k); return it == h->tensors.end() || !it->second.loaded ? nullptr : &it->second; };
    auto layer = [&](const std::string& conv, const std::string& bn) {
        BalanceLayer L; L.w = T(conv + ".weight"); L.b = T(conv + ".bias");
        if (!bn.empty()) { L.g = T(bn + ".weight"); L.beta = T(bn + ".bias"); L.mean = T(bn + ".running_mean"); L.var = T(bn + ".running_var"); }
        return L;
    };
    if (c.head_type == NWW_HEAD_BCRESNET) {
        // the operands of a block's two products are scaled per PIXEL ROW in the kernel (dual_x3, bc_chain) and their weights per tensor, so a
        // channel 2^g off its neighbours costs them (and the weight columns that compensate it) g bits all the same.  Balanced here:
        //   depthwise[c] against pointwise[:, c] of the same block - nothing nonlinear between them, so under every activation;
        //   under ReLU, the init conv's BatchNorm, and each block's TWO BatchNorms as one channel (bn1 + shortcut.1: the sum of the bounds,
        //   the same 2^e), against the next block's pointwise and shortcut.0 columns - the last block's against fc.weight
        const bool relu = c.activation == ACT_RELU;
        auto usable = [](const BalanceLayer& L, size_t C) {
            return L.w && !L.w->shape.empty() && (size_t)L.w->shape[0] == C && C > 0 && L.w->data.size() % C == 0 &&
                   (!L.g || (L.beta && L.mean && L.var && L.g->data.size() == C && L.beta->data.size() == C && L.mean->data.size() == C && L.var->data.size() == C));
        };
        auto reads = [](HostTensor* W, size_t C) { return W && !W->shape.empty() && W->shape[0] > 0 && (W->data.size() / (size_t)W->shape[0]) % C == 0 && W->data.size() % (size_t)W->shape[0] == 0; };
        const size_t ch[4] = {32, 64, 128, 256};
        double bound_h = NWW_F16_FEATURE_BOUND;
        for (int i = 0; i <= 3; ++i) {
            const std::string q = "model.block" + std::to_string(i), qn = "model.block" + std::to_string(i + 1);
            if (relu) {                                   // the channels of h_i: the init conv (i = 0) or block i
                std::vector<BalanceLayer> prod;
                std::vector<double> in;
                if (i == 0) { prod = {layer("model.init_conv.0", "model.init_conv.1")}; in = {bound_h}; }
                else { prod = {layer(q + ".pointwise", q + ".bn1"), layer(q + ".shortcut.0", q + ".shortcut.1")}; in = {0.0, bound_h}; }
                std::vector<HostTensor*> cons;
                if (i < 3) cons = {T(qn + ".pointwise.weight"), T(qn + ".shortcut.0.weight")};
                else cons = {T("model.fc.weight")};
                for (const BalanceLayer& L : prod) if (!usable(L, ch[i]) || !L.g) return;
                for (HostTensor* W : cons) if (!reads(W, ch[i])) return;
                if (i > 0) {                              // d_i's bound: the depthwise rows as balanced in the pass before, on h_(i-1)'s bound
                    const HostTensor* dw = T(q + ".depthwise.weight");
                    double worst = 0.0;
                    for (size_t cc = 0; cc < ch[i - 1]; ++cc) { double l1 = 0.0; for (int k = 0; k < 9; ++k) l1 += std::fabs((double)dw->data[cc * 9 + k]); worst = std::fmax(worst, l1); }
                    in[0] = worst * bound_h;
                }
                bound_h = balance_channels(prod, in, cons);
            }
            if (i < 3) {
                BalanceLayer dw; dw.w = T(qn + ".depthwise.weight");
                HostTensor* pw = T(qn + ".pointwise.weight");
                if (!usable(dw, ch[i]) || dw.w->data.size() != ch[i] * 9 || !reads(pw, ch[i])) return;
                (void)balance_channels(dw, {pw}, 1.0);
            }
        }
        return;
    }
    std::vector<std::pair<BalanceLayer, HostTensor*>> links;      // a layer and the weight that reads its channels
    if (c.head_type == NWW_HEAD_CNN) {
        links = {{layer("model.conv1", ""), T("model.conv2.weight")}, {layer("model.conv2", ""), T("model.fc1.weight")}};
    } else if (c.head_type == NWW_HEAD_CRNN && c.n_crnn_channels >= 3 && c.crnn_channels[0] == 16 && c.crnn_channels[1] == 32) {
        links = {{layer("model.cnn.0", "model.cnn.1"), T("model.cnn.4.weight")}, {layer("model.cnn.4", "model.cnn.5"), T("model.cnn.8.weight")}};
    } else if (c.head_type == NWW_HEAD_E2E_DNN) {
        links = {{layer("model.conv_block.0", "model.conv_block.1"), T("model.conv_block.4.weight")},
                 {layer("model.conv_block.4", "model.conv_block.5"), T("model.conv_block.8.weight")}};
    }
    double bound = NWW_F16_FEATURE_BOUND;
    for (auto& lk : links) {
        const BalanceLayer& L = lk.first;
        if (!L.w || !lk.second || L.w->shape.empty() || (L.g && !(L.beta && L.mean && L.var))) return;
        const size_t Cout = (size_t)L.w->shape[0], N = (size_t)lk.second->shape[0];
        if (Cout == 0 || N == 0 || L.w->data.size() % Cout || (lk.second->data.size() / N) % Cout) return;
        bound = balance_channels(L, {lk.second}, bound);
    }
}

// every BatchNorm folded (eval): alpha = w/sqrt(var+eps), beta = b - mean*alpha (PyTorch CPU kernel form)
void fold_batchnorms(nww_handle* h) {
    std::vector<std::string> bn_prefixes;
    for (const auto& k : h->keys) {
        const std::string sfx = ".running_var";
        if (k.size() > sfx.size() && k.compare(k.size() - sfx.size(), sfx.size(), sfx) == 0)
            bn_prefixes.push_back(k.substr(0, k.size() - sfx.size()));
    }
    for (const auto& p : bn_prefixes) {
        const HostTensor &w = h->tensors[p + ".weight"], &b = h->tensors[p + ".bias"], &m = h->tensors[p + ".running_mean"],
                         &v = h->tensors[p + ".running_var"];
        HostTensor al, be;
        al.shape = be.shape = w.shape;
        al.data.resize(w.data.size()); be.data.resize(w.data.size());
        for (size_t i = 0; i < w.data.size(); ++i) {
            const float invstd = 1.0f / std::sqrt(v.data[i] + 1e-5f);
            al.data[i] = w.data[i] * invstd;
            be.data[i] = b.data[i] - m.data[i] * al.data[i];
        }
        al.loaded = be.loaded = true;
        h->tensors[p + ".alpha"] = al;
        h->tensors[p + ".beta"] = be;
    }
}

// BcResNet: depthwise 3x3 weights tap-major [9][C] for the channels-last kernels
void transpose_depthwise(nww_handle* h) {
    for (int i = 1; i <= 3; ++i) {
        const std::string k = "model.block" + std::to_string(i) + ".depthwise.weight";
        const HostTensor& w = h->tensors[k];
        const int C = (int)w.shape[0];
        HostTensor wt;
        wt.shape = {9, C};
        wt.data.resize((size_t)9 * C);
        for (int ch = 0; ch < C; ++ch)
            for (int tap = 0; tap < 9; ++tap) wt.data[(size_t)tap * C + ch] = w.data[(size_t)ch * 9 + tap];
        wt.loaded = true;
        h->tensors[k + "_t"] = wt;
    }
}

// E2E head on the transposed plane: the three 3x3 filters with their taps transposed, out[f][kx][ky] = w[f][ky][kx] (a convolution of
// the transposed plane with these gives the transposed result of the original convolution)
void transpose_e2e_filters(nww_handle* h) {
    for (int i = 0; i < 3; ++i) {
        const std::string k = "model.conv_block." + std::to_string(4 * i) + ".weight";
        const HostTensor& w = h->tensors[k];
        HostTensor wt;
        wt.shape = w.shape;
        wt.data.resize(w.data.size());
        for (size_t f = 0; f + 9 <= w.data.size(); f += 9)
            for (int ky = 0; ky < 3; ++ky)
                for (int kx = 0; kx < 3; ++kx) wt.data[f + kx * 3 + ky] = w.data[f + ky * 3 + kx];
        wt.loaded = true;
        h->tensors[k + "_t"] = wt;
    }
}

// QuartzNet: everything a block's launches read, folded ONCE in float64 (derived tensors "<block>.qn.*"):
//   pw [Cout][Cin] = alpha pointwise, res [Cout][Cin] = alpha_r projection, bias [Cout] = alpha (W_pw b_dw + b_pw) + beta (+ alpha_r b_res + beta_r),
//   dw_t [k][Cp] the depthwise taps tap-major, zeros past Cin (Cp = Cin up to 32), amax [1] = max_c sum_j |tap|, and where qn_x3 has the
//   widths wcat [Cout][qn_x3_ktot]: pw and res side by side in the fused kernel's chunk order (qn_x3_col)
void fold_quartznet(nww_handle* h) {
    const auto blocks = nww_quartznet_blocks(h->cfg);
    for (size_t i = 0; i < blocks.size(); ++i) {
        const int Cin = blocks[i].cin, Cout = blocks[i].cout, k = blocks[i].k, Cp = qn_x3_cp(Cin);
        const bool proj = Cin != Cout;
        const std::string p = nww_quartznet_prefix(h->cfg) + "quartznet_blocks." + std::to_string(i);
        auto D = [&](const std::string& key) -> const std::vector<float>& { return h->tensors[p + key].data; };
        auto fold = [&](const std::string& bn, std::vector<double>& al, std::vector<double>& be) {
            const auto &w = D(bn + ".weight"), &b = D(bn + ".bias"), &mu = D(bn + ".running_mean"), &var = D(bn + ".running_var");
            al.resize(Cout); be.resize(Cout);
            for (int c = 0; c < Cout; ++c) { al[c] = (double)w[c] / std::sqrt((double)var[c] + 1e-5); be[c] = (double)b[c] - (double)mu[c] * al[c]; }
        };
        const auto &dw = D(".depthwise_conv.weight"), &bdw = D(".depthwise_conv.bias"), &pw = D(".pointwise_conv.weight"), &bpw = D(".pointwise_conv.bias");
        std::vector<double> al, be, alr, ber;
        fold(".batch_norm", al, be);
        if (proj) fold(".residual_connector.1", alr, ber);
        HostTensor tpw, tres, tb, tdw, tam, tcat;
        tpw.shape = {Cout, Cin}; tpw.data.resize((size_t)Cout * Cin);
        tb.shape = {Cout}; tb.data.resize(Cout);
        if (proj) { tres.shape = {Cout, Cin}; tres.data.resize((size_t)Cout * Cin); }
        const bool cat = Cout % 32 == 0 && Cin <= QN_MAX_C && Cout <= QN_MAX_C;
        const int Ktot = qn_x3_ktot(Cin, proj);
        if (cat) { tcat.shape = {Cout, Ktot}; tcat.data.assign((size_t)Cout * Ktot, 0.0f); }
        for (int co = 0; co < Cout; ++co) {
            double bias = (double)bpw[co];
            for (int ci = 0; ci < Cin; ++ci) {
                const double w = (double)pw[(size_t)co * Cin + ci];
                bias += w * (double)bdw[ci];
                tpw.data[(size_t)co * Cin + ci] = (float)(al[co] * w);
                if (cat) tcat.data[(size_t)co * Ktot + qn_x3_col(Cin, proj, 0, ci)] = tpw.data[(size_t)co * Cin + ci];
            }
            bias = al[co] * bias + be[co];
            if (proj) {
                const auto &rw = D(".residual_connector.0.weight"), &rb = D(".residual_connector.0.bias");
                for (int ci = 0; ci < Cin; ++ci) {
                    tres.data[(size_t)co * Cin + ci] = (float)(alr[co] * (double)rw[(size_t)co * Cin + ci]);
                    if (cat) tcat.data[(size_t)co * Ktot + qn_x3_col(Cin, proj, 1, ci)] = tres.data[(size_t)co * Cin + ci];
                }
                bias += alr[co] * (double)rb[co] + ber[co];
            }
            tb.data[co] = (float)bias;
        }
        tdw.shape = {k, Cp}; tdw.data.assign((size_t)k * Cp, 0.0f);
        double amax = 0.0;
        for (int ci = 0; ci < Cin; ++ci) {
            double sum = 0.0;
            for (int j = 0; j < k; ++j) { tdw.data[(size_t)j * Cp + ci] = dw[(size_t)ci * k + j]; sum += std::fabs((double)dw[(size_t)ci * k + j]); }
            amax = std::fmax(amax, sum);
        }
        tam.shape = {1}; tam.data = {(float)(amax * (1.0 + 1e-6))};        // rounded up: it is a bound
        for (auto* t : {&tpw, &tres, &tb, &tdw, &tam, &tcat}) t->loaded = !t->data.empty();
        h->tensors[p + ".qn.pw"] = tpw; h->tensors[p + ".qn.bias"] = tb; h->tensors[p + ".qn.dw_t"] = tdw; h->tensors[p + ".qn.amax"] = tam;
        if (proj) h->tensors[p + ".qn.res"] = tres;
        if (cat) h->tensors[p + ".qn.wcat"] = tcat;
    }
}

// The raw-PCM frontend: each stage's BatchNorm folded into its conv ONCE in float64 (derived tensors "<conv>.raw.*"):
//   w [k][Cin][Cout] = alpha weight, tap-major so that the lanes of conv1d_strided read consecutive floats; b [Cout] = beta (the convs
//   have no bias of their own)
void fold_raw_frontend(nww_handle* h) {
    const nww_config& c = h->cfg;
    for (int i = 0, Cin = 1; i < c.n_blocks; ++i) {
        const int Cout = c.layer_dim << i, k = i == 0 ? 41 : 13;
        const std::string conv = "model.frontend.conv_blocks." + std::to_string(3 * i), bn = "model.frontend.conv_blocks." + std::to_string(3 * i + 1);
        const auto &w = h->tensors[conv + ".weight"].data, &g = h->tensors[bn + ".weight"].data, &b = h->tensors[bn + ".bias"].data,
                   &mu = h->tensors[bn + ".running_mean"].data, &var = h->tensors[bn + ".running_var"].data;
        HostTensor tw, tb;
        tw.shape = {k, Cin, Cout}; tw.data.resize((size_t)k * Cin * Cout);
        tb.shape = {Cout}; tb.data.resize(Cout);
        for (int co = 0; co < Cout; ++co) {
            const double al = (double)g[co] / std::sqrt((double)var[co] + 1e-5);
            tb.data[co] = (float)((double)b[co] - (double)mu[co] * al);
            for (int ci = 0; ci < Cin; ++ci)
                for (int j = 0; j < k; ++j) tw.data[((size_t)j * Cin + ci) * Cout + co] = (float)(al * (double)w[((size_t)co * Cin + ci) * k + j]);
        }
        tw.loaded = tb.loaded = true;
        h->tensors[conv + ".raw.w"] = tw; h->tensors[conv + ".raw.b"] = tb;
        if (i > 0 && Cout % 32 == 0 && Cin % 16 == 0) {      // raw_x3's operand: the same folded weights as [Cout][k Cin], tap-major columns
            HostTensor tk;
            tk.shape = {Cout, k * Cin}; tk.data.resize((size_t)Cout * k * Cin);
            for (int co = 0; co < Cout; ++co)
                for (int j = 0; j < k; ++j)
                    for (int ci = 0; ci < Cin; ++ci) tk.data[((size_t)co * k + j) * Cin + ci] = tw.data[((size_t)j * Cin + ci) * Cout + co];
            tk.loaded = true;
            h->tensors[conv + ".raw.wk"] = tk;
        }
        Cin = Cout;
    }
}

// RawAudioBackbone: each stage's BatchNorm2d folded into its conv ONCE in float64, and the 3x3 taps transposed to the channels-last plane
// the frontend writes ([A = image W][Bd = image H][C]: the A tap is the weight's kw, the Bd tap its kh).  Derived tensors "<conv>.c2.*":
//   w [3 (A)][3 (Bd)][Cin][Cout] = alpha weight, tap-major for conv2d_strided; b [Cout] = beta (the convs have no bias of their own);
//   where conv2s_x3 has the shape, its operand: wk [CoutP][9 Cp] the same weights as rows with tap-major columns (Cin padded to Cp, Cout to
//   CoutP with zeros), every row times its own power of two - the row's largest magnitude lands in [2^14, 2^15), a zero row takes 1 - and
//   un [CoutP] the reciprocals.  A row whose scale cannot be formed (a value that is not finite, a power of two outside float32) leaves
//   wk out, and the planner takes conv2d_strided
void fold_raw_backbone(nww_handle* h) {
    const RawCnnLayer* ly = nww_raw_cnn_layers();
    for (int i = 0; i < 4; ++i) {
        const int Cin = ly[i].cin, Cout = ly[i].cout;
        const std::string conv = "model.backbone.conv" + std::to_string(i + 1) + ".0", bn = "model.backbone.conv" + std::to_string(i + 1) + ".1";
        const auto &w = h->tensors[conv + ".weight"].data, &g = h->tensors[bn + ".weight"].data, &b = h->tensors[bn + ".bias"].data,
                   &mu = h->tensors[bn + ".running_mean"].data, &var = h->tensors[bn + ".running_var"].data;
        HostTensor tw, tb;
        tw.shape = {3, 3, Cin, Cout}; tw.data.resize((size_t)9 * Cin * Cout);
        tb.shape = {Cout}; tb.data.resize(Cout);
        for (int co = 0; co < Cout; ++co) {
            const double al = (double)g[co] / std::sqrt((double)var[co] + 1e-5);
            tb.data[co] = (float)((double)b[co] - (double)mu[co] * al);
            for (int ci = 0; ci < Cin; ++ci)
                for (int kh = 0; kh < 3; ++kh)
                    for (int kw = 0; kw < 3; ++kw)
                        tw.data[((size_t)(kw * 3 + kh) * Cin + ci) * Cout + co] = (float)(al * (double)w[(((size_t)co * Cin + ci) * 3 + kh) * 3 + kw]);
        }
        tw.loaded = tb.loaded = true;
        h->tensors[conv + ".c2.w"] = tw; h->tensors[conv + ".c2.b"] = tb;
        if (!conv2s_x3_supported(Cin, Cout, ly[i].sA, ly[i].sB)) continue;
        const int Cp = conv2s_x3_cp(Cin), CoutP = conv2s_x3_coutp(Cout), K = 9 * Cp;
        HostTensor tk, tu;
        tk.shape = {CoutP, K}; tk.data.assign((size_t)CoutP * K, 0.0f);
        tu.shape = {CoutP}; tu.data.assign(CoutP, 1.0f);
        bool ok = true;
        for (int co = 0; co < Cout && ok; ++co) {
            float m = 0.0f;
            for (int q = 0; q < 9 * Cin; ++q) { const float v = std::fabs(tw.data[(size_t)q * Cout + co]); if (!(v <= m)) m = v; }   // a NaN sticks
            if (!std::isfinite(m) || !std::isfinite(tb.data[co])) { ok = false; break; }
            int e = 0;
            if (m > 0.0f) e = 14 - std::ilogb(m);
            if (e > 120 || e < -120) { ok = false; break; }
            const float ws = std::ldexp(1.0f, e);
            tu.data[co] = std::ldexp(1.0f, -e);
            for (int t = 0; t < 9; ++t)
                for (int ci = 0; ci < Cin; ++ci) tk.data[(size_t)co * K + t * Cp + ci] = tw.data[((size_t)t * Cin + ci) * Cout + co] * ws;
        }
        if (!ok) continue;
        tk.loaded = tu.loaded = true;
        h->tensors[conv + ".c2.wk"] = tk; h->tensors[conv + ".c2.un"] = tu;
    }
}

// every loaded tensor but the frontend's in one device arena, each 16-byte aligned: assembled in its host image (nww_handle::h_weights,
// which the planner reads the weights' values from and nww_finalize releases) and uploaded in one copy
int upload_weight_arena(nww_handle* h) {
    size_t total = 0;
    for (auto& kv : h->tensors) {
        if (!kv.second.loaded || kv.first.rfind("frontend.", 0) == 0) continue;
        kv.second.dev_off = total;
        total += (kv.second.data.size() + 3) & ~(size_t)3;
    }
    h->h_weights.clear();
    h->h_weights.reserve(total + 4);
    for (const auto& kv : h->tensors) {                              // in offset order: each tensor, then zeros up to the next one
        if (!kv.second.loaded || kv.first.rfind("frontend.", 0) == 0) continue;
        h->h_weights.resize(kv.second.dev_off, 0.0f);
        h->h_weights.insert(h->h_weights.end(), kv.second.data.begin(), kv.second.data.end());
    }
    h->h_weights.resize(total + 4, 0.0f);
    HIP_TRY(h, hipMalloc(&h->d_weights, h->h_weights.size() * sizeof(float)));
    HIP_TRY(h, hipMemcpy(h->d_weights, h->h_weights.data(), h->h_weights.size() * sizeof(float), hipMemcpyHostToDevice));
    return NWW_OK;
}

int build_frontend_tables(nww_handle* h) {
    std::vector<float> win, fb;
    auto wi = h->tensors.find("frontend.window");
    if (wi != h->tensors.end() && wi->second.loaded) win = wi->second.data; else fe_default_window(h->fe.win_length, win);
    auto fi = h->tensors.find("frontend.mel_fb");
    if (fi != h->tensors.end() && fi->second.loaded) fb = fi->second.data; else fe_default_melfb(h->fe, fb);
    h->fe_window = win; h->fe_mel_fb = fb;
    FeTables tb;
    const std::string e = fe_build_tables(h->fe, win.data(), fb.data(), &tb);
    if (!e.empty()) return fail(h, NWW_ERR_INVALID, "frontend tables: %s", e.c_str());
    const size_t tbytes = (sizeof(FeTables) + 15) & ~(size_t)15;
    HIP_TRY(h, hipMalloc(&h->d_tables, tbytes));
    HIP_TRY(h, hipMemset(h->d_tables, 0, tbytes));
    HIP_TRY(h, hipMemcpy(h->d_tables, &tb, sizeof(FeTables), hipMemcpyHostToDevice));
    h->mel_max_taps = 0;
    for (int j = 0; j < h->fe.n_mels; ++j) h->mel_max_taps = tb.mel_cnt[j] > h->mel_max_taps ? tb.mel_cnt[j] : h->mel_max_taps;
    std::vector<Fe2MelPlan> plan(1);
    const std::string e2 = fe2_build_mel_plan(h->fe, fb.data(), plan.data());
    if (!e2.empty()) return fail(h, NWW_ERR_INVALID, "frontend mel plan: %s", e2.c_str());
    HIP_TRY(h, hipMalloc(&h->d_melplan, sizeof(Fe2MelPlan)));
    HIP_TRY(h, hipMemcpy(h->d_melplan, plan.data(), sizeof(Fe2MelPlan), hipMemcpyHostToDevice));
    // (the DFT on the matrix pipe - frontend3 - was built in round 5, parity-green and slower: tools/ubench/fe3/)
    return NWW_OK;
}
