// bank.h - what makes K handles a bank (nww_bank.hip): the rules on the members that need no device, as host-only code (no HIP here:
// tests/hostemu/bank_check.cpp compiles it with g++).  A bank shares ONE frontend pass, so every member's mel frontend must be the
// leader's, bit for bit: the FeParams fields and the window and filterbank tables the frontend was finalized with.  Values are
// compared as bytes - a float that differs by one ulp differs, -0.0f differs from 0.0f and a NaN equals itself.
#pragma once
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <string>
#include "../../include/nww.h"
#include "fe_tables.h"

// a member's frontend: its parameters and the tables it was finalized with (loaded through frontend.window / frontend.mel_fb or built in)
struct BankFrontend {
    FeParams fe;
    const float* window = nullptr; size_t n_window = 0;
    const float* mel_fb = nullptr; size_t n_mel_fb = 0;
};

// the first field in which b differs from a, by its nww_config name (the tables by their tensor keys), or nullptr: identical
inline const char* bank_frontend_diff(const BankFrontend& a, const BankFrontend& b) {
    const FeParams &x = a.fe, &y = b.fe;
    if (x.sample_rate != y.sample_rate) return "sample_rate";
    if (x.n_fft != y.n_fft) return "n_fft";
    if (x.win_length != y.win_length) return "win_length";
    if (x.hop != y.hop) return "hop_length";
    if (x.n_mels != y.n_mels) return "n_mels";
    if (x.center != y.center) return "center";
    if (std::memcmp(&x.f_min, &y.f_min, sizeof(float))) return "f_min";
    if (std::memcmp(&x.f_max, &y.f_max, sizeof(float))) return "f_max";
    if (std::memcmp(&x.amin, &y.amin, sizeof(float))) return "amin";
    if (std::memcmp(&x.db_mult, &y.db_mult, sizeof(float))) return "db_multiplier";
    if (a.n_window != b.n_window || (a.n_window && std::memcmp(a.window, b.window, a.n_window * sizeof(float)))) return "frontend.window";
    if (a.n_mel_fb != b.n_mel_fb || (a.n_mel_fb && std::memcmp(a.mel_fb, b.mel_fb, a.n_mel_fb * sizeof(float)))) return "frontend.mel_fb";
    return nullptr;
}

// what the rules read of a member (filled from its handle by nww_bank.hip; handle == nullptr: a NULL member, nothing else is read)
struct BankMember {
    const void* handle = nullptr;
    bool finalized = false;
    int device = 0;
    bool raw_head = false;         // e2e_quartznet / e2e_cnn: a learned frontend
    bool frames_major = false;     // the head consumes frames-major log-mel: !mel_major_features || e2e_transposed
    BankFrontend frontend;
};

// The rules in the order include/nww.h states them (the window's shape rule is nww_bank.hip's: it needs the frame law of each head).
// Returns NWW_OK or the error code, with the text - which names the offending member by its index - in `text`.  k == 1 needs a
// finalized handle and nothing more: that bank is the plain call on members[0].
inline int bank_members_check(const BankMember* m, int k, std::string& text) {
    char buf[384];
    auto say = [&](int code) { text = buf; return code; };
    if (!m || k < 1) {
        std::snprintf(buf, sizeof(buf), "a bank needs k >= 1 members (got %s, k = %d)", m ? "a list" : "NULL", k);
        return say(NWW_ERR_INVALID);
    }
    for (int j = 0; j < k; ++j) {
        if (!m[j].handle) { std::snprintf(buf, sizeof(buf), "member %d is NULL", j); return say(NWW_ERR_INVALID); }
        if (!m[j].finalized) {
            std::snprintf(buf, sizeof(buf), "member %d: model not finalized: call nww_finalize after loading the state_dict", j);
            return say(NWW_ERR_INVALID);
        }
        for (int i = 0; i < j; ++i)
            if (m[i].handle == m[j].handle) {
                std::snprintf(buf, sizeof(buf), "member %d is the same handle as member %d: a bank needs distinct handles", j, i);
                return say(NWW_ERR_INVALID);
            }
        if (m[j].device != m[0].device) {
            std::snprintf(buf, sizeof(buf), "member %d is on device %d and member 0 on device %d: a bank runs on one", j, m[j].device, m[0].device);
            return say(NWW_ERR_INVALID);
        }
    }
    if (k == 1) return NWW_OK;
    for (int j = 0; j < k; ++j)
        if (m[j].raw_head) {
            std::snprintf(buf, sizeof(buf), "member %d is a raw-PCM head (e2e_quartznet / e2e_cnn): its frontend is learned, a bank has nothing to share with it", j);
            return say(NWW_ERR_INVALID);
        }
    for (int j = 1; j < k; ++j) {
        const char* d = bank_frontend_diff(m[0].frontend, m[j].frontend);
        if (d) {
            std::snprintf(buf, sizeof(buf), "member %d: its frontend differs from member 0's in %s: a bank shares one frontend pass", j, d);
            return say(NWW_ERR_INVALID);
        }
    }
    for (int j = 0; j < k; ++j)
        if (!m[j].frames_major) {
            std::snprintf(buf, sizeof(buf), "member %d reads mel-major log-mel (an e2e_dnn planned in the reference's orientation): a bank's head input is "
                                            "frames-major", j);
            return say(NWW_ERR_UNSUPPORTED);
        }
    return NWW_OK;
}
