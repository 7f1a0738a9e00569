// bank_check.cpp - the rules of csrc/bank.h that make K handles a bank, on plain structs (tests/test_bank_host.py; g++ with
// -fsanitize=address,undefined, no HIP): the frontend comparison - equal configs, every FeParams field perturbed in turn, one table
// entry changed by one ulp, tables of another length, -0.0f against 0.0f and a NaN against itself - and the member validation - a
// duplicate handle, a NULL member, an unfinalized one, another device, a raw-PCM head, a mel-major head, k = 0, k = 1 - with the code,
// the member named in the text and the order in which the rules fire.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "bank.h"

static int g_fail = 0, g_checks = 0;
#define CHECK(cond, ...)                                                        \
    do {                                                                        \
        ++g_checks;                                                             \
        if (!(cond)) {                                                          \
            if (++g_fail <= 20) { std::printf("FAIL %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
        }                                                                       \
    } while (0)

struct Tables { std::vector<float> window, fb; };

static Tables make_tables(const FeParams& p) {
    Tables t;
    fe_default_window(p.win_length, t.window);
    fe_default_melfb(p, t.fb);
    return t;
}

static BankFrontend frontend(const FeParams& p, const Tables& t) {
    BankFrontend f;
    f.fe = p;
    f.window = t.window.data(); f.n_window = t.window.size();
    f.mel_fb = t.fb.data(); f.n_mel_fb = t.fb.size();
    return f;
}

static bool is(const char* got, const char* want) { return want ? (got && !std::strcmp(got, want)) : !got; }

static void frontends() {
    const FeParams base;
    const Tables t = make_tables(base);
    const BankFrontend a = frontend(base, t);
    // equal configs: two copies of the tables at other addresses
    const Tables t2 = make_tables(base);
    CHECK(is(bank_frontend_diff(a, frontend(base, t2)), nullptr), "equal");
    CHECK(t.window.data() != t2.window.data() && t.window.size() == 400 && t.fb.size() == 201 * 64, "tables");
    // every field in turn
    struct Case { const char* name; void (*poke)(FeParams&); };
    const Case cases[] = {
        {"sample_rate", [](FeParams& p) { p.sample_rate = 8000; }}, {"n_fft", [](FeParams& p) { p.n_fft = 512; }},
        {"win_length", [](FeParams& p) { p.win_length = 320; }},    {"hop_length", [](FeParams& p) { p.hop = 128; }},
        {"n_mels", [](FeParams& p) { p.n_mels = 40; }},             {"center", [](FeParams& p) { p.center = 0; }},
        {"f_min", [](FeParams& p) { p.f_min = 20.f; }},             {"f_max", [](FeParams& p) { p.f_max = 7600.f; }},
        {"amin", [](FeParams& p) { p.amin = 1e-9f; }},              {"db_multiplier", [](FeParams& p) { p.db_mult = 20.f; }},
    };
    for (const Case& c : cases) {
        FeParams p = base;
        c.poke(p);
        // (the same tables: only the field differs)
        const char* d = bank_frontend_diff(a, frontend(p, t));
        CHECK(is(d, c.name), "%s reported as %s", c.name, d ? d : "(equal)");
        CHECK(is(bank_frontend_diff(frontend(p, t), a), c.name), "%s, other way round", c.name);
    }
    // two fields: the first in the header's order is named
    { FeParams p = base; p.amin = 1e-9f; p.n_mels = 40; CHECK(is(bank_frontend_diff(a, frontend(p, t)), "n_mels"), "first of two"); }
    // a float field by one ulp, -0.0f against 0.0f, a NaN against itself
    { FeParams p = base; p.f_max = std::nextafterf(p.f_max, 0.f); CHECK(is(bank_frontend_diff(a, frontend(p, t)), "f_max"), "ulp of f_max"); }
    { FeParams p = base; p.f_min = -0.0f; CHECK(is(bank_frontend_diff(a, frontend(p, t)), "f_min"), "-0.0f"); }
    { FeParams p = base; p.amin = NAN; FeParams q = p; CHECK(is(bank_frontend_diff(frontend(p, t), frontend(q, t)), nullptr), "NaN equals itself as bytes"); }
    // one table entry by one ulp, each table, first / middle / last entry
    for (int which = 0; which < 2; ++which) {
        const size_t n = which ? t.fb.size() : t.window.size();
        for (size_t at : {(size_t)0, n / 2 + 3, n - 1}) {
            Tables u = t;
            float& v = (which ? u.fb : u.window)[at];
            v = std::nextafterf(v, 2.0f);
            const char* d = bank_frontend_diff(a, frontend(base, u));
            CHECK(is(d, which ? "frontend.mel_fb" : "frontend.window"), "table %d entry %zu reported as %s", which, at, d ? d : "(equal)");
        }
    }
    // both tables differ: the window is named; another length; no table at all on both sides
    { Tables u = t; u.window[7] += 0.25f; u.fb[9] += 0.25f; CHECK(is(bank_frontend_diff(a, frontend(base, u)), "frontend.window"), "window first"); }
    { Tables u = t; u.fb.pop_back(); CHECK(is(bank_frontend_diff(a, frontend(base, u)), "frontend.mel_fb"), "shorter filterbank"); }
    { BankFrontend e; e.fe = base; BankFrontend f = e; CHECK(is(bank_frontend_diff(e, f), nullptr), "no tables"); CHECK(is(bank_frontend_diff(a, e), "frontend.window"), "tables against none"); }
}

static void members() {
    const FeParams base;
    const Tables t = make_tables(base);
    int dummy[4];                                        // four distinct addresses to stand for handles
    auto bank = [&](int k) {
        std::vector<BankMember> m((size_t)k);
        for (int j = 0; j < k; ++j) { m[(size_t)j].handle = &dummy[j]; m[(size_t)j].finalized = true; m[(size_t)j].frames_major = true; m[(size_t)j].frontend = frontend(base, t); }
        return m;
    };
    std::string text;
    auto names = [&](int j) { return text.find("member " + std::to_string(j)) != std::string::npos; };
    { auto m = bank(4); CHECK(bank_members_check(m.data(), 4, text) == NWW_OK, "four equal members: %s", text.c_str()); }
    { auto m = bank(1); CHECK(bank_members_check(m.data(), 1, text) == NWW_OK, "k = 1"); }
    // k = 0, a negative k, no list
    { auto m = bank(1); CHECK(bank_members_check(m.data(), 0, text) == NWW_ERR_INVALID && text.find("k >= 1") != std::string::npos, "k = 0: %s", text.c_str()); }
    { auto m = bank(1); CHECK(bank_members_check(m.data(), -3, text) == NWW_ERR_INVALID, "k < 0"); }
    CHECK(bank_members_check(nullptr, 2, text) == NWW_ERR_INVALID, "NULL list");
    // a NULL member, wherever it stands
    for (int j = 0; j < 3; ++j) {
        auto m = bank(3);
        m[(size_t)j] = BankMember();
        CHECK(bank_members_check(m.data(), 3, text) == NWW_ERR_INVALID && names(j) && text.find("NULL") != std::string::npos, "NULL member %d: %s", j, text.c_str());
    }
    // duplicate handles
    { auto m = bank(4); m[3].handle = m[1].handle;
      CHECK(bank_members_check(m.data(), 4, text) == NWW_ERR_INVALID && names(3) && names(1) && text.find("distinct") != std::string::npos, "duplicate: %s", text.c_str()); }
    // unfinalized, another device
    { auto m = bank(3); m[2].finalized = false; CHECK(bank_members_check(m.data(), 3, text) == NWW_ERR_INVALID && names(2) && text.find("finalized") != std::string::npos, "unfinalized: %s", text.c_str()); }
    { auto m = bank(1); m[0].finalized = false; CHECK(bank_members_check(m.data(), 1, text) == NWW_ERR_INVALID && names(0), "unfinalized, k = 1"); }
    { auto m = bank(3); m[1].device = 2; CHECK(bank_members_check(m.data(), 3, text) == NWW_ERR_INVALID && names(1) && text.find("device 2") != std::string::npos, "device: %s", text.c_str()); }
    // a raw-PCM head: refused among k > 1 (as the leader too), fine alone
    for (int j = 0; j < 2; ++j) {
        auto m = bank(2);
        m[(size_t)j].raw_head = true;
        CHECK(bank_members_check(m.data(), 2, text) == NWW_ERR_INVALID && names(j) && text.find("raw-PCM") != std::string::npos, "raw head %d: %s", j, text.c_str());
    }
    { auto m = bank(1); m[0].raw_head = true; m[0].frames_major = true; CHECK(bank_members_check(m.data(), 1, text) == NWW_OK, "a raw head alone"); }
    // a frontend that differs: the member and the field
    { auto m = bank(3); m[2].frontend.fe.n_mels = 40;
      CHECK(bank_members_check(m.data(), 3, text) == NWW_ERR_INVALID && names(2) && text.find("n_mels") != std::string::npos, "n_mels: %s", text.c_str()); }
    { Tables u = t; u.fb[1234] = std::nextafterf(u.fb[1234], 2.0f);
      auto m = bank(3); m[1].frontend = frontend(base, u);
      CHECK(bank_members_check(m.data(), 3, text) == NWW_ERR_INVALID && names(1) && text.find("frontend.mel_fb") != std::string::npos, "ulp: %s", text.c_str()); }
    // a mel-major head: UNSUPPORTED among k > 1, fine alone
    { auto m = bank(3); m[1].frames_major = false; CHECK(bank_members_check(m.data(), 3, text) == NWW_ERR_UNSUPPORTED && names(1), "mel-major: %s", text.c_str()); }
    { auto m = bank(1); m[0].frames_major = false; CHECK(bank_members_check(m.data(), 1, text) == NWW_OK, "mel-major alone"); }
    // the order of the rules: a duplicate before a frontend, a frontend before the orientation
    { auto m = bank(3); m[2].handle = m[0].handle; m[1].frontend.fe.hop = 128; CHECK(bank_members_check(m.data(), 3, text) == NWW_ERR_INVALID && text.find("distinct") != std::string::npos, "order 1: %s", text.c_str()); }
    { auto m = bank(3); m[1].frames_major = false; m[2].frontend.fe.hop = 128; CHECK(bank_members_check(m.data(), 3, text) == NWW_ERR_INVALID && text.find("hop_length") != std::string::npos, "order 2: %s", text.c_str()); }
}

int main() {
    frontends();
    members();
    std::printf("checks=%d\n", g_checks);
    if (g_fail) std::printf("FAILED %d checks\n", g_fail);
    else std::printf("ok\n");
    return g_fail ? 1 : 0;
}
