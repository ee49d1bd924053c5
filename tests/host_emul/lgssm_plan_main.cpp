// Host driver of csrc/lgssm_plan.hpp for tests/test_lgssm_plan_cpu.py.
//   stdin, one engine per line:  d dy T n_chains n_models segments dense allow_missing step_model chain_model [RXHIP_NAME=value ...]
//   stdout: "key <field> <1 if changing that field alone changes the engine-pool key>" for every hook field, then "plan <S> <L> <Llast> <pack> <fused> <rev_cand>" per line
#include <cstdio>
#include <iostream>
#include <map>
#include <sstream>
#include <string>

#include "lgssm_plan.hpp"

using namespace rxhip::plan;

static void change(bool& v) { v = !v; }
static void change(int& v) { v += 1; }
static void change(unsigned long long& v) { v -= 1; }
static void change(Text& v) { v.s[0] = 'x'; }

int main() {
#define X(type, field, dflt)                                   \
    {                                                          \
        ScheduleHooks a, b;                                    \
        change(b.field);                                       \
        std::string ka, kb;                                    \
        a.append_key(ka);                                      \
        b.append_key(kb);                                      \
        std::printf("key %s %d\n", #field, ka != kb ? 1 : 0);  \
    }
    RXHIP_SCHEDULE_HOOKS(X)
#undef X
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        Shape s;
        int dense, missing, stepm, chainm;
        if (!(in >> s.d >> s.dy >> s.T >> s.n_chains >> s.n_models >> s.segments >> dense >> missing >> stepm >> chainm)) continue;
        s.dense = dense != 0; s.allow_missing = missing != 0; s.step_model = stepm != 0; s.chain_model = chainm != 0;
        std::map<std::string, std::string> env;
        for (std::string kv; in >> kv;) env[kv.substr(0, kv.find('='))] = kv.substr(kv.find('=') + 1);
        const ScheduleHooks h = ScheduleHooks::read([&](const char* n) { auto it = env.find(n); return it == env.end() ? nullptr : it->second.c_str(); });
        const Flags f = static_flags(s, h);
        const Segmentation g = segmentation(s, f, h);
        const bool fused = want_fused(f.uniform, g.S, s.n_chains, s.T, h);
        std::printf("plan %d %lld %lld %d %d %d\n", g.S, g.L, g.Llast, f.pack, fused ? 1 : 0, rev_cand(fused, s.n_chains, s.d, s.dy, s.T, h) ? 1 : 0);
    }
    return 0;
}
