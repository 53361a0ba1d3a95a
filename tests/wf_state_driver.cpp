// wf_state_driver.cpp — csrc/wfmt.h's wf_decide() without a device, for tests/test_wf_state_host.py (built there with the address
// and undefined-behaviour sanitizers).  One input line per model:
//     f32 tp moe H F finalized w2d_uploaded expert_uploaded  n  {target family value group} x n
// names the facts and the n calls to draw from.  Every sequence of one, two and three of those calls is played from the
// untouched state; the answer is one line per model, five characters per call in the order
//     for a: emit(a);  for b: emit(a b);  for c: emit(a b c)
// namely the code (0: NVL_OK, I: NVL_ERR_INVALID, S: NVL_ERR_STATE) and the state after the call (wf ef hf as b / 8 / m /
// 3, 6, 1 for INT4 of group 32, 64, 128; a8 as 0 / 1).  A refusal without a message, or one that moves the state, is an X.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../nano-vllm-go_amd/csrc/wfmt.h"

using namespace nvl;

static char fmt_char(int wf) {
    switch (wf_base(wf)) {
        case WF_BF16: return 'b';
        case WF_FP8: return '8';
        case WF_MXFP4: return 'm';
        default: return wf_group(wf) == 32 ? '3' : (wf_group(wf) == 64 ? '6' : (wf_group(wf) == 128 ? '1' : '?'));
    }
}

static WfState play(const WfState& s, const WfFacts& f, const WfRequest& r, std::string& out) {
    const WfDecision d = wf_decide(s, f, r);
    char code = d.code == NVL_OK ? '0' : (d.code == NVL_ERR_INVALID ? 'I' : (d.code == NVL_ERR_STATE ? 'S' : '?'));
    const bool same = d.state.wf == s.wf && d.state.ef == s.ef && d.state.hf == s.hf && d.state.a8 == s.a8;
    const size_t nfn = strlen(r.fn);     // a refusal's message: "<entry point>: <why>"
    if (d.code != NVL_OK && (!same || strlen(d.msg) <= nfn + 2 || strncmp(d.msg, r.fn, nfn) != 0 || strncmp(d.msg + nfn, ": ", 2) != 0)) code = 'X';
    if (d.code == NVL_OK && d.msg[0]) code = 'X';
    out += code;
    out += fmt_char(d.state.wf);
    out += fmt_char(d.state.ef);
    out += fmt_char(d.state.hf);
    out += d.state.a8 ? '1' : '0';
    return d.state;
}

int main() {
    int b[8], n;
    while (scanf("%d %d %d %d %d %d %d %d %d", &b[0], &b[1], &b[2], &b[3], &b[4], &b[5], &b[6], &b[7], &n) == 9) {
        const WfFacts f{b[0] != 0, b[1] != 0, b[2] != 0, b[3], b[4], b[5] != 0, b[6] != 0, b[7] != 0};
        std::vector<WfRequest> calls((size_t)n);
        for (auto& r : calls) {
            if (scanf("%d %d %d %d", &r.target, &r.family, &r.value, &r.group) != 4) return 2;
            if (r.target < WT_PROJ || r.target > WT_ACT || r.family < WFAM_FP8 || r.family > WFAM_GQ) return 3;
            r.fn = r.target == WT_ACT ? "nvl_set_act_dtype" : wf_family(r.family).setter[r.target];
        }
        std::string out;
        for (const auto& a : calls) {
            const WfState sa = play(WfState{}, f, a, out);
            for (const auto& bb : calls) {
                const WfState sb = play(sa, f, bb, out);
                for (const auto& c : calls) play(sb, f, c, out);
            }
        }
        out += '\n';
        fwrite(out.data(), 1, out.size(), stdout);
    }
    return 0;
}
