// Stand-alone driver of csrc/spec_loop.h for tests/test_spec_loop_host.py (built there with the address and undefined-
// behaviour sanitizers): plays nvl::SpecLoop against a fake verify step, and runs nvl::lookup_draft.  Reads cases from
// stdin, one per line, and answers each on stdout:
//   C n_seqs n_steps k T rule  cache[n_seqs]  hist_len[n_seqs]  n_acc  acc[n_acc]
//       rule 0: room = T - cache - 1 (the lookup loops); rule 1: room = T - max(cache, history) - 1 (nvl_decode_speculative).
//       The fake verify step takes the next accept count of the list (cyclically) for each active sequence, clamps it to
//       k_pass, returns the synthetic id 1000 * i + step for step `step` of sequence i, and advances the cache by
//       min(acc + 1, keep) as the real pass does.
//     -> per pass "P k_pass na" followed by "i keep pos acc take first_step" per active sequence, then
//        "OUT passes id[n_steps * n_seqs]" (-1 = never written)
//   L k ngram n h[n]
//     -> "D take draft[k]"
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "../nano-vllm-go_amd/csrc/spec_loop.h"

static void loop_case(std::istringstream& in) {
    int n_seqs, n_steps, k, T, rule, n_acc;
    in >> n_seqs >> n_steps >> k >> T >> rule;
    std::vector<int> cache((size_t)n_seqs), hlen((size_t)n_seqs);
    for (int& c : cache) in >> c;
    for (int& h : hlen) in >> h;
    in >> n_acc;
    std::vector<int> accs((size_t)n_acc);
    for (int& a : accs) in >> a;

    nvl::SpecLoop loop(n_seqs, n_steps);
    std::vector<int64_t> seq_ids((size_t)n_seqs);
    for (int i = 0; i < n_seqs; i++) {
        seq_ids[(size_t)i] = 100 + i;
        loop.hist[(size_t)i].assign((size_t)hlen[(size_t)i], 7);      // (the last id is the sequence's first token)
    }
    std::vector<int32_t> out((size_t)n_steps * n_seqs, -1), accepted((size_t)n_seqs, 0);
    size_t next_acc = 0;
    const auto pos = [&](int i) { return rule ? std::max(cache[(size_t)i], (int)loop.hist[(size_t)i].size()) : cache[(size_t)i]; };
    while (loop.plan(k, seq_ids.data(), [&](int i) { return T - pos(i) - 1; })) {
        const int S = loop.S;
        printf("P %d %d", loop.k_pass, loop.na);
        for (int a = 0; a < loop.na; a++) {
            const int i = loop.who[(size_t)a], keep = loop.keep[(size_t)a];
            if (loop.ids[(size_t)a] != 100 + i || loop.toks[(size_t)a * S] != loop.hist[(size_t)i].back()) { printf(" BAD-ROW"); }
            const int acc = std::min(accs[next_acc++ % accs.size()], loop.k_pass);
            loop.acc[(size_t)a] = acc;
            for (int j = 0; j <= acc; j++) loop.got[(size_t)a * S + j] = 1000 * i + loop.done[(size_t)i] + j;
            const int take = std::min(acc + 1, keep);
            printf("  %d %d %d %d %d %d", i, keep, pos(i), acc, take, loop.done[(size_t)i]);
            cache[(size_t)i] += take;
        }
        printf("\n");
        loop.emit(out.data(), accepted.data());
    }
    printf("OUT %d", loop.passes);
    for (int32_t t : out) printf(" %d", t);
    printf("\n");
}

static void lookup_case(std::istringstream& in) {
    int k, ngram, n;
    in >> k >> ngram >> n;
    std::vector<int32_t> h((size_t)n), draft((size_t)k);
    for (int32_t& t : h) in >> t;
    const int take = nvl::lookup_draft(h.data(), n, k, ngram, draft.data());
    printf("D %d", take);
    for (int32_t t : draft) printf(" %d", t);
    printf("\n");
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string kind;
        if (!(in >> kind)) continue;
        if (kind == "C") loop_case(in);
        else if (kind == "L") lookup_case(in);
        else { fprintf(stderr, "unknown case kind %s\n", kind.c_str()); return 2; }
    }
    return 0;
}
