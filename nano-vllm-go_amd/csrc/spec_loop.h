// The host arithmetic of the speculative decode loops (nvl_decode_greedy_lookup, nvl_decode_sampled_lookup,
// nvl_decode_speculative) and the prompt-lookup drafter.  Plain C++17, standard headers only, no model and no stream: the
// entry points in nvllm.hip supply the draft step and the verify pass, tests/spec_loop_driver.cpp supplies fakes.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

namespace nvl {

// prompt-lookup drafting (nvl_lookup_draft; the caller has checked history / draft_out != NULL, n >= 1, k >= 1): the
// longest suffix of up to `ngram` ids that occurs earlier in the history, latest occurrence first; the k ids that followed
// it are the draft (the last one repeated when fewer follow).  Returns how many ids really followed, 0 = no match (the
// draft is then the last id k times).
inline int lookup_draft(const int32_t* history, int n, int k, int ngram, int32_t* draft_out) {
    for (int g = std::min(ngram, n - 1); g >= 1; g--)
        for (int s = n - g - 1; s >= 0; s--) {
            if (memcmp(history + s, history + n - g, (size_t)g * 4) != 0) continue;
            const int take = std::min(k, n - (s + g));       // (s < n - g: at least one token follows the match)
            for (int j = 0; j < k; j++) draft_out[j] = history[s + g + std::min(j, take - 1)];
            return take;
        }
    for (int j = 0; j < k; j++) draft_out[j] = history[n - 1];
    return 0;
}

// One loop = n_steps ids for each of n_seqs sequences, produced by passes of 1 + k_pass rows per still-active sequence.
// Per pass: plan() -> the caller drafts into toks[a * S + 1 ..] and verifies (acc[a] accepted drafts, got[a * S ..] the
// pass's ids) -> emit().  toks / acc / got are reused across passes.
struct SpecLoop {
    int n_seqs, n_steps;
    std::vector<int> done;                        // ids emitted so far, per sequence
    std::vector<std::vector<int32_t>> hist;       // the host histories: non-empty, the last id is the next input token
    // the pass being assembled: active sequence a is sequence who[a] with id ids[a]; at most keep[a] of its ids are emitted
    std::vector<int> who, keep;
    std::vector<int64_t> ids;
    std::vector<int32_t> toks, acc, got;          // [na][S] input rows, [na] accepted drafts, [na][S] the pass's ids
    int na = 0, k_pass = 0, S = 1, passes = 0;

    SpecLoop(int n_seqs_, int n_steps_) : n_seqs(n_seqs_), n_steps(n_steps_), done((size_t)n_seqs_, 0), hist((size_t)n_seqs_) {}

    // The next pass.  room(i) = how many rows BEYOND the first still fit sequence i (its cache, and whatever else the
    // caller's draft step grows); k_pass = min(k, the most ids any active sequence still wants - 1, every active room), so no
    // row of a pass lies past the last position.  false: every sequence is done.
    template <typename Room>
    bool plan(int k, const int64_t* seq_ids, Room room) {
        who.clear(); ids.clear(); keep.clear();
        int fit = k;
        k_pass = 0;
        for (int i = 0; i < n_seqs; i++) {
            if (done[(size_t)i] >= n_steps) continue;
            who.push_back(i); ids.push_back(seq_ids[i]); keep.push_back(n_steps - done[(size_t)i]);
            k_pass = std::max(k_pass, n_steps - done[(size_t)i] - 1);
            fit = std::min(fit, (int)room(i));
        }
        if (who.empty()) return false;
        k_pass = std::min(k_pass, fit);
        na = (int)who.size(); S = 1 + k_pass;
        toks.assign((size_t)na * S, 0); acc.assign((size_t)na, 0); got.assign((size_t)na * S, -1);
        for (int a = 0; a < na; a++) toks[(size_t)a * S] = hist[(size_t)who[(size_t)a]].back();
        return true;
    }

    // the draft step of the lookup loops: k_pass ids per active sequence from its own history, into toks[a][1 ..]
    void draft_by_lookup(int ngram) {
        for (int a = 0; a < na && k_pass > 0; a++) {
            const std::vector<int32_t>& h = hist[(size_t)who[(size_t)a]];
            (void)lookup_draft(h.data(), (int)h.size(), k_pass, ngram, &toks[(size_t)a * S + 1]);
        }
    }

    // After the verify pass: sequence who[a] emits take = min(acc[a] + 1, keep[a]) ids, got[a][0 .. take), into
    // out_tokens[n_steps][n_seqs] and onto its history.  accepted_out (or NULL) counts the emitted ids that were drafts:
    // min(acc[a], take) (an accepted run cut short by keep counts only what was emitted).
    void emit(int32_t* out_tokens, int32_t* accepted_out = nullptr) {
        passes++;
        for (int a = 0; a < na; a++) {
            const int i = who[(size_t)a], take = std::min(acc[(size_t)a] + 1, keep[(size_t)a]);
            for (int j = 0; j < take; j++) {
                const int32_t t = got[(size_t)a * S + j];
                out_tokens[(size_t)(done[(size_t)i] + j) * n_seqs + i] = t;
                hist[(size_t)i].push_back(t);
            }
            done[(size_t)i] += take;
            if (accepted_out) accepted_out[i] += std::min(acc[(size_t)a], take);
        }
    }
};

}  // namespace nvl
