"""The host arithmetic of the speculative decode loops (csrc/spec_loop.h: which sequences a pass carries, k_pass, keep, what is
emitted where) and the prompt-lookup drafter, without a device: tests/spec_loop_driver.cpp plays nvl::SpecLoop against a fake
verify step under the address and undefined-behaviour sanitizers, as a child process, and every answer is compared exactly with
the restatement below."""
import math
import subprocess
from pathlib import Path

import numpy as np
import pytest

from test_spec_decode_host import restated as restated_lookup

HERE = Path(__file__).resolve().parent


def restated(n_seqs, n_steps, k, T, rule, cache, hlen, accs):
    """the loop of nvl_decode_greedy_lookup / _sampled_lookup (rule 0) and nvl_decode_speculative (rule 1), include/nvllm.h"""
    done, cache, hlen, at = [0] * n_seqs, list(cache), list(hlen), 0
    out, passes = [-1] * (n_steps * n_seqs), []
    while any(d < n_steps for d in done):
        who = [i for i in range(n_seqs) if done[i] < n_steps]
        pos = {i: max(cache[i], hlen[i]) if rule else cache[i] for i in who}
        k_pass = min([k, max(n_steps - done[i] - 1 for i in who)] + [T - pos[i] - 1 for i in who])
        rows = []
        for i in who:
            keep, acc = n_steps - done[i], min(accs[at % len(accs)], k_pass)
            at, take = at + 1, min(acc + 1, keep)
            rows.append((i, keep, pos[i], acc, take, done[i]))
            for j in range(take):
                out[(done[i] + j) * n_seqs + i] = 1000 * i + done[i] + j
            done[i], cache[i], hlen[i] = done[i] + take, cache[i] + take, hlen[i] + take
        passes.append((k_pass, rows))
    return passes, out


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("spec_loop") / "spec_loop_driver"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    str(HERE / "spec_loop_driver.cpp"), "-o", str(exe)], check=True)

    def run(lines):
        r = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        return r.stdout.splitlines()
    return run


def play(driver, cases):
    """cases: (n_seqs, n_steps, k, T, rule, cache, hlen, accs) -> [(passes, out)], each checked against the restatement and
    the invariants that hold for every case"""
    lines = ["C " + " ".join(map(str, [n, s, k, T, rule, *cache, *hlen, len(accs), *accs]))
             for n, s, k, T, rule, cache, hlen, accs in cases]
    answer = iter(driver(lines))
    res = []
    for case in cases:
        n, s, k, T, rule, cache, hlen, accs = case
        passes = []
        for line in answer:
            f = line.split()
            assert "BAD-ROW" not in f, (case, line)
            v = list(map(int, f[1:]))
            if f[0] == "OUT":
                n_passes, out = v[0], v[1:]
                break
            assert f[0] == "P" and len(v) == 2 + 6 * v[1], line
            passes.append((v[0], [tuple(v[2 + 6 * a:8 + 6 * a]) for a in range(v[1])]))
        assert (passes, out) == restated(*case), case
        assert n_passes == len(passes)
        # every sequence emits exactly n_steps ids, in order, at out[step * n_seqs + i]
        assert out == [1000 * i + step for step in range(s) for i in range(n)], case
        # no row of any pass lies past the last position
        for k_pass, rows in passes:
            assert 0 <= k_pass <= k and all(pos + 1 + k_pass <= T for _, _, pos, _, _, _ in rows), (case, k_pass, rows)
        assert math.ceil(s / (k + 1)) <= n_passes <= s, case
        res.append((passes, out))
    return res


def test_named_cases(driver):
    ALL, NONE = [7], [0]
    (last, full, none, cut, one, one_k7) = play(driver, [
        # sequence 0 ends exactly at position T - 1 and sequence 1 is far behind it (test_loop_up_to_the_last_position)
        (2, 12, 3, 64, 0, [52, 10], [1, 1], [1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 0, 0]),
        (1, 12, 3, 64, 0, [5], [1], ALL),
        (1, 12, 3, 64, 0, [5], [1], NONE),
        # sequence 0 rejects everything, so the passes stay wide while sequence 1 accepts past what it still wants
        (2, 6, 3, 64, 0, [5, 5], [1, 1], [0, 3]),
        (3, 1, 3, 64, 0, [5, 63, 0], [1, 1, 1], ALL),
        (1, 1, 7, 64, 1, [20], [63], ALL),
    ])
    # sequence 0 reaches position T - 1 with one id to go: its room forces a pass of one row while sequence 1 still wants six
    assert any(k_pass == 0 and len(rows) == 2 and max(keep for _, keep, *_ in rows) > 1 for k_pass, rows in last[0])
    assert max(pos + 1 + k_pass for k_pass, rows in last[0] for _, _, pos, *_ in rows) == 64
    assert len(full[0]) == math.ceil(12 / 4)
    assert len(none[0]) == 12
    assert any(acc + 1 > keep and take == keep for _, rows in cut[0] for _, keep, _, acc, take, _ in rows)
    assert [p[0] for p in one[0]] == [0] and [p[0] for p in one_k7[0]] == [0]


@pytest.mark.parametrize("seed", range(4))
def test_seeded_cases(driver, seed):
    r = np.random.default_rng(seed)
    cases = []
    for _ in range(100):
        n, s, k, rule = int(r.integers(1, 5)), int(r.integers(1, 17)), int(r.integers(1, 8)), int(r.integers(0, 2))
        T = int(r.integers(s + 1, 80))
        slack = int(r.integers(0, 3)) * int(r.integers(0, 8))       # often 0: some sequence ends exactly at T - 1
        cache = [int(r.integers(0, T - s + 1)) for _ in range(n)]
        cache[int(r.integers(0, n))] = max(T - s - slack, 0)
        hlen = [int(r.integers(1, T - s + 1)) for _ in range(n)]
        accs = r.integers(0, 8, int(r.integers(1, 12))).tolist()
        cases.append((n, s, k, T, rule, cache, hlen, accs))
    play(driver, cases)


def test_lookup_draft_under_the_sanitizers(driver):
    """the seeded histories of test_spec_decode_host.py through the header's lookup_draft"""
    cases = []
    for seed in range(6):
        r = np.random.default_rng(seed)
        for _ in range(200):
            n = int(r.integers(1, 40))
            h = r.integers(0, int(r.integers(2, 6)), n).tolist()
            cases.append((h, int(r.integers(1, 8)), int(r.integers(1, 5))))
    got = driver(["L " + " ".join(map(str, [k, g, len(h), *h])) for h, k, g in cases])
    assert len(got) == len(cases)
    for line, (h, k, g) in zip(got, cases):
        v = list(map(int, line.split()[1:]))
        assert (v[1:], v[0]) == restated_lookup(h, k, g), (h, k, g)
