"""The one decision function of the weight-format setters (csrc/wfmt.h wf_decide) without a device: tests/wf_state_driver.cpp
plays every sequence of up to three calls drawn from all eight setters under the address and undefined-behaviour sanitizers,
as a child process, and every code and every state after a call is compared exactly with tests/wf_state_reference.py.

Calls: off, on and an unknown value of each setter; nvl_set_gq_weight_dtype at groups 32, 64, 128 and at 48.
Facts, crossed: bf16 / f32, tensor parallel or not, MoE / dense, widths that every group size divides or not, and none or one of
the three "too late" flags."""
import itertools
import subprocess
from pathlib import Path

import pytest

import wf_state_reference as R

HERE = Path(__file__).resolve().parent

# the setter's name -> wfmt.h's (target WT_*, family WFAM_*)
REQUEST = {"nvl_set_weight_dtype": (0, 0), "nvl_set_mx_weight_dtype": (0, 1), "nvl_set_gq_weight_dtype": (0, 2),
           "nvl_set_expert_dtype": (1, 0), "nvl_set_mx_expert_dtype": (1, 1), "nvl_set_gq_expert_dtype": (1, 2),
           "nvl_set_mx_head_dtype": (2, 1), "nvl_set_act_dtype": (3, 0)}
CALLS = R.calls()
CODE = {R.OK: "0", R.INVALID: "I", R.STATE: "S"}
FMT = {R.BF16: "b", R.FP8: "8", R.MXFP4: "m", R.int4(32): "3", R.int4(64): "6", R.int4(128): "1"}


def all_facts():
    for f32, tp, moe, (H, F), late in itertools.product((False, True), (False, True), (False, True), ((256, 512), (256, 64), (96, 512)),
                                                        (None, "finalized", "w2d_uploaded", "expert_uploaded")):
        f = R.Facts(f32, tp, moe, H, F, False, False, False)
        yield f._replace(**{late: True}) if late else f


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("wf_state") / "wf_state_driver"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    str(HERE / "wf_state_driver.cpp"), "-o", str(exe)], check=True)

    def run(lines):
        r = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        return r.stdout.splitlines()
    return run


def restated(facts):
    """the driver's answer for one model, from the restatement: one row of answers per state met, reused"""
    rows = {}

    def row(s):       # -> (the answers of every call from state s, joined; the states after them)
        if s not in rows:
            res = [R.step(s, facts, c) for c in CALLS]
            rows[s] = ([CODE[code] + FMT[t.wf] + FMT[t.ef] + FMT[t.hf] + "01"[t.a8] for code, t in res], [t for _, t in res])
        return rows[s]

    out = []
    text_a, next_a = row(R.START)
    for a in range(len(CALLS)):
        out.append(text_a[a])
        text_b, next_b = row(next_a[a])
        for b in range(len(CALLS)):
            out.append(text_b[b])
            out.append("".join(row(next_b[b])[0]))
    return "".join(out)


def test_every_sequence_of_up_to_three_calls(driver):
    facts = list(all_facts())
    spec = " ".join(f"{REQUEST[n][0]} {REQUEST[n][1]} {v} {g}" for n, v, g in CALLS)
    got = driver([" ".join(str(int(x)) for x in f) + f" {len(CALLS)} " + spec for f in facts])
    assert len(got) == len(facts)
    n = len(CALLS)
    for f, line in zip(facts, got):
        want = restated(f)
        assert len(line) == len(want) == 5 * (n + n * n + n ** 3)
        if line != want:
            at = next(i for i in range(len(want)) if line[i] != want[i]) // 5
            pytest.fail(f"{f}: answer {at} is {line[5 * at:5 * at + 5]}, the restatement gives {want[5 * at:5 * at + 5]}")
        assert "X" not in line and "?" not in line


def test_the_walk_reaches_every_format():
    """the sequences are long enough to matter: within three calls every stored format, expert format, head format and
    activation mode is reached on a bf16 MoE model"""
    f = R.Facts(False, False, True, 256, 512, False, False, False)
    seen = {R.START}
    for _ in range(3):
        seen |= {R.step(s, f, c)[1] for s in seen for c in CALLS}
    assert {s.wf for s in seen} == set(FMT) and {s.ef for s in seen} == set(FMT)
    assert {s.hf for s in seen} == {R.BF16, R.MXFP4} and {s.a8 for s in seen} == {False, True}
