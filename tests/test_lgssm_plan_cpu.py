"""The host-only schedule planner of the state-space engines (csrc/lgssm_plan.hpp), without a GPU.

The header is compiled with g++ into a small driver (tests/host_emul/lgssm_plan_main.cpp) and its segmentation is held to rows derived by hand
from the documented rules: the two headline shapes (C2, C1) and one row per documented decision (include/rxhip.h "Environment").
OPEN: the table recorded on an MI355X from the commit before the planner was split out (tests/golden/lgssm_schedules.json through
rxhip_get_schedule) is not here — no device was available; the shapes of DECISIONS are the ones to record.  The same driver shows that every
field of ScheduleHooks is part of the engine-pool key.
"""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rxinfer.jl_amd", "csrc")

# by hand from the rules in lgssm_plan.hpp (d = dy = 4, one model):
#   C2, T = 10⁵ × 1024 chains: 99999 steps, S_target = ⌈131072 / 1024⌉ = 128 (below the latency bound ⌈√(3.3 · 99999)⌉ = 575; no small-sweep cap above
#       16 chains), L = ⌈99999 / 128⌉ = 782, S = ⌈99999 / 782⌉ = 128
#   C1, T = 1000 × 1 chain: 999 steps, cap = 256 lanes, ⌈999 / 256⌉ = 4 ≤ 32 so the short segments of k_small_sweep: S_target = min(256, 999 / 3) = 256,
#       L = ⌈999 / 256⌉ = 4, S = ⌈999 / 4⌉ = 250
HAND = [
    dict(name="c2_headline", d=4, dy=4, T=100000, n_chains=1024, n_models=1, segments=0, allow_missing=False, step_model=False, chain_model=False, hooks={}, S=128, L=782),
    dict(name="c1", d=4, dy=4, T=1000, n_chains=1, n_models=1, segments=0, allow_missing=False, step_model=False, chain_model=False, hooks={}, S=250, L=4),
]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("lgssm_plan") / "lgssm_plan_main")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, "-o", exe, os.path.join(ROOT, "tests", "host_emul", "lgssm_plan_main.cpp")], check=True)
    return exe


def _run(exe, rows):
    lines = []
    for r in rows:
        dense = r["d"] > 4 or r["dy"] > 4   # no kernels of the d, dy ≤ 4 family: the MFMA path
        f = [r["d"], r["dy"], r["T"], r["n_chains"], r["n_models"], r["segments"], int(dense), int(r["allow_missing"]), int(r["step_model"]), int(r["chain_model"])]
        lines.append(" ".join(map(str, f)) + "".join(f" {k}={v}" for k, v in r["hooks"].items()))
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
    keys = {l.split()[1]: l.split()[2] == "1" for l in out if l.startswith("key ")}
    plans = [tuple(map(int, l.split()[1:])) for l in out if l.startswith("plan ")]
    assert len(plans) == len(rows)
    return keys, plans


def test_header_has_no_hip_dependency():
    src = open(os.path.join(CSRC, "lgssm_plan.hpp")).read()
    assert not re.search(r"#include\s*[<\"]hip", src)


def test_hand_derived_rows(driver):
    _, plans = _run(driver, HAND)
    for r, p in zip(HAND, plans):
        assert (p[0], p[1]) == (r["S"], r["L"]), (r["name"], p)


def _row(name, d, T, C, **kw):
    r = dict(name=name, d=d, dy=d, T=T, n_chains=C, n_models=1, segments=0, allow_missing=False, step_model=False, chain_model=False, hooks={})
    r.update(kw)
    return r


# one row per documented decision of the segmentation
DECISIONS = [
    _row("small_cap_16_chains", 4, 400, 16), _row("small_cap_17_chains", 4, 400, 17), _row("small_short_4_chains", 4, 400, 4),
    _row("small_sweep_off", 4, 400, 4, hooks={"RXHIP_SMALL_SWEEP": "0"}),
    _row("segments_5_T203", 4, 203, 128, segments=5), _row("per_chain_models", 4, 1000, 64, n_models=64, chain_model=True), _row("T1", 4, 1, 4), _row("T2", 4, 2, 4),
    _row("c3", 64, 10000, 1), _row("d16_split", 16, 1000, 512), _row("d16_split_off", 16, 1000, 512, hooks={"RXHIP_DENSE_SPLIT": "0"}),
    _row("d8_even_batch", 8, 1000, 6), _row("d8_odd_batch", 8, 1000, 7), _row("d8_no_pack", 8, 1000, 6, hooks={"RXHIP_NO_PACK": "1"}),
    _row("masked_d4", 4, 1000, 8, allow_missing=True), _row("masked_d4_one_segment", 4, 1000, 8, allow_missing=True, hooks={"RXHIP_ONE_SEGMENT": "1"}),
]


def test_documented_decisions(driver):
    _, plans = _run(driver, DECISIONS)
    S = {r["name"]: p[0] for r, p in zip(DECISIONS, plans)}
    L = {r["name"]: p[1] for r, p in zip(DECISIONS, plans)}
    pack = {r["name"]: p[3] for r, p in zip(DECISIONS, plans)}
    for r, p in zip(DECISIONS, plans):   # no empty segment, every step in one: (S − 1) · L + Llast = T − 1 with 1 ≤ Llast ≤ L
        if r["T"] > 1:
            assert (p[0] - 1) * p[1] + p[2] == r["T"] - 1 and 1 <= p[2] <= p[1], (r["name"], p)
    assert 16 * S["small_cap_16_chains"] <= 256 and L["small_cap_16_chains"] >= 3      # the lanes of k_small_sweep's one workgroup; short segments, 3 steps at least
    assert 17 * S["small_cap_17_chains"] > 256 and L["small_cap_17_chains"] >= 8       # above 16 chains: no cap, segments of 8 steps at least
    # 4 chains, 399 steps: 64 lanes' worth of short segments, L = ⌈399 / 64⌉ = 7; without k_small_sweep the latency bound ⌈√(3.3 · 399)⌉ = 37 segments of 11
    assert (S["small_short_4_chains"], L["small_short_4_chains"]) == (57, 7) and (S["small_sweep_off"], L["small_sweep_off"]) == (37, 11)
    assert (S["segments_5_T203"], L["segments_5_T203"]) == (5, 41)                      # a request: L = ⌈202 / 5⌉, S = ⌈202 / 41⌉
    assert (S["T1"], S["T2"], L["T2"]) == (0, 1, 1)
    assert (S["per_chain_models"], L["per_chain_models"]) == (56, 18)                   # the latency bound ⌈√(3.3 · 999)⌉ = 58 segments: L = ⌈999 / 58⌉ = 18
    assert S["c3"] == 1000                                                              # d = 64, time-invariant: four workgroups per CU of segments (⌈9999 / 1024⌉ = 10 steps)
    assert (S["d16_split"], L["d16_split"]) == (32, 32) and S["d16_split_off"] == 24   # the split asks for ≈ 32-step segments; without it 256 · 48 / 512 = 24
    assert (pack["d8_even_batch"], pack["d8_odd_batch"], pack["d8_no_pack"]) == (2, 1, 1)
    assert (S["masked_d4"], L["masked_d4"]) == (32, 32) and S["masked_d4_one_segment"] == 1   # 8 chains: the 256-lane cap (32 segments) applies, the short segments do not


def test_every_hook_field_is_in_the_pool_key(driver):
    keys, _ = _run(driver, HAND)
    src = open(os.path.join(CSRC, "lgssm_plan.hpp")).read()
    fields = re.findall(r"^\s*X\(([^,]+),\s*(\w+),", src, flags=re.M)
    assert len(fields) >= 20 and set(keys) == {f for _, f in fields}   # the driver loops over the header's own list
    assert all(keys.values()), [k for k, v in keys.items() if not v]


def test_hooks_are_read_by_name(driver):
    base = dict(HAND[1])
    rows = [dict(base, hooks={"RXHIP_ONE_PASS": "1"}), dict(base, hooks={"RXHIP_ONE_PASS": "0"}), dict(base, n_chains=64, T=65536 + 1, hooks={}),
            dict(base, n_chains=64, T=65536, hooks={}), dict(base, n_chains=64, hooks={"RXHIP_ONE_PASS": "1", "RXHIP_MEAN_RECORDS": "1"}),
            dict(base, n_chains=64, hooks={"RXHIP_ONE_PASS": "1", "RXHIP_BACKWARD_LANES": "1"}), dict(base, n_chains=64, hooks={"RXHIP_ONE_PASS": "1"})]
    _, plans = _run(driver, rows)
    assert [p[4] for p in plans] == [1, 0, 1, 1, 1, 1, 1]      # one-pass: forced on / off, from chains · T = 4194304 on
    assert [p[5] for p in plans[4:]] == [0, 0, 1]              # reverse-filter candidates: not with records, not on the lanes' backward sweep
