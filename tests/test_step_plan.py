"""The step's schedule (csrc/lqro_plan.hpp: plan_step) pinned on the CPU.

Every schedule gives bit-identical results, so no GPU test notices a wrong
side width or a lost split; this does.  tests/cpp/lqro_plan_main.cpp, which
includes nothing of the project but lqro_plan.hpp, is compiled with g++ and
run over tests/golden/step_plan.json: every StepPlan field of every case must
equal the recorded one.  The recorded values come from the commit before
plan_step existed (the fixture's `provenance`), not from plan_step.
"""
import json
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAIN = os.path.join(ROOT, "tests", "cpp", "lqro_plan_main.cpp")
FIXTURE = os.path.join(ROOT, "tests", "golden", "step_plan.json")


def test_plan_matches_recorded_schedule(tmp_path):
    exe = str(tmp_path / "lqro_plan_main")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", MAIN, "-o", exe], check=True)
    with open(FIXTURE) as f:
        fx = json.load(f)
    cases = fx["cases"]
    assert len(cases) >= 300 and all(len(c["in"]) == len(fx["input_fields"]) for c in cases)
    text = "".join(" ".join(str(v) for v in c["in"]) + "\n" for c in cases)
    r = subprocess.run([exe], input=text, capture_output=True, text=True, check=True)
    lines = r.stdout.splitlines()
    assert len(lines) == len(cases)
    wrong = []
    for c, line in zip(cases, lines):
        got = {k: int(v) for k, v in (tok.split("=") for tok in line.split())}
        want = dict(zip(fx["output_fields"], c["out"]))
        assert set(got) == set(want), (c["name"], sorted(got), sorted(want))
        for k in fx["output_fields"]:
            if got[k] != want[k]:
                wrong.append((c["name"], k, got[k], want[k]))
    assert not wrong, f"{len(wrong)} fields differ (case, field, got, recorded): {wrong[:20]}"


def test_named_cases_read_as_documented():
    """The cases a reader can check by hand say what DESIGN §6.1 and the
    planner's comments say."""
    with open(FIXTURE) as f:
        fx = json.load(f)
    out = {c["name"]: dict(zip(fx["output_fields"], c["out"])) for c in fx["cases"]}
    c3 = out["c3_steady_qhull_balance_off"]   # 177 inside pairs + 4 spare: "192 -> 181 side CUs"
    assert (c3["side"], c3["nwait"], c3["hot"], c3["split"], c3["spec"], c3["early"]) == (181, 181, 1, 1, 1, 1)
    assert (c3["nblk"], c3["nside"]) == (75, 181)
    first = out["c3_first_two_steps_qhull"]
    assert (first["hot"], first["nwait"], first["split"], first["early"], first["nblk"]) == (0, 0, 0, 0, 256)
    for name in ("n_cu_63_plain", "smoke_sizes_plain_12", "smoke_sizes_plain_32", "slots_65535_plain",
                 "culling_on_plain"):
        assert (out[name]["hot"], out[name]["nwait"]) == (0, 0), name
    assert out["culling_on_plain"]["npr"] == 8
    assert out["slots_65536_hot"]["hot"] == 1
    c5, c5_off = out["c5_shard_balance_on"], out["c5_shard_balance_off"]
    assert c5["hot"] == 1 and c5["big_inline"] == 1 and c5["side"] < c5_off["side"] == 224
    p1 = out["phase1_own_newv_early_internal"]
    assert (p1["early"], p1["early_internal"]) == (1, 1)
    assert out["canonical_local_1067_inside"]["hot"] == 1 and out["canonical_local_2496_inside"]["hot"] == 0
