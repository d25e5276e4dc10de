"""Writes tests/golden/cli_record.json: what rtp_main answers to every case of tests/cli_cases.py — refused with which exit code and
"rtp_main: …" line, or handed to which frame driver.  Run it once against an rtp_main of the commit whose answers are the reference
(the parent of parse_cli), on a machine WITHOUT a GPU, never against the tree under test:

  python3 tests/golden/make_cli_record.py <that build>/ray-tracing-practice_amd/rtp_main

Without a GPU an accepted command line dies at its first device call, and the message says which driver it had entered: check_rt's
"RT error = … at FILE:LINE" (SITES below: the five call sites of that commit), or the message of one of the four device objects main()
made itself — all of them recorded as code 0, "driver:<name>".  One class of cases is recorded by hand instead, cli_cases.is_moved(): the
refusals that the reference build reached only behind a successful rt_env_create; the script asserts that the reference build fails in
rt_env_create there, and that no other case belongs to that class.  The record holds each distinct answer once and, per case in the order
of cases(), its index."""
import concurrent.futures
import json
import os
import re
import subprocess
import sys
import tempfile
from pathlib import Path

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import cli_cases as cc          # noqa: E402

# the first device call of each driver in the reference commit's sources
SITES = {"host/render_driver.cpp:355": "lens", "host/render_driver.cpp:524": "adaptive", "host/render_driver.cpp:596": "sharded",
         "host/render_driver.cpp:283": "pipelined", "host/main.cpp:739": "frames"}
CREATED = re.compile(r"^rtp_main: (?:(?:--fog-grid|--fog-heat|--fog-glow-sample): rt_|--env: (?:%s): rt_env_)" % "|".join(map(re.escape, cc.LOADABLE_ENV)))
ENV_CREATED = re.compile(r"^rtp_main: --env: \S+: rt_env_")


def answer(exe, scene, cwd, case):
    args, devices = case
    env = {k: v for k, v in os.environ.items() if k != "RTP_DEVICES"}
    if devices is not None:
        env["RTP_DEVICES"] = devices
    r = subprocess.run([exe, "--gpu", *args], input=scene, capture_output=True, text=True, encoding="utf-8", cwd=cwd, env=env, timeout=60)          # no case may time out
    sites = set(re.findall(r"at (host/\w+\.cpp:\d+) '", r.stderr)) if "RT error = " in r.stderr else set()
    if sites:          # (the pipelined driver prints once per GPU, the lines can interleave and the threads' exits collide: any exit code)
        assert len(sites) == 1, (cc.case_id(case), r.returncode, r.stderr)
        return 0, "driver:" + SITES[sites.pop()], "RT error"
    lines = [l for l in r.stderr.splitlines() if l.startswith("rtp_main: ")]
    assert len(lines) == 1, (cc.case_id(case), r.returncode, r.stderr)
    line = lines[0]
    assert r.returncode in (2, 99), (cc.case_id(case), r.returncode, r.stderr)
    if CREATED.match(line):
        return 0, "driver:lens", line
    return r.returncode, line, line


def main():
    exe = os.path.abspath(sys.argv[1])
    with open(os.path.join(HERE, "test_config.txt")) as f:
        scene = f.read()
    all_cases = cc.cases()
    with tempfile.TemporaryDirectory() as cwd:
        before = cc.make_files(Path(cwd))
        with concurrent.futures.ThreadPoolExecutor(8) as pool:
            got = list(pool.map(lambda c: answer(exe, scene, cwd, c), all_cases))
        assert sorted(os.listdir(cwd)) == before, os.listdir(cwd)
    answers, index, moved = [], [], 0
    for case, (code, verdict, line) in zip(all_cases, got):
        if cc.is_moved(case):          # by hand: the refusal behind rt_env_create, in the order of the reference commit's blocks
            assert ENV_CREATED.match(line) and "rt_env_create" in line, (cc.case_id(case), line)
            code, verdict = 99, "rtp_main: " + cc.moved_refusal(case)
            moved += 1
        else:
            assert not (ENV_CREATED.match(line) and "--lit" in case[0] and cc.has_faulty_lit_tail(case)), ("an unmarked case of the moved class", cc.case_id(case))
        if [code, verdict] not in answers:
            answers.append([code, verdict])
        index.append(answers.index([code, verdict]))
    cpu = subprocess.run([exe, "--cpu"], stdin=subprocess.DEVNULL, capture_output=True, text=True, encoding="utf-8", timeout=60)          # the one refusal before --gpu
    assert cpu.returncode == 2 and cpu.stderr.startswith("rtp_main: --cpu"), (cpu.returncode, cpu.stderr)
    record = {"cases": len(all_cases), "ids_sha256": cc.ids_digest(all_cases), "moved": moved, "answers": answers, "answer_of_case": index,
              "cpu_mode": [cpu.returncode, cpu.stderr.rstrip("\n")]}
    with open(os.path.join(HERE, "cli_record.json"), "w") as f:
        json.dump(record, f, separators=(",", ":"), ensure_ascii=False)
        f.write("\n")
    print(f"{len(all_cases)} cases, {len(answers)} distinct answers, {sum(1 for a in answers if a[0])} refusal texts, {moved} recorded by hand")


if __name__ == "__main__":
    main()
