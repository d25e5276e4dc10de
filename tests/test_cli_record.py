"""rtp_main's command line (host/cli.cpp) against the record of tests/golden/cli_record.json, which
tests/golden/make_cli_record.py took from the rtp_main before parse_cli: for every case of tests/cli_cases.py the exit code and the text of
its refusal, or the frame driver it is handed to.  No GPU: parse_cli needs none, and only refused command lines go through rtp_main itself."""
import json
import os
import subprocess

import cli_cases as cc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PKG = os.path.join(ROOT, "ray-tracing-practice_amd")
EXE = os.path.join(PKG, "rtp_main")


def _record():
    with open(os.path.join(HERE, "golden", "cli_record.json"), encoding="utf-8") as f:
        record = json.load(f)
    all_cases = cc.cases()
    assert len(all_cases) == record["cases"] == len(record["answer_of_case"])
    assert cc.ids_digest(all_cases) == record["ids_sha256"], "the case list differs from the recorded one"
    return all_cases, record


def test_parse_cli_gives_every_recorded_answer(tmp_path):
    """tests/cpu_native/cli_probe.cpp — parse_cli, cli.cpp and the image readers alone — under AddressSanitizer + UBSan, once over all
    cases: every code and verdict is the recorded one, the sanitizers stay silent, and no file is written."""
    all_cases, record = _record()
    exe = str(tmp_path / "cli_probe")
    srcs = [os.path.join(HERE, "cpu_native", "cli_probe.cpp")] + [os.path.join(PKG, "host", f) for f in ("cli.cpp", "texture_io.cpp", "jpeg_decoder.cpp")]
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-ffp-contract=off", "-o", exe] + srcs,
                   check=True)
    cwd = tmp_path / "cwd"
    cwd.mkdir()
    before = cc.make_files(cwd)
    lines = "".join(cc.case_line(c) + "\n" for c in all_cases)
    out = subprocess.run([exe], input=lines, capture_output=True, text=True, encoding="utf-8", cwd=cwd, timeout=300,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert out.returncode == 0 and out.stderr == "", out.stderr[-2000:]
    got = out.stdout.splitlines()
    assert len(got) == len(all_cases)
    wrong = []
    for case, line, k in zip(all_cases, got, record["answer_of_case"]):
        code, verdict = record["answers"][k]
        if line != f"{code}\t{verdict}":
            wrong.append((cc.case_id(case), line, (code, verdict)))
    assert not wrong, f"{len(wrong)} of {len(all_cases)} answers differ from the record; the first: {wrong[:5]}"
    assert sorted(os.listdir(cwd)) == before


def test_rtp_main_prints_every_recorded_refusal(test_config_text, tmp_path):
    """One case per distinct refusal of the record through rtp_main itself: the exit code and the "rtp_main: …" line are the recorded ones,
    and the working directory holds no new file.  (Accepted command lines are not run: with a GPU they would render.)"""
    all_cases, record = _record()
    before = cc.make_files(tmp_path)
    first = {}
    for case, k in zip(all_cases, record["answer_of_case"]):
        first.setdefault(k, case)
    refused = [(record["answers"][k], case) for k, case in sorted(first.items()) if record["answers"][k][0] != 0]
    assert len(refused) >= 67 and {code for (code, _), _ in refused} == {2, 99}
    for (code, verdict), (args, devices) in refused:
        env = {k: v for k, v in os.environ.items() if k != "RTP_DEVICES"}
        if devices is not None:
            env["RTP_DEVICES"] = devices
        r = subprocess.run([EXE, "--gpu", *args], input=test_config_text, capture_output=True, text=True, encoding="utf-8", cwd=tmp_path, env=env, timeout=60)
        said = [l for l in r.stderr.splitlines() if l.startswith("rtp_main: ")]
        assert (r.returncode, said) == (code, [verdict]), (args, devices, r.returncode, r.stderr[-400:])
        assert r.stdout == ""
    r = subprocess.run([EXE, "--cpu"], stdin=subprocess.DEVNULL, capture_output=True, text=True, encoding="utf-8", cwd=tmp_path, timeout=60)          # the refusal before --gpu
    assert [r.returncode, r.stderr.rstrip("\n")] == record["cpu_mode"] and r.stdout == ""
    assert sorted(os.listdir(tmp_path)) == before
