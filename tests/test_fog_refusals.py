"""The parameter refusals of the twelve fog entry points against the record of tests/golden/fog_refusals.json, which
tests/golden/make_fog_refusals.py took from the build before the calls were folded onto one setup: status and full message of every case
of tests/fog_refusal_cases.py, so every refusal's text and its place in the order of checks.  No GPU: every call has a NULL scene."""
import json
import os

import fog_refusal_cases as fc
import rtp_bindings as rb

HERE = os.path.dirname(os.path.abspath(__file__))


def test_every_refusal_is_the_recorded_one():
    with open(os.path.join(HERE, "golden", "fog_refusals.json")) as f:
        record = json.load(f)
    all_cases = fc.cases()
    assert len(all_cases) == record["cases"] == len(record["message_of_case"])
    assert fc.ids_digest(all_cases) == record["ids_sha256"], "the case list differs from the recorded one"
    entries = {c[0] for c in all_cases}
    assert len(entries) == 12 and all(e in rb.RTP_AMD_SYMBOLS for e in entries), entries
    call = fc.Caller(rb.amd_lib())
    wrong = []
    for case, k in zip(all_cases, record["message_of_case"]):
        got = call(case)
        want = (record["status"], record["messages"][k])
        if got != want:
            wrong.append((fc.case_id(case), got, want))
    assert not wrong, f"{len(wrong)} of {len(all_cases)} refusals differ from the record; the first: {wrong[:5]}"
