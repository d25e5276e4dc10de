"""Writes tests/golden/fog_refusals.json: (status, message) of every case of tests/fog_refusal_cases.py, from the library this process
loads.  Run it once against a build of the commit whose refusals are the reference (the parent of the fold), not against
the tree under test:

  RTP_AMD_LIB=<that build>/ray-tracing-practice_amd/librtp_amd.so python3 tests/golden/make_fog_refusals.py

Every case must be refused with RT_ERR_INVALID_ARG there (no case may get as far as reading a handle); the script asserts it.  The record
holds each distinct message once and, per case in the order of cases(), its index."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.join(ROOT, "ray-tracing-practice_amd"), os.path.join(ROOT, "tests")]

import fog_refusal_cases as fc          # noqa: E402
import rtp_bindings as rb          # noqa: E402


def main():
    call = fc.Caller(rb.amd_lib())
    all_cases = fc.cases()
    messages, index = [], []
    for case in all_cases:
        status, message = call(case)
        assert status == fc.INVALID, (fc.case_id(case), status, message)
        if message not in messages:
            messages.append(message)
        index.append(messages.index(message))
    record = {"cases": len(all_cases), "ids_sha256": fc.ids_digest(all_cases), "status": fc.INVALID, "messages": messages, "message_of_case": index}
    with open(os.path.join(HERE, "fog_refusals.json"), "w") as f:
        json.dump(record, f, separators=(",", ":"))
        f.write("\n")
    print(f"{len(all_cases)} cases, {len(messages)} distinct messages")


if __name__ == "__main__":
    main()
