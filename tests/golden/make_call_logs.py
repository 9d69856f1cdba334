"""Generate tests/golden/call_logs.json — the op sequence of the window loop's three callers over the CPU stand-ins:
    python tests/golden/make_call_logs.py
Run it on the commit whose launch sequence is to be pinned (first: the parent of the commit that introduced `EmageAudioModel._window_step`)
and ONLY there: a later change that moves a launch on purpose regenerates the file and says so.  Needs no device and no reference tree.
The workloads are those of tests/call_log_cases.py; per workload the file keeps the number of calls, the count per op name and a SHA-256 of
the newline-joined names (the lists themselves run to tens of thousands of names)."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import call_log_cases  # noqa: E402


def main():
    doc = {name: call_log_cases.digest(call_log_cases.calls_of(name)) for name in call_log_cases.WORKLOADS}
    path = os.path.join(HERE, "call_logs.json")
    with open(path, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    for name, d in doc.items():
        print(f"{name}: {d['n']} calls, {len(d['counts'])} ops, sha256 {d['sha256'][:16]}")
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
