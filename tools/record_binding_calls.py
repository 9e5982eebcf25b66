"""Writes tests/golden/binding_calls.json: what every wrapper of api.py hands to the render library, as tests/binding_model.py's driver
records it against a stand-in library (no GPU; the host library is the real one).  tests/test_binding_calls.py compares the working
tree's api.py with it.  Run it on the commit whose behaviour is to be kept:

    python tools/record_binding_calls.py [--commit NAME] [--out FILE]

The file's first line names that commit (default: git's HEAD) and, with --note, what was changed on purpose since; one line per
wrapper follows."""
import argparse
import importlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def dumps(commit, entries, note=None):
    lines = [json.dumps({"recorded_from": commit, **({"note": note} if note else {})})] + [json.dumps(e) for e in entries]
    return "[\n" + ",\n".join(lines) + "\n]\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", default=None)
    ap.add_argument("--note", default=None, help="what in the file is deliberately not that commit's behaviour")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "binding_calls.json"))
    a = ap.parse_args()
    commit = a.commit or subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, stdout=subprocess.PIPE, text=True, check=True).stdout.strip()
    import binding_model
    api = importlib.import_module("rendering-learning_amd").api
    saved = []

    def patch(obj, name, value):
        saved.append((obj, name, getattr(obj, name)))
        setattr(obj, name, value)

    try:
        entries = binding_model.drive(api, patch)
    finally:
        for obj, name, value in reversed(saved):
            setattr(obj, name, value)
    with open(a.out, "w") as f:
        f.write(dumps(commit, entries, a.note))
    print(f"{a.out}: {len(entries)} wrappers, {sum(len(v['calls']) for e in entries for v in e.values() if isinstance(v, dict) and 'calls' in v)} calls")


if __name__ == "__main__":
    main()
