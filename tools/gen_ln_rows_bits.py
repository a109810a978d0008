"""Writes tests/golden/ln_rows_bits.json: SHA-256 digests of every output buffer of the fp16 row-LayerNorm entry points
on the fixed inputs of tests/ln_rows_cases.py, from the library that is built in this tree, on the MI355X.

Run it on the commit whose bits are to be kept (the parent of a refactor), never on the refactored tree:
    python tools/gen_ln_rows_bits.py [OUT.json]
Every case runs twice; a buffer whose two digests differ is reported and left out."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "multimodal-isic_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import ln_rows_cases as C  # noqa: E402


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "ln_rows_bits.json")
    digests, unstable = {}, []
    for group in C.GROUPS:
        first, second = C.digests(group), C.digests(group)
        assert first.keys() == second.keys()
        for k in first:
            if first[k] == second[k]:
                digests[k] = first[k]
            else:
                unstable.append(k)
    try:
        hipcc = subprocess.run(["hipcc", "--version"], capture_output=True, text=True).stdout.strip().splitlines()[:2]
    except OSError:
        hipcc = ["hipcc not found"]
    doc = {"about": "sha256 of the output buffers of tests/ln_rows_cases.py; written by tools/gen_ln_rows_bits.py",
           "hipcc": hipcc, "not_reproducible": unstable, "digests": digests}
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(digests)} digests -> {out_path}; not reproducible: {unstable}")


if __name__ == "__main__":
    main()
