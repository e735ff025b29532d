"""Generates tests/golden/cli_trees_parent.json: what `hygeia infer`,
`infer_many` and `infer_genome` write, print and launch over two small
chromosomes, with the launch functions replaced by the deterministic fakes of
tests/cli_trees.py. Recorded from the commit before the three commands were
put on one task driver (run from the repo root at that commit: ``python
tests/golden/make_cli_trees.py``). Needs no GPU.

tests/test_cli_trees_cpu.py runs the same collect() on the code under test and
compares every entry.
"""
from __future__ import annotations

import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

OUT = os.path.join(HERE, "cli_trees_parent.json")


def main() -> None:
    import pytest

    import cli_trees

    with tempfile.TemporaryDirectory() as root, pytest.MonkeyPatch.context() as mp:
        doc = cli_trees.golden_doc(cli_trees.collect(root, mp))
    with open(OUT, "w") as f:
        json.dump(doc, f, indent=0, sort_keys=True)
        f.write("\n")
    print({name: len(r["tree"]) for name, r in doc.items() if "tree" in r})


if __name__ == "__main__":
    main()
