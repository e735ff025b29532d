"""Generates tests/golden/tg_plan_parent.json: what the two-group launcher
selects (widths, LDS bytes, global-weights flag, per-chain scratch) over a scan
of model shapes, forced widths and launch sizes, recorded from the library of
the commit before the launcher was rewritten around one kernel plan (run from
the repo root against that library: ``HYG_LIB_PATH=/path/to/libhygeia_amd.so
python tests/golden/make_tg_plan.py``). Needs no GPU: every value is a
host-side diagnostic of the C ABI, and with 1 or 100 000 chains it does not
depend on the device's CU count.

tests/test_tg_plan_cpu.py recomputes the rows with scan() on the library under
test and compares: the digest over all of them, and the rows of K = 6, 12, 13
one by one so that a failure names the case.
"""
from __future__ import annotations

import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

OUT = os.path.join(HERE, "tg_plan_parent.json")
KS = range(2, 17)
BS = (25, 64)
MS = (1, 2, 49, 50, 51, 54, 63, 64, 65, 127, 128, 129, 200, 255, 256)
FORCED = ((0, 0), (512, 768), (768, 512), (64, 128))
CHAINS = (1, 100000)
ROWS_KEPT = (6, 12, 13)  # K whose rows the fixture holds in full
COLUMNS = ("K M B force_fwd force_bwd n_chains | threads_fwd threads_bwd lds_fwd lds_bwd "
           "lds_fwd_256 lds_fwd_512 lds_fwd_768 lds_bwd_256 lds_bwd_512 lds_bwd_768 global_weights scratch_per_chain")


def small_model(K: int, M: int, B: int):
    """A model of the shape with tiny tables (the selection reads the shape alone)."""
    from hygeia_amd import synthetic as syn
    from hygeia_amd import two_group

    mu, sg = syn.regime_params(K)
    return two_group.CaseControlModel(mu, sg, two_group.uniform_theta(K, 0.8), num_resampled_ancestors=M,
                                      num_samples_backward=B, max_total_reads=4, max_duration=8)


def scan(lib, ks=KS):
    """Yields (model, row) per case, the model open and the widths forced as the
    row says while the consumer holds it; row is the text of COLUMNS' values."""
    from hygeia_amd import _lib

    for K in ks:
        for B in BS:
            for M in MS:
                try:
                    m = small_model(K, M, B)
                except (ValueError, _lib.HygError):
                    continue  # not a shape the model accepts
                try:
                    h = m.handle
                    fixed = [lib.hyg_tg_lds_bytes(h, nt, b) for b in (0, 1) for nt in (256, 512, 768)]
                    fixed += [lib.hyg_tg_global_weights(h),
                              lib.hyg_tg_workspace_bytes(h, 2, 1000) - lib.hyg_tg_workspace_bytes(h, 1, 1000)]
                    for force in FORCED:
                        assert lib.hyg_tg_force_threads(*force) == 0
                        for n in CHAINS:
                            ntf = lib.hyg_tg_threads_per_chain(h, n)
                            ntb = lib.hyg_tg_backward_threads_per_chain(h, n)
                            row = [K, M, B, *force, n, "|", ntf, ntb, lib.hyg_tg_lds_bytes(h, ntf, 0),
                                   lib.hyg_tg_lds_bytes(h, ntb, 1), *fixed]
                            yield m, " ".join(str(x) for x in row)
                finally:
                    lib.hyg_tg_force_threads(0, 0)
                    m.close()


def digest(rows) -> str:
    return hashlib.sha256("\n".join(rows).encode()).hexdigest()


def main() -> None:
    from hygeia_amd import _lib

    rows = [row for _, row in scan(_lib.load())]
    shapes = len({tuple(r.split()[:3]) for r in rows})
    doc = {"columns": COLUMNS, "shapes": shapes, "n_rows": len(rows), "sha256": digest(rows),
           "rows": [r for r in rows if int(r.split()[0]) in ROWS_KEPT]}
    with open(OUT, "w") as f:
        json.dump(doc, f, indent=0)
        f.write("\n")
    print(shapes, "shapes,", len(rows), "rows,", doc["sha256"])


if __name__ == "__main__":
    main()
