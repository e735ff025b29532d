"""`hygeia infer`, `infer_many` and `infer_genome` end to end without a GPU:
the two launch functions they call are deterministic fakes (tests/cli_trees.py),
everything else is the commands' own code. Over two chromosomes (2 400 and
1 300 sites, segments of 1 000, two particle counts, seeds 0 and 5) the three
commands write the same 165 files, and files, messages, launches and error
behaviour equal tests/golden/cli_trees_parent.json, recorded by
tests/golden/make_cli_trees.py before the commands were put on one task driver.
"""
import json
import os
import sys
import zlib

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cli_trees  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cli_trees_parent.json")
DIRS = {"chrom_21_0", "chrom_21_1", "chrom_21_2", "chrom_X_0", "chrom_X_1"}
N_VALUES = {12 * 48, 20 * 48}  # M (2K + K^2) at K = 6: 576 and 960


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    with pytest.MonkeyPatch.context() as mp:
        yield cli_trees.collect(str(tmp_path_factory.mktemp("cli_trees")), mp)


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as fh:
        return json.load(fh)


def test_the_three_commands_write_the_same_tree(runs, golden):
    trees = {c: cli_trees.digests(runs[c]["tree"]) for c in ("infer", "infer_many", "infer_genome")}
    for c, r in runs.items():
        if c in trees:
            assert r["rc"] == [0] * len(r["rc"]) and r["error"] is None and r["stderr"] == "", c
            assert len(r["tree"]) == 165 and {os.path.dirname(k) for k in r["tree"]} == DIRS, c
            assert len(trees[c]) == 165 - 2 * 10  # two time files per (batch, seed) task
    assert trees["infer"] == trees["infer_many"] == trees["infer_genome"]
    for c in trees:  # (the golden holds the one tree under "infer")
        assert trees[c] == golden["infer"]["tree"], c
    # --chroms 21 alone: chromosome 21's files of the whole genome's run
    alone = cli_trees.digests(runs["infer_genome_21"]["tree"])
    assert alone == {k: v for k, v in golden["infer"]["tree"].items() if k.startswith("chrom_21_")}
    assert len(alone) == 87


def test_time_files_and_the_pro_rata_rule(runs):
    for c in ("infer", "infer_many", "infer_genome", "infer_genome_21"):
        t = cli_trees.times(runs[c]["tree"])
        assert len(t) == (12 if c == "infer_genome_21" else 20), c
        for k, v in t.items():
            if os.path.basename(k).startswith("optimal_time_backward_"):
                assert v == {}, (c, k)
            else:
                assert set(v) == N_VALUES and all(isinstance(x, float) and x >= 0 for x in v.values()), (c, k)
    # within one launch, a task's time over its n_sites is the same for every task
    chroms = {zlib.crc32(c.encode()): c for c, _ in cli_trees.CHROMS}
    for c in ("infer_many", "infer_genome", "infer_genome_21"):
        t = cli_trees.times(runs[c]["tree"])
        launches = [x for x in runs[c]["calls"] if x[0] == "run_chains_host"]
        per_m = len(N_VALUES)
        for j, (_, _, _, chains, _) in enumerate(launches):  # infer_many: chromosome 21's two launches, then X's
            N = sorted(N_VALUES)[j % per_m]
            rate = [t[os.path.join(f"chrom_{chroms[cid >> 32]}_{cid & 0xFFFFFFFF}", f"optimal_time_{seed}.txt")][N] / n
                    for (_, n, seed, cid, _) in chains]
            assert rate == pytest.approx([rate[0]] * len(rate), rel=1e-12), (c, j)


def test_stdout_and_stderr_are_the_parents(runs, golden):
    for c, r in runs.items():
        assert r["stdout"] == golden[c]["stdout"], c
        assert r["stderr"] == golden[c]["stderr"], c
        assert r["rc"] == golden[c]["rc"], c
    assert runs["infer"]["stdout"].startswith("specified flags:\n--mu=")
    assert runs["infer"]["stdout"].count("\n12\n20\n") == 10
    assert runs["infer_many"]["stdout"] == runs["infer_genome"]["stdout"] * 2 == "12\n20\n" * 2
    assert runs["msg_infer"]["stdout"].endswith("\nBatch index is too large for the chromosome\n")
    assert runs["msg_infer"]["rc"] == [0] and runs["msg_infer"]["wrote"] == ["res"]
    assert sorted(runs["msg_infer"]["tree"]) == ["chrom_21_7/flags0.txt"]  # written before the data is read
    assert runs["msg_infer_many"]["stdout"] == "Batch index is too large for the chromosome (batch 7)\n12\n20\n"
    assert runs["msg_infer_genome"]["stdout"] == \
        "Batch index is too large for the chromosome (chromosome 21, batch 7)\n" \
        "Batch index is too large for the chromosome (chromosome X, batch 7)\n12\n20\n"
    for c in ("msg_infer", "msg_infer_many", "msg_infer_genome"):
        assert cli_trees.digests(runs[c]["tree"]) == golden[c]["tree"], c


def test_recorded_launches(runs, golden):
    for c, r in runs.items():
        assert json.loads(json.dumps(r["calls"])) == golden[c]["calls"], c
    assert [x[0] for x in runs["infer"]["calls"]] == ["run"] * 20  # ten tasks, two particle counts
    many = runs["infer_many"]["calls"]
    # one CaseControlModel and no index: the single-model entry; a launch per particle count and chromosome
    assert [(x[0], x[1], x[2], x[4]) for x in many] == [("run_chains_host", 6, False, None)] * 2 + \
        [("run_chains_host", 4, False, None)] * 2
    genome = runs["infer_genome"]["calls"]
    assert [(x[0], x[1], x[2], x[4]) for x in genome] == [("run_chains_host", 10, True, [0] * 6 + [1] * 4)] * 2
    assert genome[0][3] == genome[1][3]
    alone = runs["infer_genome_21"]["calls"]
    assert [(x[0], x[1], x[2], x[4]) for x in alone] == [("run_chains_host", 6, True, [0] * 6)] * 2
    assert alone[0][3] == many[0][3]  # the chains of infer_many --chrom 21


def test_last_timings_keys(runs, golden):
    for c, r in runs.items():
        assert r["timings"] == golden[c]["timings"], c
    assert runs["infer"]["timings"] == [["chains", "device", "parse", "writes"]] * 10
    assert runs["infer_many"]["timings"] == [["chains", "device", "parse", "writes"]] * 2
    assert runs["infer_genome"]["timings"] == [["chains", "device", "parse", "writes"]]


def test_error_behaviour(runs, golden):
    for c in ("bad_infer", "bad_infer_many", "bad_infer_genome", "missing_theta"):
        r = runs[c]
        assert (r["error"], r["wrote"]) == (golden[c]["error"], golden[c]["wrote"]), c
        assert cli_trees.digests(r["tree"]) == golden[c]["tree"] and r["calls"] == [], c
    for c in ("bad_infer", "bad_infer_many"):
        assert runs[c]["error"] == "AssertionError: methylated reads exceed total reads" and runs[c]["rc"] == []
    assert runs["bad_infer_many"]["wrote"] == []
    r = runs["bad_infer_genome"]
    assert r["error"] is None and r["rc"] == [1] and r["wrote"] == []
    assert r["stderr"] == "hygeia infer_genome: chromosome 21: methylated reads exceed total reads\n"
    r = runs["missing_theta"]
    assert r["rc"] == [1] and r["wrote"] == [] and r["stderr"].startswith("hygeia infer_genome: chromosome X: ")
