"""`hygeia estimate_genome` on the GPU: three small chromosomes (400, 250 and
61 rows, 2 samples, an update every 50 steps) in one launch write, per
chromosome, the files of `hygeia estimate_parameters_and_regimes` run alone
with that chromosome's files, parameters and seed, byte for byte (_tree: a
.gz file is its decompressed bytes, the container carries the time it was
written); the --parameters_dir form (the single-group pipeline's step 3); and
`hygeia infer_genome` reads the theta files it wrote.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from cli_trees import _tree, _write_chrom  # noqa: E402

pytestmark = pytest.mark.gpu

CHROMS = (("3", 400, 5), ("11", 250, 6), ("X", 61, 7))  # name, rows, rng seed
COMMON = ["--n_steps_without_parameter_update", "50", "--u", "3", "--randomise_rng_seed", "FALSE",
          "--estimate_regime_probabilities"]
STEMS = ("regimes", "theta_trace", "p", "kappa", "omega", "theta")


def _single_paths(out_dir, chrom):
    j = lambda stem: os.path.join(out_dir, f"{stem}_{chrom}.csv.gz")  # noqa: E731
    return ["--regime_probabilities_csv_file", j("regimes"), "--theta_trace_csv_file", j("theta_trace"),
            "--p_csv_file", j("p"), "--kappa_csv_file", j("kappa"), "--omega_csv_file", j("omega"),
            "--theta_file", j("theta")]


def _single_inputs(data, chrom):
    j = lambda stem: os.path.join(data, f"{stem}_{chrom}.txt.gz")  # noqa: E731
    return ["--genomic_positions_csv_file", j("positions"), "--n_total_reads_csv_file", j("n_total_reads_control"),
            "--n_methylated_reads_csv_file", j("n_methylated_reads_control")]


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """The first run (with estimation), shared: the genome command's tree and
    the three single commands' tree."""
    from hygeia_amd import _lib, cli

    if _lib.load().hyg_device_count() <= 0:
        pytest.fail("no HIP device visible: the GPU tests must run on an MI355X")
    root = tmp_path_factory.mktemp("estimate_genome")
    for k, (chrom, rows, _) in enumerate(CHROMS):
        _write_chrom(str(root), chrom, rows, k)
    data = str(root / "data")
    genome, single = str(root / "genome"), str(root / "single")
    rc = cli.main(["estimate_genome", "--data_dir", data, "--output_dir", genome, "--estimate_parameters",
                   "--rng_seed", "5,6,7"] + COMMON)
    assert rc == 0
    os.makedirs(single)
    for chrom, _, seed in CHROMS:
        assert cli.main(["estimate_parameters_and_regimes", "--estimate_parameters", "--rng_seed", str(seed)] + COMMON +
                        _single_inputs(data, chrom) + _single_paths(single, chrom)) == 0
    return {"root": root, "data": data, "genome": genome, "single": single}


def test_with_estimation_writes_the_single_commands_files(runs):
    th0 = [np.random.default_rng(seed).standard_normal(36) for _, _, seed in CHROMS]
    assert not np.array_equal(th0[0], th0[1]) and not np.array_equal(th0[1], th0[2])
    genome, single = _tree(runs["genome"]), _tree(runs["single"])
    assert genome.pop("rng_seeds.csv") == b"chrom,rng_seed\n3,5\n11,6\nX,7\n"  # --chroms all: 3, 11, X
    assert sorted(genome) == sorted(single) == sorted(f"{s}_{c}.csv.gz" for s in STEMS for c, _, _ in CHROMS)
    for k in single:
        assert genome[k] == single[k], k
    # each chromosome ran from its own theta_0 (the trace's first row), and theta moved
    first = [genome[f"theta_trace_{c}.csv.gz"].split(b"\n")[1] for c, _, _ in CHROMS]
    assert len(set(first)) == 3
    rows = genome["theta_trace_3.csv.gz"].split(b"\n")
    assert len(rows) == 1 + 399 + 1 and rows[1] != rows[399]


def test_with_parameters_dir_equals_single_runs_with_input_files(runs, tmp_path):
    from hygeia_amd import cli

    genome, single = str(tmp_path / "genome"), str(tmp_path / "single")
    par = runs["genome"]
    assert cli.main(["estimate_genome", "--data_dir", runs["data"], "--output_dir", genome, "--parameters_dir", par,
                     "--chroms", "X,3,11", "--rng_seed", "9"] + COMMON) == 0
    os.makedirs(single)
    for chrom, _, _ in CHROMS:
        j = lambda stem: os.path.join(par, f"{stem}_{chrom}.csv.gz")  # noqa: E731
        assert cli.main(["estimate_parameters_and_regimes", "--rng_seed", "9", "--p_input_csv_file", j("p"),
                         "--kappa_input_csv_file", j("kappa"), "--omega_input_csv_file", j("omega")] + COMMON +
                        _single_inputs(runs["data"], chrom) + _single_paths(single, chrom)) == 0
    g, s = _tree(genome), _tree(single)
    assert g.pop("rng_seeds.csv") == b"chrom,rng_seed\nX,9\n3,9\n11,9\n"
    assert sorted(g) == sorted(s) == sorted(f"regimes_{c}.csv.gz" for c, _, _ in CHROMS)
    for k in s:
        assert g[k] == s[k], k
    # the chromosomes' parameters differ, and they matter: chromosome 3 under the flag defaults gives other regimes
    assert cli.main(["estimate_genome", "--data_dir", runs["data"], "--output_dir", str(tmp_path / "flags"),
                     "--chroms", "3", "--rng_seed", "9"] + COMMON) == 0
    assert _tree(str(tmp_path / "flags"))["regimes_3.csv.gz"] != g["regimes_3.csv.gz"]


def test_infer_genome_reads_the_theta_files(runs, tmp_path, monkeypatch):
    from hygeia_amd import cli

    monkeypatch.chdir(tmp_path)
    assert cli.main(["infer_genome", "--chroms", "all", "--data_dir", runs["data"], "--single_group_dir",
                     runs["genome"], "--results_dir", "res", "--num_samples_backward", "7"]) == 0
    assert sorted(os.listdir(tmp_path / "res")) == ["chrom_11_0", "chrom_3_0", "chrom_X_0"]
