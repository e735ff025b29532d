"""Shared by tests/test_cli_trees_cpu.py, tests/golden/make_cli_trees.py and
tests/test_gpu_tg_multi.py: the input writer of the infer_genome tests, the
normalised view of a results tree, and deterministic fakes of the two launch
functions the `hygeia infer*` commands call, with which the three commands run
end to end without a GPU (collect)."""
import ast
import contextlib
import gzip
import hashlib
import io
import os
import zlib

import numpy as np


def _theta(K, k):
    """Model k's theta: the uniform one moved by N(0, 1) per entry (transition
    log-weights and omega logits alike), far more than any rounding."""
    from hygeia_amd import two_group

    rng = np.random.default_rng(7000 + 13 * K + k)
    return two_group.uniform_theta(K, 0.8) + rng.normal(0.0, 1.0, K * K)


def _write_chrom(root, chrom, T, k, K=6, S=2):
    """One chromosome's input files: counts and positions under root/data, its
    own theta under root/sg."""
    from hygeia_amd import synthetic as syn

    data = syn.simulate(T, S, S, K=K, seed=60 + k, coverage=30.0)
    os.makedirs(os.path.join(root, "data"), exist_ok=True)
    os.makedirs(os.path.join(root, "sg"), exist_ok=True)
    np.savetxt(os.path.join(root, "data", f"positions_{chrom}.txt.gz"), syn.positions(T, 60 + k).astype(np.float64),
               fmt="%s")
    for g in ("control", "case"):
        np.savetxt(os.path.join(root, "data", f"n_total_reads_{g}_{chrom}.txt.gz"),
                   data[f"tot_{g}"].astype(np.float64), fmt="%s", delimiter=",")
        np.savetxt(os.path.join(root, "data", f"n_methylated_reads_{g}_{chrom}.txt.gz"),
                   data[f"meth_{g}"].astype(np.float64), fmt="%s", delimiter=",")
    with gzip.open(os.path.join(root, "sg", f"theta_{chrom}.csv.gz"), "wt") as fh:
        fh.write("data\n" + "\n".join(repr(float(x)) for x in _theta(K, 20 + k)) + "\n")


def _tree(root):
    """Every file under root -> its content, byte for byte. The gzip and zip
    containers carry the time they were written, so a .gz file is its
    decompressed bytes and an .npz its members' names, dtypes, shapes and bytes."""
    out = {}
    for dirpath, _, files in os.walk(root):
        for name in files:
            p = os.path.join(dirpath, name)
            if name.endswith(".npz"):
                with np.load(p) as z:
                    content = [(k, str(z[k].dtype), z[k].shape, z[k].tobytes()) for k in sorted(z.files)]
            elif name.endswith(".gz"):
                with gzip.open(p, "rb") as fh:
                    content = fh.read()
            else:
                with open(p, "rb") as fh:
                    content = fh.read()
            out[os.path.relpath(p, root)] = content
    return out


def is_time_file(relpath):
    return os.path.basename(relpath).startswith("optimal_time_")


def digests(tree):
    """relative path -> sha256 of the _tree content, the optimal_time_* files
    (wall-clock times) left out."""
    out = {}
    for k in sorted(tree):
        if is_time_file(k):
            continue
        h = hashlib.sha256()
        if isinstance(tree[k], bytes):
            h.update(tree[k])
        else:
            for name, dtype, shape, raw in tree[k]:
                h.update(f"{name}|{dtype}|{tuple(shape)}|".encode())
                h.update(raw)
        out[k] = h.hexdigest()
    return out


def times(tree):
    """relative path -> the dict an optimal_time_* file holds."""
    return {k: ast.literal_eval(v.decode()) for k, v in tree.items() if is_time_file(k)}


# ------------------------------------------------------------------- fakes
def _rows(tc, tk, seed, chain_id, model):
    """A chain's fake outputs: a function of its own total-read rows, its seed,
    its chain id and its model's parameters, so that a result that reaches the
    wrong task, or runs under the wrong chromosome's model, shows."""
    K, B = model.n_regimes, model.num_samples_backward
    crc = zlib.crc32(bytes(model.params))
    tc, tk = (np.asarray(a).reshape(len(a), -1).astype(np.int64) for a in (tc, tk))
    v = (tc.sum(1) + 3 * tk.sum(1) + 7 * int(seed) + (int(chain_id) & 0xFFFF) + (int(chain_id) >> 32) % 997
         + crc % 1009) % 1000
    merged = (v[:, None] + np.arange(B)[None, :]).astype(np.int16)
    control = np.stack([merged, merged + 1], axis=2)
    split = (v / 1000.0).astype(np.float32)
    regime = (split[:, None] + np.arange(2 * K, dtype=np.float32)[None, :]).astype(np.float32)
    return dict(merged=merged, control=control, case=control + 2, split_probs=split, regime_probs=regime,
                log_z=float(v.sum()) + crc % 1009)


class Fakes:
    """two_group.run and two_group.run_chains_host without a device. `calls`
    records every launch: ("run", seed, chain_id, n_sites) or ("run_chains_host",
    n_chains, whether it was given a model list, chain tuples, chain_model)."""

    def __init__(self):
        self.calls = []

    def run(self, observations, n_total_reads, model, seed, chain_id=0):
        from hygeia_amd import two_group

        assert isinstance(model, two_group.CaseControlModel)
        r = _rows(n_total_reads["control"], n_total_reads["case"], seed, chain_id, model)
        T = len(r["merged"])
        self.calls.append(("run", int(seed), int(chain_id), T))
        res = two_group.BackwardSimulationResults(step=np.arange(T), particle={
            "merged_state": r["merged"], "control_state": r["control"], "case_state": r["case"]})
        return res, None, {k: r[k] for k in ("split_probs", "regime_probs", "log_z")}

    def run_chains_host(self, observations, n_total_reads, model, chains, n_out_rows, final_weights=False,
                        chain_model=None):
        from hygeia_amd import two_group

        is_list = not isinstance(model, two_group.CaseControlModel)
        models = list(model) if is_list else [model]
        assert (chain_model is not None) == is_list
        idx = [int(k) for k in chain_model] if is_list else [0] * len(chains)
        self.calls.append(("run_chains_host", len(chains), is_list, [tuple(int(x) for x in c) for c in chains],
                           idx if is_list else None))
        K, B, R, n = models[0].n_regimes, models[0].num_samples_backward, int(n_out_rows), len(chains)
        out = {"merged": np.full((R, B), -1, np.int16), "control": np.full((R, B, 2), -1, np.int16),
               "case": np.full((R, B, 2), -1, np.int16), "split_probs": np.full(R, -1, np.float32),
               "regime_probs": np.full((R, 2 * K), -1, np.float32), "log_z": np.zeros(n, np.float64),
               "status": np.zeros(n, np.int32)}
        for i, (s0, T, seed, cid, o0) in enumerate(chains):
            r = _rows(n_total_reads["control"][s0:s0 + T], n_total_reads["case"][s0:s0 + T], seed, cid, models[idx[i]])
            for k in ("merged", "control", "case", "split_probs", "regime_probs"):
                out[k][o0:o0 + T] = r[k]
            out["log_z"][i] = r["log_z"]
        return out


# ----------------------------------------------------------------- the runs
COMMON = ["--segment_size", "1000", "--buffer_size", "50", "--num_samples_backward", "7",
          "--num_resampled_particles", "12", "--num_resampled_particles", "20", "--results_dir", "res"]
SEEDS = (0, 5)
CHROMS = (("21", 2400), ("X", 1300))  # batches 0-2 and 0-1 at --segment_size 1000
BAD_SITE = 1500  # of chromosome 21 (batch 1): one more methylated read than total reads


def write_inputs(root):
    """root/data, root/sg: the two chromosomes; root/data_bad: the same with one
    methylated > total site; root/sg_missing: without theta_X."""
    for k, (chrom, T) in enumerate(CHROMS):
        _write_chrom(root, chrom, T, k)
    os.makedirs(os.path.join(root, "data_bad"))
    os.makedirs(os.path.join(root, "sg_missing"))
    for name in os.listdir(os.path.join(root, "data")):
        with gzip.open(os.path.join(root, "data", name), "rb") as fh:
            raw = fh.read()
        if name == "n_methylated_reads_control_21.txt.gz":
            meth = np.loadtxt(io.BytesIO(raw), delimiter=",", ndmin=2)
            tot = np.loadtxt(os.path.join(root, "data", "n_total_reads_control_21.txt.gz"), delimiter=",", ndmin=2)
            meth[BAD_SITE, 0] = tot[BAD_SITE, 0] + 1
            np.savetxt(os.path.join(root, "data_bad", name), meth, fmt="%s", delimiter=",")
        else:
            with gzip.open(os.path.join(root, "data_bad", name), "wb") as fh:
                fh.write(raw)
    with open(os.path.join(root, "sg", "theta_21.csv.gz"), "rb") as src, \
            open(os.path.join(root, "sg_missing", "theta_21.csv.gz"), "wb") as dst:
        dst.write(src.read())


def collect(root, mp):
    """Writes the inputs under root and runs every command of the pinned set,
    each from a directory of its own under root (paths in the flags files and
    the messages are relative, so they do not name the machine). mp: a
    pytest.MonkeyPatch. Returns {run name: dict(rc, stdout, stderr, error,
    tree, wrote, calls, timings)}; a run of several commands (the ten `hygeia infer`
    tasks, infer_many per chromosome) holds their outputs one after another."""
    from hygeia_amd import cli, two_group

    write_inputs(root)
    mp.setenv("HYGEIA_SERVER", "0")
    mp.setenv("HYGEIA_PARSE_CACHE", "0")
    mp.delenv("HYGEIA_TASK_TIMING", raising=False)
    fakes = Fakes()
    mp.setattr(two_group, "run", fakes.run)
    mp.setattr(two_group, "run_chains_host", fakes.run_chains_host)
    seeds = ",".join(str(s) for s in SEEDS)

    def run(name, commands, data="data", sg="sg"):
        os.makedirs(os.path.join(root, name))
        mp.chdir(os.path.join(root, name))
        fakes.calls = []
        r = dict(rc=[], error=None, timings=[])
        out, err = io.StringIO(), io.StringIO()
        with contextlib.redirect_stdout(out), contextlib.redirect_stderr(err):
            for argv in commands:
                try:
                    r["rc"].append(cli.main(argv + COMMON + ["--data_dir", f"../{data}", "--single_group_dir",
                                                             f"../{sg}"]))
                except AssertionError as e:
                    r["error"] = f"{type(e).__name__}: {e}"
                r["timings"].append(sorted(cli.LAST_TIMINGS))
        r.update(stdout=out.getvalue(), stderr=err.getvalue(), calls=fakes.calls,
                 wrote=sorted(os.listdir(os.path.join(root, name))), tree=_tree(os.path.join(root, name, "res")))
        return r

    tasks = [(c, b, s) for c, T in CHROMS for b in range(T // 1000 + 1) for s in SEEDS]
    runs = {
        "infer": run("infer", [["infer", "--chrom", c, "--batch", str(b), "--seed", str(s)] for c, b, s in tasks]),
        "infer_many": run("infer_many", [["infer_many", "--chrom", c, "--seeds", seeds] for c, _ in CHROMS]),
        "infer_genome": run("infer_genome", [["infer_genome", "--chroms", "all", "--seeds", seeds]]),
        "infer_genome_21": run("infer_genome_21", [["infer_genome", "--chroms", "21", "--seeds", seeds]]),
        # the three wordings of the too-large message
        "msg_infer": run("msg_infer", [["infer", "--chrom", "21", "--batch", "7"]]),
        "msg_infer_many": run("msg_infer_many", [["infer_many", "--chrom", "21", "--batches", "0,7"]]),
        "msg_infer_genome": run("msg_infer_genome", [["infer_genome", "--chroms", "all", "--batches", "0,7"]]),
        # a site with more methylated than total reads; a missing theta file
        "bad_infer": run("bad_infer", [["infer", "--chrom", "21", "--batch", "1"]], data="data_bad"),
        "bad_infer_many": run("bad_infer_many", [["infer_many", "--chrom", "21"]], data="data_bad"),
        "bad_infer_genome": run("bad_infer_genome", [["infer_genome", "--chroms", "all"]], data="data_bad"),
        "missing_theta": run("missing_theta", [["infer_genome", "--chroms", "21,X"]], sg="sg_missing"),
    }
    return runs


def golden_doc(runs):
    """What tests/golden/cli_trees_parent.json holds of collect()'s runs:
    digests and short strings. The trees of the batched commands are those of
    the `infer` run (the test asserts it), so they are held once."""
    doc = {name: dict(rc=r["rc"], error=r["error"], stdout=r["stdout"], stderr=r["stderr"], timings=r["timings"],
                      calls=[list(c) for c in r["calls"]], wrote=r["wrote"], tree=digests(r["tree"]))
           for name, r in runs.items()}
    for name in ("infer_many", "infer_genome"):
        assert doc[name].pop("tree") == doc["infer"]["tree"]
    assert doc["infer_genome_21"].pop("tree") == {k: v for k, v in doc["infer"]["tree"].items()
                                                  if k.startswith("chrom_21_")}
    return doc
