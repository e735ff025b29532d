"""`hygeia log_z`: log Z of a genome's tasks over a grid of model settings.

log Z is the particle filter's estimate of the log marginal likelihood of a
task's reads, the number `hygeia infer` writes to
log_normalizing_constants_optimal_{seed}.txt. The pipeline has no estimator for
--omega_case, --merge_log_prob, --split_prob and --minimum_duration; this
command evaluates log Z for every combination of the values given for them, for
every (chromosome, batch, seed) task of `hygeia infer_genome`'s inputs, in
forward-only launches (two_group.filter_chains_host: no ancestor history, no
backward simulation, no trajectories).

One multi-model launch per (--num_resampled_particles, --minimum_duration)
value, which the models of one launch must share; within it the models are
(chromosome theta) x (setting) and the chains task x seed x setting. Seeds and
chain ids are `infer`'s, so a row's log Z is, bit for bit, what `infer` writes
for that task, seed and setting.

Writes results_dir/log_z.tsv, one row per (chrom, batch, seed, M, setting), and
results_dir/log_z_summary.tsv, one row per (M, setting) with the sum over the
tasks of the log of the seeds' mean Z. Neighbouring tasks overlap in their
buffer rows, so that sum counts buffer rows twice: it is a score for comparing
settings on the same tasks, not the likelihood of the genome.

--trimmed makes the launches traced (trace="log_z": log Z_t = log p^(y_0..t)
after every site of a chain) and also writes log_z_trimmed.tsv and
log_z_trimmed_summary.tsv: a task's increment is log Z at the end of its return
range (cli.segment_index, the rows `infer` keeps) minus log Z just before it,
so every site of a chromosome is counted once. With --batches all the return
ranges tile each chromosome and the summary is the setting's estimate of the
genome's log-likelihood, each task's increment conditioned on its left buffer
only (not on the sites before it). The two other files are unchanged.

`hygeia filter_genome` (filter_genome below) writes the trace itself: per task
the filtering marginals P(split_t | y_0..t), P(regime_t | y_0..t) and log Z_t.
"""
from __future__ import annotations

import itertools
import math
import os
from typing import Sequence

import numpy as np

from . import cli

_GRID = {"omega_case": "multi_float", "merge_log_prob": "multi_float", "split_prob": "multi_float",
         "minimum_duration": "multi_int"}
# infer_genome's flags; the four settings take comma lists (their Cartesian product, in this order)
LOGZ_FLAGS = [(n, _GRID[n], [d], h + " (a comma list: the grid)") if n in _GRID else (n, k, d, h)
              for n, k, d, h in cli.GENOME_FLAGS]
COLUMNS = ("chrom", "batch", "seed", "num_resampled_particles", "minimum_duration", "omega_case", "merge_log_prob",
           "split_prob", "n_sites", "log_z")
SUMMARY_COLUMNS = ("num_resampled_particles", "minimum_duration", "omega_case", "merge_log_prob", "split_prob",
                   "n_tasks", "n_seeds", "sum_log_mean_z")
LOGZ_FLAGS.append(("trimmed", "bool", False, "also write log_z_trimmed.tsv and log_z_trimmed_summary.tsv: per task the "
                   "increment of log Z over its return range, from traced launches; with --batches all their sum "
                   "estimates the genome's log-likelihood, each increment conditioned on its task's left buffer only"))
TRIMMED_COLUMNS = COLUMNS[:-2] + ("n_trimmed_sites", "log_z_increment")
TRIMMED_SUMMARY_COLUMNS = SUMMARY_COLUMNS[:-1] + ("n_trimmed_sites", "sum_log_mean_z_increment")


def settings_of(f):
    """The grid of the flags: (omega_case, merge_log_prob, split_prob) in flag order, the last varying fastest."""
    return list(itertools.product([float(x) for x in f["omega_case"]], [float(x) for x in f["merge_log_prob"]],
                                  [float(x) for x in f["split_prob"]]))


def log_mean_exp(x: np.ndarray) -> float:
    """logsumexp(x) - log(len(x)): the log of the mean of exp(x)."""
    x = np.asarray(x, dtype=np.float64)
    m = float(x.max())
    if not math.isfinite(m):
        return m
    return m + math.log(float(np.exp(x - m).sum())) - math.log(x.shape[0])


def _field(v) -> str:
    return repr(float(v)) if isinstance(v, (float, np.floating)) else str(v)


def _write_tsv(path: str, columns, rows) -> None:
    with open(path, "w") as fh:
        fh.write("\t".join(columns) + "\n")
        for row in rows:
            fh.write("\t".join(_field(v) for v in row) + "\n")


def main(argv: Sequence[str]) -> int:
    from . import _lib, two_group

    f = cli.parse_flags(argv, LOGZ_FLAGS)
    seeds, settings = cli._seeds(f), settings_of(f)
    groups = cli._genome_groups(f)  # every chromosome read and checked before anything is written
    if not groups or not seeds:
        return 0
    mu, sigma, _ = cli._regimes(f)
    cli._use_task_device(_lib.load(import_torch=False))
    # the sites of every chromosome's tasks one after another, as infer_genome lays them out
    parts = {k: [] for k in ("mc", "tc", "mk", "tk")}
    tasks, site0, max_reads, max_len, ranges = [], 0, 0, [], []
    for g, (chrom, _, ctasks, meth_c, tot_c, meth_k, tot_k, _) in enumerate(groups):
        lo_all, hi_all = min(t[1] for t in ctasks), max(t[2] for t in ctasks)
        for k, a in (("mc", meth_c), ("tc", tot_c), ("mk", meth_k), ("tk", tot_k)):
            parts[k].append(a[lo_all:hi_all])
        max_reads = max(max_reads, int(max(tot_c[lo_all:hi_all].max(initial=0), tot_k[lo_all:hi_all].max(initial=0))))
        for (b, lo, hi, r0, r1) in ctasks:
            tasks.append((g, chrom, b, site0 + lo - lo_all, hi - lo))
            ranges.append((r0, max(r0, r1)))  # the task's return range, relative to its first row
        max_len.append(max(t[2] - t[1] for t in ctasks))
        site0 += hi_all - lo_all
    counts = {k: v[0] if len(v) == 1 else np.concatenate(v) for k, v in parts.items()}
    # chains: task x seed x setting; the model of (chromosome g, setting s) is g * len(settings) + s
    trimmed = bool(f["trimmed"])
    chains, chain_model, where, out_rows = [], [], [], 0
    for k, (g, chrom, b, begin, n) in enumerate(tasks):
        for sd in seeds:
            for s in range(len(settings)):
                chains.append((begin, n, sd, cli.chain_id(chrom, b), out_rows if trimmed else 0))
                chain_model.append(g * len(settings) + s)
                where.append((chrom, b, sd, s, n, k))
                out_rows += n
    trace = dict(trace="log_z", n_out_rows=out_rows) if trimmed else {}  # (none: the launch as it always was)
    rows, summary, trows, tsummary = [], [], [], []
    n_trimmed = sum(r1 - r0 for r0, r1 in ranges)
    for M in f["num_resampled_particles"]:
        for u in f["minimum_duration"]:
            models = []
            try:
                for g, group in enumerate(groups):
                    for (omega, merge, split) in settings:
                        # one common max_total_reads: the models of a launch share the emission table
                        models.append(two_group.CaseControlModel(
                            mu, sigma, group[1], minimum_duration=int(u), omega_case=omega, merge_log_prob=merge,
                            split_prob=split, num_resampled_ancestors=int(M),
                            num_samples_backward=int(f["num_samples_backward"]), multinomial=bool(f["multinomial"]),
                            max_total_reads=max_reads, max_duration=max_len[g] + 1))
                r = two_group.filter_chains_host({"control": counts["mc"], "case": counts["mk"]},
                                                 {"control": counts["tc"], "case": counts["tk"]}, models, chains,
                                                 chain_model=chain_model, **trace)
            finally:
                for m in models:
                    m.close()
            log_z, status = np.asarray(r["log_z"], dtype=np.float64), np.asarray(r["status"])
            inc = np.zeros(len(chains))
            for i, (chrom, b, sd, s, n, k) in enumerate(where):
                row = (chrom, b, sd, int(M), int(u)) + settings[s] + (n, float(log_z[i]))
                if status[i] != 0:
                    raise _lib.HygError(int(status[i]), "log_z: the chain of " + ", ".join(
                        f"{c}={_field(v)}" for c, v in zip(COLUMNS[:-2], row)) + " failed")
                rows.append(row)
                if trimmed:
                    (r0, r1), L = ranges[k], r["log_z_t"][chains[i][4]:chains[i][4] + n]
                    if r1 > r0:
                        inc[i] = float(L[r1 - 1]) - (float(L[r0 - 1]) if r0 > 0 else 0.0)
                    trows.append(row[:-2] + (r1 - r0, float(inc[i])))
            per = log_z.reshape(len(tasks), len(seeds), len(settings))
            per_inc = inc.reshape(per.shape)
            for s, setting in enumerate(settings):
                total = math.fsum(log_mean_exp(per[t, :, s]) for t in range(len(tasks)))
                summary.append((int(M), int(u)) + setting + (len(tasks), len(seeds), total))
                if trimmed:
                    total = math.fsum(log_mean_exp(per_inc[t, :, s]) for t in range(len(tasks)))
                    tsummary.append((int(M), int(u)) + setting + (len(tasks), len(seeds), n_trimmed, total))
    out_dir = str(f["results_dir"])
    os.makedirs(out_dir, exist_ok=True)
    _write_tsv(os.path.join(out_dir, "log_z.tsv"), COLUMNS, rows)
    _write_tsv(os.path.join(out_dir, "log_z_summary.tsv"), SUMMARY_COLUMNS, summary)
    if trimmed:
        _write_tsv(os.path.join(out_dir, "log_z_trimmed.tsv"), TRIMMED_COLUMNS, trows)
        _write_tsv(os.path.join(out_dir, "log_z_trimmed_summary.tsv"), TRIMMED_SUMMARY_COLUMNS, tsummary)
    return 0


def filter_genome(argv: Sequence[str]) -> int:
    """`hygeia filter_genome`: the filter's own per-site output for every
    (chromosome, batch, seed) task of `hygeia infer_genome`'s flags and inputs,
    from one traced multi-model forward-only launch per
    --num_resampled_particles value (two_group.filter_chains_host, trace="all":
    no ancestor history, no backward simulation). Writes, in infer_genome's task
    directories with its flags files, filter_split_probs_{N}_{seed}.npz and
    filter_regime_probs_{N}_{seed}.npz (f32: P(split_t | y_0..t), P(regime_t |
    y_0..t)), filter_log_z_{N}_{seed}.npz (f64: log p^(y_0..t)) -- every row of
    the task, buffers included, arrays as optimal_split_probs_{N}_{seed}.npz --
    and log_normalizing_constants_optimal_{seed}.txt as `infer` writes it."""
    from . import _lib, two_group

    f = cli.parse_flags(argv, cli.GENOME_FLAGS)
    seeds = cli._seeds(f)
    groups = cli._genome_groups(f)  # every chromosome read and checked before anything is written
    if not groups or not seeds:
        return 0
    mu, sigma, K = cli._regimes(f)
    cli._use_task_device(_lib.load(import_torch=False))
    parts = {k: [] for k in ("mc", "tc", "mk", "tk")}
    chains, chain_model, where, out, site0, max_reads, max_len = [], [], [], 0, 0, 0, []
    for g, (chrom, _, tasks, meth_c, tot_c, meth_k, tot_k, _) in enumerate(groups):
        lo_all, hi_all = min(t[1] for t in tasks), max(t[2] for t in tasks)
        for k, a in (("mc", meth_c), ("tc", tot_c), ("mk", meth_k), ("tk", tot_k)):
            parts[k].append(a[lo_all:hi_all])
        max_reads = max(max_reads, int(max(tot_c[lo_all:hi_all].max(initial=0), tot_k[lo_all:hi_all].max(initial=0))))
        for (b, lo, hi, _, _) in tasks:
            for sd in seeds:
                chains.append((site0 + lo - lo_all, hi - lo, sd, cli.chain_id(chrom, b), out))
                chain_model.append(g)
                where.append((chrom, b, sd))
                out += hi - lo
        max_len.append(max(t[2] - t[1] for t in tasks))
        site0 += hi_all - lo_all
    counts = {k: v[0] if len(v) == 1 else np.concatenate(v) for k, v in parts.items()}
    results = []
    for M in f["num_resampled_particles"]:
        models = two_group.genome_models([g[1] for g in groups], mu, sigma, max_reads, [n + 1 for n in max_len],
                                         **cli._model_kw(f, M))
        try:
            r = two_group.filter_chains_host({"control": counts["mc"], "case": counts["mk"]},
                                             {"control": counts["tc"], "case": counts["tk"]}, models, chains,
                                             chain_model=chain_model, trace="all", n_out_rows=out)
        finally:
            for model in models:
                model.close()
        status = np.asarray(r["status"])
        if (status != 0).any():
            i = int(np.nonzero(status)[0][0])
            raise _lib.HygError(int(status[i]), "filter_genome: the chain of chrom={}, batch={}, seed={}, "
                                "num_resampled_particles={} failed".format(*where[i], int(M)))
        results.append((int(M) * (2 * K + K * K), r))
    log_z = {}
    for i, (chrom, b, sd) in enumerate(where):
        path = cli._task_dir(f, chrom, b)
        os.makedirs(path, exist_ok=True)
        with open(os.path.join(path, f"flags{sd}.txt"), "w") as fh:
            fh.write(cli.serialize_flags(dict(f, chrom=chrom, batch=b, seed=sd)))  # of that task's `hygeia infer`
        rows = slice(chains[i][4], chains[i][4] + chains[i][1])
        for N, r in results:
            for name, key in (("filter_split_probs", "split_probs"), ("filter_regime_probs", "regime_probs"),
                              ("filter_log_z", "log_z_t")):
                np.savez_compressed(os.path.join(path, f"{name}_{N}_{sd}"), r[key][rows])
            log_z.setdefault((path, sd), {})[N] = float(r["log_z"][i])
    for (path, sd), v in log_z.items():
        with open(os.path.join(path, f"log_normalizing_constants_optimal_{sd}.txt"), "w") as fh:
            print(v, file=fh)
    return 0
