"""`hygeia fit_genome`: omega_case, merge_log_prob and split_prob fitted from
the joint trajectories by Monte-Carlo EM.

A full launch (hyg_tg_run_chains) leaves B x seeds joint draws of the whole
latent path per task in HBM. Under the model's own transition law
(case_control_regime_model.py:80-87, case_control_distributions.py:246-291)
the three settings enter the complete-data likelihood of a path only through a
handful of integer counts:

  table[m(x)][m(y)]   over the transitions x -> y whose ancestor may switch its
                      merged state (min(d_c(x), d_k(x)) >= minimum_duration):
                      split_prob is the rate of 1 -> 0, exp(merge_log_prob)
                      that of 0 -> 1;
  trials[j], events[j] over the transitions whose case part is scored by the
                      hazard rho_case(d_k(x)) (the fourth branch): how often it
                      could fire at the case duration j and how often it did.

The E-step is the launch `infer_genome` already runs, the statistics are one
streaming pass over its outputs (hyg_tg_transition_stats, em_kernels.hip), the
M-step (m_step) is two ratios and a 1-D maximisation.

What this is not: the launches are particle approximations and neighbouring
tasks overlap in their buffers, so fit_trace.tsv's log Z sum is a diagnostic
and not a likelihood that must rise; the control side's theta comes from the
single-group step and is not refitted; minimum_duration is not fitted (compare
its values with `hygeia log_z`); durations are read modulo 2^16 as the outputs
store them. There is no CPU path for the statistics: without the HIP library
or a GPU transition_stats raises. rho_case and m_step need numpy alone.
"""
from __future__ import annotations

import math
import os
from typing import Callable, Dict, Sequence, Tuple

import numpy as np

from . import _lib

SETTINGS = ("omega_case", "merge_log_prob", "split_prob")
MAX_DCAP = 4096  # kEmMaxDcap (em_common.h)
_OMEGA_LO, _OMEGA_HI = 1e-3, 1.0 - 1e-3  # the search interval inside (0, 1): a mean case sojourn of up to 2 000 sites


def stats_len(dcap: int) -> int:
    return 4 + 2 * (int(dcap) + 1)


def split_stats(stats: np.ndarray, dcap: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """hyg_tg_transition_stats' vector as (table [2][2], trials [dcap + 1], events [dcap + 1]), int64."""
    s = np.asarray(stats, dtype=np.int64).reshape(-1)
    if s.shape[0] != stats_len(dcap):
        raise ValueError(f"{s.shape[0]} statistics, expected {stats_len(dcap)} for dcap = {dcap}")
    n = int(dcap) + 1
    return s[:4].reshape(2, 2).copy(), s[4:4 + n].copy(), s[4 + n:].copy()


def transition_stats(merged, control, kase, B: int, groups: Sequence[Tuple[int, int]],
                     block_rows: Sequence[Sequence[int]], n_sites: int, minimum_duration: int, dcap: int = 1024,
                     stats=None, stream=None):
    """The transition statistics of the trajectories merged [rows][B], control
    / kase [rows][B][2] int16 (device tensors, hyg_tg_outputs layout), groups
    and block_rows as changepoints.site_events (sorted by site, disjoint).
    stats: a device int64 tensor [4 + 2 (dcap + 1)] that the call adds to (a
    genome is a sum over chromosomes), zeros when None. Returns (table [2][2],
    trials, events) of stats after the call, numpy int64."""
    from .changepoints import _check_trajectories, _groups_args
    from .dmp import _torch
    from .dmr import _sp

    torch = _torch()
    if merged is None or control is None or kase is None:
        raise ValueError("merged, control and kase are all needed")
    dev = _check_trajectories(torch, (merged, control, kase))
    if stats is None:
        stats = torch.zeros(stats_len(dcap), dtype=torch.int64, device=dev)
    elif stats.dtype != torch.int64 or not stats.is_contiguous() or stats.device != dev or \
            stats.numel() != stats_len(dcap):
        raise ValueError(f"stats must be a contiguous int64 tensor of {stats_len(dcap)} entries on the trajectories' "
                         "device")
    g_arr, br, br_p, n_groups, n_seeds = _groups_args(groups, block_rows)
    _lib.check(_lib.load().hyg_tg_transition_stats(
        merged.data_ptr(), control.data_ptr(), kase.data_ptr(), int(B), g_arr, br_p, n_groups, n_seeds, int(n_sites),
        int(minimum_duration), int(dcap), stats.data_ptr(), _sp(stream, dev)))
    return split_stats(stats.cpu().numpy(), dcap)


# ------------------------------------------------------------------ hazard
def rho_case(d, omega: float, kappa: float, u: int) -> np.ndarray:
    """The case hazard rho(d) of case_control_regime_model.py:111-168 in
    float64: with X ~ NegativeBinomial(total_count = kappa, probs = omega), pmf
    C(x + kappa - 1, x) (1 - omega)^kappa omega^x, rho(d) = pmf(d - u) /
    P(X >= d - u); 0 below u; the survival is 1 at d == u; 0.1 where the ratio
    is not finite. The survival is the tail sum of the pmf, formed in log space
    (never 1 - cdf), so it neither cancels nor underflows; the reference holds
    the cdf in float32 and falls to 0.1 once that rounds to 1."""
    d = np.asarray(d, dtype=np.int64)
    omega, kappa, u = float(omega), float(kappa), int(u)
    out = np.zeros(d.shape, dtype=np.float64)
    at = d >= u
    if not at.any():
        return out
    if not (0.0 < omega < 1.0) or not kappa > 0.0:
        out[at] = 0.1
        return out
    x_max = int(d.max()) - u
    # the terms past x_max until the rest of the tail is below e^-50 of the last one kept
    n = x_max + 1 + min(int(math.ceil(50.0 / -math.log(omega))) + 64, 4_000_000)
    x = np.arange(n, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        # log pmf(x) = kappa log(1 - omega) + sum_{y < x} log(omega (y + kappa) / (y + 1))
        steps = math.log(omega) + np.log(x[:-1] + kappa) - np.log(x[:-1] + 1.0)
        log_pmf = kappa * math.log1p(-omega) + np.concatenate([[0.0], np.cumsum(steps)])
        log_tail = np.logaddexp.accumulate(log_pmf[::-1])[::-1]  # log P(X >= x)
        log_tail[0] = 0.0
        h = np.exp(log_pmf[:x_max + 1] - log_tail[:x_max + 1])
    h = np.where(np.isfinite(h), h, 0.1)
    out[at] = h[d[at] - u]
    return out


def q_omega(trials, events, omega: float, kappa: float, u: int, rho: Callable = rho_case) -> float:
    """Q(omega) = sum_j events[j] log rho(j) + (trials[j] - events[j]) log(1 -
    rho(j)) over the bins with trials[j] > 0; a term whose count is zero is
    dropped before its log is taken. -inf where a counted term has probability
    0 (or rho leaves [0, 1])."""
    trials, events = np.asarray(trials, dtype=np.float64), np.asarray(events, dtype=np.float64)
    j = np.flatnonzero(trials > 0)
    if j.size == 0:
        return 0.0
    r = np.asarray(rho(j, omega, kappa, u), dtype=np.float64)
    ev, no = events[j], trials[j] - events[j]
    with np.errstate(divide="ignore", invalid="ignore"):
        a = np.where(ev > 0, ev * np.log(np.where(ev > 0, r, 1.0)), 0.0)
        b = np.where(no > 0, no * np.log(np.where(no > 0, 1.0 - r, 1.0)), 0.0)
    q = float(math.fsum(a) + math.fsum(b)) if np.all(np.isfinite(a)) and np.all(np.isfinite(b)) else -math.inf
    return q if not math.isnan(q) else -math.inf


def _maximise(fn: Callable[[float], float], lo: float, hi: float, start: float) -> Tuple[float, float]:
    """A bracketed search for the maximiser of fn over [lo, hi]: the best point
    of a logit-spaced grid (and `start`) brackets it between its neighbours,
    golden section narrows the bracket. Returns (argument, value) of the best
    point seen."""
    logit = np.linspace(math.log(lo / (1.0 - lo)), math.log(hi / (1.0 - hi)), 41)
    pts = sorted(set([lo, hi] + [float(1.0 / (1.0 + math.exp(-z))) for z in logit[1:-1]] +
                     ([start] if lo <= start <= hi else [])))
    vals = [fn(p) for p in pts]
    i = int(np.argmax(vals))
    best = (pts[i], vals[i])
    a, b = pts[max(i - 1, 0)], pts[min(i + 1, len(pts) - 1)]
    g = (math.sqrt(5.0) - 1.0) / 2.0
    c, d = b - g * (b - a), a + g * (b - a)
    fc, fd = fn(c), fn(d)
    for _ in range(80):
        if b - a <= 1e-10:
            break
        if fc >= fd:
            b, d, fd = d, c, fc
            c = b - g * (b - a)
            fc = fn(c)
        else:
            a, c, fc = c, d, fd
            d = a + g * (b - a)
            fd = fn(d)
    for p, v in ((c, fc), (d, fd)):
        if v > best[1]:
            best = (p, v)
    return best


def m_step(stats, current: Dict[str, float], u: int, kappa_case: float = 2.0, fit: Sequence[str] = SETTINGS,
           rho: Callable = rho_case):
    """One M-step. stats: (table [2][2], trials, events), counts of drawn
    paths or their expectations (float64); current: the three settings now;
    fit: the subset to update. Returns (settings, record):

      split_prob           = n[1][0] / (n[1][0] + n[1][1])
      exp(merge_log_prob)  = n[0][1] / (n[0][0] + n[0][1])
      omega_case           = argmax over (0, 1) of q_omega, by a bracketed 1-D
                             search with the current value as a candidate, so
                             Q(new) >= Q(current) whatever the search does (a
                             generalised EM step)

    A setting without a trial, or whose update would leave the model's open
    interval (0 < split_prob < 1, merge_log_prob < 0, 0 < omega_case < 1, the
    search interval's ends counting as outside), keeps its value; record[name]
    = {"updated", "reason"} says why. record["q_before"], record["q_after"]: Q
    at omega_case before and after. rho(d, omega, kappa, u) is the hazard."""
    table, trials, events = stats
    table = np.asarray(table, dtype=np.float64).reshape(2, 2)
    trials, events = np.asarray(trials, dtype=np.float64), np.asarray(events, dtype=np.float64)
    unknown = [n for n in fit if n not in SETTINGS]
    if unknown:
        raise ValueError(f"unknown setting(s) to fit: {', '.join(unknown)}")
    new = {n: float(current[n]) for n in SETTINGS}
    record: Dict[str, object] = {n: {"updated": False, "reason": "not fitted"} for n in SETTINGS}

    def ratio(name, hit, miss, to_value):
        hit, miss = float(hit), float(miss)
        if not hit + miss > 0:
            record[name] = {"updated": False, "reason": "no trial"}
        elif not (hit > 0 and miss > 0 and 0.0 < hit / (hit + miss) < 1.0):
            record[name] = {"updated": False, "reason": f"{hit:g} of {hit + miss:g} trials: the update would leave "
                                                         "the open interval"}
        else:
            new[name] = to_value(hit / (hit + miss))
            record[name] = {"updated": True, "reason": ""}

    if "split_prob" in fit:
        ratio("split_prob", table[1, 0], table[1, 1], float)
    if "merge_log_prob" in fit:
        ratio("merge_log_prob", table[0, 1], table[0, 0], math.log)
    q = lambda w: q_omega(trials, events, w, kappa_case, u, rho)  # noqa: E731
    q_before = q(new["omega_case"])
    q_after = q_before
    if "omega_case" in fit:
        if not float(trials.sum()) > 0:
            record["omega_case"] = {"updated": False, "reason": "no trial"}
        else:
            w, qw = _maximise(q, _OMEGA_LO, _OMEGA_HI, new["omega_case"])
            if not qw > q_before:
                record["omega_case"] = {"updated": False, "reason": "no value of the search raises Q"}
            elif w <= _OMEGA_LO or w >= _OMEGA_HI:
                record["omega_case"] = {"updated": False, "reason": "Q is largest at an end of (0, 1): the update "
                                                                    "would leave the open interval"}
            else:
                new["omega_case"], q_after = float(w), qw
                record["omega_case"] = {"updated": True, "reason": ""}
    record["q_before"], record["q_after"] = q_before, q_after
    return new, record


# -------------------------------------------------------------- fit_genome
def fit_flags():
    from . import cli

    return cli.GENOME_FLAGS + [
        ("iterations", "int", 10, "EM iterations: each is one full launch of the tasks and one M-step"),
        ("fit", "string", ",".join(SETTINGS), "the settings to fit, a comma list of " + ", ".join(SETTINGS)),
        ("dcap", "int", 1024, "case durations of at least this many sites share the hazard histograms' last bin "
                              f"(1 to {MAX_DCAP})"),
    ]


TRACE_COLUMNS = ("iteration", "omega_case_in", "merge_log_prob_in", "split_prob_in", "omega_case_out",
                 "merge_log_prob_out", "split_prob_out", "n00", "n01", "n10", "n11", "trials", "events", "q_before",
                 "q_after", "sum_log_z")


def serialize_settings(settings: Dict[str, float]) -> str:
    """The three flags as `infer` writes them to its flags file (cli.serialize_flags)."""
    return "\n".join(f"--{n}={float(settings[n])}" for n in SETTINGS)


def _save_npz(path: str, arrays: Dict[str, np.ndarray]) -> None:
    """np.savez with a fixed member time stamp, so that a rerun writes the same bytes."""
    import zipfile

    with zipfile.ZipFile(path, "w", zipfile.ZIP_STORED) as z:
        for name, a in arrays.items():
            with z.open(zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), "w") as fh:
                np.lib.format.write_array(fh, np.ascontiguousarray(a), allow_pickle=False)


def genome_layout(groups, seeds):
    """infer_genome's launch layout of the groups (chrom, theta, tasks, meth_c,
    tot_c, meth_k, tot_k, positions): the count rows of the chromosomes one
    after another, a chain per (task, seed) in that order, and per chromosome
    the addressing of its trimmed rows for the statistics (hyg_dmp_group list
    and block rows, as get_change_points groups a chromosome's batches).
    Returns (counts {mc, tc, mk, tk}, chains, chain_model, out_rows, max_reads,
    max_len, per_chrom [(chrom, n_sites, groups, block_rows)])."""
    from . import cli

    parts = {k: [] for k in ("mc", "tc", "mk", "tk")}
    chains, chain_model, per_chrom, out, site0, max_reads, max_len = [], [], [], 0, 0, 0, []
    for g, (chrom, _, tasks, meth_c, tot_c, meth_k, tot_k, positions) in enumerate(groups):
        lo_all, hi_all = min(t[1] for t in tasks), max(t[2] for t in tasks)
        for k, a in (("mc", meth_c), ("tc", tot_c), ("mk", meth_k), ("tk", tot_k)):
            parts[k].append(a[lo_all:hi_all])
        max_reads = max(max_reads, int(max(tot_c[lo_all:hi_all].max(initial=0), tot_k[lo_all:hi_all].max(initial=0))))
        rows = []
        for (b, lo, hi, r0, r1) in tasks:
            begins = []
            for sd in seeds:
                chains.append((site0 + lo - lo_all, hi - lo, sd, cli.chain_id(chrom, b), out))
                chain_model.append(g)
                begins.append(out + r0)
                out += hi - lo
            if r1 > r0:  # the task's trimmed rows: one group, a seed block per seed
                rows.append(((lo + r0, r1 - r0), begins))
        rows.sort(key=lambda x: x[0][0])
        per_chrom.append((chrom, int(positions.shape[0]), [r[0] for r in rows], [r[1] for r in rows]))
        max_len.append(max(t[2] - t[1] for t in tasks))
        site0 += hi_all - lo_all
    counts = {k: v[0] if len(v) == 1 else np.concatenate(v) for k, v in parts.items()}
    return counts, chains, chain_model, out, max_reads, max_len, per_chrom


def main(argv: Sequence[str]) -> int:
    """`hygeia fit_genome`: --iterations Monte-Carlo EM steps over the tasks of
    `hygeia infer_genome`'s flags and inputs. An iteration builds the models at
    the current settings, runs every (chromosome, batch, seed) task in one full
    launch whose outputs stay on the device (two_group.DeviceChains), adds the
    transition statistics of every chromosome's trimmed rows and applies
    m_step. Writes to --results_dir: fit_trace.tsv (a row per iteration),
    fit_stats_{iteration}.npz (table, trials, events) and fitted_flags.txt (the
    three flags as `infer` takes them). The launches' randomness is their
    (seed, chain id) alone, so a rerun writes the same bytes."""
    from . import cli, two_group
    from .evidence import _write_tsv

    f = cli.parse_flags(argv, fit_flags())
    seeds = cli._seeds(f)
    fit = [x for x in str(f["fit"]).split(",") if x != ""]
    if any(x not in SETTINGS for x in fit) or not fit:
        raise cli.FlagError(f"--fit takes a comma list of {', '.join(SETTINGS)}: {f['fit']!r}")
    dcap, iterations = int(f["dcap"]), int(f["iterations"])
    if not 1 <= dcap <= MAX_DCAP:
        raise cli.FlagError(f"--dcap must lie in [1, {MAX_DCAP}]")
    if iterations < 1:
        raise cli.FlagError("--iterations must be >= 1")
    if len(f["num_resampled_particles"]) != 1:
        raise cli.FlagError("fit_genome takes one --num_resampled_particles value")
    if not seeds:
        raise cli.FlagError("--seeds is empty")
    M, u = int(f["num_resampled_particles"][0]), int(f["minimum_duration"])
    current = {n: float(f[n]) for n in SETTINGS}
    if not (0.0 < current["omega_case"] < 1.0 and current["merge_log_prob"] < 0.0 and
            0.0 < current["split_prob"] < 1.0):
        raise cli.FlagError("the starting settings must lie inside the model's open intervals: 0 < omega_case < 1, "
                            "merge_log_prob < 0, 0 < split_prob < 1")
    groups = cli._genome_groups(f)  # every chromosome read and checked before anything is written
    if not groups:
        return 0
    from .dmp import _torch

    torch = _torch()
    cli._use_task_device(_lib.load())
    dev = torch.device("cuda", torch.cuda.current_device())
    mu, sigma, _ = cli._regimes(f)
    counts, chains, chain_model, out_rows, max_reads, max_len, per_chrom = genome_layout(groups, seeds)
    # (uint16 counts as int16 tensors: the same bits, the dtype torch can hold)
    mc, tc, mk, tk = (torch.from_numpy(a.view(np.int16)).to(dev) for a in
                      two_group._counts(counts["mc"], counts["tc"], counts["mk"], counts["tk"]))
    B = int(f["num_samples_backward"])
    out_dir = str(f["results_dir"])
    os.makedirs(out_dir, exist_ok=True)
    trace, E, workspace = [], None, None
    for it in range(1, iterations + 1):
        models = two_group.genome_models([g[1] for g in groups], mu, sigma, max_reads, [n + 1 for n in max_len],
                                         **cli._model_kw(dict(f, **current), M))
        try:
            dc = two_group.DeviceChains(models, chains, out_rows, device=dev, workspace=workspace,
                                        chain_model=chain_model)
            workspace = dc.ws  # the settings do not change a launch's shape: one history buffer serves every iteration
            E = dc.emission(mc, tc, mk, tk, E=E)
            dc.run(E)
            torch.cuda.synchronize(dev)
            status = dc.status.cpu().numpy()
            if (status != 0).any():
                raise _lib.HygError(int(status[status != 0][0]), f"fit_genome: chains failed in iteration {it}")
            stats = torch.zeros(stats_len(dcap), dtype=torch.int64, device=dev)
            for (_, n_sites, grp, block_rows) in per_chrom:
                if grp:
                    transition_stats(dc.merged, dc.control, dc.case, B, grp, block_rows, n_sites, u, dcap, stats=stats)
            sum_log_z = math.fsum(dc.log_z.cpu().numpy().tolist())
        finally:
            for model in models:
                model.close()
        st = split_stats(stats.cpu().numpy(), dcap)
        new, rec = m_step(st, current, u, 2.0, fit)  # (kappa_case: CaseControlModel's default, which no flag sets)
        table, trials, events = st
        trace.append((it,) + tuple(current[n] for n in SETTINGS) + tuple(new[n] for n in SETTINGS) +
                     tuple(int(v) for v in table.reshape(-1)) + (int(trials.sum()), int(events.sum()),
                                                                 float(rec["q_before"]), float(rec["q_after"]),
                                                                 float(sum_log_z)))
        _save_npz(os.path.join(out_dir, f"fit_stats_{it}.npz"), {"table": table, "trials": trials, "events": events})
        for n in SETTINGS:
            if n in fit and not rec[n]["updated"]:
                print(f"hygeia fit_genome: iteration {it}: {n} keeps {current[n]!r} ({rec[n]['reason']})")
        current = new
    _write_tsv(os.path.join(out_dir, "fit_trace.tsv"), TRACE_COLUMNS, trace)
    with open(os.path.join(out_dir, "fitted_flags.txt"), "w") as fh:
        fh.write(serialize_settings(current))
    return 0
