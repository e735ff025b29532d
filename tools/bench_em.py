"""Measurement of the transition-statistics pass on MI355X (hyg_tg_transition_stats,
hygeia_amd/em.py).

Workload: tools/bench_cp.py's -- one chromosome of chr1's size, 2 424 617 CpG
sites in 100k-site groups, 10 seed blocks x B = 25 trajectories per site (P =
250), sticky synthetic int16 paths made on the device in the hyg_tg_outputs
layout -- with `hygeia fit_genome`'s defaults (minimum_duration 3, dcap 1024).

Timed with device events, one warm-up then `--reps` rounds, median and spread:
transition_stats against cp_site_events_kernel (hyg_cp_site_events, the
yardstick: it streams the same (d, r) words and merged once and adds to LDS
only at events) over the same arrays in the same run, the two alternating.
Each with the bytes it needs and its share of the HBM peak. The 2 x 2 table and
the histograms' totals are checked against torch reductions of the same words.

Prints one JSON line; `--out` also writes it to a file (profiles/em_bench.json).
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_cp import HBM_PEAK_GBS, placed, rate, sticky_states, timed, truth_sites  # noqa: E402


def torch_stats(merged, control, kase, S, T, B, first, u, dcap):
    """(table [4], trials total, events total, pooled last bin) by torch reductions over [S][T][B]."""
    import torch

    m = (merged.view(S, T, B) != 0)
    c, k = control.view(torch.int32).view(S, T, B), kase.view(torch.int32).view(S, T, B)
    live = torch.ones(T, dtype=torch.bool, device=merged.device)
    live[first] = False
    live = live[None, 1:, None]
    mx, my = m[:, :-1], m[:, 1:]
    dcx, dkx = c[:, :-1] & 0xffff, k[:, :-1] & 0xffff
    free = live & (torch.minimum(dcx, dkx) >= u)
    table = [int((free & (mx == a) & (my == b)).sum()) for a in (False, True) for b in (False, True)]
    del free
    trial = live & ~my & ~(mx & ((c[:, 1:] & 0xffff) != 1)) & ~(~mx & ((c[:, 1:] >> 16) == (k[:, :-1] >> 16)))
    n_trials = int(trial.sum())
    n_events = int((trial & ((k[:, 1:] & 0xffff) == 1)).sum())
    pooled = int((trial & (dkx >= dcap)).sum())
    return table, n_trials, n_events, pooled


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sites", type=int, default=2_424_617)
    ap.add_argument("--B", type=int, default=25)
    ap.add_argument("--seeds", type=int, default=10)
    ap.add_argument("--K", type=int, default=6)
    ap.add_argument("--segment", type=int, default=100_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--minimum_duration", type=int, default=3)
    ap.add_argument("--dcap", type=int, default=1024)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    from hygeia_amd import build, changepoints as cp, em

    if not torch.cuda.is_available():
        raise SystemExit("bench_em.py needs a HIP device")
    dev = torch.device("cuda", 0)
    T, B, S, K = a.sites, a.B, a.seeds, a.K
    P = B * S
    rng = np.random.default_rng(7)
    truth = [torch.from_numpy(truth_sites(T, rng)).to(dev) for _ in range(3)]  # control, case, merged
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    control = torch.empty((S * T, B, 2), dtype=torch.int16, device=dev)
    kase = torch.empty_like(control)
    merged = torch.empty((S * T, B), dtype=torch.int16, device=dev)
    for s in range(S):  # seed-major blocks, a group's rows contiguous inside each
        control[s * T:(s + 1) * T] = sticky_states(placed(truth[0], T, B, gen, dev), K, gen, dev)
        kase[s * T:(s + 1) * T] = sticky_states(placed(truth[1], T, B, gen, dev), K, gen, dev)
        merged[s * T:(s + 1) * T] = (1 - torch.cumsum(placed(truth[2], T, B, gen, dev), dim=0) % 2).to(torch.int16)
    groups = [(g0, min(a.segment, T - g0)) for g0 in range(0, T, a.segment)]
    block_rows = [[s * T + g0 for s in range(S)] for g0, _ in groups]
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream(dev)

    events = torch.zeros((T, cp.N_KINDS), dtype=torch.int32, device=dev)
    stats = torch.zeros(em.stats_len(a.dcap), dtype=torch.int64, device=dev)

    def run_stats():
        stats.zero_()
        return em.transition_stats(merged, control, kase, B, groups, block_rows, T, a.minimum_duration, a.dcap,
                                   stats=stats)

    def run_events():
        return cp.site_events(merged, control, kase, B, groups, block_rows, T, events=events)

    # the two alternate, twice over; timed() warms up, then takes `reps` rounds
    rounds = {"site_events": [], "transition_stats": []}
    got = None
    for _ in range(2):
        _, t = timed(run_events, a.reps, stream)
        rounds["site_events"].append(t)
        got, t = timed(run_stats, a.reps, stream)
        rounds["transition_stats"].append(t)
    nbytes = T * P * (2 + 4 + 4)
    # the headline is the second round's median of `reps`; the first round's shows the spread
    t_se = rate(dict(rounds["site_events"][-1]), nbytes + T * cp.N_KINDS * 4)
    t_ts = rate(dict(rounds["transition_stats"][-1]), nbytes + em.stats_len(a.dcap) * 8)

    table, trials, ev = got
    first = torch.tensor([g0 for g0, _ in groups], device=dev)
    want = torch_stats(merged, control, kase, S, T, B, first, a.minimum_duration, a.dcap)
    ok = (table.reshape(-1).tolist() == want[0] and int(trials.sum()) == want[1] and int(ev.sum()) == want[2]
          and int(trials[a.dcap]) == want[3])
    line = {
        "metric": "transition statistics of one chromosome: event times per kernel",
        "data": "synthetic (sticky paths)", "n_gpus": 1,
        "config": {"sites": T, "B": B, "seeds": S, "P": P, "K": K, "groups": len(groups),
                   "minimum_duration": a.minimum_duration, "dcap": a.dcap, "reps": a.reps},
        "kernels": {"site_events": t_se, "transition_stats": t_ts},
        "rounds_median_ms": {k: [t["median_ms"] for t in v] for k, v in rounds.items()},
        "transition_stats_over_site_events_time": t_ts["median_ms"] / t_se["median_ms"],
        "target": "transition_stats_over_site_events_time <= 2",
        "counts": {"table": table.reshape(-1).tolist(), "trials": int(trials.sum()), "events": int(ev.sum()),
                   "pooled_last_bin": int(trials[a.dcap]), "nonzero_trial_bins": int(np.count_nonzero(trials)),
                   "transitions": (T - len(groups)) * P},
        "hbm_peak_GB_per_s": HBM_PEAK_GBS,
        "parity": {"table_and_totals": "all sites, torch reductions", "ok": bool(ok)},
        "source_hash": build.source_hash(),
    }
    print(json.dumps(line), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(json.dumps(line, indent=1) + "\n")
    if not ok:
        raise SystemExit("bench_em.py: the table or the totals differ from the torch reductions")


if __name__ == "__main__":
    main()
