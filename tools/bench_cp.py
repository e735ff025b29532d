"""Measurement of the change-point pass on MI355X (hyg_cp_*, hygeia_amd/changepoints.py).

Workload: one chromosome of chr1's size -- 2 424 617 CpG sites in 100k-site
groups, 10 seed blocks x B = 25 trajectories per site (P = 250), K = 6 -- with
sticky synthetic int16 paths made on the device in the hyg_tg_outputs layout
(per group kind a shared truth set of change sites about 48 sites apart; each
trajectory places a truth change with probability 0.9 at the truth site +
U{-3..3} and changes of its own with probability 0.002 per site; durations
count up from an event, regimes change at events; merged splits and merges at
its own truth sites), positions with CpG-like gaps, and `hygeia
get_change_points`' flag defaults (site_prob 0.05, gap 300 bp, level 9/10).

Timed with device events, one warm-up then `--reps` rounds, median and spread:
site_events against hyg_dmp_site_counts (the existing kernel that reads the
same arrays), and per kind find_windows, window_counts and window_intervals,
window_counts of the control windows against hyg_dmr_region_counts over the
same windows. Each with the bytes it needs and its share of the HBM peak. The
control column of the event matrix and a sample of the windows are checked
against torch reductions of the same trajectories.

Prints one JSON line; `--out` also writes it to a file (profiles/cp_bench.json).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0
GAPS = np.array([2, 10, 40, 200, 900], dtype=np.int64)
GAP_PROBS = np.array([.3, .3, .2, .15, .05])


def truth_sites(T: int, rng, mean: float = 40.0) -> np.ndarray:
    """Ascending sites at least 8 apart with geometric spacing."""
    n = int(T / (8 + mean) * 1.5) + 64
    while True:
        at = 12 + np.cumsum(8 + rng.geometric(1.0 / mean, n))
        if at[-1] >= T:
            return at[at < T - 4]
        n *= 2


def placed(truth, T: int, B: int, gen, dev):
    """[T][B] bool: the changes of B trajectories around the truth sites."""
    import torch

    ev = torch.rand((T, B), device=dev, generator=gen) < 0.002
    n = truth.shape[0]
    take = torch.rand((n, B), device=dev, generator=gen) < 0.9
    at = (truth[:, None] + torch.randint(-3, 4, (n, B), device=dev, generator=gen)).clamp_(1, T - 1)
    col = torch.arange(B, device=dev)[None, :].expand(n, B)
    ev[at[take], col[take]] = True
    ev[0] = False
    return ev


def sticky_states(ev, K: int, gen, dev):
    """(d, r) [T][B][2] int16 of the change indicators ev: d counts up from a change, r changes at it."""
    import torch

    T, B = ev.shape
    t = torch.arange(T, device=dev)[:, None]
    last = torch.where(ev, t, 0).cummax(dim=0).values
    d0 = torch.randint(0, 500, (B,), device=dev, generator=gen)
    d = t - last + torch.where(last == 0, d0[None, :], 0)
    shift = torch.randint(1, K, (T, B), device=dev, generator=gen)
    r = (torch.randint(0, K, (B,), device=dev, generator=gen)[None, :] + torch.cumsum(ev * shift, dim=0)) % K
    return torch.stack([d, r], dim=-1).to(torch.int16)


def timed(fn, reps: int, stream):
    import torch

    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    out = fn()  # warm-up
    torch.cuda.synchronize()
    ms, wall = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        ev[0].record(stream)
        out = fn()
        ev[1].record(stream)
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1000.0)  # the call as its caller sees it (allocations, copies, waits)
        ms.append(ev[0].elapsed_time(ev[1]))
    return out, {"median_ms": float(np.median(ms)), "min_ms": min(ms), "max_ms": max(ms),
                 "wall_median_ms": float(np.median(wall))}


def rate(t: dict, nbytes: int) -> dict:
    t["bytes"] = int(nbytes)
    t["GB_per_s"] = nbytes / (t["median_ms"] / 1000.0) / 1e9
    t["frac_of_hbm_peak"] = t["GB_per_s"] / HBM_PEAK_GBS
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sites", type=int, default=2_424_617)
    ap.add_argument("--B", type=int, default=25)
    ap.add_argument("--seeds", type=int, default=10)
    ap.add_argument("--K", type=int, default=6)
    ap.add_argument("--segment", type=int, default=100_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--site_prob", type=float, default=0.05)
    ap.add_argument("--max_gap_bp", type=int, default=300)
    ap.add_argument("--level", default="0.9")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    from hygeia_amd import build, changepoints as cp, dmp, dmr

    if not torch.cuda.is_available():
        raise SystemExit("bench_cp.py needs a HIP device")
    dev = torch.device("cuda", 0)
    T, B, S, K = a.sites, a.B, a.seeds, a.K
    P = B * S
    rng = np.random.default_rng(7)
    truth = [torch.from_numpy(truth_sites(T, rng)).to(dev) for _ in range(3)]  # control, case, merged
    pos = torch.from_numpy(10_000 + np.cumsum(rng.choice(GAPS, size=T, p=GAP_PROBS))).to(dev)
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
    level = cp.parse_level(a.level)
    min_count = dmr.min_count_of(a.site_prob, P)

    counts = torch.zeros((T, 2 + 2 * K), dtype=torch.int32, device=dev)
    _, t_sc = timed(lambda: dmp.site_counts(merged, control, kase, B, K, groups, block_rows, T, counts=counts),
                    a.reps, stream)
    events = torch.zeros((T, cp.N_KINDS), dtype=torch.int32, device=dev)
    _, t_se = timed(lambda: cp.site_events(merged, control, kase, B, groups, block_rows, T, events=events), a.reps,
                    stream)
    rate(t_sc, T * P * (2 + 4 + 4) + T * (2 + 2 * K) * 4)
    rate(t_se, T * P * (2 + 4 + 4) + T * cp.N_KINDS * 4)

    # parity: the control column against a torch reduction of the same words
    first = torch.zeros(T, dtype=torch.bool, device=dev)
    first[torch.tensor([g0 for g0, _ in groups], device=dev)] = True
    w32 = control.view(torch.int32).view(S, T, B)
    cont = (w32[:, :-1] & -65536) | ((w32[:, :-1] + 1) & 0xffff)
    E0 = torch.zeros((S, T, B), dtype=torch.bool, device=dev)
    E0[:, 1:] = w32[:, 1:] != cont
    E0[:, first] = False
    ok = bool(torch.equal(E0.sum(dim=(0, 2)).to(torch.int32), events[:, 0]))
    del cont

    kinds = {}
    for name, kind in cp.OUTPUT_KINDS:
        w, t_fw = timed(lambda: cp.find_windows(events, kind, min_count, pos, a.max_gap_bp), a.reps, stream)
        w = w.contiguous()
        wc, t_wc = timed(lambda: cp.window_counts(merged, control, kase, B, groups, block_rows, T, kind, w), a.reps,
                         stream)
        wi, t_wi = timed(lambda: cp.window_intervals(events, kind, w, level), a.reps, stream)
        n_w = int(w.shape[0])
        lens = w[:, 1] - w[:, 0]
        total = int(lens.sum().item())
        per = 4 if kind < 3 else 2  # one (d, r) word of one group, or one int16 of merged, per trajectory and row
        # distinct bytes: the window's rows and the row before its first
        rate(t_wc, (total + n_w) * P * per + n_w * (16 + 8))
        rate(t_wi, 2 * total * 4 + n_w * (16 + 32))
        rate(t_fw, 2 * (T * (4 + 8)) + 4 * n_w * 16)
        wc_h, wi_h, lens_h = wc.cpu().numpy(), wi.cpu().numpy(), lens.cpu().numpy()
        kinds[name] = {
            "windows": {"n": n_w, "total_sites": total, "frac_of_sites": total / T,
                        "length_quantiles_50_90_99_max": [int(x) for x in np.quantile(lens_h, [.5, .9, .99, 1.])]
                        if n_w else [],
                        "frac_with_0_lt_n_any_lt_P": float(((wc_h[:, 0] > 0) & (wc_h[:, 0] < P)).mean()) if n_w else 0.,
                        "frac_n_one_ne_n_any": float((wc_h[:, 0] != wc_h[:, 1]).mean()) if n_w else 0.,
                        "frac_lo_lt_hi": float((wi_h[:, 2] < wi_h[:, 3]).mean()) if n_w else 0.},
            "find_windows": t_fw, "window_counts": t_wc, "window_intervals": t_wi}
        if kind == 0:  # the yardstick over the same windows, and a sample of them against torch
            _, t_rc = timed(lambda: dmr.region_counts(control, kase, B, groups, block_rows, T, w, (4, 5)), a.reps,
                            stream)
            rate(t_rc, total * P * (4 + 4) + n_w * (16 + 8))
            kinds[name]["dmr_region_counts_same_windows"] = t_rc
            kinds[name]["window_counts_over_region_counts_time"] = t_wc["median_ms"] / t_rc["median_ms"]
            for i in torch.linspace(0, n_w - 1, min(n_w, 300), device=dev).long().unique().tolist():
                r0, r1 = int(w[i, 0]), int(w[i, 1])
                sp = E0[:, r0:r1].sum(dim=1).reshape(-1)
                ok &= (int((sp >= 1).sum()), int((sp == 1).sum())) == (int(wc[i, 0]), int(wc[i, 1]))
                ok &= int(wi[i, 0]) == int(events[r0:r1, 0].sum()) and r0 <= int(wi[i, 2]) <= int(wi[i, 3]) < r1
    # the pathological input: the whole chromosome as one window, walked by one workgroup
    whole = torch.tensor([[0, T]], dtype=torch.int64, device=dev)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    ev[0].record(stream)
    wc_whole = cp.window_counts(merged, control, kase, B, groups, block_rows, T, 0, whole)
    ev[1].record(stream)
    wi_whole = cp.window_intervals(events, 0, whole, level)
    ev[2].record(stream)
    torch.cuda.synchronize()
    ok &= int(wc_whole[0, 0]) == P and int(wi_whole[0, 0]) == int(events[:, 0].sum())
    whole_ms = ev[0].elapsed_time(ev[1])
    line = {
        "metric": "change-point pass on one chromosome: event times per kernel",
        "data": "synthetic (sticky paths)", "n_gpus": 1,
        "config": {"sites": T, "B": B, "seeds": S, "P": P, "K": K, "groups": len(groups), "site_prob": a.site_prob,
                   "min_count": min_count, "max_gap_bp": a.max_gap_bp, "level": str(level), "reps": a.reps},
        "kernels": {"dmp_site_counts": t_sc, "site_events": t_se},
        "site_events_over_site_counts_time": t_se["median_ms"] / t_sc["median_ms"],
        "kinds": kinds,
        "whole_chromosome_window": {"window_counts_ms": whole_ms, "bytes": T * P * 4,
                                    "GB_per_s": T * P * 4 / (whole_ms / 1000.0) / 1e9,
                                    "window_intervals_ms": ev[1].elapsed_time(ev[2]),
                                    "n_any": int(wc_whole[0, 0]), "n_one": int(wc_whole[0, 1]),
                                    "n_events": int(wi_whole[0, 0])},
        "hbm_peak_GB_per_s": HBM_PEAK_GBS,
        "parity": {"control_column": "all sites", "windows_sampled": 300, "ok": bool(ok)},
        "source_hash": build.source_hash(),
    }
    print(json.dumps(line), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(json.dumps(line, indent=1) + "\n")
    if not ok:
        raise SystemExit("bench_cp.py: the event column or the sampled windows differ from the torch reductions")


if __name__ == "__main__":
    main()
