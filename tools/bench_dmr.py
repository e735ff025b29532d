"""Measurement of the region (DMR) pass on MI355X (hyg_dmr_*, hygeia_amd/dmr.py).

Workload: one chromosome of chr1's size -- 2 424 617 CpG sites in 100k-site
segments, 10 seed blocks x B = 25 trajectories per site (P = 250), K = 6 --
with sticky synthetic int16 trajectories made on the device in the
hyg_tg_outputs layout (a shared truth track of differential stretches; each
trajectory keeps its indicator with probability 0.95 per site, else follows
the truth with probability 0.6 or a coin), positions with CpG-like gaps, and
`hygeia get_dmrs`' flag defaults (site_prob 0.5, gap 300 bp, 3 sites, 4/5).

Timed with device events, one warm-up then `--reps` rounds, median and spread:
hyg_dmp_site_counts (the existing kernel that reads the same arrays: the
yardstick), find_regions, region_counts, region_sums. Each with the bytes it
reads and its share of the HBM peak. A sample of the regions is checked
against torch reductions of the same trajectories.

Prints one JSON line; `--out` also writes it to a file (profiles/dmr_bench.json).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
from fractions import Fraction

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0
GAPS = np.array([2, 10, 40, 200, 900], dtype=np.int64)
GAP_PROBS = np.array([.3, .3, .2, .15, .05])


def truth_track(T: int, rng) -> np.ndarray:
    """Differential stretches of geometric lengths (p = 0.08), each on with probability 0.45."""
    n = int(T * 0.08 * 1.5) + 64
    while True:
        lens = rng.geometric(0.08, n)
        if lens.sum() >= T:
            break
        n *= 2
    return np.repeat(rng.random(n) < 0.45, lens)[:T]


def sticky_block(truth, B: int, K: int, gen, dev):
    """One seed block: (control, case) [T][B][2] int16 (d, r)."""
    import torch

    T = truth.shape[0]
    renew = torch.rand((T, B), device=dev, generator=gen) >= 0.95
    renew[0] = True
    follow = torch.rand((T, B), device=dev, generator=gen) < 0.6
    coin = torch.rand((T, B), device=dev, generator=gen) < 0.5
    fresh = torch.where(follow, truth[:, None], coin)
    last = torch.where(renew, torch.arange(T, device=dev)[:, None], 0).cummax(dim=0).values  # last renewal <= t
    D = torch.gather(fresh, 0, last)
    control = torch.randint(0, K, (T, B, 2), dtype=torch.int16, device=dev, generator=gen)
    case = control.clone()
    shift = torch.randint(1, K, (T, B), dtype=torch.int16, device=dev, generator=gen)
    case[..., 1] = torch.where(D, (control[..., 1] + shift) % K, control[..., 1])
    case[..., 0] = torch.randint(0, 9, (T, B), dtype=torch.int16, device=dev, generator=gen)  # durations differ freely
    return control, case


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sites", type=int, default=2_424_617)
    ap.add_argument("--B", type=int, default=25)
    ap.add_argument("--seeds", type=int, default=10)
    ap.add_argument("--K", type=int, default=6)
    ap.add_argument("--segment", type=int, default=100_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--site_prob", type=float, default=0.5)
    ap.add_argument("--max_gap_bp", type=int, default=300)
    ap.add_argument("--min_sites", type=int, default=3)
    ap.add_argument("--min_fraction", default="0.8")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    from hygeia_amd import build, dmp, dmr

    if not torch.cuda.is_available():
        raise SystemExit("bench_dmr.py needs a HIP device")
    dev = torch.device("cuda", 0)
    T, B, S, K = a.sites, a.B, a.seeds, a.K
    P = B * S
    rng = np.random.default_rng(7)
    truth = torch.from_numpy(truth_track(T, rng)).to(dev)
    pos = torch.from_numpy(10_000 + np.cumsum(rng.choice(GAPS, size=T, p=GAP_PROBS))).to(dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    control = torch.empty((S * T, B, 2), dtype=torch.int16, device=dev)
    kase = torch.empty_like(control)
    for s in range(S):  # seed-major blocks, a segment's rows contiguous inside each
        control[s * T:(s + 1) * T], kase[s * T:(s + 1) * T] = sticky_block(truth, B, K, gen, dev)
    merged = torch.ones((S * T, B), dtype=torch.int16, device=dev)
    groups = [(g0, min(a.segment, T - g0)) for g0 in range(0, T, a.segment)]
    block_rows = [[s * T + g0 for s in range(S)] for g0, _ in groups]
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream(dev)
    fraction = dmr.parse_min_fraction(a.min_fraction)
    min_count = dmr.min_count_of(a.site_prob, P)

    counts = torch.zeros((T, 2 + 2 * K), dtype=torch.int32, device=dev)
    _, t_sc = timed(lambda: dmp.site_counts(merged, control, kase, B, K, groups, block_rows, T, counts=counts),
                    a.reps, stream)
    regions, t_fr = timed(lambda: dmr.find_regions(counts, 1, min_count, pos, a.max_gap_bp, a.min_sites), a.reps,
                          stream)
    regions = regions.contiguous()
    rc, t_rc = timed(lambda: dmr.region_counts(control, kase, B, groups, block_rows, T, regions, fraction), a.reps,
                     stream)
    sums, t_rs = timed(lambda: dmr.region_sums(counts, regions), a.reps, stream)

    n_regions = int(regions.shape[0])
    lens = (regions[:, 1] - regions[:, 0])
    total_len = int(lens.sum().item())
    # bytes each pass needs: the trajectories it reads (one int16 of merged, a (d, r) pair of each group per
    # trajectory and site) and the rows it reads or writes of the count matrix
    row = (2 + 2 * K) * 4
    nbytes = {
        "site_counts": T * P * (2 + 4 + 4) + T * row,
        "find_regions": 2 * (T * (4 + 8)) + 4 * n_regions * 16,  # two passes over a count column and the positions
        "region_counts": total_len * P * (4 + 4) + n_regions * (16 + 8),
        "region_sums": total_len * row + n_regions * (16 + 2 * row),
    }
    for name, t in (("site_counts", t_sc), ("find_regions", t_fr), ("region_counts", t_rc), ("region_sums", t_rs)):
        t["bytes"] = int(nbytes[name])
        t["GB_per_s"] = nbytes[name] / (t["median_ms"] / 1000.0) / 1e9
        t["frac_of_hbm_peak"] = t["GB_per_s"] / HBM_PEAK_GBS

    # parity on a sample of the regions: torch reductions of the same trajectories
    sample = torch.linspace(0, n_regions - 1, min(n_regions, 300), device=dev).long().unique()
    ok = True
    c4 = control.view(S, T, B, 2)[..., 1]
    k4 = kase.view(S, T, B, 2)[..., 1]
    for i in sample.tolist():
        r0, r1 = int(regions[i, 0]), int(regions[i, 1])
        sp = (c4[:, r0:r1] != k4[:, r0:r1]).sum(dim=1).reshape(-1).long()  # [S * B]
        n = r1 - r0
        exp = (int((sp == n).sum()), int((sp * fraction.denominator >= fraction.numerator * n).sum()))
        ok &= exp == (int(rc[i, 0]), int(rc[i, 1]))
        ok &= bool(torch.equal(sums[i], counts[r0:r1].long().sum(dim=0)))
    # the pathological input (min_count = 0): the whole chromosome as one region, walked by one workgroup
    whole = torch.tensor([[0, T]], dtype=torch.int64, device=dev)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record(stream)
    rc_whole = dmr.region_counts(control, kase, B, groups, block_rows, T, whole, fraction)
    ev[1].record(stream)
    torch.cuda.synchronize()
    whole_ms = ev[0].elapsed_time(ev[1])
    ok &= int(rc_whole[0, 0]) == 0  # no sticky trajectory is differential at every site
    rc_h = rc.cpu().numpy()
    line = {
        "metric": "region (DMR) pass on one chromosome: event times per kernel",
        "data": "synthetic (sticky trajectories)", "n_gpus": 1,
        "config": {"sites": T, "B": B, "seeds": S, "P": P, "K": K, "segments": len(groups),
                   "site_prob": a.site_prob, "min_count": min_count, "max_gap_bp": a.max_gap_bp,
                   "min_sites": a.min_sites, "min_fraction": str(Fraction(fraction)), "reps": a.reps},
        "regions": {"n": n_regions, "total_sites": total_len, "longest": int(lens.max().item()) if n_regions else 0,
                    "frac_of_sites": total_len / T,
                    "frac_with_0_lt_n_all_lt_P": float(((rc_h[:, 0] > 0) & (rc_h[:, 0] < P)).mean()) if n_regions else 0.,
                    "frac_n_all_ne_n_frac": float((rc_h[:, 0] != rc_h[:, 1]).mean()) if n_regions else 0.},
        "kernels": {"dmp_site_counts": t_sc, "find_regions": t_fr, "region_counts": t_rc, "region_sums": t_rs},
        "region_counts_vs_site_counts_bytes_per_s": t_rc["GB_per_s"] / t_sc["GB_per_s"],
        "whole_chromosome_region": {"ms": whole_ms, "bytes": T * P * 8, "GB_per_s": T * P * 8 / (whole_ms / 1000.0) / 1e9,
                                    "n_all": int(rc_whole[0, 0]), "n_frac": int(rc_whole[0, 1])},
        "hbm_peak_GB_per_s": HBM_PEAK_GBS,
        "parity_sample": {"regions": int(sample.numel()), "ok": bool(ok)},
        "source_hash": build.source_hash(),
    }
    print(json.dumps(line), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(json.dumps(line, indent=1) + "\n")
    if not ok:
        raise SystemExit("bench_dmr.py: the sampled regions differ from the torch reductions")


if __name__ == "__main__":
    main()
